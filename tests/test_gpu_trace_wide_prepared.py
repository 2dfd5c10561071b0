"""vd_trace_prepare_wide_dev (a prepared VdTraceSceneWide, with VD_OPT_TRACE_TIGHT_TLAS a private wide LBVH over tight boxes) and
vd_trace_accel_refit_dev (the private top level of any accel - narrow agglomerative, narrow LBVH, wide - follows the instances without
a rebuild).

The oracle walks narrow nodes only: scenes of up to 32 768 instances are built narrow for it and handed to the GPU through widen()
and relocate() (200 000 slots: indices pass 16 bits).  Option off, the prepared walk is the exact one - records equal the oracle's
bit for bit.  Tight, the acceptance is test_gpu_trace_tight.py's (`tight_rule`): hit flags and any-hit flags equal, distances within
1e-5 absolute, and - asked here on top - bit-equal for every hit; instance and triangle agree on more than 99.9 % of those."""
import numpy as np
import pytest

from chain_scenes import chain_mixed_scene, chain_rays, chain_scene
from conftest import golden
from voidin_amd import abi, synth
from voidin_amd.runtime import VoidinError
from wide_scenes import disjoint_instances, first_bad, grid_rays, mesh_set, records_equal, relocate, widen

pytestmark = pytest.mark.gpu

ABS_TOL = 1e-5          # the project's: "traversal hit distances match within 1e-5" - absolute


def prepare(ctx, ctx_options, scene_arrays, tight):
    """(accel, DeviceScene) of scene_arrays - wide when its nodes are TLAS_NODE_WIDE - prepared with trace.tight_tlas = tight."""
    ds = ctx.device_scene(scene_arrays)
    ctx_options("trace.tight_tlas", tight)
    acc = ctx.trace_prepare(ds)
    ctx_options("trace.tight_tlas", 0)              # the option acts when the scene is prepared, not when it is traced
    return acc, ds


def run(ctx, acc, rays):
    """(records, flags) of vd_trace_prepared_dev and vd_trace_any_prepared_dev."""
    import torch
    n = len(rays)
    d_rays, d_hits = ctx.upload(rays), ctx.empty(n * 16)
    d_hits.fill_(0xEE)
    d_any = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.trace_prepared_dev(acc, d_rays, n, d_hits)
    ctx.trace_any_prepared_dev(acc, d_rays, n, d_any)
    torch.cuda.synchronize()
    return d_hits.cpu().numpy()[: n * 16].view(abi.HIT).copy(), d_any.cpu().numpy().astype(np.uint32)


def tight_rule(got, flags, want, min_hits=1):
    """The acceptance of a tight top level against the exact walk's records `want`; returns the number of hits."""
    hit = want["hit"] == 1
    assert np.array_equal(got["hit"], want["hit"]), f"{int((got['hit'] != want['hit']).sum())} hit flags differ"
    assert np.array_equal(flags, want["hit"]), f"{int((flags != want['hit']).sum())} any-hit flags differ"
    assert hit.sum() >= min_hits, int(hit.sum())
    err = np.abs(got["dist"][hit].astype(np.float64) - want["dist"][hit])
    assert np.all(err <= ABS_TOL), float(err.max())
    same = got["dist"][hit].view(np.uint32) == want["dist"][hit].view(np.uint32)
    assert same.all(), f"{int((~same).sum())} of {int(hit.sum())} hit distances are not bit-equal"
    agree = (got["instance"][hit] == want["instance"][hit]) & (got["triangle"][hit] == want["triangle"][hit])
    assert not same.any() or agree[same].mean() > 0.999, float(agree[same].mean())
    return int(hit.sum())


def wide_form(scene, seed):
    """The narrow scene with its top level widened and relocated."""
    wide, _ = relocate(widen(scene[0]), seed=seed)
    return (wide,) + tuple(scene[1:])


@pytest.fixture(scope="module")
def parity_scenes(oracle):
    """test_gpu_trace_wide.py's: the golden 40-instance scene with its own rays, 300 instances of three meshes under 128 x 128 rays."""
    g = golden("trace_40.npz")
    s40 = (g["tlas"], g["instances"], g["meshes"], g["bvh_nodes"], g["vertices"], g["indices"])
    infos, B, V, I = mesh_set(oracle, [synth.uv_sphere(1.0, 4), synth.knot_mesh(96, 24), synth.triangle_soup(64)])
    inst = synth.instances(300, n_mesh=3, seed=synth.SEED_BASE + 18, extent=50.0, scale_range=(0.5, 3.0))
    s300 = (oracle.tlas_build(inst, infos), inst, infos, B, V, I)
    r300 = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 40), pitch_deg=0), 128, 128)
    out = {}
    for name, scene, rays in (("trace_40", s40, np.ascontiguousarray(g["rays"], dtype=abi.RAY)), ("synth_300", s300, r300)):
        want, _ = oracle.trace(scene, rays, threads=8)
        assert 0 < want["hit"].sum() < len(rays)
        out[name] = (scene, rays, want)
    return out


@pytest.fixture(scope="module")
def tight_scenes(oracle):
    """test_gpu_trace_tight.py's two: A = 400 overlapping instances of one knot (the stress scene in small) under 192 x 192 rays,
    B = 500 instances of three meshes under 256 x 256 rays.  name -> (narrow scene, rays, the oracle's records)."""
    infos, B, V, I = mesh_set(oracle, [synth.knot_mesh(128, 32)])
    inst = synth.instances(400, n_mesh=1, seed=synth.SEED_BASE + 8, extent=120.0, scale_range=(0.5, 2.0))
    a = (oracle.tlas_build(inst, infos), inst, infos, B, V, I)
    ra = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 90), pitch_deg=0), 192, 192)
    infos, B, V, I = mesh_set(oracle, [synth.uv_sphere(1.0, 4), synth.knot_mesh(96, 24), synth.triangle_soup(64)])
    inst = synth.instances(500, n_mesh=3, seed=synth.SEED_BASE + 8, extent=60.0, scale_range=(0.5, 3.0))
    b = (oracle.tlas_build(inst, infos), inst, infos, B, V, I)
    rb = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 45), pitch_deg=0), 256, 256)
    return {"A": (a, ra, oracle.trace(a, ra, threads=8)[0]), "B": (b, rb, oracle.trace(b, rb, threads=8)[0])}


@pytest.mark.parametrize("fan", [1, 3])
@pytest.mark.parametrize("form", ["in place", "relocated"])
@pytest.mark.parametrize("name", ["trace_40", "synth_300"])
def test_exact_walk_option_off(ctx, ctx_options, parity_scenes, name, form, fan):
    scene, rays, want = parity_scenes[name]
    arrays = wide_form(scene, 40 + len(scene[0])) if form == "relocated" else (widen(scene[0]),) + tuple(scene[1:])
    ctx_options("trace.fan", fan)
    ctx_options("trace.waves", 1)                      # one wave per CU: 16 384 rays are one per lane, the call may fan out
    acc, ds = prepare(ctx, ctx_options, arrays, 0)
    info = acc.info()
    assert info["wide"] and info["tight_tlas"] == 0 and info["tight_fallback_instances"] == 0 and info["refits_since_build"] == 0
    assert info["d_tlas_nodes"] == ds.tensors[0].data_ptr() and info["n_tlas_nodes"] == len(arrays[0])
    assert info["triangle_bytes"] == 36 * (len(scene[5]) // 3)
    got, flags = run(ctx, acc, rays)
    assert records_equal(got, want), (name, form, fan, first_bad(got, want))
    assert np.array_equal(flags, want["hit"])
    acc.refit()                                        # no private top level: a no-op
    assert acc.info() == info
    acc.close()


@pytest.mark.parametrize("kind,length", [("tlas", 200), ("tlas", 1400), ("mixed", (1000, 400))])
def test_stack_seams_through_the_prepared_deep_pass(ctx, ctx_options, oracle, kind, length):
    """Chains, widened and relocated: depths across the LDS / register seam at 24, the first pass's 128 entries and the second
    pass's first 1 Ki entries - walked by trace_wide_kernel<., true, .> and trace_deep_wide_kernel<., true> over the accel's leaves."""
    scene = chain_scene(oracle, length) if kind == "tlas" else chain_mixed_scene(oracle, *length)
    far_x = (length if kind == "tlas" else max(length)) + 50.0
    rays, far_side, cheap = chain_rays(2_000, far_x, seed=77)
    want, _, depth = oracle.trace(scene, rays, threads=16, depths=True)
    top = int(depth.max())
    n_leaves = length if kind == "tlas" else length[0]
    assert (top > 128 + 1024) == (n_leaves >= 1000) and top > 128 and (depth <= 24).any() and want["hit"][depth == top].sum() > 0
    acc, _ = prepare(ctx, ctx_options, wide_form(scene, top), 0)
    got, flags = run(ctx, acc, rays)
    assert records_equal(got, want), (kind, length, first_bad(got, want))
    assert np.array_equal(flags, want["hit"])
    acc.close()


@pytest.mark.parametrize("name,min_hits", [("A", 2000), ("B", 1000)])
def test_tight_overlapping_instances(ctx, ctx_options, tight_scenes, name, min_hits):
    scene, rays, want = tight_scenes[name]
    n = len(scene[1])
    for option in (1, 2):                              # both values select the LBVH for a wide accel
        acc, ds = prepare(ctx, ctx_options, wide_form(scene, 7 + n), option)
        info = acc.info()
        assert info["tight_tlas"] == 2 and info["n_tlas_nodes"] == 2 * n and info["tight_fallback_instances"] == 0, info
        assert info["d_tlas_nodes"] != ds.tensors[0].data_ptr() and info["d_tlas_nodes"]
        got, flags = run(ctx, acc, rays)
        tight_rule(got, flags, want, min_hits)
        acc.close()


def test_smallest_trees_and_grid_tails(ctx, ctx_options, oracle):
    """The thirty-scene generator of test_gpu_trace_tight.py with 257 instances added (a tail of one behind a full workgroup)."""
    rng = np.random.default_rng(20261004)
    pool = [synth.triangle_soup(1, seed=5), synth.triangle_soup(2, seed=6), synth.triangle_soup(3, seed=7), synth.triangle_soup(10, seed=8),
            synth.uv_sphere(1.0, 3), synth.knot_mesh(24, 8), synth.plane_mesh(2.0, 2.0)]
    total, counts = 0, set()
    for scene_no in range(30):
        picks = rng.choice(len(pool), size=int(rng.integers(1, 4)), replace=False)
        n_inst = int(rng.choice([2, 3, 7, 40, 200, 257]))
        counts.add(n_inst)
        inst = synth.instances(n_inst, n_mesh=len(picks), seed=synth.SEED_BASE + 300 + scene_no, extent=12.0, scale_range=(0.5, 3.0))
        infos, B, V, I = mesh_set(oracle, [pool[m] for m in picks])
        scene = (oracle.tlas_build(inst, infos), inst, infos, B, V, I)
        n_rays = 1500
        rays = np.zeros(n_rays, dtype=abi.RAY)
        eye = rng.normal(size=(n_rays, 3)).astype(np.float32) * rng.choice([0.5, 6.0, 25.0], size=(n_rays, 1)).astype(np.float32)
        d = rng.normal(size=(n_rays, 3)).astype(np.float32) * 5.0 - eye
        d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6).astype(np.float32)
        axis = rng.integers(0, n_rays, size=60)
        d[axis] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, size=60)] * rng.choice([-1.0, 1.0], size=(60, 1)).astype(np.float32)
        rays["eye"], rays["dir"] = eye, d.astype(np.float32)
        want, _ = oracle.trace(scene, rays, threads=8)
        acc, ds = prepare(ctx, ctx_options, wide_form(scene, 900 + scene_no), 1)
        info = acc.info()
        assert info["tight_tlas"] == 2 and info["n_tlas_nodes"] == 2 * n_inst and info["tight_fallback_instances"] == 0, (scene_no, info)
        assert info["d_tlas_nodes"] != ds.tensors[0].data_ptr()
        got, flags = run(ctx, acc, rays)
        total += tight_rule(got, flags, want, min_hits=0)
        acc.close()
    assert total > 2000 and counts == {2, 3, 7, 40, 200, 257}, (total, counts)


def test_past_16_bits_of_instances(ctx, ctx_options, oracle):
    """40 000 pairwise disjoint spheres: no two instances can tie, so the record of a ray does not depend on the top level.  The
    yardstick is the plain wide walk over vd_tlas_build_lbvh_wide of the same scene (tests/test_gpu_tlas_lbvh.py holds that pair to
    two exact narrow halves); the prepared tight accel must give its records in all four fields."""
    import torch
    n, n_rays = 40_000, 65_536
    infos, B, V, I = mesh_set(oracle, [synth.uv_sphere(1.0, 5)])
    inst, side = disjoint_instances(n, seed=7)                  # the scene and rays of test_gpu_tlas_lbvh.py's two-halves test
    rays = grid_rays(n_rays, side, seed=77)
    nodes = ctx.tlas_build_lbvh(inst, infos, wide=True)
    arrays = (nodes, inst, infos, B, V, I)
    ds = ctx.device_scene(arrays)
    d_rays, d_hits = ctx.upload(rays), ctx.empty(n_rays * 16)
    d_any = torch.full((n_rays,), 7, dtype=torch.int32, device="cuda")
    ctx.trace_wide_dev(ds, d_rays, n_rays, d_hits)
    ctx.trace_any_wide_dev(ds, d_rays, n_rays, d_any)
    torch.cuda.synchronize()
    want, want_any = d_hits.cpu().numpy()[: n_rays * 16].view(abi.HIT).copy(), d_any.cpu().numpy().astype(np.uint32)
    assert n_rays // 4 <= want["hit"].sum() < n_rays and np.array_equal(want_any, want["hit"])
    acc, _ = prepare(ctx, ctx_options, arrays, 2)
    info = acc.info()
    assert info["tight_tlas"] == 2 and info["n_tlas_nodes"] == 80_000 and info["tight_fallback_instances"] == 0, info
    got, flags = run(ctx, acc, rays)
    if not records_equal(got, want):
        # equal-distance triangles inside one instance would show here: say which rays, then hold them to the tight rule
        print("\nrays whose records differ from the yardstick's:", first_bad(got, want))
        tight_rule(got, flags, want)
    assert records_equal(got, want), first_bad(got, want)
    assert np.array_equal(flags, want_any)
    acc.close()


def test_motion_refit_then_update(ctx, ctx_options, oracle, tight_scenes):
    """Every instance moves (vd_compute_update_dev with the inverse kept in step, by more than a box); refit() then update() of a
    wide accel and of narrow accels of both builders, each against the oracle's walk of the moved scene under a fresh exact build."""
    import torch
    scene, rays, _ = tight_scenes["A"]
    n = len(scene[1])
    ids = np.arange(n, dtype=np.uint32)
    time, dt = np.pi, 0.25                                  # compute_update.wgsl: rotz by 2 sin(time / 2) dt = 0.5 rad about the world's z axis
    moved = oracle.compute_update(ids, scene[1], time, dt, True)
    shift = np.linalg.norm(moved["transform"][:, 12:15] - scene[1]["transform"][:, 12:15], axis=1)
    largest_box = 2.0 * np.linalg.norm(scene[2][0]["max"] - scene[2][0]["min"])      # the mesh's diagonal at the largest scale: no tight box is wider
    assert np.median(shift) > largest_box and shift.max() > 2.0 * largest_box, (float(np.median(shift)), float(largest_box))
    want, _ = oracle.trace((oracle.tlas_build(moved, scene[2]), moved) + tuple(scene[2:]), rays, threads=8)
    assert want["hit"].sum() > 2000
    for kind, option in (("wide", 2), ("narrow", 1), ("narrow", 2)):
        acc, ds = prepare(ctx, ctx_options, wide_form(scene, 11) if kind == "wide" else scene, option)
        mode = 2 if kind == "wide" else option

        def state():
            i = acc.info()
            assert i["tight_tlas"] == mode and i["tight_fallback_instances"] == 0 and i["wide"] == (kind == "wide"), (kind, option, i)
            return i
        first = state()
        ctx.compute_update_dev(ctx.upload(ids), n, ds.tensors[1], n, time, dt, True)
        torch.cuda.synchronize()
        assert ds.tensors[1].cpu().numpy().view(abi.INSTANCE).tobytes() == moved.tobytes()
        acc.refit()
        after_refit = state()
        assert after_refit["d_tlas_nodes"] == first["d_tlas_nodes"] and after_refit["n_tlas_nodes"] == first["n_tlas_nodes"]
        got, flags = run(ctx, acc, rays)
        tight_rule(got, flags, want, 2000)
        acc.update()
        after_update = state()
        got, flags = run(ctx, acc, rays)
        tight_rule(got, flags, want, 2000)
        if kind == "wide":
            assert [first["refits_since_build"], after_refit["refits_since_build"], after_update["refits_since_build"]] == [0, 1, 0]
        acc.close()


def test_decline_and_return(ctx, ctx_options, oracle):
    import torch
    infos, B, V, I = mesh_set(oracle, [synth.uv_sphere(1.0, 6), synth.knot_mesh(48, 12)])
    good = synth.instances(60, n_mesh=2, seed=synth.SEED_BASE + 43, extent=20.0, scale_range=(0.6, 2.5))
    bad = good.copy()
    bad["transform"][17, 12] += np.float32(3.5)              # moved without its inverse: |T * Tinv - I| = 3.5 > 1e-3
    rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 35), pitch_deg=0), 160, 160)
    bad_scene = (oracle.tlas_build(bad, infos), bad, infos, B, V, I)
    want_bad, _ = oracle.trace(bad_scene, rays, threads=8)
    want_good, _ = oracle.trace((oracle.tlas_build(good, infos), good, infos, B, V, I), rays, threads=8)
    assert want_bad["hit"].sum() > 1000
    acc, ds = prepare(ctx, ctx_options, wide_form(bad_scene, 60), 1)
    own = ds.tensors[0].data_ptr()

    def put(inst):
        ds.tensors[1].copy_(torch.from_numpy(np.ascontiguousarray(inst).view(np.uint8).reshape(-1)))

    def declined():
        info = acc.info()
        assert info["tight_tlas"] == 0 and info["tight_fallback_instances"] == 1 and info["d_tlas_nodes"] == own and info["n_tlas_nodes"] == 200_000, info
        got, flags = run(ctx, acc, rays)
        assert records_equal(got, want_bad), first_bad(got, want_bad)        # the scene's own top level: the exact walk
        assert np.array_equal(flags, want_bad["hit"])
    declined()
    put(good)
    acc.refit()
    info = acc.info()
    assert info["tight_tlas"] == 2 and info["tight_fallback_instances"] == 0 and info["d_tlas_nodes"] != own and info["n_tlas_nodes"] == 120, info
    got, flags = run(ctx, acc, rays)
    tight_rule(got, flags, want_good, 1000)
    put(bad)
    acc.refit()
    declined()
    acc.close()


def test_deformed_mesh(ctx, ctx_options, oracle):
    """The vertices shrink in the device buffer, the BLAS is refitted, update_geometry() de-indexes the leaves again: the accel's
    records are those of the plain wide call walking indices[] -> vertices[] of the same buffers."""
    import torch
    v, i = synth.knot_mesh(64, 16)
    infos, B, V, I = mesh_set(oracle, [(v, i)])
    inst = synth.instances(100, n_mesh=1, seed=synth.SEED_BASE + 33, extent=30.0, scale_range=(0.5, 2.0))
    scene = (oracle.tlas_build(inst, infos), inst, infos, B, V, I)
    rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 40), pitch_deg=0), 128, 128)
    acc, ds = prepare(ctx, ctx_options, wide_form(scene, 33), 0)
    before, _ = run(ctx, acc, rays)
    V2 = (V.astype(np.float32) * np.array([0.7, 0.85, 0.6], np.float32)).astype(np.float32)
    ds.tensors[4].copy_(torch.from_numpy(V2.reshape(-1).view(np.uint8)))
    ds.tensors[3].copy_(torch.from_numpy(ctx.bvh_refit(V2, I, B).view(np.uint8).reshape(-1)))
    acc.update_geometry()
    got, flags = run(ctx, acc, rays)
    ctx_options("trace.auto_prepare", 0)
    n = len(rays)
    d_hits = ctx.empty(n * 16)
    ctx.trace_wide_dev(ds, ctx.upload(rays), n, d_hits)
    torch.cuda.synchronize()
    want = d_hits.cpu().numpy()[: n * 16].view(abi.HIT)
    assert want["hit"].sum() > 300 and not records_equal(want, before)
    assert records_equal(got, want), first_bad(got, want)
    assert np.array_equal(flags, want["hit"])
    acc.close()


def test_one_context_both_kinds(ctx, ctx_options, parity_scenes):
    scene, rays, want = parity_scenes["synth_300"]
    narrow, _ = prepare(ctx, ctx_options, scene, 2)
    wide, _ = prepare(ctx, ctx_options, wide_form(scene, 300), 2)
    assert narrow.info()["tight_tlas"] == 2 and not narrow.info()["wide"] and wide.info()["tight_tlas"] == 2 and wide.info()["wide"]
    first = {}
    for rep in range(2):
        for name, acc in (("narrow", narrow), ("wide", wide)):
            got, flags = run(ctx, acc, rays)
            if rep == 0:
                tight_rule(got, flags, want, 1000)
                first[name] = (got, flags)
            assert records_equal(got, first[name][0]) and np.array_equal(flags, first[name][1]), (rep, name)
    # each info call refuses a handle of the other kind
    import ctypes as C
    assert ctx.lib.vd_trace_accel_info(wide.h, C.byref(abi.TraceAccelInfo())) == abi.VD_ERR_INVALID_ARG
    assert b"vd_trace_accel_info_wide" in ctx.lib.vd_last_error(ctx.h)
    assert ctx.lib.vd_trace_accel_info_wide(narrow.h, C.byref(abi.TraceAccelInfoWide())) == abi.VD_ERR_INVALID_ARG
    assert b"use vd_trace_accel_info" in ctx.lib.vd_last_error(ctx.h) and b"use vd_trace_accel_info_wide" not in ctx.lib.vd_last_error(ctx.h)
    assert ctx.lib.vd_trace_accel_info(narrow.h, C.byref(abi.TraceAccelInfo())) == abi.VD_OK
    assert ctx.lib.vd_trace_accel_info_wide(wide.h, C.byref(abi.TraceAccelInfoWide())) == abi.VD_OK
    narrow.close(); wide.close()


def test_prepare_wide_refuses_what_prepare_refuses(ctx, ctx_options, parity_scenes):
    scene, rays, want = parity_scenes["trace_40"]
    arrays = (widen(scene[0]),) + tuple(scene[1:])
    ds = ctx.device_scene(arrays)
    ds.struct.n_tlas_nodes = 2 * abi.TLAS_WIDE_MAX_INSTANCES + 2
    with pytest.raises(VoidinError) as e:
        ctx.trace_prepare(ds)
    assert e.value.code == abi.VD_ERR_INVALID_ARG and "VD_TLAS_WIDE_MAX_INSTANCES" in str(e.value)
    ds = ctx.device_scene(arrays)
    ds.struct.n_indices = 0
    with pytest.raises(VoidinError) as e:
        ctx.trace_prepare(ds)
    assert e.value.code == abi.VD_ERR_INVALID_ARG and "incomplete scene" in str(e.value)
    bad = np.array(scene[5], dtype=np.uint32, copy=True)
    bad[5] = len(scene[4]) + 1000                      # a vertex index past the vertex buffer
    with pytest.raises(VoidinError) as e:
        ctx.trace_prepare(ctx.device_scene(arrays[:5] + (bad,)))
    assert e.value.code == abi.VD_ERR_INVALID_ARG
    acc, _ = prepare(ctx, ctx_options, arrays, 0)      # and the next call is right
    got, flags = run(ctx, acc, rays)
    assert records_equal(got, want)
    acc.close()
