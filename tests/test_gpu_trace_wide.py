"""vd_trace_wide_dev / vd_trace_any_wide_dev: the walk over VdTlasNodeWide (32-bit child ids).

The oracle walks narrow nodes only, so every scene here is a narrow scene whose top level is rewritten as wide nodes
(left = left_right & 0xffff, right = left_right >> 16) and then RELOCATED: the root stays at 0, every other node goes to a seeded
random slot of a 200 000-slot array (indices pass 16 bits), child ids follow, unused slots are 0xff bytes.  The topology is the
narrow scene's, so each ray's record must equal vd_ref_trace of the narrow scene bit for bit - dist, hit, instance, triangle."""
import numpy as np
import pytest

from chain_scenes import chain_mixed_scene, chain_rays, chain_scene
from conftest import golden
from voidin_amd import abi, synth
from voidin_amd.runtime import VoidinError
from wide_scenes import first_bad, mesh_set, reachable, records_equal, relocate, widen

pytestmark = pytest.mark.gpu


def _wide_calls(ctx, scene, wide_nodes, rays):
    """(records, flags) of vd_trace_wide_dev and vd_trace_any_wide_dev over `scene` with `wide_nodes` as its top level."""
    import torch
    n = len(rays)
    ds = ctx.device_scene((wide_nodes,) + tuple(scene[1:]))
    assert ds.wide
    d_rays, d_hits = ctx.upload(rays), ctx.empty(n * 16)
    d_hits.fill_(0xEE)
    d_any = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.trace_wide_dev(ds, d_rays, n, d_hits)
    ctx.trace_any_wide_dev(ds, d_rays, n, d_any)
    torch.cuda.synchronize()
    return d_hits.cpu().numpy()[: n * 16].view(abi.HIT), d_any.cpu().numpy().astype(np.uint32)


@pytest.fixture(scope="module")
def parity_scenes(oracle):
    """name -> (narrow scene, rays, the oracle's records): the golden 40-instance scene with its own rays, and a seeded scene of
    300 instances of three meshes under 16 384 primary rays (one per lane of a grid of one wave per CU)."""
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
    assert out["trace_40"][2]["dist"].tobytes() == g["dist"].tobytes()
    return out


@pytest.mark.parametrize("fan", [1, 3])
@pytest.mark.parametrize("auto_prepare", [0, 1])
@pytest.mark.parametrize("form", ["in place", "relocated"])
@pytest.mark.parametrize("name", ["trace_40", "synth_300"])
def test_oracle_parity_through_relocated_nodes(ctx, ctx_options, parity_scenes, name, form, auto_prepare, fan):
    scene, rays, want = parity_scenes[name]
    wide = widen(scene[0])
    if form == "relocated":
        wide, pos = relocate(wide, seed=40 + len(scene[0]))
        assert len(wide) == 200_000 and reachable(wide).sum() <= len(scene[0])
    ctx_options("trace.auto_prepare", auto_prepare)
    ctx_options("trace.fan", fan)
    ctx_options("trace.waves", 1)                      # a grid of one wave per CU: 16 384 rays are one per lane, the call may fan out
    got, flags = _wide_calls(ctx, scene, wide, rays)
    assert records_equal(got, want), (name, form, auto_prepare, fan, first_bad(got, want))
    assert np.array_equal(flags, want["hit"])


def test_the_fan_out_runs_on_the_wide_walk(ctx, ctx_options, oracle):
    """A dense scene (1 500 overlapping instances: rays of thousands of steps) under 16 384 rays and a grid of one wave per CU:
    draining waves turn their rays into jobs.  The fan-out leaves no trace in the ABI, so that it ran is shown the way the narrow
    tests show it - 1, 2, 3 and 4 launches give the same bytes, and those are the oracle's - plus the time: with jobs made, the
    call with fan-out must not be the same call (vd_last_gpu_ms differs; printed, not asserted)."""
    infos, B, V, I = mesh_set(oracle, [synth.knot_mesh(64, 16), synth.uv_sphere(1.0, 6)])
    inst = synth.instances(1500, n_mesh=2, seed=synth.SEED_BASE + 8, extent=60.0, scale_range=(0.5, 2.0))
    scene = (oracle.tlas_build(inst, infos), inst, infos, B, V, I)
    rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 45.0), pitch_deg=0), 128, 128)
    want, _ = oracle.trace(scene, rays, threads=16)
    assert want["hit"].sum() > 3000
    wide, _ = relocate(widen(scene[0]), seed=1500)
    ctx_options("trace.waves", 1)
    ctx.set_timing(True)
    try:
        ms = {}
        for fan in (1, 2, 3, 4):
            ctx_options("trace.fan", fan)
            got, flags = _wide_calls(ctx, scene, wide, rays)
            ms[fan] = round(ctx.last_gpu_ms(), 3)
            assert records_equal(got, want), (fan, first_bad(got, want))
            assert np.array_equal(flags, want["hit"]), fan
    finally:
        ctx.set_timing(False)
    print(f"\nwide walk, 1500 instances, 16384 rays, any-hit call ms by launches: {ms}")


@pytest.mark.parametrize("kind,length", [("tlas", 200), ("tlas", 1400), ("mixed", (200, 60)), ("mixed", (1000, 400))])
def test_stack_seams(ctx, ctx_options, oracle, kind, length):
    """Chains, widened and relocated: depths across the LDS / register seam at 24 and the first pass's 128 entries (200 leaves) and
    across the second pass's first 1 Ki entries (1 400 leaves; 1 000 leaves + a 400-triangle BLAS chain entered on top of them)."""
    scene = chain_scene(oracle, length) if kind == "tlas" else chain_mixed_scene(oracle, *length)
    far_x = (length if kind == "tlas" else max(length)) + 50.0
    rays, far_side, cheap = chain_rays(2_000, far_x, seed=77)
    want, _, depth = oracle.trace(scene, rays, threads=16, depths=True)
    top = int(depth.max())
    n_leaves = length if kind == "tlas" else length[0]
    assert (top > 128 + 1024) == (n_leaves >= 1000) and top > 128 and (depth <= 24).any() and want["hit"][depth == top].sum() > 0
    wide, _ = relocate(widen(scene[0]), seed=top)
    for auto_prepare in (0, 1):
        ctx_options("trace.auto_prepare", auto_prepare)
        got, flags = _wide_calls(ctx, scene, wide, rays)
        assert records_equal(got, want), (kind, length, auto_prepare, first_bad(got, want))
        assert np.array_equal(flags, want["hit"])


def _knot_scene(oracle, n_inst=200):
    infos, B, V, I = mesh_set(oracle, [synth.knot_mesh(64, 16)])
    inst = synth.instances(n_inst, n_mesh=1, seed=synth.SEED_BASE + 33, extent=40.0, scale_range=(0.5, 2.0))
    return (oracle.tlas_build(inst, infos), inst, infos, B, V, I)


def test_two_pairs_naming_one_left_child(ctx, oracle):
    """Unreachable slots of the array name a reachable node's LEFT child with another right child (the reference's own arrays keep
    such slots: tlas.rs:62-84; tests/test_gpu_tlas_trace.py does this to the narrow walk).  The wide walk's records sit at the
    PARENT's index, one writer each, so such a slot cannot disturb a reachable step: same records, every repetition."""
    scene = _knot_scene(oracle)
    rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 45), pitch_deg=0), 160, 160)
    want, _ = oracle.trace(scene, rays, threads=8)
    assert want["hit"].sum() > 500
    wide, pos = relocate(widen(scene[0]), seed=5)
    reach = reachable(wide)
    interior = np.nonzero(reach & ((wide["left"] != 0) | (wide["right"] != 0)))[0]
    free = np.nonzero(~reach)[0]
    assert len(interior) > 50
    stale = wide.copy()
    lo = free[free < interior.min()][:32] if (free < interior.min()).any() else free[:0]
    for n, k in enumerate(np.concatenate([lo, free[-64:], free[1000:1032]])):        # below and above the nodes they contest
        stale["left"][k] = wide["left"][interior[(7 * n) % len(interior)]]
        stale["right"][k] = interior[(3 * n + 1) % len(interior)]
        stale["instance_idx"][k] = 0xffffffff
    assert not reachable(stale)[~reach].any()
    for rep in range(3):
        got, flags = _wide_calls(ctx, scene, stale, rays)
        assert records_equal(got, want), (rep, first_bad(got, want))
        assert np.array_equal(flags, want["hit"])


def test_errors(ctx, oracle):
    """A child id past the array, or an interior node without a left child, is VD_ERR_INVALID_ARG when a ray REACHES it and nothing
    at all when none does; too many nodes is refused before anything is launched; and the next narrow call is right."""
    import torch
    scene = _knot_scene(oracle, 120)
    tl = scene[0]
    inst = scene[1]
    dirs = np.array([(0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)], dtype=np.float32)
    aim = np.zeros(len(inst) * 6, dtype=abi.RAY)           # at every instance from six sides: every reachable node is reached
    for k, d in enumerate(dirs):
        aim["eye"][k::6] = inst["transform"][:, 12:15] - 30.0 * d; aim["dir"][k::6] = d
    want, _ = oracle.trace(scene, aim, threads=8)
    wide, pos = relocate(widen(tl), seed=9)
    reach = reachable(wide)
    interior = np.nonzero(reach & ((wide["left"] != 0) | (wide["right"] != 0)))[0]
    deep_node = int(interior[len(interior) // 2])
    free = np.nonzero(~reach)[0]

    def run(nodes, n_nodes=None):
        ds = ctx.device_scene((nodes,) + tuple(scene[1:]))
        if n_nodes is not None:
            ds.struct.n_tlas_nodes = n_nodes
        d_h = ctx.empty(len(aim) * 16)
        ctx.trace_wide_dev(ds, ctx.upload(aim), len(aim), d_h)
        torch.cuda.synchronize()
        return d_h.cpu().numpy()[: len(aim) * 16].view(abi.HIT)

    assert records_equal(run(wide), want)
    cases = {}
    for name, field, value in (("right child past the array", "right", len(wide)), ("left child far past the array", "left", 0xfffffff0),
                               ("interior node with left == 0", "left", 0)):
        bad = wide.copy(); bad[field][deep_node] = value
        cases[name] = bad
        hidden = wide.copy(); hidden[field][free[3]] = value; hidden["right" if field == "left" else "left"][free[3]] = int(interior[0])
        assert records_equal(run(hidden), want), name          # the same node where no ray gets: VD_OK and the same records
    for name, bad in cases.items():
        with pytest.raises(VoidinError) as e:
            run(bad)
        assert e.value.code == abi.VD_ERR_INVALID_ARG, name
    # the any-hit form reports it too
    with pytest.raises(VoidinError) as e:
        ds = ctx.device_scene((cases["right child past the array"],) + tuple(scene[1:]))
        ctx.trace_any_wide_dev(ds, ctx.upload(aim), len(aim), torch.zeros(len(aim), dtype=torch.int32, device="cuda"))
    assert e.value.code == abi.VD_ERR_INVALID_ARG
    # everything the narrow call refuses: a leaf whose instance lies outside the buffer
    leaf = int(np.nonzero(reach & (wide["left"] == 0) & (wide["right"] == 0))[0][0])
    bad_leaf = wide.copy(); bad_leaf["instance_idx"][leaf] = len(inst) + 5
    with pytest.raises(VoidinError) as e:
        run(bad_leaf)
    assert e.value.code == abi.VD_ERR_INVALID_ARG
    # more nodes than the wide layout is specified for: refused at once (the array is not read)
    with pytest.raises(VoidinError) as e:
        run(wide, n_nodes=2 * abi.TLAS_WIDE_MAX_INSTANCES + 2)
    assert e.value.code == abi.VD_ERR_INVALID_ARG and "VD_TLAS_WIDE_MAX_INSTANCES" in str(e.value)
    # after the failing calls: the narrow call, and the wide one again
    d_h = ctx.empty(len(aim) * 16)
    ctx.trace_dev(ctx.device_scene(scene), ctx.upload(aim), len(aim), d_h)
    torch.cuda.synchronize()
    assert records_equal(d_h.cpu().numpy()[: len(aim) * 16].view(abi.HIT), want)
    assert records_equal(run(wide), want)
    # host-pointer form
    assert records_equal(ctx.trace_wide((widen(tl),) + tuple(scene[1:]), aim), want)
