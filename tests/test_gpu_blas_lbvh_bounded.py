"""VD_OPT_BLAS_LBVH_MAX_DEPTH: the depth-bounded LBVH bottom level on the GPU against the top-down numpy restatement of
tests/blas_lbvh_bounded_cases.py byte for byte - through vd_bvh_build_lbvh_dev, the host form, a plan of many meshes with the counts
on the device, and a captured HIP graph - the bounds that cannot fire against the unbounded build, the refusal of a bound that
cannot hold the mesh, and the consumers of a BLAS over the D = 23 helmet."""
import numpy as np
import pytest

import blas_lbvh_bounded_cases as bounded
import blas_lbvh_cases as cases
from blas_refit_cases import deform
from conftest import fields_equal, first_difference
from test_gpu_blas_lbvh import _build_dev, _input
from test_gpu_blas_lbvh_batch import Batch, _expect_equals_single
from voidin_amd import abi, synth
from voidin_amd.runtime import VoidinError
from wide_scenes import disjoint_instances, first_bad, grid_rays, mesh_set, records_equal

pytestmark = pytest.mark.gpu

OPTION = "blas.lbvh_max_depth"
_refs = {}


def _reference(name, D, arrays=None):
    """The restatement of one input under one bound, computed once and shared, never written."""
    if (name, D) not in _refs:
        v, i = arrays if arrays is not None else _input(name)
        r = bounded.lbvh_bounded_reference(v, i, D)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[(name, D)] = (np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(i, dtype=np.uint32), r)
    return _refs[(name, D)]


def _check(ctx, ctx_options, name, D, arrays=None):
    """Nodes, indices, the result record, the canary past n_nodes, two builds identical.  -> (nodes, indices, restatement)."""
    v, i, r = _reference(name, D, arrays)
    ctx_options(OPTION, D)
    raw, idx, res = _build_dev(ctx, v, i)
    n = int(res["n_nodes"])
    assert (n, int(res["max_depth"]), int(res["n_bad_indices"]), int(res["_pad"])) == (r["n_nodes"], r["max_depth"], r["n_bad_indices"], 0), (name, D)
    assert int(res["max_depth"]) <= D
    got = raw[: n * 32].view(abi.BVH_NODE)
    assert fields_equal(got, r["nodes"]), (name, D, first_difference(got, r["nodes"]))
    assert np.array_equal(idx, r["indices"])
    assert (raw[n * 32:] == 0xCD).all(), "bytes past n_nodes were written"
    raw2, idx2, res2 = _build_dev(ctx, v, i, fill=0x11)
    assert raw2[: n * 32].tobytes() == raw[: n * 32].tobytes() and idx2.tobytes() == idx.tobytes() and res2.tobytes() == res.tobytes(), "two builds differ"
    return got, idx, r


@pytest.mark.parametrize("T", [4, 5, 8, 9, 64, 65, 1025, 4097])
def test_soup_equals_the_restatement(ctx, ctx_options, T):
    fired = 0
    for D in (bounded.needr(T), bounded.needr(T) + 1, 23):
        got, idx, r = _check(ctx, ctx_options, T, D)
        fired += r["switches"]
        nodes_h, idx_h = ctx.bvh_build_lbvh(*_input(T))                 # the host-pointer form: the same bytes
        assert nodes_h.tobytes() == got.tobytes() and np.array_equal(idx_h, idx)
    assert fired > 0 or T in (4, 5, 9)                                    # (the rule fires at the tightest bound of the others)


@pytest.mark.parametrize("name", ["helmet", "knot", "sphere"] + sorted(cases.special_cases()))
def test_mesh_equals_the_restatement(ctx, ctx_options, name):
    biting = 16 if name in ("helmet", "knot", "sphere") else 9
    for D in (23, biting):
        _, _, r = _check(ctx, ctx_options, name, D)
        if name in ("helmet", "knot", "sphere"):
            assert r["switches"] > 0 or (name, D) == ("knot", 23)       # knot() is 18 deep: 23 leaves it alone


def test_duplicates_equal_the_restatement(ctx, ctx_options):
    """Ranges of equal codes hold more positions than codes: switch nodes whose end keys differ in the code (delta < 32) and ones
    inside a run of one code (delta >= 32), whose low words keep the positions' common prefix."""
    for D in (11, 12):
        _, _, r = _check(ctx, ctx_options, "duplicates", D, arrays=bounded.duplicates_case())
        assert r["switch_delta_below_32"] > 0 and r["switch_delta_from_32"] > 0


def test_random_soups_on_a_grid_equal_the_restatement(ctx, ctx_options):
    fired = 0
    for c, (v, i, D) in enumerate(bounded.random_cases()):
        fired += _check(ctx, ctx_options, f"random{c}", D, arrays=(v, i))[2]["switches"] > 0
    assert fired >= 10


def _unbounded(ctx, ctx_options, name):
    ctx_options(OPTION, None)
    v, i = _input(name)
    raw, idx, res = _build_dev(ctx, np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(i, dtype=np.uint32))
    return raw, idx, res


@pytest.mark.parametrize("name", ["helmet", "identical_1000", 4097])
def test_a_bound_that_cannot_fire_gives_the_unbounded_bytes(ctx, ctx_options, name):
    """D = 62 (and anything above, read as 62) runs the key pass and the second tree pass over keys that are all (code, position)."""
    raw0, idx0, res0 = _unbounded(ctx, ctx_options, name)
    v, i = _input(name)
    for D in (62, 1000):
        ctx_options(OPTION, D)
        raw, idx, res = _build_dev(ctx, np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(i, dtype=np.uint32))
        assert res.tobytes() == res0.tobytes() and raw.tobytes() == raw0.tobytes() and idx.tobytes() == idx0.tobytes()


def test_a_negative_value_restores_the_unbounded_build(ctx, ctx_options):
    raw0, idx0, res0 = _unbounded(ctx, ctx_options, "helmet")
    assert int(res0["max_depth"]) == 24                                   # what the option is for
    v, i, r = _reference("helmet", 23)
    ctx_options(OPTION, 23)
    assert int(_build_dev(ctx, v, i)[2]["max_depth"]) == 23
    ctx_options(OPTION, -1)
    raw, idx, res = _build_dev(ctx, v, i)
    assert res.tobytes() == res0.tobytes() and raw.tobytes() == raw0.tobytes() and idx.tobytes() == idx0.tobytes()
    ctx_options(OPTION, 0)
    raw, idx, res = _build_dev(ctx, v, i)
    assert res.tobytes() == res0.tobytes() and raw.tobytes() == raw0.tobytes() and idx.tobytes() == idx0.tobytes()


def test_a_bound_that_cannot_hold_the_mesh_is_refused(ctx, ctx_options):
    import torch
    v, i = cases.special_cases()["identical_1000"]
    v, i = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(i, dtype=np.uint32)
    ctx_options(OPTION, 8)
    d_v, d_i = ctx.upload(v), ctx.upload(i)
    d_n = torch.full((2000 * 32,), 0xCD, dtype=torch.uint8, device="cuda")
    d_r = torch.full((16,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(VoidinError) as e:
        ctx.bvh_build_lbvh_dev(d_v, len(v), d_i, 1000, d_n, 2000, d_r)
    assert e.value.code == abi.VD_ERR_INVALID_ARG and "VD_OPT_BLAS_LBVH_MAX_DEPTH" in str(e.value) and "is 9" in str(e.value), e.value
    torch.cuda.synchronize()
    assert (d_n.cpu().numpy() == 0xCD).all() and (d_r.cpu().numpy() == 0xEE).all() and np.array_equal(d_i.cpu().numpy()[: 12000].view(np.uint32), i)
    with pytest.raises(VoidinError) as e:
        ctx.bvh_build_lbvh(v, i)
    assert e.value.code == abi.VD_ERR_INVALID_ARG
    ctx_options(OPTION, 9)
    _check(ctx, ctx_options, "identical_1000", 9)


BATCH_CAPS = [3, 4, 300, 1025, 4097]
BATCH_COUNTS = [0, 3, 4, 1025, 2000]


def test_planned_build_equals_the_single_bounded_builds(ctx, ctx_options):
    """A plan made under D = 12: every mesh == its single bounded build (itself checked against the restatement above), a count of 0
    gives an all-zero result; the option set to 0 AFTER the plan changes nothing in the plan's next build."""
    meshes = [synth.triangle_soup(c, seed=synth.SEED_BASE + 300 + c) for c in BATCH_CAPS]
    ctx_options(OPTION, 12)
    b = Batch(ctx, meshes)
    try:
        b.load(BATCH_COUNTS)
        b.build()
        first = b.fetch()
        memo = {}
        for m, (v, i) in enumerate(meshes):
            _expect_equals_single(ctx, first[m], v, i, BATCH_COUNTS[m], BATCH_CAPS[m], memo, m)
        T = min(BATCH_COUNTS[4], BATCH_CAPS[4])
        want = bounded.lbvh_bounded_reference(meshes[4][0], meshes[4][1][: 3 * T], 12)
        got = first[4][0][: 32 * want["n_nodes"]].view(abi.BVH_NODE)
        assert want["switches"] > 0 and fields_equal(got, want["nodes"]), first_difference(got, want["nodes"])
        assert int(first[4][2]["max_depth"]) == want["max_depth"] <= 12
        ctx_options(OPTION, 0)                                            # the plan latched 12
        b.load(BATCH_COUNTS)
        b.build()
        for m, (raw, idx, res) in enumerate(b.fetch()):
            assert raw.tobytes() == first[m][0].tobytes() and idx.tobytes() == first[m][1].tobytes() and res.tobytes() == first[m][2].tobytes(), m
        v, i = meshes[4]
        unb = _build_dev(ctx, np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(i[: 3 * T], dtype=np.uint32))
        assert unb[2].tobytes() != first[4][2].tobytes() or unb[0][: 64 * T].tobytes() != first[4][0][: 64 * T].tobytes(), "the bound changed nothing: no test"
    finally:
        b.close()


def test_plan_refuses_a_capacity_the_bound_cannot_hold(ctx, ctx_options):
    meshes = [synth.triangle_soup(c, seed=synth.SEED_BASE + 300 + c) for c in (64, 1000)]
    ctx_options(OPTION, 8)
    code, statuses, handle = _plan_statuses(ctx, meshes)
    assert code == abi.VD_ERR_INVALID_ARG and statuses == [0, abi.VD_ERR_INVALID_ARG] and not handle
    assert b"VD_OPT_BLAS_LBVH_MAX_DEPTH" in ctx.lib.vd_last_error(ctx.h)
    ctx_options(OPTION, 9)
    code, statuses, handle = _plan_statuses(ctx, meshes)
    assert code == abi.VD_OK and statuses == [0, 0] and handle
    ctx.lib.vd_bvh_lbvh_plan_release(ctx.h, handle)


def _plan_statuses(ctx, meshes):
    """vd_bvh_lbvh_plan_dev over device copies of the meshes -> (return code, the items' statuses, the plan handle or None)."""
    import ctypes as C
    import torch
    keep = []
    items = (abi.BvhLbvhBatchItem * len(meshes))()
    for m, (v, i) in enumerate(meshes):
        cap = len(i) // 3
        d_v, d_i = ctx.upload(np.ascontiguousarray(v, dtype=np.float32)), ctx.upload(np.ascontiguousarray(i, dtype=np.uint32))
        d_n = torch.zeros((64 * cap,), dtype=torch.uint8, device="cuda")
        keep.append((d_v, d_i, d_n))
        it = items[m]
        it.verts_xyz, it.indices_inout, it.nodes, it.mesh_info = abi.ptr(d_v), abi.ptr(d_i), abi.ptr(d_n), None
        it.n_vert, it.tri_cap, it.node_cap = len(v), cap, 2 * cap
    h = C.c_void_p()
    code = ctx.lib.vd_bvh_lbvh_plan_dev(ctx.h, C.addressof(items), len(meshes), C.byref(h))
    return code, [it.status for it in items], h.value


def test_bounded_rebuild_from_a_hip_graph(ctx, ctx_options):
    """A 4 096-triangle bounded build captured after one uncaptured warm-up call under the same bound (which sizes the work memory,
    the explicit keys included); three replays with vertices AND indices rewritten, each equal to an uncaptured build."""
    import torch
    T, D = 4096, 12
    cap = 2 * T
    v0, i0 = synth.triangle_soup(T, seed=synth.SEED_BASE + 400)
    ctx_options(OPTION, D)
    d_v, d_i = ctx.upload(v0), ctx.upload(i0)
    d_n = torch.zeros((cap * 32,), dtype=torch.uint8, device="cuda")
    d_r = torch.zeros((16,), dtype=torch.uint8, device="cuda")

    def frame():
        ctx.bvh_build_lbvh_dev(d_v, len(v0), d_i, T, d_n, cap, d_r)

    frame()                                              # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    main_stream = torch.cuda.current_stream().cuda_stream
    try:
        with torch.cuda.graph(graph):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            frame()
    finally:
        ctx.set_stream(main_stream)
    seen, fired = set(), 0
    rng = np.random.default_rng(43)
    for f in range(3):
        v = deform(v0, phase=0.5 * (f + 1), specials=False)
        i = i0.reshape(-1, 3)[rng.permutation(T)][:, [1, 2, 0]].reshape(-1).copy()
        d_v.copy_(ctx.upload(v)); d_i[: 12 * T].copy_(ctx.upload(i)[: 12 * T])
        d_n.fill_(0xCD)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        raw, idx, res = _build_dev(ctx, v, i)
        n = int(res["n_nodes"])
        assert d_r.cpu().numpy().tobytes() == res.tobytes() and int(res["max_depth"]) <= D
        got = d_n.cpu().numpy()
        assert got[: n * 32].tobytes() == raw[: n * 32].tobytes() and (got[n * 32:] == 0xCD).all()
        assert d_i.cpu().numpy()[: 12 * T].tobytes() == idx.tobytes()
        seen.add(got[: n * 32].tobytes())
        fired += bounded.lbvh_bounded_reference(v, i, D)["switches"] > 0 if f == 0 else 0
    assert len(seen) == 3 and fired == 1                 # three different frames; the rule fires in what was replayed


def test_trace_over_the_bounded_helmet(ctx, ctx_options, oracle):
    """vd_trace_dev, vd_trace_prepared_dev and vd_trace_any_dev over the GPU-built D = 23 helmet == the oracle over the same arrays in
    all four record fields (27 disjoint instances, 40 000 rays)."""
    import torch
    v, i, r = _reference("helmet", 23)
    ctx_options(OPTION, 23)
    nodes, idx = ctx.bvh_build_lbvh(v, i)
    assert fields_equal(nodes, r["nodes"]) and r["max_depth"] == 23
    infos, B, V, I = mesh_set(oracle, [(v, i)])
    inst, side = disjoint_instances(27, 5)
    rays = grid_rays(40_000, side, 7)
    arrays = (oracle.tlas_build(inst, infos), inst, infos, nodes, V, idx)
    want, deepest = oracle.trace(arrays, rays, threads=16)
    assert want["hit"].sum() > 1000 and (want["hit"] == 0).any() and deepest <= 24
    n = len(rays)
    d_rays = ctx.upload(rays)
    ds = ctx.device_scene(arrays)
    d_h, d_p = ctx.empty(n * 16), ctx.empty(n * 16)
    d_any = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.trace_dev(ds, d_rays, n, d_h)
    ctx.trace_any_dev(ds, d_rays, n, d_any)
    accel = ctx.trace_prepare(ds)
    ctx.trace_prepared_dev(accel, d_rays, n, d_p)
    torch.cuda.synchronize()
    got = d_h.cpu().numpy()[: n * 16].view(abi.HIT)
    got_p = d_p.cpu().numpy()[: n * 16].view(abi.HIT)
    assert records_equal(got, want), first_bad(got, want)
    assert records_equal(got_p, want), first_bad(got_p, want)
    assert np.array_equal(d_any.cpu().numpy().astype(np.uint32), want["hit"])
    accel.close()


def test_refit_takes_the_bounded_array(ctx, ctx_options):
    import torch
    v, i, r = _reference("helmet", 23)
    ctx_options(OPTION, 23)
    nodes, idx = ctx.bvh_build_lbvh(v, i)
    d_v, d_i, d_n = ctx.upload(v), ctx.upload(idx), ctx.upload(nodes)
    items = (abi.BvhRefitItem * 1)()
    items[0].verts_xyz, items[0].indices, items[0].nodes, items[0].mesh_info = abi.ptr(d_v), abi.ptr(d_i), abi.ptr(d_n), None
    items[0].n_vert, items[0].n_tri, items[0].n_nodes = len(v), len(idx) // 3, len(nodes)
    plan = ctx.bvh_refit_plan(items)
    assert items[0].status == 0
    ctx.bvh_refit_planned(plan); torch.cuda.synchronize()
    assert d_n.cpu().numpy()[: len(nodes) * 32].tobytes() == nodes.tobytes(), "a refit changed a bounded LBVH array"
    plan.close()
