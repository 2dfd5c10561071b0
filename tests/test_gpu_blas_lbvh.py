"""vd_bvh_build_lbvh*: the LBVH bottom level on the GPU against the numpy restatement of tests/blas_lbvh_cases.py (built top-down
by another algorithm) byte for byte, one large mesh by vectorised invariants, every consumer of a BLAS over the array, and the
build replayed from a HIP graph."""
import os

import numpy as np
import pytest

import blas_lbvh_cases as cases
from blas_refit_cases import deform, refit_reference
from conftest import GOLDEN, fields_equal, first_difference, golden
from voidin_amd import abi, synth
from voidin_amd.obj import ObjModel
from voidin_amd.runtime import VoidinError
from wide_scenes import disjoint_instances, first_bad, grid_rays, mesh_set, records_equal

pytestmark = pytest.mark.gpu

SOUP_SIZES = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097]
NAMED = ["knot", "sphere", "cube_obj", "plane", "helmet"] + sorted(cases.special_cases())
_refs = {}


def _input(name):
    if isinstance(name, int):
        return synth.triangle_soup(name, seed=synth.SEED_BASE + 300 + name)
    if name in ("knot", "sphere"):
        return getattr(cases, name)()
    if name == "bad_index":
        return cases.bad_index_case()
    if name == "cube_obj":
        return ObjModel.load(os.path.join(GOLDEN, "cube.obj"))[0].arrays()
    if name in ("plane", "helmet"):
        g = golden({"plane": "blas_plane.npz", "helmet": "helmet.npz"}[name])
        return g["vertices"], g["indices"]
    return cases.special_cases()[name]


def _reference(name):
    """The restatement of one input, computed once and shared."""
    if name not in _refs:
        v, i = _input(name)
        r = cases.lbvh_reference(v, i)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[name] = (np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(i, dtype=np.uint32), r)
    return _refs[name]


def _build_dev(ctx, v, i, fill=0xCD, d_nodes=None):
    """-> (node bytes of the whole capacity max(2, 2T), index array, result record)."""
    import torch
    T = len(i) // 3
    cap = max(2, 2 * T)
    d_v, d_i = ctx.upload(v), ctx.upload(i)
    d_n = torch.full((cap * 32,), fill, dtype=torch.uint8, device="cuda")
    d_r = torch.full((16,), 0xEE, dtype=torch.uint8, device="cuda")
    ctx.bvh_build_lbvh_dev(d_v, len(v), d_i, T, d_n, cap, d_r)
    torch.cuda.synchronize()
    res = d_r.cpu().numpy().view(abi.BVH_LBVH_RESULT)[0]
    return d_n.cpu().numpy(), d_i.cpu().numpy()[: 12 * T].view(np.uint32), res


def _check_against_restatement(ctx, name):
    v, i, r = _reference(name)
    raw, idx, res = _build_dev(ctx, v, i)
    n = int(res["n_nodes"])
    assert (n, int(res["max_depth"]), int(res["n_bad_indices"]), int(res["_pad"])) == (r["n_nodes"], r["max_depth"], r["n_bad_indices"], 0)
    got = raw[: n * 32].view(abi.BVH_NODE)
    assert fields_equal(got, r["nodes"]), first_difference(got, r["nodes"])
    assert np.array_equal(idx, r["indices"])
    assert (raw[n * 32:] == 0xCD).all(), "bytes past n_nodes were written"
    raw2, idx2, res2 = _build_dev(ctx, v, i, fill=0x11)
    assert raw2[: n * 32].tobytes() == raw[: n * 32].tobytes() and idx2.tobytes() == idx.tobytes() and res2.tobytes() == res.tobytes(), "two builds differ"
    return got, idx


@pytest.mark.parametrize("T", SOUP_SIZES)
def test_soup_equals_the_restatement(ctx, T):
    v, i, r = _reference(T)
    got, idx = _check_against_restatement(ctx, T)
    nodes_h, idx_h = ctx.bvh_build_lbvh(v, i)                          # the host-pointer form: the same bytes
    assert nodes_h.tobytes() == got.tobytes() and np.array_equal(idx_h, idx)


@pytest.mark.parametrize("T", [65_536, 65_537])
def test_soup_at_the_edge_of_the_scan_in_parts(ctx, T):
    """65 536 triangles are the last size whose digit table (256 counters per 1 024 pairs: 16 384) one workgroup scans as a whole;
    65 537 is the first that is scanned in parts of 1 024 counters, the last part a quarter full."""
    _check_against_restatement(ctx, T)


@pytest.mark.parametrize("name", NAMED)
def test_mesh_equals_the_restatement(ctx, name):
    _check_against_restatement(ctx, name)


def test_bad_index_is_counted_and_the_host_form_refuses(ctx):
    v, i, r = _reference("bad_index")
    assert r["n_bad_indices"] == 2
    _check_against_restatement(ctx, "bad_index")                       # the bytes: that corner is a NaN vertex
    with pytest.raises(VoidinError) as e:
        ctx.bvh_build_lbvh(v, i)
    assert e.value.code == abi.VD_ERR_INVALID_ARG, e.value                # not a HIP error: the build ran and counted
    fake = 1 << 20
    lib = ctx.lib
    assert lib.vd_bvh_build_lbvh_dev(ctx.h, fake, 3, fake, 0, fake, 2, fake) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_build_lbvh_dev(ctx.h, fake, 3, fake, 5, fake, 9, fake) == abi.VD_ERR_INVALID_ARG            # node_cap < 2 T
    assert lib.vd_bvh_build_lbvh_dev(ctx.h, fake, 3, fake, 1, fake, 1, fake) == abi.VD_ERR_INVALID_ARG            # node_cap < 2
    assert lib.vd_bvh_build_lbvh_dev(ctx.h, fake, 3, fake, abi.BVH_LBVH_MAX_TRIANGLES + 1, fake, 0xffffffff, fake) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_build_lbvh_dev(ctx.h, fake, 3, fake, 1, fake + 8, 2, fake) == abi.VD_ERR_INVALID_ARG         # nodes not 16-byte aligned
    for hole in range(4):
        args = [fake, 3, fake, 1, fake, 2, fake]
        args[(0, 2, 4, 6)[hole]] = None
        assert lib.vd_bvh_build_lbvh_dev(ctx.h, *args) == abi.VD_ERR_INVALID_ARG


def _levels(nodes):
    """Node ids level by level from node 0 (vectorised per level)."""
    out, cur = [], np.array([0], dtype=np.int64)
    while len(cur):
        out.append(cur)
        inner = cur[nodes["count"][cur] == 0]
        lf = nodes["left_first"][inner].astype(np.int64)
        cur = np.concatenate([lf, lf + 1])
    return out


def test_large_mesh_by_invariants(ctx):
    """2 097 153 triangles: one past the LARGEST boundary of the kernels a build runs - the extent fold's grid stops growing at
    1 024 blocks of 2 048 elements = 2 097 152 (tlas.hip: kExtentBlocks * kExtentPerBlock), beyond which its blocks take a second
    grid-stride round.  2 097 152 is also a multiple of the 256-thread blocks of blas_lbvh.hip, of the sort's 1 024-pair unit and
    of its 4-wave block, so the last block, unit and sort block hold ONE element, and the digit table (256 counters per unit:
    524 544) is scanned in 513 parts of 1 024, the last a quarter full.  (The other boundary, the scan in parts from 65 537
    elements on, is test_soup_at_the_edge_of_the_scan_in_parts.)"""
    import torch
    v, i = synth.knot_mesh(1024, 1024)
    i = np.concatenate([i, i[:3]])
    T = len(i) // 3
    assert T == 2_097_153
    raw, idx, res = _build_dev(ctx, v, i)
    n = int(res["n_nodes"])
    nodes = raw[: n * 32].view(abi.BVH_NODE)
    assert (raw[n * 32:] == 0xCD).all() and int(res["n_bad_indices"]) == 0
    # the indices are the stable code-sorted input
    bmin, bmax, _ = cases.triangle_boxes(v, i)
    codes = cases.codes_of_boxes(bmin, bmax)
    order = np.argsort(codes, kind="stable")
    assert np.array_equal(idx.reshape(-1, 3), i.reshape(-1, 3)[order])
    keys = (codes[order].astype(np.uint64) << np.uint64(32)) | np.arange(T, dtype=np.uint64)
    # child ids are greater than parent ids, siblings adjacent, every pair 2, 4, 6, ... used once, node 1 all-zero
    ids = np.arange(n, dtype=np.int64)
    interior = (nodes["count"] == 0) & (ids != 1)
    lf = nodes["left_first"].astype(np.int64)
    assert nodes[1].tobytes() == bytes(32) and n == 2 + 2 * int(interior.sum())
    assert (lf[interior] > ids[interior]).all() and np.array_equal(np.sort(lf[interior]), np.arange(2, n, 2))
    # ranges, interior counts bottom-up, level by level: the leaves tile [0, T) in pre-order with counts 1..3
    levels = _levels(nodes)
    assert len(levels) - 1 == int(res["max_depth"]) and sum(len(l) for l in levels) == n - 1
    lo, hi, cnt = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    leaf = ~interior & (ids != 1)
    assert ((nodes["count"][leaf] >= 1) & (nodes["count"][leaf] <= 3)).all()
    lo[leaf], hi[leaf] = lf[leaf], lf[leaf] + nodes["count"][leaf].astype(np.int64) - 1
    for lev in reversed(levels):
        k = lev[interior[lev]]
        assert (hi[lf[k]] + 1 == lo[lf[k] + 1]).all()                    # left before right, no gap
        lo[k], hi[k], cnt[k] = lo[lf[k]], hi[lf[k] + 1], 1 + cnt[lf[k]] + cnt[lf[k] + 1]
    assert lo[0] == 0 and hi[0] == T - 1
    k = ids[interior]
    assert (hi[k] - lo[k] >= 3).all()                                    # a node of <= 3 positions is a leaf
    # the reference's numbering: the left child's pair follows its parent's, the right child's follows the whole left subtree
    L, R = lf[k], lf[k] + 1
    assert (lf[L][interior[L]] == (lf[k] + 2)[interior[L]]).all()
    assert (lf[R][interior[R]] == (lf[k] + 2 + 2 * cnt[L])[interior[R]]).all()
    # the split rule on a seeded sample: the right child starts at the first key with the highest bit in which the end keys differ
    for x in np.random.default_rng(20).choice(k, size=2000, replace=False):
        a, s = int(keys[lo[x]]), int(lo[lf[x] + 1])
        b = (a ^ int(keys[hi[x]])).bit_length() - 1
        assert (int(keys[s - 1]) >> b) & 1 == 0 and (int(keys[s]) >> b) & 1 == 1 and lo[x] < s <= hi[x]
    # refit equality: vd_bvh_refit_planned_dev over the array changes no byte
    d_v, d_i, d_n = ctx.upload(v), ctx.upload(idx), ctx.upload(nodes)
    items = (abi.BvhRefitItem * 1)()
    items[0].verts_xyz, items[0].indices, items[0].nodes, items[0].mesh_info = abi.ptr(d_v), abi.ptr(d_i), abi.ptr(d_n), None
    items[0].n_vert, items[0].n_tri, items[0].n_nodes = len(v), T, n
    plan = ctx.bvh_refit_plan(items)
    ctx.bvh_refit_planned(plan)
    torch.cuda.synchronize()
    assert d_n.cpu().numpy()[: n * 32].tobytes() == nodes.tobytes()
    plan.close()


def test_refit_takes_the_array(ctx):
    """vd_bvh_refit_plan_dev accepts the LBVH array; a refit of the unmoved mesh changes no byte; after a deformation it equals
    refit_reference."""
    import torch
    v, i, r = _reference("knot")
    nodes, idx = ctx.bvh_build_lbvh(v, i)
    assert fields_equal(nodes, r["nodes"])
    d_v, d_i, d_n = ctx.upload(v), ctx.upload(idx), ctx.upload(nodes)
    items = (abi.BvhRefitItem * 1)()
    items[0].verts_xyz, items[0].indices, items[0].nodes, items[0].mesh_info = abi.ptr(d_v), abi.ptr(d_i), abi.ptr(d_n), None
    items[0].n_vert, items[0].n_tri, items[0].n_nodes = len(v), len(idx) // 3, len(nodes)
    plan = ctx.bvh_refit_plan(items)
    assert items[0].status == 0
    ctx.bvh_refit_planned(plan); torch.cuda.synchronize()
    assert d_n.cpu().numpy()[: len(nodes) * 32].tobytes() == nodes.tobytes(), "a refit changed an LBVH array"
    v2 = deform(v, phase=0.3)
    d_v.copy_(ctx.upload(v2))
    ctx.bvh_refit_planned(plan); torch.cuda.synchronize()
    got, want = d_n.cpu().numpy()[: len(nodes) * 32].view(abi.BVH_NODE), refit_reference(v2, idx, nodes)
    assert fields_equal(got, want), first_difference(got, want)
    assert not fields_equal(want, nodes)
    plan.close()


@pytest.fixture(scope="module")
def scenes(oracle):
    """Per mesh, computed once: the scene of the CPU test (27 disjoint instances, 40 000 rays) over the exact bottom level."""
    made = {}

    def get(mesh):
        if mesh not in made:
            v, i, r = _reference(mesh)
            infos, B, V, I = mesh_set(oracle, [(v, i)])
            inst, side = disjoint_instances(27, 5)
            made[mesh] = (infos, B, V, I, inst, oracle.tlas_build(inst, infos), grid_rays(40_000, side, 7))
        return made[mesh]
    return get


@pytest.mark.parametrize("mesh", ["knot", "sphere"])
def test_trace_over_the_lbvh_bottom_level(ctx, oracle, scenes, mesh):
    """vd_trace_dev, vd_trace_prepared_dev and vd_trace_any_dev over the GPU-built LBVH array == the oracle over the same arrays in all
    four record fields; vd_trace_dev's hit flags and distance bits == those of the exact-BLAS scene (inputs verified for that in
    tests/test_blas_lbvh_cases.py)."""
    import torch
    v, i, r = _reference(mesh)
    infos, B, V, I, inst, tl, rays = scenes(mesh)
    nodes, idx = ctx.bvh_build_lbvh(v, i)
    assert fields_equal(nodes, r["nodes"])
    arrays = (tl, inst, infos, nodes, V, idx)
    want, _ = oracle.trace(arrays, rays, threads=16)
    assert want["hit"].sum() > 1000 and (want["hit"] == 0).any()
    n = len(rays)
    d_rays = ctx.upload(rays)
    ds = ctx.device_scene(arrays)
    d_h, d_p = ctx.empty(n * 16), ctx.empty(n * 16)
    d_any = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.trace_dev(ds, d_rays, n, d_h)
    ctx.trace_any_dev(ds, d_rays, n, d_any)
    accel = ctx.trace_prepare(ds)                                      # vd_trace_prepare_dev validates the BLAS it is given
    ctx.trace_prepared_dev(accel, d_rays, n, d_p)
    torch.cuda.synchronize()
    got = d_h.cpu().numpy()[: n * 16].view(abi.HIT)
    got_p = d_p.cpu().numpy()[: n * 16].view(abi.HIT)
    assert records_equal(got, want), first_bad(got, want)
    assert records_equal(got_p, want), first_bad(got_p, want)
    assert np.array_equal(d_any.cpu().numpy().astype(np.uint32), want["hit"])
    accel.close()
    d_e = ctx.empty(n * 16)
    ctx.trace_dev(ctx.device_scene((tl, inst, infos, B, V, I)), d_rays, n, d_e)
    torch.cuda.synchronize()
    exact = d_e.cpu().numpy()[: n * 16].view(abi.HIT)
    assert np.array_equal(exact["hit"], got["hit"]) and np.array_equal(exact["dist"].view(np.uint32), got["dist"].view(np.uint32))


def test_traverse_iter_over_the_lbvh_array(ctx, oracle):
    import torch
    v, i, r = _reference("knot")
    nodes, idx = ctx.bvh_build_lbvh(v, i)
    rng = np.random.default_rng(31)
    n = 8192
    o = rng.normal(size=(n, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * 3.0
    t = (rng.random((n, 3)) - 0.5) * 1.2
    rays = np.zeros(n, dtype=abi.RAY)
    rays["eye"], rays["dir"] = o, (t - o) / np.linalg.norm(t - o, axis=1, keepdims=True)
    want = oracle.traverse_iter(nodes, v, idx, rays)
    assert (want >= 0).sum() > n // 8 and (want < 0).any()
    d_out = ctx.empty(n * 4)
    ctx.traverse_iter_dev(ctx.upload(nodes), len(nodes), ctx.upload(v), ctx.upload(idx), ctx.upload(rays), n, d_out)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy()[: n * 4].view(np.float32).tobytes() == want.tobytes()


def test_rebuild_from_a_hip_graph(ctx):
    """A 4 096-triangle build captured into a HIP graph after one uncaptured warm-up call (which sizes the context's work memory: the
    captured call then only enqueues).  Everything goes to the ONE stream of the context, so the graph is a single chain.  Three
    replays with vertices AND indices rewritten in place between them; each equals an uncaptured build of that frame's mesh."""
    import torch
    T = 4096
    cap = 2 * T
    v0, i0 = synth.triangle_soup(T, seed=synth.SEED_BASE + 400)
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
    seen = set()
    rng = np.random.default_rng(41)
    for f in range(3):
        v = deform(v0, phase=0.5 * (f + 1), specials=False)
        i = i0.reshape(-1, 3)[rng.permutation(T)][:, [1, 2, 0]].reshape(-1).copy()       # other triangles in other places, corners rotated
        d_v.copy_(ctx.upload(v)); d_i[: 12 * T].copy_(ctx.upload(i)[: 12 * T])
        d_n.fill_(0xCD)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        raw, idx, res = _build_dev(ctx, v, i)
        n = int(res["n_nodes"])
        assert d_r.cpu().numpy().tobytes() == res.tobytes()
        got = d_n.cpu().numpy()
        assert got[: n * 32].tobytes() == raw[: n * 32].tobytes() and (got[n * 32:] == 0xCD).all()
        assert d_i.cpu().numpy()[: 12 * T].tobytes() == idx.tobytes()
        seen.add(got[: n * 32].tobytes())
    assert len(seen) == 3                                # three different frames
