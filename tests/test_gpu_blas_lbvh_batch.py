"""vd_bvh_lbvh_plan_dev / vd_bvh_build_lbvh_planned_dev / vd_bvh_build_lbvh_batch: many meshes built by one call, every triangle
count read on the device.  Each mesh's nodes, indices and result must be byte for byte what the single build gives for it alone:
checked against the numpy restatement of tests/blas_lbvh_cases.py for small meshes in one plan, against vd_bvh_build_lbvh_dev for
larger ones, and through replays of ONE captured call while the counts change in device memory."""
import ctypes as C

import numpy as np
import pytest

import blas_lbvh_cases as cases
from blas_refit_cases import mesh_bounds_reference
from conftest import fields_equal, first_difference
from voidin_amd import abi, synth
from voidin_amd.runtime import VoidinError

pytestmark = pytest.mark.gpu

CANARY = 0xCD
# small meshes between large ones: with 256 slots per unit a mesh's slots end inside a sort block of four units, and seams
# between meshes fall everywhere in those blocks
SOUPS = [1024, 1, 257, 2, 1023, 3, 64, 4, 1025, 5, 255, 7, 63, 8, 256, 65]
_refs = {}


def _input(name):
    if isinstance(name, int):
        return synth.triangle_soup(name, seed=synth.SEED_BASE + 500 + name)
    if name == "bad_index":
        return cases.bad_index_case()
    return cases.special_cases()[name]


def _reference(name):
    """The restatement of one input, computed once and shared, never written."""
    if name not in _refs:
        v, i = _input(name)
        r = cases.lbvh_reference(v, i)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[name] = (np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(i, dtype=np.uint32).reshape(-1), r)
    return _refs[name]


def _restatement_set():
    specials = sorted(cases.special_cases())
    names = list(SOUPS)
    for k, s in enumerate(specials):                       # the special meshes and the bad-index one between the soups
        names.insert(2 * k + 1, s)
    names.insert(len(names) // 2, "bad_index")
    return names


class Batch:
    """K meshes on the device with one plan over them.  Node and index buffers hold the canary wherever nothing was put."""

    def __init__(self, ctx, meshes, infos=None):
        import torch
        self.ctx, self.meshes, self.K = ctx, meshes, len(meshes)
        self.caps = [len(i) // 3 for _, i in meshes]
        self.d_v = [ctx.upload(np.ascontiguousarray(v, dtype=np.float32)) for v, _ in meshes]
        self.d_i = [torch.full((12 * c,), CANARY, dtype=torch.uint8, device="cuda") for c in self.caps]
        self.d_n = [torch.full((32 * max(2, 2 * c),), CANARY, dtype=torch.uint8, device="cuda") for c in self.caps]
        self.d_info = [None if infos is None or infos[m] is None else ctx.upload(infos[m]) for m in range(self.K)]
        self.d_res = torch.full((16 * self.K,), 0xEE, dtype=torch.uint8, device="cuda")
        self.d_cnt = torch.zeros((self.K,), dtype=torch.int32, device="cuda")
        self.items = (abi.BvhLbvhBatchItem * self.K)()
        for m, (v, i) in enumerate(meshes):
            it = self.items[m]
            it.verts_xyz, it.indices_inout, it.nodes = abi.ptr(self.d_v[m]), abi.ptr(self.d_i[m]), abi.ptr(self.d_n[m])
            it.mesh_info = None if self.d_info[m] is None else abi.ptr(self.d_info[m])
            it.n_vert, it.tri_cap, it.node_cap = len(v), self.caps[m], max(2, 2 * self.caps[m])
        self.plan = ctx.bvh_lbvh_plan(self.items)
        assert all(it.status == 0 for it in self.items)

    def load(self, counts):
        """Canary everywhere, then the first T_m triangles of every mesh as they came; the counts as given (unclamped)."""
        import torch
        for m, (_, i) in enumerate(self.meshes):
            T = min(int(counts[m]), self.caps[m])
            self.d_i[m].fill_(CANARY)
            if T:
                self.d_i[m][: 12 * T].copy_(torch.from_numpy(np.ascontiguousarray(i[: 3 * T], dtype=np.uint32).view(np.uint8)))
            self.d_n[m].fill_(CANARY)
        self.d_res.fill_(0xEE)
        self.d_cnt.copy_(torch.from_numpy(np.asarray(counts, dtype=np.uint32).view(np.int32)))
        torch.cuda.synchronize()

    def build(self, with_counts=True):
        import torch
        self.ctx.bvh_build_lbvh_planned_dev(self.plan, self.d_cnt if with_counts else None, self.d_res)
        torch.cuda.synchronize()

    def fetch(self):
        """-> per mesh (node bytes of the whole capacity, index words of the whole capacity, result record)."""
        res = self.d_res.cpu().numpy().view(abi.BVH_LBVH_RESULT)
        return [(self.d_n[m].cpu().numpy(), self.d_i[m].cpu().numpy().view(np.uint32), res[m]) for m in range(self.K)]

    def close(self):
        self.plan.close()


def _single(ctx, v, i, T):
    """vd_bvh_build_lbvh_dev of the first T triangles alone -> (node bytes [: n_nodes], index words, result bytes)."""
    import torch
    cap = max(2, 2 * T)
    d_v, d_i = ctx.upload(np.ascontiguousarray(v, dtype=np.float32)), ctx.upload(np.ascontiguousarray(i[: 3 * T], dtype=np.uint32))
    d_n = torch.full((cap * 32,), 0x11, dtype=torch.uint8, device="cuda")
    d_r = torch.full((16,), 0xEE, dtype=torch.uint8, device="cuda")
    ctx.bvh_build_lbvh_dev(d_v, len(v), d_i, T, d_n, cap, d_r)
    torch.cuda.synchronize()
    res = d_r.cpu().numpy()
    n = int(res.view(abi.BVH_LBVH_RESULT)[0]["n_nodes"])
    return d_n.cpu().numpy()[: 32 * n].tobytes(), d_i.cpu().numpy()[: 12 * T].tobytes(), res.tobytes()


def _expect_equals_single(ctx, got, v, i, count, cap, memo=None, key=None):
    """One item after a build with `count` == the single build of its first min(count, cap) triangles; canaries elsewhere."""
    raw, idx, res = got
    T = min(int(count), cap)
    if T == 0:
        assert res.tobytes() == bytes(16), "T == 0: the result is all zero"
        assert (raw == CANARY).all() and (idx.view(np.uint8) == CANARY).all(), "T == 0: nothing is written"
        return
    if memo is not None and (key, T) in memo:
        want = memo[(key, T)]
    else:
        want = _single(ctx, v, i, T)
        if memo is not None:
            memo[(key, T)] = want
    n = int(res["n_nodes"])
    assert res.tobytes() == want[2], (key, T, res)
    assert raw[: 32 * n].tobytes() == want[0], (key, T)
    assert idx[: 3 * T].tobytes() == want[1], (key, T)
    assert (raw[32 * n:] == CANARY).all(), "bytes past n_nodes were written"
    assert (idx[3 * T:].view(np.uint8) == CANARY).all(), "indices past 3 T were written"


def _check_against_restatement(name, raw, idx, res):
    v, i, r = _reference(name)
    n = int(res["n_nodes"])
    assert (n, int(res["max_depth"]), int(res["n_bad_indices"]), int(res["_pad"])) == (r["n_nodes"], r["max_depth"], r["n_bad_indices"], 0), name
    got = np.ascontiguousarray(raw[: n * 32]).view(abi.BVH_NODE)
    assert fields_equal(got, r["nodes"]), (name, first_difference(got, r["nodes"]))
    assert np.array_equal(idx[: len(i)], r["indices"]), name


def test_one_plan_of_small_meshes_equals_the_restatement(ctx):
    names = _restatement_set()
    meshes = [_reference(n)[:2] for n in names]
    b = Batch(ctx, meshes)
    b.load(b.caps)
    b.build(with_counts=False)                               # a null d_n_tri: every tri_cap
    for name, (raw, idx, res) in zip(names, b.fetch()):
        _check_against_restatement(name, raw, idx, res)
        assert (raw[int(res["n_nodes"]) * 32:] == CANARY).all(), f"{name}: bytes past n_nodes were written"
    res = b.d_res.cpu().numpy().view(abi.BVH_LBVH_RESULT)
    bad = [n for n, r in zip(names, res) if r["n_bad_indices"]]
    assert bad == ["bad_index"] and int(res[names.index("bad_index")]["n_bad_indices"]) == 2
    first = [x[0].tobytes() + x[1].tobytes() + x[2].tobytes() for x in b.fetch()]
    b.load(b.caps)
    b.build()                                                # the same through the counts: the same bytes
    assert [x[0].tobytes() + x[1].tobytes() + x[2].tobytes() for x in b.fetch()] == first
    b.close()


def test_larger_batch_equals_the_single_build(ctx):
    """70 meshes of 1 000 triangles (1 024 slots each) and one of 4 097 (4 352 slots): 76 032 slots, past 65 536, and a digit table
    of 76 032 counters, which is scanned in 75 parts of 1 024, the last a quarter full."""
    meshes = [synth.triangle_soup(1000, seed=synth.SEED_BASE + 600 + m) for m in range(70)]
    meshes.insert(35, synth.triangle_soup(4097, seed=synth.SEED_BASE + 699))
    b = Batch(ctx, meshes)
    b.load(b.caps)
    b.build()
    for m, got in enumerate(b.fetch()):
        _expect_equals_single(ctx, got, *meshes[m], b.caps[m], b.caps[m], key=m)
    b.close()


def test_batch_of_exactly_one_mesh(ctx):
    """1 000 triangles: 1 024 slots, four units, one sort block; the digit table is scanned by one workgroup."""
    mesh = synth.triangle_soup(1000, seed=synth.SEED_BASE + 601)
    b = Batch(ctx, [mesh])
    b.load(b.caps)
    b.build()
    _expect_equals_single(ctx, b.fetch()[0], *mesh, 1000, 1000)
    b.close()


def test_counts_on_the_device_through_a_hip_graph(ctx):
    """ONE captured planned call, replayed while d_n_tri is rewritten in device memory between the replays."""
    import torch
    caps = [1, 3, 4, 5, 100, 256, 257, 1000, 2, 600]
    meshes = [synth.triangle_soup(c, seed=synth.SEED_BASE + 700 + c) for c in caps]
    b = Batch(ctx, meshes)
    b.load(caps)
    b.build()                                                # warm-up, uncaptured
    graph = torch.cuda.CUDAGraph()
    main_stream = torch.cuda.current_stream().cuda_stream
    try:
        with torch.cuda.graph(graph):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx.bvh_build_lbvh_planned_dev(b.plan, b.d_cnt, b.d_res)
    finally:
        ctx.set_stream(main_stream)
    mixed = [0, 1, 3, 4, 99, 0, 1, 3, 1, 599]                 # 0 / 1 / 3 / 4 / cap - 1
    assert mixed[4] == caps[4] - 1 and mixed[9] == caps[9] - 1
    above = list(caps)
    above[7] = caps[7] + 12345                                # read as tri_cap
    memo, frames = {}, []
    for counts in (caps, mixed, [0] * len(caps), caps, above):
        b.load(counts)
        graph.replay()
        torch.cuda.synchronize()
        got = b.fetch()
        for m in range(b.K):
            _expect_equals_single(ctx, got[m], *meshes[m], counts[m], caps[m], memo=memo, key=m)
        frames.append(b"".join(x[0].tobytes() + x[1].tobytes() + x[2].tobytes() for x in got))
    assert frames[3] == frames[0], "full again differs from the first full frame: something was left behind by the frames between"
    assert frames[4] == frames[0], "a count above tri_cap is read as tri_cap"
    assert len({frames[0], frames[1], frames[2]}) == 3
    b.close()


def test_mesh_info_bounds(ctx):
    """min / max == the float32 fold over ALL vertices (a NaN vertex ignored, an unreferenced vertex counted), the other 24 bytes
    of the record untouched; items with and without a mesh_info side by side; a mesh of two vertex chunks; a mesh with count 0."""
    v0, i0 = synth.triangle_soup(200, seed=synth.SEED_BASE + 800)
    v0 = np.concatenate([v0, np.float32([[1e6, -1e6, 5e5], [np.nan, np.nan, np.nan]])]).astype(np.float32)      # unreferenced, far outside; a NaN vertex
    v0[7, 1] = np.nan
    v1, i1 = synth.triangle_soup(50, seed=synth.SEED_BASE + 801)
    v2, i2 = synth.triangle_soup(2000, seed=synth.SEED_BASE + 802)                                                # 6 000 vertices: two chunks of 4 096
    assert len(v2) > 4096
    v3, i3 = synth.triangle_soup(30, seed=synth.SEED_BASE + 803)
    meshes = [(v0, i0), (v1, i1), (v2, i2), (v3, i3)]

    def info(seed):
        a = np.frombuffer(np.random.default_rng(seed).bytes(48), dtype=abi.MESH_INFO).copy()
        return a
    infos = [info(1), None, info(2), info(3)]
    b = Batch(ctx, meshes, infos=infos)
    counts = [200, 50, 2000, 0]
    for _ in range(2):                                       # twice: the fold's words are re-armed by the build itself
        b.load(counts)
        b.build()
        for m, (v, i) in enumerate(meshes):
            if infos[m] is None:
                continue
            got = b.d_info[m].cpu().numpy()[:48].view(abi.MESH_INFO)
            lo, hi = mesh_bounds_reference(v)
            assert got["min"][0].tobytes() == lo.tobytes() and got["max"][0].tobytes() == hi.tobytes(), m
            raw, want = got.view(np.uint8), infos[m].view(np.uint8)
            keep = np.r_[12:16, 28:48]
            assert np.array_equal(raw[keep], want[keep]), "a field other than min / max was written"
        for m, got in enumerate(b.fetch()):
            _expect_equals_single(ctx, got, *meshes[m], counts[m], b.caps[m])
    assert float(b.d_info[0].cpu().numpy()[:48].view(abi.MESH_INFO)["max"][0][0]) == 1e6
    b.close()


def test_host_form_equals_the_restatement_and_refuses_a_bad_index(ctx):
    names = [n for n in _restatement_set() if n != "bad_index"]
    out = ctx.bvh_build_lbvh_batch([_reference(n)[:2] for n in names])
    for name, (nodes, idx, res) in zip(names, out):
        _check_against_restatement(name, nodes.view(np.uint8).reshape(-1), idx, res)
    # counts from the host, one of them 0 and one above its capacity
    (va, ia, _), (vb, ib, _), (vc, ic, _) = _reference(64), _reference(257), _reference(5)
    out = ctx.bvh_build_lbvh_batch([(va, ia), (vb, ib), (vc, ic)], n_tri=[64 + 9, 0, 5])
    _check_against_restatement(64, out[0][0].view(np.uint8).reshape(-1), out[0][1], out[0][2])
    assert len(out[1][0]) == 0 and out[1][2].tobytes() == bytes(16) and np.array_equal(out[1][1], ib)
    _check_against_restatement(5, out[2][0].view(np.uint8).reshape(-1), out[2][1], out[2][2])
    with pytest.raises(VoidinError) as e:
        ctx.bvh_build_lbvh_batch([(va, ia), _reference("bad_index")[:2], (vc, ic)])
    assert e.value.code == abi.VD_ERR_INVALID_ARG, e.value
    assert [it.status for it in e.value.items][:3] == [0, abi.VD_ERR_INVALID_ARG, 0]


def test_plan_with_a_live_context(ctx):
    """n_items == 0 is a plan that does nothing; a refused item returns no plan and says why; null plan / results."""
    lib = ctx.lib
    empty = ctx.bvh_lbvh_plan((abi.BvhLbvhBatchItem * 1)(), n_items=0)
    assert empty.h
    assert lib.vd_bvh_build_lbvh_planned_dev(ctx.h, empty.h, None, 1 << 20) == abi.VD_OK
    assert lib.vd_bvh_build_lbvh_planned_dev(ctx.h, empty.h, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_build_lbvh_planned_dev(ctx.h, None, None, 1 << 20) == abi.VD_ERR_INVALID_ARG
    empty.close()
    fake = 1 << 20
    items = (abi.BvhLbvhBatchItem * 2)()
    for it in items:
        it.verts_xyz, it.indices_inout, it.nodes, it.n_vert, it.tri_cap, it.node_cap = fake, fake, fake, 3, 10, 20
    items[1].node_cap = 19
    out = C.c_void_p(0x1234)
    assert lib.vd_bvh_lbvh_plan_dev(ctx.h, C.addressof(items), 2, C.byref(out)) == abi.VD_ERR_INVALID_ARG
    assert out.value is None and [it.status for it in items] == [0, abi.VD_ERR_INVALID_ARG]
    assert b"item 1" in lib.vd_last_error(ctx.h)
