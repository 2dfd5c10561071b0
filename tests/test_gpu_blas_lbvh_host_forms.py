"""The host side of the LBVH bottom level and the BLAS refit (voidin_amd/csrc/blas_lbvh.hip, blas_refit.hip): vd_bvh_build_lbvh_batch
and vd_bvh_refit stage in the one arena every host-pointer form shares (vd_stage_blobs), write nothing but what they report, and a
refusal - by the host form, by the refit plan, by the LBVH plan - leaves the context usable.

This file was first run unchanged against a build of the commit BEFORE these two host forms moved onto the shared staging
(profiles/blas_lbvh_host_layer.md, section 4): it passed there as it does here."""
import ctypes as C

import numpy as np

import blas_lbvh_cases as cases
import test_gpu_blas_host_forms as sah
from blas_refit_cases import deform, mesh_bounds_reference, refit_reference
from conftest import fields_equal
from voidin_amd import abi, synth
from voidin_amd.runtime import Context

pytestmark = sah.pytestmark

FILL = sah.FILL
_refs = {}


def soup(n_tri, seed_off=0):
    v, i = synth.triangle_soup(n_tri, seed=synth.SEED_BASE + 700 + n_tri + seed_off)
    return np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(i, dtype=np.uint32).reshape(-1)


def lbvh_want(n_tri, T=None, seed_off=0):
    """The restatement's tree of the first T triangles of soup(n_tri): computed once, shared, never written to."""
    T = n_tri if T is None else T
    if (n_tri, T, seed_off) not in _refs:
        v, i = soup(n_tri, seed_off)
        r = cases.lbvh_reference(v, i[: 3 * T])
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[(n_tri, T, seed_off)] = r
    return _refs[(n_tri, T, seed_off)]


def filled_info():
    a = np.zeros(1, dtype=abi.MESH_INFO)
    a.view(np.uint8)[:] = FILL
    return a


class HostBatch:
    """Meshes as VdBvhLbvhBatchItems with host arrays: node arrays and VdMeshInfos prefilled, the indices as they came."""

    def __init__(self, c, meshes, counts=None, with_info=()):
        self.c, self.meshes, self.K = c, meshes, len(meshes)
        self.items = (abi.BvhLbvhBatchItem * self.K)()
        self.idx = [i.copy() for _, i in meshes]
        self.nodes = [sah.filled(max(2, 2 * (len(i) // 3)) + 3) for _, i in meshes]
        self.infos = [filled_info() if m in with_info else None for m in range(self.K)]
        for m, (v, i) in enumerate(meshes):
            it = self.items[m]
            it.verts_xyz, it.indices_inout, it.nodes = v.ctypes.data, self.idx[m].ctypes.data, self.nodes[m].ctypes.data
            it.mesh_info = None if self.infos[m] is None else self.infos[m].ctypes.data
            it.n_vert, it.tri_cap, it.node_cap, it.status = len(v), len(i) // 3, len(self.nodes[m]), 0x7777
        self.counts = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
        self.results = np.zeros(self.K, dtype=abi.BVH_LBVH_RESULT)
        self.results.view(np.uint8)[:] = FILL

    def run(self):
        return self.c.lib.vd_bvh_build_lbvh_batch(self.c.h, C.addressof(self.items), self.K, None if self.counts is None else self.counts.ctypes.data,
                                                  self.results.ctypes.data)

    def outputs_untouched(self):
        infos_ok = all(f is None or sah.untouched(f) for f in self.infos)
        return infos_ok and all(sah.untouched(n) for n in self.nodes) and all(np.array_equal(a, i) for a, (_, i) in zip(self.idx, self.meshes))

    def check(self, want):
        """Item m is want[m] = the restatement of its first T_m triangles (None: T_m == 0); nothing behind n_nodes nodes or 3 T_m
        indices is written; a VdMeshInfo has the bounds of ALL the mesh's vertices and its other fields as they were."""
        for m, r in enumerate(want):
            (v, i), res, nodes = self.meshes[m], self.results[m], self.nodes[m]
            assert self.items[m].status == abi.VD_OK
            if r is None:
                assert res.tobytes() == bytes(16) and sah.untouched(nodes) and np.array_equal(self.idx[m], i), f"item {m}: T == 0"
            else:
                n, T = r["n_nodes"], len(r["indices"]) // 3
                assert (int(res["n_nodes"]), int(res["max_depth"]), int(res["n_bad_indices"]), int(res["_pad"])) == (n, r["max_depth"], 0, 0), f"item {m}"
                assert fields_equal(nodes[:n], r["nodes"]) and sah.untouched(nodes[n:]), f"item {m}: nodes"
                assert np.array_equal(self.idx[m][: 3 * T], r["indices"]) and np.array_equal(self.idx[m][3 * T:], i[3 * T:]), f"item {m}: indices"
            if self.infos[m] is not None:
                lo, hi = mesh_bounds_reference(v)
                f = self.infos[m]
                assert f["min"][0].tobytes() == lo.tobytes() and f["max"][0].tobytes() == hi.tobytes(), f"item {m}: bounds"
                assert all(sah.untouched(f[k]) for k in ("index_count", "base_index", "vertex_offset", "bvh_index", "junk")), f"item {m}: VdMeshInfo"


def good_batch(c, extra=None, seed_off=0):
    """1, 3, 4, 256, 257 and 700 triangles, a mesh whose count is 0 and one whose count is above its capacity, three with a
    VdMeshInfo; `extra`: one more mesh of that many triangles, built from half of them."""
    sizes = [1, 3, 4, 256, 257, 700, 5, 64] + ([extra] if extra else [])
    counts = [1, 3, 4, 256, 257, 700, 0, 1000] + ([extra // 2] if extra else [])
    b = HostBatch(c, [soup(n, seed_off) for n in sizes], counts, with_info=(2, 6, 7))
    assert b.run() == abi.VD_OK, c.lib.vd_last_error(c.h)
    b.check([None if t == 0 else lbvh_want(n, min(t, n), seed_off) for n, t in zip(sizes, counts)])


def good_refit(c, n_tri, seed_off=0):
    """vd_bvh_refit of the restatement's tree over deformed vertices; the reserved slot 1 holds the fill and keeps it."""
    v, _ = soup(n_tri, seed_off)
    r = lbvh_want(n_tri, None, seed_off)
    moved = deform(v, phase=0.4)
    nodes = r["nodes"].copy()
    nodes[1:2].view(np.uint8)[:] = FILL
    want = refit_reference(moved, r["indices"], nodes)
    idx = r["indices"].copy()
    rc = c.lib.vd_bvh_refit(c.h, moved.ctypes.data, len(moved), idx.ctypes.data, n_tri, nodes.ctypes.data, len(nodes))
    assert rc == abi.VD_OK, c.lib.vd_last_error(c.h)
    assert fields_equal(nodes, want) and sah.untouched(nodes[1:2]) and np.array_equal(idx, r["indices"]), f"refit of {n_tri} triangles"


def good_lbvh(c, n_tri, seed_off=0):
    v, i = soup(n_tri, seed_off)
    r = lbvh_want(n_tri, None, seed_off)
    idx, nodes, n = i.copy(), sah.filled(2 * n_tri + 3), C.c_uint32(0)
    rc = c.lib.vd_bvh_build_lbvh(c.h, v.ctypes.data, len(v), idx.ctypes.data, n_tri, nodes.ctypes.data, len(nodes), C.addressof(n))
    assert rc == abi.VD_OK, c.lib.vd_last_error(c.h)
    assert n.value == r["n_nodes"] and fields_equal(nodes[: n.value], r["nodes"]) and sah.untouched(nodes[n.value:]), f"LBVH of {n_tri} triangles"
    assert np.array_equal(idx, r["indices"])


def test_the_lbvh_and_refit_host_forms_share_the_arena(oracle):
    """One fresh context: the SAH build, the LBVH batch, the refit and the single LBVH build one after the other, then in another
    order with other and larger inputs - each call finds the arena in the layout another form left and has to grow it.  Every
    result is its reference's bit for bit, and no output byte that the call does not report is written."""
    c = Context(0)
    try:
        sah.good_build(c, oracle, 513)
        good_batch(c)
        good_refit(c, 700)
        good_lbvh(c, 513)
        good_lbvh(c, 1500, seed_off=1)                    # 168 KB of staging, 336 KB, 1 MB, 1.4 MB: the arena doubles at each
        good_refit(c, 3000, seed_off=1)
        sah.good_build(c, oracle, 9000)
        good_batch(c, extra=12000, seed_off=1)
        good_refit(c, 257)
        good_batch(c)
    finally:
        c.close()


def test_a_refusal_leaves_the_context_usable():
    c = Context(0)
    try:
        import torch
        err = lambda: c.lib.vd_last_error(c.h)
        # an index >= n_vert in item 1 of 3, through the host batch: named by status and text, nothing is copied back
        meshes = [soup(257), soup(700), soup(4)]
        bad = meshes[1][1].copy(); bad[3 * 301 + 2] = len(meshes[1][0])
        b = HostBatch(c, [meshes[0], (meshes[1][0], bad), meshes[2]], with_info=(0, 1))
        assert b.run() == abi.VD_ERR_INVALID_ARG
        assert err() == b"vd_bvh_lbvh_plan: item 1: an index >= n_vert"
        assert [it.status for it in b.items] == [abi.VD_OK, abi.VD_ERR_INVALID_ARG, abi.VD_OK]
        assert b.outputs_untouched()
        good_batch(c)
        # a node with two parents, through vd_bvh_refit: node 3 is a child of node 0 and of node 2
        v, i = soup(2)
        nodes = np.zeros(5, dtype=abi.BVH_NODE)
        nodes["left_first"], nodes["count"] = [2, 0, 3, 0, 1], [0, 0, 0, 1, 1]
        nodes["min"], nodes["max"] = 7.0, -7.0
        before = nodes.copy()
        rc = c.lib.vd_bvh_refit(c.h, v.ctypes.data, len(v), i.ctypes.data, 2, nodes.ctypes.data, len(nodes))
        assert rc == abi.VD_ERR_INVALID_ARG and err() == b"vd_bvh_refit_plan: item 0: a node has two parents"
        assert nodes.tobytes() == before.tobytes()
        good_refit(c, 700)
        # a bad middle item through vd_bvh_lbvh_plan_dev, on a live context: no plan is returned
        keep = []
        items = (abi.BvhLbvhBatchItem * 3)()
        for m, n_tri in enumerate((257, 700, 4)):
            v, i = soup(n_tri)
            d_v, d_i = c.upload(v), c.upload(i)
            d_n = torch.full((2 * n_tri * sah.NODE,), FILL, dtype=torch.uint8, device=c.torch_device)
            keep.append((d_v, d_i, d_n))
            items[m].verts_xyz, items[m].indices_inout, items[m].nodes = abi.ptr(d_v), abi.ptr(d_i), abi.ptr(d_n)
            items[m].n_vert, items[m].tri_cap, items[m].node_cap, items[m].status = len(v), n_tri, 2 * n_tri, 0x7777
        items[1].node_cap = 2 * 700 - 1
        h = C.c_void_p(0x7777)
        rc = c.lib.vd_bvh_lbvh_plan_dev(c.h, C.addressof(items), 3, C.byref(h))
        assert rc == abi.VD_ERR_INVALID_ARG and not h.value
        assert err() == b"vd_bvh_lbvh_plan: item 1: node_cap < max(2, 2 * tri_cap)"
        assert [it.status for it in items] == [abi.VD_OK, abi.VD_ERR_INVALID_ARG, abi.VD_OK]
        torch.cuda.synchronize()
        assert all(bool((d_n == FILL).all()) for _, _, d_n in keep)
        items[1].node_cap = 2 * 700
        plan = c.bvh_lbvh_plan(items)
        d_res = torch.full((16 * 3,), FILL, dtype=torch.uint8, device=c.torch_device)
        plan.build(None, d_res)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(abi.BVH_LBVH_RESULT)
        for m, n_tri in enumerate((257, 700, 4)):
            r = lbvh_want(n_tri)
            got = keep[m][2].cpu().numpy().view(abi.BVH_NODE)
            assert int(res[m]["n_nodes"]) == r["n_nodes"] and fields_equal(got[: r["n_nodes"]], r["nodes"]) and sah.untouched(got[r["n_nodes"]:])
            assert np.array_equal(keep[m][1].cpu().numpy().view(np.uint32), r["indices"])
        plan.close()
        good_batch(c)
    finally:
        c.close()
