"""The host side of the SAH bottom-level builder (voidin_amd/csrc/blas.hip): vd_bvh_build and vd_bvh_build_batch stage their
meshes in the one arena every host-pointer form shares (vd_stage_blobs), a refusal joins what it queued and leaves the context
usable, and the launches a build makes are a function of its input alone.

The refusal texts and the table of build statistics were taken from the commit BEFORE the host side was cut into stages, by
running this file against a build of it (profiles/blas_host_layer.md, section 3)."""
import ctypes as C

import numpy as np
import pytest

from conftest import fields_equal
from voidin_amd import abi, synth
from voidin_amd.runtime import Context

pytestmark = pytest.mark.gpu

FILL = 0xC3
NODE = abi.BVH_NODE.itemsize
_oracle_trees = {}


def soup(n_tri, seed=None):
    v, i = synth.triangle_soup(n_tri, seed=synth.SEED_BASE + 300 + n_tri if seed is None else seed)
    return np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3), np.asarray(i, dtype=np.uint32).reshape(-1).copy()


def want_tree(oracle, n_tri, seed=None):
    """The oracle's tree of soup(n_tri, seed): computed once, shared, never written to."""
    if (n_tri, seed) not in _oracle_trees:
        nodes, idx = oracle.bvh_build(*soup(n_tri, seed))
        nodes.flags.writeable = False
        idx.flags.writeable = False
        _oracle_trees[(n_tri, seed)] = (nodes, idx)
    return _oracle_trees[(n_tri, seed)]


def filled(n_nodes):
    a = np.zeros(n_nodes, dtype=abi.BVH_NODE)
    a.view(np.uint8)[:] = FILL
    return a


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def host_build(c, v, i):
    """vd_bvh_build into a prefilled array of 2 * n_tri + 3 nodes -> (rc, the whole array, n_nodes, the indices)."""
    idx = i.copy()
    nodes = filled(2 * (len(i) // 3) + 3)
    n = C.c_uint32(0)
    rc = c.lib.vd_bvh_build(c.h, v.ctypes.data, len(v), idx.ctypes.data, len(idx) // 3, nodes.ctypes.data, len(nodes), C.addressof(n))
    return rc, nodes, n.value, idx


def dev_build(c, v, i, node_cap=None):
    """vd_bvh_build_dev likewise, on device buffers."""
    import torch
    d_v, d_i = c.upload(v), c.upload(i)
    cap = 2 * (len(i) // 3) + 3 if node_cap is None else node_cap
    d_n = torch.full((cap * NODE,), FILL, dtype=torch.uint8, device=c.torch_device)
    n = C.c_uint32(0)
    rc = c.lib.vd_bvh_build_dev(c.h, abi.ptr(d_v), len(v), abi.ptr(d_i), len(i) // 3, abi.ptr(d_n), cap, C.addressof(n))
    return rc, d_n.cpu().numpy().view(abi.BVH_NODE), n.value, d_i.cpu().numpy().view(np.uint32)


def good_build(c, oracle, n_tri, seed=None):
    wn, wi = want_tree(oracle, n_tri, seed)
    rc, nodes, n, idx = host_build(c, *soup(n_tri, seed))
    assert rc == abi.VD_OK, c.lib.vd_last_error(c.h)
    assert n == len(wn) and fields_equal(nodes[:n], wn) and np.array_equal(idx, wi), f"{n_tri} triangles"
    assert untouched(nodes[n:]), f"{n_tri} triangles: bytes behind the {n} nodes"


class Batch:
    """Three meshes as VdBvhBatchItems, with host arrays or device buffers, own node arrays or one packed buffer."""

    def __init__(self, c, meshes, packed, device, packed_first=0, packed_cap=None, own_cap=None):
        import torch
        self.c, self.meshes, self.packed, self.device, self.first = c, meshes, packed, device, packed_first
        K = len(meshes)
        self.items = (abi.BvhBatchItem * K)()
        self.keep = []
        for m, (v, i) in enumerate(meshes):
            n_tri = len(i) // 3
            cap = 2 * n_tri + 3 if own_cap is None else own_cap[m]
            if device:
                d_v, d_i = c.upload(v), c.upload(i)
                own = None if packed else torch.full((cap * NODE,), FILL, dtype=torch.uint8, device=c.torch_device)
                ptrs = abi.ptr(d_v), abi.ptr(d_i), None if packed else abi.ptr(own)
                self.keep.append((d_v, d_i, own))
            else:
                idx = i.copy()
                own = None if packed else filled(cap)
                ptrs = v.ctypes.data, idx.ctypes.data, None if packed else own.ctypes.data
                self.keep.append((v, idx, own))
            self.items[m].verts_xyz, self.items[m].indices_inout, self.items[m].out_nodes = ptrs
            self.items[m].n_vert, self.items[m].n_tri, self.items[m].node_cap = len(v), n_tri, 0 if packed else cap
            self.items[m].status, self.items[m].out_n_nodes, self.items[m].out_first_node = 0x7777, 0x7777, 0x7777
        self.cap = (packed_first + sum(2 * (len(i) // 3) + 3 for _, i in meshes) if packed_cap is None else packed_cap) if packed else 0
        if not packed:
            self.shared = None
        elif device:
            self.shared = torch.full((max(self.cap, 1) * NODE,), FILL, dtype=torch.uint8, device=c.torch_device)
        else:
            self.shared = filled(max(self.cap, 1))
        self.end = C.c_uint32(0x7777)

    def run(self):
        fn = self.c.lib.vd_bvh_build_batch_dev if self.device else self.c.lib.vd_bvh_build_batch
        shared = None if not self.packed else (abi.ptr(self.shared) if self.device else self.shared.ctypes.data)
        return fn(self.c.h, C.addressof(self.items), len(self.meshes), shared, self.cap, self.first, C.addressof(self.end))

    def report(self):
        return [(int(it.status), int(it.out_n_nodes), int(it.out_first_node)) for it in self.items], int(self.end.value)

    def nodes(self, m):
        """Mesh m's whole node array (own), or the whole packed buffer."""
        a = self.shared if self.packed else self.keep[m][2]
        return a.cpu().numpy().view(abi.BVH_NODE) if self.device else a

    def indices(self, m):
        return self.keep[m][1].cpu().numpy().view(np.uint32) if self.device else self.keep[m][1]

    def check(self, want):
        """Every mesh equals want[m]; own arrays untouched behind their nodes, the packed buffer outside [first, end)."""
        report, end = self.report()
        at = self.first
        for m, (wn, wi) in enumerate(want):
            assert report[m] == (abi.VD_OK, len(wn), at if self.packed else 0), f"mesh {m}: {report[m]}"
            a = self.nodes(m)
            lo = at if self.packed else 0
            assert fields_equal(a[lo: lo + len(wn)], wn), f"mesh {m}: nodes"
            assert np.array_equal(self.indices(m), wi), f"mesh {m}: indices"
            if self.packed:
                at += len(wn)
            else:
                assert untouched(a[len(wn):]), f"mesh {m}: bytes behind its nodes"
        assert end == at
        if self.packed:
            a = self.nodes(0)
            assert untouched(a[: self.first]) and untouched(a[at:]), "bytes outside the packed range"


def test_the_host_forms_share_the_arena(oracle):
    """One fresh context runs the host forms one after the other - single builds from 3 to 3000 triangles, batches with own
    arrays and packed behind 11 nodes, a top-level build, an LBVH build, then a smaller and a larger single build: the arena
    shrinks in use and grows.  Every result is the oracle's and the _dev form's on a second context, bit for bit; no byte
    behind the nodes in use or outside the packed range is written."""
    a, b = Context(0), Context(0)
    try:
        for n_tri in (3, 513, 2049, 3000):
            wn, wi = want_tree(oracle, n_tri)
            good_build(a, oracle, n_tri)
            rc, nodes, n, idx = dev_build(b, *soup(n_tri))
            assert rc == abi.VD_OK and n == len(wn) and fields_equal(nodes[:n], wn) and np.array_equal(idx, wi) and untouched(nodes[n:])
        meshes = [soup(n) for n in (3, 513, 2049)]
        want = [want_tree(oracle, n) for n in (3, 513, 2049)]
        for packed, first in ((False, 0), (True, 11)):
            for c, device in ((a, False), (b, True)):
                batch = Batch(c, meshes, packed, device, packed_first=first)
                assert batch.run() == abi.VD_OK, c.lib.vd_last_error(c.h)
                batch.check(want)
        infos = synth.mesh_infos()
        inst = synth.instances(500, seed=synth.SEED_BASE + 61, extent=80.0)
        tl = a.tlas_build(inst, infos)
        assert fields_equal(tl, oracle.tlas_build(inst, infos))
        d_tl = b.empty(len(tl) * abi.TLAS_NODE.itemsize)
        b.tlas_build_dev(b.upload(inst), len(inst), b.upload(np.ascontiguousarray(infos, dtype=abi.MESH_INFO)), len(infos), d_tl)
        assert d_tl.cpu().numpy()[: tl.nbytes].tobytes() == tl.tobytes()
        v, i = soup(513)
        ln, li = a.bvh_build_lbvh(v, i)
        d_i, d_n, d_res = b.upload(i), b.empty(2 * 513 * NODE), b.empty(16)
        b.bvh_build_lbvh_dev(b.upload(v), len(v), d_i, 513, d_n, 2 * 513, d_res)
        assert int(d_res.cpu().numpy().view(np.uint32)[0]) == len(ln)
        assert d_n.cpu().numpy()[: ln.nbytes].tobytes() == ln.tobytes() and np.array_equal(d_i.cpu().numpy().view(np.uint32), li)
        good_build(a, oracle, 513)
        good_build(a, oracle, 9000)
        wn, wi = want_tree(oracle, 9000)
        rc, nodes, n, idx = dev_build(b, *soup(9000))
        assert rc == abi.VD_OK and n == len(wn) and fields_equal(nodes[:n], wn) and np.array_equal(idx, wi) and untouched(nodes[n:])
    finally:
        a.close()
        b.close()


DEGENERATE = b"vd_bvh_build: every split candidate rejected (the reference builder crashes on this input)"


def test_a_refusal_leaves_the_context_usable(oracle):
    """Four refusals on one context - found with a level queued ahead, by the precompute, by the room check before the
    copy-out, in the packed buffer - each with its status, its exact text and, for a batch, every item's report as the
    builder always left them; each followed at once by a good build of another mesh."""
    c = Context(0)
    try:
        err = lambda: c.lib.vd_last_error(c.h)
        # an infinite vertex at 5000 triangles: every candidate cost of its node is inf or NaN
        v, i = soup(5000)
        v = v.copy(); v[5, 1] = np.inf
        rc, nodes, n, idx = host_build(c, v, i)
        assert rc == abi.VD_ERR_DEGENERATE and err() == DEGENERATE
        assert untouched(nodes) and np.array_equal(idx, i)
        good_build(c, oracle, 2049, seed=901)
        # an index >= n_vert at 2049 triangles
        v, i = soup(2049)
        i = i.copy(); i[301] = len(v) + 5
        rc, nodes, n, idx = host_build(c, v, i)
        assert rc == abi.VD_ERR_INVALID_ARG and err() == b"vd_bvh_build: index >= n_vert (mesh 0 of the build)"
        assert untouched(nodes) and np.array_equal(idx, i)
        good_build(c, oracle, 2049, seed=902)
        # vd_bvh_build_dev with node_cap one pair short
        need = len(want_tree(oracle, 2049)[0])
        rc, nodes, n, idx = dev_build(c, *soup(2049), node_cap=need - 2)
        assert rc == abi.VD_ERR_INVALID_ARG and err() == b"vd_bvh_build: node_cap too small (mesh 0 of the build needs %d nodes)" % need
        assert untouched(nodes) and n == 0
        good_build(c, oracle, 2049, seed=903)
        # a packed buffer that is full at mesh 1 of 3: one node short of 11 + mesh 0 + mesh 1
        sizes = (513, 2049, 3)
        meshes = [soup(n) for n in sizes]
        n0, n1 = (len(want_tree(oracle, n)[0]) for n in sizes[:2])
        refused = [(abi.VD_OK, 0, 0), (abi.VD_ERR_INVALID_ARG, 0, 0), (abi.VD_OK, 0, 0)]
        batch = Batch(c, meshes, True, True, packed_first=11, packed_cap=11 + n0 + n1 - 1)
        assert batch.run() == abi.VD_ERR_INVALID_ARG
        assert err() == b"vd_bvh_build_batch: the packed node buffer is full at mesh 1 (or its node indices pass 2^32)"
        assert batch.report() == (refused, 11) and untouched(batch.nodes(0))
        good_build(c, oracle, 2049, seed=904)
        batch = Batch(c, meshes, True, False, packed_first=11, packed_cap=11 + n0 + n1 - 1)
        assert batch.run() == abi.VD_ERR_INVALID_ARG
        assert err() == b"vd_bvh_build_batch: item 1 needs %d nodes: node_cap / packed_cap too small" % n1
        assert batch.report() == (refused, 11) and untouched(batch.nodes(0))
        assert all(np.array_equal(batch.indices(m), meshes[m][1]) for m in range(3))
        good_build(c, oracle, 2049, seed=901)
    finally:
        c.close()


# (levels_phase_a, n_top_nodes, n_mid_roots, n_small_roots, kernel_launches) of the commit before this file, per input and
# payload width (blas.wide_payload); "knot" is synth.knot_mesh(1024, 256), the size at which the mid tier starts early
STATS = ("levels_phase_a", "n_top_nodes", "n_mid_roots", "n_small_roots", "kernel_launches")
EXPECTED = {
    ("1", False): (0, 2, 0, 0, 6),
    ("513", False): (0, 4, 1, 2, 9),
    ("2049", False): (1, 12, 2, 6, 107),
    ("3000", False): (1, 16, 2, 8, 107),
    ("3000", True): (1, 16, 2, 8, 107),
    ("9000", False): (3, 58, 8, 29, 205),
    ("9000", True): (3, 58, 8, 29, 205),
    ("knot", False): (10, 2964, 364, 1481, 549),
}


@pytest.mark.parametrize("name,wide", sorted(EXPECTED))
def test_the_launch_sequence_did_not_move(ctx, ctx_options, name, wide):
    if wide:
        ctx_options("blas.wide_payload", 1)
    v, i = synth.knot_mesh(1024, 256) if name == "knot" else soup(int(name))
    ctx.bvh_build(v, i)
    st = ctx.bvh_last_build_stats()
    got = tuple(st[k] for k in STATS)
    print(name, wide, got)
    assert got == EXPECTED[(name, wide)]
