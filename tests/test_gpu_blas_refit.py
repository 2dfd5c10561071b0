"""BLAS refit on the GPU (vd_bvh_refit*, vd_trace_accel_update_geometry_dev) against the numpy reference of
tests/blas_refit_cases.py: min / max bit for bit, everything else untouched."""
import ctypes as C

import numpy as np
import pytest

from blas_refit_cases import (FIXTURES, chain_mesh, deform, mesh_bounds_reference, refit_reference, tree_depth, with_outlier)
from conftest import fields_equal, first_difference, golden
from voidin_amd import abi, synth
from voidin_amd.runtime import VoidinError

pytestmark = pytest.mark.gpu

CANARY_NODES = 8


def _f32(t):
    return t.cpu().numpy().view(np.float32)


class DevMesh:
    """One mesh on the device: vertices, permuted indices, nodes with a canary region behind n_nodes, a MeshInfo."""

    def __init__(self, ctx, v, idx, nodes):
        import torch
        self.n_vert, self.n_tri, self.n_nodes = len(v), len(idx) // 3, len(nodes)
        self.d_v, self.d_i = ctx.upload(np.ascontiguousarray(v, dtype=np.float32)), ctx.upload(np.ascontiguousarray(idx, dtype=np.uint32))
        self.d_n = torch.full(((self.n_nodes + CANARY_NODES) * 32,), 0xC3, dtype=torch.uint8, device="cuda")
        self.d_n[: self.n_nodes * 32] = ctx.upload(nodes)
        info = np.zeros(1, dtype=abi.MESH_INFO)
        info["min"], info["max"] = 77.0, -77.0
        info["index_count"], info["base_index"], info["vertex_offset"], info["bvh_index"], info["junk"] = len(idx), 11, 22, 33, (44, 55)
        self.info_before = info.copy()
        self.d_info = ctx.upload(info)

    def fill(self, item, with_info=True):
        item.verts_xyz, item.indices, item.nodes = abi.ptr(self.d_v), abi.ptr(self.d_i), abi.ptr(self.d_n)
        item.mesh_info = abi.ptr(self.d_info) if with_info else None
        item.n_vert, item.n_tri, item.n_nodes = self.n_vert, self.n_tri, self.n_nodes

    def set_vertices(self, ctx, v):
        self.d_v.copy_(ctx.upload(np.ascontiguousarray(v, dtype=np.float32)))

    def nodes(self):
        raw = self.d_n.cpu().numpy()
        assert (raw[self.n_nodes * 32:] == 0xC3).all(), "bytes past n_nodes were written"
        return raw[: self.n_nodes * 32].view(abi.BVH_NODE)

    def info(self):
        return self.d_info.cpu().numpy().view(abi.MESH_INFO)


def _check(got, nodes_before, want, what=""):
    assert fields_equal(got, want), (what, first_difference(got, want))
    assert np.array_equal(got["left_first"], nodes_before["left_first"]) and np.array_equal(got["count"], nodes_before["count"]), what
    if len(got) > 1 and not (nodes_before["left_first"][nodes_before["count"] == 0] == 1).any():
        assert got[1:2].tobytes() == nodes_before[1:2].tobytes(), what + ": the reserved node 1 was written"


def _check_info(mesh, v, what=""):
    info, lo_hi = mesh.info(), mesh_bounds_reference(v)
    assert info["min"][0].tobytes() == lo_hi[0].tobytes() and info["max"][0].tobytes() == lo_hi[1].tobytes(), (what, info["min"], info["max"], lo_hi)
    for f in ("index_count", "base_index", "vertex_offset", "bvh_index", "junk"):
        assert np.array_equal(info[f], mesh.info_before[f]), (what, f)


@pytest.mark.parametrize("name", FIXTURES)
def test_refit_identity_on_golden_fixtures(ctx, name):
    """refit(build(x), x) == build(x) on data the GPU builder did not make: the +-1e30 start, the NaN rule, root-is-a-leaf."""
    g = golden(name)
    stale = np.array(g["nodes"], copy=True)
    keep1 = stale[1:2].copy()
    stale["min"] += 1.0; stale["max"] -= 1.0
    stale[1:2] = keep1
    nodes = ctx.bvh_refit(g["vertices"], g["indices_out"], stale)
    assert fields_equal(nodes, g["nodes"]), first_difference(nodes, g["nodes"])


MESHES = [("soup", n) for n in (1, 3, 4, 5, 64, 65, 513, 2049, 3000)] + [("knot", (128, 32)), ("knot", (512, 64))]


def _mesh(kind, arg):
    return synth.triangle_soup(arg, seed=synth.SEED_BASE + 70 + arg) if kind == "soup" else synth.knot_mesh(*arg)


@pytest.mark.parametrize("kind,arg", MESHES, ids=[f"{k}-{a}" for k, a in MESHES])
def test_deformed_meshes_vs_reference(ctx, kind, arg):
    v, i = _mesh(kind, arg)
    v = with_outlier(v)                                           # one unreferenced vertex outside the mesh
    nodes, idx = ctx.bvh_build(v, i)
    mesh = DevMesh(ctx, v, idx, nodes)
    items = (abi.BvhRefitItem * 1)()
    mesh.fill(items[0])
    plan = ctx.bvh_refit_plan(items)
    assert items[0].status == 0
    ctx.bvh_refit_planned(plan); ctx.synchronize()
    _check(mesh.nodes(), nodes, nodes, "identity")                # nothing moved yet: the build's own boxes
    _check_info(mesh, v, "identity")
    v2 = deform(v, phase=0.4)
    mesh.set_vertices(ctx, v2)
    ctx.bvh_refit_planned(plan); ctx.synchronize()
    want = refit_reference(v2, idx, nodes)
    assert not fields_equal(want, nodes)
    _check(mesh.nodes(), nodes, want, "deformed")
    _check_info(mesh, v2, "deformed")
    root_lo = want["min"][0]
    assert not np.array_equal(mesh.info()["min"][0], root_lo)     # the two folds really differ (the outlier, the +-inf start)
    assert fields_equal(ctx.bvh_refit(v2, idx, nodes), want)      # the host-pointer form
    plan.close()


@pytest.mark.parametrize("n_tri,ratio", [(1500, 1.045), (5000, 1.012)])
def test_chain_trees(ctx, n_tri, ratio):
    """Trees hundreds of levels deep: the depth no per-level scheme survives."""
    v, i = chain_mesh(n_tri, ratio)
    nodes, idx = ctx.bvh_build(v, i)
    assert tree_depth(nodes) > 30                                 # what the builder's 8 bins make of a chain: 37 and 38 levels
    mesh = DevMesh(ctx, v, idx, nodes)
    items = (abi.BvhRefitItem * 1)()
    mesh.fill(items[0], with_info=False)
    plan = ctx.bvh_refit_plan(items)
    for scale in (0.5, 1.75):
        v2 = v.copy(); v2[:, 0] *= np.float32(scale)
        mesh.set_vertices(ctx, v2)
        ctx.bvh_refit_planned(plan); ctx.synchronize()
        _check(mesh.nodes(), nodes, refit_reference(v2, idx, nodes), f"x * {scale}")
    assert mesh.info().tobytes() == mesh.info_before.tobytes()    # an item without mesh_info: nothing written there
    plan.close()


@pytest.mark.parametrize("fences", [0, 1])
def test_hand_made_chain_a_thousand_levels_deep(ctx, ctx_options, fences):
    """A refit takes any valid topology, not only the builder's: node 0 -> {leaf, interior -> {leaf, interior -> ...}}, one
    triangle per leaf, 1000 levels - a climb of 1000 dependent hand-overs, in both forms of the hand-over."""
    ctx_options("blas.refit_fences", fences)
    depth = 1000
    v, idx = synth.triangle_soup(depth + 1, seed=synth.SEED_BASE + 123)
    nodes = np.zeros(2 * depth + 2, dtype=abi.BVH_NODE)
    for d in range(depth):                                        # interior node of level d: 0, then 3, 5, 7, ...
        k = 0 if d == 0 else 2 * d + 1
        nodes["left_first"][k] = 2 * d + 2                        # children 2d + 2 (a leaf) and 2d + 3 (the next interior node)
        nodes["left_first"][2 * d + 2], nodes["count"][2 * d + 2] = d, 1
    nodes["left_first"][2 * depth + 1], nodes["count"][2 * depth + 1] = depth, 1
    assert tree_depth(nodes) == depth
    mesh = DevMesh(ctx, v, idx, nodes)
    items = (abi.BvhRefitItem * 1)()
    mesh.fill(items[0])
    plan = ctx.bvh_refit_plan(items)
    for phase in (0.1, 1.3, 2.9):
        v2 = deform(v, phase=phase)
        mesh.set_vertices(ctx, v2)
        ctx.bvh_refit_planned(plan); ctx.synchronize()
        _check(mesh.nodes(), nodes, refit_reference(v2, idx, nodes), f"phase {phase}")
        _check_info(mesh, v2, f"phase {phase}")
    plan.close()


def _packed_batch(ctx, meshes):
    """vd_bvh_build_batch_dev into ONE node buffer; -> (d_nodes, [(d_v, d_i, first, n_nodes)], canary start)."""
    import torch
    cap = sum(max(2 * (len(i) // 3), 2) for _, i in meshes)
    d_nodes = torch.full(((cap + CANARY_NODES) * 32,), 0xC3, dtype=torch.uint8, device="cuda")
    d_nodes[: cap * 32] = 0
    items = (abi.BvhBatchItem * len(meshes))()
    parts = []
    for m, (v, i) in enumerate(meshes):
        d_v, d_i = ctx.upload(np.ascontiguousarray(v, dtype=np.float32)), ctx.upload(np.ascontiguousarray(i, dtype=np.uint32))
        items[m].verts_xyz, items[m].indices_inout, items[m].out_nodes = abi.ptr(d_v), abi.ptr(d_i), None
        items[m].n_vert, items[m].n_tri, items[m].node_cap = len(v), len(i) // 3, 0
        parts.append([d_v, d_i])
    end = ctx.bvh_build_batch_dev(items, len(meshes), d_nodes, cap, 0)
    for m in range(len(meshes)):
        parts[m] += [int(items[m].out_first_node), int(items[m].out_n_nodes)]
    return d_nodes, parts, end


@pytest.mark.parametrize("fences", [0, 1])
def test_one_plan_many_meshes_many_frames(ctx, ctx_options, fences):
    """Five meshes packed into one node buffer, one plan, three refits with nothing reset in between: the counters re-arm
    themselves.  Both forms of the hand-over between two climbers (VD_OPT_BLAS_REFIT_FENCES) give the same bytes."""
    ctx_options("blas.refit_fences", fences)
    meshes = [synth.triangle_soup(n, seed=synth.SEED_BASE + 90 + n) for n in (1, 4, 300, 2049)] + [synth.knot_mesh(128, 32)]
    assert len(meshes[-1][1]) // 3 == 8192
    d_nodes, parts, end = _packed_batch(ctx, meshes)
    built = d_nodes.cpu().numpy()[: end * 32].view(abi.BVH_NODE).copy()
    idx = [p[1].cpu().numpy().view(np.uint32).copy() for p in parts]
    d_infos = ctx.upload(np.zeros(len(meshes), dtype=abi.MESH_INFO))
    items = (abi.BvhRefitItem * len(meshes))()
    for m, (d_v, d_i, first, n_nodes) in enumerate(parts):
        items[m].verts_xyz, items[m].indices, items[m].nodes = abi.ptr(d_v), abi.ptr(d_i), abi.ptr(d_nodes) + 32 * first
        items[m].mesh_info = abi.ptr(d_infos) + 48 * m
        items[m].n_vert, items[m].n_tri, items[m].n_nodes = len(meshes[m][0]), len(idx[m]) // 3, n_nodes
    plan = ctx.bvh_refit_plan(items)
    assert all(items[m].status == 0 for m in range(len(meshes)))
    for frame in range(3):
        vs = [deform(v, phase=0.3 + 0.9 * frame, specials=(frame != 1)) for v, _ in meshes]
        for (d_v, *_), v2 in zip(parts, vs):
            d_v.copy_(ctx.upload(v2))
        ctx.bvh_refit_planned(plan); ctx.synchronize()
        raw = d_nodes.cpu().numpy()
        assert (raw[-CANARY_NODES * 32:] == 0xC3).all() and not raw[end * 32: -CANARY_NODES * 32].any(), "bytes past the last mesh's nodes were written"
        infos = d_infos.cpu().numpy().view(abi.MESH_INFO)
        for m, (_, _, first, n_nodes) in enumerate(parts):
            before = built[first: first + n_nodes]
            got = raw[first * 32: (first + n_nodes) * 32].view(abi.BVH_NODE)
            want = refit_reference(vs[m], idx[m], before)
            _check(got, before, want, f"frame {frame} mesh {m}")
            assert fields_equal(ctx.bvh_refit(vs[m], idx[m], before), got), f"frame {frame} mesh {m}: single-item refit"
            lo, hi = mesh_bounds_reference(vs[m])
            assert infos["min"][m].tobytes() == lo.tobytes() and infos["max"][m].tobytes() == hi.tobytes(), f"frame {frame} mesh {m}"
    plan.close()


def test_refit_replays_from_a_hip_graph(ctx):
    """vd_bvh_refit_planned_dev only enqueues a kernel - no host read, no allocation, no memset - so it is captured the way
    tests/test_gpu_frame_loop.py captures its frame and replayed with the vertex buffer rewritten between replays."""
    import torch
    v, i = synth.knot_mesh(64, 32)
    v = with_outlier(v)
    nodes, idx = ctx.bvh_build(v, i)
    mesh = DevMesh(ctx, v, idx, nodes)
    items = (abi.BvhRefitItem * 1)()
    mesh.fill(items[0])
    plan = ctx.bvh_refit_plan(items)
    ctx.bvh_refit_planned(plan)                                   # warm-up: the code object is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    main_stream = torch.cuda.current_stream().cuda_stream
    try:
        with torch.cuda.graph(graph):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx.bvh_refit_planned(plan)
    finally:
        ctx.set_stream(main_stream)
    for frame in range(3):
        v2 = deform(v, phase=1.1 * frame + 0.2)
        mesh.set_vertices(ctx, v2)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _check(mesh.nodes(), nodes, refit_reference(v2, idx, nodes), f"replay {frame}")
        _check_info(mesh, v2, f"replay {frame}")
    plan.close()


def test_trace_after_a_deformation(ctx, oracle):
    """deform -> vd_bvh_refit_planned_dev -> vd_tlas_refit_dev -> vd_trace_accel_update_geometry_dev -> trace: the prepared
    walk, the plain walk and the oracle over the very same refit buffers agree on every VdHit field; at least a tenth of the
    rays change their distance against the undeformed frame, so a stale triangle copy (or stale boxes) cannot pass."""
    import torch
    knot, ball = synth.knot_mesh(32, 32), synth.uv_sphere(1.0, 3)
    assert len(knot[1]) // 3 == 2048
    V, I, B = [], [], []
    infos = np.zeros(2, dtype=abi.MESH_INFO)
    vo = bo = no = 0
    for k, (v, i) in enumerate((knot, ball)):
        nodes, idx = ctx.bvh_build(v, i)
        infos[k]["min"], infos[k]["max"] = synth.mesh_bounds(v)
        infos[k]["index_count"], infos[k]["base_index"], infos[k]["vertex_offset"], infos[k]["bvh_index"] = len(idx), bo, vo, no
        V.append(v); I.append(idx); B.append(nodes)
        vo += len(v); bo += len(idx); no += len(nodes)
    n_knot_v, n_knot_nodes = len(V[0]), len(B[0])
    V, I, B = np.concatenate(V), np.concatenate(I), np.concatenate(B)

    def at(x, y, z, s, mesh):
        M = np.diag([s, s, s, 1.0]); M[:3, 3] = (x, y, z)
        return synth.instance_from_matrix(M.T.reshape(16), mesh)      # column-major

    inst = np.array([at(-8, 0, 0, 1, 0), at(0, 0, 0, 1, 0), at(8, 0, 0, 1, 0), at(0, 0, -6, 2.5, 1)], dtype=abi.INSTANCE)
    tl = ctx.tlas_build(inst, infos)
    side = 64
    gx, gy = np.meshgrid(np.linspace(-11.3, 11.3, side), np.linspace(-3.4, 3.4, side))
    rays = np.zeros(side * side, dtype=abi.RAY)
    rays["eye"] = np.stack([gx.ravel(), gy.ravel(), np.full(side * side, 30.0)], axis=1).astype(np.float32)
    rays["dir"] = (0.02, -0.01, -1.0)
    ds = ctx.device_scene((tl, inst, infos, B, V, I))
    acc = ctx.trace_prepare(ds)
    d_tl, d_inst, d_infos, d_bvh, d_v, d_i = ds.tensors
    items = (abi.BvhRefitItem * 1)()
    items[0].verts_xyz, items[0].indices, items[0].nodes, items[0].mesh_info = abi.ptr(d_v), abi.ptr(d_i), abi.ptr(d_bvh), abi.ptr(d_infos)
    items[0].n_vert, items[0].n_tri, items[0].n_nodes = n_knot_v, 2048, n_knot_nodes
    plan = ctx.bvh_refit_plan(items)
    d_rays, d_prep, d_plain = ctx.upload(rays), ctx.empty(len(rays) * 16), ctx.empty(len(rays) * 16)
    ctx.trace_prepared_dev(acc, d_rays, len(rays), d_prep); ctx.synchronize()
    frame0 = d_prep.cpu().numpy().view(abi.HIT)[: len(rays)].copy()
    # the frame, in the order of INTEGRATION.md
    knot2 = deform(knot[0] * np.float32(1.12), phase=0.8, specials=False)
    d_v[: n_knot_v * 12] = ctx.upload(knot2)
    ctx.bvh_refit_planned(plan)
    ctx.tlas_refit_dev(d_inst, len(inst), d_infos, len(infos), d_tl)
    acc.update_geometry()
    ctx.trace_prepared_dev(acc, d_rays, len(rays), d_prep)
    ctx.trace_dev(ds, d_rays, len(rays), d_plain)
    ctx.synchronize()
    prep, plain = d_prep.cpu().numpy().view(abi.HIT)[: len(rays)], d_plain.cpu().numpy().view(abi.HIT)[: len(rays)]
    V2, B2 = _f32(d_v).reshape(-1, 3), d_bvh.cpu().numpy().view(abi.BVH_NODE)
    infos2, tl2 = d_infos.cpu().numpy().view(abi.MESH_INFO), d_tl.cpu().numpy().view(abi.TLAS_NODE)
    assert fields_equal(B2[:n_knot_nodes], refit_reference(knot2, I[: 3 * 2048], B[:n_knot_nodes]))
    assert B2[n_knot_nodes:].tobytes() == B[n_knot_nodes:].tobytes()          # the rigid mesh's nodes
    assert fields_equal(tl2, oracle.tlas_refit(inst, infos2, tl))
    want, _ = oracle.trace((tl2, inst, infos2, B2, V2, I), rays, threads=8)
    for f in abi.HIT.names:
        assert prep[f].tobytes() == want[f].tobytes(), f"prepared walk: {f}"
        assert plain[f].tobytes() == want[f].tobytes(), f"plain walk: {f}"
    changed = (prep["dist"].view(np.uint32) != frame0["dist"].view(np.uint32)).mean()
    assert changed >= 0.1, changed
    plan.close(); acc.close()


def _bad_plan(ctx, mesh, edit=None, **sizes):
    import torch
    items = (abi.BvhRefitItem * 2)()
    good = mesh.good
    good.fill(items[0])
    mesh.fill(items[1])
    if edit is not None:
        nodes = mesh.nodes().copy()
        edit(nodes)
        mesh.d_n[: mesh.n_nodes * 32] = ctx.upload(nodes)
    for k, val in sizes.items():
        setattr(items[1], k, val)
    h = C.c_void_p(0x5555)
    rc = ctx.lib.vd_bvh_refit_plan_dev(ctx.h, C.addressof(items), 2, C.byref(h))
    torch.cuda.synchronize()
    return rc, items, h


def test_rejections(ctx):
    v, i = synth.triangle_soup(300, seed=synth.SEED_BASE + 99)
    nodes, idx = ctx.bvh_build(v, i)
    interior = int(np.nonzero((nodes["count"] == 0) & (np.arange(len(nodes)) > 3))[0][0])      # not the root, not one of its children
    leaf = int(np.nonzero(nodes["count"] > 0)[0][-1])

    def fresh():
        m = DevMesh(ctx, v, idx, nodes)
        m.good = DevMesh(ctx, v, idx, nodes)
        return m

    inner = np.nonzero((nodes["count"] == 0) & (np.arange(len(nodes)) > 1))[0]
    # an interior node a whose own children lie far behind, and a later interior node j in front of them: a claims j's
    # children first, then j's own claim meets them taken - before the sweep reaches a's former children, now orphans
    early, later = next((int(a), int(j)) for a in inner for j in inner if a < j < nodes["left_first"][a])

    def child_not_after_parent(n): n["left_first"][interior] = interior           # children must lie in (own id, n_nodes)
    def child_past_the_end(n): n["left_first"][interior] = len(n) - 1             # left_first + 1 == n_nodes
    def two_parents(n): n["left_first"][early] = n["left_first"][later]
    def orphan(n):                                                                # the last interior node turns into a leaf: its children lose their parent
        last = int(np.nonzero(n["count"] == 0)[0][-1])
        assert last > 1 and n["left_first"][last] > 1
        n["count"][last] = 1; n["left_first"][last] = 0
    def leaf_range(n): n["left_first"][leaf] = len(idx) // 3 - int(n["count"][leaf]) + 1

    cases = [(child_not_after_parent, {}, "children are not both in"), (child_past_the_end, {}, "children are not both in"),
             (two_parents, {}, "two parents"), (orphan, {}, "has no parent"), (leaf_range, {}, "triangle range"),
             (None, {"n_vert": int(idx.max())}, "index >= n_vert"),
             (None, {"n_nodes": 0}, "n_nodes < 1")]
    for edit, sizes, message in cases:
        rc, items, h = _bad_plan(ctx, fresh(), edit, **sizes)
        what = edit.__name__ if edit else str(sizes)
        assert rc == abi.VD_ERR_INVALID_ARG, what
        assert message in ctx.lib.vd_last_error(ctx.h).decode(), (what, ctx.lib.vd_last_error(ctx.h))      # THAT check refused it
        assert items[1].status == abi.VD_ERR_INVALID_ARG and items[0].status == 0, what
        assert not h.value, what + ": a plan was returned"
    # null arguments: errors, not crashes
    items = (abi.BvhRefitItem * 1)()
    h = C.c_void_p()
    assert ctx.lib.vd_bvh_refit_plan_dev(None, C.addressof(items), 1, C.byref(h)) == abi.VD_ERR_INVALID_ARG
    assert ctx.lib.vd_bvh_refit_plan_dev(ctx.h, None, 1, C.byref(h)) == abi.VD_ERR_INVALID_ARG and not h.value
    assert ctx.lib.vd_bvh_refit_plan_dev(ctx.h, C.addressof(items), 1, None) == abi.VD_ERR_INVALID_ARG
    assert ctx.lib.vd_bvh_refit_planned_dev(ctx.h, None) == abi.VD_ERR_INVALID_ARG
    assert ctx.lib.vd_bvh_refit_plan_release(ctx.h, None) == abi.VD_ERR_INVALID_ARG
    assert ctx.lib.vd_trace_accel_update_geometry_dev(ctx.h, None) == abi.VD_ERR_INVALID_ARG
    rc = ctx.lib.vd_bvh_refit_plan_dev(ctx.h, C.addressof(items), 1, C.byref(h))      # null pointers inside the item
    assert rc == abi.VD_ERR_INVALID_ARG and items[0].status == abi.VD_ERR_INVALID_ARG and not h.value
    with pytest.raises(VoidinError) as e:
        ctx.bvh_refit(v, idx, nodes[:0])
    assert e.value.code == abi.VD_ERR_INVALID_ARG
    # an empty plan is a plan that does nothing
    empty = ctx.bvh_refit_plan((abi.BvhRefitItem * 1)(), 0)
    assert empty.h.value
    ctx.bvh_refit_planned(empty); ctx.synchronize()
    empty.close()
    # and the context is fine afterwards
    assert fields_equal(ctx.bvh_refit(v, idx, nodes), nodes)
