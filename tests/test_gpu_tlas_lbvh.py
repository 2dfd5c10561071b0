"""vd_tlas_build_lbvh[_wide]_dev: the LBVH top level - its node array slot by slot against the layout include/voidin_abi.h
states and a numpy restatement of the codes, its boxes against the exact build's leaves and the refit's arithmetic, and what
rays hit through it against the exact top level (scenes of pairwise DISJOINT instances: no two instances can tie in distance and
inside an instance the BLAS order decides, so a ray's record does not depend on the shape of the top level)."""
import numpy as np
import pytest

from conftest import golden
from voidin_amd import abi, synth
from voidin_amd.runtime import VoidinError
from wide_scenes import disjoint_instances, first_bad, grid_rays, mesh_set, records_equal

pytestmark = pytest.mark.gpu

BAD_CODE = 0x3fffffff


def _children(nodes):
    if nodes.dtype == abi.TLAS_NODE_WIDE:
        return nodes["left"].astype(np.int64), nodes["right"].astype(np.int64)
    return (nodes["left_right"] & 0xffff).astype(np.int64), (nodes["left_right"] >> 16).astype(np.int64)


def _codes(leaf_min, leaf_max):
    """The codes of the header, restated: 30-bit Morton code of the box centre, 10 bits per axis of the extent of the finite
    centres, x in the highest bit of each triple; a non-finite centre -> 0x3fffffff.  float32 throughout, as the kernel."""
    half = np.float32(0.5)
    with np.errstate(all="ignore"):
        c = (half * (leaf_min + leaf_max)).astype(np.float32)
        fin = np.isfinite(c).all(axis=1)
        codes = np.full(len(c), BAD_CODE, dtype=np.uint32)
        if fin.any():
            lo, hi = c[fin].min(axis=0), c[fin].max(axis=0)
            q = np.zeros((len(c), 3), dtype=np.uint32)
            for k in range(3):
                if hi[k] > lo[k]:
                    t = ((c[:, k] - lo[k]) / (hi[k] - lo[k])).astype(np.float32)
                    q[:, k] = np.where(fin, np.minimum(np.maximum((t * np.float32(1024.0)).astype(np.float32), np.float32(0)), np.float32(1023)), 0).astype(np.uint32)

            def spread(v):
                v = (v | (v << 16)) & 0x030000ff; v = (v | (v << 8)) & 0x0300f00f; v = (v | (v << 4)) & 0x030c30c3; v = (v | (v << 2)) & 0x09249249
                return v
            m = (spread(q[:, 0].astype(np.uint64)) << 2) | (spread(q[:, 1].astype(np.uint64)) << 1) | spread(q[:, 2].astype(np.uint64))
            codes[fin] = m[fin].astype(np.uint32)
    return codes


def _same(a, b):
    """== on floats, a NaN equal to a NaN (boxes of the NaN scene)."""
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _bottom_up_order(nodes, n):
    """Interior slots n+1 .. 2n-1 ordered children-before-parents (iterative post-order from the root 2n - 1)."""
    left, right = _children(nodes)
    order, stack = [], [(2 * n - 1, False)]
    while stack:
        k, done = stack.pop()
        if k <= n:
            continue
        if done:
            order.append(k)
        else:
            stack += [(k, True), (int(left[k]), False), (int(right[k]), False)]
    return order


def _fresh_union(nodes, n, leaf_min, leaf_max):
    """min / max of every node of the topology in `nodes` from the given leaf boxes (per sorted leaf slot), by np.fmin / np.fmax."""
    mn, mx = nodes["min"].copy(), nodes["max"].copy()
    mn[1:n + 1], mx[1:n + 1] = leaf_min, leaf_max
    left, right = _children(nodes)
    for k in _bottom_up_order(nodes, n):
        mn[k], mx[k] = np.fmin(mn[left[k]], mn[right[k]]), np.fmax(mx[left[k]], mx[right[k]])
    if n >= 2:
        mn[2 * n], mx[2 * n], mn[0], mx[0] = mn[2 * n - 1], mx[2 * n - 1], mn[2 * n - 1], mx[2 * n - 1]
    else:
        mn[0], mx[0], mn[2], mx[2] = mn[1], mx[1], mn[1], mx[1]
    return mn, mx


def _check_structure(ctx, inst, meshes, wide):
    import torch
    n = len(inst)
    dt = abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE
    d_i, d_m = ctx.upload(inst), ctx.upload(meshes)
    d_n = torch.full(((2 * n + 1) * dt.itemsize,), 0xCD, dtype=torch.uint8, device="cuda")
    ctx.tlas_build_lbvh_dev(d_i, n, d_m, len(meshes), d_n, wide=wide)
    torch.cuda.synchronize()
    raw = d_n.cpu().numpy().tobytes()
    nodes = np.frombuffer(raw, dtype=dt)
    left, right = _children(nodes)
    exact = ctx.tlas_build(inst, meshes, wide=wide)                       # its leaf i + 1 is instance i (tlas.rs:34-54)
    # leaves: slots 1..n, a permutation of the instances, in sorted code order (equal codes: by instance index - the sort is stable)
    leaves = nodes[1:n + 1]
    assert (left[1:n + 1] == 0).all() and (right[1:n + 1] == 0).all()
    order = leaves["instance_idx"].astype(np.int64)
    assert sorted(order.tolist()) == list(range(n))
    assert leaves["min"].tobytes() == exact["min"][1 + order].tobytes() and leaves["max"].tobytes() == exact["max"][1 + order].tobytes()
    codes = _codes(exact["min"][1:n + 1], exact["max"][1:n + 1])
    assert np.array_equal(order, np.argsort(codes, kind="stable")), "leaves are not in sorted code order"
    if wide:
        assert (nodes["_pad"] == 0).all()
    if n == 1:
        assert left[2] == 1 and right[2] == 1 and nodes[0].tobytes() == nodes[1].tobytes()
        assert nodes["min"][2].tobytes() == nodes["min"][1].tobytes() and nodes["max"][2].tobytes() == nodes["max"][1].tobytes()
    else:
        interior = np.arange(n + 1, 2 * n)                                # n+1 .. 2n-2 and the root 2n-1
        assert (nodes["instance_idx"][n + 1:] == 0xffffffff).all()
        assert ((left[interior] >= 1) & (left[interior] <= 2 * n - 2) & (right[interior] >= 1) & (right[interior] <= 2 * n - 2)).all()
        assert (left[interior] != right[interior]).all()
        # every slot 1 .. 2n-2 is the child of exactly one interior node: a tree over all leaves with 2n-1 as its root
        assert sorted(np.concatenate([left[interior], right[interior]]).tolist()) == list(range(1, 2 * n - 1))
        assert left[2 * n] == 2 * n - 1 and right[2 * n] == 2 * n - 1                     # tlas.rs:59: the closing self-merge
        assert nodes[0].tobytes() == nodes[2 * n - 1].tobytes()                           # node 0: the TRUE root's copy
        assert nodes["min"][2 * n].tobytes() == nodes["min"][2 * n - 1].tobytes() and nodes["max"][2 * n].tobytes() == nodes["max"][2 * n - 1].tobytes()
    # every instance in exactly one leaf reachable from node 0
    seen, todo = [], [0]
    while todo:
        k = todo.pop()
        if left[k] == 0 and right[k] == 0:
            seen.append(int(nodes["instance_idx"][k]))
        else:
            todo += [int(left[k]), int(right[k])]
    assert sorted(seen) == list(range(n))
    # every interior box is the union of its children's
    mn, mx = _fresh_union(nodes, n, leaves["min"], leaves["max"])
    assert _same(nodes["min"], mn) and _same(nodes["max"], mx)
    # the refit takes the array as it is and changes no byte: the boxes are the oracle-checked refit arithmetic's
    d_r = d_n.clone()
    ctx.tlas_refit_dev(d_i, n, d_m, len(meshes), d_r, wide=wide)
    torch.cuda.synchronize()
    assert d_r.cpu().numpy().tobytes() == raw, "vd_tlas_refit changed an LBVH array"
    # the same bytes again
    d_2 = torch.full_like(d_n, 0x11)
    ctx.tlas_build_lbvh_dev(d_i, n, d_m, len(meshes), d_2, wide=wide)
    torch.cuda.synchronize()
    assert d_2.cpu().numpy().tobytes() == raw, "two builds differ"
    return nodes, d_i, d_m, d_n


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1000])
def test_structure(ctx, n, wide):
    meshes = synth.mesh_infos()
    inst = synth.instances(n, seed=synth.SEED_BASE + 50 + n, extent=120.0)
    nodes, d_i, d_m, d_n = _check_structure(ctx, inst, meshes, wide)
    # host-pointer form: the same bytes
    assert ctx.tlas_build_lbvh(inst, meshes, wide=wide).tobytes() == nodes.tobytes()


def test_structure_40000_wide_and_refit_after_motion(ctx, oracle):
    import torch
    n = 40_000
    meshes = synth.mesh_infos()
    inst = synth.instances(n, seed=synth.SEED_BASE + 51, extent=900.0)
    nodes, d_i, d_m, d_n = _check_structure(ctx, inst, meshes, True)
    assert int(max(nodes["left"].max(), nodes["right"].max())) > 0xffff
    # the instances move (compute_update.wgsl): the refit of the LBVH tree == a fresh union over the same topology
    ids = np.arange(0, n, 3, dtype=np.uint32)
    ctx.compute_update_dev(ctx.upload(ids), len(ids), d_i, n, 1.3, 0.016, True)
    ctx.tlas_refit_dev(d_i, n, d_m, len(meshes), d_n, wide=True)
    torch.cuda.synchronize()
    moved = oracle.compute_update(ids, inst, 1.3, 0.016, True)
    assert d_i.cpu().numpy().tobytes() == moved.tobytes()
    after = d_n.cpu().numpy().view(abi.TLAS_NODE_WIDE)
    assert np.array_equal(after["left"], nodes["left"]) and np.array_equal(after["right"], nodes["right"]) and np.array_equal(after["instance_idx"], nodes["instance_idx"])
    exact = ctx.tlas_build(moved[:2000], meshes, wide=True)                                # leaf boxes of the first 2000 moved instances
    order = nodes["instance_idx"][1:n + 1].astype(np.int64)
    sel = np.nonzero(order < 2000)[0]
    assert after["min"][1 + sel].tobytes() == exact["min"][1 + order[sel]].tobytes()
    mn, mx = _fresh_union(after, n, after["min"][1:n + 1], after["max"][1:n + 1])
    assert _same(after["min"], mn) and _same(after["max"], mx)
    assert not _same(after["min"], nodes["min"])


@pytest.mark.parametrize("wide", [False, True])
def test_structure_with_nan_and_infinite_boxes(ctx, wide):
    """tests/golden/tlas_nan_60.npz: NaN and inf - inf transforms.  A centre with a non-finite coordinate gets the fixed code
    0x3fffffff and sorts last; the boxes still fold with the NaN-ignoring union."""
    g = golden("tlas_nan_60.npz")
    inst, meshes = g["instances"], g["meshes"]
    nodes, *_ = _check_structure(ctx, inst, meshes, wide)
    exact = ctx.tlas_build(inst, meshes, wide=wide)
    codes = _codes(exact["min"][1:len(inst) + 1], exact["max"][1:len(inst) + 1])
    n_bad = int((codes == BAD_CODE).sum())
    assert 0 < n_bad < len(inst)
    assert (codes[nodes["instance_idx"][1 + len(inst) - n_bad: 1 + len(inst)]] == BAD_CODE).all()


def test_limits(ctx):
    """Checked before the device is touched: the pointers are never followed."""
    fake = 1 << 20
    lib = ctx.lib
    assert lib.vd_tlas_build_lbvh_dev(ctx.h, fake, abi.TLAS_MAX_INSTANCES + 1, fake, 1, fake) == abi.VD_ERR_TLAS_OVERFLOW
    assert lib.vd_tlas_build_lbvh(ctx.h, fake, abi.TLAS_MAX_INSTANCES + 1, fake, 1, fake) == abi.VD_ERR_TLAS_OVERFLOW
    assert lib.vd_tlas_build_lbvh_wide_dev(ctx.h, fake, abi.TLAS_WIDE_MAX_INSTANCES + 1, fake, 1, fake) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_tlas_build_lbvh_wide(ctx.h, fake, abi.TLAS_WIDE_MAX_INSTANCES + 1, fake, 1, fake) == abi.VD_ERR_INVALID_ARG
    for fn in (lib.vd_tlas_build_lbvh_dev, lib.vd_tlas_build_lbvh_wide_dev):
        assert fn(ctx.h, fake, 0, fake, 1, fake) == abi.VD_ERR_INVALID_ARG
        assert fn(ctx.h, fake, 4, fake, 0, fake) == abi.VD_ERR_INVALID_ARG
        assert fn(ctx.h, None, 4, fake, 1, fake) == abi.VD_ERR_INVALID_ARG


def _sphere_scene(oracle, n, seed):
    infos, B, V, I = mesh_set(oracle, [synth.uv_sphere(1.0, 5)])
    inst, side = disjoint_instances(n, seed)
    assert np.abs(V).max() <= 1.0 + 1e-6
    return inst, side, infos, B, V, I


def test_same_hits_as_the_exact_top_level(ctx, oracle):
    """3 000 disjoint instances, 32 768 rays.  Narrow: the ORACLE's walk over the GPU-built narrow LBVH array == the oracle's walk
    over the oracle's exact array.  Wide: vd_trace_wide_dev over the wide LBVH array == the same records.  Every ray is compared."""
    import torch
    n = 3000
    inst, side, infos, B, V, I = _sphere_scene(oracle, n, seed=6)
    rays = grid_rays(32_768, side, seed=66)
    want, _ = oracle.trace((oracle.tlas_build(inst, infos), inst, infos, B, V, I), rays, threads=16)
    assert want["hit"].sum() > len(rays) // 4 and (want["hit"] == 0).any()
    narrow = ctx.tlas_build_lbvh(inst, infos)
    got_n, _ = oracle.trace((narrow, inst, infos, B, V, I), rays, threads=16)
    assert records_equal(got_n, want), first_bad(got_n, want)
    wide = ctx.tlas_build_lbvh(inst, infos, wide=True)
    ds = ctx.device_scene((wide, inst, infos, B, V, I))
    d_h = ctx.empty(len(rays) * 16)
    d_any = torch.full((len(rays),), 7, dtype=torch.int32, device="cuda")
    ctx.trace_wide_dev(ds, ctx.upload(rays), len(rays), d_h)
    ctx.trace_any_wide_dev(ds, ctx.upload(rays), len(rays), d_any)
    torch.cuda.synchronize()
    got_w = d_h.cpu().numpy()[: len(rays) * 16].view(abi.HIT)
    assert records_equal(got_w, want), first_bad(got_w, want)
    assert np.array_equal(d_any.cpu().numpy().astype(np.uint32), want["hit"])
    # and the narrow LBVH array under the narrow GPU walk
    d_h2 = ctx.empty(len(rays) * 16)
    ctx.trace_dev(ctx.device_scene((narrow, inst, infos, B, V, I)), ctx.upload(rays), len(rays), d_h2)
    torch.cuda.synchronize()
    assert records_equal(d_h2.cpu().numpy()[: len(rays) * 16].view(abi.HIT), want)


def test_past_32768_real_instances(ctx, oracle):
    """40 000 disjoint instances under ONE wide LBVH top level against the same scene as two narrow exact scenes of 20 000: per ray
    the chunk with the smaller dist (instance index offset by the chunk's base), a miss only where both miss."""
    import torch
    n, half = 40_000, 20_000
    inst, side, infos, B, V, I = _sphere_scene(oracle, n, seed=7)
    rays = grid_rays(65_536, side, seed=77)
    n_rays = len(rays)
    d_rays, d_m = ctx.upload(rays), ctx.upload(infos)
    chunk = []
    for base in (0, half):
        part = np.ascontiguousarray(inst[base: base + half])
        d_i = ctx.upload(part)
        d_t = ctx.empty((2 * half + 1) * 32)
        ctx.tlas_build_dev(d_i, half, d_m, len(infos), d_t)
        torch.cuda.synchronize()
        tl = d_t.cpu().numpy()[: (2 * half + 1) * 32].view(abi.TLAS_NODE)
        d_h = ctx.empty(n_rays * 16)
        ctx.trace_dev(ctx.device_scene((tl, part, infos, B, V, I)), d_rays, n_rays, d_h)
        torch.cuda.synchronize()
        h = d_h.cpu().numpy()[: n_rays * 16].view(abi.HIT).copy()
        h["instance"][h["hit"] == 1] += base
        chunk.append(h)
    a, b = chunk
    both = (a["hit"] == 1) & (b["hit"] == 1)
    assert not (both & (a["dist"] == b["dist"])).any()                    # disjoint instances: no tie between the chunks
    take_b = (b["hit"] == 1) & ((a["hit"] == 0) | (b["dist"] < a["dist"]))
    want = np.where(take_b, b, a)
    assert want["hit"].sum() >= n_rays // 4
    assert (take_b & (want["hit"] == 1)).sum() > 1000 and (~take_b & (want["hit"] == 1)).sum() > 1000       # both chunks win rays
    assert (want["dist"][want["hit"] == 0] == np.float32(1e30)).all()
    d_i, d_n = ctx.upload(inst), ctx.empty((2 * n + 1) * 48)
    ctx.tlas_build_lbvh_dev(d_i, n, d_m, len(infos), d_n, wide=True)
    torch.cuda.synchronize()
    wide = d_n.cpu().numpy()[: (2 * n + 1) * 48].view(abi.TLAS_NODE_WIDE)
    ds = ctx.device_scene((wide, inst, infos, B, V, I))
    d_h = ctx.empty(n_rays * 16)
    d_any = torch.full((n_rays,), 7, dtype=torch.int32, device="cuda")
    ctx.trace_wide_dev(ds, d_rays, n_rays, d_h)
    ctx.trace_any_wide_dev(ds, d_rays, n_rays, d_any)
    torch.cuda.synchronize()
    got = d_h.cpu().numpy()[: n_rays * 16].view(abi.HIT)
    assert records_equal(got, want), first_bad(got, want)
    assert np.array_equal(d_any.cpu().numpy().astype(np.uint32), want["hit"])


def test_frame_loop_rebuilds_from_a_hip_graph(ctx, oracle):
    """{compute_update, vd_tlas_build_lbvh_wide_dev} over 4 096 instances captured into a HIP graph after one uncaptured warm-up
    call (which sizes the context's work memory: the captured call then only enqueues).  Everything goes to the ONE stream of the
    context, so the captured graph is a single chain.  Three replays; after each the nodes equal an uncaptured build of that frame's
    instances."""
    import torch
    n = 4096
    meshes = synth.mesh_infos()
    inst = synth.instances(n, seed=synth.SEED_BASE + 52, extent=300.0)
    ids = np.arange(0, n, 2, dtype=np.uint32)
    d_m, d_i, d_ids = ctx.upload(meshes), ctx.upload(inst), ctx.upload(ids)
    nbytes = (2 * n + 1) * 48
    d_n, d_check = ctx.empty(nbytes), ctx.empty(nbytes)
    t, dt = 0.7, 0.016

    def frame():
        ctx.compute_update_dev(d_ids, len(ids), d_i, n, t, dt, True)
        ctx.tlas_build_lbvh_dev(d_i, n, d_m, len(meshes), d_n, wide=True)

    frame()                                              # warm-up
    torch.cuda.synchronize()
    ref_inst = oracle.compute_update(ids, inst, t, dt, True)
    graph = torch.cuda.CUDAGraph()
    main_stream = torch.cuda.current_stream().cuda_stream
    try:
        with torch.cuda.graph(graph):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            frame()
    finally:
        ctx.set_stream(main_stream)
    seen = set()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        ref_inst = oracle.compute_update(ids, ref_inst, t, dt, True)
        assert d_i.cpu().numpy().tobytes() == ref_inst.tobytes()
        ctx.tlas_build_lbvh_dev(ctx.upload(ref_inst), n, d_m, len(meshes), d_check, wide=True)
        torch.cuda.synchronize()
        got = d_n.cpu().numpy()[:nbytes].tobytes()
        assert got == d_check.cpu().numpy()[:nbytes].tobytes()
        seen.add(got)
    assert len(seen) == 3                                # three different frames
