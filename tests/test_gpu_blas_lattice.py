"""The SAH BLAS build on lattice meshes (tests/blas_lattice_cases.py), against the C oracle bit for bit.  Vertices on a
lattice make different splits cost exactly the same and put centroids exactly on split planes in nodes of every size -
tests/test_blas_lattice_cases.py shows that on the CPU - so the tree depends on each tier of blas.hip keeping the FIRST
minimum of its 21 costs and evaluating `centroid < pos`, not `<=`: phase A (> 2048 primitives), the mid tier (513..2048),
phase B (<= 512) and its lane groups (<= 32).  A mismatch names the first differing node in pre-order, its primitive
count and that count's size class: which tier to open."""
import ctypes as C

import numpy as np
import pytest

import blas_lattice_cases as cases
import blas_lbvh_cases as lbvh
from conftest import fields_equal
from test_gpu_blas import diff_report
from voidin_amd import abi, synth
from voidin_amd.runtime import VoidinError

pytestmark = pytest.mark.gpu

PAD = 8                                      # canary rows in front of and behind the node buffer of a _dev build
_want = {}


def _expected(oracle, name, arrays=None):
    """The oracle's (nodes, indices) of one input, computed once and shared, never written."""
    if name not in _want:
        v, i = arrays if arrays is not None else cases.case(name)
        nodes, idx = oracle.bvh_build(v, i)
        nodes.setflags(write=False); idx.setflags(write=False)
        _want[name] = (nodes, idx)
    return _want[name]


def _assert_tree(got, want, what):
    nodes, idx = got
    want_nodes, want_idx = want
    assert fields_equal(nodes, want_nodes), f"{what}: {cases.first_difference(nodes, want_nodes)}; {diff_report(nodes, want_nodes)}"
    assert np.array_equal(idx, want_idx), f"{what}: nodes equal, index permutation differs first at triangle {int(np.flatnonzero(idx != want_idx)[0]) // 3}"


def _upload(ctx, a, dtype):
    """A private copy on the device: the arrays of cases.case() are shared and read-only."""
    return ctx.upload(np.array(a, dtype=dtype))


def _build_dev(ctx, v, i):
    """vd_bvh_build_dev into node_cap = 2T rows between canary rows -> (nodes, indices)."""
    import torch
    n_tri = len(i) // 3
    cap = 2 * n_tri
    d_v, d_i = _upload(ctx, v, np.float32), _upload(ctx, i, np.uint32)
    d_all = torch.full(((cap + 2 * PAD) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    n = ctx.bvh_build_dev(d_v, len(v), d_i, n_tri, d_all[PAD * 32: (PAD + cap) * 32], cap)
    torch.cuda.synchronize()
    raw = d_all.cpu().numpy()
    assert (raw[: PAD * 32] == 0xA5).all() and (raw[(PAD + n) * 32:] == 0xA5).all(), "a node outside [0, n_nodes) was written"
    return raw[PAD * 32: (PAD + n) * 32].view(abi.BVH_NODE).copy(), d_i.cpu().numpy().view(np.uint32)[: 3 * n_tri].copy()


def _check_tiers(ctx, name, want_nodes, what):
    """The tier the case is there for really ran."""
    st = ctx.bvh_last_build_stats()
    print(f"{name} [{what}]: {len(want_nodes)} nodes, stats {st}")
    counts = cases.subtree_counts(want_nodes)
    interior = counts[want_nodes["count"] == 0]
    if (interior > cases.VD_MID_MAX).any():
        assert st["levels_phase_a"] >= 1, (name, what, st)
    else:
        assert st["levels_phase_a"] == 0, (name, what, st)
    if ((interior > cases.VD_SMALL_MAX) & (interior <= cases.VD_MID_MAX)).any():
        assert st["n_mid_roots"] > 0, (name, what, st)
    assert st["n_small_roots"] > 0, (name, what, st)
    return st


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_in_three_forms(ctx, oracle, ctx_options, name):
    v, i = cases.case(name)
    want = _expected(oracle, name)
    _assert_tree(ctx.bvh_build(v, i), want, f"{name}, vd_bvh_build")
    st = _check_tiers(ctx, name, want[0], "host form")
    if len(i) // 3 > cases.VD_MID_MAX:
        assert st["levels_phase_a"] >= 1
    if name == "grid_48x48":
        assert st["levels_phase_a"] >= 2
    _assert_tree(_build_dev(ctx, v, i), want, f"{name}, vd_bvh_build_dev")
    _check_tiers(ctx, name, want[0], "_dev form")
    # the 8-byte payload with 21 predicate bits: a second implementation of the predicate in phase A
    ctx_options("blas.wide_payload", 1)
    _assert_tree(_build_dev(ctx, v, i), want, f"{name}, vd_bvh_build_dev with blas.wide_payload")
    _check_tiers(ctx, name, want[0], "_dev form, wide payload")


def test_a_mismatch_names_node_count_and_class(oracle):
    """What the assertions above print when a tier is wrong, on a tree damaged by hand."""
    want = _expected(oracle, "grid_24x24")
    bad = want[0].copy()
    k = int(bad["left_first"][0])                                    # the root's left child
    bad["max"][k][0] += 3.0
    counts = cases.subtree_counts(want[0])
    with pytest.raises(AssertionError) as e:
        _assert_tree((bad, want[1]), want, "grid_24x24")
    msg = str(e.value)
    assert f"first differing node {k} " in msg and f"{counts[k]} primitives" in msg and f"size class {cases.size_class(int(counts[k]))}" in msg


def test_one_batch_of_all_cases(ctx, oracle):
    """Every case, two random soups and the first lattice once more in ONE packed build: the phases run once for all of
    them, so lattice and random segments share launches.  Each mesh == its single build == the oracle."""
    names = cases.NAMES + ["soup_700", "soup_3000", cases.NAMES[0]]
    arrays = {"soup_700": synth.triangle_soup(700, seed=synth.SEED_BASE + 910), "soup_3000": synth.triangle_soup(3000, seed=synth.SEED_BASE + 911)}
    meshes = [arrays[n] if n in arrays else cases.case(n) for n in names]
    want = [_expected(oracle, n, arrays.get(n)) for n in names]
    shared, parts = ctx.bvh_build_batch(meshes, packed=True)
    st = ctx.bvh_last_build_stats()
    print("batch:", st)
    assert st["levels_phase_a"] >= 2 and st["n_mid_roots"] > 0 and st["n_small_roots"] > 0
    at = 0
    for m, (name, (first, n_nodes, idx), w) in enumerate(zip(names, parts, want)):
        assert first == at and n_nodes == len(w[0]), f"mesh {m} ({name}): nodes [{first}, +{n_nodes}) want [{at}, +{len(w[0])})"
        _assert_tree((shared[first: first + n_nodes], idx), w, f"mesh {m} ({name}) of the batch")
        at += n_nodes
    assert at == len(shared)
    for m, (name, mesh, w) in enumerate(zip(names, meshes, want)):
        _assert_tree(ctx.bvh_build(*mesh), w, f"{name}, single build")
    a, b = parts[0], parts[-1]                                       # the same lattice twice
    assert shared[a[0]: a[0] + a[1]].tobytes() == shared[b[0]: b[0] + b[1]].tobytes() and np.array_equal(a[2], b[2])


def _swap_xy(nodes):
    out = nodes.copy()
    out["min"] = nodes["min"][:, [1, 0, 2]]
    out["max"] = nodes["max"][:, [1, 0, 2]]
    return out


def test_transforms_that_keep_the_lattice(ctx, oracle):
    """The flat 48 x 48 grid shifted by integers, scaled by a power of two (coordinates stay exact, ties stay ties) and
    with x and y swapped.  The first minimum in (axis, bin) order is not symmetric in the axes: the oracle's tree of the
    swapped input is NOT its tree of the input with the boxes swapped - and the GPU must follow it both ways."""
    v, i = cases.case("grid_48x48")
    base = _expected(oracle, "grid_48x48")
    shifted = (v + np.float32([1024, -2048, 512])).astype(np.float32)
    assert np.array_equal(shifted.astype(np.float64), v.astype(np.float64) + [1024, -2048, 512])
    scaled = (v * np.float32(2.0 ** -20)).astype(np.float32)
    assert np.array_equal(scaled.astype(np.float64) * 2.0 ** 20, v.astype(np.float64))
    swapped = np.ascontiguousarray(v[:, [1, 0, 2]])
    for what, vv in (("shifted", shifted), ("scaled", scaled), ("x and y swapped", swapped)):
        want = _expected(oracle, "grid_48x48 " + what, (vv, i))
        _assert_tree(ctx.bvh_build(vv, i), want, "grid_48x48 " + what)
        assert ctx.bvh_last_build_stats()["levels_phase_a"] >= 2
        _assert_tree(_build_dev(ctx, vv, i), want, "grid_48x48 " + what + ", _dev")
    sw = _expected(oracle, "grid_48x48 x and y swapped")
    assert len(sw[0]) != len(base[0]) or not fields_equal(sw[0], _swap_xy(base[0])) or not np.array_equal(sw[1], base[1]), \
        "swapping the axes of the input gave the swapped tree: the grid no longer ties across axes"
    # a power-of-two scale keeps every comparison: the same topology and permutation, the boxes scaled
    sc = _expected(oracle, "grid_48x48 scaled")
    assert np.array_equal(sc[1], base[1]) and np.array_equal(sc[0]["left_first"], base[0]["left_first"])
    assert np.array_equal(sc[0]["max"].astype(np.float64) * 2.0 ** 20, base[0]["max"].astype(np.float64))


def _dev_build_rc(ctx, v, i):
    import torch
    n_tri = len(i) // 3
    d_v, d_i = _upload(ctx, v, np.float32), _upload(ctx, i, np.uint32)
    d_n = ctx.empty(2 * n_tri * 32)
    n_nodes = C.c_uint32(0)
    rc = ctx.lib.vd_bvh_build_dev(ctx.h, abi.ptr(d_v), len(v), abi.ptr(d_i), n_tri, abi.ptr(d_n), 2 * n_tri, C.addressof(n_nodes))
    torch.cuda.synchronize()
    return rc


def test_degenerate_inputs_agree_with_the_oracle(ctx, oracle):
    """Every candidate rejected - the reference crashes, the oracle and the library say VD_ERR_DEGENERATE, through host and
    device pointers: in a node of five equal centroids deep below a mid-tier root (phase B finds it), and in the root of
    2304 and of 5000 identical triangles (phase A's all-rejected path; up to 2048 the mid tier takes the root)."""
    tri_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    inputs = [("deep", cases.deep_degenerate())]
    inputs += [(f"{n} identical", (tri_v, np.tile(np.array([0, 1, 2], np.uint32), n))) for n in (2304, 5000)]
    for what, (v, i) in inputs:
        with pytest.raises(oracle.OracleError) as eo:
            oracle.bvh_build(v, i)
        assert eo.value.code == abi.VD_ERR_DEGENERATE, what
        with pytest.raises(VoidinError) as e:
            ctx.bvh_build(v, i)
        assert e.value.code == abi.VD_ERR_DEGENERATE, what
        print(what, ctx.bvh_last_build_stats())                      # (a refused build leaves levels_phase_a at 0)
        assert _dev_build_rc(ctx, v, i) == abi.VD_ERR_DEGENERATE, what
    # the context is as usable as before
    _assert_tree(ctx.bvh_build(*cases.case("grid_24x24")), _expected(oracle, "grid_24x24"), "grid_24x24 after the refusals")


def _host_batch(ctx, meshes, packed):
    """vd_bvh_build_batch through the C ABI -> (return code, vd_last_error, every item's status)."""
    K = len(meshes)
    items = (abi.BvhBatchItem * K)()
    keep = []
    for m, (v, i) in enumerate(meshes):
        v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
        i = np.array(i, dtype=np.uint32).reshape(-1).copy()
        nodes = np.zeros(2 * (len(i) // 3), dtype=abi.BVH_NODE)
        keep.append((v, i, nodes))
        items[m].verts_xyz, items[m].indices_inout, items[m].out_nodes = v.ctypes.data, i.ctypes.data, None if packed else nodes.ctypes.data
        items[m].n_vert, items[m].n_tri, items[m].node_cap = len(v), len(i) // 3, 0 if packed else len(nodes)
    cap = sum(len(k[2]) for k in keep)
    shared = np.zeros(cap, dtype=abi.BVH_NODE)
    rc = ctx.lib.vd_bvh_build_batch(ctx.h, C.addressof(items), K, shared.ctypes.data if packed else None, cap if packed else 0, 0, None)
    return rc, ctx.lib.vd_last_error(ctx.h), [items[m].status for m in range(K)]


def test_every_tier_names_its_degenerate_mesh(ctx, oracle):
    """The node that no candidate splits found by phase B (the deep input), by the mid tier (2000 identical triangles) and
    by phase A (2304): as mesh 3 of 5, each is named.  Of two degenerate meshes that the same tier finds, the first."""
    tri_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    identical = lambda n: (tri_v, np.tile(np.array([0, 1, 2], np.uint32), n))
    good = [cases.case(n) for n in ("voxel_6", "grid_33x32", "grid_16x16", "grid_24x24")]
    for what, bad in (("phase B", cases.deep_degenerate()), ("mid tier", identical(2000)), ("phase A", identical(2304))):
        rc, text, status = _host_batch(ctx, good[:3] + [bad] + good[3:], True)
        print(what, rc, text, status)
        assert rc == abi.VD_ERR_DEGENERATE and b"mesh 3" in text, what
        assert status == [0, 0, 0, abi.VD_ERR_DEGENERATE, 0], what
    for what, bad in (("phase B", cases.deep_degenerate()), ("phase A", identical(2304))):
        rc, text, status = _host_batch(ctx, [good[0], bad, good[1], good[2], bad], False)
        assert rc == abi.VD_ERR_DEGENERATE and b"mesh 1" in text and status == [0, abi.VD_ERR_DEGENERATE, 0, 0, 0], (what, text, status)
    # one mesh: the text as it always was, the status set
    rc, text, status = _host_batch(ctx, [cases.deep_degenerate()], True)
    assert rc == abi.VD_ERR_DEGENERATE and b"mesh" not in text and status == [abi.VD_ERR_DEGENERATE]
    _assert_tree(ctx.bvh_build(*cases.case("grid_16x16")), _expected(oracle, "grid_16x16"), "grid_16x16 after the refused batches")


def test_degenerate_mesh_in_a_batch_is_named(ctx, oracle):
    """The deep degenerate input as mesh 3 of 5: the batch fails with VD_ERR_DEGENERATE, the error text and the items'
    status name mesh 3, and the next build on the context is right."""
    names = ["voxel_6", "grid_33x32", "grid_16x16", None, "grid_24x24"]
    meshes = [cases.deep_degenerate() if n is None else cases.case(n) for n in names]
    K = len(meshes)
    for packed in (False, True):
        rc, text, status = _host_batch(ctx, meshes, packed)
        print("packed" if packed else "own arrays", rc, text, status)
        assert rc == abi.VD_ERR_DEGENERATE and b"mesh 3" in text
        assert status == [0, 0, 0, abi.VD_ERR_DEGENERATE, 0]
        shared_ok, parts = ctx.bvh_build_batch([meshes[m] for m in (0, 1, 2, 4)])             # a following valid build
        for (first, n_nodes, idx), n in zip(parts, (names[m] for m in (0, 1, 2, 4))):
            _assert_tree((shared_ok[first: first + n_nodes], idx), _expected(oracle, n), f"{n} after the refused batch")
    # the device-pointer form names it too
    items = (abi.BvhBatchItem * K)()
    dev = []
    for m, (v, i) in enumerate(meshes):
        d_v, d_i = _upload(ctx, v, np.float32), _upload(ctx, i, np.uint32)
        d_n = ctx.empty(2 * (len(i) // 3) * 32)
        dev.append((d_v, d_i, d_n))
        items[m].verts_xyz, items[m].indices_inout, items[m].out_nodes = abi.ptr(d_v), abi.ptr(d_i), abi.ptr(d_n)
        items[m].n_vert, items[m].n_tri, items[m].node_cap = len(v), len(i) // 3, 2 * (len(i) // 3)
    with pytest.raises(VoidinError) as e:
        ctx.bvh_build_batch_dev(items, K)
    assert e.value.code == abi.VD_ERR_DEGENERATE and b"mesh 3" in ctx.lib.vd_last_error(ctx.h)
    assert [items[m].status for m in range(K)] == [0, 0, 0, abi.VD_ERR_DEGENERATE, 0]
    _assert_tree(ctx.bvh_build(*cases.case("voxel_6")), _expected(oracle, "voxel_6"), "voxel_6 after the refused batches")


DOWNSTREAM = ["grid_48x48", "voxel_10"]


@pytest.mark.parametrize("name", DOWNSTREAM)
def test_refit_of_the_build_returns_its_bytes(ctx, oracle, name):
    """bvh_refit(v, i, build(v, i)) == build(v, i): boxes of flat triangles have zero extent on one axis."""
    v, i = cases.case(name)
    nodes, idx = ctx.bvh_build(v, i)
    _assert_tree((nodes, idx), _expected(oracle, name), name)
    stale = nodes.copy()
    keep1 = stale[1:2].copy()
    stale["min"] += 1.0; stale["max"] -= 1.0
    stale[1:2] = keep1
    again = ctx.bvh_refit(v, idx, stale)
    assert again.tobytes() == nodes.tobytes(), cases.first_difference(again, nodes)
    tri = v[idx.reshape(-1, 3)]
    assert ((tri.max(axis=1) - tri.min(axis=1)) == 0).any(axis=1).all()          # every triangle is flat on some axis


@pytest.mark.parametrize("name", DOWNSTREAM)
def test_lbvh_build_equals_its_restatement(ctx, ctx_options, name):
    """vd_bvh_build_lbvh, unbounded and under a depth bound that does not fire: lattices give runs of equal Morton codes."""
    v, i = cases.case(name)
    r = lbvh.lbvh_reference(v, i)
    codes = r["codes"]
    assert (codes[1:] == codes[:-1]).sum() > len(codes) // 4 and r["max_depth"] <= 23
    for bound in (None, 23):
        if bound is not None:
            ctx_options("blas.lbvh_max_depth", bound)
        nodes, idx = ctx.bvh_build_lbvh(v, i)
        assert len(nodes) == r["n_nodes"] and fields_equal(nodes, r["nodes"]), (bound, cases.first_difference(nodes, r["nodes"]))
        assert np.array_equal(idx, r["indices"]), bound


def _bundle(oracle, name):
    """32 x 32 primary rays looking down -z at the mesh from above its middle, at a height where pixel centres fall on
    lattice lines: rays through shared edges and vertices."""
    v, _ = cases.case(name)
    mid = (v.max(axis=0) + v.min(axis=0)) / 2
    height = {"grid_48x48": 72.0, "voxel_10": 24.0}[name]
    cam = synth.camera_uniform(eye=(float(mid[0]), float(mid[1]), float(v[:, 2].max()) + height), pitch_deg=0.0, aspect=1.0)
    return oracle.primary_rays(cam, 32, 32)


@pytest.mark.parametrize("name", DOWNSTREAM)
def test_traverse_iter_over_the_sah_tree(ctx, oracle, name):
    import torch
    v, i = cases.case(name)
    nodes, idx = ctx.bvh_build(v, i)
    _assert_tree((nodes, idx), _expected(oracle, name), name)
    rays = _bundle(oracle, name)
    want = oracle.traverse_iter(nodes, v, idx, rays)
    print(name, "hits", int((want >= 0).sum()), "of", len(rays))
    assert (want >= 0).sum() > len(rays) // 4 and (want < 0).any()
    d_out = torch.full((len(rays),), 7.0, dtype=torch.float32, device="cuda")
    ctx.traverse_iter_dev(ctx.upload(nodes), len(nodes), _upload(ctx, v, np.float32), ctx.upload(idx), ctx.upload(rays), len(rays), d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{name}: {bad.size} rays differ, first {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"
