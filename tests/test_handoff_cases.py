"""The input pairs of tests/handoff_cases.py have teeth: alternating them changes every word that changes hands inside a launch.
Proved on the CPU from the references alone, for the very shapes tests/test_gpu_handoffs.py runs - a condition of that test, not a
measurement, and without a tolerance: a seed for which it does not hold is a wrong seed."""
import numpy as np
import pytest

import handoff_cases as H
from conftest import fields_equal
from voidin_amd import abi


def _all_boxes_change(a, b, interior, what):
    holds, kept = H.teeth(a, b, interior)
    assert interior.sum() > 0, what
    assert holds, f"{what}: {kept} of {int(interior.sum())} interior nodes keep all six words of their box"


@pytest.mark.parametrize("n,wide", [(4096, False), (32768, False), (40000, True)])
def test_tlas_refit_every_interior_box_changes(oracle, n, wide):
    meshes, inputs = H.tlas_refit_inputs(n)
    (_, a), (_, b1) = inputs
    assert (a["transform"][:, H.TRANSLATION] != b1["transform"][:, H.TRANSLATION]).all(), "every translation moves"
    assert (a["transform"][:, H.LINEAR] != b1["transform"][:, H.LINEAR]).any(axis=1).all(), "every scale changes"
    topology = H.pairwise_topology(n, wide)
    ea, eb = H.tlas_refit_expected(oracle, topology, meshes, inputs)
    _all_boxes_change(ea, eb, H.tlas_interior(ea), f"n = {n}")
    for f in set(ea.dtype.names) - {"min", "max"}:
        assert np.array_equal(ea[f], topology[f]) and np.array_equal(eb[f], topology[f]), f"{f}: one topology"


@pytest.mark.parametrize("wide", [False, True])
def test_children_first_is_the_same_tree(oracle, wide):
    """The renumbering the GPU test applies to an LBVH top level: here to a tree whose numbering is NOT children-first (a
    pairwise tree with its interior ids reversed), so the oracle's ascending sweep would read boxes it has not made yet."""
    n = 1000
    meshes, inputs = H.tlas_refit_inputs(4096)
    inst = inputs[0][1][:n]
    good = H.pairwise_topology(n, wide)
    flip = np.arange(2 * n + 1)
    flip[n + 1:2 * n - 1] = flip[n + 1:2 * n - 1][::-1].copy()          # the root stays 2n - 1
    left, right = H.tlas_children(good)
    bad = good.copy()
    bad[flip] = good
    inv = np.argsort(flip)
    H._set_children(bad, flip[left][inv], flip[right][inv])
    back = H.children_first(bad)
    want, got = oracle.tlas_refit(inst, meshes, good), oracle.tlas_refit(inst, meshes, back)
    wrong = oracle.tlas_refit(inst, meshes, bad)
    for f in ("min", "max"):       # the same root, the same multiset of interior boxes, the same leaves
        assert got[f][[0, 2 * n - 1, 2 * n]].tobytes() == want[f][[0, 2 * n - 1, 2 * n]].tobytes()
        assert np.array_equal(np.sort(got[f][n + 1:2 * n], axis=0), np.sort(want[f][n + 1:2 * n], axis=0))
        assert got[f][1:n + 1].tobytes() == want[f][1:n + 1].tobytes()
    assert not np.array_equal(np.sort(wrong["min"][n + 1:2 * n], axis=0), np.sort(want["min"][n + 1:2 * n], axis=0)), \
        "the oracle's sweep over the other numbering reads boxes it has not made yet: the renumbering is needed"


@pytest.mark.parametrize("plan", list(H.REFIT_PLANS))
def test_blas_refit_every_interior_box_changes(oracle, plan):
    built, inputs = H.blas_refit_inputs(plan, oracle)
    (_, va), (_, vb) = inputs
    ea, eb = H.blas_refit_expected(built, va), H.blas_refit_expected(built, vb)
    leaves = 0
    for m, ((na, ia), (nb, ib), (v, idx, nodes)) in enumerate(zip(ea, eb, built)):
        assert fields_equal(na, nodes), "A is the mesh as built: the refit reference gives the build's boxes back"
        assert (va[m] != vb[m]).any(axis=1).all(), "every vertex moves"
        _all_boxes_change(na, nb, H.blas_interior(na), f"{plan}[{m}]")
        assert ia[0].tobytes() != ib[0].tobytes() and ia[1].tobytes() != ib[1].tobytes(), "the MeshInfo bounds change too"
        leaves += int((nodes["count"] > 0).sum())
    if plan == "three":
        assert leaves >= 16 * 256 and leaves % 256, "at least 16 blocks of 256 climbers, the last one ragged"


@pytest.mark.parametrize("name,bound", [("soup4097", 0), ("soup4097", 12), ("helmet", 0)])
def test_blas_lbvh_boxes_and_meta_change(name, bound):
    a, b1, b2 = H.lbvh_expected(name, bound)
    assert a["n_nodes"] == b1["n_nodes"] and np.array_equal(a["nodes"]["left_first"], b1["nodes"]["left_first"]) and np.array_equal(a["nodes"]["count"], b1["nodes"]["count"]), \
        "times two changes no code: the same tree"
    assert np.array_equal(a["indices"], b1["indices"])
    _all_boxes_change(a["nodes"], b1["nodes"], H.blas_interior(a["nodes"]), f"{name} D={bound}")
    assert H.meta_teeth(a["nodes"], b2["nodes"]) >= 0.5, "A / B2: left_first / count of at least half of the interior nodes"
    if bound:
        assert a["max_depth"] <= bound and a["switches"] > 0, "the bound binds"


def test_blas_lbvh_bound_of_12_cannot_take_the_helmet():
    """15 452 triangles need a radix depth of 13: the library refuses the bound (VD_ERR_INVALID_ARG), so the bounded variant runs
    the 4 097-triangle soup only."""
    with pytest.raises(ValueError):
        H.lbvh_expected("helmet", 12)


def test_blas_lbvh_plan_inputs_change_boxes_counts_and_trees():
    e = H.lbvh_plan_expected()
    inp = H.lbvh_plan_inputs()
    assert H.PLAN_COUNTS["B1"] == [0, 3, 4, 1025, 2000] and H.PLAN_CAPS == [3, 4, 300, 1025, 4097]
    for m, cap in enumerate(H.PLAN_CAPS):
        assert all(len(inp[t][1][m]) == 3 * cap and len(inp[t][0][m]) == len(inp["A"][0][m]) for t in inp), "one shape"
    m = H.PLAN_CAPS.index(1025)                              # the one mesh whose count A and B1 share: the same tree, other boxes
    _all_boxes_change(e["A"][m]["nodes"], e["B1"][m]["nodes"], H.blas_interior(e["A"][m]["nodes"]), "1025")
    for m in (3, 4):                                         # the meshes with interior nodes to speak of
        for x, y in (("A", "B1"), ("B1", "B2"), ("B2", "A")):
            a, b = e[x][m]["nodes"], e[y][m]["nodes"]
            k = min(len(a), len(b))
            inner = H.blas_interior(a)[:k] & H.blas_interior(b)[:k]
            _all_boxes_change(a[:k], b[:k], inner, f"mesh {m} {x}/{y}")
    assert H.meta_teeth(e["A"][4]["nodes"], e["B1"][4]["nodes"]) >= 0.5 and H.meta_teeth(e["A"][4]["nodes"], e["B2"][4]["nodes"]) >= 0.5
    assert e["B1"][0] is None, "a count of 0: nothing is built"


@pytest.mark.parametrize("name", H.BUILD_MESHES)
def test_bvh_build_boxes_and_links_change(oracle, name):
    (na, ia), (nb1, ib1), (nb2, _) = H.bvh_build_expected(oracle, name)
    assert len(na) == len(nb1) and np.array_equal(na["left_first"], nb1["left_first"]) and np.array_equal(ia, ib1), "times two: the same tree"
    _all_boxes_change(na, nb1, H.blas_interior(na), name)
    assert H.meta_teeth(na, nb2) >= 0.5


def test_tlas_lbvh_inputs_are_one_shape():
    """The LBVH top level has no byte-level restatement: whether its boxes change between the inputs is asserted on the GPU, on
    the outputs tests/test_gpu_tlas_lbvh.py::_check_structure has accepted.  Here: the inputs differ the way they are meant to."""
    for n in (4096, 40000):
        meshes, inputs = H.tlas_lbvh_inputs(n)
        (_, a), (_, b1), (_, b2) = inputs
        assert len(a) == len(b1) == len(b2) == n and a.dtype == abi.INSTANCE
        assert np.array_equal(b1["transform"][:, H.TRANSLATION], a["transform"][:, H.TRANSLATION] * np.float32(2.0))
        assert (b2["transform"][:, H.TRANSLATION] != a["transform"][:, H.TRANSLATION]).any(axis=1).all()
