"""The lattice cases of tests/blas_lattice_cases.py, on the CPU: both restatements of the reference's builder agree on
them, the census finds - in nodes of EVERY size class - the tied minima and the centroids on split planes that make the
tree depend on `<` against `<=`, and a restatement with `<=` in either place, in one size class only, builds another tree.
That is what entitles tests/test_gpu_blas_lattice.py to pin the four implementations in blas.hip with them."""
import numpy as np
import pytest

import blas_lattice_cases as cases
from conftest import fields_equal
from oracle import np_restate as npr
from voidin_amd import abi, synth

_census = {}


def _counted(name):
    """(Census, (nodes, indices)) of one case, built once and shared."""
    if name not in _census:
        _census[name] = cases.census(*cases.case(name))
    return _census[name]


def test_the_case_set():
    want = {"grid_48x48": 4608, "grid_33x32": 2112, "grid_24x24": 1152, "grid_16x16": 512, "grid_37x29_alt": 2 * 37 * 29,
            "grid_32x32_unit": 2048}
    for name, n_tri in want.items():
        v, i = cases.case(name)
        assert v.dtype == np.float32 and i.dtype == np.uint32 and len(i) == 3 * n_tri and int(i.max()) == len(v) - 1
    v, i = cases.case("grid_48x48")
    assert len(v) == 49 * 49 and set(np.unique(v[:, 0])) == set(np.arange(49) * 3.0) and not v[:, 2].any()
    v, i = cases.case("grid_37x29_alt")
    assert v[:, 0].max() == 3 * 37 and v[:, 1].max() == 6 * 29
    v, i = cases.case("grid_23x23_height")
    z = v[:, 2].reshape(24, 24)
    assert z.any() and np.array_equal(z, z.T)
    for name, lo in (("voxel_10", cases.VD_MID_MAX + 1), ("voxel_6", cases.VD_SMALL_MAX + 1)):
        v, i = cases.case(name)
        assert len(i) // 3 >= lo and np.array_equal(v, np.round(v / 3) * 3) and len(np.unique(v, axis=0)) == len(v)
        tri = v[i.reshape(-1, 3)].astype(np.float64)
        assert (np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) == 9.0).all()   # half a 3 x 3 quad each
    assert cases.case("voxel_6")[0] is cases.case("voxel_6")[0]                   # made once
    v2, i2 = cases.with_repeats(*cases.case("grid_16x16"), 5, 2)
    assert len(i2) == 3 * 514 and np.array_equal(i2[-6:], np.tile(cases.case("grid_16x16")[1][15:18], 2))


@pytest.mark.parametrize("name", cases.NAMES)
def test_restatement_equals_the_c_oracle(oracle, name):
    v, i = cases.case(name)
    want_nodes, want_idx = oracle.bvh_build(v, i)
    nodes, idx = npr.bvh_build(v, i)
    assert fields_equal(nodes, want_nodes), cases.first_difference(nodes, want_nodes)
    assert np.array_equal(idx, want_idx)
    # ... and the census is the same code path apart from the recording
    c_nodes, c_idx = _counted(name)[1]
    assert c_nodes.tobytes() == nodes.tobytes() and c_idx.tobytes() == idx.tobytes()


def test_census_conditions_hold_in_every_size_class():
    """Conditions, not measurements: per size class, over the case set, >= 2 nodes whose minimal cost is reached by
    candidates with different left sets, >= 1 of them across axes, >= 50 (triangle, candidate) pairs with the centroid
    exactly on the plane.  Above 2048 the pairs on a zero-extent axis count too (a flat grid's z: all seven planes
    coincide with every centroid, `<` sends all of them right and `<=` would not); the voxel surface has the other kind."""
    total = {c: dict(nodes=0, tied=0, tied_across_axes=0, on_plane=0, on_plane_flat=0) for c in cases.SIZE_CLASSES}
    for name in cases.NAMES:
        c = _counted(name)[0]
        table = c.table()
        print(cases.format_table(name, len(cases.case(name)[1]) // 3, table))
        for cls, t in table.items():
            for k in t:
                total[cls][k] += t[k]
        for r in c.rows:                                                          # what a row holds
            assert len(r["costs"]) == 21 == len(r["lefts"]) and r["count"] >= 4
            assert all(len(l) < r["count"] for l in r["lefts"])                   # one element is never examined: never all left
    print(cases.format_table("the whole case set", sum(len(cases.case(n)[1]) // 3 for n in cases.NAMES), total))
    for cls, t in total.items():
        assert t["tied"] >= 2, (cls, t)
        assert t["tied_across_axes"] >= 1, (cls, t)
        on_plane = t["on_plane"] + (t["on_plane_flat"] if cls == ">2048" else 0)
        assert on_plane >= 50, (cls, t)
    assert total[">2048"]["on_plane"] > 0 and _counted("voxel_10")[0].table()[">2048"]["on_plane"] > 0
    # the tiers the GPU tests expect each case to reach
    for name in ("grid_48x48", "grid_33x32", "grid_37x29_alt", "voxel_10"):
        assert _counted(name)[0].table()[">2048"]["nodes"] >= 1
    assert _counted("grid_48x48")[0].table()[">2048"]["nodes"] == 3               # two levels of phase A
    for name in cases.NAMES:
        assert (_counted(name)[0].table()["513..2048"]["nodes"] > 0) == (name != "grid_16x16")


SENSITIVITY = {"<=32": "grid_16x16", "33..512": "grid_16x16", "513..2048": "grid_24x24", ">2048": "grid_48x48"}


@pytest.mark.parametrize("kind", ["tie", "predicate"])
@pytest.mark.parametrize("size_class", list(cases.SIZE_CLASSES))
def test_a_mutant_in_one_size_class_builds_another_tree(size_class, kind):
    """`<=` in the cost comparison, or in the shuffle predicate, in the nodes of ONE size class: the tree (or the index
    permutation) differs from the reference's - so a kernel tier with that mistake cannot pass the GPU comparison."""
    name = SENSITIVITY[size_class]
    v, i = cases.case(name)
    want_nodes, want_idx = _counted(name)[1]
    got = cases.mutant_build(kind, size_class, v, i)
    assert got is None or got[0].tobytes() != want_nodes.tobytes() or got[1].tobytes() != want_idx.tobytes(), \
        f"{name}: the {kind} mutant in {size_class} builds the reference's tree - a generator has drifted"


def test_a_random_soup_has_neither():
    """Why the existing inputs could not stand in: in a 3000-triangle soup no node above 32 primitives has a tied minimum
    and no centroid lies on any plane."""
    c, _ = cases.census(*synth.triangle_soup(3000, seed=7))
    table = c.table()
    print(cases.format_table("triangle_soup(3000, seed=7)", 3000, table))
    for cls, t in table.items():
        assert t["on_plane"] == 0 and t["on_plane_flat"] == 0, (cls, t)
        assert cls == "<=32" or t["tied"] == 0, (cls, t)
    assert table[">2048"]["nodes"] == 1 and table["513..2048"]["nodes"] > 0


def test_deep_degenerate_input_is_an_error_in_both(oracle):
    v, i = cases.deep_degenerate()
    assert len(i) // 3 == 1152 + 4
    with pytest.raises(ValueError, match="degenerate"):
        npr.bvh_build(v, i)
    with pytest.raises(oracle.OracleError) as e:
        oracle.bvh_build(v, i)
    assert e.value.code == abi.VD_ERR_DEGENERATE
    # the root itself splits: the node that fails lies below it
    c = cases.Census(v, i)
    with pytest.raises(ValueError):
        c.build()
    assert len(c.rows) >= 2 and c.rows[0]["count"] == 1156


def test_first_difference_names_node_count_and_class(oracle):
    """The one line a GPU mismatch prints: first differing node in pre-order, its primitive count, its size class."""
    v, i = cases.case("grid_24x24")
    want = _counted("grid_24x24")[1][0]
    assert cases.first_difference(want, want) == "all nodes equal"
    counts = cases.subtree_counts(want)
    assert counts[0] == 1152 and counts[2] + counts[3] == 1152
    order = cases.preorder(want)
    assert order[:2] == [0, 2] and sorted(order) == [k for k in range(len(want)) if k != 1]
    bad = want.copy()
    late, early = order[40], order[7]
    bad["min"][late][0] += 1
    bad["max"][early][1] += 1
    msg = cases.first_difference(bad, want)
    assert f"node {early} " in msg and f"{counts[early]} primitives" in msg and cases.size_class(int(counts[early])) in msg
    assert "node count" in cases.first_difference(want[:-2], want)
