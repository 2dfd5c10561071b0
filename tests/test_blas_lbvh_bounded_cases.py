"""The numpy restatement of the depth-bounded LBVH bottom level (tests/blas_lbvh_bounded_cases.py; the definition is in
include/voidin_abi.h under VD_OPT_BLAS_LBVH_MAX_DEPTH): the bounds at which the rule cannot fire give the unbounded tree, the
bound holds and the leaves still tile the positions, the boxes are a refit's, the rule really fires on the inputs the GPU tests
use (tests/test_gpu_blas_lbvh_bounded.py), and the oracle's trace through the D = 23 helmet never holds more than 24 entries and
finds what it finds through the exact bottom level."""
import numpy as np
import pytest

import blas_lbvh_bounded_cases as bounded
import blas_lbvh_cases as cases
from blas_refit_cases import refit_reference, tree_depth
from test_blas_lbvh_cases import check_invariants
from test_gpu_blas_lbvh import NAMED, _input
from voidin_amd import abi, synth
from wide_scenes import disjoint_instances, grid_rays, mesh_set

_unbounded = {}


def _soup(T):
    return synth.triangle_soup(T, seed=synth.SEED_BASE + 300 + T)


def _lbvh(name):
    if name not in _unbounded:
        _unbounded[name] = cases.lbvh_reference(*_input(name))
    return _unbounded[name]


def _same_tree(a, b):
    return (a["nodes"].tobytes() == b["nodes"].tobytes() and np.array_equal(a["indices"], b["indices"]) and
            (a["n_nodes"], a["max_depth"], a["n_bad_indices"]) == (b["n_nodes"], b["max_depth"], b["n_bad_indices"]))


def test_needr_by_hand():
    assert [bounded.needr(k) for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 1000, 1024, 1025, 1 << 24)] == \
        [0, 0, 0, 0, 1, 2, 2, 2, 2, 3, 3, 4, 9, 9, 10, 23]
    assert [bounded.effective_bound(d) for d in (None, -1, 0, 1, 23, 62, 63, 1 << 40)] == [0, 0, 0, 1, 23, 62, 62, 62]


def test_eight_points_by_hand():
    """x = 0, 1, 2, 3, 4, 5, 6, 100: the codes put seven points left of bit 9 and one right of it.  Unbounded: {0..6} | {7}, then
    {0..3} | {4..6}, then {0, 1} | {2, 3}: depth 3.  D = 2: the root's radix split needs 1 + needr(7) = 3 > 2, so the root is the
    switch node and the tree is the one over the positions: {0..3} | {4..7}, pairs below."""
    v, i = cases.point_triangles([0, 1, 2, 3, 4, 5, 6, 100])
    u = cases.lbvh_reference(v, i)
    assert u["max_depth"] == 3 and u["nodes"]["left_first"][3] == 7 and u["nodes"]["count"][3] == 1
    r = bounded.lbvh_bounded_reference(v, i, 2)
    assert (r["switches"], r["switch_positions"], r["max_depth"], r["n_nodes"]) == (1, 8, 2, 8)
    n = r["nodes"]
    assert n["left_first"].tolist() == [2, 0, 4, 6, 0, 2, 4, 6] and n["count"].tolist() == [0, 0, 0, 0, 2, 2, 2, 2]
    assert n["min"][:, 0].tolist() == [0, 0, 0, 4, 0, 2, 4, 6] and n["max"][:, 0].tolist() == [100, 0, 3, 100, 1, 3, 5, 100]
    assert _same_tree(bounded.lbvh_bounded_reference(v, i, 3), u)


@pytest.mark.parametrize("name", NAMED)
def test_bounds_that_cannot_fire_give_the_unbounded_tree(name):
    v, i = _input(name)
    for D in (0, 62):
        r = bounded.lbvh_bounded_reference(v, i, D)
        assert r["switches"] == 0 and _same_tree(r, _lbvh(name)), (name, D)


def _check_bounded(v, i, D):
    r = bounded.lbvh_bounded_reference(v, i, D)
    assert r["max_depth"] <= D and tree_depth(r["nodes"]) == r["max_depth"]
    check_invariants(r, v, i)                                             # every sorted position lies in exactly one leaf, ...
    v_ext, tri_ext, _ = cases._with_nan_vertex(v, i)
    again = refit_reference(v_ext, tri_ext[r["order"]].reshape(-1), r["nodes"])
    assert again.tobytes() == r["nodes"].tobytes(), "a refit of the restated array changes it"
    return r


@pytest.mark.parametrize("name", NAMED)
def test_the_bound_holds_and_the_leaves_tile_the_positions(name):
    v, i = _input(name)
    T = len(i) // 3
    for D in sorted({max(1, bounded.needr(T)), max(1, bounded.needr(T) + 1), 16 if T > 4000 else 9, 23}):
        if bounded.needr(T) <= D:
            _check_bounded(v, i, D)


@pytest.mark.parametrize("T", [4, 5, 8, 9, 64, 65, 1025, 4097])
def test_soups_at_their_tightest_bounds(T):
    v, i = _soup(T)
    for D in (bounded.needr(T), bounded.needr(T) + 1, 23):
        _check_bounded(v, i, D)


def test_the_rule_fires_on_the_inputs_of_the_gpu_tests():
    """The numbers of the prototype the option was designed with."""
    h = bounded.lbvh_bounded_reference(*_input("helmet"), 23)
    assert (_lbvh("helmet")["max_depth"], h["max_depth"], h["switches"], h["switch_positions"]) == (24, 23, 5, 34)
    k = bounded.lbvh_bounded_reference(*_input("knot"), 16)
    assert k["switches"] == 58 and k["max_depth"] == 16
    s = bounded.lbvh_bounded_reference(*_soup(4097), 12)
    assert s["switches"] == 92 and s["max_depth"] == 12
    for T, D in ((64, 5), (8, 2)):
        r = bounded.lbvh_bounded_reference(*_soup(T), D)
        assert (r["switches"], r["switch_positions"]) == (1, T), "the root is the switch node"
    sp = bounded.lbvh_bounded_reference(*_input("sphere"), 23)
    assert (_lbvh("sphere")["max_depth"], sp["max_depth"]) == (24, 23) and sp["switches"] > 0


def test_duplicates_switch_above_and_inside_runs_of_equal_codes():
    v, i = bounded.duplicates_case()
    for D in (11, 12):
        r = _check_bounded(v, i, D)
        assert r["switch_delta_below_32"] > 0 and r["switch_delta_from_32"] > 0, (D, r["switches"])


def test_random_soups_on_a_grid():
    fired = 0
    for v, i, D in bounded.random_cases():
        fired += _check_bounded(v, i, D)["switches"] > 0
    assert fired >= 10


def test_identical_1000_passes_at_9_and_is_refused_at_8():
    v, i = cases.special_cases()["identical_1000"]
    r = _check_bounded(v, i, 9)
    assert r["switches"] == 0 and r["max_depth"] == 9                     # the position tree IS the unbounded one
    with pytest.raises(ValueError):
        bounded.lbvh_bounded_reference(v, i, 8)


def test_the_option_id_and_the_argument_checks_that_need_no_gpu():
    assert abi.OPTIONS["blas.lbvh_max_depth"] == 19
    lib = abi.load()
    assert lib.vd_ctx_set_option(None, abi.OPTIONS["blas.lbvh_max_depth"], 23) == abi.VD_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def oracle_():
    from oracle import ref
    ref.load()
    return ref


def test_the_oracle_walks_the_bounded_helmet_within_24_entries(oracle_):
    """27 disjoint instances of the helmet, 40 000 rays (the scene of test_trace_over_the_lbvh_bottom_level): the walk that enters
    both children holds at most max_depth + 1 <= 24 entries, and hit flags and distance BITS equal those over the exact BLAS."""
    v, i = _input("helmet")
    r = bounded.lbvh_bounded_reference(v, i, 23)
    infos, B, V, I = mesh_set(oracle_, [(v, i)])
    inst, side = disjoint_instances(27, 5)
    rays = grid_rays(40_000, side, 7)
    tl = oracle_.tlas_build(inst, infos)
    exact, _ = oracle_.trace((tl, inst, infos, B, V, I), rays, threads=16)
    fast, deepest = oracle_.trace((tl, inst, infos, r["nodes"], V, r["indices"]), rays, threads=16)
    print(f"helmet, D = 23: deepest oracle stack {deepest}, max_depth {r['max_depth']}")
    assert deepest <= 24
    assert exact["hit"].sum() > 1000 and (exact["hit"] == 0).any()
    assert np.array_equal(exact["hit"], fast["hit"]) and np.array_equal(exact["dist"].view(np.uint32), fast["dist"].view(np.uint32))
