"""The expected values of the ray-interval tests (tests/trace_range_cases.py), checked WITHOUT a GPU: the brute force restates
the oracle, its answers are decided by one triangle nearly everywhere, and every class of interval that
tests/test_gpu_trace_range.py relies on is populated - a GPU test there cannot pass on an empty set."""
import numpy as np
import pytest

import trace_range_cases as cases
from voidin_amd import abi
from voidin_amd.runtime import set_ray_range

F = np.float32


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_brute_force_over_the_half_line_is_the_oracle(oracle, name):
    c = cases.case(name, oracle)
    n = len(c.rays)
    e = cases.expected(c.hits, np.zeros(n, F), np.full(n, 1e30, F), c.miss_record())
    assert e.records["dist"].tobytes() == c.want["dist"].tobytes()                    # bit for bit, misses (1e30) included
    assert np.array_equal(e.records["hit"], c.want["hit"]) and 0 < c.want["hit"].sum() < n
    u = e.unique
    assert e.records[u].tobytes() == c.want[u].tobytes()                               # where one triangle decides: all four words
    assert (~u).mean() <= 0.02


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_class_of_interval_is_populated(oracle, name):
    c = cases.case(name, oracle)
    cut, ended, not_unique = cases.populations(c, c.t_min, c.t_max)
    print(f"\n{name}: first hit cut away by t_min with a later one inside {cut:.3f}, turned into misses by t_max {ended:.3f}, "
          f"left out of the instance / triangle comparison {not_unique:.3f}")
    assert not_unique <= 0.02
    assert ended >= 0.05
    if name == "golden":
        # the fixture's own rays: fewer than 5 % of them (47 of 1024 as committed) meet two triangles at all, so the bound cannot be
        # reached there - every ray that does meet two is in the class, which is the most the fixture allows
        two = np.isfinite(c.hits.nth(1))
        assert two.any() and cut == two.mean()
    else:
        assert cut >= 0.05


def test_the_chain_scene_reaches_the_deep_pass_with_real_intervals(oracle):
    """Rays whose first hit is cut away while nothing ends them walk on exactly as the unbounded ray does until it accepts its
    first triangle - so they hold what it holds there: more than the 128 entries of a lane."""
    c = cases.case("chain", oracle)
    _, deepest, depth, at_hit = oracle.trace(c.scene, c.rays, threads=8, first_hit=True)
    assert deepest > 128
    t_lo, t_hi = cases.normalise(c.t_min, c.t_max)
    first = c.hits.nth(0)
    deep = (at_hit != 0xFFFFFFFF) & (at_hit > 128) & (first <= t_lo) & (t_hi == F(1e30))
    assert deep.sum() >= 20


def test_the_big_call_is_large_enough_to_fan_out(oracle):
    c = cases.case("seeded", oracle)
    rays, t_min, t_max, ray_of = cases.big_call(c, 103, cases.SEED + 50)
    assert len(rays) >= 420_000 and len(rays) >= 256 * 24 * 64                       # one ray per lane of the persistent grid
    assert rays[4096:8192].tobytes() == c.rays.tobytes() and not np.array_equal(t_min[:4096], t_min[4096:8192])
    e = cases.expected(c.hits, t_min, t_max, c.miss_record(), ray_of)
    assert 0.2 < e.records["hit"].mean() < 0.5 and (~e.unique).mean() <= 0.02


def test_field_normalisation_and_the_helper():
    t_lo, t_hi = cases.normalise([np.nan, -1.0, -0.0, np.inf, 2.0], [np.nan, np.inf, 3e30, -1.0, 0.0])
    assert np.array_equal(t_lo, np.array([0, 0, 0, np.inf, 2], F)) and np.array_equal(t_hi, np.array([1e30, 1e30, 1e30, -1, 0], F))
    rays = np.zeros(3, dtype=abi.RAY)
    assert set_ray_range(rays, 0.5, [1.0, 2.0, 3.0]) is rays
    assert rays["_pad0"].tolist() == [0.5] * 3 and rays["_pad1"].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(TypeError):
        set_ray_range(np.zeros(3, dtype=abi.HIT), 0, 1)


def test_the_shadow_scene_separates_the_segment_from_the_half_line(oracle):
    """The reference's shadow ray has no end: the sphere BEHIND the light shadows point 0.  On the segment to the light it does not;
    the sphere between point 1 and the light shadows it either way."""
    scene, pos, nor, light = cases.shadow_scene(oracle)
    rays = oracle.shadow_rays(pos, nor, light)
    want, _ = oracle.trace(scene, rays, threads=1)
    assert want["hit"].tolist() == [1, 1] and 1.7 < want["dist"][0] < 1.9 and 0.3 < want["dist"][1] < 0.6
    hits = cases.brute_force(scene, rays)
    miss = np.zeros(1, dtype=abi.HIT)[0]
    e = cases.expected(hits, np.zeros(2, F), np.ones(2, F), miss)
    assert e.records["hit"].tolist() == [0, 1] and e.records["dist"][1] == want["dist"][1]
