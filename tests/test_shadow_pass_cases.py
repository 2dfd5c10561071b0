"""tests/shadow_pass_cases.py without a GPU: the float32 twin of the range rule against hand values, the packing, the recorded
brute-force answer against the brute force itself and against the oracle, and the CONDITIONS that keep tests/test_gpu_shadow_pass.py
from being vacuous - a pass that finds everything in range, or nothing, or no occluded pair, must not be able to pass it."""
import numpy as np

import shadow_pass_cases as S
import trace_range_cases as cases
from voidin_amd import abi

F = np.float32


def _light(position, radius):
    l = np.zeros(1, dtype=abi.LIGHT)
    l["position"], l["radius"] = position, radius
    return l


def test_the_twin_against_hand_values():
    pos = np.array([[0, 0, 0], [3, 4, 0], [1, 2, 2], [0, 0, 10]], F)             # 0, 5, 3 and 10 away from the origin
    assert S.dist(pos, [0, 0, 0]).tolist() == [0.0, 5.0, 3.0, 10.0]
    nan, inf = F(np.nan), F(np.inf)
    for radius, want in ((5.0, [1, 1, 1, 0]), (np.nextafter(F(5), F(0)), [1, 0, 1, 0]), (0.0, [1, 0, 0, 0]), (-0.0, [1, 0, 0, 0]), (-1.0, [0, 0, 0, 0]),
                         (inf, [1, 1, 1, 1]), (nan, [1, 1, 1, 1]), (-inf, [0, 0, 0, 0]), (3.0, [1, 0, 1, 0]), (1e30, [1, 1, 1, 1])):
        assert S.in_range(pos, _light([0, 0, 0], radius))[:, 0].tolist() == [bool(w) for w in want], radius
    # a NaN distance is in range whatever the radius; an infinite one against an infinite radius (inf - inf) too
    assert S.in_range(pos, _light([nan, 0, 0], 1.0)).all() and S.in_range(pos, _light([inf, 0, 0], inf)).all()
    assert not S.in_range(pos, _light([inf, 0, 0], 1e30)).any()
    # the order of the sum: (dx*dx + dy*dy) + dz*dz in float32, not another association
    p = np.array([[F(1e-4), F(4096), F(0.5)]], F)
    d = S.dist(p, [0, 0, 0])[0]
    assert d == np.sqrt(F(F(F(1e-4) * F(1e-4) + F(4096) * F(4096)) + F(0.5) * F(0.5)))


def test_packing():
    bits = np.zeros((3, 65), bool)
    bits[0, 0] = bits[0, 31] = bits[1, 32] = bits[2, 64] = bits[2, 63] = True
    w = S.pack(bits)
    assert w.dtype == np.uint32 and w.shape == (3, 3)
    assert w.tolist() == [[0x80000001, 0, 0], [0, 1, 0], [0, 0x80000000, 1]]
    assert S.pack(np.ones((2, 33), bool)).tolist() == [[0xFFFFFFFF, 1]] * 2       # nothing at or above the light count
    assert S.pack(np.ones((1, 1), bool)).tolist() == [[1]]


def test_the_seeded_case_is_not_vacuous(oracle):
    scene, pos, nor = S.points(oracle)
    assert len(pos) == S.N_POINTS == 2142 and nor.shape == pos.shape
    lts = S.lights()
    assert len(lts) == 65 and (len(lts) + 31) // 32 == 3
    assert not (pos[:, None, :] == lts["position"][None, :, :]).all(axis=2).any()                  # no light coincides with a point
    for on in (0, 1):
        w = S.seeded_want(oracle, S.N_POINTS, S.N_LIGHTS, on)
        share = w.reach.mean()
        occluded = w.occluded.sum() / w.reach.sum()
        per_light = w.reach.mean(axis=0)
        print(f"\nrange option {on}: in-range share {share:.3f}, per light {per_light.min():.3f} .. {per_light.max():.3f}, occluded share {occluded:.3f}")
        assert 0.25 <= share <= 0.75
        assert occluded >= 0.15 and 1.0 - occluded >= 0.15
        assert (w.reach.any(axis=0) & (~w.reach).any(axis=0)).all()                                   # every light: a point in range, one out of it
        assert w.n_rays == w.reach.sum() and w.in_range_words.shape == (S.N_POINTS, 3)
        assert (w.in_range_words[:, 2] <= 1).all() and (w.occluded_words & ~w.in_range_words == 0).all()
        # every shape of the GPU test has rays, and - but for the 1 x 1 corner - pairs out of range
        for n_points in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2142):
            for n_lights in (1, 31, 32, 33, 65):
                sub = w.reach[:n_points, :n_lights]
                assert sub.any() and (n_points * n_lights == 1 or not sub.all()), (n_points, n_lights)
    off, on = S.seeded_want(oracle, S.N_POINTS, S.N_LIGHTS, 0), S.seeded_want(oracle, S.N_POINTS, S.N_LIGHTS, 1)
    assert (on.occluded <= off.occluded).all() and (on.occluded != off.occluded).sum() > 10          # the option changes the answer


def test_the_record_is_the_brute_forces_answer(oracle):
    """Every 37th ray of the 139 230 through the brute force again; and all of them against the oracle: an interval with only an
    upper end keeps the closest hit or nothing (tests/test_gpu_trace_range.py::test_upper_bound_exact_from_the_oracle)."""
    scene, pos, nor = S.points(oracle)
    lts = S.lights()
    hit = S.any_hit(oracle, "seeded", scene, pos, nor, lts, True)
    rays = S.shadow_rays(oracle, pos, nor, lts)
    flat = hit.T.reshape(-1)                                                       # light-major, as the rays are
    sample = np.arange(0, len(rays), 37)
    assert np.array_equal(S.segment_hits(scene, rays[sample]), flat[sample])
    rec = oracle.trace(scene, rays, threads=8)[0]
    assert np.array_equal((rec["hit"] == 1) & (rec["dist"] < F(1)), flat)
    assert 0 < flat[sample].sum() < len(sample)


def test_the_hand_made_set_sits_on_the_edges(oracle):
    scene, pos, nor, lts = S.hand_made(oracle)
    at = lts["position"][0]
    d = S.dist(pos, at)
    assert len(pos) == 6 and not (pos[:, None, :] == lts["position"][None, :, :]).all(axis=2).any()
    reach = S.in_range(pos, lts)
    r = lts["radius"]
    assert r[1] == d[0] and reach[0, 1] and r[2] < d[0] and not reach[0, 2]        # exactly the distance: in range; one float below: out
    assert r[3] == d[1] and reach[1, 3] and r[4] < d[1] and not reach[1, 4]
    assert not reach[:, 0].any() and reach[:, 5].all() and np.isnan(r[6]) and reach[:, 6].all()      # 0, +inf, NaN
    assert not reach[:, 7].any() and np.signbit(r[8]) and r[8] == 0 and not reach[:, 8].any()        # negative, -0.0
    off, on = S.hand_want(oracle, 0), S.hand_want(oracle, 1)
    # shadow_scene's promise for its two points and its light: [1, 1] by default, [0, 1] on the segment to the light
    assert off.occluded[:2, 5].tolist() == [True, True] and on.occluded[:2, 5].tolist() == [False, True]
    assert 0 < off.n_rays < reach.size
