"""tests/fan_supply_cases.py without a GPU: the properties of the input that tests/test_gpu_trace_fan_supply.py relies on, from the
oracle alone - most rays are occluded and occluded far from their point (jobs die in long runs only then), no ray needs the deep
second pass, and the rays are what vd_shadow_rays_dev makes under "trace.ray_range"."""
import numpy as np

import fan_supply_cases as S

F = np.float32


def test_the_rays_are_shadow_rays_of_surface_points(oracle):
    pos, nor = S.points(oracle)
    assert pos.shape == nor.shape == (S.N_POINTS, 3) and S.N_POINTS == 256 * 64
    assert np.allclose(np.linalg.norm(nor.astype(np.float64), axis=1), 1.0, atol=1e-6)
    n = len(S.LIGHTS)
    r = S.rays(oracle, n)
    assert len(r) == n * S.N_POINTS and 16384 <= S.N_LIGHTS * S.N_POINTS <= 65536
    assert len(S.rays(oracle)) == S.N_LIGHTS * S.N_POINTS and S.rays(oracle).tobytes() == r[: S.N_LIGHTS * S.N_POINTS].tobytes()
    for l in range(n):
        part = r[l * S.N_POINTS: (l + 1) * S.N_POINTS]
        want = oracle.shadow_rays(pos, nor, S.LIGHTS[l])
        assert part["eye"].tobytes() == want["eye"].tobytes() and part["dir"].tobytes() == want["dir"].tobytes()
        # origin = point + normal * 1e-4, dir = light - point, in float32
        assert part["eye"].tobytes() == (pos + nor * F(0.0001)).astype(F).tobytes()
        assert part["dir"].tobytes() == (S.LIGHTS[l][None, :] - pos).astype(F).tobytes()
    assert (r["_pad0"] == 0).all() and (r["_pad1"] == 1).all()
    lts = S.lights(n)
    assert (lts["position"] == S.LIGHTS).all() and (np.linalg.norm(r["dir"], axis=1) < lts["radius"][0]).all()      # every pair in range


def test_most_rays_are_occluded_far_from_their_point(oracle):
    """Floors: OCCLUDED_FLOOR = 0.9 of every light's rays occluded (measured 0.979, 0.984, 0.981, 0.941), the median distance to
    the occluder above FAR_FLOOR = 2 world units (measured 4.98, 4.87, 4.68, 4.15) - against 0.6 for lights on the camera's side, whose
    rays end on their own tube - and both answers present, so that a walk which answers a constant fails."""
    n = len(S.LIGHTS)
    fl = S.flags(oracle, n).reshape(n, S.N_POINTS)
    share = fl.mean(axis=1)
    r, rec = S.rays(oracle, n), S.records(oracle, n)
    d = np.where(rec["hit"] == 1, rec["dist"].astype(np.float64) * np.linalg.norm(r["dir"].astype(np.float64), axis=1), np.nan).reshape(n, S.N_POINTS)
    med = np.nanmedian(d, axis=1)
    print(f"\noccluded share per light {np.round(share, 3).tolist()}, median distance to the occluder {np.round(med, 2).tolist()}, "
          f"90th percentile {np.round(np.nanpercentile(d, 90, axis=1), 1).tolist()}")
    assert (share >= S.OCCLUDED_FLOOR).all() and (share < 1.0).all()
    assert (med >= S.FAR_FLOOR).all()
    assert ((fl == 0).sum(axis=1) >= 100).all()                                    # the free rays: a few hundred per light, the longest of all
    assert set(np.unique(fl).tolist()) == {0, 1}
    assert np.array_equal(S.flags(oracle), fl[: S.N_LIGHTS].reshape(-1))
    assert np.isclose(np.median(S.hit_distance(oracle)), np.nanmedian(d[: S.N_LIGHTS]))


def test_no_ray_takes_the_deep_second_pass(oracle):
    """A ray whose far-only depth passes 128 is walked again by the second pass, which does not fan out: none here (measured: 32)."""
    deep = S.depths(oracle, len(S.LIGHTS))
    print(f"\ndeepest stack {int(deep.max())} of 128 entries")
    assert deep.max() <= 128 and deep.max() >= 16                                  # ... and deep enough for a fan-out to make many jobs per ray


def test_the_records_are_the_oracles_below_the_light(oracle):
    n = len(S.LIGHTS)
    rec, raw = S.records(oracle, n), oracle.trace(S.scene(oracle), S.rays(oracle, n), threads=8)[0]
    keep = (raw["hit"] == 1) & (raw["dist"] < F(1))
    assert rec[keep].tobytes() == raw[keep].tobytes() and 0 < keep.sum() < len(keep)
    miss = rec[~keep]
    assert (miss["hit"] == 0).all() and (miss["dist"] == F(1e30)).all() and (miss["instance"] == 0xffffffff).all() and (miss["triangle"] == 0xffffffff).all()


def test_the_second_ray_set(oracle):
    r, fl = S.primary_flags(oracle)
    assert len(r) == S.SIDE * S.SIDE >= S.N_POINTS and (r["_pad1"] == F(1e30)).all()
    assert S.N_POINTS <= fl.sum() < len(fl)
