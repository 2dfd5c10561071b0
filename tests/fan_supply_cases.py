"""The input of the job-supply tests of the trace fan-out (voidin_amd/csrc/trace.hip, "the supply rule").  Shared by
tests/test_fan_supply_cases.py (CPU: the properties the GPU tests rely on, from the oracle alone) and
tests/test_gpu_trace_fan_supply.py; a helper module, no tests in it.

What it is for.  Launch p >= 1 of a fanned-out call hands out JOBS, and a wave skips a job it draws when the slot is a filler or -
in the any-hit form - when the job's ray is already known to be occluded.  A wave that drew nothing but skipped jobs used to end
with supply left; when every wave ended so, the jobs behind were never walked and their rays kept the 0 of their first fan-out.
Long runs of skipped jobs need rays that (a) live long enough to fan out - kFanAge = 512 stepping iterations of their wave - and
(b) are occluded in the end, so that one job's hit kills all its ray's other jobs, the ones a launch-1 job appended for launch 2
above all.

Scene: the dense scene of tests/test_gpu_trace_range.py::test_jobs_carry_the_interval (1 500 overlapping instances of a knot and a
sphere in a 60-cube; a point of it lies inside ~23 instance boxes).  Rays: shadow rays as vd_shadow_rays_dev makes them, origin =
point + normal * 1e-4, dir = light - point, interval (0, 1) under "trace.ray_range".  Points: the hit points of the 144 x 144
primary rays of that test's camera (eye (0, 2.5, 45), looking down -z), the first N_POINTS = 16 384 of them.  Normals: the primary
ray's unit direction - the side of the surface the primary ray LEAVES through.  The walk culls back faces and these meshes are
wound so that it accepts the walls that face away from a ray's origin (a primary ray hits the far wall of a tube), so the open side
of such a point is the far one: pushed the other way, 82 - 99 % of the rays end on the near wall of their own tube within 0.6 units,
after a few dozen steps, and never fan out.  Lights: LIGHTS, behind the cluster as the camera sees it, so that a shadow ray
goes on through ~50 more units of it: 94 - 98 % are occluded, at a median of 4 - 5 units and a 90th percentile of 21 - 25 from their point,
after the boxes of 49 (median) to 200 (90th percentile) instances; the 2 % that reach the light cross 170 - 270 boxes.  (The
figures are printed and pinned by tests/test_fan_supply_cases.py.)

Rays are light-major, ray l * N_POINTS + p, as vd_shadow_pass*_dev traces them.  rays(oracle, n_lights) gives the first
n_lights * N_POINTS; N_LIGHTS says how many the GPU tests use (the smallest count at which the walk before the supply rule
failed: profiles/trace_fan_supply.md).  Expected flag of a ray: the oracle's closest hit lies on the open segment - hit and
dist < 1 (the rule tests/test_shadow_pass_cases.py::test_the_record_is_the_brute_forces_answer holds against the brute force).
It takes 0.4 s per light on 8 threads, so nothing is recorded.  Everything is computed once per process and shared: nobody changes
what these functions return."""
import numpy as np

from voidin_amd import abi, synth
from wide_scenes import mesh_set

F = np.float32
SEED = synth.SEED_BASE + 8
SIDE = 144
N_POINTS = 16384                   # one ray per lane of a grid of one wave per CU (256 CUs x 64): the least that may fan out
LIGHTS = np.array([[0.0, 2.5, -90.0], [20.0, 10.0, -80.0], [-25.0, -5.0, -85.0], [0.0, 60.0, -60.0]], F)
N_LIGHTS = 2                       # what the GPU tests trace: 32 768 rays
OCCLUDED_FLOOR = 0.9               # "most rays are occluded": measured 0.979 / 0.984 / 0.981 / 0.941 per light
FAR_FLOOR = 2.0                    # ... "and far along the ray": the median distance from the point to the hit, in world units (measured 4.2 - 5.0)
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def scene(oracle):
    def make():
        infos, B, V, I = mesh_set(oracle, [synth.knot_mesh(64, 16), synth.uv_sphere(1.0, 6)])
        inst = synth.instances(1500, n_mesh=2, seed=SEED, extent=60.0, scale_range=(0.5, 2.0))
        return (oracle.tlas_build(inst, infos), inst, infos, B, V, I)
    return _once("scene", make)


def primary(oracle):
    """The primary rays the points come from: a second ray set of another kind for the tests that alternate calls."""
    return _once("primary", lambda: oracle.primary_rays(synth.camera_uniform(eye=(0, 2.5, 45.0), pitch_deg=0), SIDE, SIDE))


def points(oracle):
    """-> (positions [N_POINTS][3], normals [N_POINTS][3])."""
    def make():
        rays = primary(oracle)
        want, _ = oracle.trace(scene(oracle), rays, threads=8)
        hit = want["hit"] == 1
        assert hit.sum() >= N_POINTS, int(hit.sum())
        pos = (rays["eye"] + rays["dir"] * want["dist"][:, None])[hit][:N_POINTS]
        nor = rays["dir"][hit][:N_POINTS].astype(np.float64)
        nor /= np.linalg.norm(nor, axis=1)[:, None]
        return np.ascontiguousarray(pos, F), np.ascontiguousarray(nor, F)
    return _once("points", make)


def lights(n_lights=N_LIGHTS):
    """LIGHT records with a radius that puts every point in range."""
    out = np.zeros(n_lights, dtype=abi.LIGHT)
    out["position"], out["radius"] = LIGHTS[:n_lights], 1e6
    return out


def rays(oracle, n_lights=N_LIGHTS):
    """The shadow rays of the first n_lights lights, light-major, with the interval (0, 1) in the pad fields."""
    def make():
        pos, nor = points(oracle)
        r = np.concatenate([oracle.shadow_rays(pos, nor, LIGHTS[l]) for l in range(len(LIGHTS))])
        r["_pad0"], r["_pad1"] = 0.0, 1.0
        return r
    return _once("rays", make)[: n_lights * N_POINTS]


def _walked(oracle):
    """(closest-hit records, far-only stack depth) of all len(LIGHTS) * N_POINTS rays."""
    def make():
        rec, _, far = oracle.trace(scene(oracle), rays(oracle, len(LIGHTS)), threads=8, depths=True)
        return rec, far
    return _once("walked", make)


def records(oracle, n_lights=N_LIGHTS):
    """The closest-hit records vd_trace*_dev gives these rays under the interval (0, 1): the oracle's where its hit lies below 1,
    the miss record elsewhere (an interval with only an upper end keeps the closest hit or nothing)."""
    def make():
        rec = _walked(oracle)[0].copy()
        gone = ~((rec["hit"] == 1) & (rec["dist"] < F(1)))
        rec["hit"][gone], rec["dist"][gone], rec["instance"][gone], rec["triangle"][gone] = 0, F(1e30), 0xffffffff, 0xffffffff
        return rec
    return _once("records", make)[: n_lights * N_POINTS]


def flags(oracle, n_lights=N_LIGHTS):
    """uint32 per ray: 1 = something lies on the open segment between the point and the light."""
    return np.ascontiguousarray(records(oracle, n_lights)["hit"]).astype(np.uint32)


def depths(oracle, n_lights=N_LIGHTS):
    return _walked(oracle)[1][: n_lights * N_POINTS]


def hit_distance(oracle, n_lights=N_LIGHTS):
    """World-space distance from the point to the closest occluder, for the occluded rays."""
    r, rec = rays(oracle, n_lights), records(oracle, n_lights)
    occ = rec["hit"] == 1
    return (rec["dist"][occ].astype(np.float64) * np.linalg.norm(r["dir"][occ].astype(np.float64), axis=1))


def primary_flags(oracle):
    """The any-hit flags of the primary rays (the second ray set), pads (0, 1e30)."""
    def make():
        r = primary(oracle).copy()
        r["_pad0"], r["_pad1"] = 0.0, 1e30
        return r, oracle.trace(scene(oracle), r, threads=8)[0]["hit"].astype(np.uint32)
    return _once("primary_flags", make)
