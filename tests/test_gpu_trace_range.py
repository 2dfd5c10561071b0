"""VD_OPT_TRACE_RAY_RANGE ("trace.ray_range"): every vd_trace* call reads VdRay::_pad0 / _pad1 as the ray's interval (t_min, t_max)
- include/voidin_abi.h, "Ray intervals" has the definition.  Expected records: the oracle where the interval cannot matter, the brute
force of tests/trace_range_cases.py where it does (dist and hit bit for bit; instance and triangle where one triangle decides).
Every call here writes between canary rows, which must survive it."""
import numpy as np
import pytest

import trace_range_cases as cases
from voidin_amd import abi, synth
from voidin_amd.runtime import set_ray_range
from wide_scenes import mesh_set, widen

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 8                                     # canary rows in front of and behind every output
DEV_FORMS = ("dev", "indexed", "prepared", "tight", "wide", "wide_indexed", "wide_prepared")
HOST_FORMS = ("host", "host_wide")


class Rig:
    """One scene on the device in every shape a trace call takes: narrow and wide nodes (the same topology: wide_scenes.widen),
    prepared plain, prepared with a private LBVH top level (VD_OPT_TRACE_TIGHT_TLAS = 2) and prepared wide."""

    def __init__(self, ctx, scene):
        self.ctx, self.scene = ctx, scene
        self.wide_scene = (widen(scene[0]),) + tuple(scene[1:])
        self.ds, self.dw = ctx.device_scene(scene), ctx.device_scene(self.wide_scene)
        self.acc = ctx.trace_prepare(self.ds)
        ctx.set_option("trace.tight_tlas", 2)
        try:
            self.acc_tight = ctx.trace_prepare(self.ds)
        finally:
            ctx.set_option("trace.tight_tlas", None)
        self.acc_wide = ctx.trace_prepare(self.dw)

    def close(self):
        for a in (self.acc, self.acc_tight, self.acc_wide):
            a.close()

    def run(self, form, rays, ctx_options, closest=True, any_hit=True):
        """-> (records or None, flags or None) of one form; the canary rows around both outputs are checked."""
        import torch
        ctx, n = self.ctx, len(rays)
        if form in HOST_FORMS:
            return (ctx.trace(self.scene, rays) if form == "host" else ctx.trace_wide(self.wide_scene, rays)), None
        ctx_options("trace.auto_prepare", 0 if form.endswith("indexed") else None)
        d_rays = ctx.upload(rays)
        d_hits = torch.full(((n + 2 * PAD) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        d_any = torch.full((n + 2 * PAD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        hits, flags = d_hits[PAD * 16:], d_any[PAD:]
        if form in ("dev", "indexed"):
            call, call_any, arg = ctx.trace_dev, ctx.trace_any_dev, self.ds
        elif form in ("wide", "wide_indexed"):
            call, call_any, arg = ctx.trace_wide_dev, ctx.trace_any_wide_dev, self.dw
        else:
            call, call_any = ctx.trace_prepared_dev, ctx.trace_any_prepared_dev
            arg = {"prepared": self.acc, "tight": self.acc_tight, "wide_prepared": self.acc_wide}[form]
        if closest:
            call(arg, d_rays, n, hits)
        if any_hit:
            call_any(arg, d_rays, n, flags)
        torch.cuda.synchronize()
        h, a = d_hits.cpu().numpy(), d_any.cpu().numpy()
        assert (h[: PAD * 16] == 0xA5).all() and (h[(PAD + n) * 16:] == 0xA5).all(), f"{form}: a record outside the call's {n}"
        assert (a[:PAD] == 0x5A5A5A5A).all() and (a[PAD + n:] == 0x5A5A5A5A).all(), f"{form}: a flag outside the call's {n}"
        rec = h[PAD * 16: (PAD + n) * 16].view(abi.HIT).copy() if closest else None
        if not closest:
            assert (h == 0xA5).all()
        return rec, (a[PAD: PAD + n].astype(np.uint32) if any_hit else None)


@pytest.fixture(scope="module")
def rigs(ctx, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Rig(ctx, cases.case(name, oracle).scene)
        return made[name]
    yield get
    for r in made.values():
        r.close()


def bad_rows(got, want, rows=None):
    """Indices where the four words differ (of `rows`: a mask; default all)."""
    d = (got["dist"].view(np.uint32) != want["dist"].view(np.uint32)) | (got["hit"] != want["hit"]) | \
        (got["instance"] != want["instance"]) | (got["triangle"] != want["triangle"])
    return np.flatnonzero(d if rows is None else d & rows)


def check(got, flags, e, what):
    """A call's records / flags against the brute force's answer under the reporting rule."""
    if got is not None:
        bad = np.flatnonzero((got["dist"].view(np.uint32) != e.records["dist"].view(np.uint32)) | (got["hit"] != e.records["hit"]))
        assert bad.size == 0, (what, "dist / hit", bad.size, bad[:5].tolist(), got[bad[:3]].tolist(), e.records[bad[:3]].tolist())
        bad = bad_rows(got, e.records, e.unique)
        assert bad.size == 0, (what, "instance / triangle", bad.size, bad[:5].tolist(), got[bad[:3]].tolist(), e.records[bad[:3]].tolist())
    if flags is not None:
        bad = np.flatnonzero(flags != e.records["hit"])
        assert bad.size == 0, (what, "any-hit flag", bad.size, bad[:5].tolist())


# ---- 1. identity ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.NAMES)
def test_the_whole_half_line_gives_the_bytes_of_the_default(ctx, ctx_options, oracle, rigs, name):
    """Option on, pads (0, 1e30): byte for byte what the option off gives - narrow and wide, plain, indexed and prepared (with a
    private top level too), closest and any, the host forms; on the chain scene through the deep second pass.  And with the option
    off the pads are ignored, whatever they hold."""
    c, rig = cases.case(name, oracle), rigs(name)
    full = cases.with_range(c.rays, 0.0, 1e30)
    junk = cases.with_range(c.rays, c.t_min, c.t_max)
    for form in DEV_FORMS + HOST_FORMS:
        ctx_options("trace.ray_range", 0)
        base, base_any = rig.run(form, c.rays, ctx_options)
        if form != "tight":                                                   # (its own visit order: ties may name another triangle)
            assert base.tobytes() == c.want.tobytes(), form
        ign, ign_any = rig.run(form, junk, ctx_options)
        ctx_options("trace.ray_range", 1)
        on, on_any = rig.run(form, full, ctx_options)
        assert on.tobytes() == base.tobytes() and ign.tobytes() == base.tobytes(), form
        if form in DEV_FORMS:
            assert np.array_equal(base_any, c.want["hit"]) and np.array_equal(on_any, base_any) and np.array_equal(ign_any, base_any), form


# ---- 2. / 3. one bound, exact from the oracle -----------------------------------------------------------------------------------

def _around(d):
    """The values a bound is tried at for a ray whose oracle distance is d."""
    with np.errstate(over="ignore"):
        return {"d": d, "next above d": np.nextafter(d, F(np.inf)), "next below d": np.nextafter(d, F(0)), "d / 2": (d / F(2)).astype(F),
                "2 d": (d * F(2)).astype(F)}


@pytest.mark.parametrize("name", cases.NAMES)
def test_upper_bound_exact_from_the_oracle(ctx, ctx_options, oracle, rigs, name):
    """t_max at, one float around, half and twice each ray's oracle distance d: the oracle's record - all four words - when
    d < t_max, the miss record otherwise.  (The end is exclusive: t_max = d loses the hit.)"""
    c, rig = cases.case(name, oracle), rigs(name)
    ctx_options("trace.ray_range", 1)
    d = c.want["dist"]
    for label, t_max in _around(d).items():
        want = c.want.copy()
        want[~((c.want["hit"] == 1) & (d < np.fmin(t_max, F(1e30))))] = c.miss_record()
        assert want["hit"].sum() == (c.want["hit"].sum() if label in ("next above d", "2 d") else 0)
        rays = cases.with_range(c.rays, 0.0, t_max)
        for form in DEV_FORMS + (HOST_FORMS if label == "next above d" else ()):
            got, flags = rig.run(form, rays, ctx_options)
            bad = bad_rows(got, want)
            assert bad.size == 0, (label, form, bad.size, bad[:5].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist())
            assert flags is None or np.array_equal(flags, want["hit"]), (label, form)
    assert c.want["hit"].sum() > 100


@pytest.mark.parametrize("name", cases.NAMES)
def test_lower_bound(ctx, ctx_options, oracle, rigs, name):
    """t_min at, one float around, half and twice d.  Where d > t_min the oracle's record is expected in all four words; where
    d <= t_min - t_min == d included: that end is exclusive too - the first hit is gone and the brute force decides."""
    c, rig = cases.case(name, oracle), rigs(name)
    ctx_options("trace.ray_range", 1)
    d = c.want["dist"]
    for k, (label, t_min) in enumerate(_around(d).items()):
        t_max = np.full(len(d), np.inf if k % 2 else 1e30, F)
        e = cases.expected(c.hits, t_min, t_max, c.miss_record())
        keeps = (c.want["hit"] == 1) & (d > t_min)
        rays = cases.with_range(c.rays, t_min, t_max)
        for form in DEV_FORMS + (HOST_FORMS if label == "d" else ()):
            got, flags = rig.run(form, rays, ctx_options)
            bad = bad_rows(got, c.want, keeps)
            assert bad.size == 0, (label, form, "the first hit survives", bad.size, bad[:5].tolist(), got[bad[:3]].tolist(), c.want[bad[:3]].tolist())
            check(got, flags, e, (label, form))
        if label in ("d", "next above d", "2 d"):
            assert not keeps.any()
        if label in ("d", "next above d"):
            assert (e.records["hit"] == 1).sum() > 20                            # later hits take over


# ---- 4. / 5. both bounds, closest and any, every form ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.NAMES)
def test_intervals_around_the_first_two_hits(ctx, ctx_options, oracle, rigs, name):
    """Random intervals placed around each ray's first two intersections (trace_range_cases.intervals; the classes are counted
    in tests/test_trace_range_cases.py): the closest hit inside, and the any-hit flag = that record's `hit`, on every form.  On the
    chain scene the rays whose first hit is cut away hold more than 128 entries: the deep second pass walks them again, with the
    same interval."""
    c, rig = cases.case(name, oracle), rigs(name)
    ctx_options("trace.ray_range", 1)
    e = cases.expected(c.hits, c.t_min, c.t_max, c.miss_record())
    assert 0 < e.records["hit"].sum() < len(c.rays) and not np.array_equal(e.records["hit"], c.want["hit"])
    rays = cases.with_range(c.rays, c.t_min, c.t_max)
    for form in DEV_FORMS + HOST_FORMS:
        got, flags = rig.run(form, rays, ctx_options)
        check(got, flags, e, form)
        if got is not None:
            assert (got["dist"][got["hit"] == 0] == F(1e30)).all()           # a miss never reports t_max
    # the flag alone (no closest-hit call before it in the stream)
    for form in ("prepared", "wide_prepared", "dev"):
        _, flags = rig.run(form, rays, ctx_options, closest=False)
        check(None, flags, e, (form, "any only"))


# ---- 6. field normalisation -----------------------------------------------------------------------------------------------------

def test_odd_values_in_the_fields(ctx, ctx_options, oracle, rigs):
    """NaN, negative, -0.0 and +inf in either field, t_max <= t_min, t_max = 0: the defined result (a NaN or negative t_min is 0,
    a NaN or oversized t_max is 1e30, everything else stays and misses), VD_OK and no error flag - a failing call raises."""
    c, rig = cases.case("seeded", oracle), rigs("seeded")
    ctx_options("trace.ray_range", 1)
    d = c.want["dist"]
    nan, inf = F(np.nan), F(np.inf)
    specials = [(nan, 1e30), (-1.0, 1e30), (-0.0, 1e30), (inf, 1e30), (-inf, inf), (0.0, nan), (0.0, -1.0), (0.0, -0.0), (0.0, 0.0), (0.0, inf), (0.0, 3e38),
                (5.0, 3.0), (nan, nan), (inf, -inf), (-nan, -nan), (1e30, 1e30)]
    n = len(c.rays)
    which = np.arange(n) % (len(specials) + 1)
    t_min = np.array([s[0] for s in specials] + [0.0], F)[which]
    t_max = np.array([s[1] for s in specials] + [0.0], F)[which]
    last = which == len(specials)
    t_min[last], t_max[last] = d[last], d[last]                               # t_max == t_min == the hit itself
    e = cases.expected(c.hits, t_min, t_max, c.miss_record())
    full = np.isin(which, [0, 1, 2, 4, 5, 9, 10, 12, 14])                     # these read as (0, 1e30)
    assert e.records[full].tobytes() == c.want[full].tobytes() and (e.records["hit"][~full] == 0).all() and e.records["hit"].sum() > 500
    rays = cases.with_range(c.rays, t_min, t_max)
    for form in DEV_FORMS + HOST_FORMS:
        got, flags = rig.run(form, rays, ctx_options)
        check(got, flags, e, form)


# ---- 7. the fan-out and a full job list, with real intervals ----------------------------------------------------------------------

def test_a_call_large_enough_to_fan_out(ctx, ctx_options, oracle, rigs):
    """421 888 rays (the seeded scene's, 103 times over, every copy with its own intervals) - one ray per lane of the persistent
    grid and more.  VD_OPT_TRACE_FAN 3 against 1, and 3 with a job list of 1000 slots (it fills up: waves keep their rays): the
    same bytes, which are the brute force's; and the whole half-line still gives the bytes of the option off."""
    c, rig = cases.case("seeded", oracle), rigs("seeded")
    rays, t_min, t_max, ray_of = cases.big_call(c, 103, cases.SEED + 50)
    e = cases.expected(c.hits, t_min, t_max, c.miss_record(), ray_of)
    ranged = set_ray_range(rays.copy(), t_min, t_max)
    for form in ("prepared", "dev"):
        first = None
        for fan, slots in ((1, None), (3, None), (3, 1000)):
            ctx_options("trace.fan", fan)
            ctx_options("trace.fan_slots", slots)
            ctx_options("trace.ray_range", 1)
            got, flags = rig.run(form, ranged, ctx_options)
            if first is None:
                first = (got.tobytes(), flags.tobytes())
                check(got, flags, e, (form, fan))
            assert (got.tobytes(), flags.tobytes()) == first, (form, fan, slots)
        ctx_options("trace.fan_slots", None)
        for fan in (1, 3):                                                    # identity at this size, one launch and fanned out
            ctx_options("trace.fan", fan)
            ctx_options("trace.ray_range", 1)
            on, on_any = rig.run(form, set_ray_range(rays.copy(), 0.0, 1e30), ctx_options)
            ctx_options("trace.ray_range", 0)
            off, off_any = rig.run(form, rays, ctx_options)
            assert on.tobytes() == off.tobytes() and np.array_equal(on_any, off_any), (form, fan)
            assert off[:4096].tobytes() == c.want.tobytes()


def test_jobs_carry_the_interval(ctx, ctx_options, oracle):
    """A dense scene (1 500 overlapping instances: rays of thousands of steps) under 16 384 rays and a grid of one wave per CU, the
    setting in which draining waves turn rays into jobs (tests/test_gpu_trace_wide.py).  A job holds the ray's upper end as its
    starting distance and reads the lower end from the ray again: 2, 3 and 4 launches give the bytes of one launch, for intervals
    that cut each ray's first hit away (t_min between 1 and 1.5 times the unbounded distance; every other ray ends at 3 times),
    and every 32nd ray's record is the brute force's.  That jobs were made leaves no trace in the ABI (same bytes by design); the
    times of the any-hit calls by launches are printed, as tests/test_gpu_trace_wide.py does."""
    infos, B, V, I = mesh_set(oracle, [synth.knot_mesh(64, 16), synth.uv_sphere(1.0, 6)])
    inst = synth.instances(1500, n_mesh=2, seed=synth.SEED_BASE + 8, extent=60.0, scale_range=(0.5, 2.0))
    scene = (oracle.tlas_build(inst, infos), inst, infos, B, V, I)
    rig = Rig(ctx, scene)
    ctx.set_timing(True)
    try:
        rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 45.0), pitch_deg=0), 128, 128)
        ctx_options("trace.waves", 1)
        ctx_options("trace.fan", 1)
        ctx_options("trace.ray_range", 0)
        off, _ = rig.run("prepared", rays, ctx_options)
        assert off["hit"].sum() > 3000
        rng = np.random.default_rng(cases.SEED + 60)
        d = np.where(off["hit"] == 1, off["dist"], F(10)).astype(F)
        t_min = (d * (F(1) + F(0.5) * rng.random(len(rays)).astype(F))).astype(F)
        t_max = np.where(np.arange(len(rays)) % 2 == 0, F(1e30), d * F(3)).astype(F)
        ranged = set_ray_range(rays.copy(), t_min, t_max)
        sub = np.arange(0, len(rays), 32)                                      # an expectation of its own for a sample of the rays
        miss = off[off["hit"] == 0][0]
        e = cases.expected(cases.brute_force(scene, rays[sub]), t_min[sub], t_max[sub], miss)
        assert (e.records["hit"] == 1).sum() > 30 and (e.records["hit"] == 0).sum() > 30
        ctx_options("trace.ray_range", 1)
        ms = {}
        for form in ("prepared", "wide_prepared", "indexed"):
            first = None
            for fan in (1, 2, 3, 4):
                ctx_options("trace.fan", fan)
                got, flags = rig.run(form, ranged, ctx_options)
                ms[(form, fan)] = round(ctx.last_gpu_ms(), 3)
                check(got[sub], flags[sub], e, (form, fan, "every 32nd ray"))
                if first is None:
                    first = (got.tobytes(), flags.tobytes())
                    hit = got["hit"] == 1
                    assert hit.sum() > 1000 and (got["dist"][hit] > t_min[hit]).all() and (got["dist"][hit] < t_max[hit]).all()
                    assert (got["dist"][~hit] == F(1e30)).all() and np.array_equal(flags, got["hit"])
                assert (got.tobytes(), flags.tobytes()) == first, (form, fan)
        print(f"\n1500 instances, 16384 rays with intervals, any-hit call ms by (form, launches): {ms}")
    finally:
        ctx.set_timing(False)
        rig.close()


# ---- 8. the generators ----------------------------------------------------------------------------------------------------------

def test_generators_write_the_interval_under_the_option(ctx, ctx_options, oracle):
    import torch
    c = cases.case("seeded", oracle)
    hit = c.want["hit"] == 1
    pts = (c.rays["eye"] + c.rays["dir"] * c.want["dist"][:, None])[hit].astype(F)
    nor = (-c.rays["dir"][hit]).astype(F)
    light = np.array([3.0, 40.0, 20.0], F)
    cam = synth.camera_uniform(eye=(0, 2.5, 40), pitch_deg=0)
    want_shadow, want_primary = oracle.shadow_rays(pts, nor, light), oracle.primary_rays(cam, 64, 48)
    d_pts, d_nor = ctx.upload(pts), ctx.upload(nor)
    for on, pads_shadow, pads_primary in ((0, (0.0, 0.0), (0.0, 0.0)), (1, (0.0, 1.0), (0.0, 1e30))):
        ctx_options("trace.ray_range", on)
        d_sr = torch.full(((len(pts) + 2 * PAD) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.shadow_rays_dev(d_pts, d_nor, len(pts), light, d_sr[PAD * 32:])
        d_pr = torch.full(((64 * 48 + 2 * PAD) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.primary_rays_dev(cam, 64, 48, d_pr[PAD * 32:])
        torch.cuda.synchronize()
        host = np.zeros(64 * 48, dtype=abi.RAY)
        ctx._chk(ctx.lib.vd_primary_rays(ctx.h, np.ascontiguousarray(cam, dtype=abi.CAMERA).ctypes.data, 64, 48, host.ctypes.data))
        for what, raw, want, pads in (("shadow", d_sr.cpu().numpy(), want_shadow, pads_shadow), ("primary", d_pr.cpu().numpy(), want_primary, pads_primary)):
            n = len(want)
            assert (raw[: PAD * 32] == 0xA5).all() and (raw[(PAD + n) * 32:] == 0xA5).all(), what
            got = raw[PAD * 32: (PAD + n) * 32].view(abi.RAY)
            assert got["eye"].tobytes() == want["eye"].tobytes() and got["dir"].tobytes() == want["dir"].tobytes(), (what, on)
            assert (got["_pad0"].view(np.uint32) == F(pads[0]).view(np.uint32)).all() and (got["_pad1"].view(np.uint32) == F(pads[1]).view(np.uint32)).all(), (what, on)
            if not on:
                assert got.tobytes() == want.tobytes(), what                  # all 32 bytes are today's
        assert host.tobytes() == d_pr.cpu().numpy()[PAD * 32: (PAD + 64 * 48) * 32].tobytes(), on


# ---- 9. the point of it ---------------------------------------------------------------------------------------------------------

def test_an_occluder_behind_the_light_no_longer_shadows(ctx, ctx_options, oracle):
    """The shadow pass (vd_shadow_rays_dev, then any-hit) on trace_range_cases.shadow_scene: by default the sphere BEHIND the light
    shadows point 0 - the reference's behaviour, asserted - and under the option it does not; the sphere between point 1 and the
    light shadows it either way.  Through the plain, the prepared and the wide any-hit call."""
    import torch
    scene, pos, nor, light = cases.shadow_scene(oracle)
    rig = Rig(ctx, scene)
    try:
        for on, want in ((0, [1, 1]), (1, [0, 1])):
            ctx_options("trace.ray_range", on)
            d_sr = ctx.empty(2 * 32)
            ctx.shadow_rays_dev(ctx.upload(pos), ctx.upload(nor), 2, light, d_sr)
            for call, arg in ((ctx.trace_any_dev, rig.ds), (ctx.trace_any_prepared_dev, rig.acc), (ctx.trace_any_wide_dev, rig.dw),
                              (ctx.trace_any_prepared_dev, rig.acc_wide), (ctx.trace_any_prepared_dev, rig.acc_tight)):
                d_occ = torch.full((2,), 7, dtype=torch.int32, device="cuda")
                call(arg, d_sr, 2, d_occ)
                torch.cuda.synchronize()
                assert d_occ.cpu().numpy().tolist() == want, (on, call.__name__)
    finally:
        rig.close()
