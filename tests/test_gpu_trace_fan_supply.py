"""The job supply of the trace fan-out (voidin_amd/csrc/trace.hip: "a wave ends only when its launch's supply is exhausted") on the
input of tests/fan_supply_cases.py: 32 768 shadow rays of the dense scene, 98 % of them occluded far from their point, under
"trace.waves" = 1 (a grid of one wave per CU: 16 384 lanes, so the call may fan out) and "trace.ray_range" = 1.

1. Supply invariants, tuning build (vd_debug_trace_fan, in a child process that loads libvoidin_hip_tuning.so as
   tests/test_gpu_scan_fault.py does): after every fanned call jobs were made, every position of every job launch was drawn, no
   wave left with supply behind it, and the flags / records are the oracle's.
2. Same bytes, production build: 2, 3 and 4 launches against one and against the oracle, EVERY ray, prepared, plain and indexed,
   each fanned call repeated and alternated with a call on a second ray set - the loss was timing-dependent.
3. The shadow pass on these points and lights under the library's default fan-out against the per-light loop of one launch.

Before the supply rule (the parent's kernels with only the counter added), on an MI355X (profiles/trace_fan_supply.md has the
tables): in every any-hit call of 3 or 4 launches, and in the shadow pass, 3 to 11 waves ended with supply left (0 with 2 launches and in
the closest-hit call) - test 1 failed in 7 of 7 runs, at 16 384, 32 768 and 65 536 rays.  Every position was drawn all the same (the
supply of launch 2, ~5 500 jobs, is smaller than the grid's first draw of 16 384) and no flag differed, so tests 2 and 3 passed at the
parent in 3 of 3 runs: at this size they are guards, and REPEATS is small.  The loss itself needs a job launch whose dead tail is
longer than what the grid draws at once; it shows at 770 743 rays a call on 393 216 lanes (17 of 49.3 M pairs before, 0 after).
JOB_FACTOR: a call that appends fewer jobs than the grid has lanes hands every job out in its first draw; measured 1.58 (2 launches)
to 1.93 (4 launches) at 32 768 rays, and 0.77 to 0.94 at 16 384, which is why the tests trace two lights."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import fan_supply_cases as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

CSRC = os.path.join(ROOT, "voidin_amd", "csrc")
TUNING = os.path.join(CSRC, "libvoidin_hip_tuning.so")
REPEATS = 3                      # fanned calls per (form, launches) in the byte test, each followed by a call on the second ray set
JOB_FACTOR = 1                   # jobs appended >= JOB_FACTOR x waves x 64: a list that the grid's first draw cannot empty

# The child prints one line of figures per call BEFORE it judges, collects what is wrong and fails at the end with all of it.
CHILD = textwrap.dedent("""
    import ctypes as C, json, sys
    import numpy as np
    import torch
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    from oracle import ref
    import fan_supply_cases as S
    from voidin_amd import abi
    from voidin_amd.runtime import Context
    ref.load()
    N_LIGHTS, JOB_FACTOR = %(n_lights)d, %(job_factor)d
    ctx = Context(0)
    lib = ctx.lib
    lib.vd_debug_trace_fan.restype = C.c_int
    lib.vd_debug_trace_fan.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    rays, want, rec = S.rays(ref, N_LIGHTS), S.flags(ref, N_LIGHTS), S.records(ref, N_LIGHTS)
    n = len(rays)
    ds = ctx.device_scene(S.scene(ref))
    acc = ctx.trace_prepare(ds)
    d_rays = ctx.upload(rays)
    ctx.set_option("trace.waves", 1)
    ctx.set_option("trace.ray_range", 1)
    wrong = []

    def supply(what, launches):
        w = (C.c_uint32 * 16)()
        assert lib.vd_debug_trace_fan(ctx.h, w) == 0
        w = list(w)
        early, ran, lanes, slots, jobs = w[0], w[1], w[2] * 64, w[3], w[4]
        size = [w[8 + p] - w[8 + p - 1] for p in range(1, ran)]
        undrawn = [max(0, size[p - 1] - w[4 + p]) for p in range(1, ran)]
        fig = {"call": what, "launches": ran, "lanes": lanes, "jobs": jobs, "factor": round(jobs / lanes, 2), "slots": slots,
               "supply": size, "undrawn": undrawn, "early_ends": early}
        if ran != launches: wrong.append((what, "launches", ran))
        if lanes != 16384: wrong.append((what, "lanes", lanes))
        if jobs < JOB_FACTOR * lanes: wrong.append((what, "jobs", jobs, "wanted at least", JOB_FACTOR * lanes))
        if any(undrawn): wrong.append((what, "positions never drawn, by launch", undrawn))
        if early: wrong.append((what, "waves that ended with supply left", early))
        return fig

    for launches in (2, 3, 4):
        ctx.set_option("trace.fan", launches)
        for form in ("prepared", "plain"):
            d_any = torch.full((n,), 7, dtype=torch.int32, device="cuda")
            if form == "prepared": ctx.trace_any_prepared_dev(acc, d_rays, n, d_any)
            else: ctx.trace_any_dev(ds, d_rays, n, d_any)
            torch.cuda.synchronize()
            fig = supply("any %%s %%d" %% (form, launches), launches)
            bad = np.flatnonzero(d_any.cpu().numpy().astype(np.uint32) != want)
            fig["flags_differ"] = int(bad.size)
            print(json.dumps(fig), flush=True)
            if bad.size: wrong.append((fig["call"], "flags differ from the oracle's", int(bad.size), bad[:5].tolist()))
    # closest hit, once: same invariants, the oracle's records in all four words
    ctx.set_option("trace.fan", 3)
    d_hits = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device="cuda")
    ctx.trace_prepared_dev(acc, d_rays, n, d_hits)
    torch.cuda.synchronize()
    fig = supply("closest prepared 3", 3)
    got = d_hits.cpu().numpy().view(abi.HIT)
    bad = np.flatnonzero((got["hit"] != rec["hit"]) | (got["dist"].view(np.uint32) != rec["dist"].view(np.uint32)) |
                         (got["instance"] != rec["instance"]) | (got["triangle"] != rec["triangle"]))
    fig["records_differ"] = int(bad.size)
    print(json.dumps(fig), flush=True)
    if bad.size: wrong.append((fig["call"], "records differ from the oracle's", int(bad.size), bad[:5].tolist(), got[bad[:2]].tolist(), rec[bad[:2]].tolist()))
    # the shadow pass under the library's default: it is this walk, three launches, and it makes jobs
    ctx.set_option("trace.fan", None)
    pos, nor = S.points(ref)
    lts = S.lights(N_LIGHTS)
    d_occ = torch.full((S.N_POINTS,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    info = ctx.shadow_pass_prepared_dev(acc, ctx.upload(pos), ctx.upload(nor), S.N_POINTS, ctx.upload(lts), N_LIGHTS, d_occ)
    torch.cuda.synchronize()
    fig = supply("shadow pass, default fan", 3)
    words = d_occ.cpu().numpy().astype(np.uint32)
    bits = ((words[:, None] >> np.arange(N_LIGHTS, dtype=np.uint32)[None, :]) & 1).T.reshape(-1)
    fig["flags_differ"] = int((bits != want).sum())
    print(json.dumps(fig), flush=True)
    if info["n_chunks"] != 1 or info["n_rays"] != n: wrong.append(("shadow pass", info))
    if fig["flags_differ"]: wrong.append(("shadow pass", "bits differ from the oracle's", fig["flags_differ"]))
    acc.close()
    assert not wrong, wrong
    print("fan supply test OK")
""")


def child_source(n_lights=S.N_LIGHTS, job_factor=JOB_FACTOR):
    return CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "n_lights": n_lights, "job_factor": job_factor}


def test_every_job_is_drawn_and_no_wave_ends_with_supply_left():
    src_newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp")))
    if not os.path.exists(TUNING) or os.path.getmtime(TUNING) < src_newest:
        subprocess.run(["make", "-C", CSRC, "tuning"], check=True, capture_output=True, timeout=1200)
    env = dict(os.environ, VOIDIN_HIP_LIB=TUNING)
    out = subprocess.run([sys.executable, "-c", child_source()], env=env, capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "fan supply test OK" in out.stdout, out.stdout[-3000:] + out.stderr[-4000:]


class Rig:
    def __init__(self, ctx, oracle):
        self.ctx = ctx
        self.ds = ctx.device_scene(S.scene(oracle))
        self.acc = ctx.trace_prepare(self.ds)
        self.rays, self.want = S.rays(oracle), S.flags(oracle)
        self.rays_b, self.want_b = S.primary_flags(oracle)
        self.d_rays, self.d_rays_b = ctx.upload(self.rays), ctx.upload(self.rays_b)

    def any_hit(self, form, second=False):
        """The flags of one any-hit call of `form` on the shadow rays (second: on the primary rays), on the context as it is set."""
        import torch
        d_rays, n = (self.d_rays_b, len(self.rays_b)) if second else (self.d_rays, len(self.rays))
        d_any = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        if form == "prepared":
            self.ctx.trace_any_prepared_dev(self.acc, d_rays, n, d_any)
        else:
            self.ctx.trace_any_dev(self.ds, d_rays, n, d_any)
        return d_any.cpu().numpy().astype(np.uint32)


@pytest.fixture(scope="module")
def rig(ctx, oracle):
    r = Rig(ctx, oracle)
    yield r
    r.acc.close()


@pytest.mark.parametrize("form", ["prepared", "plain", "indexed"])
def test_fanned_any_hit_calls_give_the_flags_of_one_launch(ctx, ctx_options, rig, form):
    """2, 3 and 4 launches against one launch and against the oracle, every ray, REPEATS times each, every fanned call followed by
    a call on the primary rays (another supply in the same arena), whose flags are held against the oracle too."""
    ctx_options("trace.waves", 1)
    ctx_options("trace.ray_range", 1)
    ctx_options("trace.auto_prepare", 0 if form == "indexed" else None)
    ctx_options("trace.fan", 1)
    one = rig.any_hit(form)
    assert np.array_equal(one, rig.want), (form, "one launch against the oracle", int((one != rig.want).sum()))
    assert np.array_equal(rig.any_hit(form, second=True), rig.want_b), (form, "one launch, second ray set")
    differ = {}
    for launches in (2, 3, 4):
        ctx_options("trace.fan", launches)
        for k in range(REPEATS):
            got, got_b = rig.any_hit(form), rig.any_hit(form, second=True)
            differ[(launches, k)] = (int((got != one).sum()), int((got_b != rig.want_b).sum()))
    print(f"\n{form}: flags that differ from one launch's (shadow rays, primary rays) by (launches, repeat): {differ}")
    assert not any(a or b for a, b in differ.values()), (form, differ)


def test_the_shadow_pass_under_the_default_fan_out_equals_the_loop_of_one_launch(ctx, ctx_options, oracle, rig):
    """vd_shadow_pass_prepared_dev on these points and lights (every pair in range: one chunk of 32 768 rays) with "trace.fan" left
    to the library against per light vd_shadow_rays_dev + vd_trace_any_prepared_dev with "trace.fan" = 1: every bit."""
    import torch
    ctx_options("trace.waves", 1)
    ctx_options("trace.ray_range", 1)
    pos, nor = S.points(oracle)
    lts = S.lights()
    P, L = S.N_POINTS, len(lts)
    d_pos, d_nor, d_lts = ctx.upload(pos), ctx.upload(nor), ctx.upload(lts)
    ctx_options("trace.fan", 1)
    loop = np.zeros(P, np.uint32)
    d_sr, d_flag = ctx.empty(P * 32), torch.empty((P,), dtype=torch.int32, device="cuda")
    for l in range(L):
        ctx.shadow_rays_dev(d_pos, d_nor, P, lts["position"][l], d_sr)
        if l == 0:
            assert d_sr.cpu().numpy()[: P * 32].tobytes() == rig.rays[:P].tobytes()       # the input of the other tests IS what the generator makes
        ctx.trace_any_prepared_dev(rig.acc, d_sr, P, d_flag)
        loop |= d_flag.cpu().numpy().astype(np.uint32) << np.uint32(l)
    assert np.array_equal(loop, (rig.want.reshape(L, P) << np.arange(L, dtype=np.uint32)[:, None]).sum(axis=0).astype(np.uint32))
    ctx_options("trace.fan", 3)                # the last fanned call over this top level made jobs: the default does not rest
    rig.any_hit("prepared")
    ctx_options("trace.fan", None)
    for k in range(REPEATS):
        d_occ = torch.full((P,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        info = ctx.shadow_pass_prepared_dev(rig.acc, d_pos, d_nor, P, d_lts, L, d_occ)
        torch.cuda.synchronize()
        assert info["n_rays"] == P * L and info["n_chunks"] == 1 and info["words_per_point"] == 1
        got = d_occ.cpu().numpy().astype(np.uint32)
        assert np.array_equal(got, loop), (k, int((got != loop).sum()), np.flatnonzero(got != loop)[:5].tolist())
