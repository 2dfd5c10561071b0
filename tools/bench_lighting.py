#!/usr/bin/env python3
"""The lighting pass (vd_lighting_dev, vd_shade_gbuffer_prepared_dev: include/voidin_lighting.h) on the stress scene of
tools/bench_gbuffer_trace.py: a --rays x --rays G-buffer traced on the device (vd_gbuffer_trace_prepared_dev, geometric normals), rows
at the 256-byte pitches a copy_texture_to_buffer gives, a seeded material table, lights placed in the box of the receivers with radii
scaled until a given share of the (receiver, light) pairs is in range (as tools/bench_shadow_gbuffer.py does).  profiles/lighting.md
has a run.

  A/B   the composed call against the two calls it is made of (vd_shadow_gbuffer_prepared_dev into the caller's own bit arrays, then
        vd_lighting_dev), alternated in one process on one context, wall clock around each with the device drained before and after,
        median and spread of --reps after a warm-up of both.  During the warm-up the two images are compared byte for byte.
  --step-only   the step alone over bits the pass wrote once, --calls times per configuration (lights, share): 64 lights at 0.05 and at
        1.0, 1024 lights at 0.05 - for a run under `rocprofv3 --kernel-trace --stats`, whose lighting_kernel dispatches come in that
        order (one warm-up call first, each).  Prints per configuration the set in-range bits, the (wave, light) visits of the walk - the
        set bits of the OR over each run of 64 pixels -, the algorithmic bytes (29 + 8 W in and 16 out a pixel) and the time between
        two stream events around each call (the kernel plus its launch).

    python tools/bench_lighting.py [--rays 1024] [--reps 21] [--lights 64] [--share 0.05] [--step-only] [--calls 5]"""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voidin_amd import abi, synth
from voidin_amd.runtime import Context

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=1024, help="side of the square G-buffer")
ap.add_argument("--reps", type=int, default=21, help="timed repetitions of each variant (alternated)")
ap.add_argument("--lights", type=int, default=64, help="lights of the A/B")
ap.add_argument("--share", type=float, default=0.05, help="share of the pairs in range in the A/B")
ap.add_argument("--step-only", action="store_true")
ap.add_argument("--calls", type=int, default=5, help="calls per configuration with --step-only")
args = ap.parse_args()
assert args.reps >= 20 or args.step_only
ctx = Context(0)
tv, ti = synth.knot_mesh(512, 128)
nodes_b, idx_b = ctx.bvh_build(tv, ti)
infos = np.zeros(1, dtype=abi.MESH_INFO)
infos[0]["min"], infos[0]["max"] = synth.mesh_bounds(tv)
infos[0]["index_count"] = len(idx_b)
inst_t = synth.instances(2000, n_mesh=1, seed=synth.SEED_BASE + 8, extent=120.0, scale_range=(0.5, 2.0))
tl = ctx.tlas_build(inst_t, infos)
ds = ctx.device_scene((tl, inst_t, infos, nodes_b, tv, idx_b))
acc = ctx.trace_prepare(ds)

# ---- the G-buffer, traced -----------------------------------------------------------------------------------------------------------
S = args.rays
N = S * S
cam = synth.camera_uniform(eye=(0, 2.5, 90), pitch_deg=0)
pitch = lambda row: (row + 255) // 256 * 256
pitches = (pitch(4 * S), pitch(8 * S), pitch(S))
img = [torch.full((S * p,), 0xC3, dtype=torch.uint8, device="cuda") for p in pitches]
ctx.gbuffer_trace_prepared_dev(acc, Context.gbuffer_geometry(ds), cam, Context.gbuffer_target(img[0], img[1], img[2], S, S, *pitches))
gb = Context.gbuffer(img[0], img[1], img[2], S, S, *pitches)
d_pts, d_nor = ctx.empty(N * 12), ctx.empty(N * 12)
d_pix, d_cnt = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
P = ctx.gbuffer_points_dev(cam, gb, d_pts, d_nor, d_pix, d_cnt)
pts = d_pts.cpu().numpy()[: P * 12].view(np.float32).reshape(P, 3)
del d_pts, d_nor, d_pix
print(f"{S} x {S} pixels, {P} receivers")
ctx.set_option("trace.ray_range", 1)

seed = synth.SEED_BASE + 90
table = np.zeros(abi.LIGHTING_MATERIALS, dtype=abi.FLAT_MATERIAL)
table["albedo"] = synth.uniform01(seed, 8, 3 * len(table)).reshape(-1, 3).astype(np.float32)
table["specular"] = synth.uniform01(seed, 9, len(table)).astype(np.float32)
table["emissive"] = (0.1 * synth.uniform01(seed, 10, 3 * len(table))).reshape(-1, 3).astype(np.float32)
d_table = ctx.upload(table)
lo, hi = pts.min(axis=0), pts.max(axis=0)
sample = pts[:: max(1, P // 20000)].astype(np.float64)


def lights(L, share):
    """L lights inside the box of the receivers, radii (0.5 .. 1) * R with R found on a sample of them so that `share` of the pairs is
    in range."""
    lts = np.zeros(L, dtype=abi.LIGHT)
    for axis in range(3):
        lts["position"][:, axis] = (lo[axis] + (hi[axis] - lo[axis]) * synth.uniform01(seed, axis, L)).astype(np.float32)
    unit = (0.5 + 0.5 * synth.uniform01(seed, 3, L)).astype(np.float32)
    dist = np.concatenate([np.sqrt(((lts["position"][None, k: k + 64, :].astype(np.float64) - sample[:, None, :]) ** 2).sum(axis=2)) for k in range(0, L, 64)], axis=1)
    a, b = 0.0, 4.0 * float(dist.max())
    if share < 1.0:
        for _ in range(40):
            mid = 0.5 * (a + b)
            a, b = (mid, b) if (dist <= unit[None, :] * mid).mean() < share else (a, mid)
    lts["radius"] = unit * np.float32(b)
    lts["color"] = synth.uniform01(seed, 4, 3 * L).reshape(L, 3).astype(np.float32)
    return lts


def target():
    p = pitch(16 * S)
    t = torch.full((S * p,), 0xC3, dtype=torch.uint8, device="cuda")
    return t, Context.color_target(t, S, S, p)


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms[0]), 3), "max_ms": round(float(ms[-1]), 3),
            "spread_pct": round(float(100.0 * (ms[-1] - ms[0]) / np.median(ms)), 2)}


def popcount(t):
    """Set bits of an int32 tensor of words."""
    w = t.cpu().numpy().view(np.uint8)
    return int(np.unpackbits(w).sum())


if args.step_only:
    rows = []
    for L, share in ((64, 0.05), (64, 1.0), (1024, 0.05)):
        W = (L + 31) // 32
        d_lts = ctx.upload(lights(L, share))
        d_occ, d_inr = torch.zeros(N * W, dtype=torch.int32, device="cuda"), torch.zeros(N * W, dtype=torch.int32, device="cuda")
        info = ctx.shadow_gbuffer_prepared_dev(acc, cam, gb, d_lts, L, d_occ, d_inr)
        buf, tg = target()
        ctx.lighting_dev(cam, gb, d_lts, L, d_occ, d_inr, d_table, tg)                 # warm-up
        torch.cuda.synchronize()
        us = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.lighting_dev(cam, gb, d_lts, L, d_occ, d_inr, d_table, tg)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        bits = popcount(d_inr)
        # what the walk visits: per wave (64 consecutive pixels) the lights in the OR of its words - 64 lane slots each
        padded = np.zeros(((N + 63) // 64 * 64, W), np.uint32)
        padded[:N] = d_inr.cpu().numpy().view(np.uint32).reshape(N, W)
        per_wave = np.ascontiguousarray(np.bitwise_or.reduce(padded.reshape(-1, 64, W), axis=1))
        visits = int(np.unpackbits(per_wave.view(np.uint8)).sum())
        assert bits == info["n_rays"]
        rows.append({"lights": L, "share_asked": share, "words_per_pixel": W, "set_in_range_bits": bits, "set_occluded_bits": popcount(d_occ),
                     "wave_visits": visits, "lanes_adding_per_visit": round(bits / max(1, visits), 2),
                     "share_of_receiver_pairs": round(bits / (P * L), 4), "bytes_in": N * (29 + 8 * W), "bytes_out": N * 16,
                     "event_us": {"median": round(float(np.median(us)), 1), "min": round(float(min(us)), 1), "max": round(float(max(us)), 1)}})
        print(f"{L} lights, share {share}: {bits} set bits in {visits} (wave, light) visits, W = {W}, {N * (29 + 8 * W) + N * 16} algorithmic bytes, {rows[-1]['event_us']['median']} us between events")
        del d_occ, d_inr, buf
    print(json.dumps({"pixels": N, "receivers": P, "calls": args.calls, "rows": rows}))
else:
    L, W = args.lights, (args.lights + 31) // 32
    d_lts = ctx.upload(lights(L, args.share))
    d_occ, d_inr = torch.zeros(N * W, dtype=torch.int32, device="cuda"), torch.zeros(N * W, dtype=torch.int32, device="cuda")
    buf_a, tg_a = target()
    buf_b, tg_b = target()
    infos_seen = {}

    def composed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        infos_seen["composed"] = ctx.shade_gbuffer_prepared_dev(acc, cam, gb, d_lts, L, d_table, tg_a)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def two_calls():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        infos_seen["two"] = ctx.shadow_gbuffer_prepared_dev(acc, cam, gb, d_lts, L, d_occ, d_inr)
        ctx.lighting_dev(cam, gb, d_lts, L, d_occ, d_inr, d_table, tg_b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    composed(); two_calls()                                                        # warm-up of both, and the bytes compared
    differ = int((buf_a != buf_b).sum().item())
    assert differ == 0 and infos_seen["composed"] == infos_seen["two"], (differ, infos_seen)
    rgba = buf_a.cpu().numpy().reshape(S, pitch(16 * S))[:, : 16 * S].copy().view(np.float32).reshape(N, 4)
    assert np.isfinite(rgba).all() and (rgba >= 0).all() and (rgba[:, 3] == 1).all()
    t_c, t_2 = [], []
    for _ in range(args.reps):
        t_c.append(composed())
        t_2.append(two_calls())
    out = {"pixels": N, "receivers": P, "lights": L, "share_asked": args.share, "set_in_range_bits": infos_seen["two"]["n_rays"], "reps": args.reps,
           "bytes_that_differ": differ, "composed": stats(t_c), "two_calls": stats(t_2),
           "composed_minus_two_calls_ms": round(float(np.median(t_c) - np.median(t_2)), 3)}
    print(f"{S} x {S} pixels, {L} lights, {out['set_in_range_bits']} pairs in range: composed {out['composed']['median_ms']:.3f} ms "
          f"({out['composed']['min_ms']:.3f} .. {out['composed']['max_ms']:.3f}), two calls {out['two_calls']['median_ms']:.3f} ms "
          f"({out['two_calls']['min_ms']:.3f} .. {out['two_calls']['max_ms']:.3f}): {out['composed_minus_two_calls_ms']:+.3f} ms; bytes that differ: {differ}")
    print(json.dumps(out))
acc.close()
ctx.close()
