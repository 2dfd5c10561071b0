#!/usr/bin/env python3
"""The shadow pass for many lights (vd_shadow_pass_prepared_dev, include/voidin_shadow.h) against the loop it replaces - per light
vd_shadow_rays_dev + vd_trace_any_prepared_dev over ALL points - on the stress scene of tools/ab_trace.py (2000 overlapping
instances of a 131 k-triangle knot), prepared, under VD_OPT_TRACE_RAY_RANGE (shadow rays that stop at the light).  Points: the hit
points of --rays x --rays primary rays.  64 lights inside the box of the points, radii scaled so that the share of (point, light)
pairs in range is about 1.0, 0.25 and 0.05.  profiles/shadow_pass.md has a run.

  A/B   the pass and the loop alternated in one process on one context: wall clock around each (both end with the stream drained;
        vd_last_gpu_ms only covers the last inner walk), median and spread of --reps after a warm-up of both.  The loop is given a
        head start: it does NOT fold its 64 flag arrays into bits, which a renderer would still have to do.  During the warm-up
        the pass's bits are compared with the loop's flags, masked by the pass's own in-range bits.
  --pass-only   the pass alone, a few times per share, and the bytes each of its kernels must move, computed from the shapes: for
        a run under `rocprofv3 --kernel-trace --stats`, whose kernel times those bytes are set against.

    python tools/bench_shadow_pass.py [--rays 1024] [--reps 21] [--pass-only] [--fan 1]"""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voidin_amd import abi, synth
from voidin_amd.runtime import Context

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=1024, help="side of the square of primary rays whose hit points are the points")
ap.add_argument("--reps", type=int, default=21, help="timed repetitions of each variant (alternated)")
ap.add_argument("--lights", type=int, default=64)
ap.add_argument("--shares", type=float, nargs="+", default=(1.0, 0.25, 0.05))
ap.add_argument("--pass-only", action="store_true")
ap.add_argument("--fan", type=int, default=None, help="VD_OPT_TRACE_FAN for the whole run (default: the library's; 1 = the one-launch walk, whose flags are "
                "reproducible on this scene: profiles/shadow_pass.md, section 3)")
args = ap.parse_args()
assert args.reps >= 20 or args.pass_only
ctx = Context(0)
tv, ti = synth.knot_mesh(512, 128)
nodes_b, idx_b = ctx.bvh_build(tv, ti)
infos = np.zeros(1, dtype=abi.MESH_INFO)
infos[0]["min"], infos[0]["max"] = synth.mesh_bounds(tv)
infos[0]["index_count"] = len(idx_b)
inst_t = synth.instances(2000, n_mesh=1, seed=synth.SEED_BASE + 8, extent=120.0, scale_range=(0.5, 2.0))
tl = ctx.tlas_build(inst_t, infos)
rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 90), pitch_deg=0), args.rays, args.rays)
ds = ctx.device_scene((tl, inst_t, infos, nodes_b, tv, idx_b))
acc = ctx.trace_prepare(ds)
d_hits = ctx.empty(len(rays) * 16)
ctx.trace_prepared_dev(acc, ctx.upload(rays), len(rays), d_hits)
hits = d_hits.cpu().numpy()[: len(rays) * 16].view(abi.HIT)
m = hits["hit"] == 1
pts = (rays["eye"][m] + rays["dir"][m] * hits["dist"][m, None]).astype(np.float32)
nor = (-rays["dir"][m]).astype(np.float32)
del d_hits
P, L = len(pts), args.lights
W = (L + 31) // 32
d_pts, d_nor = ctx.upload(pts), ctx.upload(nor)
ctx.set_option("trace.ray_range", 1)
ctx.set_option("trace.fan", args.fan)

# lights: positions inside the box of the points, radii (0.5 .. 1) * R with R found on a sample of the points
lo, hi = pts.min(axis=0), pts.max(axis=0)
seed = synth.SEED_BASE + 90
lts = np.zeros(L, dtype=abi.LIGHT)
for axis in range(3):
    lts["position"][:, axis] = (lo[axis] + (hi[axis] - lo[axis]) * synth.uniform01(seed, axis, L)).astype(np.float32)
unit = (0.5 + 0.5 * synth.uniform01(seed, 3, L)).astype(np.float32)
sample = pts[:: max(1, P // 20000)].astype(np.float64)
dist = np.sqrt(((lts["position"][None, :, :].astype(np.float64) - sample[:, None, :]) ** 2).sum(axis=2))


def radius_scale(share):
    if share >= 1.0:
        return 4.0 * float(dist.max())
    a, b = 0.0, 4.0 * float(dist.max())
    for _ in range(40):
        mid = 0.5 * (a + b)
        a, b = (mid, b) if (dist <= unit[None, :] * mid).mean() < share else (a, mid)
    return b


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms[0]), 3), "max_ms": round(float(ms[-1]), 3),
            "spread_pct": round(float(100.0 * (ms[-1] - ms[0]) / np.median(ms)), 2)}


d_occ = torch.zeros(P * W, dtype=torch.int32, device="cuda")
d_inr = torch.zeros(P * W, dtype=torch.int32, device="cuda")
d_rays = ctx.empty(P * 32)
d_flag = torch.zeros(P, dtype=torch.int32, device="cuda")


def run_pass(d_lts):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = ctx.shadow_pass_prepared_dev(acc, d_pts, d_nor, P, d_lts, L, d_occ, d_inr)
    return (time.perf_counter() - t0) * 1e3, info


def run_loop(lights, check):
    """-> (ms, pairs whose flag differs from the pass's bit; None when not checked)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bad = 0
    for l in range(L):
        ctx.shadow_rays_dev(d_pts, d_nor, P, lights["position"][l], d_rays)
        ctx.trace_any_prepared_dev(acc, d_rays, P, d_flag)
        if check:
            reach = (d_inr.view(P, W)[:, l >> 5] >> (l & 31)) & 1
            occ = (d_occ.view(P, W)[:, l >> 5] >> (l & 31)) & 1
            bad += int((occ != ((d_flag != 0).to(torch.int32) & reach)).sum().item())
    return (time.perf_counter() - t0) * 1e3, (bad if check else None)


out = {"points": P, "lights": L, "reps": args.reps, "fan": args.fan, "shares": {}}
tiles = (P + 511) // 512
for share in args.shares:
    lights = lts.copy()
    lights["radius"] = unit * np.float32(radius_scale(share))
    d_lts = ctx.upload(lights)
    _, info = run_pass(d_lts)                                                  # warm-up of the pass (and the bits the loop is checked against)
    R = info["n_rays"]
    row = {"in_range_share": round(R / (P * L), 4), "n_rays": R, "n_chunks": info["n_chunks"],
           # what each kernel must move per call, from the shapes (positions 12 B, normals 12 B, a ray 32 B, a flag 4 B, a cell 4 B)
           "bytes": {"shadow_count_kernel": P * 12 + tiles * L * 4, "shadow_scan_kernel": tiles * L * 8,
                     # ... and per chunk the positions (and normals) of the tiles it touches - all of them when it spans a light
                     "shadow_write_kernel": R * 32 + info["n_chunks"] * P * 24, "shadow_fold_kernel": R * 4 + info["n_chunks"] * (P * 12 + 2 * P * W * 4)}}
    if args.pass_only:
        for _ in range(5):
            run_pass(d_lts)
    else:
        _, bad = run_loop(lights, True)                                        # warm-up of the loop, checked
        t_pass, t_loop = [], []
        for _ in range(args.reps):
            t_pass.append(run_pass(d_lts)[0])
            t_loop.append(run_loop(lights, False)[0])
        row.update({"pass": stats(t_pass), "loop": stats(t_loop), "pairs_that_differ": bad,
                    "loop_over_pass": round(float(np.median(t_loop) / np.median(t_pass)), 3)})
        print(f"share {row['in_range_share']:.3f} ({R} rays, {info['n_chunks']} chunks): pass {row['pass']['median_ms']:.2f} ms ({row['pass']['min_ms']:.2f} .. "
              f"{row['pass']['max_ms']:.2f}), loop of {L} calls {row['loop']['median_ms']:.2f} ms ({row['loop']['min_ms']:.2f} .. {row['loop']['max_ms']:.2f}): "
              f"x{row['loop_over_pass']}; pairs that differ: {bad}")
    out["shares"][str(share)] = row
print(json.dumps(out))
acc.close()
ctx.close()
