#!/usr/bin/env python3
"""What VD_OPT_TRACE_RAY_RANGE costs and what it buys, on the stress scene of tools/ab_trace.py (2000 overlapping instances of a
131 k-triangle knot), prepared scene, closest hit and any hit (profiles/trace_ray_range.md has a run):

  (a) the option off against the option on with full-range pads (0, 1e30) - the same walk through the RANGE instantiations of the
      kernels, the same bytes out.  The two are alternated in one process, --reps times each; median and spread of both.
      Twice: as the call runs by default (three launches: the fan-out's kernels, 5 waves per SIMD) and as one launch
      (VD_OPT_TRACE_FAN = 1: the plain kernels, 6 waves per SIMD, the ones nearest to their register limit).
  (b) shadow rays from the primary hit points towards a point light inside the scene: any-hit with the option off (rays without
      an end: the reference's shadow pass) against the option on (segments that stop at the light) - the rate, and how many
      flags differ.

    python tools/bench_trace_range.py [--rays 1024] [--reps 7]"""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voidin_amd import abi, synth
from voidin_amd.runtime import Context, set_ray_range

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=1024, help="side of the square of primary rays")
ap.add_argument("--reps", type=int, default=7, help="timed repetitions of each variant (alternated)")
ap.add_argument("--light", type=float, nargs=3, default=(5.0, 20.0, 10.0))
args = ap.parse_args()
assert args.reps >= 5
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
n = len(rays)
ctx.set_timing(True)


def stats(ms, n_rays):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms[0]), 3), "max_ms": round(float(ms[-1]), 3),
            "spread_pct": round(float(100.0 * (ms[-1] - ms[0]) / np.median(ms)), 2), "mrays_s": round(n_rays / float(np.median(ms)) / 1e3, 1)}


def alternate(variants, n_rays, d_hits, d_any):
    """variants: name -> (option value, device rays).  One warm-up of each, then --reps rounds that run every variant once:
    closest hit, then any hit, each timed by the library's own events.  -> name -> (closest ms, any ms, closest bytes, any bytes)"""
    out = {k: ([], [], None, None) for k in variants}
    for rep in range(-1, args.reps):
        for name, (opt, d_r) in variants.items():
            ctx.set_option("trace.ray_range", opt)
            ctx.trace_prepared_dev(acc, d_r, n_rays, d_hits); t_cl = ctx.last_gpu_ms()
            ctx.trace_any_prepared_dev(acc, d_r, n_rays, d_any); t_any = ctx.last_gpu_ms()
            if rep < 0:
                out[name] = ([], [], d_hits.cpu().numpy()[: n_rays * 16].tobytes(), d_any.cpu().numpy()[:n_rays].tobytes())
            else:
                out[name][0].append(t_cl); out[name][1].append(t_any)
    ctx.set_option("trace.ray_range", None)
    return out


# ---- (a) the same walk through the RANGE instantiations -------------------------------------------------------------------------
d_hits, d_any = ctx.empty(n * 16), torch.zeros(n, dtype=torch.int32, device="cuda")
d_plain, d_full = ctx.upload(rays), ctx.upload(set_ray_range(rays.copy(), 0.0, 1e30))
res_a, gap, same = {}, {}, {}
for launches, fan in (("three launches", 3), ("one launch", 1)):
    ctx.set_option("trace.fan", fan)
    a = alternate({"off": (0, d_plain), "on (0, 1e30)": (1, d_full)}, n, d_hits, d_any)
    same[launches] = a["off"][2] == a["on (0, 1e30)"][2] and a["off"][3] == a["on (0, 1e30)"][3]
    r = res_a[launches] = {k: {"closest": stats(v[0], n), "any": stats(v[1], n)} for k, v in a.items()}
    for k, v in r.items():
        print(f"(a) {launches}, {k:14s} closest {v['closest']['mrays_s']:7.1f} Mrays/s (median {v['closest']['median_ms']:.3f} ms, {v['closest']['min_ms']:.3f} .. {v['closest']['max_ms']:.3f})"
              f"   any {v['any']['mrays_s']:7.1f} Mrays/s (median {v['any']['median_ms']:.3f} ms, {v['any']['min_ms']:.3f} .. {v['any']['max_ms']:.3f})")
    gap[launches] = {q: round(100.0 * (r["on (0, 1e30)"][q]["median_ms"] / r["off"][q]["median_ms"] - 1.0), 2) for q in ("closest", "any")}
    print(f"(a) {launches}, on against off, medians: closest {gap[launches]['closest']:+.2f} %, any {gap[launches]['any']:+.2f} % (spread of the off runs: closest "
          f"{r['off']['closest']['spread_pct']} %, any {r['off']['any']['spread_pct']} %); same bytes: {same[launches]}")
    if fan == 3:
        first_off = a["off"][2]
ctx.set_option("trace.fan", 3)

# ---- (b) shadow rays from the primary hit points towards a light inside the scene ------------------------------------------------
hits = np.frombuffer(first_off, dtype=abi.HIT)
m = hits["hit"] == 1
pts = (rays["eye"][m] + rays["dir"][m] * hits["dist"][m, None]).astype(np.float32)
nor = (-rays["dir"][m]).astype(np.float32)
n_s = len(pts)
d_pts, d_nor = ctx.upload(pts), ctx.upload(nor)
shadow = {}
for name, opt in (("off: rays without an end", 0), ("on: segments to the light", 1)):
    ctx.set_option("trace.ray_range", opt)
    d_sr = ctx.empty(n_s * 32)
    ctx.shadow_rays_dev(d_pts, d_nor, n_s, args.light, d_sr)
    shadow[name] = (opt, d_sr)
d_hits_s, d_any_s = ctx.empty(n_s * 16), torch.zeros(n_s, dtype=torch.int32, device="cuda")
b = alternate(shadow, n_s, d_hits_s, d_any_s)
res_b = {k: {"any": stats(v[1], n_s), "closest": stats(v[0], n_s)} for k, v in b.items()}
f_off, f_on = (np.frombuffer(b[k][3], dtype=np.uint32) for k in shadow)
for k, v in res_b.items():
    print(f"(b) {k:26s} any {v['any']['mrays_s']:7.1f} Mrays/s (median {v['any']['median_ms']:.3f} ms, {v['any']['min_ms']:.3f} .. {v['any']['max_ms']:.3f})")
print(f"(b) {n_s} shadow rays, light at {tuple(args.light)}: shadowed {int(f_off.sum())} without an end, {int(f_on.sum())} on the segment; "
      f"{int((f_off != f_on).sum())} flags differ ({int(((f_on == 1) & (f_off == 0)).sum())} the other way round)")
print(json.dumps({"rays": n, "reps": args.reps, "a": res_a, "a_gap_pct": gap, "a_same_bytes": same, "b": res_b, "b_rays": n_s,
                  "b_shadowed_off": int(f_off.sum()), "b_shadowed_on": int(f_on.sum()), "b_flags_differ": int((f_off != f_on).sum())}))
acc.close()
ctx.close()
