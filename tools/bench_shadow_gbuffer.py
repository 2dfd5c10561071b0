#!/usr/bin/env python3
"""The shadow pass straight from the G-buffer (vd_shadow_gbuffer_prepared_dev, include/voidin_gbuffer.h) against what the library
could do before it: vd_shadow_pass_prepared_dev on points that are ALREADY decoded - so the difference is the front end (count,
scan, decode + compaction, one more blocking read-back) and the scatter back to pixels.  The stress scene, lights and in-range shares
of tools/bench_shadow_pass.py, under VD_OPT_TRACE_RAY_RANGE.  G-buffer: --rays x --rays pixels, one primary ray through every pixel
centre; depth = the hit point's clip z / w, normal = minus the ray direction in the octahedral code, material 1 where the ray hit
and 0 elsewhere, rows at the 256-byte pitches a copy_texture_to_buffer gives.  profiles/shadow_gbuffer.md has a run.

  A/B   the two calls alternated in one process on one context, wall clock around each (both block), median and spread of --reps
        after a warm-up of both.  During the warm-up the per-pixel words are compared with the bare pass's per-point words at the
        points' pixels, and every other pixel's words with zero - under the library's own fan-out unless --fan says otherwise (the
        fanned-out any-hit walk is reproducible since the supply rule: profiles/shadow_pass.md, section 3; profiles/trace_fan_supply.md).
  --gbuffer-only   the new call alone, a few times per share, and the bytes each of its kernels must move, computed from the
        shapes: for a run under `rocprofv3 --kernel-trace --stats`.

    python tools/bench_shadow_gbuffer.py [--rays 1024] [--reps 21] [--gbuffer-only] [--fan N]"""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voidin_amd import abi, synth
from voidin_amd.runtime import Context

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=1024, help="side of the square G-buffer")
ap.add_argument("--reps", type=int, default=21, help="timed repetitions of each variant (alternated)")
ap.add_argument("--lights", type=int, default=64)
ap.add_argument("--shares", type=float, nargs="+", default=(1.0, 0.25, 0.05))
ap.add_argument("--gbuffer-only", action="store_true")
ap.add_argument("--fan", type=int, default=0, help="VD_OPT_TRACE_FAN for the whole run (0 = the library's default, as the tables of profiles/shadow_pass.md "
                "were taken; 1 = the one-launch walk)")
args = ap.parse_args()
assert args.reps >= 20 or args.gbuffer_only
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

# ---- the G-buffer -----------------------------------------------------------------------------------------------------------------
S = args.rays
cam = synth.camera_uniform(eye=(0, 2.5, 90), pitch_deg=0)
M = cam["clip_to_world"].reshape(4, 4).astype(np.float64).T
i = np.arange(S * S)
clip = np.stack([(i % S + 0.5) / S * 2 - 1, (1 - (i // S + 0.5) / S) * 2 - 1, np.full(S * S, 1e-3), np.ones(S * S)])
p = (M @ clip).T
eye = cam["view_position"][:3].astype(np.float64)
d = p[:, :3] / p[:, 3:4] - eye[None, :]
rays = np.zeros(S * S, dtype=abi.RAY)
rays["eye"] = eye.astype(np.float32)
rays["dir"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
d_hits = ctx.empty(len(rays) * 16)
ctx.trace_prepared_dev(acc, ctx.upload(rays), len(rays), d_hits)
hits = d_hits.cpu().numpy()[: len(rays) * 16].view(abi.HIT)
m = hits["hit"] == 1
del d_hits
hit_pts = rays["eye"][m].astype(np.float64) + rays["dir"][m].astype(np.float64) * hits["dist"][m, None].astype(np.float64)
PV = cam["projection"].reshape(4, 4).astype(np.float64).T @ cam["view"].reshape(4, 4).astype(np.float64).T
c4 = (PV @ np.concatenate([hit_pts, np.ones((len(hit_pts), 1))], axis=1).T).T
depth = np.zeros(S * S, np.float32)
depth[m] = (c4[:, 2] / c4[:, 3]).astype(np.float32)


def encode_octahedral_32(n):
    """encoding.wgsl:4-15 (a zero component of the lower hemisphere folds with sign +1)."""
    v = n / np.abs(n).sum(axis=1, keepdims=True)
    sgn = lambda a: np.where(a < 0, -1.0, 1.0)
    fold = v[:, 2] < 0
    x = np.where(fold, (1 - np.abs(v[:, 1])) * sgn(v[:, 0]), v[:, 0])
    y = np.where(fold, (1 - np.abs(v[:, 0])) * sgn(v[:, 1]), v[:, 1])
    q = lambda a: np.floor((a * 0.5 + 0.5) * 65535 + 0.5).astype(np.uint32)
    return (q(y) << np.uint32(16)) | q(x)


normal_uv = np.zeros((S * S, 2), np.uint32)
normal_uv[m, 0] = encode_octahedral_32(-rays["dir"][m].astype(np.float64))
material = m.astype(np.uint8)                                     # 1 where the ray hit (a receiver), 0 elsewhere
pitch = lambda row: (row + 255) // 256 * 256


def rows(img, row_bytes):
    buf = np.zeros((S, pitch(row_bytes)), np.uint8)
    buf[:, :row_bytes] = np.ascontiguousarray(img).view(np.uint8).reshape(S, row_bytes)
    return ctx.upload(buf.reshape(-1))


d_depth, d_nuv, d_mat = rows(depth, 4 * S), rows(normal_uv, 8 * S), rows(material, S)
gb = Context.gbuffer(d_depth, d_nuv, d_mat, S, S, pitch(4 * S), pitch(8 * S), pitch(S))
N, L = S * S, args.lights
W = (L + 31) // 32
ctx.set_option("trace.ray_range", 1)
ctx.set_option("trace.fan", args.fan or None)

# the points the bare pass is given: the front end's own output, decoded once
d_pts, d_nor = ctx.empty(N * 12), ctx.empty(N * 12)
d_pix, d_cnt = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
P = ctx.gbuffer_points_dev(cam, gb, d_pts, d_nor, d_pix, d_cnt)
assert P == int(m.sum())
pts = d_pts.cpu().numpy()[: P * 12].view(np.float32).reshape(P, 3)
print(f"{S} x {S} pixels, {P} receivers; decoded positions within {float(np.abs(pts - hit_pts).max()):.2e} of the hit points")

# lights: positions inside the box of the points, radii (0.5 .. 1) * R with R found on a sample of the points (tools/bench_shadow_pass.py)
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


d_occ_pt = torch.zeros(P * W, dtype=torch.int32, device="cuda")
d_inr_pt = torch.zeros(P * W, dtype=torch.int32, device="cuda")
d_occ_px = torch.zeros(N * W, dtype=torch.int32, device="cuda")
d_inr_px = torch.zeros(N * W, dtype=torch.int32, device="cuda")


def run_pass(d_lts):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = ctx.shadow_pass_prepared_dev(acc, d_pts, d_nor, P, d_lts, L, d_occ_pt, d_inr_pt)
    return (time.perf_counter() - t0) * 1e3, info


def run_gbuffer(d_lts):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = ctx.shadow_gbuffer_prepared_dev(acc, cam, gb, d_lts, L, d_occ_px, d_inr_px)
    return (time.perf_counter() - t0) * 1e3, info


def words_that_differ():
    """The per-pixel words against the bare pass's per-point words at the points' pixels, and against zero elsewhere."""
    pix = d_pix[:P].long()
    bad = 0
    for px, pt in ((d_occ_px, d_occ_pt), (d_inr_px, d_inr_pt)):
        px = px.view(N, W)
        bad += int((px[pix] != pt.view(P, W)).sum().item())
        rest = torch.ones(N, dtype=torch.bool, device="cuda")
        rest[pix] = False
        bad += int((px[rest] != 0).sum().item())
    return bad


out = {"pixels": N, "receivers": P, "lights": L, "reps": args.reps, "fan": args.fan, "shares": {}}
tiles = (N + 511) // 512
for share in args.shares:
    lights = lts.copy()
    lights["radius"] = unit * np.float32(radius_scale(share))
    d_lts = ctx.upload(lights)
    _, info = run_gbuffer(d_lts)                                               # warm-up of both, and the bits compared
    _, pinfo = run_pass(d_lts)
    assert info["n_points"] == P and info["n_rays"] == pinfo["n_rays"], (info, pinfo)
    row = {"in_range_share": round(info["n_rays"] / (P * L), 4), "n_rays": info["n_rays"], "n_chunks": info["n_chunks"], "words_that_differ": words_that_differ(),
           # what each new kernel must move per call, from the shapes: a material byte a pixel, a count / an offset a tile; depth and
           # the normal word (its 8-byte pair is what a line holds) and 28 bytes out a receiver; the words of every pixel out, of a receiver in
           "bytes": {"gbuffer_count_kernel": N + tiles * 4, "gbuffer_scan_kernel": tiles * 8 + 4,
                     "gbuffer_write_kernel": N + tiles * 4 + P * (4 + 8 + 28), "gbuffer_scatter_kernel": N + tiles * 4 + 2 * W * 4 * (N + P)}}
    if args.gbuffer_only:
        for _ in range(5):
            run_gbuffer(d_lts)
    else:
        t_gb, t_pass = [], []
        for _ in range(args.reps):
            t_gb.append(run_gbuffer(d_lts)[0])
            t_pass.append(run_pass(d_lts)[0])
        row.update({"gbuffer": stats(t_gb), "pass": stats(t_pass), "gbuffer_minus_pass_ms": round(float(np.median(t_gb) - np.median(t_pass)), 3)})
        print(f"share {row['in_range_share']:.3f} ({info['n_rays']} rays, {info['n_chunks']} chunks): from the G-buffer {row['gbuffer']['median_ms']:.2f} ms "
              f"({row['gbuffer']['min_ms']:.2f} .. {row['gbuffer']['max_ms']:.2f}), the pass on decoded points {row['pass']['median_ms']:.2f} ms "
              f"({row['pass']['min_ms']:.2f} .. {row['pass']['max_ms']:.2f}): +{row['gbuffer_minus_pass_ms']} ms; words that differ: {row['words_that_differ']}")
    out["shares"][str(share)] = row
print(json.dumps(out))
acc.close()
ctx.close()
