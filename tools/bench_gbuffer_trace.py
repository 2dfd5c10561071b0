#!/usr/bin/env python3
"""The G-buffer from primary rays (vd_gbuffer_trace_prepared_dev, include/voidin_gbuffer_trace.h) on the stress scene of
tools/bench_shadow_gbuffer.py: --rays x --rays pixels, per-vertex normals and uvs from a fixed seed, rows at the 256-byte pitches a
copy_texture_to_buffer gives.  profiles/gbuffer_trace.md has a run.

  A/B   the composed call against the three calls it is made of (vd_gbuffer_rays_dev, vd_trace_prepared_dev,
        vd_gbuffer_resolve_dev with the caller's own ray and record buffers), alternated in one process on one context, wall clock
        around each with the device drained before and after, median and spread of --reps after a warm-up of both.  During the
        warm-up the three images of the two are compared byte for byte, and fed to vd_gbuffer_points_dev.
  --kernels-only   the composed call alone, a few times: for a run under `rocprofv3 --kernel-trace --stats`.  Prints the bytes each
        of the two new kernels must move, computed from the shapes and the hit count.

    python tools/bench_gbuffer_trace.py [--rays 1024] [--reps 21] [--kernels-only] [--no-attributes]"""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voidin_amd import abi, synth
from voidin_amd.runtime import Context

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=1024, help="side of the square G-buffer")
ap.add_argument("--reps", type=int, default=21, help="timed repetitions of each variant (alternated)")
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--no-attributes", action="store_true", help="geometric normals, no uvs")
args = ap.parse_args()
assert args.reps >= 20 or args.kernels_only
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
nv = len(np.asarray(tv).reshape(-1, 3))
seed = synth.SEED_BASE + 97
d_normals = None if args.no_attributes else ctx.upload((synth.uniform01(seed, 0, 3 * nv) * 2 - 1).astype(np.float32))
d_uvs = None if args.no_attributes else ctx.upload(synth.uniform01(seed, 1, 2 * nv).astype(np.float32))
geo = Context.gbuffer_geometry(ds, d_normals, d_uvs)

S = args.rays
N = S * S
cam = synth.camera_uniform(eye=(0, 2.5, 90), pitch_deg=0)
pitch = lambda row: (row + 255) // 256 * 256
pitches = (pitch(4 * S), pitch(8 * S), pitch(S))


def images():
    t = [torch.full((S * p,), 0xC3, dtype=torch.uint8, device="cuda") for p in pitches]
    return t, Context.gbuffer_target(t[0], t[1], t[2], S, S, *pitches)


img_a, tg_a = images()
img_b, tg_b = images()
d_rays, d_hits = ctx.empty(N * 32), ctx.empty(N * 16)


def composed():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.gbuffer_trace_prepared_dev(acc, geo, cam, tg_a)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def three_calls():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.gbuffer_rays_dev(cam, S, S, d_rays)
    ctx.trace_prepared_dev(acc, d_rays, N, d_hits)
    ctx.gbuffer_resolve_dev(cam, geo, d_hits, tg_b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms[0]), 3), "max_ms": round(float(ms[-1]), 3),
            "spread_pct": round(float(100.0 * (ms[-1] - ms[0]) / np.median(ms)), 2)}


composed(); three_calls()                                                      # warm-up of both, and the bytes compared
differ = sum(int((a != b).sum().item()) for a, b in zip(img_a, img_b))
hit = d_hits.cpu().numpy()[: N * 16].view(abi.HIT)["hit"] == 1
H = int(hit.sum())
material = img_a[2].cpu().numpy().reshape(S, pitches[2])[:, :S].reshape(-1)
assert differ == 0 and (material[~hit] == 0).all(), differ
d_pos, d_nor = ctx.empty(N * 12), ctx.empty(N * 12)
d_pix, d_cnt = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
P = ctx.gbuffer_points_dev(cam, Context.gbuffer(img_a[0], img_a[1], img_a[2], S, S, *pitches), d_pos, d_nor, d_pix, d_cnt)
assert P == int((material != 0).sum() - (material == 2).sum())
# what the two kernels must move per call, from the shapes: 32 bytes a ray out; a 16-byte record in and 4 + 8 + 1 bytes out a pixel,
# and per HIT pixel the instance's mesh + material and two matrices (8 + 128), three words of the mesh record, three indices, three
# positions and - with attributes - three normals and three uvs, counted as if no two pixels shared a line
per_hit = 8 + 128 + 12 + 12 + 36 + (0 if args.no_attributes else 36 + 24)
out = {"pixels": N, "hits": H, "receivers": P, "attributes": not args.no_attributes, "reps": args.reps, "bytes_that_differ": differ,
       "bytes": {"gbuffer_rays_kernel": N * 32, "gbuffer_resolve_kernel": N * (16 + 13) + H * per_hit},
       "algorithmic_bytes_per_pixel": {"miss": 16 + 13, "hit": 16 + 13 + per_hit}}
if args.kernels_only:
    for _ in range(5):
        composed()
else:
    t_c, t_3 = [], []
    for _ in range(args.reps):
        t_c.append(composed())
        t_3.append(three_calls())
    out.update({"composed": stats(t_c), "three_calls": stats(t_3), "composed_minus_three_calls_ms": round(float(np.median(t_c) - np.median(t_3)), 3)})
    print(f"{S} x {S} pixels, {H} hits: composed {out['composed']['median_ms']:.3f} ms ({out['composed']['min_ms']:.3f} .. {out['composed']['max_ms']:.3f}), "
          f"three calls {out['three_calls']['median_ms']:.3f} ms ({out['three_calls']['min_ms']:.3f} .. {out['three_calls']['max_ms']:.3f}): "
          f"{out['composed_minus_three_calls_ms']:+.3f} ms; bytes that differ: {differ}")
print(json.dumps(out))
acc.close()
ctx.close()
