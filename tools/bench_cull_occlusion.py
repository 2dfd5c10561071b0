"""The occlusion-culled draw lists (vd_cull_compact_hiz_dev; vd_cull_early_dev + vd_cull_late_dev) against the compositions
that were the only way to get them before - in ONE process, candidate and yardstick alternating, five repetitions each
(median, min .. max), HIP events on the context's stream, inputs resident:
  hiz          vs  vd_cull_mask_dev -> vd_occlusion_mask_dev -> vd_expand_mask_dev, the mesh-id table built beforehand
                   (the composition's best case);
  early + late vs  vd_cull_mask_dev -> (F & P by torch) -> vd_expand_mask_dev, vd_occlusion_mask_dev(F) ->
                   (V & ~P by torch) -> vd_expand_mask_dev;
  lower bound      vd_cull_compact_dev alone, and pass 1 of each mode alone (vd_last_gpu_ms_stage 0) as TB/s on its
                   algorithmic bytes: 144 + 1/8 + 1 per instance for hiz and early, + 2/8 for late's mask traffic.
10 M instances of the bench's wide cloud and of the `dist small` cloud under the default camera, a 1920 x 1080 pyramid of a
synthetic depth (a near wall over part of the screen; the fraction of the frustum set it hides is reported).  P for early / late: the
unoccluded set of a camera a step away (what last frame leaves), written to a separate buffer so every step does the same work.
Usage (on a GPU box): python tools/bench_cull_occlusion.py [--n 10000000] [--steps 50] [--reps 5] [--dists baseline,small]
                                                           [--out result.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voidin_amd import abi, synth  # noqa: E402
from voidin_amd.runtime import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--dists", default="baseline,small")
ap.add_argument("--out", default="")
args = ap.parse_args()

CLOUDS = {"baseline": dict(scale_range=(0.25, 4.0)), "small": dict(scale_range=(0.02, 0.6), extent=600.0)}
# (distance of the wall, fraction of the screen width it covers from the left).  The small cloud: about a third of its frustum
# set is hidden.  The wide cloud: the bug-compatible frustum radius keeps 95 % of ALL instances - most of them off screen or
# behind the eye, where nothing is ever occluded - so even a wall over the whole screen hides well under a third; it gets that wall.
WALL = {"baseline": (30.0, 1.0), "small": (30.0, 0.57)}
W, H = 1920, 1080


def synthetic_depth(distance, cover, znear=0.001):
    """Cleared depth (0 = infinitely far) with a wall `distance` away over the left `cover` of the screen."""
    d = np.zeros((H, W), dtype=np.float32)
    d[:, : int(W * cover)] = np.float32(znear / distance)
    return d


ctx = Context(0)
n = args.n
meshes = synth.mesh_infos()
n_mesh = len(meshes)
d_m = ctx.upload(meshes)
cam, cam_prev = synth.camera_uniform(), synth.camera_uniform(eye=(2.5, 5.0, 12.5), yaw_deg=1.0)
n_words = (n + 63) // 64
d_out, d_out2 = ctx.empty(n * 20), ctx.empty(n * 20)
d_cnt = torch.zeros(16, dtype=torch.int32, device="cuda")
L = ctx.hiz_layout(W, H)
d_pyr = torch.zeros(L.total_texels, dtype=torch.float32, device="cuda")
d_mask, d_occ, d_tmp = (torch.zeros(n_words, dtype=torch.int64, device="cuda") for _ in range(3))
d_prev, d_vis = torch.zeros(n_words, dtype=torch.int64, device="cuda"), torch.zeros(n_words, dtype=torch.int64, device="cuda")
ev = lambda: torch.cuda.Event(enable_timing=True)
result = {"n": n, "steps": args.steps, "reps": args.reps, "pyramid": [W, H], "dists": {}}


def popcount(t):
    return int(np.unpackbits(t.cpu().numpy().view(np.uint8)).sum())


def stats(ts):
    ts = np.array(ts)
    return {"median": round(float(np.median(ts)), 4), "min": round(float(ts.min()), 4), "max": round(float(ts.max()), 4)}


for dist in args.dists.split(","):
    inst = synth.instances(n, seed=synth.SEED_BASE + 3, with_inverse=False, **CLOUDS[dist])
    d_i = ctx.upload(inst)
    d_ids = torch.from_numpy(np.minimum(inst["mesh"], n_mesh - 1).astype(np.uint8)).to("cuda")     # the composition's id table, pre-built
    del inst
    ctx.hiz_build_dev(ctx.upload(synthetic_depth(*WALL[dist])), W, H, d_pyr)
    # P = what a frame with the camera a step away leaves
    ctx.cull_mask_dev(cam_prev, d_m, n_mesh, d_i, n, d_prev)
    ctx.occlusion_mask_dev(cam_prev, d_m, n_mesh, d_i, n, d_pyr, W, H, d_prev, d_prev)
    torch.cuda.synchronize()

    def hiz():
        ctx.cull_compact_hiz_dev(cam, d_m, n_mesh, d_i, n, d_pyr, W, H, d_out, d_cnt)

    def hiz_composition():
        ctx.cull_mask_dev(cam, d_m, n_mesh, d_i, n, d_mask)
        ctx.occlusion_mask_dev(cam, d_m, n_mesh, d_i, n, d_pyr, W, H, d_mask, d_occ)
        ctx.expand_mask_dev(d_occ, n, n, d_ids, d_m, n_mesh, d_out2, d_cnt[1:], id_bytes=1)

    def early_late():
        ctx.cull_early_dev(cam, d_m, n_mesh, d_i, n, d_prev, d_out, d_cnt[2:])
        ctx.cull_late_dev(cam, d_m, n_mesh, d_i, n, d_pyr, W, H, d_prev, d_vis, d_out2, d_cnt[3:])

    def early_late_composition():
        ctx.cull_mask_dev(cam, d_m, n_mesh, d_i, n, d_mask)
        torch.bitwise_and(d_mask, d_prev, out=d_tmp)
        ctx.expand_mask_dev(d_tmp, n, n, d_ids, d_m, n_mesh, d_out, d_cnt[4:], id_bytes=1)
        ctx.occlusion_mask_dev(cam, d_m, n_mesh, d_i, n, d_pyr, W, H, d_mask, d_occ)
        torch.bitwise_and(d_occ, torch.bitwise_not(d_prev, out=d_tmp), out=d_tmp)
        ctx.expand_mask_dev(d_tmp, n, n, d_ids, d_m, n_mesh, d_out2, d_cnt[5:], id_bytes=1)

    def plain():
        ctx.cull_compact_dev(cam, d_m, n_mesh, d_i, n, d_out, d_cnt[6:])

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    # same bytes first
    hiz()
    hiz_composition()
    torch.cuda.synchronize()
    c = d_cnt.cpu().numpy()
    same_hiz = bool(c[0] == c[1] and torch.equal(d_out[: int(c[0]) * 20], d_out2[: int(c[0]) * 20]))
    n_f, n_v = popcount(d_mask), popcount(d_occ)
    early_late()
    torch.cuda.synchronize()
    e_list, l_list = d_out[: int(d_cnt[2]) * 20].clone(), d_out2[: int(d_cnt[3]) * 20].clone()
    vis_equal = bool(torch.equal(d_vis, d_occ))
    early_late_composition()
    torch.cuda.synchronize()
    c = d_cnt.cpu().numpy()
    same_el = bool(c[2] == c[4] and c[3] == c[5] and torch.equal(e_list, d_out[: int(c[4]) * 20]) and torch.equal(l_list, d_out2[: int(c[5]) * 20]))
    del e_list, l_list

    t = {k: [] for k in ("hiz", "hiz_composition", "early_late", "early_late_composition", "plain")}
    for _ in range(args.reps):
        t["hiz"].append(timed(hiz))
        t["hiz_composition"].append(timed(hiz_composition))
        t["early_late"].append(timed(early_late))
        t["early_late_composition"].append(timed(early_late_composition))
        t["plain"].append(timed(plain))
    # the passes alone (event pairs around each pass cost a few us of idle: not part of the step times above)
    ctx.set_timing(True)
    p = {k: [] for k in ("hiz", "early", "late", "plain", "hiz_expand", "early_expand", "late_expand", "mask", "occlusion_mask", "expand_mask")}
    for _ in range(args.steps):
        hiz()
        p["hiz"].append(ctx.last_gpu_ms_stage(0)); p["hiz_expand"].append(ctx.last_gpu_ms_stage(1))
        ctx.cull_early_dev(cam, d_m, n_mesh, d_i, n, d_prev, d_out, d_cnt[2:])
        p["early"].append(ctx.last_gpu_ms_stage(0)); p["early_expand"].append(ctx.last_gpu_ms_stage(1))
        ctx.cull_late_dev(cam, d_m, n_mesh, d_i, n, d_pyr, W, H, d_prev, d_vis, d_out2, d_cnt[3:])
        p["late"].append(ctx.last_gpu_ms_stage(0)); p["late_expand"].append(ctx.last_gpu_ms_stage(1))
        plain()
        p["plain"].append(ctx.last_gpu_ms_stage(0))
        ctx.cull_mask_dev(cam, d_m, n_mesh, d_i, n, d_mask)
        p["mask"].append(ctx.last_gpu_ms())
        ctx.occlusion_mask_dev(cam, d_m, n_mesh, d_i, n, d_pyr, W, H, d_mask, d_occ)
        p["occlusion_mask"].append(ctx.last_gpu_ms())
        ctx.expand_mask_dev(d_occ, n, n, d_ids, d_m, n_mesh, d_out2, d_cnt[1:], id_bytes=1)
        p["expand_mask"].append(ctx.last_gpu_ms())
    ctx.set_timing(False)
    med = {k: float(np.median(v)) for k, v in p.items()}
    c = d_cnt.cpu().numpy()

    def verdict(cand, yard):
        a, b = np.array(t[cand]), np.array(t[yard])
        spread = max(b.max() - b.min(), a.max() - a.min())
        return {"speedup": round(float(np.median(b) / np.median(a)), 3), "spread_ms": round(float(spread), 4),
                "faster_by_more_than_the_spread": bool(np.median(b) - np.median(a) > spread)}

    row = {"frustum_set": n_f, "unoccluded": n_v, "hidden_fraction_of_frustum_set": round(1.0 - n_v / max(n_f, 1), 4),
           "early_count": int(c[2]), "late_count": int(c[3]),
           "step_ms": {k: stats(v) for k, v in t.items()},
           "hiz_vs_composition": verdict("hiz", "hiz_composition"),
           "early_late_vs_composition": verdict("early_late", "early_late_composition"),
           "same_bytes": {"hiz": same_hiz, "early_late": same_el, "visible_out_equals_occlusion_mask": vis_equal},
           "pass_ms": {k: round(v, 4) for k, v in med.items()},
           "pass1_TBps": {"hiz": round(n * 145.125 / med["hiz"] / 1e9, 3), "early": round(n * 145.125 / med["early"] / 1e9, 3),
                          "late": round(n * 145.375 / med["late"] / 1e9, 3), "plain": round(n * 145.125 / med["plain"] / 1e9, 3)}}
    result["dists"][dist] = row
    print(f"{dist}: " + json.dumps(row), flush=True)
    del d_i, d_ids

print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
