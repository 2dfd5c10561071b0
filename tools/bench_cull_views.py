"""vd_cull_compact_views_dev (K cameras, one read of the instances) against K consecutive vd_cull_compact_dev calls - the
only way to get K views before it - in ONE process, the two alternating, five repetitions each (median, min .. max).
Inputs resident; consecutive steps alternate two instance buffers (the second is the first after one compute_update step:
every transform differs, mesh ids equal), as bench.py's headline steps do; HIP events on the context's stream.
Also: the shared pass 1 alone per K (vd_last_gpu_ms_stage 0) beside cull_mask_tiled_kernel, as TB/s on its algorithmic
bytes 144 + K/8 + 1 per instance, and every view of the first views call compared with the single-view call's bytes.
Usage (on a GPU box): python tools/bench_cull_views.py [--n 10000000] [--views 1,2,3,4,6,8] [--steps 50] [--reps 5]
                                                       [--dists baseline,small] [--out result.json]"""
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
ap.add_argument("--views", default="1,2,3,4,6,8")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--dists", default="baseline,small")
ap.add_argument("--out", default="")
args = ap.parse_args()

CAMERAS = [synth.camera_uniform(),
           synth.camera_uniform(yaw_deg=90.0, pitch_deg=0.0), synth.camera_uniform(yaw_deg=180.0, pitch_deg=0.0),
           synth.camera_uniform(yaw_deg=270.0, pitch_deg=0.0),
           synth.camera_uniform(pitch_deg=89.0), synth.camera_uniform(pitch_deg=-89.0),
           synth.camera_uniform(eye=(100.0, 50.0, -200.0), yaw_deg=45.0, pitch_deg=-30.0),
           synth.camera_uniform(jitter=(0.001, -0.001))]
CLOUDS = {"baseline": dict(scale_range=(0.25, 4.0)), "small": dict(scale_range=(0.02, 0.6), extent=600.0)}

ctx = Context(0)
n = args.n
meshes = synth.mesh_infos()
n_mesh = len(meshes)
d_m = ctx.upload(meshes)
ks = [int(k) for k in args.views.split(",")]
k_max = max(ks)
d_out = ctx.empty(k_max * n * 20)
d_cnt = torch.zeros(16, dtype=torch.int32, device="cuda")
ev = lambda: torch.cuda.Event(enable_timing=True)
result = {"n": n, "steps": args.steps, "reps": args.reps, "dists": {}}

for dist in args.dists.split(","):
    inst = synth.instances(n, seed=synth.SEED_BASE + 3, with_inverse=False, **CLOUDS[dist])
    d_a = ctx.upload(inst)
    del inst
    d_b = d_a.clone()
    d_idx = torch.arange(n, dtype=torch.int32, device="cuda")
    ctx.compute_update_dev(d_idx, n, d_b, n, 1.0, 0.016)
    torch.cuda.synchronize()
    del d_idx
    step_no = [0]

    def src():
        step_no[0] += 1
        return d_a if step_no[0] & 1 else d_b

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

    rows = {}
    for k in ks:
        cams = np.concatenate([np.ascontiguousarray(c, dtype=abi.CAMERA).reshape(1) for c in CAMERAS[:k]])

        def views():
            ctx.cull_compact_views_dev(cams, d_m, n_mesh, src(), n, d_out, d_cnt, False, n)

        def sequential():
            s = src()
            for v in range(k):
                ctx.cull_compact_dev(cams[v], d_m, n_mesh, s, n, d_out[v * n * 20:], d_cnt[v:], False)

        # same bytes first (buffer a): every view of the views call against the single-view call
        step_no[0] = 0
        views()
        torch.cuda.synchronize()
        counts = [int(c) for c in d_cnt[:k].cpu().numpy()]
        d_one, d_c1 = ctx.empty(n * 20), torch.zeros(4, dtype=torch.int32, device="cuda")
        same = True
        for v in range(k):
            ctx.cull_compact_dev(cams[v], d_m, n_mesh, d_a, n, d_one, d_c1, False)
            torch.cuda.synchronize()
            c1 = int(d_c1[0].item())
            same = same and c1 == counts[v] and torch.equal(d_one[: c1 * 20], d_out[v * n * 20: v * n * 20 + c1 * 20])
        del d_one
        t_views, t_seq = [], []
        for _ in range(args.reps):
            t_views.append(timed(views))
            t_seq.append(timed(sequential))
        # the passes alone (event pairs around each pass cost a few us of idle: not part of the step times above)
        ctx.set_timing(True)
        p1, p2, s1 = [], [], []
        for _ in range(args.steps):
            views()
            if k > 1:
                p1.append(ctx.last_gpu_ms_stage(0)); p2.append(ctx.last_gpu_ms_stage(1))
            ctx.cull_compact_dev(cams[0], d_m, n_mesh, src(), n, d_out, d_cnt, False)
            s1.append(ctx.last_gpu_ms_stage(0))
        ctx.set_timing(False)
        tv, ts = np.array(t_views), np.array(t_seq)
        row = {"views_ms": {"median": round(float(np.median(tv)), 4), "min": round(float(tv.min()), 4), "max": round(float(tv.max()), 4)},
               "sequential_ms": {"median": round(float(np.median(ts)), 4), "min": round(float(ts.min()), 4), "max": round(float(ts.max()), 4)},
               "sequential_spread_pct": round(float((ts.max() - ts.min()) / np.median(ts) * 100), 2),
               "speedup": round(float(np.median(ts) / np.median(tv)), 3),
               "faster_by_more_than_the_spread": bool(np.median(ts) - np.median(tv) > ts.max() - ts.min()),
               "survivors": counts, "views_equal_single_view_calls": bool(same),
               "single_view_pass1_ms": round(float(np.median(s1)), 4),
               "single_view_pass1_TBps": round(n * 145.125 / np.median(s1) / 1e9, 3)}
        if k > 1:
            row.update({"pass1_ms": round(float(np.median(p1)), 4), "expansions_ms": round(float(np.median(p2)), 4),
                        "pass1_TBps": round(n * (145.0 + k / 8.0) / np.median(p1) / 1e9, 3)})
        rows[str(k)] = row
        print(f"{dist} K={k}: " + json.dumps(row), flush=True)
    result["dists"][dist] = rows
    del d_a, d_b

print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
