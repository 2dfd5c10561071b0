"""vd_cull_compact_lod_dev / vd_cull_batch_lod_dev (a level of detail per instance, chosen in pass 1) against
vd_cull_compact_dev / vd_cull_batch_dev on the same instances, in ONE process: the benchmark's camera and cloud, 16 groups
x 4 LODs = 64 rows against the 16 meshes whose boxes the groups carry, thresholds at the quartiles of the projected size
(estimated on a sample), min_size 0 and at the 5 % quantile.
Inputs resident; consecutive steps alternate two instance buffers (the second is the first after one compute_update step:
every transform differs), as bench.py's headline steps do; one HIP event pair per step on the context's stream, median over
the steps after a warm-up.  Two regimes, for BOTH sides:
  ids change   the second buffer's mesh ids are the first's + 1 (mod 16): every row of the id table differs from the
               previous step's and is rewritten - what LOD rows that change with distance cost, and the comparable
               regime for the yardstick;
  ids static   both buffers carry the same mesh ids: only the rows whose LOD changed between the two are rewritten.
The stages come from vd_last_gpu_ms_stage in a loop of their own (event pairs inside a call cost a few us of idle).
Usage (on a GPU box): python tools/bench_cull_lod.py [--n 10000000] [--steps 30] [--warmup 5] [--out result.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voidin_amd import synth  # noqa: E402
from voidin_amd.runtime import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--groups", type=int, default=16)
ap.add_argument("--lods", type=int, default=4)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
assert args.steps >= 20

ctx = Context(0)
n, n_group = args.n, args.groups
cam = synth.camera_uniform()
base = synth.mesh_infos(n_group)
inst = synth.instances(n, n_mesh=n_group, seed=synth.SEED_BASE + 3, with_inverse=False)
scale = float(np.float32(540.0) * np.float32(cam["projection"].reshape(-1)[5]))
min_distance = float(np.asarray(cam["znear"]).reshape(-1)[0])
_, plain_groups = synth.lod_groups(base, args.lods, switch_size=[0.0] * (args.lods - 1))
sample = synth.lod_size_estimate(cam, plain_groups, inst[:: max(n // 200_000, 1)], scale, min_distance)
sample = sample[np.isfinite(sample)]
quantiles = [float(np.quantile(sample, 1.0 - (k + 1) / args.lods)) for k in range(args.lods - 1)]
rows, groups = synth.lod_groups(base, args.lods, switch_size=quantiles)
n_rows = len(rows)

d_a = ctx.upload(inst)
del inst
d_b = d_a.clone()
d_idx = torch.arange(n, dtype=torch.int32, device="cuda")
ctx.compute_update_dev(d_idx, n, d_b, n, 1.0, 0.016)
torch.cuda.synchronize()
mesh_a, mesh_b = [t.view(torch.int32).view(n, 36)[:, 32] for t in (d_a, d_b)]    # VdInstance.mesh: byte 128 of 144
d_g, d_rows, d_base = ctx.upload(groups), ctx.upload(rows), ctx.upload(base)
d_list, d_ids = ctx.empty(n * 20), ctx.empty(n * 4)
d_cmds = ctx.empty(n_rows * 20)
d_cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
step_no = [0]


def src():
    step_no[0] += 1
    return d_a if step_no[0] & 1 else d_b


def per_step_ms(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    return {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "max": round(float(t.max()), 4)}


def stages(fn):
    ctx.set_timing(True)
    for _ in range(args.warmup):
        fn()
    s0, s1 = [], []
    for _ in range(args.steps):
        fn()
        s0.append(ctx.last_gpu_ms_stage(0)); s1.append(ctx.last_gpu_ms_stage(1))
    ctx.set_timing(False)
    return round(float(np.median(s0)), 4), round(float(np.median(s1)), 4)


result = {"n": n, "groups": n_group, "lods": args.lods, "rows": n_rows, "steps": args.steps, "warmup": args.warmup,
          "switch_size": quantiles, "cases": []}
for regime in ("ids change", "ids static"):
    mesh_b.copy_((mesh_a + 1) % n_group if regime == "ids change" else mesh_a)
    torch.cuda.synchronize()
    for min_q in (None, 0.05):
        P = {"scale": scale, "min_distance": min_distance, "min_size": 0.0 if min_q is None else float(np.quantile(sample, min_q))}

        def lod():
            ctx.cull_compact_lod_dev(cam, P, d_g, n_group, d_rows, n_rows, src(), n, d_list, d_cnt, False)

        def plain():
            ctx.cull_compact_dev(cam, d_base, n_group, src(), n, d_list, d_cnt[4:], False)

        def lod_batched():
            ctx.cull_batch_lod_dev(cam, P, d_g, n_group, d_rows, n_rows, src(), n, d_cmds, d_ids, d_cnt)

        def plain_batched():
            ctx.cull_batch_dev(cam, d_base, n_group, src(), n, d_cmds, d_ids, d_cnt[4:])

        row = {"regime": regime, "min_size": P["min_size"]}
        row["plain_ms"] = per_step_ms(plain)
        row["lod_ms"] = per_step_ms(lod)
        row["plain_ms_again"] = per_step_ms(plain)                           # order effects: the first figure once more
        row["plain_batched_ms"] = per_step_ms(plain_batched)
        row["lod_batched_ms"] = per_step_ms(lod_batched)
        row["plain_pass1_ms"], row["plain_expansion_ms"] = stages(plain)
        row["lod_pass1_ms"], row["lod_expansion_ms"] = stages(lod)
        row["plain_batched_pass1_ms"], row["plain_grouping_ms"] = stages(plain_batched)
        row["lod_batched_pass1_ms"], row["lod_grouping_ms"] = stages(lod_batched)
        ctx.cull_compact_lod_dev(cam, P, d_g, n_group, d_rows, n_rows, d_a, n, d_list, d_cnt, False)
        ctx.cull_compact_dev(cam, d_base, n_group, d_a, n, d_list, d_cnt[4:], False)
        row["drawn"], row["in_frustum"] = int(d_cnt[0].item()), int(d_cnt[4].item())
        ctx.cull_batch_lod_dev(cam, P, d_g, n_group, d_rows, n_rows, d_a, n, d_cmds, d_ids, d_cnt)
        torch.cuda.synchronize()
        per_row = d_cmds.cpu().numpy()[: n_rows * 20].view(np.uint32).reshape(n_rows, 5)[:, 1].astype(np.int64)
        row["drawn_per_lod"] = per_row.reshape(n_group, args.lods).sum(axis=0).tolist()
        assert int(per_row.sum()) == row["drawn"] and (row["drawn"] == row["in_frustum"]) == (min_q is None)
        row["lod_over_plain"] = round(row["lod_ms"]["median"] / row["plain_ms"]["median"], 3)
        row["pass1_lod_over_plain"] = round(row["lod_pass1_ms"] / row["plain_pass1_ms"], 3)
        row["batched_lod_over_plain"] = round(row["lod_batched_ms"]["median"] / row["plain_batched_ms"]["median"], 3)
        result["cases"].append(row)
        print(json.dumps(row), flush=True)

print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
