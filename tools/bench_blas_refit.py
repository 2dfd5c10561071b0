"""vd_bvh_refit_planned_dev against vd_bvh_build_dev (vd_bvh_build_batch_dev for the batch) of the SAME data, from device
arrays, in ONE process: the 15 k-triangle helmet fixture, knot meshes of 131 k and 524 k triangles, the 8.4 M-triangle
bench mesh, and a packed batch of 64 helmets in one plan.
Method: everything resident; two vertex buffers (the mesh and a smooth deformation of it) alternate from step to step - a
plan keeps its items' pointers, so there is one plan per vertex buffer over the same nodes; a warm-up, then the median over
the steps.  A refit only enqueues: one HIP event pair per step on the context's stream.  A build blocks and permutes the
indices in place: the indices are restored outside the timed region and the call is timed on the host clock between two
synchronisations (it returns when the nodes are complete).
A/B in the same loop: the refit with VD_OPT_BLAS_REFIT_FENCES = 1 (an agent-scope fence pair per hand-over), then the default again.
Bandwidth: the fraction of 8 TB/s the refit reaches on ALGORITHMIC bytes - T * (12 + 36) read (indices, three vertices per
triangle), nodes * 32 written, nodes * 8 for parent ids and arrival counters.
Usage (on a GPU box): python tools/bench_blas_refit.py [--cases helmet,knot131k,knot524k,knot8m,helmets64] [--steps 50]
                                                       [--build-steps 10] [--warmup 5] [--out result.json] [--md table.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voidin_amd import abi, synth  # noqa: E402
from voidin_amd.runtime import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="helmet,knot131k,knot524k,knot8m,helmets64")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--build-steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--md", default="")
args = ap.parse_args()

PEAK = 8e12
ctx = Context(0)


def helmet():
    g = np.load(os.path.join(ROOT, "tests", "golden", "helmet.npz"))
    return np.ascontiguousarray(g["vertices"], dtype=np.float32), np.ascontiguousarray(g["indices"], dtype=np.uint32)


def bend(v, phase):
    p = v.astype(np.float64)
    s = float(np.abs(p).max()) or 1.0
    d = np.stack([np.sin(4.0 * p[:, 1] / s + phase), np.cos(3.0 * p[:, 2] / s - phase), np.sin(5.0 * p[:, 0] / s + 2 * phase)], axis=1)
    return (p + 0.05 * s * d).astype(np.float32)


def median_ms(samples):
    t = np.array(samples)
    return {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "max": round(float(t.max()), 4)}


def events_ms(fn, steps):
    for k in range(args.warmup):
        fn(k)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for k, (e0, e1) in enumerate(ev):
        e0.record()
        fn(k)
        e1.record()
    torch.cuda.synchronize()
    return median_ms([e0.elapsed_time(e1) for e0, e1 in ev])


def host_ms(prepare, fn, steps):
    out = []
    for k in range(args.warmup + steps):
        prepare(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        torch.cuda.synchronize()
        if k >= args.warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return median_ms(out)


def run_case(name, meshes):
    """meshes: [(v, i)]; one mesh = vd_bvh_build_dev, several = vd_bvh_build_batch_dev into one packed node buffer."""
    K = len(meshes)
    n_tri = sum(len(i) // 3 for _, i in meshes)
    d_va = [ctx.upload(v) for v, _ in meshes]
    d_vb = [ctx.upload(bend(v, 0.7 + 0.01 * m)) for m, (v, _) in enumerate(meshes)]
    d_i0 = [ctx.upload(i) for _, i in meshes]
    d_i = [t.clone() for t in d_i0]
    cap = sum(max(2 * (len(i) // 3), 2) for _, i in meshes)
    d_nodes = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    d_infos = torch.zeros(K * 48, dtype=torch.uint8, device="cuda")

    def restore(_k):
        for a, b in zip(d_i, d_i0):
            a.copy_(b)

    batch = (abi.BvhBatchItem * K)()

    def build(k):
        src = d_va if k % 2 == 0 else d_vb
        if K == 1:
            return [(0, ctx.bvh_build_dev(src[0], len(meshes[0][0]), d_i[0], len(meshes[0][1]) // 3, d_nodes, cap))]
        for m in range(K):
            batch[m].verts_xyz, batch[m].indices_inout, batch[m].out_nodes = abi.ptr(src[m]), abi.ptr(d_i[m]), None
            batch[m].n_vert, batch[m].n_tri, batch[m].node_cap = len(meshes[m][0]), len(meshes[m][1]) // 3, 0
        ctx.bvh_build_batch_dev(batch, K, d_nodes, cap, 0)
        return [(int(batch[m].out_first_node), int(batch[m].out_n_nodes)) for m in range(K)]

    build_ms = host_ms(restore, build, args.build_steps)
    restore(0)
    layout = build(0)                                             # the topology the plans are made for: built from buffer A
    n_nodes = sum(n for _, n in layout)
    plans = []
    for src in (d_va, d_vb):
        items = (abi.BvhRefitItem * K)()
        for m, (first, n) in enumerate(layout):
            items[m].verts_xyz, items[m].indices, items[m].nodes = abi.ptr(src[m]), abi.ptr(d_i[m]), abi.ptr(d_nodes) + 32 * first
            items[m].mesh_info = abi.ptr(d_infos) + 48 * m
            items[m].n_vert, items[m].n_tri, items[m].n_nodes = len(meshes[m][0]), len(meshes[m][1]) // 3, n
        t0 = time.perf_counter()
        plans.append(ctx.bvh_refit_plan(items))
        plan_ms = (time.perf_counter() - t0) * 1e3
    built = d_nodes.clone()
    refit_ms = events_ms(lambda k: ctx.bvh_refit_planned(plans[k % 2]), args.steps)
    ctx.set_option("blas.refit_fences", 1)                        # A/B: an agent-scope release / acquire fence pair per hand-over on top
    fenced_ms = events_ms(lambda k: ctx.bvh_refit_planned(plans[k % 2]), args.steps)
    ctx.set_option("blas.refit_fences", None)
    refit_again_ms = events_ms(lambda k: ctx.bvh_refit_planned(plans[k % 2]), args.steps)      # order effects: the first figure once more
    ctx.bvh_refit_planned(plans[0]); torch.cuda.synchronize()
    identity = bool(torch.equal(built, d_nodes))                  # refit(build(x), x) == build(x), checked on the way
    algo_bytes = n_tri * 48 + n_nodes * 32 + n_nodes * 8
    row = {"case": name, "meshes": K, "triangles": n_tri, "nodes": n_nodes, "refit_ms": refit_ms, "refit_ms_again": refit_again_ms, "refit_with_fences_ms": fenced_ms, "build_ms": build_ms,
           "plan_ms_once": round(plan_ms, 3), "build_over_refit": round(build_ms["median"] / refit_ms["median"], 1),
           "algorithmic_bytes": algo_bytes, "fraction_of_8TBps": round(algo_bytes / (refit_ms["median"] * 1e-3) / PEAK, 4),
           "identity_holds": identity}
    for p in plans:
        p.close()
    print(json.dumps(row), flush=True)
    return row


CASES = {"helmet": lambda: [helmet()], "knot131k": lambda: [synth.knot_mesh(512, 128)], "knot524k": lambda: [synth.knot_mesh(1024, 256)],
         "knot8m": lambda: [synth.knot_mesh(2048, 2048)], "helmets64": lambda: [helmet()] * 64}
rows = [run_case(c, CASES[c]()) for c in args.cases.split(",") if c]
result = {"steps": args.steps, "build_steps": args.build_steps, "warmup": args.warmup, "cases": rows}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
if args.md:
    lines = ["| case | triangles | nodes | refit ms (median, min-max) | the same again | refit with fences ms | rebuild ms (median, min-max) | rebuild / refit | algorithmic bytes | of 8 TB/s | plan, once, ms | refit(build(x), x) == build(x) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| {case} | {triangles} | {nodes} | {a[median]} ({a[min]}-{a[max]}) | {c[median]} | {d[median]} ({d[min]}-{d[max]}) | {b[median]} ({b[min]}-{b[max]}) | {build_over_refit} | {algorithmic_bytes} | {f:.2%} | {plan_ms_once} | {ok} |".format(
            a=r["refit_ms"], b=r["build_ms"], c=r["refit_ms_again"], d=r["refit_with_fences_ms"], f=r["fraction_of_8TBps"],
            ok="yes" if r["identity_holds"] else "NO", **r))
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write("\n".join(lines) + "\n")
