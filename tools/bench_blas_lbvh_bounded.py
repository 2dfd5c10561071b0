"""The depth-bounded LBVH bottom level (VD_OPT_BLAS_LBVH_MAX_DEPTH) against the UNBOUNDED build of the same mesh in ONE process,
the two taking turns step by step: what the two added passes cost, and what the bounded tree costs a trace.
  builds   the helmet fixture and the knots of tools/bench_blas_lbvh.py: vd_bvh_build_lbvh_dev from device arrays with the option at
           0 and at --bound, on the host clock between two synchronisations and by an event pair on the stream; with --graph each
           captured into a HIP graph (<= 200 000 triangles) and timed per replay.
  batches  --batch: 256 soups of 1 024 triangles and 64 helmets, one plan made with the option at 0 and one at --bound, per
           vd_bvh_build_lbvh_planned_dev by an event pair.
  trace    --trace: bench.py's stress scene (2 000 instances, 1 Mi primary rays, prepared path, closest hit and any hit) over the
           131 072-triangle knot and over the helmet, each built unbounded, at --bound and at --tight, alternating; the ratios of
           the rates to the unbounded tree's.
  --profile T: nothing but a warm-up and a few bounded builds of a T-triangle knot, for a kernel-trace run of a profiler around
           this script.
Usage (on a GPU box): python tools/bench_blas_lbvh_bounded.py [--cases helmet,knot131k,knot524k,knot8m] [--bound 23] [--tight 16]
                      [--steps 50] [--warmup 5] [--graph] [--batch] [--trace] [--profile 15452] [--out result.json]"""
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
ap.add_argument("--cases", default="helmet,knot131k,knot524k,knot8m")
ap.add_argument("--bound", type=int, default=23)
ap.add_argument("--tight", type=int, default=16)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--graph", action="store_true")
ap.add_argument("--batch", action="store_true")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--profile", type=int, default=0)
ap.add_argument("--out", default="")
args = ap.parse_args()

OPTION = "blas.lbvh_max_depth"
ctx = Context(0)


def helmet():
    g = np.load(os.path.join(ROOT, "tests", "golden", "helmet.npz"))
    return np.ascontiguousarray(g["vertices"], dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(g["indices"], dtype=np.uint32).reshape(-1)


def stats(samples):
    t = np.array(samples)
    return {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "max": round(float(t.max()), 4)}


class Mesh:
    def __init__(self, v, i):
        self.n_vert, self.n_tri = len(v), len(i) // 3
        self.cap = max(2, 2 * self.n_tri)
        self.d_v, self.d_i0 = ctx.upload(v), ctx.upload(i)
        self.d_i = self.d_i0.clone()
        self.d_nodes = torch.zeros(self.cap * 32, dtype=torch.uint8, device="cuda")
        self.d_res = torch.zeros(16, dtype=torch.uint8, device="cuda")

    def restore(self):
        self.d_i.copy_(self.d_i0)

    def build(self):
        ctx.bvh_build_lbvh_dev(self.d_v, self.n_vert, self.d_i, self.n_tri, self.d_nodes, self.cap, self.d_res)

    def result(self):
        torch.cuda.synchronize()
        return self.d_res.cpu().numpy().view(abi.BVH_LBVH_RESULT)[0]


def capture(m, bound):
    ctx.set_option(OPTION, bound)
    m.restore(); m.build(); torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    main_stream = torch.cuda.current_stream().cuda_stream
    try:
        with torch.cuda.graph(graph):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            m.build()
    finally:
        ctx.set_stream(main_stream)
    return graph


def run_case(name, v, i):
    m = Mesh(v, i)
    bounds = {"unbounded": 0, "bounded": args.bound}
    host, stream, res = {k: [] for k in bounds}, {k: [] for k in bounds}, {}
    for k in range(args.warmup + args.steps):
        for which, D in bounds.items():                  # taking turns
            ctx.set_option(OPTION, D)
            m.restore(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(); m.build(); e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                host[which].append((time.perf_counter() - t0) * 1e3); stream[which].append(e0.elapsed_time(e1))
            if k == 0:
                res[which] = m.result().copy()
    row = {"case": name, "triangles": m.n_tri, "bound": args.bound}
    for which in bounds:
        row[which] = {"host_ms": stats(host[which]), "stream_ms": stats(stream[which]), "n_nodes": int(res[which]["n_nodes"]),
                      "max_depth": int(res[which]["max_depth"])}
    row["bounded_over_unbounded"] = {"host": round(float(np.median(host["bounded"]) / np.median(host["unbounded"])), 3),
                                     "stream": round(float(np.median(stream["bounded"]) / np.median(stream["unbounded"])), 3)}
    if args.graph and m.n_tri <= 200_000:
        graphs = {which: capture(m, D) for which, D in bounds.items()}
        t_g = {which: [] for which in bounds}
        for k in range(args.warmup + args.steps):
            for which, g in graphs.items():
                m.restore(); torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); g.replay(); e1.record()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    t_g[which].append(e0.elapsed_time(e1))
        for which in bounds:
            row[which]["graph_replay_ms"] = stats(t_g[which])
    ctx.set_option(OPTION, None)
    print(json.dumps(row), flush=True)
    return row


def batch_case(name, meshes):
    K = len(meshes)
    caps = [len(i) // 3 for _, i in meshes]
    d_v = [ctx.upload(v) for v, _ in meshes]
    d_i0 = [ctx.upload(i) for _, i in meshes]
    d_i = [t.clone() for t in d_i0]
    d_n = [torch.zeros(64 * c, dtype=torch.uint8, device="cuda") for c in caps]
    d_res = torch.zeros(16 * K, dtype=torch.uint8, device="cuda")
    items = (abi.BvhLbvhBatchItem * K)()
    for m, (v, _) in enumerate(meshes):
        it = items[m]
        it.verts_xyz, it.indices_inout, it.nodes, it.mesh_info = abi.ptr(d_v[m]), abi.ptr(d_i[m]), abi.ptr(d_n[m]), None
        it.n_vert, it.tri_cap, it.node_cap = len(v), caps[m], 2 * caps[m]
    plans = {}
    for which, D in (("unbounded", 0), ("bounded", args.bound)):
        ctx.set_option(OPTION, D)
        plans[which] = ctx.bvh_lbvh_plan(items)          # the plan latches the option
    ctx.set_option(OPTION, None)
    t, depth = {k: [] for k in plans}, {}
    for k in range(args.warmup + args.steps):
        for which, plan in plans.items():
            for a, b in zip(d_i, d_i0):
                a.copy_(b)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); ctx.bvh_build_lbvh_planned_dev(plan, None, d_res); e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                t[which].append(e0.elapsed_time(e1))
            depth[which] = int(d_res.cpu().numpy().view(abi.BVH_LBVH_RESULT)["max_depth"].max())
    for plan in plans.values():
        plan.close()
    row = {"case": name, "meshes": K, "triangles": int(sum(caps)), "bound": args.bound,
           "unbounded": {"stream_ms": stats(t["unbounded"]), "max_depth": depth["unbounded"]},
           "bounded": {"stream_ms": stats(t["bounded"]), "max_depth": depth["bounded"]},
           "bounded_over_unbounded": round(float(np.median(t["bounded"]) / np.median(t["unbounded"])), 3)}
    print(json.dumps(row), flush=True)
    return row


def trace_case(name, tv, ti):
    infos = np.zeros(1, dtype=abi.MESH_INFO)
    infos[0]["min"], infos[0]["max"] = synth.mesh_bounds(tv)
    infos[0]["index_count"] = len(ti)
    inst = synth.instances(2000, n_mesh=1, seed=synth.SEED_BASE + 8, extent=120.0, scale_range=(0.5, 2.0))
    tl = ctx.tlas_build(inst, infos)
    rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 90), pitch_deg=0), 1024, 1024)
    d_rays, d_hits = ctx.upload(rays), ctx.empty(len(rays) * 16)
    d_any = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
    accs, depth = {}, {}
    for which, D in (("unbounded", 0), ("bounded", args.bound), ("tight", args.tight)):
        ctx.set_option(OPTION, D)
        nodes, idx = ctx.bvh_build_lbvh(tv, ti)
        m = Mesh(tv, ti); m.build(); depth[which] = int(m.result()["max_depth"])
        accs[which] = ctx.trace_prepare(ctx.device_scene((tl, inst, infos, nodes, tv, idx)))
    ctx.set_option(OPTION, None)
    ctx.set_option("trace.fan", 3)
    ctx.set_timing(True)
    t = {k: {"closest": [], "any": []} for k in accs}
    hit = {}
    for rep in range(args.warmup + 10):
        for k, acc in accs.items():                      # alternating
            ctx.trace_prepared_dev(acc, d_rays, len(rays), d_hits); torch.cuda.synchronize(); a = ctx.last_gpu_ms()
            ctx.trace_any_prepared_dev(acc, d_rays, len(rays), d_any); torch.cuda.synchronize(); b = ctx.last_gpu_ms()
            if rep >= args.warmup:
                t[k]["closest"].append(a); t[k]["any"].append(b)
            hit[k] = d_hits.cpu().numpy()[: len(rays) * 16].view(abi.HIT)["hit"].copy()
    ctx.set_timing(False)
    ctx.set_option("trace.fan", None)
    for acc in accs.values():
        acc.close()
    rate = {k: {q: round(len(rays) / float(np.median(v)) / 1e3, 1) for q, v in d.items()} for k, d in t.items()}
    row = {"case": "trace_" + name, "n_rays": len(rays), "scene": f"2000 instances x {len(ti) // 3}-triangle {name}", "Mrays_per_s": rate,
           "bounds": {"bounded": args.bound, "tight": args.tight}, "max_depth": depth, "hits": int(hit["unbounded"].sum()),
           "over_unbounded": {k: {q: round(rate[k][q] / rate["unbounded"][q], 3) for q in ("closest", "any")} for k in ("bounded", "tight")},
           "same_hit_flags": bool(np.array_equal(hit["unbounded"], hit["bounded"]) and np.array_equal(hit["unbounded"], hit["tight"]))}
    print(json.dumps(row), flush=True)
    return row


CASES = {"helmet": helmet, "knot131k": lambda: synth.knot_mesh(512, 128), "knot524k": lambda: synth.knot_mesh(1024, 256),
         "knot8m": lambda: synth.knot_mesh(2048, 2048)}

if args.profile:
    if args.profile == 15452:
        v, i = helmet()
    else:
        u = 1 << int(np.ceil(np.log2(max(4.0, (args.profile / 2) ** 0.5))))
        v, i = synth.knot_mesh(u, args.profile // (2 * u))
    m = Mesh(v, i)
    ctx.set_option(OPTION, args.bound)
    for _ in range(2 + 5):
        m.restore(); m.build()
    print(json.dumps({"profiled_triangles": m.n_tri, "n_nodes": int(m.result()["n_nodes"]), "max_depth": int(m.result()["max_depth"])}))
    sys.exit(0)

rows = [run_case(c, *CASES[c]()) for c in args.cases.split(",") if c]
if args.batch:
    rows.append(batch_case("256 x 1024", [synth.triangle_soup(1024, seed=synth.SEED_BASE + 700 + m) for m in range(256)]))
    rows.append(batch_case("64 helmets", [helmet()] * 64))
if args.trace:
    rows.append(trace_case("knot", *synth.knot_mesh(512, 128)))
    rows.append(trace_case("helmet", *helmet()))
result = {"steps": args.steps, "warmup": args.warmup, "cases": rows}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
