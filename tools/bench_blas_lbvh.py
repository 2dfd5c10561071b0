"""vd_bvh_build_lbvh_dev against vd_bvh_build_dev of the SAME mesh, from device arrays, in ONE process, alternating the two: the
15 k-triangle helmet fixture and the knots of tools/bench_bvh.py at 131 072, 524 288 and 8 388 608 triangles.
Method: everything resident; both builders permute the indices in place, so the indices are restored outside the timed region.
The exact build blocks and is timed on the host clock between two synchronisations; the LBVH build only enqueues and is timed the
same way (what a caller who waits for it sees) AND by a HIP event pair (what it costs on the stream).  A warm-up, then the median
with the range over the steps; the two builders take turns step by step.
--graph: the LBVH build captured into a HIP graph, timed per replay by an event pair.
--trace: bench.py's stress scene (2 000 instances of the 131 072-triangle knot, 1 Mi primary rays, prepared path, closest hit and
any hit) over the exact bottom level and over the LBVH one in the same run, alternating; the ratio of the rates, node counts,
max_depth.
--profile T: nothing but a warm-up and a few LBVH builds of a T-triangle knot, for a kernel-trace run of a profiler around this
script (the timings above are taken with the profiler off).
Usage (on a GPU box): python tools/bench_blas_lbvh.py [--cases helmet,knot131k,knot524k,knot8m] [--steps 50] [--warmup 5] [--graph]
                                                      [--trace] [--profile 1048576] [--out result.json] [--md table.md]"""
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
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--graph", action="store_true")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--profile", type=int, default=0)
ap.add_argument("--out", default="")
ap.add_argument("--md", default="")
args = ap.parse_args()

ctx = Context(0)


def helmet():
    g = np.load(os.path.join(ROOT, "tests", "golden", "helmet.npz"))
    return np.ascontiguousarray(g["vertices"], dtype=np.float32), np.ascontiguousarray(g["indices"], dtype=np.uint32)


def stats(samples):
    t = np.array(samples)
    return {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "max": round(float(t.max()), 4)}


class Mesh:
    def __init__(self, v, i):
        self.n_vert, self.n_tri = len(v), len(i) // 3
        self.cap = max(2, 2 * self.n_tri)
        self.d_v, self.d_i0 = ctx.upload(v), ctx.upload(i)
        self.d_i = self.d_i0.clone()
        self.d_exact = torch.zeros(self.cap * 32, dtype=torch.uint8, device="cuda")
        self.d_lbvh = torch.zeros(self.cap * 32, dtype=torch.uint8, device="cuda")
        self.d_res = torch.zeros(16, dtype=torch.uint8, device="cuda")

    def restore(self):
        self.d_i.copy_(self.d_i0)

    def exact(self):
        return ctx.bvh_build_dev(self.d_v, self.n_vert, self.d_i, self.n_tri, self.d_exact, self.cap)

    def lbvh(self):
        ctx.bvh_build_lbvh_dev(self.d_v, self.n_vert, self.d_i, self.n_tri, self.d_lbvh, self.cap, self.d_res)

    def result(self):
        torch.cuda.synchronize()
        return self.d_res.cpu().numpy().view(abi.BVH_LBVH_RESULT)[0]


def run_case(name, v, i):
    m = Mesh(v, i)
    t_exact, t_lbvh, t_lbvh_ev = [], [], []
    n_exact = 0
    for k in range(args.warmup + args.steps):
        m.restore(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_exact = m.exact()
        torch.cuda.synchronize()
        a = (time.perf_counter() - t0) * 1e3
        m.restore(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(); m.lbvh(); e1.record()
        torch.cuda.synchronize()
        b = (time.perf_counter() - t0) * 1e3
        if k >= args.warmup:
            t_exact.append(a); t_lbvh.append(b); t_lbvh_ev.append(e0.elapsed_time(e1))
    res = m.result()
    row = {"case": name, "triangles": m.n_tri, "exact_ms": stats(t_exact), "lbvh_ms": stats(t_lbvh), "lbvh_stream_ms": stats(t_lbvh_ev),
           "exact_nodes": int(n_exact), "lbvh_nodes": int(res["n_nodes"]), "lbvh_max_depth": int(res["max_depth"]),
           "exact_over_lbvh": round(float(np.median(t_exact) / np.median(t_lbvh)), 2)}
    if args.graph and m.n_tri <= 200_000:
        m.restore(); m.lbvh(); torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        main_stream = torch.cuda.current_stream().cuda_stream
        try:
            with torch.cuda.graph(graph):
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                m.lbvh()
        finally:
            ctx.set_stream(main_stream)
        t_g = []
        for k in range(args.warmup + args.steps):
            m.restore(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); graph.replay(); e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                t_g.append(e0.elapsed_time(e1))
        row["lbvh_graph_replay_ms"] = stats(t_g)
    print(json.dumps(row), flush=True)
    return row


def trace_case():
    tv, ti = synth.knot_mesh(512, 128)
    infos = np.zeros(1, dtype=abi.MESH_INFO)
    infos[0]["min"], infos[0]["max"] = synth.mesh_bounds(tv)
    infos[0]["index_count"] = len(ti)
    inst = synth.instances(2000, n_mesh=1, seed=synth.SEED_BASE + 8, extent=120.0, scale_range=(0.5, 2.0))
    tl = ctx.tlas_build(inst, infos)
    rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 90), pitch_deg=0), 1024, 1024)
    d_rays, d_hits = ctx.upload(rays), ctx.empty(len(rays) * 16)
    d_any = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
    nodes_e, idx_e = ctx.bvh_build(tv, ti)
    nodes_l, idx_l = ctx.bvh_build_lbvh(tv, ti)
    m = Mesh(tv, ti); m.lbvh(); depth = int(m.result()["max_depth"])
    accs = {"exact": ctx.trace_prepare(ctx.device_scene((tl, inst, infos, nodes_e, tv, idx_e))),
            "lbvh": ctx.trace_prepare(ctx.device_scene((tl, inst, infos, nodes_l, tv, idx_l)))}
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
    rate = {k: {q: round(len(rays) / float(np.median(v)) / 1e3, 1) for q, v in d.items()} for k, d in t.items()}
    row = {"case": "trace", "n_rays": len(rays), "scene": "2000 instances x 131 072-triangle knot", "Mrays_per_s": rate,
           "lbvh_over_exact": {q: round(rate["lbvh"][q] / rate["exact"][q], 3) for q in ("closest", "any")},
           "exact_nodes": len(nodes_e), "lbvh_nodes": len(nodes_l), "lbvh_max_depth": depth,
           "same_hit_flags": bool(np.array_equal(hit["exact"], hit["lbvh"]))}
    print(json.dumps(row), flush=True)
    return row


CASES = {"helmet": helmet, "knot131k": lambda: synth.knot_mesh(512, 128), "knot524k": lambda: synth.knot_mesh(1024, 256),
         "knot8m": lambda: synth.knot_mesh(2048, 2048)}

if args.profile:
    u = 1 << int(np.ceil(np.log2(max(4.0, (args.profile / 2) ** 0.5))))      # a power of two: 1 048 576 -> 1024 x 512 quads
    v, i = synth.knot_mesh(u, args.profile // (2 * u))
    m = Mesh(v, i)
    for _ in range(2 + 5):
        m.restore(); m.lbvh()
    print(json.dumps({"profiled_triangles": m.n_tri, "n_nodes": int(m.result()["n_nodes"])}))
    sys.exit(0)

rows = [run_case(c, *CASES[c]()) for c in args.cases.split(",") if c]
if args.trace:
    rows.append(trace_case())
result = {"steps": args.steps, "warmup": args.warmup, "cases": rows}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
if args.md:
    lines = ["| case | triangles | exact build ms (median, min-max) | LBVH build ms, host clock | LBVH build ms, on the stream | graph replay ms | exact / LBVH | exact nodes | LBVH nodes | LBVH max_depth |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["case"] == "trace":
            continue
        g = r.get("lbvh_graph_replay_ms")
        lines.append("| {case} | {triangles} | {a[median]} ({a[min]}-{a[max]}) | {b[median]} ({b[min]}-{b[max]}) | {c[median]} ({c[min]}-{c[max]}) | {g} | {exact_over_lbvh} | {exact_nodes} | {lbvh_nodes} | {lbvh_max_depth} |".format(
            a=r["exact_ms"], b=r["lbvh_ms"], c=r["lbvh_stream_ms"], g="{median} ({min}-{max})".format(**g) if g else "not measured", **r))
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write("\n".join(lines) + "\n")
