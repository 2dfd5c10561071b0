"""vd_bvh_build_lbvh_planned_dev (many meshes, one call) against a loop of vd_bvh_build_lbvh_dev over the SAME meshes, in ONE process,
the legs taking turns step by step:
  (a) loop     one vd_bvh_build_lbvh_dev per mesh, back to back on the stream;
  (b) planned  one vd_bvh_build_lbvh_planned_dev over a plan of all meshes, the counts in device memory;
  (c) graph    (b) captured into a HIP graph, one replay;
  (d) floor    ONE vd_bvh_build_lbvh_dev of a triangle soup with as many triangles as the whole batch.
Method: everything resident; every leg permutes the indices in place, so they are restored outside the timed region.  Each step of
each leg is timed by an event pair on the stream; a warm-up, then the median with the range over the steps.
Cases: 16 / 256 / 4 096 soups of 1 024 triangles, 256 soups of 100 triangles, 64 copies of the 15 k-triangle helmet fixture.
--profile CASE: nothing but a warm-up and a few planned builds of that case, for a kernel-trace run of a profiler around this script
(the timings above are taken with the profiler off).
Usage (on a GPU box): python tools/bench_blas_lbvh_batch.py [--cases m16x1024,m256x1024,m4096x1024,m256x100,helmet64] [--steps 50]
                                                            [--warmup 5] [--profile m256x1024] [--out result.json] [--md table.md]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voidin_amd import abi, synth  # noqa: E402
from voidin_amd.runtime import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="m16x1024,m256x1024,m4096x1024,m256x100,helmet64")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--profile", default="")
ap.add_argument("--out", default="")
ap.add_argument("--md", default="")
args = ap.parse_args()

ctx = Context(0)
lib = ctx.lib


def stats(samples):
    t = np.array(samples)
    return {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "max": round(float(t.max()), 4)}


def soups(k, t):
    return [synth.triangle_soup(t, seed=synth.SEED_BASE + 900 + m) for m in range(k)]


def helmets(k):
    g = np.load(os.path.join(ROOT, "tests", "golden", "helmet.npz"))
    v, i = np.ascontiguousarray(g["vertices"], dtype=np.float32), np.ascontiguousarray(g["indices"], dtype=np.uint32)
    return [(v + np.float32(m), i) for m in range(k)]


class Meshes:
    """K meshes in three device arrays (vertices, indices, nodes: each mesh at a 256-byte aligned offset) + K result records."""

    def __init__(self, meshes, plan=True):
        self.K = len(meshes)
        self.n_vert = [len(v) for v, _ in meshes]
        self.n_tri = [len(i) // 3 for _, i in meshes]
        up = lambda b: (b + 255) & ~255  # noqa: E731
        self.ov = np.concatenate([[0], np.cumsum([up(12 * n) for n in self.n_vert])]).astype(np.int64)
        self.oi = np.concatenate([[0], np.cumsum([up(12 * t) for t in self.n_tri])]).astype(np.int64)
        self.on = np.concatenate([[0], np.cumsum([up(32 * max(2, 2 * t)) for t in self.n_tri])]).astype(np.int64)
        hv, hi = np.zeros(self.ov[-1], dtype=np.uint8), np.zeros(self.oi[-1], dtype=np.uint8)
        for m, (v, i) in enumerate(meshes):
            hv[self.ov[m]: self.ov[m] + 12 * self.n_vert[m]] = np.ascontiguousarray(v, dtype=np.float32).view(np.uint8).reshape(-1)
            hi[self.oi[m]: self.oi[m] + 12 * self.n_tri[m]] = np.ascontiguousarray(i, dtype=np.uint32).view(np.uint8).reshape(-1)
        self.d_v, self.d_i0 = torch.from_numpy(hv).cuda(), torch.from_numpy(hi).cuda()
        self.d_i = self.d_i0.clone()
        self.d_n = torch.zeros(int(self.on[-1]), dtype=torch.uint8, device="cuda")
        self.d_res = torch.zeros(16 * self.K, dtype=torch.uint8, device="cuda")
        self.d_cnt = torch.from_numpy(np.array(self.n_tri, dtype=np.uint32).view(np.int32)).cuda()
        pv, pi, pn, pr = self.d_v.data_ptr(), self.d_i.data_ptr(), self.d_n.data_ptr(), self.d_res.data_ptr()
        self.single_args = [(pv + int(self.ov[m]), self.n_vert[m], pi + int(self.oi[m]), self.n_tri[m], pn + int(self.on[m]), max(2, 2 * self.n_tri[m]),
                             pr + 16 * m) for m in range(self.K)]
        self.items = (abi.BvhLbvhBatchItem * self.K)()
        for m, a in enumerate(self.single_args):
            it = self.items[m]
            it.verts_xyz, it.n_vert, it.indices_inout, it.tri_cap, it.nodes, it.node_cap = a[:6]
            it.mesh_info = None
        self.plan = ctx.bvh_lbvh_plan(self.items) if plan else None

    def restore(self):
        self.d_i.copy_(self.d_i0)

    def loop(self):
        for a in self.single_args:
            rc = lib.vd_bvh_build_lbvh_dev(ctx.h, *a)
            assert rc == 0, rc

    def planned(self):
        ctx.bvh_build_lbvh_planned_dev(self.plan, self.d_cnt, self.d_res)

    def results(self):
        torch.cuda.synchronize()
        return self.d_res.cpu().numpy().view(abi.BVH_LBVH_RESULT).copy()


def timed(restore, fn):
    restore(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def capture(fn):
    graph = torch.cuda.CUDAGraph()
    main_stream = torch.cuda.current_stream().cuda_stream
    try:
        with torch.cuda.graph(graph):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            fn()
    finally:
        ctx.set_stream(main_stream)
    return graph


def run_case(name, meshes):
    b = Meshes(meshes)
    total = sum(b.n_tri)
    floor = Meshes([synth.triangle_soup(total, seed=synth.SEED_BASE + 899)], plan=False)
    b.restore(); b.loop(); want = b.results()
    b.restore(); b.planned(); got = b.results()
    assert got.tobytes() == want.tobytes(), "the planned build's results differ from the loop's"
    floor.loop(); torch.cuda.synchronize()
    graph = capture(b.planned)
    t = {"loop": [], "planned": [], "graph": [], "floor": []}
    for k in range(args.warmup + args.steps):
        s = {"loop": timed(b.restore, b.loop), "planned": timed(b.restore, b.planned), "graph": timed(b.restore, graph.replay),
             "floor": timed(floor.restore, floor.loop)}
        if k >= args.warmup:
            for leg, ms in s.items():
                t[leg].append(ms)
    assert b.results().tobytes() == want.tobytes(), "the replayed build's results differ from the loop's"
    row = {"case": name, "meshes": b.K, "triangles": total, "loop_ms": stats(t["loop"]), "planned_ms": stats(t["planned"]), "graph_ms": stats(t["graph"]),
           "floor_ms": stats(t["floor"]), "loop_over_planned": round(float(np.median(t["loop"]) / np.median(t["planned"])), 1),
           "planned_over_floor": round(float(np.median(t["planned"]) / np.median(t["floor"])), 2)}
    print(json.dumps(row), flush=True)
    b.plan.close()
    return row


CASES = {"m16x1024": lambda: soups(16, 1024), "m256x1024": lambda: soups(256, 1024), "m4096x1024": lambda: soups(4096, 1024),
         "m256x100": lambda: soups(256, 100), "helmet64": lambda: helmets(64)}

if args.profile:
    b = Meshes(CASES[args.profile]())
    for _ in range(2 + 5):
        b.restore(); b.planned()
    print(json.dumps({"profiled_case": args.profile, "meshes": b.K, "n_nodes": int(b.results()["n_nodes"].sum())}))
    sys.exit(0)

rows = [run_case(c, CASES[c]()) for c in args.cases.split(",") if c]
result = {"steps": args.steps, "warmup": args.warmup, "cases": rows}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
if args.md:
    lines = ["| case | meshes | triangles | (a) loop of single builds ms (median, min-max) | (b) planned call ms | (c) graph replay ms | (d) one mesh of all triangles ms | (a) / (b) | (b) / (d) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| {case} | {meshes} | {triangles} | {a[median]} ({a[min]}-{a[max]}) | {b[median]} ({b[min]}-{b[max]}) | {c[median]} ({c[min]}-{c[max]}) | {d[median]} ({d[min]}-{d[max]}) | {loop_over_planned} | {planned_over_floor} |".format(
            a=r["loop_ms"], b=r["planned_ms"], c=r["graph_ms"], d=r["floor_ms"], **r))
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write("\n".join(lines) + "\n")
