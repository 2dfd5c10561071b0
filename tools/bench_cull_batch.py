"""vd_cull_batch_dev (one command per mesh + the survivors' ids grouped by mesh) against vd_cull_compact_dev (one 20-byte
command per survivor) on the same scenes, in ONE process: n_mesh in {16, 256, 4096}, mesh ids random and sorted in runs.
Inputs resident; consecutive steps alternate two instance buffers (the second is the first after one compute_update step:
every transform differs, mesh ids equal), as bench.py's headline steps do; one HIP event pair per step on the context's
stream, median over the steps after a warm-up.  The two stages of the batched step come from vd_last_gpu_ms_stage in a
loop of their own (event pairs inside a call cost a few us of idle).
--compact-lib PATH: the yardstick vd_cull_compact_dev is ALSO run from another build of the library (the parent commit's
libvoidin_hip.so), loaded beside this one with a context of its own.
Usage (on a GPU box): python tools/bench_cull_batch.py [--n 10000000] [--meshes 16,256,4096] [--steps 30] [--warmup 5]
                                                       [--run 4096] [--compact-lib parent/libvoidin_hip.so] [--out result.json]"""
import argparse
import ctypes as C
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
ap.add_argument("--meshes", default="16,256,4096")
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--run", type=int, default=4096, help="length of a run of equal mesh ids in the run-sorted scenes")
ap.add_argument("--compact-lib", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
assert args.steps >= 20

ctx = Context(0)
n = args.n
cam = synth.camera_uniform()
cam_c = np.ascontiguousarray(cam, dtype=abi.CAMERA)
inst = synth.instances(n, seed=synth.SEED_BASE + 3, with_inverse=False, scale_range=(0.25, 4.0))
d_a = ctx.upload(inst)
del inst
d_b = d_a.clone()
d_idx = torch.arange(n, dtype=torch.int32, device="cuda")
ctx.compute_update_dev(d_idx, n, d_b, n, 1.0, 0.016)
torch.cuda.synchronize()
mesh_col = [t.view(torch.int32).view(n, 36)[:, 32] for t in (d_a, d_b)]       # VdInstance.mesh: byte 128 of 144

parent = None
if args.compact_lib:                                                           # the same entry point from another build
    plib = C.CDLL(os.path.abspath(args.compact_lib))
    plib.vd_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    plib.vd_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    plib.vd_cull_compact_dev.argtypes = abi.PROTOTYPES["vd_cull_compact_dev"][1]
    ph = C.c_void_p()
    assert plib.vd_ctx_create(0, C.byref(ph)) == 0
    assert plib.vd_ctx_set_stream(ph, torch.cuda.current_stream().cuda_stream) == 0
    parent = (plib, ph)

d_list = ctx.empty(n * 20)
d_ids = ctx.empty(n * 4)
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


result = {"n": n, "steps": args.steps, "warmup": args.warmup, "run": args.run, "cases": []}
for n_mesh in [int(m) for m in args.meshes.split(",")]:
    meshes = synth.mesh_infos(n_mesh)
    d_m = ctx.upload(meshes)
    d_cmds = ctx.empty(n_mesh * 20)
    for order in ("random", "runs"):
        if order == "random":
            g = torch.Generator(device="cuda")
            g.manual_seed(1234 + n_mesh)
            ids = torch.randint(0, n_mesh, (n,), dtype=torch.int32, device="cuda", generator=g)
        else:
            ids = ((d_idx // args.run) % n_mesh).to(torch.int32)
        for col in mesh_col:
            col.copy_(ids)
        torch.cuda.synchronize()

        def batched():
            ctx.cull_batch_dev(cam, d_m, n_mesh, src(), n, d_cmds, d_ids, d_cnt)

        def compacted():
            ctx.cull_compact_dev(cam, d_m, n_mesh, src(), n, d_list, d_cnt[4:], False)

        def compacted_parent():
            plib, ph = parent
            assert plib.vd_cull_compact_dev(ph, cam_c.ctypes.data, d_m.data_ptr(), n_mesh, src().data_ptr(), n, d_list.data_ptr(),
                                            d_cnt[4:].data_ptr(), 0) == 0

        row = {"n_mesh": n_mesh, "ids": order}
        row["batch_ms"] = per_step_ms(batched)
        row["compact_ms"] = per_step_ms(compacted)
        if parent:
            row["compact_parent_build_ms"] = per_step_ms(compacted_parent)
        row["batch_ms_again"] = per_step_ms(batched)                            # order effects: the first figure once more
        ctx.cull_batch_dev(cam, d_m, n_mesh, d_a, n, d_cmds, d_ids, d_cnt)       # same buffer for both: the counts agree
        ctx.cull_compact_dev(cam, d_m, n_mesh, d_a, n, d_list, d_cnt[4:], False)
        survivors = int(d_cnt[0].item())
        assert survivors == int(d_cnt[4].item())
        ctx.set_timing(True)
        s0, s1, c0, c1 = [], [], [], []
        for _ in range(args.steps):
            batched()
            s0.append(ctx.last_gpu_ms_stage(0)); s1.append(ctx.last_gpu_ms_stage(1))
            compacted()
            c0.append(ctx.last_gpu_ms_stage(0)); c1.append(ctx.last_gpu_ms_stage(1))
        ctx.set_timing(False)
        row.update({"survivors": survivors,
                    "batch_pass1_ms": round(float(np.median(s0)), 4), "batch_grouping_ms": round(float(np.median(s1)), 4),
                    "compact_pass1_ms": round(float(np.median(c0)), 4), "compact_expansion_ms": round(float(np.median(c1)), 4),
                    "batch_bytes_written": n_mesh * 20 + survivors * 4 + 4, "compact_bytes_written": survivors * 20 + 4})
        yard = row.get("compact_parent_build_ms", row["compact_ms"])["median"]
        row["batch_over_compact"] = round(row["batch_ms"]["median"] / yard, 3)
        result["cases"].append(row)
        print(json.dumps(row), flush=True)

print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
