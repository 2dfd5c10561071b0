"""vd_tlas_build_lbvh_wide_dev of two builds of the library, alternating in one run: the time per build at 65 536 and 1 Mi instances
and a digest of the node bytes (a change to the shared LBVH stages - codes, sort, tree - must leave every byte as it was).
The legs are libraries made by tools/build_ab.sh (AB_SRC=<csrc of the other checkout> for an earlier commit); each measurement
runs in a child process of its own with VOIDIN_HIP_LIB set, the legs taking turns round by round.
Usage (on a GPU box): python tools/ab_tlas_lbvh.py --libs build/ab/parent/libvoidin_hip.so,build/ab/head/libvoidin_hip.so [--rounds 3]
                                                   [--sizes 65536,1048576] [--reps 20] [--out result.json]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--libs", default="")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--sizes", default="65536,1048576")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default="")
ap.add_argument("--child", action="store_true")
args = ap.parse_args()
sizes = [int(x) for x in args.sizes.split(",")]

if args.child:
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from voidin_amd import abi, synth
    from voidin_amd.runtime import Context
    abi.load(strict=False)                                # an earlier commit's library lacks the newer entry points: bind what it has
    ctx = Context(0)
    meshes = synth.mesh_infos()
    d_m = ctx.upload(meshes)
    out = {}
    for n in sizes:
        d_i = ctx.upload(synth.instances(n, seed=synth.SEED_BASE + 9, extent=2000.0, with_inverse=False))
        d_n = ctx.empty((2 * n + 1) * 48)
        for _ in range(3):
            ctx.tlas_build_lbvh_dev(d_i, n, d_m, len(meshes), d_n, wide=True)
        torch.cuda.synchronize()
        t = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); ctx.tlas_build_lbvh_dev(d_i, n, d_m, len(meshes), d_n, wide=True); e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        out[str(n)] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(min(t)), 4), "max_ms": round(float(max(t)), 4),
                       "sha1": hashlib.sha1(d_n.cpu().numpy()[: (2 * n + 1) * 48].tobytes()).hexdigest()}
    print("AB " + json.dumps(out))
    sys.exit(0)

libs = [os.path.abspath(p) for p in args.libs.split(",") if p]
assert len(libs) == 2, "--libs A,B"
rows = []
for r in range(args.rounds):
    for leg, lib in enumerate(libs):
        env = dict(os.environ, VOIDIN_HIP_LIB=lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--sizes", args.sizes, "--reps", str(args.reps)],
                           env=env, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-2000:])
            sys.exit(1)                                   # nothing more is started after a failed leg
        line = [x for x in p.stdout.splitlines() if x.startswith("AB ")][-1]
        rows.append({"round": r, "leg": "AB"[leg], "lib": os.path.relpath(lib, ROOT), "sizes": json.loads(line[3:])})
        print(json.dumps(rows[-1]), flush=True)
same = {str(n): len({row["sizes"][str(n)]["sha1"] for row in rows}) == 1 for n in sizes}
result = {"rows": rows, "same_bytes_in_every_leg": same}
print(json.dumps({"same_bytes_in_every_leg": same}))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
