"""The wide walk and the LBVH top level, measured in one process (results: profiles/trace_wide.md).

  (a) build time: vd_tlas_build_lbvh[_wide]_dev at 32 768 (narrow and wide), 65 536 and 1 Mi (wide) instances, with the exact
      builds at 32 768 (narrow) and 65 536 (wide) from the same run as the yardstick;
  (b) cost of the wide encoding: bench.py's stress scene (2 000 instances of a 131 k-triangle knot, EXACT topology) under
      vd_trace_dev and under vd_trace_wide_dev over the same nodes rewritten as wide ones - closest hit and any hit; the narrow
      call is measured twice per round (before and after the wide one): the difference of those two is the spread; the per-call
      records through a 64-ray call (records + the longest of 64 rays);
  (c) first numbers at size: trace rate over the LBVH top level at 65 536 and 1 Mi instances of the bench cloud's placement
      (synth.instances defaults), and the per-call record cost there: a call of 64 rays that look away from the scene - they miss
      the root's box, so the call is its records and its launches.

Prepared wide scenes and the accel refit (results: profiles/trace_wide_prepared.md):

  (p) the scenes of (c) under (a) the plain vd_trace_wide_dev over the LBVH of the reference's boxes - the baseline, twice per
      repetition: the difference of the two is the spread -, (b) the prepared accel with VD_OPT_TRACE_TIGHT_TLAS off and (c) the
      prepared accel with its private tight top level; closest hit and any hit.  --big-reps: repetitions at --big (a baseline call
      there takes seconds);
  (d) vd_trace_accel_update_dev (rebuild) against vd_trace_accel_refit_dev on those accels, and at 32 768 instances on narrow accels
      of both builders;
  (e) the stress scene of (b): narrow tight (both builders) against wide tight over the same instances.

Device events (torch, on the context's stream), warm-up, medians of --reps (>= 30) with the compared forms alternating inside each
repetition.  One JSON line per measurement on stdout; --out FILE keeps them."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from voidin_amd import abi, synth  # noqa: E402
from voidin_amd.runtime import Context  # noqa: E402


def widen(tl):
    w = np.zeros(len(tl), dtype=abi.TLAS_NODE_WIDE)
    w["min"], w["max"], w["instance_idx"] = tl["min"], tl["max"], tl["instance_idx"]
    w["left"], w["right"] = tl["left_right"] & np.uint32(0xffff), tl["left_right"] >> np.uint32(16)
    return w


def alternate(forms, reps, warmup):
    """forms: {name: callable}; every repetition runs each form once, in order, each between two device events.
    Returns {name: (median ms, min ms, max ms)}."""
    ms = {k: [] for k in forms}
    for r in range(warmup + reps):
        for name, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            if r >= warmup:
                ms[name].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--exact-reps", type=int, default=5, help="repetitions of the exact builds (hundreds of ms each)")
    ap.add_argument("--big", type=int, default=1 << 20, help="the largest instance count of (a) and (c)")
    ap.add_argument("--big-reps", type=int, default=30, help="repetitions of (p) at --big instances")
    ap.add_argument("--legs", default="abc", help="which of (a), (b), (c), (p), (d), (e) to run; r = of (c) only the per-call records")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    # ---- (a) build time ----------------------------------------------------------------------------------------------
    meshes = synth.mesh_infos()
    d_m = ctx.upload(meshes)
    for n in sorted({32768, 65536, args.big}) if "a" in args.legs else ():
        inst = synth.instances(n, seed=synth.SEED_BASE + 7, extent=2000.0 if n > 65536 else 400.0)
        d_i = ctx.upload(inst)
        d_w = ctx.empty((2 * n + 1) * 48)
        forms = {"lbvh_wide": lambda: ctx.tlas_build_lbvh_dev(d_i, n, d_m, len(meshes), d_w, wide=True)}
        if n <= abi.TLAS_MAX_INSTANCES:
            d_n = ctx.empty((2 * n + 1) * 32)
            forms["lbvh_narrow"] = lambda: ctx.tlas_build_lbvh_dev(d_i, n, d_m, len(meshes), d_n)
        forms["refit_wide"] = lambda: ctx.tlas_refit_dev(d_i, n, d_m, len(meshes), d_w, wide=True)        # of the LBVH tree just built
        res = alternate(forms, args.reps, args.warmup)
        for k, (med, lo, hi) in res.items():
            emit(leg="a", n_instances=n, form=k, median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), reps=args.reps)
        if n <= 65536:
            d_e = ctx.empty((2 * n + 1) * 48)
            wide_exact = n > abi.TLAS_MAX_INSTANCES
            res = alternate({"exact_wide" if wide_exact else "exact_narrow": lambda: ctx.tlas_build_dev(d_i, n, d_m, len(meshes), d_e, wide=wide_exact)},
                            args.exact_reps, 1)
            for k, (med, lo, hi) in res.items():
                emit(leg="a", n_instances=n, form=k, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), reps=args.exact_reps)
        del d_i, d_w

    # ---- (b) the wide encoding on the stress scene -------------------------------------------------------------------------
    if "b" in args.legs:
        leg_b(ctx, args, emit)
    if "c" in args.legs or "r" in args.legs:
        leg_c(ctx, args, emit, records_only="c" not in args.legs)
    if "p" in args.legs or "d" in args.legs:
        leg_p(ctx, args, emit)
    if "d" in args.legs:
        leg_d_narrow(ctx, args, emit)
    if "e" in args.legs:
        leg_e(ctx, args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    ctx.close()


def leg_b(ctx, args, emit):
    tv, ti = synth.knot_mesh(512, 128)
    nodes_b, idx_b = ctx.bvh_build(tv, ti)
    infos = np.zeros(1, dtype=abi.MESH_INFO)
    infos[0]["min"], infos[0]["max"] = synth.mesh_bounds(tv)
    infos[0]["index_count"] = len(idx_b)
    inst_t = synth.instances(2000, n_mesh=1, seed=synth.SEED_BASE + 8, extent=120.0, scale_range=(0.5, 2.0))
    tl = ctx.tlas_build(inst_t, infos)
    rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 90), pitch_deg=0), 1024, 1024)
    n_rays = len(rays)
    ds_n = ctx.device_scene((tl, inst_t, infos, nodes_b, tv, idx_b))
    ds_w = ctx.device_scene((widen(tl), inst_t, infos, nodes_b, tv, idx_b))
    d_rays = ctx.upload(rays)
    d_h1, d_h2 = ctx.empty(n_rays * 16), ctx.empty(n_rays * 16)
    d_a1 = torch.zeros(n_rays, dtype=torch.int32, device="cuda")
    d_a2 = torch.zeros(n_rays, dtype=torch.int32, device="cuda")
    ctx.set_option("trace.fan", 3)                     # pinned, as bench.py does: the default's skip rule depends on the calls before
    res = alternate({"narrow_closest": lambda: ctx.trace_dev(ds_n, d_rays, n_rays, d_h1),
                     "wide_closest": lambda: ctx.trace_wide_dev(ds_w, d_rays, n_rays, d_h2),
                     "narrow_closest_again": lambda: ctx.trace_dev(ds_n, d_rays, n_rays, d_h1),
                     "narrow_any": lambda: ctx.trace_any_dev(ds_n, d_rays, n_rays, d_a1),
                     "wide_any": lambda: ctx.trace_any_wide_dev(ds_w, d_rays, n_rays, d_a2),
                     "narrow_any_again": lambda: ctx.trace_any_dev(ds_n, d_rays, n_rays, d_a1),
                     "narrow_64_rays": lambda: ctx.trace_dev(ds_n, d_rays, 64, d_h1),
                     "wide_64_rays": lambda: ctx.trace_wide_dev(ds_w, d_rays, 64, d_h2)}, args.reps, args.warmup)
    # (the 64-ray calls come last in a repetition and overwrite the first 64 records: the comparison below re-runs the full calls)
    ctx.trace_dev(ds_n, d_rays, n_rays, d_h1); ctx.trace_wide_dev(ds_w, d_rays, n_rays, d_h2)
    torch.cuda.synchronize()
    same = d_h1.cpu().numpy()[: n_rays * 16].tobytes() == d_h2.cpu().numpy()[: n_rays * 16].tobytes() and bool((d_a1 == d_a2).all().item())
    for k, (med, lo, hi) in res.items():
        emit(leg="b", scene="stress: 2000 instances x 131k-triangle knot, exact topology", form=k, n_rays=64 if "64" in k else n_rays,
             median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
             Mrays_per_s=None if "64" in k else round(n_rays / med / 1e3, 1), reps=args.reps, same_bytes_narrow_vs_wide=same)
    ctx.set_option("trace.fan", None)


def leg_c(ctx, args, emit, records_only=False):
    n_rays = 1 << 20
    d_h1, d_h2 = ctx.empty(n_rays * 16), ctx.empty(n_rays * 16)
    d_a1 = torch.zeros(n_rays, dtype=torch.int32, device="cuda")
    ctx.set_option("trace.fan", 3)
    # ---- (c) first numbers at size -----------------------------------------------------------------------------------------
    sv, si = synth.knot_mesh(64, 16)
    nodes_s, idx_s = ctx.bvh_build(sv, si)
    infos_s = np.zeros(1, dtype=abi.MESH_INFO)
    infos_s[0]["min"], infos_s[0]["max"] = synth.mesh_bounds(sv)
    infos_s[0]["index_count"] = len(idx_s)
    d_ms = ctx.upload(infos_s)
    for n in sorted({65536, args.big}):
        inst = synth.instances(n, n_mesh=1, seed=synth.SEED_BASE + 9)          # the bench cloud's placement: the defaults
        d_i = ctx.upload(inst)
        d_w = ctx.empty((2 * n + 1) * 48)
        ctx.tlas_build_lbvh_dev(d_i, n, d_ms, 1, d_w, wide=True)
        torch.cuda.synchronize()
        wide = d_w.cpu().numpy()[: (2 * n + 1) * 48].view(abi.TLAS_NODE_WIDE)
        ds = ctx.device_scene((wide, inst, infos_s, nodes_s, sv, idx_s))
        rays_c = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 1500), pitch_deg=0), 1024, 1024)
        d_rc = ctx.upload(rays_c)
        away = np.zeros(64, dtype=abi.RAY)                                     # from far outside, looking away: the root's box is missed
        away["eye"], away["dir"] = (0.0, 0.0, 1.0e6), (0.0, 0.0, 1.0)
        d_away = ctx.upload(away)
        forms = {"closest": lambda: ctx.trace_wide_dev(ds, d_rc, len(rays_c), d_h1),
                 "any": lambda: ctx.trace_any_wide_dev(ds, d_rc, len(rays_c), d_a1),
                 "64_rays": lambda: ctx.trace_wide_dev(ds, d_rc, 64, d_h2),
                 "64_rays_that_miss_the_root": lambda: ctx.trace_wide_dev(ds, d_away, 64, d_h2)}
        if records_only:
            forms = {"64_rays_that_miss_the_root": forms["64_rays_that_miss_the_root"]}
        res = alternate(forms, args.reps, args.warmup)
        hit_share = None
        if not records_only:
            ctx.trace_wide_dev(ds, d_rc, len(rays_c), d_h1)
            torch.cuda.synchronize()
            hit_share = round(float(d_h1.cpu().numpy()[: len(rays_c) * 16].view(abi.HIT)["hit"].mean()), 3)
        for k, (med, lo, hi) in res.items():
            emit(leg="c", n_instances=n, n_tlas_nodes=2 * n + 1, form=k, n_rays=64 if "64" in k else len(rays_c), median_ms=round(med, 4),
                 min_ms=round(lo, 4), max_ms=round(hi, 4), Mrays_per_s=None if "64" in k else round(len(rays_c) / med / 1e3, 1),
                 hit_share=hit_share, reps=args.reps)
        del ds, d_i, d_w
    ctx.set_option("trace.fan", None)


def prepare(ctx, ds, tight):
    ctx.set_option("trace.tight_tlas", tight)
    acc = ctx.trace_prepare(ds)
    ctx.set_option("trace.tight_tlas", None)
    return acc


def leg_p(ctx, args, emit):
    """(p) and the wide half of (d): the scenes of leg_c."""
    n_rays = 1 << 20
    d_h = [ctx.empty(n_rays * 16) for _ in range(3)]
    d_a = [torch.zeros(n_rays, dtype=torch.int32, device="cuda") for _ in range(3)]
    ctx.set_option("trace.fan", 3)
    sv, si = synth.knot_mesh(64, 16)
    nodes_s, idx_s = ctx.bvh_build(sv, si)
    infos_s = np.zeros(1, dtype=abi.MESH_INFO)
    infos_s[0]["min"], infos_s[0]["max"] = synth.mesh_bounds(sv)
    infos_s[0]["index_count"] = len(idx_s)
    d_ms = ctx.upload(infos_s)
    rays_c = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 1500), pitch_deg=0), 1024, 1024)
    d_rc = ctx.upload(rays_c)
    for n in sorted({65536, args.big}):
        inst = synth.instances(n, n_mesh=1, seed=synth.SEED_BASE + 9)          # the bench cloud's placement: the defaults
        d_i = ctx.upload(inst)
        d_w = ctx.empty((2 * n + 1) * 48)
        ctx.tlas_build_lbvh_dev(d_i, n, d_ms, 1, d_w, wide=True)
        torch.cuda.synchronize()
        wide = d_w.cpu().numpy()[: (2 * n + 1) * 48].view(abi.TLAS_NODE_WIDE)
        ds = ctx.device_scene((wide, inst, infos_s, nodes_s, sv, idx_s))
        exact, tight = prepare(ctx, ds, 0), prepare(ctx, ds, 2)
        info = tight.info()
        assert info["tight_tlas"] == 2 and info["n_tlas_nodes"] == 2 * n, info
        reps = args.reps if n <= 65536 else args.big_reps
        if "p" in args.legs:
            res = alternate({"a_plain_closest": lambda: ctx.trace_wide_dev(ds, d_rc, n_rays, d_h[0]),
                             "b_prepared_exact_closest": lambda: ctx.trace_prepared_dev(exact, d_rc, n_rays, d_h[1]),
                             "c_prepared_tight_closest": lambda: ctx.trace_prepared_dev(tight, d_rc, n_rays, d_h[2]),
                             "a_plain_closest_again": lambda: ctx.trace_wide_dev(ds, d_rc, n_rays, d_h[0]),
                             "a_plain_any": lambda: ctx.trace_any_wide_dev(ds, d_rc, n_rays, d_a[0]),
                             "b_prepared_exact_any": lambda: ctx.trace_any_prepared_dev(exact, d_rc, n_rays, d_a[1]),
                             "c_prepared_tight_any": lambda: ctx.trace_any_prepared_dev(tight, d_rc, n_rays, d_a[2]),
                             "a_plain_any_again": lambda: ctx.trace_any_wide_dev(ds, d_rc, n_rays, d_a[0])}, reps, min(args.warmup, reps))
            torch.cuda.synchronize()
            h = [x.cpu().numpy()[: n_rays * 16].view(abi.HIT) for x in d_h]
            hit = h[0]["hit"] == 1
            check = {"b_same_bytes_as_a": h[0].tobytes() == h[1].tobytes() and bool((d_a[0] == d_a[1]).all().item()),
                     "c_same_hit_flags": bool((h[0]["hit"] == h[2]["hit"]).all()) and bool((d_a[0] == d_a[2]).all().item()),
                     "c_dist_not_bit_equal": int((h[0]["dist"][hit].view(np.uint32) != h[2]["dist"][hit].view(np.uint32)).sum()),
                     "hit_share": round(float(hit.mean()), 3)}
            for k, (med, lo, hi) in res.items():
                emit(leg="p", n_instances=n, form=k, n_rays=n_rays, median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                     Mrays_per_s=round(n_rays / med / 1e3, 2), reps=reps, **check)
        if "d" in args.legs:
            res = alternate({"update_rebuild": tight.update, "refit": tight.refit, "refit_again": tight.refit}, args.reps, args.warmup)
            for k, (med, lo, hi) in res.items():
                emit(leg="d", accel="wide lbvh", n_instances=n, form=k, median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), reps=args.reps)
        exact.close(); tight.close()
        del ds, d_i, d_w
    ctx.set_option("trace.fan", None)


def leg_d_narrow(ctx, args, emit):
    """(d) at 32 768 instances (32 767 for the LBVH: 2n must fit 16 bits) on narrow accels of both builders."""
    sv, si = synth.knot_mesh(64, 16)
    nodes_s, idx_s = ctx.bvh_build(sv, si)
    infos_s = np.zeros(1, dtype=abi.MESH_INFO)
    infos_s[0]["min"], infos_s[0]["max"] = synth.mesh_bounds(sv)
    infos_s[0]["index_count"] = len(idx_s)
    for mode, n in ((1, 32768), (2, 32767)):
        inst = synth.instances(n, n_mesh=1, seed=synth.SEED_BASE + 9)
        tl = ctx.tlas_build_lbvh(inst, infos_s)                                 # the scene's own top level is not what is measured
        ds = ctx.device_scene((tl, inst, infos_s, nodes_s, sv, idx_s))
        acc = prepare(ctx, ds, mode)
        assert acc.info()["tight_tlas"] == mode, acc.info()
        reps = args.exact_reps if mode == 1 else args.reps
        res = alternate({"update_rebuild": acc.update, "refit": acc.refit, "refit_again": acc.refit}, reps, 1 if mode == 1 else args.warmup)
        for k, (med, lo, hi) in res.items():
            emit(leg="d", accel="narrow agglomerative" if mode == 1 else "narrow lbvh", n_instances=n, form=k, median_ms=round(med, 4),
                 min_ms=round(lo, 4), max_ms=round(hi, 4), reps=reps)
        acc.close()


def leg_e(ctx, args, emit):
    """(e) the stress scene: narrow tight (agglomerative, LBVH) against wide tight (LBVH) over the same instances."""
    tv, ti = synth.knot_mesh(512, 128)
    nodes_b, idx_b = ctx.bvh_build(tv, ti)
    infos = np.zeros(1, dtype=abi.MESH_INFO)
    infos[0]["min"], infos[0]["max"] = synth.mesh_bounds(tv)
    infos[0]["index_count"] = len(idx_b)
    inst_t = synth.instances(2000, n_mesh=1, seed=synth.SEED_BASE + 8, extent=120.0, scale_range=(0.5, 2.0))
    tl = ctx.tlas_build(inst_t, infos)
    rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 90), pitch_deg=0), 1024, 1024)
    n_rays = len(rays)
    d_rays = ctx.upload(rays)
    ds_n = ctx.device_scene((tl, inst_t, infos, nodes_b, tv, idx_b))
    ds_w = ctx.device_scene((widen(tl), inst_t, infos, nodes_b, tv, idx_b))
    accs = {"narrow_agglomerative": prepare(ctx, ds_n, 1), "narrow_lbvh": prepare(ctx, ds_n, 2), "wide_lbvh": prepare(ctx, ds_w, 2),
            "narrow_exact": prepare(ctx, ds_n, 0)}
    d_h = {k: ctx.empty(n_rays * 16) for k in accs}
    d_a = {k: torch.zeros(n_rays, dtype=torch.int32, device="cuda") for k in accs}
    ctx.set_option("trace.fan", 3)
    forms = {}
    for k, acc in accs.items():
        forms[k + "_closest"] = (lambda acc=acc, k=k: ctx.trace_prepared_dev(acc, d_rays, n_rays, d_h[k]))
    forms["narrow_lbvh_closest_again"] = lambda: ctx.trace_prepared_dev(accs["narrow_lbvh"], d_rays, n_rays, d_h["narrow_lbvh"])
    for k, acc in accs.items():
        forms[k + "_any"] = (lambda acc=acc, k=k: ctx.trace_any_prepared_dev(acc, d_rays, n_rays, d_a[k]))
    forms["narrow_lbvh_any_again"] = lambda: ctx.trace_any_prepared_dev(accs["narrow_lbvh"], d_rays, n_rays, d_a["narrow_lbvh"])
    res = alternate(forms, args.reps, args.warmup)
    torch.cuda.synchronize()
    same = d_h["narrow_lbvh"].cpu().numpy()[: n_rays * 16].tobytes() == d_h["wide_lbvh"].cpu().numpy()[: n_rays * 16].tobytes()
    for k, (med, lo, hi) in res.items():
        emit(leg="e", scene="stress: 2000 instances x 131k-triangle knot", form=k, n_rays=n_rays, median_ms=round(med, 4), min_ms=round(lo, 4),
             max_ms=round(hi, 4), Mrays_per_s=round(n_rays / med / 1e3, 1), reps=args.reps, same_bytes_narrow_lbvh_vs_wide_lbvh=same)
    for acc in accs.values():
        acc.close()
    ctx.set_option("trace.fan", None)


if __name__ == "__main__":
    main()
