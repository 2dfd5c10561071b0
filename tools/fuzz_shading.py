"""Random cases through the shading chain against its float32 twins, byte for byte (two NaNs are equal): vd_lighting_dev fed bit words
of every count from 0 to 32 a pixel (part "lighting"); vd_gbuffer_points_dev and vd_shadow_gbuffer*_dev in all four forms of the scene
over random G-buffers on random scenes, chunked and not, VD_OPT_TRACE_RAY_RANGE off and on (part "shadow"); vd_gbuffer_trace*_dev into
vd_shade_gbuffer*_dev (part "chain").  tests/fuzz_shading_cases.py makes the cases and what is expected of them; a case is a function of
(seed, part, number), so `--only K` replays case K of a campaign alone.
    python tools/fuzz_shading.py [--cases 500,100,50] [--seed 1] [--parts lighting,shadow,chain] [--only K]
`run(cases, seed, ctx)` is what tests/test_gpu_fuzz_shading.py calls with a fixed seed.  Every output is written over a prefill between
canary words or guard regions, at pitches larger than the rows where the case says so; a canary, a guard or row padding that changed
is a mismatch like any other."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import fuzz_shading_cases as Z  # noqa: E402
import gbuffer_trace_cases as T  # noqa: E402
from oracle import ref  # noqa: E402
from voidin_amd import abi  # noqa: E402
from voidin_amd.runtime import Context  # noqa: E402

PARTS = Z.PARTS


def _checks():
    """The device-side helpers of the families' own tests (imported late: they import torch-using modules)."""
    from test_gpu_gbuffer_trace import DeviceGeometry, Target as ImageTarget
    from test_gpu_lighting import Target, same as same_colour
    from test_gpu_shadow_gbuffer import Case, Images, check_points, same as same_words
    from test_gpu_trace_range import Rig
    return dict(DeviceGeometry=DeviceGeometry, ImageTarget=ImageTarget, Target=Target, same_colour=same_colour, Case=Case, Images=Images,
                check_points=check_points, same_words=same_words, Rig=Rig)


def lighting_case(ctx, c, H, d_table):
    """-> the descriptions of what differs (none: [])."""
    im = H["Images"](ctx, c.gb, pitches=c.pitches)
    tg = H["Target"](c.w, c.h, pitch=c.colour_pitch)
    d_lts, d_inr, d_occ = (ctx.upload(c.lts), ctx.upload(c.inr), ctx.upload(c.occ)) if c.n_lights else (None, None, None)
    ctx.lighting_dev(c.cam, im.c, d_lts, c.n_lights, d_occ, d_inr, d_table, tg.t)
    H["same_colour"](tg.read(), c.want(), "colour")
    return []


def shadow_case(ctx, c, H, d_table):
    bad = []
    w = c.words()
    case = H["Case"](ctx, c.sc.scene, c.gb, c.lts, pitches=c.pitches)
    try:
        try:
            H["check_points"](ctx, case.im, "points")
        except AssertionError as e:
            bad.append(f"vd_gbuffer_points_dev: {e}")
        ctx.set_option("trace.ray_range", c.ray_range)
        for form in Z.SHADOW_FORMS:
            try:
                occ, inr, info = case.run(form, case.im, c.n_lights, max_chunk_rays=c.max_chunk_rays)
                H["same_words"](inr, w.inr, "in range")
                H["same_words"](occ, w.occ[c.ray_range], "occluded")
                got = {k: info[k] for k in w.info}
                assert got == w.info, ("info", got, w.info)
            except AssertionError as e:
                bad.append(f"form {form}: {e}")
    finally:
        ctx.set_option("trace.ray_range", None)
        case.close()
    return bad


def chain_case(ctx, c, H, d_table):
    bad = []
    w = c.words()
    rig, dev = H["Rig"](ctx, c.scene), H["DeviceGeometry"](ctx, c.full_geo)
    d_lts = ctx.upload(c.lts) if c.n_lights else None
    normals, uvs = c.geo.normals is not None, c.geo.tex_coords is not None
    p = dev.full
    geometry = abi.GBufferGeometry(p.instances, p.n_instances, p.meshes, p.n_meshes, p.vertices, p.n_vertices, p.indices, p.n_indices,
                                   p.normals if normals else None, p.tex_coords if uvs else None)
    try:
        ctx.set_option("trace.ray_range", c.ray_range)
        for form in Z.CHAIN_FORMS:
            try:
                t = H["ImageTarget"](c.w, c.h)
                tg = H["Target"](c.w, c.h, pitch=c.colour_pitch)
                if form == "scene":
                    ctx.gbuffer_trace_dev(rig.ds, c.cam, t.c, dev.d_normals if normals else None, dev.d_tex_coords if uvs else None)
                    info = ctx.shade_gbuffer_dev(rig.ds, c.cam, t.gbuffer(), d_lts, c.n_lights, d_table, tg.t, c.max_chunk_rays)
                else:
                    accel = {"prepared": rig.acc, "wide": rig.acc_wide}[form]
                    ctx.gbuffer_trace_prepared_dev(accel, geometry, c.cam, t.c)
                    info = ctx.shade_gbuffer_prepared_dev(accel, c.cam, t.gbuffer(), d_lts, c.n_lights, d_table, tg.t, c.max_chunk_rays)
                differs = T.same_image(t.read(), c.img)
                assert differs is None, ("image",) + differs
                H["same_colour"](tg.read(), c.colour(), "colour")
                got = {k: info[k] for k in w.info}
                assert got == w.info, ("info", got, w.info)
            except AssertionError as e:
                bad.append(f"form {form}: {e}")
    finally:
        ctx.set_option("trace.ray_range", None)
        rig.close()
    return bad


RUNNERS = {"lighting": lighting_case, "shadow": shadow_case, "chain": chain_case}


def run(cases, seed, ctx=None, log=print, parts=PARTS, only=None, campaign=False):
    """-> {part: mismatches}.  cases: a count for every part, or {part: count}; only: the case numbers to run (the others are not made:
    a case depends on its own number alone); campaign: the shadow part draws from light counts up to 1024.  A status other than VD_OK is
    not counted and passed by: it ends the run (VoidinError), the options restored."""
    import lighting_cases as L
    ref.load()
    ctx = ctx or Context(0)
    H = _checks()
    d_table = ctx.upload(L.materials())
    bad = {}
    for part in parts:
        bad[part] = 0
        for k in range(cases[part] if isinstance(cases, dict) else cases):
            if only is not None and k not in only:
                continue
            c = Z.make(part, seed, k, ref, campaign)
            try:
                differs = RUNNERS[part](ctx, c, H, d_table)
            except AssertionError as e:
                differs = [str(e)]
            for line in differs:
                bad[part] += 1
                log(f"{c.describe()}: DIFFERS: {line}")
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="48,12,8", help="one count, or one per part in the order of --parts")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--only", type=int, action="append", help="run this case number alone (may be given more than once)")
    args = ap.parse_args()
    parts = tuple(args.parts.split(","))
    counts = [int(x) for x in args.cases.split(",")]
    counts = dict(zip(parts, counts * len(parts) if len(counts) == 1 else counts))
    bad = run(counts, args.seed, log=lambda m: print(m, flush=True), parts=parts, only=args.only, campaign=True)
    print("; ".join(f"{part}: {counts[part]} cases, {bad[part]} mismatches" for part in parts))
    sys.exit(1 if any(bad.values()) else 0)
