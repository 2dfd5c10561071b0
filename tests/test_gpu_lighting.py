"""vd_lighting_dev and vd_shade_gbuffer_dev / vd_shade_gbuffer_prepared_dev (include/voidin_lighting.h): the shadow shader's light loop
summed on the device.  The step is compared BYTE FOR BYTE with the float32 twin of tests/lighting_cases.py, fed the very bit words
the call is fed - the twin's in-range bits and a seeded random subset of them as occlusion, so no walk is needed - and the composed
calls with the two calls they are made of on the same context, and once with the twin fed the CPU's expectation of the pass.  Every
image is written at a pitch larger than its row, over a prefill, between canary words; all of that must survive a call."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_cases as G
import lighting_cases as L
import shadow_pass_cases as S
from test_gpu_shadow_gbuffer import FORMS, PAD, PITCHES, Case, Images, shapes
from voidin_amd import abi, synth
from voidin_amd.runtime import Context, VoidinError
from write_set import FILL, Fences

pytestmark = pytest.mark.gpu

LIGHTS = (0, 1, 31, 32, 33, 65)
MANY = dict(n=1024, seed=L.SEED + 1, box=S.BOX, radii=(2.0, 18.0))      # W = 32: about 5 % of the pairs of the 64 x 9 crop in range


class Target:
    """A colour image on the device over a prefill, its rows 48 bytes further apart than they are long, between PAD canary words."""

    def __init__(self, width, height, fill=FILL, pitch=None):
        import torch
        self.w, self.h, self.fill = width, height, fill
        self.pitch = 16 * width + 48 if pitch is None else pitch
        self.raw = torch.full((2 * PAD * 4 + self.pitch * height,), fill, dtype=torch.uint8, device="cuda")
        self.t = Context.color_target(self.raw[PAD * 4:], width, height, self.pitch)

    def read(self):
        """-> float32 [pixels][4], after the canaries and the row padding were found untouched."""
        import torch
        torch.cuda.synchronize()
        host = self.raw.cpu().numpy()
        assert (host[: PAD * 4] == self.fill).all() and (host[PAD * 4 + self.pitch * self.h:] == self.fill).all(), "a word outside the image"
        rows = host[PAD * 4: PAD * 4 + self.pitch * self.h].reshape(self.h, self.pitch)
        assert (rows[:, 16 * self.w:] == self.fill).all(), "row padding was written"
        return rows[:, : 16 * self.w].copy().view(np.float32).reshape(self.w * self.h, 4)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.raw == self.fill).all().item())


def same(got, want, what):
    if not G.same_floats(got, want):
        bad = np.flatnonzero(L.changed(got, want))
        raise AssertionError((what, f"{len(bad)} of {len(got)} pixels differ", bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()))


def step(ctx, im, d_lts, n_lights, inr, occ, d_table, fill=FILL):
    """One vd_lighting_dev call on fresh uploads of the words -> the image."""
    tg = Target(im.gb.width, im.gb.height, fill)
    d_inr, d_occ = (ctx.upload(np.ascontiguousarray(inr)), ctx.upload(np.ascontiguousarray(occ))) if n_lights else (None, None)
    ctx.lighting_dev(im.gb.cam, im.c, d_lts if n_lights else None, n_lights, d_occ, d_inr, d_table, tg.t)
    return tg.read()


@pytest.fixture(scope="module")
def table():
    return L.materials()


@pytest.fixture(scope="module")
def d_table(ctx, table):
    return ctx.upload(table)


@pytest.fixture(scope="module")
def seeded(ctx, oracle):
    scene, gb, _ = G.seeded_gbuffer(oracle)
    c = Case(ctx, scene, gb, S.lights())
    yield c
    c.close()


@pytest.fixture(scope="module")
def flipped(ctx, oracle, seeded):
    _, gb = L.flipped_gbuffer(oracle)
    return Images(ctx, gb)


# ---- 1. the step against the twin ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ("seeded", "flipped"))
def test_the_step_equals_the_twin_byte_for_byte(ctx, oracle, seeded, flipped, table, d_table, which):
    """Every crop of shapes() - 1 x 1, 63 / 64 / 65 wide, 17 x 31, 64 x 8, 64 x 9, 64 x 64, 65 x 3, one row of 511 / 512 / 513 / 576 pixels -
    times 0, 1, 31, 32, 33 and 65 lights: W = 0, 1, 2 and 3, the last word full, with one bit and with 31."""
    full = seeded.im if which == "seeded" else flipped
    lit = 0
    for name, im in shapes(ctx, full):
        reach = L.rule_words(im.gb, seeded.lts)
        for n_lights in LIGHTS:
            W = (n_lights + 31) // 32
            inr = reach[:, :W].copy()
            if n_lights & 31:
                inr[:, W - 1] &= np.uint32((1 << (n_lights & 31)) - 1)
            occ = L.subset_words(inr, L.SEED, stream=n_lights)
            got = step(ctx, im, seeded.d_lts, n_lights, inr, occ, d_table)
            want = L.shade(im.gb, seeded.lts[:n_lights], inr, occ, table)
            same(got, want, (which, name, n_lights))
            lit += int(inr.any())
    assert lit > 40                                           # most of the 60 lit cases had a bit to walk


def test_w32_and_the_sparse_walk(ctx, oracle, seeded, table, d_table):
    """1024 lights on the 64 x 9 crop (576 pixels: nine waves), between 2 % and 10 % of the receivers' pairs in range: the bit words come
    through LDS at their longest, most words of most waves are empty, and no wave sees all of its lights."""
    im = seeded.im.crop(64, 9)
    lts = S.lights(**MANY)
    reach = S.in_range(im.gb.points()[0], lts)
    share = reach.mean()
    assert 0.02 <= share <= 0.10, share
    inr = G.scatter(im.gb, S.pack(reach))
    assert inr.shape == (576, 32) and (inr == 0).mean() > 0.25
    occ = L.subset_words(inr, L.SEED, stream=7)
    d_lts = ctx.upload(lts)
    got = step(ctx, im, d_lts, 1024, inr, occ, d_table)
    same(got, L.shade(im.gb, lts, inr, occ, table), "1024 lights")
    # ... and 1000: the last word has 8 bits that are lights and 24 that are not, filled with ones
    inr2, occ2 = inr.copy(), occ.copy()
    inr2[:, 31] |= np.uint32(0xffffff00)
    occ2[:, 31] |= np.uint32(0xffffff00)
    same(step(ctx, im, d_lts, 1000, inr2, occ2, d_table), L.shade(im.gb, lts[:1000], inr, occ, table), "1000 lights")


def test_hand_made(ctx, oracle, table, d_table):
    """hand_gbuffer: depth 0, NaN, +inf and 1, the normal words on every edge of the decoder, materials 0, 1, 2, 3 and 255; the lights of
    shadow_pass_cases.hand_made - radius 0, NaN, +inf, negative, -0 - with colours, one of them infinite."""
    scene, gb, lts = G.hand_gbuffer(oracle)
    lts = lts.copy()
    lts["color"] = (0.25 + synth.uniform01(L.SEED, 5, 3 * len(lts)).reshape(-1, 3)).astype(np.float32)
    lts["color"][3] = (np.inf, 0.5, 0.25)                    # the light whose radius is point 1's distance
    im = Images(ctx, gb, pitches=(256, 256, 5))
    d_lts = ctx.upload(lts)
    mat = gb.material.reshape(-1)
    inr = L.rule_words(gb, lts)
    assert inr.shape == (12, 1) and (inr[G.receivers(mat)] != 0).all()
    recv = G.receivers(mat)
    pos = L.view(gb)[0]
    dark = np.flatnonzero(recv & np.isfinite(pos).all(axis=1) & (L.attenuation(S.dist(pos, lts["position"][3]), lts["radius"][3]) == 0))
    assert dark.size > 0
    # the bits of the rule: the light with the NaN radius reaches every receiver, so every receiver's sum is a NaN and leaves as 0;
    # without that light and the infinite one: finite sums; then the infinite one for EVERY pixel, within its reach or not - at atten 0
    # inf * 0 is a NaN and the pixel's red is 0, not the finite sum of the other lights
    for name, keep, force in (("rule", 0xffffffff, 0), ("finite", ~((1 << 6) | (1 << 3)) & 0xffffffff, 0), ("infinite", ~(1 << 6) & 0xffffffff, 1 << 3)):
        words = (inr & np.uint32(keep)) | np.uint32(force)
        occ = L.subset_words(words, L.SEED, stream=3)
        words[~recv] = 0xffffffff                            # materials 0 and 2: every bit SET, and none of them read
        occ[~recv] = 0xffffffff
        got = step(ctx, im, d_lts, len(lts), words, occ, d_table)
        same(got, L.shade(gb, lts, words, occ, table), ("hand-made", name))
        assert not np.isnan(got).any() and (got >= 0).all() and (got[:, 3] == 1).all()
        assert got[8].tolist() == [1, 0, 1, 1] and mat[8] == 0
        assert mat[9] == 2 and got[9, :3].tobytes() == (table[2]["albedo"] + table[2]["emissive"]).astype(np.float32).tobytes()
        if name == "rule":
            assert np.isfinite(got).all() and (got[recv, :3] == 0).all()
        if name == "finite":
            assert np.isfinite(got).all() and (got[dark, :3] > 0).all()
        if name == "infinite":
            assert (got[dark, 0] == 0).all() and (got[dark, 1:3] > 0).all() and np.isfinite(got[dark]).all(), (dark, got[dark])


def test_the_bits_decide(ctx, oracle, seeded, table, d_table):
    """One row of 64 pixels, 33 lights: the call is fed words the rule would not give, and equals the twin fed the same words."""
    im = seeded.im.crop(64, 1)
    gb, lts = im.gb, seeded.lts[:33]
    reach = L.rule_words(gb, lts)
    occ = L.subset_words(reach, L.SEED, stream=9)
    base = step(ctx, im, seeded.d_lts, 33, reach, occ, d_table)
    same(base, L.shade(gb, lts, reach, occ, table), "the rule's bits")
    # a. a light that contributes, its in-range bit cleared: skipped
    want = L.shade(gb, lts, reach, occ, table)
    p = l = None
    for q, k in ((q, k) for q in range(64) for k in range(33) if (reach[q, k >> 5] >> (k & 31)) & 1):
        without = reach.copy()
        without[q, k >> 5] &= ~np.uint32(1 << (k & 31))
        if L.changed(want, L.shade(gb, lts, without, occ, table))[q]:
            p, l = q, k
            break
    assert p is not None, "no light of the row contributes"
    cleared = reach.copy()
    cleared[p, l >> 5] &= ~np.uint32(1 << (l & 31))
    got = step(ctx, im, seeded.d_lts, 33, cleared, occ, d_table)
    same(got, L.shade(gb, lts, cleared, occ, table), "a bit cleared")
    assert L.changed(got, base).tolist() == [q == p for q in range(64)]
    # b. occluded without in range means nothing
    out = [(q, k) for q in range(64) for k in range(33) if not (reach[q, k >> 5] >> (k & 31)) & 1 and np.isfinite(L.view(gb)[0][q]).all()]
    assert len(out) > 100
    lone = occ.copy()
    for q, k in out[::7]:
        lone[q, k >> 5] |= np.uint32(1 << (k & 31))
    assert (lone & ~reach).any()
    same(step(ctx, im, seeded.d_lts, 33, reach, lone, d_table), base, "occluded bits without their in-range bits")
    # c. in range by decree, for lights out of reach: each adds +0 - the twin's bytes
    wide = reach.copy()
    for q, k in out[::5]:
        wide[q, k >> 5] |= np.uint32(1 << (k & 31))
    same(step(ctx, im, seeded.d_lts, 33, wide, occ, d_table), L.shade(gb, lts, wide, occ, table), "bits set for lights out of reach")
    # d. the bits at and above n_lights = 33 of word 1: ones, and no light is read for them
    tail_in, tail_oc = reach.copy(), occ.copy()
    tail_in[:, 1] |= np.uint32(0xfffffffe)
    tail_oc[:, 1] |= np.uint32(0xfffffffe)
    same(step(ctx, im, seeded.d_lts, 33, tail_in, tail_oc, d_table), base, "bits at and above n_lights")


# ---- 2. the write set ------------------------------------------------------------------------------------------------------------------

def test_write_set(ctx, oracle, seeded, table, d_table):
    """Two prefills give the same image, so every pixel's 16 bytes were written (Target.read holds the padding and the canaries); and with
    every buffer between the 64 KiB guards of tests/write_set.py the inputs come back unchanged and no guard is touched."""
    import torch
    im = seeded.im.crop(64, 17)
    gb, lts, n_lights, W = im.gb, seeded.lts, 65, 3
    inr = L.rule_words(gb, lts)
    occ = L.subset_words(inr, L.SEED, stream=11)
    want = L.shade(gb, lts, inr, occ, table)
    for fill in (0xEE, 0x11, 0xFF, 0x00):
        same(step(ctx, im, seeded.d_lts, n_lights, inr, occ, d_table, fill=fill), want, ("prefill", fill))
    f = Fences()
    imgs = [f.inp(name, data) for name, data in zip(("depth", "normal_uv", "material"), seeded.im.gb.rows(*PITCHES)[:3])]
    lights, mats = f.inp("lights", lts), f.inp("materials", table)
    d_in, d_oc = f.inp("in_range", inr), f.inp("occluded", occ)
    pitch = 16 * 64 + 256
    out = f.out("rgba", pitch * 17)
    c = Context.gbuffer(imgs[0].ptr, imgs[1].ptr, imgs[2].ptr, 64, 17, *PITCHES)
    ctx.lighting_dev(gb.cam, c, lights.ptr, n_lights, d_oc.ptr, d_in.ptr, mats.ptr, Context.color_target(out.ptr, 64, 17, pitch))
    torch.cuda.synchronize()
    f.check()
    rows = out.read().reshape(17, pitch)
    assert (rows[:, 1024:] == FILL).all(), "row padding was written"
    same(rows[:, :1024].copy().view(np.float32).reshape(-1, 4), want, "between the guards")


# ---- 3. enqueue-only ---------------------------------------------------------------------------------------------------------------------

def test_the_step_only_enqueues_on_the_contexts_stream(oracle, table):
    """tests/test_gpu_stream_order.py's method: warmed up on bits A; then on a side stream, behind its delay, the upload of bits B, and
    the call through the context of that stream.  The call returns while the stream is still busy; a clone taken on the stream in front
    of the upload holds the fill, the clone behind the call holds the twin's image of B."""
    import torch
    from test_gpu_stream_order import Side
    _, gb, _ = G.seeded_gbuffer(oracle)
    n_lights = 33
    lts = S.lights()[:n_lights]
    inr = L.rule_words(gb, lts)
    occA, occB = L.subset_words(inr, L.SEED, stream=1), L.subset_words(inr, L.SEED, stream=2)
    wants = {k: L.shade(gb, lts, inr, o, table) for k, o in (("A", occA), ("B", occB))}
    assert L.changed(wants["A"], wants["B"]).sum() > 1000
    side = Side()
    try:
        c = side.ctx
        im = Images(c, gb)
        d_lts, d_table, d_inr, d_occ, d_B = c.upload(lts), c.upload(table), c.upload(inr), c.upload(occA), c.upload(occB)
        tg = Target(64, 64)
        torch.cuda.synchronize()
        c.lighting_dev(gb.cam, im.c, d_lts, n_lights, d_occ, d_inr, d_table, tg.t)                     # a. warmed up, on A
        side.stream.synchronize()
        same(tg.read(), wants["A"], "warm-up call on A")
        tg.raw.fill_(FILL)
        torch.cuda.synchronize()
        side.delay(side.stream)                                                                        # b. the delay, `before`, the upload of B
        with torch.cuda.stream(side.stream):
            before = tg.raw.clone()
            d_occ.copy_(d_B, non_blocking=True)
        c.lighting_dev(gb.cam, im.c, d_lts, n_lights, d_occ, d_inr, d_table, tg.t)                     # c. the call
        assert not side.stream.query(), f"vd_lighting_dev waited for its stream, or the delay was too short (measured {side.delay_ms:.1f} ms)"
        with torch.cuda.stream(side.stream):
            after = tg.raw.clone()
        side.stream.synchronize()
        assert bool((before == FILL).all().item()), f"before holds results: written ahead of the call's place in the stream (delay measured {side.delay_ms:.1f} ms)"
        assert bool((after == tg.raw).all().item())
        same(tg.read(), wants["B"], f"after != twin(B) (delay measured {side.delay_ms:.1f} ms)")
    finally:
        side.close()


def test_the_step_replays_from_a_graph(ctx, oracle, seeded, table, d_table):
    """Captured once, replayed after the bit words were rewritten in place: the new words' image (the camera is baked in by value)."""
    import torch
    im = seeded.im
    gb, lts, n_lights = im.gb, seeded.lts, 65
    inr = L.rule_words(gb, lts)
    occA, occB = L.subset_words(inr, L.SEED, stream=21), L.subset_words(inr, L.SEED, stream=22)
    inrB = inr.copy()
    inrB[::2, 0] &= np.uint32(0x0f0f0f0f)
    occB &= inrB
    d_inr, d_occ = ctx.upload(inr), ctx.upload(occA)
    tg = Target(64, 64)
    cam = np.array(gb.cam, dtype=abi.CAMERA, copy=True)

    def call():
        ctx.lighting_dev(cam, im.c, seeded.d_lts, n_lights, d_occ, d_inr, d_table, tg.t)

    call()                                                 # warm-up: the kernel is loaded before the capture
    torch.cuda.synchronize()
    tg.raw.fill_(FILL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    main_stream = torch.cuda.current_stream().cuda_stream
    try:
        with torch.cuda.graph(graph):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            call()
    finally:
        ctx.set_stream(main_stream)
    assert tg.untouched(), "the capture ran the kernel"
    graph.replay()
    same(tg.read(), L.shade(gb, lts, inr, occA, table), "first replay")
    cam["view_position"] = 0                                   # the host copy may change after capture
    d_inr.copy_(torch.from_numpy(inrB.view(np.uint8).reshape(-1)))
    d_occ.copy_(torch.from_numpy(occB.view(np.uint8).reshape(-1)))
    tg.raw.fill_(FILL)
    torch.cuda.synchronize()
    graph.replay()
    want = L.shade(gb, lts, inrB, occB, table)
    assert L.changed(want, L.shade(gb, lts, inr, occA, table)).sum() > 500
    same(tg.read(), want, "replay over rewritten words")


# ---- 4. the composed calls ---------------------------------------------------------------------------------------------------------------

def composed(case, form, im, n_lights, d_table, fill=FILL):
    tg = Target(im.gb.width, im.gb.height, fill)
    if form == "scene":
        info = case.ctx.shade_gbuffer_dev(case.rig.ds, im.gb.cam, im.c, case.d_lts, n_lights, d_table, tg.t)
    else:
        info = case.ctx.shade_gbuffer_prepared_dev(case.accel(form), im.gb.cam, im.c, case.d_lts, n_lights, d_table, tg.t)
    return tg.read(), info


def two_calls(case, form, im, n_lights, d_table):
    """vd_shadow_gbuffer*_dev, then vd_lighting_dev over its words -> (image, info, occluded words, in-range words)."""
    import torch
    W = (n_lights + 31) // 32
    d = [torch.full((im.n_pixels * W * 4,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
    info = case.call(form, im, n_lights, d[0], d[1])
    tg = Target(im.gb.width, im.gb.height)
    case.ctx.lighting_dev(im.gb.cam, im.c, case.d_lts, n_lights, d[0], d[1], d_table, tg.t)
    return (tg.read(), info) + tuple(t.cpu().numpy().view(np.uint32).reshape(im.n_pixels, W) for t in d)


@pytest.mark.parametrize("ray_range", (0, 1))
def test_the_composed_calls_equal_their_two_calls(ctx, ctx_options, oracle, seeded, flipped, table, d_table, ray_range):
    """scene / prepared / wide / tight on 64 x 64, 17 x 31 and 1 x 1 with 33 and 65 lights, VD_OPT_TRACE_RAY_RANGE off and on: the bytes
    and the info of vd_shadow_gbuffer*_dev followed by vd_lighting_dev.  With the option off the full shape also equals the twin fed the
    CPU's expectation of the pass - the twin of the rule and the oracle's any-hit answer."""
    ctx_options("trace.ray_range", ray_range)
    occ_w, inr_w, w = L.pass_words(oracle, "seeded", seeded.rig.scene, seeded.im.gb, seeded.lts)
    cpu = L.shade(seeded.im.gb, seeded.lts, inr_w, occ_w, table)
    for form in FORMS:
        for full in (seeded.im, flipped):
            for size in ((64, 64), (17, 31), (1, 1)):
                if full is flipped and size != (64, 64):
                    continue
                im = full.crop(*size)
                for n_lights in (33, 65):
                    what = (form, ray_range, size, n_lights, "flipped" if full is flipped else "seeded")
                    got, info = composed(seeded, form, im, n_lights, d_table)
                    want, want_info, occ, inr = two_calls(seeded, form, im, n_lights, d_table)
                    same(got, want, what)
                    assert info == want_info and info["n_points"] == len(im.gb.points()[2]) and info["words_per_point"] == (n_lights + 31) // 32, (what, info, want_info)
                    same(got, L.shade(im.gb, seeded.lts[:n_lights], inr, occ, table), what + ("the twin over the pass's words",))
                    if full is seeded.im and size == (64, 64) and n_lights == 65 and not ray_range:
                        same(got, cpu, what + ("the twin over the CPU's expectation",))
                        assert info["n_rays"] == w.n_rays


def test_composed_without_receivers_and_without_lights(ctx, oracle, seeded, table, d_table):
    """An image with no receiver walks nothing and still writes every pixel; n_lights == 0 is the step alone."""
    gb = seeded.im.gb
    none = Images(ctx, gb.with_material(np.where(G.receivers(gb.material), 2, gb.material).astype(np.uint8)))
    zeros = np.zeros((4096, 2), np.uint32)
    for form in ("scene", "wide"):
        for fill in (0xEE, 0x11):
            tg = Target(64, 64, fill)
            if form == "scene":
                info = ctx.shade_gbuffer_dev(seeded.rig.ds, gb.cam, none.c, seeded.d_lts, 33, d_table, tg.t)
            else:
                info = ctx.shade_gbuffer_prepared_dev(seeded.accel(form), gb.cam, none.c, seeded.d_lts, 33, d_table, tg.t)
            assert info == {"n_points": 0, "n_rays": 0, "n_chunks": 0, "words_per_point": 2}
            same(tg.read(), L.shade(none.gb, seeded.lts[:33], zeros, zeros, table), (form, "no receiver"))
        got, info = composed(seeded, form, seeded.im, 0, d_table)
        assert info == {"n_points": 0, "n_rays": 0, "n_chunks": 0, "words_per_point": 0}
        same(got, L.shade(gb, seeded.lts[:0], None, None, table), (form, "no lights"))
        same(got, step(ctx, seeded.im, None, 0, None, None, d_table), (form, "the step alone"))


# ---- 5. arguments --------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_target_untouched(ctx, seeded, d_table):
    import torch
    lib, rig, im = ctx.lib, seeded.rig, seeded.im
    cam = np.ascontiguousarray(im.gb.cam, dtype=abi.CAMERA).reshape(1)
    k, l, m = cam.ctypes.data, seeded.d_lts.data_ptr(), d_table.data_ptr()
    tg = Target(64, 64, pitch=2048)
    bits = torch.zeros(4096 * 4, dtype=torch.int32, device="cuda")
    b = bits.data_ptr()
    scene, accel = C.byref(rig.ds.struct), rig.acc.h
    d, n, mt = (t.data_ptr() for t in im.t)

    def gb(**kw):
        f = dict(depth=d, depth_pitch=PITCHES[0], normal_uv=n, normal_uv_pitch=PITCHES[1], material=mt, material_pitch=PITCHES[2], width=64, height=64)
        f.update(kw)
        return C.byref(abi.GBuffer(f["depth"], f["depth_pitch"], f["normal_uv"], f["normal_uv_pitch"], f["material"], f["material_pitch"], f["width"], f["height"]))

    def target(**kw):
        f = dict(rgba=tg.t.rgba, pitch=2048, width=64, height=64)
        f.update(kw)
        return C.byref(abi.ColorTarget(f["rgba"], f["pitch"], f["width"], f["height"]))

    def refused(rc, word):
        assert rc == abi.VD_ERR_INVALID_ARG and word in lib.vd_last_error(ctx.h).decode(), (rc, word, lib.vd_last_error(ctx.h))

    def all3(word, g=None, t=None, camera=k, lights=l, n_lights=4, materials=m, use_default_g=True, use_default_t=True):
        g = gb() if g is None and use_default_g else g
        t = target() if t is None and use_default_t else t
        refused(lib.vd_lighting_dev(ctx.h, camera, g, lights, n_lights, b, b, materials, t), word)
        refused(lib.vd_shade_gbuffer_dev(ctx.h, scene, camera, g, lights, n_lights, 0, materials, t, None), word)
        refused(lib.vd_shade_gbuffer_prepared_dev(ctx.h, accel, camera, g, lights, n_lights, 0, materials, t, None), word)

    all3("null pointer", camera=None)
    all3("null pointer", use_default_g=False)
    all3("null pointer", use_default_t=False)
    all3("null pointer", lights=None)
    all3("null pointer", materials=None)
    all3("null pointer", t=target(rgba=None))
    for image in ("depth", "normal_uv", "material"):
        all3("null pointer", g=gb(**{image: None}))
    refused(lib.vd_lighting_dev(ctx.h, k, gb(), l, 4, None, b, m, target()), "null pointer")          # the bit arrays, when there are lights
    refused(lib.vd_lighting_dev(ctx.h, k, gb(), l, 4, b, None, m, target()), "null pointer")
    all3("size", t=target(width=63))
    all3("size", t=target(height=65))
    all3("size", g=gb(width=32))
    all3("pitch", t=target(pitch=1008))                      # below the row
    all3("pitch", t=target(pitch=1032))                      # not a multiple of 16
    all3("depth_pitch", g=gb(depth_pitch=252))
    all3("depth_pitch", g=gb(depth_pitch=258))
    all3("normal_uv_pitch", g=gb(normal_uv_pitch=504))
    all3("normal_uv_pitch", g=gb(normal_uv_pitch=516))
    all3("material_pitch", g=gb(material_pitch=63))
    big = dict(width=1 << 15, height=(1 << 15) + 1)
    all3("2^30", g=gb(depth_pitch=1 << 17, normal_uv_pitch=1 << 18, material_pitch=1 << 15, **big), t=target(pitch=1 << 19, **big))
    all3("VD_SHADOW_MAX_LIGHTS", n_lights=abi.SHADOW_MAX_LIGHTS + 1)
    # what the composed calls refuse on top
    refused(lib.vd_shade_gbuffer_dev(ctx.h, None, k, gb(), l, 4, 0, m, target(), None), "null scene")
    refused(lib.vd_shade_gbuffer_prepared_dev(ctx.h, None, k, gb(), l, 4, 0, m, target(), None), "null accel")
    wide = dict(width=2048, height=2048)
    g4, t4 = gb(depth_pitch=8192, normal_uv_pitch=16384, material_pitch=2048, **wide), target(pitch=32768, **wide)
    refused(lib.vd_shade_gbuffer_dev(ctx.h, scene, k, g4, l, 1024, 0, m, t4, None), "0xf0000000")
    refused(lib.vd_shade_gbuffer_prepared_dev(ctx.h, accel, k, g4, l, 1024, 0, m, t4, None), "0xf0000000")
    broken = abi.TraceScene.from_buffer_copy(rig.ds.struct)
    broken.bvh_nodes = None
    refused(lib.vd_shade_gbuffer_dev(ctx.h, C.byref(broken), k, gb(), l, 4, 0, m, target(), None), "incomplete scene")      # what the pass refuses
    with pytest.raises(VoidinError):
        ctx.lighting_dev(im.gb.cam, im.c, None, 4, bits, bits, d_table, tg.t)
    # nothing to do: VD_OK, nothing written - whatever the other pointers say
    for g, t in ((gb(width=0), target(width=0)), (gb(height=0), target(height=0))):
        assert lib.vd_lighting_dev(ctx.h, None, g, None, 4, None, None, None, t) == abi.VD_OK
        info = abi.ShadowGBufferInfo(7, 7, 7, 7)
        assert lib.vd_shade_gbuffer_dev(ctx.h, scene, None, g, None, 4, 0, None, t, C.byref(info)) == abi.VD_OK
        assert (info.n_points, info.n_rays, info.n_chunks, info.words_per_point) == (0, 0, 0, 0)
        assert lib.vd_shade_gbuffer_prepared_dev(ctx.h, accel, None, g, None, 4, 0, None, t, None) == abi.VD_OK
    assert tg.untouched()
