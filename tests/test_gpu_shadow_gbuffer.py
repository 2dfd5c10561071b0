"""vd_gbuffer_points_dev and vd_shadow_gbuffer_dev / vd_shadow_gbuffer_prepared_dev (include/voidin_gbuffer.h): the receivers of a
G-buffer decoded and compacted on the device, the shadow pass over them, one word set per PIXEL.  The points are compared bit for
bit with the float32 twin of tests/gbuffer_cases.py; the per-pixel words with the CPU expectation (the twin's points, the twin of the
range rule and the oracle's any-hit answer of tests/shadow_pass_cases.py, scattered to pixels) and with the COMPOSITION on the GPU -
vd_gbuffer_points_dev, vd_shadow_pass*_dev, a scatter in numpy.  Every call here writes between canary words, which must survive it."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_cases as G
import shadow_pass_cases as S
from test_gpu_trace_range import Rig
from voidin_amd import abi
from voidin_amd.runtime import Context, VoidinError
from write_set import FILL, Fences

pytestmark = pytest.mark.gpu

PAD = 8                                                    # canary words in front of and behind every output
FORMS = ("scene", "prepared", "wide", "tight")
LIGHTS = (1, 31, 32, 33, 65)
PITCHES = (G.DEPTH_PITCH, G.NORMAL_UV_PITCH, G.MATERIAL_PITCH)


class Images:
    """A G-buffer on the device at given pitches; crop(w, h) = the same device rows under a smaller VdGBuffer."""

    def __init__(self, ctx, gb, pitches=PITCHES):
        d, n, m, p = gb.rows(*pitches)
        self.ctx, self.gb, self.pitches = ctx, gb, p
        self.t = [ctx.upload(x) for x in (d, n, m)]
        self.c = Context.gbuffer(self.t[0], self.t[1], self.t[2], gb.width, gb.height, *p)

    def crop(self, w, h):
        out = Images.__new__(Images)
        out.ctx, out.gb, out.pitches, out.t = self.ctx, self.gb.crop(w, h), self.pitches, self.t
        out.c = Context.gbuffer(self.t[0], self.t[1], self.t[2], w, h, *self.pitches)
        return out

    @property
    def n_pixels(self):
        return self.gb.width * self.gb.height


def one_row(gb):
    """The image's pixels in their order as one row of width * height pixels (for the shapes a 64-wide image has no crop of).  The
    positions differ - the pixel centres do - the words and materials are the same."""
    n = gb.width * gb.height
    return G.GBuffer(gb.cam, gb.depth.reshape(1, n), gb.normal_uv.reshape(1, n, 2), gb.material.reshape(1, n))


def shapes(ctx, im):
    """The crops w x h the calls are tried at, as (name, Images): (1,1), (63,1), (64,1), (17,31), (64,8), (64,9), (64,64) of the
    64 x 64 image through its pitches - 1, 63, 64, 527, 512, 576 and 4 096 pixels.  (65, 3) is wider than that image: it is the
    upper left corner of the same pixels laid out as 3 rows of 1 365; and 511, 513 (and 65, 512, 576) pixels come as crops of the
    same pixels laid out as ONE row.  Every layout has pitches larger than its rows."""
    gb = im.gb
    out = [((w, h), im.crop(w, h)) for w, h in ((1, 1), (63, 1), (64, 1), (17, 31), (64, 8), (64, 9), (64, 64))]
    three = G.GBuffer(gb.cam, gb.depth.reshape(-1)[:4095].reshape(3, 1365), gb.normal_uv.reshape(-1, 2)[:4095].reshape(3, 1365, 2),
                      gb.material.reshape(-1)[:4095].reshape(3, 1365))
    out.append(((65, 3), Images(ctx, three, pitches=(5632, 11008, 1367)).crop(65, 3)))
    row = Images(ctx, one_row(gb), pitches=(4 * 4096 + 256, 8 * 4096 + 512, 4096 + 3))
    return out + [((w, 1), row.crop(w, 1)) for w in (65, 511, 512, 513, 576)]


class Points:
    """One vd_gbuffer_points_dev call: the arrays on the device (each between canaries, capacity width * height) and what they hold."""

    def __init__(self, ctx, im, read_back=True, fill=0xEE):
        import torch
        cap = im.n_pixels
        self.raw = [torch.full(((words + 2 * PAD) * 4,), fill, dtype=torch.uint8, device="cuda") for words in (3 * cap, 3 * cap, cap, 1)]
        self.d_pos, self.d_nor, self.d_pix, self.d_n = [r[PAD * 4:] for r in self.raw]
        self.cap, self.fill = cap, fill
        self.returned = ctx.gbuffer_points_dev(im.gb.cam, im.c, self.d_pos, self.d_nor, self.d_pix, self.d_n, read_back=read_back)

    def read(self):
        """-> (positions, normals, pixel ids, count) after the canaries and everything at or beyond the count were found untouched."""
        import torch
        torch.cuda.synchronize()
        host = [r.cpu().numpy() for r in self.raw]
        n = int(host[3][PAD * 4: PAD * 4 + 4].view(np.uint32)[0])
        assert n <= self.cap, n
        for h, words, per in zip(host, (3 * self.cap, 3 * self.cap, self.cap, 1), (3, 3, 1, 0)):
            assert (h[: PAD * 4] == self.fill).all() and (h[(PAD + words) * 4:] == self.fill).all(), "a word outside the arrays"
            if per:
                assert (h[(PAD + per * n) * 4: (PAD + words) * 4] == self.fill).all(), f"an entry at or beyond the count {n} was written"
        pos = host[0][PAD * 4: (PAD + 3 * n) * 4].view(np.float32).reshape(n, 3).copy()
        nor = host[1][PAD * 4: (PAD + 3 * n) * 4].view(np.float32).reshape(n, 3).copy()
        pix = host[2][PAD * 4: (PAD + n) * 4].view(np.uint32).copy()
        return pos, nor, pix, n


def check_points(ctx, im, what):
    p = Points(ctx, im)
    pos, nor, pix, n = p.read()
    want_pos, want_nor, want_pix = im.gb.points()
    assert n == p.returned == len(want_pix), (what, n, p.returned, len(want_pix))
    assert pix.tobytes() == want_pix.tobytes(), (what, "pixel ids")
    bad = np.flatnonzero(~(((pos.view(np.uint32) == want_pos.view(np.uint32)) | (np.isnan(pos) & np.isnan(want_pos))).all(axis=1)))
    assert bad.size == 0, (what, "positions", len(bad), bad[:4].tolist(), pos[bad[:4]].tolist(), want_pos[bad[:4]].tolist())
    assert G.same_floats(nor, want_nor), (what, "normals", np.argwhere(nor.view(np.uint32) != want_nor.view(np.uint32))[:4].tolist())
    return n


class Case:
    """A scene in every shape a call takes (Rig), a G-buffer over it and lights, all on the device."""

    def __init__(self, ctx, scene, gb, lts, pitches=PITCHES):
        self.ctx, self.rig, self.lts = ctx, Rig(ctx, scene), lts
        self.im = Images(ctx, gb, pitches)
        self.d_lts = ctx.upload(lts)

    def close(self):
        self.rig.close()

    def accel(self, form):
        return {"prepared": self.rig.acc, "wide": self.rig.acc_wide, "tight": self.rig.acc_tight}[form]

    def call(self, form, im, n_lights, d_occ, d_inr, max_chunk_rays=0):
        if form == "scene":
            return self.ctx.shadow_gbuffer_dev(self.rig.ds, im.gb.cam, im.c, self.d_lts, n_lights, d_occ, d_inr, max_chunk_rays)
        return self.ctx.shadow_gbuffer_prepared_dev(self.accel(form), im.gb.cam, im.c, self.d_lts, n_lights, d_occ, d_inr, max_chunk_rays)

    def run(self, form, im, n_lights, fill=0xEE, max_chunk_rays=0, with_in_range=True):
        """-> (occluded words [pixels][W], in-range words or None, info); the canary words around both outputs are checked."""
        import torch
        W = (n_lights + 31) // 32
        n = im.n_pixels * W
        bufs = [torch.full(((n + 2 * PAD) * 4,), fill, dtype=torch.uint8, device="cuda") for _ in range(2 if with_in_range else 1)]
        info = self.call(form, im, n_lights, bufs[0][PAD * 4:], bufs[1][PAD * 4:] if with_in_range else None, max_chunk_rays)
        torch.cuda.synchronize()
        out = []
        for b in bufs:
            raw = b.cpu().numpy()
            assert (raw[: PAD * 4] == fill).all() and (raw[(PAD + n) * 4:] == fill).all(), f"{form}: a word outside the call's {n}"
            out.append(raw[PAD * 4: (PAD + n) * 4].view(np.uint32).reshape(im.n_pixels, W).copy())
        assert info["words_per_point"] == W
        return out[0], (out[1] if with_in_range else None), info

    def composition(self, form, im, n_lights):
        """What the call replaces, on the GPU: vd_gbuffer_points_dev, vd_shadow_pass*_dev over its arrays, the scatter in numpy.
        -> (occluded words [pixels][W], in-range words, {"n_points", "n_rays"})."""
        import torch
        W = (n_lights + 31) // 32
        p = Points(self.ctx, im)
        _, _, pix, n = p.read()
        occ, inr = np.zeros((im.n_pixels, W), np.uint32), np.zeros((im.n_pixels, W), np.uint32)
        info = {"n_rays": 0}
        if n:
            d = [torch.full((n * W * 4,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
            if form == "scene":
                info = self.ctx.shadow_pass_dev(self.rig.ds, p.d_pos, p.d_nor, n, self.d_lts, n_lights, d[0], d[1])
            else:
                info = self.ctx.shadow_pass_prepared_dev(self.accel(form), p.d_pos, p.d_nor, n, self.d_lts, n_lights, d[0], d[1])
            torch.cuda.synchronize()
            occ[pix], inr[pix] = (t.cpu().numpy().view(np.uint32).reshape(n, W) for t in d)
        return occ, inr, {"n_points": n, "n_rays": info["n_rays"]}


def want(oracle, key, scene, gb, lts, ray_range):
    """The CPU expectation: (occluded words [pixels][W], in-range words, S.Want of the points)."""
    pos, nor, _ = gb.points()
    w = S.Want(S.in_range(pos, lts), S.any_hit(oracle, ("gbuffer", key), scene, pos, nor, lts, ray_range))
    return G.scatter(gb, w.occluded_words), G.scatter(gb, w.in_range_words), w


def same(got, wanted, what):
    bad = np.argwhere(got != wanted)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [hex(int(got[tuple(b)])) for b in bad[:4]], [hex(int(wanted[tuple(b)])) for b in bad[:4]])


@pytest.fixture(scope="module")
def seeded(ctx, oracle):
    scene, gb, _ = G.seeded_gbuffer(oracle)
    c = Case(ctx, scene, gb, S.lights())
    yield c
    c.close()


@pytest.fixture(scope="module")
def hand(ctx, oracle):
    c = Case(ctx, *G.hand_gbuffer(oracle), pitches=(256, 256, 5))
    yield c
    c.close()


# ---- 1. decode bytes ---------------------------------------------------------------------------------------------------------------

def test_points_equal_the_twin_bit_for_bit(ctx, oracle, seeded, hand):
    """Positions, normals, pixel ids and the count of the seeded and the hand-made G-buffer (depth 0, NaN, +inf, 1; the normal words
    on every edge of the decoder), of crops through the same pitches - 1, 63, 64, 195, 527, 512, 576 and 4 096 pixels - and of 511,
    512, 513 and 576 pixels as one row; two NaNs are equal whatever their payload."""
    assert check_points(ctx, seeded.im, "seeded") == len(seeded.im.gb.points()[2]) > 1000
    assert check_points(ctx, hand.im, "hand-made") == 10
    for name, im in shapes(ctx, seeded.im):
        check_points(ctx, im, ("crop",) + name)


def test_points_of_images_without_and_of_only_receivers_and_packed_rows(ctx, oracle, seeded):
    gb = seeded.im.gb
    recv = G.receivers(gb.material)
    none = Images(ctx, gb.with_material(np.where(recv, np.where(gb.material == 1, 0, 2), gb.material).astype(np.uint8)))
    assert check_points(ctx, none, "no receiver") == 0                     # count 0, and Points.read found nothing written
    only = Images(ctx, gb.with_material(np.where(recv, gb.material, 7).astype(np.uint8)))
    assert check_points(ctx, only, "receivers only") == 4096
    packed = Images(ctx, gb, pitches=(None, None, None))
    assert packed.pitches == (256, 512, 64)
    assert check_points(ctx, packed, "pitch equal to the row") == check_points(ctx, seeded.im, "pitch larger than the row")
    check_points(ctx, Images(ctx, gb.crop(17, 31), pitches=(None, None, None)), "packed, odd width")


# ---- 2. the pass's bits, full shape -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_full_shape_against_the_cpu_and_the_composition(ctx, oracle, seeded, form):
    """4 096 pixels x 65 lights, option off: both outputs equal pack(the twin's reach, the oracle's any-hit on the twin's points)
    scattered to pixels, and the composition on the GPU; n_points and n_rays are the twin's."""
    occ_w, inr_w, w = want(oracle, "seeded", seeded.rig.scene, seeded.im.gb, seeded.lts, False)
    occ, inr, info = seeded.run(form, seeded.im, S.N_LIGHTS)
    same(inr, inr_w, (form, "in range"))
    same(occ, occ_w, (form, "occluded"))
    c_occ, c_inr, c_info = seeded.composition(form, seeded.im, S.N_LIGHTS)
    same(occ, c_occ, (form, "occluded, against the composition"))
    same(inr, c_inr, (form, "in range, against the composition"))
    assert info["n_points"] == c_info["n_points"] == len(seeded.im.gb.points()[2]) and info["n_rays"] == c_info["n_rays"] == w.n_rays, (info, c_info, w.n_rays)
    assert info["n_chunks"] >= 1 and 0 < (occ != 0).any(axis=1).sum() <= (inr != 0).any(axis=1).sum() < 4096


# ---- 3. crops x light prefixes, the ray range on and off ---------------------------------------------------------------------------

@pytest.mark.parametrize("ray_range", (0, 1))
def test_crops_and_light_prefixes_against_the_composition(ctx, ctx_options, oracle, seeded, ray_range):
    ctx_options("trace.ray_range", ray_range)
    for k, (name, im) in enumerate(shapes(ctx, seeded.im)):
        for n_lights in LIGHTS:
            form = FORMS[(k + n_lights) % len(FORMS)]
            occ, inr, info = seeded.run(form, im, n_lights)
            c_occ, c_inr, c_info = seeded.composition(form, im, n_lights)
            what = (form, ray_range, im.gb.width, im.gb.height, n_lights)
            same(occ, c_occ, what + ("occluded",))
            same(inr, c_inr, what + ("in range",))
            assert (info["n_points"], info["n_rays"]) == (c_info["n_points"], c_info["n_rays"]), (what, info, c_info)
            assert info["n_points"] == len(im.gb.points()[2]) and inr.tobytes() == G.scatter(im.gb, S.pack(S.in_range(im.gb.points()[0], seeded.lts[:n_lights]))).tobytes(), what


@pytest.mark.parametrize("ray_range", (0, 1))
def test_hand_made_against_the_cpu(ctx, ctx_options, oracle, hand, ray_range):
    """Twelve pixels on shadow_scene, ten receivers - among them depth 0, NaN, +inf and 1 - under the hand-made lights (radius 0,
    NaN, +inf, ...): with the option on against the brute force over the open segment (segment_hits), off against the oracle."""
    ctx_options("trace.ray_range", ray_range)
    occ_w, inr_w, w = want(oracle, "hand", hand.rig.scene, hand.im.gb, hand.lts, ray_range)
    for form in FORMS:
        occ, inr, info = hand.run(form, hand.im, len(hand.lts))
        same(inr, inr_w, (form, "in range"))
        same(occ, occ_w, (form, "occluded"))
        c_occ, c_inr, _ = hand.composition(form, hand.im, len(hand.lts))
        same(occ, c_occ, (form, "occluded, against the composition"))
        assert info == {"n_points": 10, "n_rays": w.n_rays, "n_chunks": 1, "words_per_point": 1}
        assert (occ[[8, 9]] == 0).all() and (inr[[8, 9]] == 0).all()                      # materials 0 and 2


# ---- 4. chunks, what the buffers held, no in-range output, twice --------------------------------------------------------------------

def test_chunks_and_fills_do_not_change_a_byte(ctx, oracle, seeded):
    for im, n_lights, max_chunk in ((seeded.im, S.N_LIGHTS, 1500), (seeded.im.crop(64, 9), 33, 1)):
        for form in ("scene", "prepared"):
            occ1, inr1, info1 = seeded.run(form, im, n_lights)
            assert info1["n_chunks"] == 1
            for fill in (0xEE, 0xFF, 0x00):
                occ, inr, info = seeded.run(form, im, n_lights, fill=fill, max_chunk_rays=max_chunk)
                assert info["n_chunks"] > 1 and info["n_rays"] == info1["n_rays"] and info["n_points"] == info1["n_points"], (form, info, info1)
                assert occ.tobytes() == occ1.tobytes() and inr.tobytes() == inr1.tobytes(), (form, max_chunk, fill)


def test_without_the_in_range_output_and_twice(ctx, oracle, seeded):
    occ_w, _, w = want(oracle, "seeded", seeded.rig.scene, seeded.im.gb, seeded.lts, False)
    for form in ("scene", "wide"):
        occ, none, info = seeded.run(form, seeded.im, S.N_LIGHTS, with_in_range=False)
        assert none is None and info["n_rays"] == w.n_rays
        same(occ, occ_w, (form, "d_in_range == NULL"))
        first = seeded.run(form, seeded.im, S.N_LIGHTS, max_chunk_rays=20000)
        second = seeded.run(form, seeded.im, S.N_LIGHTS, max_chunk_rays=20000)
        assert first[0].tobytes() == second[0].tobytes() == occ.tobytes() and first[1].tobytes() == second[1].tobytes() and first[2] == second[2]


def test_an_image_without_receivers_writes_zeros_and_walks_nothing(ctx, oracle, seeded):
    gb = seeded.im.gb
    none = Images(ctx, gb.with_material(np.where(G.receivers(gb.material), 2, gb.material).astype(np.uint8)))
    for fill in (0xEE, 0xFF):
        occ, inr, info = seeded.run("prepared", none, 33, fill=fill)
        assert info == {"n_points": 0, "n_rays": 0, "n_chunks": 0, "words_per_point": 2}
        assert not occ.any() and not inr.any() and occ.shape == (4096, 2)


# ---- 5. the write set ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_chunk", (0, 700))
def test_write_set(ctx, oracle, seeded, max_chunk):
    """Inputs and outputs between the 64 KiB guards of tests/write_set.py: the three images, the lights and the scene buffers come
    back unchanged, no guard is touched, and of outputs one word per pixel too long nothing past width * height * W words is written."""
    import torch
    w, h, n_lights, W = 64, 17, 65, 3
    gb = seeded.im.gb.crop(w, h)
    occ_w, inr_w, wanted = want(oracle, ("seeded", w, h), seeded.rig.scene, gb, seeded.lts, False)      # (a crop has pixel centres of its own)
    rows = seeded.im.gb.rows(*PITCHES)
    f = Fences()
    imgs = [f.inp(name, data) for name, data in zip(("depth", "normal_uv", "material"), rows[:3])]
    lts = f.inp("lights", seeded.lts[:n_lights])
    scene_in = [f.inp(name, a) for name, a in zip(("tlas", "instances", "meshes", "bvh", "vertices", "indices"), seeded.rig.scene)]
    nbytes = w * h * W * 4
    occ, inr = f.out("occluded", nbytes + 4 * w * h), f.out("in_range", nbytes + 4 * w * h)
    s = abi.TraceScene()
    for k, name in enumerate(("tlas_nodes", "instances", "meshes", "bvh_nodes", "vertices", "indices")):
        setattr(s, name, scene_in[k].ptr)
        setattr(s, "n_" + name, getattr(seeded.rig.ds.struct, "n_" + name))
    c = Context.gbuffer(imgs[0].ptr, imgs[1].ptr, imgs[2].ptr, w, h, *PITCHES)
    cam = np.ascontiguousarray(gb.cam, dtype=abi.CAMERA).reshape(1)
    info = abi.ShadowGBufferInfo()
    ctx._chk(ctx.lib.vd_shadow_gbuffer_dev(ctx.h, C.byref(s), cam.ctypes.data, C.byref(c), lts.ptr, n_lights, max_chunk, occ.ptr, inr.ptr, C.byref(info)))
    torch.cuda.synchronize()
    f.check()
    occ.check_fill(nbytes)
    inr.check_fill(nbytes)
    same(occ.read(np.uint32, w * h * W).reshape(w * h, W), occ_w, "occluded")
    same(inr.read(np.uint32, w * h * W).reshape(w * h, W), inr_w, "in range")
    assert info.n_points == len(gb.points()[2]) and info.n_rays == wanted.n_rays and (info.n_chunks > 1) == (max_chunk != 0)


def test_write_set_of_the_points(ctx, oracle, seeded):
    import torch
    gb = seeded.im.gb
    pos_w, nor_w, pix_w = gb.points()
    n, cap = len(pix_w), 4096
    f = Fences()
    imgs = [f.inp(name, data) for name, data in zip(("depth", "normal_uv", "material"), gb.rows(*PITCHES)[:3])]
    pos, nor, pix, cnt = f.out("positions", 12 * cap), f.out("normals", 12 * cap), f.out("pixels", 4 * cap), f.out("count", 8)
    c = Context.gbuffer(imgs[0].ptr, imgs[1].ptr, imgs[2].ptr, 64, 64, *PITCHES)
    got = ctx.gbuffer_points_dev(gb.cam, c, pos.ptr, nor.ptr, pix.ptr, cnt.ptr)
    torch.cuda.synchronize()
    f.check()
    assert got == n == int(cnt.read(np.uint32, 1)[0])
    pos.check_fill(12 * n); nor.check_fill(12 * n); pix.check_fill(4 * n); cnt.check_fill(4)      # nothing past n_points entries
    assert G.same_floats(pos.read(np.float32, 3 * n), pos_w.reshape(-1)) and G.same_floats(nor.read(np.float32, 3 * n), nor_w.reshape(-1))
    assert pix.read(np.uint32, n).tobytes() == pix_w.tobytes()


# ---- 6. stream order -----------------------------------------------------------------------------------------------------------------

def test_stream_order(oracle):
    """tests/test_gpu_stream_order.py's method: warmed up on material image A; then on a side stream, behind its delay, the upload of
    material image B - other receivers - and the call through the context of that stream.  A clone taken on the stream in front of
    the upload holds the fill, the clone behind the call holds expected(B), and n_points is B's.  The same for the enqueue-only form
    of vd_gbuffer_points_dev, whose count and arrays are read after a stream synchronise."""
    import torch
    from test_gpu_stream_order import Side
    scene, gbA, _ = G.seeded_gbuffer(oracle)
    mB = np.roll(gbA.material, 5, axis=0)
    mB[:3] = G.LIGHT_MATERIAL                               # (a roll alone keeps the count)
    gbB = gbA.with_material(mB)
    n_lights, W = 33, 2
    lts = S.lights()[:n_lights]
    wants = {k: want(oracle, ("stream", k), scene, g, lts, False) for k, g in (("A", gbA), ("B", gbB))}
    assert wants["A"][0].tobytes() != wants["B"][0].tobytes() and wants["A"][1].tobytes() != wants["B"][1].tobytes()
    assert len(gbA.points()[2]) != len(gbB.points()[2])
    side = Side()
    try:
        c = side.ctx
        ds = c.device_scene(scene)
        im = Images(c, gbA)
        d_B = c.upload(gbB.rows(*PITCHES)[2])
        d_lts = c.upload(lts)
        outs = [torch.full((4096 * W * 4,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
        pts = [torch.full((words * 4,), FILL, dtype=torch.uint8, device="cuda") for words in (3 * 4096, 3 * 4096, 4096, 1)]
        torch.cuda.synchronize()
        c.shadow_gbuffer_dev(ds, gbA.cam, im.c, d_lts, n_lights, outs[0], outs[1])                  # a. warmed up, on A
        c.gbuffer_points_dev(gbA.cam, im.c, *pts, read_back=False)
        side.stream.synchronize()
        for o, w in zip(outs, wants["A"][:2]):
            assert o.cpu().numpy().tobytes() == w.tobytes(), "warm-up call on A"
        assert int(pts[3].cpu().numpy().view(np.uint32)[0]) == len(gbA.points()[2])
        for o in outs + pts:
            o.fill_(FILL)
        torch.cuda.synchronize()
        side.delay(side.stream)                                                                      # b. the delay, `before`, the upload of B
        with torch.cuda.stream(side.stream):
            before = [o.clone() for o in outs + pts]
            im.t[2].copy_(d_B, non_blocking=True)
        assert not side.stream.query(), f"the delay had ended before the calls were made (measured {side.delay_ms:.1f} ms)"
        c.gbuffer_points_dev(gbA.cam, im.c, *pts, read_back=False)                                   # c. the enqueue-only call, then the one that blocks
        info = c.shadow_gbuffer_dev(ds, gbA.cam, im.c, d_lts, n_lights, outs[0], outs[1])
        with torch.cuda.stream(side.stream):
            after = [o.clone() for o in outs + pts]
        side.stream.synchronize()
        for b in before:
            assert bool((b == FILL).all().item()), f"before holds results: written ahead of the call's place in the stream (delay measured {side.delay_ms:.1f} ms)"
        for a, w in zip(after[:2], wants["B"][:2]):
            assert a.cpu().numpy().tobytes() == w.tobytes(), f"after != expected(B) (delay measured {side.delay_ms:.1f} ms)"
        pos_w, nor_w, pix_w = gbB.points()
        n = len(pix_w)
        assert info["n_points"] == n == int(after[5].cpu().numpy().view(np.uint32)[0]) and info["n_rays"] == wants["B"][2].n_rays
        assert G.same_floats(after[2].cpu().numpy().view(np.float32)[: 3 * n], pos_w.reshape(-1))
        assert G.same_floats(after[3].cpu().numpy().view(np.float32)[: 3 * n], nor_w.reshape(-1))
        assert after[4].cpu().numpy().view(np.uint32)[:n].tobytes() == pix_w.tobytes()
    finally:
        side.close()


# ---- 7. arguments --------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_empty_calls(ctx, seeded):
    import torch
    lib, rig, im = ctx.lib, seeded.rig, seeded.im
    cam = np.ascontiguousarray(im.gb.cam, dtype=abi.CAMERA).reshape(1)
    k, l = cam.ctypes.data, seeded.d_lts.data_ptr()
    out = torch.full((4096 * 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    o = out.data_ptr()
    scene, accel = C.byref(rig.ds.struct), rig.acc.h
    d, n, m = (t.data_ptr() for t in im.t)

    def gb(**kw):
        f = dict(depth=d, depth_pitch=PITCHES[0], normal_uv=n, normal_uv_pitch=PITCHES[1], material=m, material_pitch=PITCHES[2], width=64, height=64)
        f.update(kw)
        return C.byref(abi.GBuffer(f["depth"], f["depth_pitch"], f["normal_uv"], f["normal_uv_pitch"], f["material"], f["material_pitch"], f["width"], f["height"]))

    def refused(rc, word):
        assert rc == abi.VD_ERR_INVALID_ARG and word in lib.vd_last_error(ctx.h).decode(), (rc, word, lib.vd_last_error(ctx.h))

    def both(word, g, camera=k, lights=l, n_lights=4, occ=o):
        refused(lib.vd_shadow_gbuffer_dev(ctx.h, scene, camera, g, lights, n_lights, 0, occ, None, None), word)
        refused(lib.vd_shadow_gbuffer_prepared_dev(ctx.h, accel, camera, g, lights, n_lights, 0, occ, None, None), word)

    refused(lib.vd_shadow_gbuffer_dev(ctx.h, None, k, gb(), l, 4, 0, o, None, None), "null scene")
    refused(lib.vd_shadow_gbuffer_prepared_dev(ctx.h, None, k, gb(), l, 4, 0, o, None, None), "null accel")
    both("null pointer", None)
    both("null pointer", gb(), camera=None)
    both("null pointer", gb(), lights=None)
    both("null pointer", gb(), occ=None)
    for image in ("depth", "normal_uv", "material"):
        both("null pointer", gb(**{image: None}))
    both("depth_pitch", gb(depth_pitch=252))
    both("depth_pitch", gb(depth_pitch=258))
    both("normal_uv_pitch", gb(normal_uv_pitch=504))
    both("normal_uv_pitch", gb(normal_uv_pitch=516))
    both("material_pitch", gb(material_pitch=63))
    both("2^30", gb(width=1 << 15, height=(1 << 15) + 1, depth_pitch=1 << 17, normal_uv_pitch=1 << 18, material_pitch=1 << 15))
    both("VD_SHADOW_MAX_LIGHTS", gb(), n_lights=abi.SHADOW_MAX_LIGHTS + 1)
    both("0xf0000000", gb(width=2048, height=2048, depth_pitch=8192, normal_uv_pitch=16384, material_pitch=2048), n_lights=1024)
    broken = abi.TraceScene.from_buffer_copy(rig.ds.struct)
    broken.bvh_nodes = None
    refused(lib.vd_shadow_gbuffer_dev(ctx.h, C.byref(broken), k, gb(), l, 4, 0, o, None, None), "incomplete scene")     # what the pass refuses
    with pytest.raises(VoidinError):
        ctx.shadow_gbuffer_dev(rig.ds, im.gb.cam, im.c, None, 4, out)
    # the front end alone
    p = (o, o + 4096 * 12, o + 4096 * 24, o + 4096 * 28)
    refused(lib.vd_gbuffer_points_dev(ctx.h, k, None, *p, None), "null pointer")
    refused(lib.vd_gbuffer_points_dev(ctx.h, None, gb(), *p, None), "null pointer")
    for hole in range(4):
        refused(lib.vd_gbuffer_points_dev(ctx.h, k, gb(), *[None if q == hole else p[q] for q in range(4)], None), "null pointer")
    refused(lib.vd_gbuffer_points_dev(ctx.h, k, gb(material=None), *p, None), "null pointer")
    refused(lib.vd_gbuffer_points_dev(ctx.h, k, gb(depth_pitch=252), *p, None), "depth_pitch")
    refused(lib.vd_gbuffer_points_dev(ctx.h, k, gb(normal_uv_pitch=516), *p, None), "normal_uv_pitch")
    refused(lib.vd_gbuffer_points_dev(ctx.h, k, gb(material_pitch=63), *p, None), "material_pitch")
    refused(lib.vd_gbuffer_points_dev(ctx.h, k, gb(width=1 << 15, height=(1 << 15) + 1, depth_pitch=1 << 17, normal_uv_pitch=1 << 18, material_pitch=1 << 15), *p, None), "2^30")
    # nothing to do: VD_OK, the info zeroed, nothing written - whatever the other pointers say
    for g, n_lights in ((gb(width=0), 4), (gb(height=0), 4), (gb(), 0), (None, 0)):
        info = abi.ShadowGBufferInfo(7, 7, 7, 7)
        assert lib.vd_shadow_gbuffer_dev(ctx.h, scene, None, g, None, n_lights, 0, o, o, C.byref(info)) == abi.VD_OK
        assert (info.n_points, info.n_rays, info.n_chunks, info.words_per_point) == (0, 0, 0, 0)
        info = abi.ShadowGBufferInfo(7, 7, 7, 7)
        assert lib.vd_shadow_gbuffer_prepared_dev(ctx.h, accel, None, g, None, n_lights, 0, o, o, C.byref(info)) == abi.VD_OK
        assert (info.n_points, info.n_rays, info.n_chunks, info.words_per_point) == (0, 0, 0, 0)
    count = C.c_uint32(7)
    assert lib.vd_gbuffer_points_dev(ctx.h, None, gb(width=0), o, o, o, o, C.byref(count)) == abi.VD_OK and count.value == 0
    assert lib.vd_gbuffer_points_dev(ctx.h, None, gb(height=0), None, None, None, None, None) == abi.VD_OK
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all().item())
