"""A whole frame on the device: vd_gbuffer_trace*_dev into a device G-buffer, vd_shade_gbuffer*_dev on that very G-buffer - and the
same as three calls, vd_gbuffer_trace*_dev, vd_shadow_gbuffer*_dev, vd_lighting_dev.  For the two frames of tests/frame_cases.py
(`room`, `seeded`) in all four forms of the scene the result is (a) the twin chain's, byte for byte - the three images, the bit words,
the colour, with VD_OPT_TRACE_RAY_RANGE off and on - and (b) the float64 frame of tests/frame_reference.py: the device's own outputs go
through the stages of tests/test_frame_reference.py with the same constants and the same robust sets, so this stands if a twin is ever
edited together with its kernel.  Every output lies between canaries or guards, over a prefill, at a pitch larger than its row."""
import numpy as np
import pytest

import frame_cases as FC
import gbuffer_trace_cases as T
from test_gpu_gbuffer_trace import DeviceGeometry, Target as ImageTarget, gpu_hits
from test_gpu_lighting import Target as ColourTarget, same as same_colour
from test_gpu_shadow_gbuffer import FORMS, PAD, Points, same as same_words
from test_gpu_trace_range import Rig
from voidin_amd import abi

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32


class Device:
    """A frame's scene in every form (Rig), its geometry with the attributes, its lights and the material table on the device."""

    def __init__(self, ctx, fr):
        self.ctx, self.rig, self.dev = ctx, Rig(ctx, fr.scene), DeviceGeometry(ctx, fr.full_geo)
        self.d_lts, self.d_table = ctx.upload(fr.lights), ctx.upload(fr.table)

    def close(self):
        self.rig.close()

    def accel(self, form):
        return {"prepared": self.rig.acc, "wide": self.rig.acc_wide, "tight": self.rig.acc_tight}[form]

    def geometry(self, fr):
        p = self.dev.full
        return abi.GBufferGeometry(p.instances, p.n_instances, p.meshes, p.n_meshes, p.vertices, p.n_vertices, p.indices, p.n_indices,
                                   p.normals if fr.normals else None, p.tex_coords if fr.tex_coords else None)

    def trace(self, fr, form):
        """vd_gbuffer_trace*_dev -> the guarded images on the device."""
        t = ImageTarget(fr.w, fr.h)
        if form == "scene":
            self.ctx.gbuffer_trace_dev(self.rig.ds, fr.cam, t.c, self.dev.d_normals if fr.normals else None, self.dev.d_tex_coords if fr.tex_coords else None)
        else:
            self.ctx.gbuffer_trace_prepared_dev(self.accel(form), self.geometry(fr), fr.cam, t.c)
        return t

    def shade(self, fr, form, t):
        """vd_shade_gbuffer*_dev over the images of trace() -> (colour [N][4], info)."""
        tg = ColourTarget(fr.w, fr.h)
        n = len(fr.lights)
        if form == "scene":
            info = self.ctx.shade_gbuffer_dev(self.rig.ds, fr.cam, t.gbuffer(), self.d_lts, n, self.d_table, tg.t)
        else:
            info = self.ctx.shade_gbuffer_prepared_dev(self.accel(form), fr.cam, t.gbuffer(), self.d_lts, n, self.d_table, tg.t)
        return tg.read(), info

    def three_calls(self, fr, form, t):
        """vd_shadow_gbuffer*_dev, then vd_lighting_dev over its words -> (colour, info, occluded words [N][W], in-range words)."""
        import torch
        n, pixels = len(fr.lights), fr.w * fr.h
        words = pixels * ((n + 31) // 32)
        bufs = [torch.full(((words + 2 * PAD) * 4,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
        d_occ, d_inr = bufs[0][PAD * 4:], bufs[1][PAD * 4:]
        if form == "scene":
            info = self.ctx.shadow_gbuffer_dev(self.rig.ds, fr.cam, t.gbuffer(), self.d_lts, n, d_occ, d_inr)
        else:
            info = self.ctx.shadow_gbuffer_prepared_dev(self.accel(form), fr.cam, t.gbuffer(), self.d_lts, n, d_occ, d_inr)
        tg = ColourTarget(fr.w, fr.h)
        self.ctx.lighting_dev(fr.cam, t.gbuffer(), self.d_lts, n, d_occ, d_inr, self.d_table, tg.t)
        colour = tg.read()
        out = []
        for b in bufs:
            raw = b.cpu().numpy()
            assert (raw[: PAD * 4] == 0xEE).all() and (raw[(PAD + words) * 4:] == 0xEE).all(), "a word outside the bit arrays"
            out.append(raw[PAD * 4: (PAD + words) * 4].view(U).reshape(pixels, -1).copy())
        return colour, info, out[0], out[1]

    def points(self, fr, t):
        """vd_gbuffer_points_dev over the images of trace(): the float32 stored-path positions -> (positions, pixel ids)."""
        class Shim:
            pass
        im = Shim()
        im.n_pixels, im.c = fr.w * fr.h, t.gbuffer()
        im.gb = Shim()
        im.gb.cam = fr.cam
        pos, _, pix, _ = Points(self.ctx, im).read()
        return pos, pix


@pytest.fixture(scope="module")
def devices(ctx, oracle):
    d = {name: Device(ctx, fr) for name, fr in FC.frames(oracle).items()}
    yield d
    for x in d.values():
        x.close()


def check_frame(ctx, oracle, dev, fr, form, ray_range, identity=True):
    """One frame in one form: (a) against the twin chain, the composed calls against the three calls; (b) the device's own outputs
    through stages a, b and c of the float64 frame."""
    what = (fr.name, fr.normals, fr.tex_coords, form, ray_range)
    c = FC.chain(oracle, fr)
    t = dev.trace(fr, form)
    depth, words, material = t.read()
    bad = T.same_image((depth, words, material), c.img)
    assert bad is None, (what, bad)
    colour, info = dev.shade(fr, form, t)
    same_colour(colour, c.colour[bool(ray_range)], what + ("the composed call against the twin",))
    colour3, info3, occ, inr = dev.three_calls(fr, form, t)
    same_colour(colour3, colour, what + ("three calls against two",))
    assert info == info3 and info["n_points"] == len(c.gb.points()[2]) and info["n_rays"] == c.want[bool(ray_range)].n_rays, (what, info, info3)
    same_words(inr, c.inr, what + ("in range",))
    same_words(occ, c.occ[bool(ray_range)], what + ("occluded",))
    assert T.same_image(t.read(), c.img) is None, (what, "a consumer wrote to the G-buffer")
    # (b) the float64 frame
    pos32, pix = dev.points(fr, t)
    ref = FC.reference(fr, depth, words, material, pos32, pix)
    hit = (depth.view(U) != 0) | (words != 0).any(axis=1) | (material != 0)          # a miss is all zeros
    rec = gpu_hits(ctx, dev.rig, fr.cam, fr.w, fr.h, form)[1] if identity else None
    a = FC.stage_a(fr, ref, hit, None if rec is None else rec["instance"], None if rec is None else rec["triangle"], depth, words, material)
    L_ = len(fr.lights)
    b = FC.stage_b(fr, ref, FC.unpack(inr, L_)[pix], FC.unpack(occ, L_)[pix], bool(ray_range))
    s = FC.stage_c(fr, depth, words, material, inr, occ, colour)
    assert a == [] and b == [] and s == [], (what, a, b, s)


@pytest.mark.parametrize("ray_range", (0, 1))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ("room", "seeded"))
def test_a_frame_is_the_twin_chain_and_the_float64_frame(ctx, ctx_options, oracle, devices, name, form, ray_range):
    ctx_options("trace.ray_range", ray_range)
    check_frame(ctx, oracle, devices[name], FC.frames(oracle)[name], form, ray_range)


@pytest.mark.parametrize("form,normals,tex_coords", (("scene", False, True), ("wide", True, False)))
def test_the_room_without_vertex_normals_and_without_uvs(ctx, ctx_options, oracle, devices, form, normals, tex_coords):
    """normals == NULL: geometric normals facing the eye (the inside-out box takes the flip); tex_coords == NULL: word 1 is 0."""
    for ray_range in (0, 1):
        ctx_options("trace.ray_range", ray_range)
        check_frame(ctx, oracle, devices["room"], FC.room(oracle).form(normals, tex_coords), form, ray_range)


def test_a_smaller_and_then_a_larger_frame_on_the_same_context(ctx, oracle, devices):
    """After the frames above: the room at 23 x 17 (the arenas of the composed calls are reused), then at 96 x 71 (they grow), then at
    its own size again - each compared the same way."""
    room = FC.room(oracle)
    for w, h in ((23, 17), (96, 71), (room.w, room.h)):
        for form in ("scene", "prepared"):
            check_frame(ctx, oracle, devices["room"], FC.resized(room, w, h), form, 0, identity=(form == "scene"))
