"""vd_gbuffer_rays_dev, vd_gbuffer_resolve_dev and vd_gbuffer_trace_dev / vd_gbuffer_trace_prepared_dev
(include/voidin_gbuffer_trace.h): the G-buffer from primary rays.  The rays and the three images are compared byte for byte with the
float32 twin of tests/gbuffer_trace_cases.py (two NaNs are equal whatever their payload); the composed calls with the three-call
composition on the GPU; and the result is fed to the consumers of voidin_gbuffer.h as it is.  Every output lies between guard regions
with its row padding prefilled (write_set.Fences): only pixel bytes may change."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_cases as G
import gbuffer_trace_cases as T
import shadow_pass_cases as S
from test_gbuffer_trace_cases import ROUND_TRIP_BOUND
from test_gpu_shadow_gbuffer import same, want
from test_gpu_trace_range import Rig
from voidin_amd import abi
from voidin_amd.runtime import Context, VoidinError
from write_set import FILL, Fences

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
FORMS = ("scene", "prepared", "wide", "tight")
SHAPES = ((1, 1), (63, 1), (64, 1), (65, 3), (17, 31), (64, 9), (64, 64), (511, 1), (512, 1), (513, 1))


class Target:
    """Three images on the device, each ONE allocation between guards, prefilled; the pitches are larger than the rows and the
    material pitch is odd."""

    def __init__(self, w, h, packed=False):
        self.w, self.h = w, h
        self.rows = (4 * w, 8 * w, w)
        self.pitches = self.rows if packed else (4 * w + 12, 8 * w + 24, (w + 3) | 1)
        self.fences = Fences()
        self.bufs = [self.fences.out(name, h * p) for name, p in zip(("depth", "normal_uv", "material"), self.pitches)]
        self.c = Context.gbuffer_target(self.bufs[0].ptr, self.bufs[1].ptr, self.bufs[2].ptr, w, h, *self.pitches)

    def read(self):
        """-> (depth [N], words [N][2], material [N]) after the guards and the row padding were found untouched."""
        import torch
        torch.cuda.synchronize()
        self.fences.check()
        out = []
        for buf, pitch, row in zip(self.bufs, self.pitches, self.rows):
            raw = buf.read().reshape(self.h, pitch)
            assert (raw[:, row:] == FILL).all(), f"{buf.name}: row padding was written"
            out.append(np.ascontiguousarray(raw[:, :row]))
        return out[0].view(F).reshape(-1), out[1].view(U).reshape(-1, 2), out[2].reshape(-1)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        self.fences.check()
        return all(b.fill_intact(0) for b in self.bufs)

    def gbuffer(self):
        return Context.gbuffer(self.bufs[0].ptr, self.bufs[1].ptr, self.bufs[2].ptr, self.w, self.h, *self.pitches)


class DeviceGeometry:
    """A gbuffer_trace_cases.Geometry on the device, with both attributes (`full`) and with neither (`bare`)."""

    def __init__(self, ctx, geo):
        self.t = [ctx.upload(np.ascontiguousarray(a)) for a in (geo.instances, geo.meshes, geo.vertices, geo.indices, geo.normals, geo.tex_coords)]
        p = [abi.ptr(t) for t in self.t]
        sizes = (len(geo.instances), len(geo.meshes), len(geo.vertices), len(geo.indices))
        self.full = abi.GBufferGeometry(p[0], sizes[0], p[1], sizes[1], p[2], sizes[2], p[3], sizes[3], p[4], p[5])
        self.bare = abi.GBufferGeometry(p[0], sizes[0], p[1], sizes[1], p[2], sizes[2], p[3], sizes[3], None, None)
        self.d_normals, self.d_tex_coords = self.t[4], self.t[5]


def fenced_records(n, size):
    f = Fences()
    return f, f.out("records", n * size)


def gpu_rays(ctx, cam, w, h):
    f, buf = fenced_records(w * h, 32)
    ctx.gbuffer_rays_dev(cam, w, h, buf.ptr)
    return f, buf


def gpu_hits(ctx, rig, cam, w, h, form="scene"):
    """vd_gbuffer_rays_dev -> the walk of `form` -> (fenced device records, the records on the host)."""
    import torch
    _, rays = gpu_rays(ctx, cam, w, h)
    f, hits = fenced_records(w * h, 16)
    if form == "scene":
        ctx.trace_dev(rig.ds, rays.ptr, w * h, hits.ptr)
    else:
        ctx.trace_prepared_dev({"prepared": rig.acc, "wide": rig.acc_wide, "tight": rig.acc_tight}[form], rays.ptr, w * h, hits.ptr)
    torch.cuda.synchronize()
    f.check()
    return hits, hits.read(abi.HIT)


def resolve(ctx, cam, geometry, d_hits, w, h, packed=False):
    t = Target(w, h, packed)
    ctx.gbuffer_resolve_dev(cam, geometry, d_hits, t.c)
    return t


@pytest.fixture(scope="module")
def seeded(ctx, oracle):
    scene, geo, cam, _ = T.seeded(oracle)

    class Seeded:
        pass
    s = Seeded()
    s.scene, s.geo, s.cam, s.rig, s.dev = scene, geo, cam, Rig(ctx, scene), DeviceGeometry(ctx, geo)
    yield s
    s.rig.close()


# ---- 1. the rays -------------------------------------------------------------------------------------------------------------------

def test_rays_equal_the_twin_bit_for_bit(ctx, seeded):
    import torch
    for cam in (seeded.cam, T.hand_camera()):
        for w, h in SHAPES:
            f, buf = gpu_rays(ctx, cam, w, h)
            torch.cuda.synchronize()
            f.check()
            got, wanted = buf.read(abi.RAY), T.rays(cam, w, h)
            assert got.tobytes() == wanted.tobytes(), (w, h, np.flatnonzero(got.view(U).reshape(-1, 8) != wanted.view(U).reshape(-1, 8))[:4].tolist())


# ---- 2. resolve against the twin --------------------------------------------------------------------------------------------------------

def test_resolve_of_the_gpus_own_records_equals_the_twin_on_every_shape(ctx, oracle, seeded):
    """Each shape is an image of its own (the pixel centres differ): rays and walk on the GPU, its records read back, resolved on
    the GPU and by the twin - with both attributes and with neither.  At 64 x 64 the records are the oracle's, too."""
    for w, h in SHAPES:
        d_hits, hits = gpu_hits(ctx, seeded.rig, seeded.cam, w, h)
        for geometry, geo in ((seeded.dev.full, seeded.geo), (seeded.dev.bare, seeded.geo.without())):
            bad = T.same_image(resolve(ctx, seeded.cam, geometry, d_hits.ptr, w, h).read(), T.resolve(seeded.cam, geo, hits, w, h))
            assert bad is None, ((w, h), geo.normals is not None, bad)
        if (w, h) == (T.W, T.H):
            rec = T.seeded(oracle)[3]
            assert (hits["hit"] == rec["hit"]).all() and hits["dist"].tobytes() == rec["dist"].tobytes() and (hits["hit"] == 1).sum() > 1000
    # one attribute without the other, and packed rows
    d_hits, hits = gpu_hits(ctx, seeded.rig, seeded.cam, 17, 31)
    p = seeded.dev.full
    for normals, uvs in ((True, False), (False, True)):
        g = abi.GBufferGeometry(p.instances, p.n_instances, p.meshes, p.n_meshes, p.vertices, p.n_vertices, p.indices, p.n_indices,
                                p.normals if normals else None, p.tex_coords if uvs else None)
        bad = T.same_image(resolve(ctx, seeded.cam, g, d_hits.ptr, 17, 31, packed=True).read(),
                           T.resolve(seeded.cam, seeded.geo.without(normals=not normals, tex_coords=not uvs), hits, 17, 31))
        assert bad is None, (normals, uvs, bad)


def test_resolve_of_the_hand_made_records_equals_the_twin(ctx):
    """Every refused record is a miss, every edge of the encoder and of the f16 convert has the twin's bits - in a row of N pixels,
    and as 3 rows of N // 3 (the same ray in every pixel, so the same values)."""
    geo, cam, rec, cases = T.hand()
    dev, d_rec = DeviceGeometry(ctx, geo), ctx.upload(rec)
    n = len(rec)
    for w, h in ((n, 1), (n // 3, 3)):
        for geometry, g in ((dev.full, geo), (dev.bare, geo.without())):
            got = resolve(ctx, cam, geometry, d_rec, w, h).read()
            bad = T.same_image(got, T.resolve(cam, g, rec[: w * h], w, h))
            assert bad is None, ((w, h), g.normals is not None, bad, [cases[i].name for i in bad[2]])
    got = resolve(ctx, cam, dev.full, d_rec, n, 1).read()
    for i, c in enumerate(cases):                        # the hand values again, on the device's bytes
        if c.branch != T.HIT:
            assert got[0][i].view(U) == 0 and (got[1][i] == 0).all() and got[2][i] == 0, c.name
        elif "uv" in c.expect and c.expect["uv"][1] is not None:
            assert int(got[1][i, 1]) & 0xffff == c.expect["uv"][1], (c.name, hex(got[1][i, 1]))


# ---- 3. the composed calls -----------------------------------------------------------------------------------------------------------

def composed(ctx, s, form, w, h, attributes=True):
    t = Target(w, h)
    if form == "scene":
        ctx.gbuffer_trace_dev(s.rig.ds, s.cam, t.c, s.dev.d_normals if attributes else None, s.dev.d_tex_coords if attributes else None)
    else:
        accel = {"prepared": s.rig.acc, "wide": s.rig.acc_wide, "tight": s.rig.acc_tight}[form]
        ctx.gbuffer_trace_prepared_dev(accel, s.dev.full if attributes else s.dev.bare, s.cam, t.c)
    return t


@pytest.mark.parametrize("form", FORMS)
def test_a_composed_call_equals_the_three_calls(ctx, oracle, seeded, form):
    for (w, h), attributes in (((64, 64), True), ((17, 31), False), ((513, 1), True)):
        got = composed(ctx, seeded, form, w, h, attributes).read()
        d_hits, _ = gpu_hits(ctx, seeded.rig, seeded.cam, w, h, form)
        three = resolve(ctx, seeded.cam, seeded.dev.full if attributes else seeded.dev.bare, d_hits.ptr, w, h).read()
        for a, b, name in zip(got, three, ("depth", "normal_uv", "material")):
            assert a.tobytes() == b.tobytes(), (form, (w, h), name)
    if form == "scene":                                  # ... and the twin over the ORACLE's records
        for attributes in (True, False):
            bad = T.same_image(composed(ctx, seeded, form, T.W, T.H, attributes).read(), T.seeded_image(oracle, attributes))
            assert bad is None, (attributes, bad)


def test_a_second_call_over_a_smaller_image_and_a_grown_arena_change_nothing(ctx, seeded):
    first = composed(ctx, seeded, "scene", 64, 9).read()
    composed(ctx, seeded, "scene", 300, 200).read()           # grows the arena
    again = composed(ctx, seeded, "scene", 64, 9).read()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------

def test_the_traced_image_feeds_the_shadow_pass_and_the_points(ctx, oracle, seeded):
    """vd_shadow_gbuffer_dev over the traced image gives the CPU expectation built from the twin's image, and vd_gbuffer_points_dev
    puts every receiver within the round-trip bound of its hit point eye + dir * dist."""
    import torch
    img = T.seeded_image(oracle)
    gb = img.gbuffer()
    lts = S.lights()
    t = composed(ctx, seeded, "scene", T.W, T.H)
    assert T.same_image(t.read(), img) is None
    occ_w, inr_w, w = want(oracle, "traced", seeded.scene, gb, lts, False)
    n, W = T.W * T.H, (len(lts) + 31) // 32
    out = [torch.full((n * W * 4,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
    info = ctx.shadow_gbuffer_dev(seeded.rig.ds, seeded.cam, t.gbuffer(), ctx.upload(lts), len(lts), out[0], out[1])
    torch.cuda.synchronize()
    occ, inr = (o.cpu().numpy().view(U).reshape(n, W) for o in out)
    same(inr, inr_w, "in range")
    same(occ, occ_w, "occluded")
    recv = G.receivers(img.material)
    assert info["n_points"] == recv.sum() == len(gb.points()[2]) and info["n_rays"] == w.n_rays and 500 < recv.sum() < (img.branch == T.HIT).sum()
    # the points
    d = [torch.full((k * n * 4,), 0xEE, dtype=torch.uint8, device="cuda") for k in (3, 3, 1, 1)]
    count = ctx.gbuffer_points_dev(seeded.cam, t.gbuffer(), *d)
    torch.cuda.synchronize()
    pos = d[0].cpu().numpy().view(F).reshape(-1, 3)[:count].astype(np.float64)
    pix = d[2].cpu().numpy().view(U)[:count]
    assert count == recv.sum() and (pix == np.flatnonzero(recv)).all()
    p, eye = img.p[pix].astype(np.float64), T.pixel_rays(seeded.cam, T.W, T.H)[0][pix].astype(np.float64)
    err = np.linalg.norm(pos - p, axis=1) / np.linalg.norm(p - eye, axis=1)
    print(f"round trip on the device: {err.max():.3e} (bound {ROUND_TRIP_BOUND:.3e})")
    assert err.max() <= ROUND_TRIP_BOUND, err.max()


# ---- 5. refusals, empty images ------------------------------------------------------------------------------------------------------------

def test_refused_arguments_and_empty_images_write_nothing(ctx, seeded):
    s, lib = seeded, ctx.lib
    cam = np.ascontiguousarray(s.cam, dtype=abi.CAMERA).reshape(1)
    d_hits = ctx.upload(np.zeros(64, dtype=abi.HIT))
    t = Target(8, 8)

    def variant(**kw):
        c = abi.GBufferTarget.from_buffer_copy(t.c)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    bad_targets = [variant(depth=None), variant(normal_uv=None), variant(material=None), variant(depth_pitch=28), variant(depth_pitch=34),
                   variant(normal_uv_pitch=56), variant(normal_uv_pitch=68), variant(material_pitch=7), variant(width=1 << 16, height=(1 << 14) + 1)]
    geo = s.dev.full

    def geo_variant(name):
        g = abi.GBufferGeometry.from_buffer_copy(geo)
        setattr(g, name, None)
        return g
    calls = []
    for c in bad_targets:
        calls.append(lambda c=c: lib.vd_gbuffer_resolve_dev(ctx.h, cam.ctypes.data, C.byref(geo), abi.ptr(d_hits), C.byref(c)))
        calls.append(lambda c=c: lib.vd_gbuffer_trace_dev(ctx.h, C.byref(s.rig.ds.struct), None, None, cam.ctypes.data, C.byref(c)))
        calls.append(lambda c=c: lib.vd_gbuffer_trace_prepared_dev(ctx.h, s.rig.acc.h, C.byref(geo), cam.ctypes.data, C.byref(c)))
    for name in ("instances", "meshes", "vertices", "indices"):
        g = geo_variant(name)
        calls.append(lambda g=g: lib.vd_gbuffer_resolve_dev(ctx.h, cam.ctypes.data, C.byref(g), abi.ptr(d_hits), C.byref(t.c)))
        calls.append(lambda g=g: lib.vd_gbuffer_trace_prepared_dev(ctx.h, s.rig.acc.h, C.byref(g), cam.ctypes.data, C.byref(t.c)))
    calls += [lambda: lib.vd_gbuffer_resolve_dev(ctx.h, None, C.byref(geo), abi.ptr(d_hits), C.byref(t.c)),
              lambda: lib.vd_gbuffer_resolve_dev(ctx.h, cam.ctypes.data, None, abi.ptr(d_hits), C.byref(t.c)),
              lambda: lib.vd_gbuffer_resolve_dev(ctx.h, cam.ctypes.data, C.byref(geo), None, C.byref(t.c)),
              lambda: lib.vd_gbuffer_resolve_dev(ctx.h, cam.ctypes.data, C.byref(geo), abi.ptr(d_hits), None),
              lambda: lib.vd_gbuffer_trace_dev(ctx.h, None, None, None, cam.ctypes.data, C.byref(t.c)),
              lambda: lib.vd_gbuffer_trace_dev(ctx.h, C.byref(s.rig.ds.struct), None, None, None, C.byref(t.c)),
              lambda: lib.vd_gbuffer_trace_dev(ctx.h, C.byref(s.rig.ds.struct), None, None, cam.ctypes.data, None),
              lambda: lib.vd_gbuffer_trace_prepared_dev(ctx.h, None, C.byref(geo), cam.ctypes.data, C.byref(t.c)),
              lambda: lib.vd_gbuffer_trace_prepared_dev(ctx.h, s.rig.acc.h, None, cam.ctypes.data, C.byref(t.c)),
              lambda: lib.vd_gbuffer_trace_prepared_dev(ctx.h, s.rig.acc.h, C.byref(geo), None, C.byref(t.c)),
              lambda: lib.vd_gbuffer_trace_prepared_dev(ctx.h, s.rig.acc.h, C.byref(geo), cam.ctypes.data, None)]
    f, rays = fenced_records(64, 32)
    calls += [lambda: lib.vd_gbuffer_rays_dev(ctx.h, None, 8, 8, rays.ptr), lambda: lib.vd_gbuffer_rays_dev(ctx.h, cam.ctypes.data, 8, 8, None),
              lambda: lib.vd_gbuffer_rays_dev(ctx.h, cam.ctypes.data, 1 << 16, (1 << 14) + 1, rays.ptr)]
    for k, call in enumerate(calls):
        assert call() == abi.VD_ERR_INVALID_ARG, k
        assert lib.vd_last_error(ctx.h).decode().startswith("vd_gbuffer_"), (k, lib.vd_last_error(ctx.h))
    # empty images: VD_OK whatever else the arguments hold
    for w, h in ((0, 8), (8, 0), (0, 0)):
        c = variant(width=w, height=h)
        assert lib.vd_gbuffer_rays_dev(ctx.h, cam.ctypes.data, w, h, rays.ptr) == abi.VD_OK
        assert lib.vd_gbuffer_resolve_dev(ctx.h, cam.ctypes.data, C.byref(geo), abi.ptr(d_hits), C.byref(c)) == abi.VD_OK
        assert lib.vd_gbuffer_trace_dev(ctx.h, C.byref(s.rig.ds.struct), None, None, cam.ctypes.data, C.byref(c)) == abi.VD_OK
        assert lib.vd_gbuffer_trace_prepared_dev(ctx.h, s.rig.acc.h, C.byref(geo), cam.ctypes.data, C.byref(c)) == abi.VD_OK
    import torch
    torch.cuda.synchronize()
    f.check()
    assert t.untouched() and rays.fill_intact(0)
    with pytest.raises(VoidinError):
        ctx.gbuffer_resolve_dev(s.cam, geo, d_hits, variant(material_pitch=7))
    with pytest.raises(TypeError):
        ctx.gbuffer_trace_dev(s.rig.dw, s.cam, t.c)
    # 2^30 pixels exactly is not refused for its size (the null hit pointer is what this call is refused for)
    assert lib.vd_gbuffer_resolve_dev(ctx.h, cam.ctypes.data, C.byref(geo), None, C.byref(variant(width=1 << 15, height=1 << 15, depth_pitch=1 << 17,
                                      normal_uv_pitch=1 << 18, material_pitch=1 << 15))) == abi.VD_ERR_INVALID_ARG
    assert b"null pointer" in lib.vd_last_error(ctx.h)
