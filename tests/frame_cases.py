"""The two frames of the end-to-end tests - scene + camera + lights + material table -> lit image - with the float32 twin chain
spelled out and the comparisons against the float64 renderer of tests/frame_reference.py.  Shared by tests/test_frame_reference.py
(CPU: the twins against the renderer) and tests/test_gpu_frame.py (the device's own outputs against it); a helper module, no tests
in it.

seeded: gbuffer_trace_cases.seeded_scene at 64 x 64 with its vertex normals and uvs, the 65 lights of shadow_pass_cases.lights(), the
material table of lighting_cases.materials().
room: hand-built and well-conditioned, 50 x 37 pixels (1 850: the last wave is partial).  A floor and a back wall (one quad mesh,
two triangles), two uv-spheres with true smooth normals (normal = position), three boxes with face normals, uvs on everything.
Instances: a non-uniform scale (floor), a rotation (wall, box 0), a translation (sphere 0), a non-uniform scale (sphere 1, material
LIGHT_MATERIAL), a box of material 0 and a MIRRORED box of a mesh of its own, wound inward with its outward vertex normals kept: a ray passes its
near faces and meets the inside of its far ones, whose stored normals (mat3(transform) of the vertex normals, no facing flip) look
away from the eye - covr > 0 - while its geometric normals take the header's flip toward the eye.
Material bytes come from ids above 255 too (0x105, 0x107).  The camera is pitched down.  Five lights: overhead (the boxes' shadows
on the floor); one whose radius ends in mid-floor; one behind the wall; one inside a box; one below sphere 0, which lies BEHIND it
on the rays from the floor, so the ray range changes its bit.
Each frame also comes without vertex normals (geometric normals facing the eye) and without uvs: Frame.form().

The twin chain: gbuffer_trace_cases.rays -> the oracle's closest hits -> gbuffer_trace_cases.resolve -> .gbuffer() ->
lighting_cases.pass_words (the twin's points, the twin of the range rule, the oracle's any-hit answer) -> lighting_cases.shade.
With the ray range on the any-hit answer is the brute force over the open segment (0, 1) of shadow_pass_cases.segment_hits; for the
seeded frame that takes a minute, so it is RECORDED in tests/golden/frame_seeded_range.npz with a digest of its points and lights
(`PYTHONPATH=. python tests/frame_cases.py` writes it anew);
tests/test_frame_reference.py holds the record against the oracle's closest hit (hit and dist < 1) on every ray.
Everything is computed once per process and shared: nobody changes what these functions return."""
import hashlib
import math
import os

import numpy as np

import frame_reference as R
import gbuffer_cases as G
import gbuffer_trace_cases as T
import lighting_cases as L
import shadow_pass_cases as S
from conftest import GOLDEN, golden
from voidin_amd import abi, synth

F, U = np.float32, np.uint32
RECORD = "frame_seeded_range.npz"
_CACHE = {}

# ---- the constants of profiles/frame_reference.md ---------------------------------------------------------------------------------
# Measured on the CPU: the largest ratio, over both frames and all three forms, of the float32 DEFINITION (the twins of
# tests/*_cases.py, not a kernel) against the float64 renderer; each is asserted at FACTOR times its measured value (the precedent
# of test_gbuffer_trace_cases.ROUND_TRIP_BOUND; any factor above 1 would do - a correct kernel equals the twin bit for bit, and an
# error of definition is orders of magnitude larger).
FACTOR = 4
DEPTH_MEASURED = 1.723e-6                        # |depth32 - depth64| / depth64 on robust hit pixels
UV_MEASURED = 1.0048e-3                           # |uv32 before the f16 rounding - uv64| / max(1, |uv64|)
NORMAL_MEASURED = 1.1008e-3                       # |decoded normal - normal64| beyond NORMAL_QUANT: the float32 u, v under the interpolation
COLOUR_MEASURED = 2.667e-6                       # |twin - float64| / S per channel
DEPTH_BOUND, UV_BOUND, COLOUR_TOL = FACTOR * DEPTH_MEASURED, FACTOR * UV_MEASURED, FACTOR * COLOUR_MEASURED
# The octahedral word.  A code is floor(c + 0.5) of a coordinate c in [0, 65535] that stands for v in [-1, 1]: a step is 2 / 65535 of
# v and the stored v is within h = 1 / 65535 of the exact one, in both coordinates.  The decoder makes of (vx, vy) a vector n with
# |n.x| + |n.y| + |n.z| = 1: above the fold n = (vx, vy, 1 - |vx| - |vy|), below it n = (sign(vx) (1 - |vy|), sign(vy) (1 - |vx|), ...) -
# on either side |dn| <= sqrt(h^2 + h^2 + (2 h)^2) = sqrt(6) h.  Such an n is at least 1 / sqrt(3) long, so the unit normal moves by
# at most sqrt(6) h * sqrt(3) = sqrt(18) / 65535 = 6.47e-5.  On top of it what float32 does in the encoder and before it: some
# 32 roundings of 2^-24 on values of size 1.
NORMAL_QUANT = math.sqrt(18.0) / 65535 + 32 * 2.0 ** -24
# That is the whole bound wherever it holds: every form of the room, and the seeded frame's geometric normals (measured: 6.01e-5).
# Interpolated normals inherit the error of the float32 u and v, which the seeded scene makes large: its eye is 40 to 90 units from
# triangles a tenth of a unit wide, and its vertex normals are random, so they turn by radians across a triangle.  For that frame with
# its vertex normals, and for it alone, the part beyond the quantisation is measured like the uv's (the same u and v make it).
NORMAL_ARITHMETIC_APPLIES = {("room", True): False, ("room", False): False, ("seeded", True): True, ("seeded", False): False}


def normal_bound(frame):
    """NORMAL_QUANT, plus FACTOR * NORMAL_MEASURED for the seeded frame with its vertex normals."""
    return NORMAL_QUANT + (FACTOR * NORMAL_MEASURED if NORMAL_ARITHMETIC_APPLIES[frame.name.split()[0], frame.normals] else 0.0)


# The occlusion cap holds for the room and for the seeded frame's geometric normals (0.4 % borderline).  With its random vertex
# normals the seeded frame misses it (6.7 %): the shadow ray starts 1e-4 along a normal that is often almost in the surface, so its
# receiver's own triangles lie within the margin of t = 0.  There the occlusion bits are compared on the robust pairs without the cap.
OCCLUSION_CAP_ASSERTED = {("room", True): True, ("room", False): True, ("seeded", True): False, ("seeded", False): True}
F16_HALF_ULP = 2.0 ** -11                    # half an ulp of a binary16, relative to the power of two below the value
# caps on what the robust flags may exclude (from the renderer alone)
CAP_PIXELS, CAP_IN_RANGE, CAP_OCCLUDED = 0.02, 0.005, 0.05


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Frame:
    def __init__(self, name, scene, geo, cam, w, h, lights, table, normals=True, tex_coords=True):
        self.name, self.scene, self.full_geo, self.cam, self.w, self.h, self.lights, self.table = name, scene, geo, cam, w, h, lights, table
        self.normals, self.tex_coords = normals, tex_coords
        self.geo = geo.without(normals=not normals, tex_coords=not tex_coords)
        self.key = (name, normals, tex_coords)

    def form(self, normals=True, tex_coords=True):
        return _once(("form", self.name, normals, tex_coords),
                     lambda: Frame(self.name, self.scene, self.full_geo, self.cam, self.w, self.h, self.lights, self.table, normals, tex_coords))


FORMS = ((True, True), (False, True), (True, False))      # (vertex normals, uvs)


# ---- the seeded frame ------------------------------------------------------------------------------------------------------------------

def seeded(oracle):
    def make():
        scene, geo = T.seeded_scene(oracle)
        return Frame("seeded", scene, geo, synth.camera_uniform(**G.CAMERA), T.W, T.H, S.lights(), L.materials())
    return _once("seeded", make)


# ---- the room --------------------------------------------------------------------------------------------------------------------------

ROOM_W, ROOM_H = 50, 37


def _outward(v, i):
    """Triangles wound so that (v1 - v0) x (v2 - v0) points away from the origin: the side intersect_trig accepts."""
    t = np.asarray(i, np.int64).reshape(-1, 3).copy()
    p = np.asarray(v, np.float64)[t]
    inward = (np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) * p.mean(axis=1)).sum(axis=1) < 0
    t[inward] = t[inward][:, [0, 2, 1]]
    return t.reshape(-1).astype(U)


def _quad():
    v, i = synth.plane_mesh(1.0, 1.0)                    # y = 0, normal +y
    return v, i, np.tile(np.array([0, 1, 0], F), (4, 1)), (v[:, [0, 2]] + F(0.5)).astype(F)


def _sphere(resolution=3):
    v, i = synth.uv_sphere(1.0, resolution)
    vside, uside = 4 * resolution, 8 * resolution
    k = np.arange(len(v))
    uv = np.stack([(k % (uside + 1)) / uside, (k // (uside + 1)) / vside], axis=1).astype(F)
    n = (v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)).astype(F)
    return v, _outward(v, i), n, uv


def _box(inside_out=False):
    """The cube [-1, 1]^3 with four vertices and the outward normal per face."""
    v, n, uv, i = [], [], [], []
    for axis in range(3):
        for s in (-1.0, 1.0):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            for ca, cb in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3); p[axis], p[a], p[b] = s, ca, cb
                v.append(p); uv.append(((ca + 1) / 2, (cb + 1) / 2))
                e = np.zeros(3); e[axis] = s
                n.append(e)
            k = len(v) - 4
            i += [k, k + 1, k + 2, k, k + 2, k + 3]
    v = np.asarray(v, F)
    i = _outward(v, np.asarray(i, U))
    if inside_out:                                       # wound inward: a ray passes the near faces and meets the far ones from inside
        i = i.reshape(-1, 3)[:, [0, 2, 1]].reshape(-1).copy()
    return v, i, np.asarray(n, F), np.asarray(uv, F)


def _trs(t=(0, 0, 0), ry_deg=0.0, rx_deg=0.0, s=(1, 1, 1)):
    """translate . rotate_y . rotate_x . scale as a mathematical 4 x 4 (float64)."""
    cy, sy, cx, sx = (f(math.radians(a)) for a in (ry_deg, rx_deg) for f in (math.cos, math.sin))
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    M = np.eye(4)
    M[:3, :3] = ry @ rx @ np.diag(np.asarray(s, np.float64))
    M[:3, 3] = t
    return M


ROOM_INSTANCES = (      # (mesh, material, transform)
    (0, 1, dict(t=(0, 0, -2), s=(24, 1, 16))),                                  # the floor: x in [-12, 12], z in [-10, 6]
    (0, 3, dict(t=(0, 5, -10), rx_deg=90, s=(24, 1, 10))),                      # the back wall: z = -10, facing +z
    (1, 255, dict(t=(3.5, 6.5, -3))),                                           # sphere 0, above light 4
    (1, G.LIGHT_MATERIAL, dict(t=(-4, 1.25, -3), s=(1.5, 1, 1.5))),             # sphere 1: a non-uniform scale, LIGHT_MATERIAL
    (2, 0x105, dict(t=(0, 1.25, -4), ry_deg=30)),                               # box 0: rotated, material byte 5
    (2, 0, dict(t=(5, 2.25, -5), s=(1, 2, 1))),                                 # box 1: material 0, light 3 inside
    (3, 0x107, dict(t=(-7.5, 1.5, -5.5), ry_deg=20, s=(-1.25, 1.25, 1.25))),    # box 2: inside out, mirrored in x
)
ROOM_LIGHTS = (         # (position, radius, colour)
    ((0.5, 9.0, -3.5), 40.0, (1.0, 0.9, 0.8)),       # 0: overhead
    ((-6.0, 2.0, 1.0), 6.0, (0.2, 0.9, 0.3)),        # 1: its radius ends in mid-floor
    ((0.0, 4.0, -13.0), 30.0, (0.9, 0.2, 0.2)),      # 2: behind the wall
    ((5.0, 2.25, -5.0), 25.0, (0.3, 0.3, 1.0)),      # 3: inside box 1
    ((3.5, 4.5, -3.0), 12.0, (0.8, 0.8, 0.2)),       # 4: sphere 0 lies behind it on the rays from the floor
)
ROOM_CAMERA = dict(eye=(0.3, 7.5, 8.0), pitch_deg=-30.0, aspect=ROOM_W / ROOM_H, fovy=math.pi / 3)


def room(oracle):
    def make():
        V, I, N, UV, B = [], [], [], [], []
        parts = (_quad(), _sphere(), _box(), _box(inside_out=True))
        infos = np.zeros(len(parts), dtype=abi.MESH_INFO)
        vo = bo = no = 0
        for k, (v, i, n, uv) in enumerate(parts):
            v = np.asarray(v, F).reshape(-1, 3)
            nodes, idx = oracle.bvh_build(v, i)
            infos[k]["min"], infos[k]["max"] = synth.mesh_bounds(v)
            infos[k]["index_count"], infos[k]["base_index"], infos[k]["vertex_offset"], infos[k]["bvh_index"] = len(idx), bo, vo, no
            V.append(v); I.append(np.asarray(idx, U)); N.append(n); UV.append(uv); B.append(nodes)
            vo += len(v); bo += len(idx); no += len(nodes)
        inst = np.stack([synth.instance_from_matrix(_trs(**kw).T.reshape(16), mesh, material) for mesh, material, kw in ROOM_INSTANCES])
        verts, idx = np.concatenate(V), np.concatenate(I)
        scene = (oracle.tlas_build(inst, infos), inst, infos, np.concatenate(B), verts, idx)
        geo = T.Geometry(inst, infos, verts, idx, np.concatenate(N), np.concatenate(UV))
        lts = np.zeros(len(ROOM_LIGHTS), dtype=abi.LIGHT)
        for k, (p, r, c) in enumerate(ROOM_LIGHTS):
            lts[k]["position"], lts[k]["radius"], lts[k]["color"], lts[k]["_pad"] = p, r, c, 0xBEEF0000 + k
        return Frame("room", scene, geo, synth.camera_uniform(**ROOM_CAMERA), ROOM_W, ROOM_H, lts, L.materials())
    return _once("room", make)


def resized(frame, w, h):
    """The same frame at another image size (the camera keeps its aspect: the pixels are not square, which no stage minds)."""
    return _once(("resized", frame.key, w, h), lambda: Frame(f"{frame.name} {w}x{h}", frame.scene, frame.full_geo, frame.cam, w, h, frame.lights, frame.table,
                                                             frame.normals, frame.tex_coords))


def frames(oracle):
    return {"room": room(oracle), "seeded": seeded(oracle)}


# ---- the twin chain --------------------------------------------------------------------------------------------------------------------

class Chain:
    """What the twins make of a frame: rec (the oracle's records of the twin's rays), img (gbuffer_trace_cases.Image), gb, and per
    ray_range in (False, True) the words and the image: occ[r], inr, colour[r]."""


def segment_any_hit(oracle, frame, gb):
    """bool [P][L]: something lies on the open segment (0, 1) of the shadow ray of every pair - shadow_pass_cases.segment_hits, for
    the seeded frame from the record."""
    pos, nor, _ = gb.points()
    lts = frame.lights
    if frame.name != "seeded":
        return S.any_hit(oracle, ("gbuffer", ("frame",) + frame.key + (frame.w, frame.h)), frame.scene, pos, nor, lts, True)
    g = golden(RECORD)
    tag = "n" if frame.normals else "g"
    assert str(g["digest_" + tag]) == S.digest(pos, nor, lts), f"{RECORD} was recorded for other points or lights: write it anew"
    return np.unpackbits(g["hit_" + tag], count=len(pos) * len(lts)).astype(bool).reshape(len(lts), len(pos)).T.copy()


def chain(oracle, frame, rays=None, cam=None, tag=()):
    """The twin chain of the module's docstring.  rays / cam: the inputs of a deliberately wrong variant (tag names it in the cache)."""
    def make():
        c = Chain()
        camera = frame.cam if cam is None else cam
        c.rays = T.rays(camera, frame.w, frame.h) if rays is None else rays
        c.rec = np.ascontiguousarray(oracle.trace(frame.scene, c.rays, threads=8)[0])
        c.img = T.resolve(camera, frame.geo, c.rec, frame.w, frame.h)
        c.gb = c.img.gbuffer()
        pos, nor, _ = c.gb.points()
        c.reach = S.in_range(pos, frame.lights)
        hit = {False: S.any_hit(oracle, ("gbuffer", ("frame",) + frame.key + (frame.w, frame.h) + tag), frame.scene, pos, nor, frame.lights, False)}
        if not tag:
            hit[True] = segment_any_hit(oracle, frame, c.gb)
        c.hit = hit
        c.want = {r: S.Want(c.reach, h) for r, h in hit.items()}
        c.inr = G.scatter(c.gb, c.want[False].in_range_words)
        c.occ = {r: G.scatter(c.gb, w.occluded_words) for r, w in c.want.items()}
        c.colour = {r: L.shade(c.gb, frame.lights, c.inr, o, frame.table) for r, o in c.occ.items()}
        return c
    return _once(("chain",) + frame.key + (frame.w, frame.h) + tag, make)


# ---- the comparisons (stages a, b, c) ---------------------------------------------------------------------------------------------------

def unpack(words, n_lights):
    """uint32 [N][W] -> bool [N][L]."""
    words = np.asarray(words, U)
    l = np.arange(n_lights)
    return ((words[:, l >> 5] >> (l & 31).astype(U)) & U(1)).astype(bool)


def f16_to_float(h):
    return np.asarray(h, np.uint16).view(np.float16).astype(np.float64)


class Reference:
    """The float64 renderer's view of a G-buffer that the float32 path stored: decode of the stored values, delta, and - computed on
    demand and kept - the primary stage at margin 8 * delta and the light bits with the ray range off and on."""

    def __init__(self, frame, depth, words, material, pos32, pix):
        self.frame, self.pix = frame, np.asarray(pix, np.int64)
        self.depth, self.words, self.material = np.asarray(depth, F).reshape(-1), np.asarray(words, U).reshape(-1, 2), np.asarray(material, np.uint8).reshape(-1)
        self.pos, self.nor, self.delta = R.decode(self.depth, self.words, frame.cam, frame.w, frame.h, at=self.pix, pos32=pos32)
        self.margin = 8.0 * self.delta
        self.sc = _once(("ref scene", frame.name.split()[0]), lambda: R._Scene(frame.scene))
        self._bits, self._shared = {}, {}

    def primary(self):
        # the primary stage reads no stored value: one per (frame, form, margin)
        return _once(("primary",) + self.frame.key + (self.frame.w, self.frame.h, self.margin), lambda: R.primary(self.sc, self.frame.geo, self.frame.cam, self.frame.w, self.frame.h, self.margin))

    def bits(self, ray_range):
        if ray_range not in self._bits:
            self._bits[ray_range] = R.light_bits(self.pos, self.nor, self.sc, self.frame.lights, ray_range, self.margin, self._shared)
        return self._bits[ray_range]


def reference(frame, depth, words, material, pos32, pix):
    """One Reference per distinct stored G-buffer: the device's images are the twin's bytes, so a GPU test shares the twin's.
    The digest covers what a Reference computes from - depth, the normal word, the float32 positions and their pixels; the uv word
    and the material image are no part of it: the decode and the light bits read neither."""
    parts = (np.asarray(depth, F), np.asarray(words, U).reshape(-1, 2)[:, 0], np.asarray(pos32, F), np.asarray(pix, np.int64))
    digest = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in parts)).hexdigest()
    shared = _once(("reference", frame.name, frame.w, frame.h, digest), lambda: Reference(frame, depth, words, material, pos32, pix))
    if shared.frame is frame:
        return shared
    # the form without uvs stores the same depths and normal words: the decode and the light bits are shared, the primary stage is its own
    own = Reference.__new__(Reference)
    own.__dict__.update(shared.__dict__)
    own.frame = frame
    return own


def reference_of_chain(frame, c):
    return reference(frame, c.img.depth, c.img.words, c.img.material, *c.gb.points()[::2])


def stage_a(frame, ref, hit, instance, triangle, depth, words, material, report=None):
    """The primary stage: the stored images (and, where known, the records' instance and triangle) against R.primary on its robust
    pixels -> the list of what disagrees (empty: the stage passes).  report: a dict that receives the measured ratios."""
    p = ref.primary()
    bad = []
    hit = np.asarray(hit, bool)
    rob = p.robust
    if rob.mean() < 1 - CAP_PIXELS:
        bad.append(("cap: robust pixels", float(rob.mean())))
    x = np.flatnonzero(rob & (hit != p.hit))
    if len(x):
        bad.append(("hit / miss", len(x), x[:4].tolist()))
    k = np.flatnonzero(rob & hit & p.hit)
    if instance is not None:
        x = k[(np.asarray(instance)[k] != p.instance[k]) | (np.asarray(triangle)[k] != p.triangle[k])]
        if len(x):
            bad.append(("instance / triangle", len(x), x[:4].tolist()))
    depth, words, material = np.asarray(depth, F).reshape(-1), np.asarray(words, U).reshape(-1, 2), np.asarray(material).reshape(-1)
    with np.errstate(all="ignore"):
        e_depth = np.abs(depth[k].astype(np.float64) - p.depth[k]) / np.abs(p.depth[k])
    x = k[~(e_depth <= DEPTH_BOUND)]
    if len(x):
        bad.append(("depth", len(x), x[:4].tolist(), float(np.nanmax(e_depth))))
    # the normal word: the direction it decodes to (in float64) against the exact unit normal, within normal_bound(frame).  (The codes
    # themselves cannot be compared: where z < 0 and x or y is next to 0 the fold's sign jumps, and two codes far apart decode to
    # directions next to each other.)
    e_dir = np.linalg.norm(R.decode_normal(words[k, 0]) - p.normal[k], axis=1)
    x = k[~(e_dir <= normal_bound(frame))]
    if len(x):
        bad.append(("normal", len(x), x[:4].tolist(), float(np.nanmax(e_dir))))
    e_uv = np.zeros(0)
    if frame.tex_coords:
        got = np.stack([f16_to_float(words[k, 1] & U(0xffff)), f16_to_float(words[k, 1] >> U(16))], axis=1)
        want = p.uv[k]
        scale = np.maximum(1.0, np.abs(want))
        half_ulp = F16_HALF_ULP * 2.0 ** np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -14)))
        e_uv = (np.abs(got - want) - half_ulp) / scale                                  # what is left for the float32 arithmetic
        x = k[~(e_uv <= UV_BOUND).all(axis=1)]
        if len(x):
            bad.append(("uv", len(x), x[:4].tolist(), float(e_uv.max())))
    else:
        x = k[words[k, 1] != 0]
        if len(x):
            bad.append(("uv word without uvs", len(x), x[:4].tolist()))
    x = np.flatnonzero(rob & hit & p.hit & (material != p.material) | rob & ~p.hit & (material != 0))
    if len(x):
        bad.append(("material", len(x), x[:4].tolist()))
    if report is not None:
        report.update(depth=float(e_depth.max()) if len(k) else 0.0, uv=float(e_uv.max()) if e_uv.size else 0.0,
                      normal=max(0.0, float(e_dir.max()) - NORMAL_QUANT) if len(k) else 0.0, robust_pixels=float(rob.mean()), hits=int(p.hit.sum()))
    return bad


def stage_b(frame, ref, in_range, occluded, ray_range, report=None):
    """The light bits [P][L] (bool, receivers in pixel order) against R.light_bits over decode of the stored G-buffer, on the robust
    bits -> the list of what disagrees."""
    b = ref.bits(ray_range)
    bad = []
    in_range, occluded = np.asarray(in_range, bool), np.asarray(occluded, bool)
    share_in = 1 - b.robust_in.mean() if b.robust_in.size else 0.0
    pairs = b.in_range & b.robust_in
    share_occ = 1 - b.robust_occ[pairs].mean() if pairs.any() else 0.0
    if share_in > CAP_IN_RANGE:
        bad.append(("cap: borderline in-range bits", float(share_in)))
    if OCCLUSION_CAP_ASSERTED[frame.name.split()[0], frame.normals] and share_occ > CAP_OCCLUDED:
        bad.append(("cap: borderline occlusion bits", float(share_occ)))
    x = np.argwhere(b.robust_in & (in_range != b.in_range))
    if len(x):
        bad.append(("in range", len(x), x[:4].tolist()))
    both = pairs & in_range & b.robust_occ
    x = np.argwhere(both & (occluded != b.occluded))
    if len(x):
        bad.append(("occluded", len(x), x[:4].tolist()))
    if report is not None:
        report.update({"borderline_in_range": float(share_in), ("borderline_occluded", ray_range): float(share_occ),
                       "in_range_share": float(b.in_range.mean()), ("occluded_share", ray_range): float(b.occluded[pairs].mean()) if pairs.any() else 0.0})
    return bad


def stage_c(frame, depth, words, material, in_range_words, occluded_words, colour, report=None, nor_sign=1.0):
    """The colour [N][4] against R.shade in float64, fed the stored G-buffer through decode and the very bits the float32 path was
    fed: per channel |colour - float64| <= COLOUR_TOL * S; and the sanity of the image -> the list of what disagrees."""
    n = frame.w * frame.h
    pos, nor, _ = R.decode(depth, words, frame.cam, frame.w, frame.h)
    L_ = len(frame.lights)
    want, S_ = R.shade(pos, nor_sign * nor, material, frame.table, frame.lights, unpack(in_range_words, L_), unpack(occluded_words, L_), frame.cam["view_position"])
    colour = np.asarray(colour, F).reshape(n, 4)
    material = np.asarray(material).reshape(-1)
    bad = []
    with np.errstate(all="ignore"):
        e = np.abs(colour[:, :3].astype(np.float64) - want[:, :3]) / S_
    e = np.where(S_ == 0, np.where(colour[:, :3] == 0, 0.0, np.inf), e)
    lit = material != G.NO_MATERIAL
    x = np.flatnonzero(lit & ~(e <= COLOUR_TOL).all(axis=1))
    if len(x):
        bad.append(("colour", len(x), x[:4].tolist(), float(np.nanmax(e[lit])) if lit.any() else 0.0, colour[x[:2]].tolist(), want[x[:2]].tolist()))
    if np.isnan(colour).any() or not (colour[:, 3] == 1).all():
        bad.append(("a NaN, or an alpha that is not 1",))
    if not (colour[~lit] == (1, 0, 1, 1)).all():
        bad.append(("a pixel of material 0 that is not magenta",))
    if report is not None:
        report["colour"] = float(e[lit].max()) if lit.any() else 0.0
    return bad


if __name__ == "__main__":      # record the seeded frame's segment answers (about two minutes)
    from oracle import ref as oracle_
    oracle_.load()
    fr = seeded(oracle_)
    out = {}
    for tag, normals in (("n", True), ("g", False)):
        f_ = fr.form(normals, True)
        img_ = T.resolve(f_.cam, f_.geo, np.ascontiguousarray(oracle_.trace(f_.scene, T.rays(f_.cam, f_.w, f_.h), threads=8)[0]), f_.w, f_.h)
        pos_, nor_, _ = img_.gbuffer().points()
        hit_ = S.segment_hits(f_.scene, S.shadow_rays(oracle_, pos_, nor_, f_.lights))
        out["hit_" + tag], out["digest_" + tag] = np.packbits(hit_), np.array(S.digest(pos_, nor_, f_.lights))
        print(RECORD, tag, len(hit_), "rays,", int(hit_.sum()), "hit")
    np.savez_compressed(os.path.join(GOLDEN, RECORD), **out)
