"""G-buffers and the expected points of the G-buffer tests (vd_gbuffer_points_dev, vd_shadow_gbuffer*_dev: include/voidin_gbuffer.h).
Shared by tests/test_gbuffer_cases.py (CPU: the twin against hand values, the encoding round trip, the populations) and
tests/test_gpu_shadow_gbuffer.py; a helper module, no tests in it.

The twin restates the header's definition in numpy float32 with an explicit .astype(F) after every operation, as
shadow_pass_cases.dist does: pixel centre -> ndc -> clip_to_world in the order ((c0*x + c1*y) + c2*z) + c3 -> three divisions; the
octahedral word -> normal; receiver = material neither 0 nor 2; the receivers in ascending pixel order are the points.

seeded_gbuffer: 64 x 64 pixels of the `seeded` scene of tests/trace_range_cases.py under its camera - one oracle closest-hit ray
through every pixel centre; depth = the hit point's clip z / w (float64, rounded: it is input data), normal = the hit triangle's
geometric normal facing the eye through a restatement of encode_octahedral_32, material from the instance (1, and 3 / 255 for
some instances: every value is a receiver's).  A miss has material 0 and depth 0; a fixed-seed 5 % of the hit pixels become
material 2 and another 5 % material 0 with their depth kept.  The scene fills about half of every 512-pixel tile, so the two tiles
the populations need whole (tests/test_gbuffer_cases.py) are made by the material assignment: in tile 0 the misses are receivers
too (depth 0: points at infinity), in tile 2 nothing is.  Rows lie at pitches larger than the row: 256-byte multiples, and an odd one for the material.

hand_gbuffer: 4 x 3 pixels over trace_range_cases.shadow_scene - depth exactly 0, NaN, +inf and 1; the normal words 0, 0xffffffff,
0x7fff8000, 0x80007fff and the encodings of the four unit normals with n.z = 0 (NO 32-bit word decodes to n.z == 0 exactly - the
sum 1 - |v.x| - |v.y| would need a half-integer code, and float32 rounding does not make one either: test_gbuffer_cases.py looks
at all of them - so these four, whose n.z is one code step below zero, are the words on that edge: they take the t > 0 fold with
every sign of x and y); materials 0, 1, 2, 3 and 255.
Everything is computed once per process and shared: nobody changes what these functions return."""
import numpy as np

import trace_range_cases as cases
from voidin_amd import abi, synth

F = np.float32
SEED = synth.SEED_BASE + 91
NO_MATERIAL, LIGHT_MATERIAL = 0, 2
TILE = 512                                  # pixels a wave of gbuffer.hip owns
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the twin -----------------------------------------------------------------------------------------------------------------

def decode_normal(n32):
    """decode_octahedral_32 (encoding.wgsl:17-28) as the header states it -> float32 [N][3]."""
    n32 = np.asarray(n32, np.uint32)
    with np.errstate(all="ignore"):
        vx = ((n32 & np.uint32(0xffff)).astype(F) / F(65535)).astype(F)
        vy = (((n32 >> np.uint32(16)) & np.uint32(0xffff)).astype(F) / F(65535)).astype(F)
        vx = ((vx * F(2)).astype(F) - F(1)).astype(F)
        vy = ((vy * F(2)).astype(F) - F(1)).astype(F)
        nz = ((F(1) - np.abs(vx)).astype(F) - np.abs(vy)).astype(F)
        t = np.where((-nz) > F(0), -nz, F(0)).astype(F)
        nx = (vx + np.where(vx > F(0), -t, t).astype(F)).astype(F)
        ny = (vy + np.where(vy > F(0), -t, t).astype(F)).astype(F)
        ln = np.sqrt((((nx * nx).astype(F) + (ny * ny).astype(F)).astype(F) + (nz * nz).astype(F)).astype(F)).astype(F)
        return np.stack([(nx / ln).astype(F), (ny / ln).astype(F), (nz / ln).astype(F)], axis=1)


def encode_normal(n):
    """encode_octahedral_32 (encoding.wgsl:4-15), restated in float32 -> uint32 [N].  One departure: in the fold of the lower
    hemisphere the sign of a component that is exactly 0 counts as +1.  WGSL's sign(0) is 0, which sends a normal with z < 0 and an
    x or y of exactly 0 to another direction altogether - (0, 0, -1) to the code of (0, 0, 1) - and no decoder brings that back;
    this function only makes input data, and the round trip it is tested by includes the south pole."""
    n = np.asarray(n, F).reshape(-1, 3)
    s = ((np.abs(n[:, 0]) + np.abs(n[:, 1])).astype(F) + np.abs(n[:, 2])).astype(F)
    v = (n / s[:, None]).astype(F)
    fold = v[:, 2] < 0
    sign = lambda a: np.where(a < 0, F(-1), F(1)).astype(F)
    x = np.where(fold, ((F(1) - np.abs(v[:, 1])).astype(F) * sign(v[:, 0])).astype(F), v[:, 0]).astype(F)
    y = np.where(fold, ((F(1) - np.abs(v[:, 0])).astype(F) * sign(v[:, 1])).astype(F), v[:, 1]).astype(F)
    dx = np.floor((((x * F(0.5)).astype(F) + F(0.5)).astype(F) * F(65535)).astype(F) + F(0.5)).astype(np.uint32)
    dy = np.floor((((y * F(0.5)).astype(F) + F(0.5)).astype(F) * F(65535)).astype(F) + F(0.5)).astype(np.uint32)
    return (dy << np.uint32(16)) | dx


def world_position(cam, x, y, width, height, depth):
    """world_position_from_depth (uv.wgsl:13-22) at the centre of pixel (x, y) -> float32 [N][3]."""
    M = np.asarray(cam["clip_to_world"], F).reshape(16)
    with np.errstate(all="ignore"):
        ux = ((np.asarray(x).astype(F) + F(0.5)).astype(F) / F(width)).astype(F)
        uy = ((np.asarray(y).astype(F) + F(0.5)).astype(F) / F(height)).astype(F)
        nx = ((ux * F(2)).astype(F) - F(1)).astype(F)
        ny = (((F(1) - uy).astype(F) * F(2)).astype(F) - F(1)).astype(F)
        nz = np.asarray(depth, F)
        w4 = [((((M[r] * nx).astype(F) + (M[4 + r] * ny).astype(F)).astype(F) + (M[8 + r] * nz).astype(F)).astype(F) + M[12 + r]).astype(F) for r in range(4)]
        return np.stack([(w4[0] / w4[3]).astype(F), (w4[1] / w4[3]).astype(F), (w4[2] / w4[3]).astype(F)], axis=1)


def receivers(material):
    material = np.asarray(material)
    return (material != NO_MATERIAL) & (material != LIGHT_MATERIAL)


class GBuffer:
    """Three images [height][width] (normal_uv: [height][width][2]) with the camera they were made under.  crop(w, h): the upper
    left corner - the same pixels at the same pitches when stored."""

    def __init__(self, cam, depth, normal_uv, material):
        self.cam, self.depth, self.normal_uv, self.material = cam, np.asarray(depth, F), np.asarray(normal_uv, np.uint32), np.asarray(material, np.uint8)
        self.height, self.width = self.material.shape
        self._points = None

    def crop(self, w, h):
        return GBuffer(self.cam, self.depth[:h, :w], self.normal_uv[:h, :w], self.material[:h, :w])

    def with_material(self, material):
        return GBuffer(self.cam, self.depth, self.normal_uv, material)

    def rows(self, depth_pitch=None, normal_uv_pitch=None, material_pitch=None, fill=0xC3):
        """-> (depth bytes, normal_uv bytes, material bytes, the three pitches): rows at the given pitches (default: packed), the
        padding filled with `fill`."""
        w, h = self.width, self.height
        pitches = (4 * w if depth_pitch is None else depth_pitch, 8 * w if normal_uv_pitch is None else normal_uv_pitch, w if material_pitch is None else material_pitch)
        out = []
        for img, pitch, row in ((self.depth, pitches[0], 4 * w), (self.normal_uv, pitches[1], 8 * w), (self.material, pitches[2], w)):
            buf = np.full((h, pitch), fill, np.uint8)
            buf[:, :row] = np.ascontiguousarray(img).view(np.uint8).reshape(h, row)
            out.append(buf.reshape(-1))
        return out[0], out[1], out[2], pitches

    def points(self):
        """The twin -> (positions [P][3], normals [P][3], pixel ids [P]) of the receivers in ascending pixel order."""
        if self._points is None:
            pix = np.flatnonzero(receivers(self.material).reshape(-1)).astype(np.uint32)
            x, y = pix % np.uint32(self.width), pix // np.uint32(self.width)
            pos = world_position(self.cam, x, y, self.width, self.height, self.depth.reshape(-1)[pix])
            nor = decode_normal(self.normal_uv.reshape(-1, 2)[pix, 0])
            self._points = np.ascontiguousarray(pos, F), np.ascontiguousarray(nor, F), pix
        return self._points


def scatter(gb, words):
    """Per-point words [P][W] -> per-pixel words [width * height][W]: a receiver's are its point's, every other pixel's zero."""
    out = np.zeros((gb.width * gb.height, words.shape[1]), np.uint32)
    out[gb.points()[2]] = words
    return out


def same_floats(a, b):
    """Bit equality of two float32 arrays in which two NaNs are equal whatever their payload (the host's default NaN and the GPU's
    differ in the sign bit)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the seeded G-buffer ------------------------------------------------------------------------------------------------------

W = H = 64
CAMERA = dict(eye=(0, 2.5, 40), pitch_deg=0)      # trace_range_cases._seeded_scene's
DEPTH_PITCH, NORMAL_UV_PITCH, MATERIAL_PITCH = 512, 768, 77      # rows of 256, 512 and 64 bytes
FULL_TILE, EMPTY_TILE = 0, 2                # tiles of 512 pixels = 8 rows: all receivers / no receiver (every crop of 8 rows and more holds the first)


def centre_rays(cam, width, height):
    """One ray per pixel from the eye through the pixel centre (float64, rounded): the line on which world_position puts the
    pixel's points."""
    M = cam["clip_to_world"].reshape(4, 4).astype(np.float64).T
    i = np.arange(width * height)
    ux, uy = (i % width + 0.5) / width, (i // width + 0.5) / height
    clip = np.stack([ux * 2 - 1, (1 - uy) * 2 - 1, np.full(len(i), 1e-3), np.ones(len(i))])
    p = (M @ clip).T
    p = p[:, :3] / p[:, 3:4]
    eye = cam["view_position"][:3].astype(np.float64)
    d = p - eye[None, :]
    rays = np.zeros(len(i), dtype=abi.RAY)
    rays["eye"] = eye.astype(F)
    rays["dir"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    return rays


def _world_triangles(scene, instance, triangle):
    """The world-space corners [N][3][3] (float64) of triangle slot `triangle` of the mesh of instance `instance`."""
    tl, inst, meshes, bn, verts, idx = scene
    verts, idx = np.asarray(verts, F).reshape(-1, 3), np.asarray(idx, np.uint32).reshape(-1)
    out = np.zeros((len(instance), 3, 3))
    for k, (i, t) in enumerate(zip(instance, triangle)):
        m = meshes[min(int(inst[i]["mesh"]), len(meshes) - 1)]
        at = int(m["base_index"]) + 3 * int(t)
        local = verts[idx[at: at + 3].astype(np.int64) + int(np.uint32(m["vertex_offset"]))].astype(np.float64)
        T = inst[i]["transform"].reshape(4, 4).astype(np.float64)          # [column][row]
        out[k] = local @ T[:3, :3] + T[3, :3]
    return out


def seeded_gbuffer(oracle):
    """-> (scene, GBuffer 64 x 64, hit mask [4096])."""
    def make():
        scene = cases.case("seeded", oracle).scene
        cam = synth.camera_uniform(**CAMERA)
        rays = centre_rays(cam, W, H)
        rec, _ = oracle.trace(scene, rays, threads=8)
        hit = rec["hit"] == 1
        at = np.flatnonzero(hit)
        eye, d = rays["eye"].astype(np.float64), rays["dir"].astype(np.float64)
        p = eye[at] + d[at] * rec["dist"][at].astype(np.float64)[:, None]
        PV = cam["projection"].reshape(4, 4).astype(np.float64).T @ cam["view"].reshape(4, 4).astype(np.float64).T
        clip = (PV @ np.concatenate([p, np.ones((len(p), 1))], axis=1).T).T
        depth = np.zeros(W * H, F)
        depth[at] = (clip[:, 2] / clip[:, 3]).astype(F)
        tri = _world_triangles(scene, rec["instance"][at], rec["triangle"][at])
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        n[(n * (eye[at] - p)).sum(axis=1) < 0] *= -1
        normal_uv = np.zeros((W * H, 2), np.uint32)
        normal_uv[at, 0] = encode_normal(n.astype(F))
        normal_uv[:, 1] = 0xA5000000 + np.arange(W * H)                      # the uv word: never read
        material = np.zeros(W * H, np.uint8)
        inst_mat = scene[1]["material"][rec["instance"][at]].astype(np.uint8)
        which = rec["instance"][at] % 7
        material[at] = np.where(which == 3, 255, np.where(which == 5, 3, inst_mat))
        # The scene fills about half of every tile, so two tiles are MADE whole by the material alone: in FULL_TILE the pixels that
        # hit nothing are receivers too (material 1 over depth 0 - their points lie at infinity, out of every light's reach), in
        # EMPTY_TILE every hit pixel has material 0 with its depth kept.
        tile = np.arange(W * H) // TILE
        material[(tile == FULL_TILE) & ~hit] = 1
        material[(tile == EMPTY_TILE) & hit] = NO_MATERIAL
        # the excluded kinds: 5 % of the hit pixels each, by a fixed-seed order, outside those two tiles
        free = at[(tile[at] != FULL_TILE) & (tile[at] != EMPTY_TILE)]
        order = free[np.argsort(synth.uniform01(SEED, 0, len(free)), kind="stable")]
        k = len(at) // 20
        material[order[:k]] = LIGHT_MATERIAL
        material[order[k: 2 * k]] = NO_MATERIAL
        return scene, GBuffer(cam, depth.reshape(H, W), normal_uv.reshape(H, W, 2), material.reshape(H, W)), hit
    return _once("seeded", make)


# ---- the hand-made G-buffer ---------------------------------------------------------------------------------------------------

HAND_CAMERA = dict(eye=(10, 1, 25), pitch_deg=0)
AXIS_WORDS = (0x8000ffff, 0x80000000, 0xffff8000, 0x00008000)       # encode_normal of (1,0,0), (-1,0,0), (0,1,0), (0,-1,0)


def hand_gbuffer(oracle):
    """-> (scene, GBuffer 4 x 3, lights): shadow_scene, its pixels' points about its z = 0 plane (linear depth 25 under a camera at
    z = 25) where the depth is an ordinary one, and the lights of shadow_pass_cases.hand_made."""
    def make():
        import shadow_pass_cases as S
        scene, _, _, lts = S.hand_made(oracle)
        cam = synth.camera_uniform(**HAND_CAMERA)
        d = F(float(cam["znear"]) / 25.0)
        depth = np.array([0, np.nan, np.inf, 1, d, d, d, d, d, d, d, d], F)
        words = np.array([0, 0xffffffff, 0x7fff8000, 0x80007fff, *AXIS_WORDS, 0, 0xffffffff, 0x7fff8000, 0x80007fff], np.uint32)
        material = np.array([1, 3, 255, 1, 3, 255, 1, 1, 0, 2, 1, 3], np.uint8)     # ten receivers: every word above is decoded
        normal_uv = np.stack([words, 0x5A000000 + np.arange(12, dtype=np.uint32)], axis=1)
        return scene, GBuffer(cam, depth.reshape(3, 4), normal_uv.reshape(3, 4, 2), material.reshape(3, 4)), lts
    return _once("hand", make)
