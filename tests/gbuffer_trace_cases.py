"""The float32 twin and the cases of the G-buffer-from-primary-rays tests (vd_gbuffer_rays_dev, vd_gbuffer_resolve_dev,
vd_gbuffer_trace*_dev: include/voidin_gbuffer_trace.h).  Shared by tests/test_gbuffer_trace_cases.py (CPU: the twin against hand
values, its encoder and f16 packing against independent ones, its restated Moeller-Trumbore against the oracle's distances, the
populations, the round trip) and tests/test_gpu_gbuffer_trace.py; a helper module, no tests in it.

The twin restates the header's definition in numpy float32 with an explicit .astype(F) after every operation, as gbuffer_cases.py does:
pixel centre -> ndc -> clip_to_world -> eye and dir by true divisions; record -> instance -> mesh -> three vertex ids, a miss at the
first level that says so; depth = clip z / w of eye + dir * dist; u, v by the expressions of intersect_trig on the instance-space
ray; the normal interpolated and sent through mat3(transform), or geometric and facing the eye; the octahedral word; the uv pair
packed to two f16 by an integer round-to-nearest-even of its own.

seeded: the `seeded` scene of tests/trace_range_cases.py (its instances given materials 1, 3, 255, 0x105, 2, 0x100 in turn) under
gbuffer_cases.CAMERA at 64 x 64, per-vertex normals (uniform in [-1, 1]^3) and uvs (uniform in [-2, 6]^2) from synth.uniform01 at a
fixed seed.  hand: a camera whose clip_to_world has two zero columns, so EVERY pixel has the ray eye = (0, 0, 5), dir = (0, 0, -1)
exactly; a unit right triangle (0,0,0) (1,0,0) (0,1,0) for which u = oe.x, v = oe.y and t = oe.z exactly; instances that are
translations, a mirror and a non-uniform scale; and one record per case (HAND) as an N x 1 image.
Everything is computed once per process and shared: nobody changes what these functions return."""
import numpy as np

import gbuffer_cases as G
import trace_range_cases as cases
from voidin_amd import abi, synth

F = np.float32
U = np.uint32
SEED = synth.SEED_BASE + 97
MAX_DIST = F(1e30)
HIT, NO_HIT, BAD_INSTANCE, BAD_MESH, BAD_TRIANGLE, BAD_INDEX, BAD_VERTEX = range(7)      # the branch a record takes
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- float32 arithmetic, one rounding per operation ---------------------------------------------------------------------------------

def _f(x):
    return np.asarray(x, F)


def mul(a, b):
    return (_f(a) * _f(b)).astype(F)


def add(a, b):
    return (_f(a) + _f(b)).astype(F)


def sub(a, b):
    return (_f(a) - _f(b)).astype(F)


def div(a, b):
    return (_f(a) / _f(b)).astype(F)


def dot(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z over [..., 3]."""
    return add(add(mul(a[..., 0], b[..., 0]), mul(a[..., 1], b[..., 1])), mul(a[..., 2], b[..., 2]))


def cross(a, b):
    """oracle/vd_oracle_math.h:23-26."""
    return np.stack([sub(mul(a[..., 1], b[..., 2]), mul(b[..., 1], a[..., 2])), sub(mul(a[..., 2], b[..., 0]), mul(b[..., 2], a[..., 0])),
                     sub(mul(a[..., 0], b[..., 1]), mul(b[..., 0], a[..., 1]))], axis=-1)


def mat_row(M, r, x, y, z, w):
    """Row r of M * (x, y, z, w), M column-major [..., 16]: ((c0*x + c1*y) + c2*z) + c3*w, the products by w carried out."""
    return add(add(add(mul(M[..., r], x), mul(M[..., 4 + r], y)), mul(M[..., 8 + r], z)), mul(M[..., 12 + r], w))


def mat_xyz(M, p, w):
    return np.stack([mat_row(M, r, p[..., 0], p[..., 1], p[..., 2], F(w)) for r in range(3)], axis=-1)


def normalise(n):
    ln = np.sqrt(dot(n, n)).astype(F)
    return div(n, ln[..., None])


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------

def pixel_rays(cam, width, height):
    """-> (eye [N][3], dir [N][3]) of the pixels in order."""
    M = _f(cam["clip_to_world"]).reshape(16)
    i = np.arange(width * height)
    x, y = (i % width).astype(F), (i // width).astype(F)
    with np.errstate(all="ignore"):
        ux, uy = div(add(x, F(0.5)), F(width)), div(add(y, F(0.5)), F(height))
        nx, ny = sub(mul(ux, F(2)), F(1)), sub(mul(sub(F(1), uy), F(2)), F(1))
        one, zero = F(1), F(0)
        pw = mat_row(M, 3, nx, ny, one, one)
        eye = np.stack([div(mat_row(M, r, nx, ny, one, one), pw) for r in range(3)], axis=-1)
        t = np.stack([mat_row(M, r, nx, ny, zero, one) for r in range(3)], axis=-1)
        return eye, normalise(t)


def rays(cam, width, height):
    """The rays vd_gbuffer_rays_dev writes -> abi.RAY [width * height]."""
    eye, d = pixel_rays(cam, width, height)
    out = np.zeros(width * height, dtype=abi.RAY)
    out["eye"], out["dir"], out["_pad0"], out["_pad1"] = eye, d, F(0), MAX_DIST
    return out


def encode(n):
    """encode_octahedral_32 with the header's two departures -> uint32 [N]: the fold's sign(0) is +1; the conversion sends a NaN to 0
    and clamps to [0, 65535]."""
    n = _f(n).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = add(add(np.abs(n[:, 0]), np.abs(n[:, 1])), np.abs(n[:, 2]))
        q = div(n, s[:, None])
        fold = q[:, 2] < 0
        sign = lambda a: np.where(a < 0, F(-1), F(1)).astype(F)
        ox = np.where(fold, mul(sub(F(1), np.abs(q[:, 1])), sign(q[:, 0])), q[:, 0]).astype(F)
        oy = np.where(fold, mul(sub(F(1), np.abs(q[:, 0])), sign(q[:, 1])), q[:, 1]).astype(F)

        def code(v):
            d = np.floor(add(mul(add(mul(v, F(0.5)), F(0.5)), F(65535)), F(0.5))).astype(F)
            d = np.where(np.isnan(d), F(0), np.clip(d, F(0), F(65535)))
            return d.astype(np.int64).astype(U)
        return (code(oy) << U(16)) | code(ox)


def f16_bits(x):
    """float32 -> the bits of the nearest binary16, ties to even, in integer arithmetic: overflow to infinity, subnormals kept, a NaN
    the quiet NaN of its sign -> uint32 [N] (low 16 bits)."""
    b = _f(x).reshape(-1).view(U).astype(np.int64)
    sign, a = (b >> 16) & 0x8000, b & 0x7fffffff
    # normal numbers: rebias the exponent by 112, keep 10 mantissa bits, round on the 13 dropped ones (a carry walks into the exponent)
    r = a - (112 << 23)
    m, rem = r >> 13, r & 0x1fff
    normal = m + ((rem > 0x1000) | ((rem == 0x1000) & ((m & 1) == 1)))
    # below 2^-14: the multiple of 2^-24 nearest to |x| (float64 holds |x| * 2^24 exactly, rint rounds ties to even)
    sub_ = np.rint(np.where(a < 0x38800000, np.abs(_f(x).reshape(-1)), F(0)).astype(np.float64) * 2.0 ** 24).astype(np.int64)
    out = np.where(a > 0x7f800000, 0x7e00, np.where(a >= 0x477ff000, 0x7c00, np.where(a >= 0x38800000, normal, sub_)))      # 0x477ff000 = 65520
    return (sign | out).astype(U)


def pack_uv(t):
    """pack2x16float -> uint32 [N]."""
    t = _f(t).reshape(-1, 2)
    return f16_bits(t[:, 0]) | (f16_bits(t[:, 1]) << U(16))


class Geometry:
    """What the resolve step gathers from, as host arrays: a trace scene's instances, meshes, vertices and indices, with per-vertex
    normals [V][3] and uvs [V][2] (either may be None)."""

    def __init__(self, instances, meshes, vertices, indices, normals=None, tex_coords=None):
        self.instances, self.meshes = np.asarray(instances, abi.INSTANCE).reshape(-1), np.asarray(meshes, abi.MESH_INFO).reshape(-1)
        self.vertices, self.indices = _f(vertices).reshape(-1, 3), np.asarray(indices, U).reshape(-1)
        self.normals = None if normals is None else _f(normals).reshape(-1, 3)
        self.tex_coords = None if tex_coords is None else _f(tex_coords).reshape(-1, 2)

    def without(self, normals=True, tex_coords=True):
        return Geometry(self.instances, self.meshes, self.vertices, self.indices, None if normals else self.normals, None if tex_coords else self.tex_coords)


class Image:
    """A resolved image: depth [N], words [N][2], material [N] in pixel order, and of the twin's intermediate values the branch of
    every record, u, v, the restated distance t and the world hit point p (rows of misses: zero)."""

    def __init__(self, cam, width, height):
        n = width * height
        self.cam, self.width, self.height = cam, width, height
        self.depth, self.words, self.material = np.zeros(n, F), np.zeros((n, 2), U), np.zeros(n, np.uint8)
        self.branch = np.zeros(n, np.int64)
        self.u, self.v, self.t, self.p = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F), np.zeros((n, 3), F)

    def gbuffer(self):
        """-> gbuffer_cases.GBuffer: what the consumers of voidin_gbuffer.h read."""
        h, w = self.height, self.width
        return G.GBuffer(self.cam, self.depth.reshape(h, w), self.words.reshape(h, w, 2), self.material.reshape(h, w))


def resolve(cam, geo, hits, width, height):
    """The twin of vd_gbuffer_resolve_dev -> Image."""
    hits = np.asarray(hits, abi.HIT).reshape(-1)
    n = width * height
    assert len(hits) == n
    out = Image(cam, width, height)
    inst, meshes = geo.instances, geo.meshes
    # the levels of the chain, a record leaving at the first that refuses it (64-bit sums: nothing wraps but the vertex id)
    branch = np.full(n, HIT)
    alive = hits["hit"] == 1
    branch[~alive] = NO_HIT

    def refuse(ok, code):
        nonlocal alive
        branch[alive & ~ok] = code
        alive = alive & ok
    refuse(hits["instance"] < len(inst), BAD_INSTANCE)
    ii = np.where(alive, hits["instance"], 0).astype(np.int64)
    mesh = inst["mesh"][ii].astype(np.int64)
    refuse(mesh < len(meshes), BAD_MESH)
    mi = meshes[np.where(alive, mesh, 0)]
    last = 3 * hits["triangle"].astype(np.int64) + 2
    refuse(last < mi["index_count"].astype(np.int64), BAD_TRIANGLE)
    refuse(mi["base_index"].astype(np.int64) + last < len(geo.indices), BAD_INDEX)
    at = np.where(alive, mi["base_index"].astype(np.int64) + last - 2, 0)
    with np.errstate(over="ignore"):
        ids = (geo.indices[at[:, None] + np.arange(3)] + mi["vertex_offset"].astype(np.int32).view(U)[:, None]).astype(U)      # bvh.wgsl:31, wrapping
    refuse((ids < len(geo.vertices)).all(axis=1), BAD_VERTEX)
    out.branch = branch
    k = np.flatnonzero(alive)
    if not len(k):
        return out
    ids, I, dist = ids[k].astype(np.int64), inst[ii[k]], hits["dist"][k].astype(F)
    eye, d = pixel_rays(cam, width, height)
    eye, d = eye[k], d[k]
    T, Ti = _f(I["transform"]), _f(I["inv_transform"])
    v0, v1, v2 = (geo.vertices[ids[:, j]] for j in range(3))
    with np.errstate(all="ignore"):
        # depth (visibility.wgsl:35-40)
        p = add(eye, mul(d, dist[:, None]))
        V, P = _f(cam["view"]).reshape(16), _f(cam["projection"]).reshape(16)
        vp = [mat_row(V, r, p[:, 0], p[:, 1], p[:, 2], F(1)) for r in range(4)]
        out.depth[k] = div(mat_row(P, 2, *vp), mat_row(P, 3, *vp))
        out.p[k] = p
        # u, v (bvh.wgsl:82-83, intersections.wgsl:26-36), and t for the comparison with the walk
        oe, od = mat_xyz(Ti, eye, 1), mat_xyz(Ti, d, 0)
        edge1, edge2 = sub(v1, v0), sub(v2, v0)
        uvec = cross(od, edge2)
        inv_det = div(F(1), dot(edge1, uvec))
        orig = sub(oe, v0)
        u = mul(inv_det, dot(orig, uvec))
        vvec = cross(orig, edge1)
        v = mul(inv_det, dot(od, vvec))
        out.u[k], out.v[k], out.t[k] = u, v, mul(inv_det, dot(edge2, vvec))
        w = sub(sub(F(1), u), v)
        bary = lambda a: add(add(mul(a[0], w[:, None]), mul(a[1], u[:, None])), mul(a[2], v[:, None]))
        if geo.normals is not None:             # visibility.wgsl:42-43: mat3(transform), not its inverse transpose
            ni = bary([geo.normals[ids[:, j]] for j in range(3)])
            nrm = np.stack([add(add(mul(T[:, r], ni[:, 0]), mul(T[:, 4 + r], ni[:, 1])), mul(T[:, 8 + r], ni[:, 2])) for r in range(3)], axis=-1)
        else:
            w0, w1, w2 = mat_xyz(T, v0, 1), mat_xyz(T, v1, 1), mat_xyz(T, v2, 1)
            nrm = cross(sub(w1, w0), sub(w2, w0))
            nrm = np.where((dot(nrm, d) > 0)[:, None], -nrm, nrm).astype(F)
        out.words[k, 0] = encode(normalise(nrm))
        if geo.tex_coords is not None:
            out.words[k, 1] = pack_uv(bary([geo.tex_coords[ids[:, j]] for j in range(3)]))
    out.material[k] = (I["material"] & U(0xff)).astype(np.uint8)
    return out


def same_image(got, want):
    """(depth, words, material) against an Image, byte for byte - two NaN depths are equal whatever their payload, and so are two
    NaN halves of the uv word.  -> None, or a description of the first difference."""
    depth, words, material = got
    depth, words, material = _f(depth).reshape(-1), np.asarray(words, U).reshape(-1, 2), np.asarray(material, np.uint8).reshape(-1)
    bad = np.flatnonzero(~((depth.view(U) == want.depth.view(U)) | (np.isnan(depth) & np.isnan(want.depth))))
    if len(bad):
        return ("depth", len(bad), bad[:4].tolist(), depth[bad[:4]].tolist(), want.depth[bad[:4]].tolist())
    bad = np.flatnonzero(words[:, 0] != want.words[:, 0])
    if len(bad):
        return ("normal word", len(bad), bad[:4].tolist(), [hex(int(x)) for x in words[bad[:4], 0]], [hex(int(x)) for x in want.words[bad[:4], 0]])
    for shift in (0, 16):
        a, b = (words[:, 1] >> U(shift)) & U(0xffff), (want.words[:, 1] >> U(shift)) & U(0xffff)
        nan = lambda h: (h & U(0x7fff)) > U(0x7c00)
        bad = np.flatnonzero(~((a == b) | (nan(a) & nan(b))))
        if len(bad):
            return ("uv word, half at bit %d" % shift, len(bad), bad[:4].tolist(), [hex(int(x)) for x in a[bad[:4]]], [hex(int(x)) for x in b[bad[:4]]])
    bad = np.flatnonzero(material != want.material)
    if len(bad):
        return ("material", len(bad), bad[:4].tolist(), material[bad[:4]].tolist(), want.material[bad[:4]].tolist())
    return None


# ---- the seeded case ------------------------------------------------------------------------------------------------------------------

W = H = 64
MATERIALS = (1, 3, 255, 0x105, 2, 0x100)       # by instance index mod 6: receivers, 0x105 -> 5, LIGHT_MATERIAL, and 0x100 -> "no material"


def seeded_scene(oracle):
    """-> (scene arrays, Geometry with both attributes)."""
    def make():
        tl, inst, meshes, bn, verts, idx = cases.case("seeded", oracle).scene
        inst = np.array(inst, dtype=abi.INSTANCE, copy=True)
        inst["material"] = np.asarray(MATERIALS, U)[np.arange(len(inst)) % len(MATERIALS)]
        nv = len(np.asarray(verts).reshape(-1, 3))
        normals = (synth.uniform01(SEED, 0, 3 * nv) * 2.0 - 1.0).astype(F).reshape(nv, 3)
        uvs = (synth.uniform01(SEED, 1, 2 * nv) * 8.0 - 2.0).astype(F).reshape(nv, 2)
        return (tl, inst, meshes, bn, verts, idx), Geometry(inst, meshes, verts, idx, normals, uvs)
    return _once("scene", make)


def seeded(oracle, width=W, height=H):
    """-> (scene, Geometry, camera, oracle's hit records of the twin's rays at width x height)."""
    def make():
        scene, geo = seeded_scene(oracle)
        cam = synth.camera_uniform(**G.CAMERA)
        rec, _ = oracle.trace(scene, rays(cam, width, height), threads=8)
        return scene, geo, cam, np.ascontiguousarray(rec)
    return _once(("seeded", width, height), make)


def seeded_image(oracle, attributes=True, width=W, height=H):
    """The twin's image over the oracle's hits, with both attributes or with neither."""
    def make():
        _, geo, cam, rec = seeded(oracle, width, height)
        return resolve(cam, geo if attributes else geo.without(), rec, width, height)
    return _once(("image", attributes, width, height), make)


# ---- the hand-made case ---------------------------------------------------------------------------------------------------------------

EYE_Z = 5.0
ZNEAR = 0.125


def hand_camera():
    """Every pixel's ray is eye = (0, 0, 5), dir = (0, 0, -1): clip_to_world's columns 0 and 1 are zero, column 2 = (0, 0, 6, 1),
    column 3 = (0, 0, -1, 0).  view = identity; projection: clip.z = ZNEAR * w, clip.w = -z - so a point at z = 0 has clip.w = 0."""
    cam = np.zeros((), dtype=abi.CAMERA)
    c2w = np.zeros(16, F); c2w[10], c2w[11], c2w[14] = 6, 1, -1
    view = np.eye(4, dtype=F).reshape(16)
    proj = np.zeros(16, F); proj[0] = proj[5] = 1; proj[11] = -1; proj[14] = ZNEAR
    cam["clip_to_world"], cam["view"], cam["projection"] = c2w, view, proj
    cam["view_position"] = (0, 0, EYE_Z, 1)
    cam["znear"] = ZNEAR
    return cam


def _instance(transform, inverse, mesh, material):
    i = np.zeros((), dtype=abi.INSTANCE)
    i["transform"], i["inv_transform"] = np.asarray(transform, F).T.reshape(16), np.asarray(inverse, F).T.reshape(16)      # column-major storage
    i["mesh"], i["material"] = mesh, material
    return i


def _translation(x, y, z):
    m = np.eye(4); m[:3, 3] = (x, y, z)
    return m


# uv.x values at the f16 boundaries, each with the bits the round-to-nearest-even convert gives and the bits round-toward-zero would
UV_EDGES = (
    (1.0 + 3 * 2.0 ** -11, 0x3c02, 0x3c01),              # halfway between two halves, the even one above
    (1.0 + 2.0 ** -11 + 2.0 ** -20, 0x3c01, 0x3c00),     # above halfway
    (1.0 + 2.0 ** -11, 0x3c00, 0x3c00),                  # halfway, the even one below
    (65504.0, 0x7bff, 0x7bff), (65519.0, 0x7bff, 0x7bff), (65520.0, 0x7c00, 0x7bff), (1e9, 0x7c00, 0x7bff),
    (2.0 ** -24, 0x0001, 0x0001), (2.0 ** -25, 0x0000, 0x0000), (3 * 2.0 ** -25, 0x0002, 0x0001), (2.0 ** -14 - 2.0 ** -25, 0x0400, 0x03ff),
    (0.0, 0x0000, 0x0000), (-0.0, 0x8000, 0x8000), (np.inf, 0x7c00, 0x7c00), (-np.inf, 0xfc00, 0xfc00), (np.nan, None, None),
)


class HandCase:
    def __init__(self, name, record, branch, **expect):
        self.name, self.record, self.branch, self.expect = name, record, branch, expect


def hand(oracle=None):
    """-> (Geometry, camera, abi.HIT records [N], [HandCase]): an N x 1 image, one record per case."""
    def make():
        tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
        # mesh 0: one triangle per attribute set, all over the same positions, behind two unused vertices and three unused indices
        attrs = []                                   # (three normals, three uvs)

        def corner(a):                              # (a, z, z) with z the zero of a's sign: with u = v = 0 it interpolates to a exactly
            z = np.where(np.isnan(a), 0.0, np.copysign(0.0, np.where(np.isnan(a), 0.0, a)))
            return np.stack([a, z, z])

        def attr(n0=(0, 0, 1), uv0=(0.25, 0.5), all_normals=None):
            attrs.append((np.asarray(all_normals, float) if all_normals is not None else corner(np.asarray(n0, float)), corner(np.asarray(uv0, float))))
            return len(attrs) - 1
        T_PLAIN = attr()
        T_ZERO = attr(all_normals=[(2, 0, 0), (-2, 0, 0), (0, 0, 0)])       # at u = 1/4, v = 1/2: 2 * 1/4 - 2 * 1/4 + 0 = 0 exactly
        T_SKEW = attr(n0=(0, 1, 1))
        T_SOUTH = attr(n0=(0, 0, -1))
        T_X0 = attr(n0=(0, 0.5, -0.5))
        T_Y0 = attr(n0=(-0.5, 0, -0.5))
        T_UV = [attr(uv0=(e[0], -e[0])) for e in UV_EDGES]
        K = len(attrs)
        n_vertices = 2 + 3 * K
        vertices = np.concatenate([np.full((2, 3), 77, F)] + [tri] * K)
        normals = np.concatenate([np.full((2, 3), 77, F)] + [a[0].astype(F) for a in attrs])
        uvs = np.concatenate([np.full((2, 2), 77, F)] + [a[1].astype(F) for a in attrs])
        idx0 = np.arange(3 * K, dtype=U)
        # mesh 2: three triangles with one vertex id each at n_vertices, the first that is out of range; mesh 3: vertex_offset -1
        # under index 0 wraps to 0xffffffff
        idx2 = np.array([n_vertices, 0, 1, 0, n_vertices, 1, 0, 1, n_vertices], U)
        idx3 = np.array([1, 2, 0], U)
        indices = np.concatenate([np.zeros(3, U), idx0, idx2, idx3])
        meshes = np.zeros(4, dtype=abi.MESH_INFO)
        meshes["index_count"] = (3 * K, 3, 9, 3)
        meshes["base_index"] = (3, len(indices) - 2, 3 + 3 * K, 3 + 3 * K + 9)     # mesh 1: its triangle's last index is the first beyond the buffer
        meshes["vertex_offset"] = (2, 0, 0, -1)
        eye4 = np.eye(4)
        inst = np.stack([
            _instance(eye4, eye4, 0, 1),                                                     # 0: u = v = 0, t = 5: clip.w = 0
            _instance(_translation(-0.25, -0.5, 1), _translation(0.25, 0.5, -1), 0, 7),      # 1: u = 1/4, v = 1/2, t = 4
            _instance(np.diag([-1.0, 1, 1, 1]), np.diag([-1.0, 1, 1, 1]), 0, 9),              # 2: mirrored in x
            _instance(_translation(0, 0, 1) @ np.diag([1.0, 4, 1, 1]), np.diag([1.0, 0.25, 1, 1]) @ _translation(0, 0, -1), 0, 255),      # 3: y scaled by 4
            _instance(_translation(0, 0, 1), _translation(0, 0, -1), 0, 256),                 # 4: material 256
            _instance(_translation(0, 0, 1), _translation(0, 0, -1), 0, 0x1ff),               # 5: material 0x1ff
            _instance(eye4, eye4, 4, 1),                                                     # 6: its mesh is the first beyond the table
            _instance(eye4, eye4, 1, 1), _instance(eye4, eye4, 2, 1), _instance(eye4, eye4, 3, 1),      # 7, 8, 9: meshes 1, 2, 3
        ])
        geo = Geometry(inst, meshes, vertices, indices, normals, uvs)
        C = []

        def case(name, dist, hit, instance, triangle, branch, **expect):
            r = np.zeros((), dtype=abi.HIT)
            r["dist"], r["hit"], r["instance"], r["triangle"] = dist, hit, instance, triangle
            C.append(HandCase(name, r, branch, **expect))
        case("hit == 0", 4, 0, 1, T_PLAIN, NO_HIT)
        case("hit == 2", 4, 2, 1, T_PLAIN, NO_HIT)
        case("the miss record of the walk", 1e30, 0, 0xffffffff, 0xffffffff, NO_HIT)
        case("instance == n_instances", 4, 1, len(inst), T_PLAIN, BAD_INSTANCE)
        case("instance 0xffffffff", 4, 1, 0xffffffff, T_PLAIN, BAD_INSTANCE)
        case("mesh >= n_meshes", 4, 1, 6, 0, BAD_MESH)
        case("triangle == the mesh's count", 4, 1, 1, K, BAD_TRIANGLE)
        case("3 * triangle + 2 wraps to 1 in 32 bits", 4, 1, 1, 0x55555555, BAD_TRIANGLE)
        case("the triangle's last index is n_indices", 5, 1, 7, 0, BAD_INDEX)
        for k in range(3):
            case(f"vertex id {k} == n_vertices", 5, 1, 8, k, BAD_VERTEX)
        case("vertex_offset -1 under index 0", 5, 1, 9, 0, BAD_VERTEX)
        case("plain hit, u = 1/4, v = 1/2", 4, 1, 1, T_PLAIN, HIT, u=0.25, v=0.5, material=7, geometric=0x80008000)
        case("clip.w == 0", 5, 1, 0, T_PLAIN, HIT, u=0.0, v=0.0, material=1, depth_not_finite=True, word0=0x80008000)
        case("mirrored instance: the geometric normal is flipped toward the eye", 5, 1, 2, T_PLAIN, HIT, geometric=0x80008000, material=9, depth_not_finite=True)
        case("y scaled by 4: mat3(transform), not the inverse transpose", 4, 1, 3, T_SKEW, HIT, material=255, skew=True)
        case("vertex normals that interpolate to zero", 4, 1, 1, T_ZERO, HIT, word0=0)
        case("normal (0, 0, -1)", 4, 1, 4, T_SOUTH, HIT, word0=0xffffffff, material=0)
        case("normal z < 0, x == 0", 4, 1, 5, T_X0, HIT, x_code=0xbfff, y_code=0xffff, material=255)
        case("normal z < 0, y == 0", 4, 1, 5, T_Y0, HIT, x_code=0x0000, y_code=0xbfff, material=255)
        for e, t in zip(UV_EDGES, T_UV):
            case(f"uv {e[0]!r}", 4, 1, 5, t, HIT, uv=e, u=0.0, v=0.0)
        return geo, hand_camera(), np.stack([c.record for c in C]), C
    return _once("hand", make)
