"""A plain float64 renderer of the whole shading chain - scene + camera -> G-buffer -> light bits -> lit image - written from the
reference's shader text and from nothing else: no BVH, no twin code, no float32 arithmetic.  Shared by tests/test_frame_reference.py
(CPU: the float32 twins of tests/*_cases.py against it) and tests/test_gpu_frame.py (the device's own outputs against it); a helper
module, no tests in it.  Of this project it imports the array dtypes of voidin_amd.abi only.

Every stage works per pixel (or per receiver) over every instance x triangle.  The shortcuts, all conservative and all in float64:
a ray is not tested against an instance whose padded world box (the corners of its mesh's vertex box through `transform`, grown by
a thousandth of its diagonal) its half-line t >= 0 does not meet, nor against a run of 128 consecutive triangles of the mesh whose
padded box the instance-space ray does not meet (a flat list of boxes, no hierarchy); the triangle tests that remain are filtered
on det and u in a rearranged (matrix product) form with a slack of 5 % before the survivors are evaluated in the reference's own
expressions.  Both ray ranges are answered from the same tests: the segment's end t < 1 is applied when the answer is asked for.

Matrices are stored column-major (16 floats, [column][row]), as the reference's mat4x4<f32>; _mat() gives the mathematical matrix.

ROBUST FLAGS.  The float32 chain under test cannot be expected to agree with float64 on a ray that grazes a triangle's edge.  What
"grazes" means is decided here, from float64 values alone: with `margin` the distance the ray's origin may be off (the callers pass
8 * delta, delta = the largest |float64 pos - float32 pos| that decode() saw), a triangle test is BORDERLINE for a ray when moving
the origin by `margin` could change its acceptance in first order - see _triangle_tests, where each margin stands next to the rule
it mirrors."""
import numpy as np

from voidin_amd import abi

D = np.float64
NO_MATERIAL, LIGHT_MATERIAL = 0, 2          # raytraced_shadows.wgsl:80-85
DET_MIN = 1e-10                             # intersections.wgsl:30
BIAS = 0.0001                               # raytraced_shadows.wgsl:98
RUN = 128                                   # triangles in a run of the second filter
assert abi.INSTANCE.itemsize == 144 and abi.LIGHT.itemsize == 32


def _mat(a):
    """16 floats, column-major -> the 4 x 4 matrix M (float64) with M @ column vector."""
    return np.asarray(a, D).reshape(4, 4).T


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


# ---- the pixel ray ---------------------------------------------------------------------------------------------------------------

def pixel_rays(cam, w, h):
    """src/bin/bvh_trace.wgsl:223-231 at the pixel centre, the y of shaders/utils/uv.wgsl:13-15 -> (eye [N][3], dir [N][3]).
    The harness's in.uv * 2 - 1 is the clip position of the fragment (its vs_main writes pos = 2 * uv - 1), whose y points UP
    while pixel rows count DOWN: ndc.y = (1 - uv.y) * 2 - 1 with uv the pixel centre over the size (uv.wgsl:1-3)."""
    M = _mat(cam["clip_to_world"])
    i = np.arange(w * h)
    ux, uy = ((i % w) + 0.5) / w, ((i // w) + 0.5) / h
    nx, ny = ux * 2.0 - 1.0, (1.0 - uy) * 2.0 - 1.0
    one, zero = np.ones_like(nx), np.zeros_like(nx)
    with np.errstate(all="ignore"):
        view_pos = M @ np.stack([nx, ny, one, one])           # :227
        view_dir = M @ np.stack([nx, ny, zero, one])          # :228
        eye = (view_pos[:3] / view_pos[3]).T                  # :230
        d = view_dir[:3].T
        return eye, d / _norm(d)[:, None]                     # :231


# ---- every instance x triangle ------------------------------------------------------------------------------------------------------

class _Scene:
    """The arrays of a trace scene as float64 triangles: per mesh the corners [T][3][3] and vertex ids [T][3] (bvh.wgsl:30-33,
    the indices as they are stored), per instance the two matrices and the padded world box."""

    def __init__(self, scene):
        _, inst, meshes, _, verts, idx = scene
        verts, idx = np.asarray(verts, D).reshape(-1, 3), np.asarray(idx, np.uint32).reshape(-1)
        self.inst, self.meshes, self.verts = inst, meshes, verts
        self.ids, self.tris = [], []
        for m in meshes:
            n = int(m["index_count"]) // 3
            ids = idx[int(m["base_index"]): int(m["base_index"]) + 3 * n].astype(np.int64).reshape(n, 3) + int(np.uint32(m["vertex_offset"]))
            self.ids.append(ids)
            self.tris.append(verts[ids])
        self.runs = []                                        # per mesh: runs of RUN consecutive triangles and their boxes [K][3]
        for t in self.tris:
            starts = np.arange(0, max(len(t), 1), RUN)
            lo = np.array([t[a: a + RUN].reshape(-1, 3).min(axis=0) for a in starts]) if len(t) else np.zeros((1, 3))
            hi = np.array([t[a: a + RUN].reshape(-1, 3).max(axis=0) for a in starts]) if len(t) else np.zeros((1, 3))
            pad = 1e-3 * _norm(hi - lo)[:, None] + 1e-6
            self.runs.append((starts, lo - pad, hi + pad))
        self.T = [_mat(i["transform"]) for i in inst]
        self.Ti = [_mat(i["inv_transform"]) for i in inst]
        lo, hi = [], []
        for k, i in enumerate(inst):
            t = self.tris[int(i["mesh"])].reshape(-1, 3)
            a, b = t.min(axis=0), t.max(axis=0)
            corners = np.array([[(a, b)[(c >> j) & 1][j] for j in range(3)] for c in range(8)])
            wc = corners @ self.T[k][:3, :3].T + self.T[k][:3, 3]
            pad = 1e-3 * np.linalg.norm(wc.max(axis=0) - wc.min(axis=0)) + 1e-6
            lo.append(wc.min(axis=0) - pad)
            hi.append(wc.max(axis=0) + pad)
        self.lo, self.hi = np.array(lo), np.array(hi)

    def meets_box(self, eye, d):
        """bool [R][I]: the half-line t >= 0 of the ray meets the padded world box of the instance."""
        return _meets(eye, d, self.lo, self.hi, 0.0)


def _meets(eye, d, lo, hi, grow):
    """bool [R][B]: the half-line t >= 0 of each ray meets each box [B][3] grown by `grow` (the slab test, in float64)."""
    with np.errstate(all="ignore"):
        lo, hi = lo[None] - grow, hi[None] + grow
        inv = 1.0 / d[:, None, :]
        a, b = (lo - eye[:, None, :]) * inv, (hi - eye[:, None, :]) * inv
        flat = d[:, None, :] == 0                             # parallel to the slab: inside it or not
        inside = (eye[:, None, :] >= lo) & (eye[:, None, :] <= hi)
        near = np.where(flat, np.where(inside, -np.inf, np.inf), np.minimum(a, b)).max(axis=2)
        far = np.where(flat, np.where(inside, np.inf, -np.inf), np.maximum(a, b)).min(axis=2)
        return (far >= near) & (far >= 0)


class Tests:
    """The triangle tests of a set of rays that were accepted or borderline, as flat arrays: ray, instance, triangle, t, u, v, and
    `accepted` (the reference's rule), `strict` (accepted whatever the origin does within the margin), `loose` (acceptable for some
    origin within it).  borderline = loose & ~strict."""

    def __init__(self, parts, n_rays):
        cat = lambda k, dt: np.concatenate([p[k] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
        self.ray, self.inst, self.tri = cat(0, np.int64), cat(1, np.int64), cat(2, np.int64)
        self.t, self.u, self.v, self.dt = cat(3, D), cat(4, D), cat(5, D), cat(6, D)
        self.accepted, self.strict, self.loose = cat(7, bool), cat(8, bool), cat(9, bool)
        self.n_rays = n_rays

    def any_hit(self, t_hi=None):
        """-> (answer [R], robust [R]) over the half-line t > 0, or over the open segment 0 < t < t_hi (the ray range: margin m_t at
        that end too): robust if some triangle is accepted and not borderline, or none is accepted or borderline."""
        accepted, strict, loose = self.accepted, self.strict, self.loose
        if t_hi is not None:
            accepted, strict = accepted & (self.t < t_hi), strict & (self.t + self.dt < t_hi)
            loose = (loose & (self.t - self.dt < t_hi)) | accepted
            strict = strict & accepted
        count = lambda m: np.bincount(self.ray[m], minlength=self.n_rays)
        return count(accepted) > 0, (count(strict) > 0) | (count(loose) == 0)

    def closest(self):
        """-> (row of the nearest accepted test per ray, -1: none; robust [R]): robust if the nearest accepted triangle is not
        borderline and nearer than every other acceptable one by the two margins of t - or if nothing is accepted or borderline."""
        first = np.full(self.n_rays, -1, np.int64)
        rows = np.flatnonzero(self.accepted)
        order = rows[np.lexsort((self.t[rows], self.ray[rows]))]
        r, at = np.unique(self.ray[order], return_index=True)
        first[r] = order[at]
        robust = np.bincount(self.ray[self.loose], minlength=self.n_rays) == 0
        robust[r] = self.strict[first[r]]
        rival = np.flatnonzero(self.loose)
        own = first[self.ray[rival]]
        keep = (own >= 0) & (own != rival)
        rival, own = rival[keep], own[keep]
        close = self.t[rival] - self.dt[rival] <= self.t[own] + self.dt[own]
        robust[self.ray[rival[close]]] = False
        return first, robust


def _triangle_tests(sc, eye, d, margin, dir_moves):
    """intersect_trig (shaders/utils/intersections.wgsl:25-45) of every ray with every triangle of every instance, on the
    instance-space ray of instance_intersect (shaders/utils/bvh.wgsl:78-87: eye and dir through inv_transform, the direction NOT
    renormalised, so t is the world ray's parameter) over the half-line t > 0 -> Tests.
    dir_moves: the direction is `target - origin` (a shadow ray), so it moves against the origin."""
    R = len(eye)
    parts = []
    meets = sc.meets_box(eye, d)
    for i in range(len(sc.inst)):
        sel = np.flatnonzero(meets[:, i])
        if not len(sel):
            continue
        m = int(sc.inst[i]["mesh"])
        Ti = sc.Ti[i]
        oe = eye[sel] @ Ti[:3, :3].T + Ti[:3, 3]              # bvh.wgsl:82
        od = d[sel] @ Ti[:3, :3].T                            # bvh.wgsl:83
        eo = margin * np.linalg.norm(Ti[:3, :3], 2)           # how far the instance-space origin moves
        ed = eo if dir_moves else 0.0                         # ... and the direction
        starts, run_lo, run_hi = sc.runs[m]
        in_run = _meets(oe, od, run_lo, run_hi, eo)
        lo_, ld_ = _norm(oe), _norm(od)
        for a, hits_run in zip(starts, in_run.T):
            rows = np.flatnonzero(hits_run)
            if not len(rows):
                continue
            tri = sc.tris[m][a: a + RUN]
            v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
            n = np.cross(e1, e2)
            ln, le2 = _norm(n), _norm(e2)
            s_, o_, d_ = sel[rows], oe[rows], od[rows]
            with np.errstate(all="ignore"):
                # the filter: det = -dir . (e1 x e2) and u * det = (oe x dir) . e2 - dir . (e2 x v0) as matrix products, u within
                # [-0.05, 1.05] widened by a bound of its margin
                det_f = -(d_ @ n.T)
                x = np.cross(o_, d_) @ e2.T
                x -= d_ @ np.cross(e2, v0).T
                x -= 0.5 * det_f
                np.abs(x, out=x)
                lim = np.abs(det_f)
                lim *= 0.55
                lim += np.outer(eo * ld_[rows] + ed * (lo_[rows] + _norm(v0).max()) + 1e-9 * lo_[rows] * ld_[rows], le2)
                lim += (1.05 * ed * ln)[None]
                ok = x <= lim
                ok &= det_f >= (DET_MIN - ed * ln - 1e-12)[None]
                r, k = np.nonzero(ok)
            if not len(r):
                continue
            k_all = k + a
            # the reference's expressions on the survivors (flat)
            with np.errstate(all="ignore"):
                ray_eye, ray_dir = o_[r], d_[r]
                edge1, edge2 = e1[k], e2[k]                   # :26-27
                uvec = np.cross(ray_dir, edge2)               # :28
                det = _dot(edge1, uvec)                       # :29
                inv_det = 1.0 / det                           # :31
                orig = ray_eye - v0[k]                        # :32
                u = inv_det * _dot(orig, uvec)                # :33
                vvec = np.cross(orig, edge1)                  # :35
                v = inv_det * _dot(ray_dir, vvec)             # :36
                t = inv_det * _dot(edge2, vvec)               # :38
                # first-order margins: det = -dir . (e1 x e2) moves with the direction only; u = orig . uvec / det with the origin
                # (|uvec|), the direction (|orig| |edge2|) and det; v = orig . (edge1 x dir) / det likewise; t = orig . (e1 x e2) / det
                # with the origin and det
                m_det = ed * ln[k]
                ad = np.abs(det)
                m_u = (eo * _norm(uvec) + ed * _norm(orig) * le2[k] + np.abs(u) * m_det) / ad
                m_v = (eo * _norm(np.cross(edge1, ray_dir)) + ed * _norm(vvec) + np.abs(v) * m_det) / ad
                m_t = (eo * ln[k] + np.abs(t) * m_det) / ad
                accepted = ~(det < DET_MIN)                   # :30   margin m_det
                strict = det - m_det >= DET_MIN
                loose = det + m_det >= DET_MIN
                accepted &= ~((u < 0.0) | (1.0 < u))          # :34   margin m_u, at both ends
                strict &= (u - m_u >= 0.0) & (u + m_u <= 1.0)
                loose &= (u + m_u >= 0.0) & (u - m_u <= 1.0)
                accepted &= ~((v < 0.0) | (u + v > 1.0))      # :37   margins m_v, and m_u + m_v for the sum
                strict &= (v - m_v >= 0.0) & (u + v + m_u + m_v <= 1.0)
                loose &= (v + m_v >= 0.0) & (u + v - m_u - m_v <= 1.0)
                accepted &= t > 0.0                           # :39   margin m_t (`t < *hit` is the closest-hit bookkeeping)
                strict &= t - m_t > 0.0
                loose &= t + m_t > 0.0
                loose |= accepted                             # (a NaN margin excludes nothing that is accepted)
                strict &= accepted
            keep = np.flatnonzero(loose)
            parts.append((s_[r[keep]], np.full(len(keep), i), k_all[keep], t[keep], u[keep], v[keep], m_t[keep], accepted[keep], strict[keep], loose[keep]))
    return Tests(parts, R)


# ---- stage 1: primary rays -> the exact G-buffer ------------------------------------------------------------------------------------

class Primary:
    """Per pixel: hit, instance, triangle, t, u, v, depth, normal [N][3], uv [N][2], material, robust."""


def primary(scene, geometry, cam, w, h, margin=0.0):
    """scene: the six arrays of a trace scene; geometry: .normals [V][3] / .tex_coords [V][2] or None (the header's two modes:
    interpolated through mat3(transform), or geometric and facing the eye); margin: see the module's docstring."""
    sc = scene if isinstance(scene, _Scene) else _Scene(scene)
    eye, d = pixel_rays(cam, w, h)
    tests = _triangle_tests(sc, eye, d, margin, False)
    first, robust = tests.closest()
    n = w * h
    out = Primary()
    out.hit, out.robust = first >= 0, robust
    k = np.flatnonzero(out.hit)
    row = first[k]
    out.instance, out.triangle = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    out.t, out.u, out.v, out.depth = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    out.normal, out.uv, out.material = np.zeros((n, 3)), np.zeros((n, 2)), np.zeros(n, np.int64)
    out.instance[k], out.triangle[k] = tests.inst[row], tests.tri[row]
    out.t[k], out.u[k], out.v[k] = tests.t[row], tests.u[row], tests.v[row]
    out.eye, out.dir = eye, d
    if not len(k):
        return out
    # shaders/visibility.wgsl:35-40: clip = proj * (view * world_pos); the depth attachment holds clip.z / clip.w
    p = eye[k] + d[k] * out.t[k][:, None]
    PV = _mat(cam["projection"]) @ _mat(cam["view"])
    clip = PV @ np.concatenate([p, np.ones((len(k), 1))], axis=1).T
    with np.errstate(all="ignore"):
        out.depth[k] = clip[2] / clip[3]
    ids = np.stack([sc.ids[int(sc.inst[i]["mesh"])][t] for i, t in zip(out.instance[k], out.triangle[k])])
    Tm = np.stack([sc.T[i][:3, :3] for i in out.instance[k]])
    u, v = out.u[k][:, None], out.v[k][:, None]
    bary = lambda a: a[ids[:, 0]] * (1.0 - u - v) + a[ids[:, 1]] * u + a[ids[:, 2]] * v      # the rasteriser's interpolation
    with np.errstate(all="ignore"):
        if geometry.normals is not None:                      # visibility.wgsl:42-43, 79: normalize(mat3(transform) * normal)
            nrm = np.einsum("nij,nj->ni", Tm, bary(np.asarray(geometry.normals, D).reshape(-1, 3)))
        else:                                                 # bvh_trace.wgsl:238: the triangle's normal, in world space, facing the eye
            verts = sc.verts
            Tt = np.stack([sc.T[i][:3, 3] for i in out.instance[k]])
            wv = [np.einsum("nij,nj->ni", Tm, verts[ids[:, j]]) + Tt for j in range(3)]
            nrm = np.cross(wv[1] - wv[0], wv[2] - wv[0])
            nrm = np.where((_dot(nrm, d[k]) > 0)[:, None], -nrm, nrm)
        out.normal[k] = nrm / _norm(nrm)[:, None]
    if geometry.tex_coords is not None:                       # visibility.wgsl:47
        out.uv[k] = bary(np.asarray(geometry.tex_coords, D).reshape(-1, 2))
    out.material[k] = np.asarray([int(sc.inst[i]["material"]) & 0xff for i in out.instance[k]])      # the R8Uint attachment
    return out


# ---- stage 2: the stored G-buffer -> pos and nor --------------------------------------------------------------------------------------

def decode_normal(word):
    """decode_octahedral_32 (shaders/utils/encoding.wgsl:17-28) -> [N][3]."""
    word = np.asarray(word, np.uint32)
    mu = 65535.0
    vx, vy = (word & np.uint32(0xffff)).astype(D) / mu, (word >> np.uint32(16)).astype(D) / mu      # :19-20
    vx, vy = vx * 2.0 - 1.0, vy * 2.0 - 1.0                   # :22
    nz = 1.0 - np.abs(vx) - np.abs(vy)                        # :23
    t = np.maximum(-nz, 0.0)                                  # :24
    nx = vx + np.where(vx > 0.0, -t, t)                       # :25
    ny = vy + np.where(vy > 0.0, -t, t)                       # :26
    n = np.stack([nx, ny, nz], axis=1)
    with np.errstate(all="ignore"):
        return n / _norm(n)[:, None]                          # :27


def encode_normal_exact(n):
    """encode_octahedral_32 (encoding.wgsl:4-15) up to the quantisation: the two coordinates in [0, 65535] BEFORE floor(. + 0.5)
    -> [N][2].  (sign(0) never matters here: a normal with z < 0 and x or y exactly 0 does not come out of float64 arithmetic.)"""
    n = np.asarray(n, D)
    with np.errstate(all="ignore"):
        q = n / np.abs(n).sum(axis=1)[:, None]
        fold = q[:, 2] < 0.0
        x = np.where(fold, (1.0 - np.abs(q[:, 1])) * np.sign(q[:, 0]), q[:, 0])
        y = np.where(fold, (1.0 - np.abs(q[:, 0])) * np.sign(q[:, 1]), q[:, 1])
        return np.stack([(x * 0.5 + 0.5) * 65535.0, (y * 0.5 + 0.5) * 65535.0], axis=1)


def decode(depth, words, cam, w, h, at=None, pos32=None):
    """world_position_from_depth (shaders/utils/uv.wgsl:13-22) at the pixel centre (uv.wgsl:1-3) and decode_octahedral_32 of the STORED
    values - float32 depth, the normal word - in float64 arithmetic -> (pos [K][3], nor [K][3], delta) for the pixels `at` (default:
    all).  delta: the largest |pos - pos32| over the finite rows when the float32 path's positions are given, else None."""
    at = np.arange(w * h) if at is None else np.asarray(at)
    depth, words = np.asarray(depth, np.float32).reshape(-1)[at].astype(D), np.asarray(words, np.uint32).reshape(w * h, -1)[at, 0]
    M = _mat(cam["clip_to_world"])
    ux, uy = ((at % w) + 0.5) / w, ((at // w) + 0.5) / h
    clip = np.stack([ux * 2.0 - 1.0, (1.0 - uy) * 2.0 - 1.0, depth, np.ones(len(at))])      # :14, :18
    with np.errstate(all="ignore"):
        world_w = M @ clip                                    # :19
        pos = (world_w[:3] / world_w[3]).T                    # :21
    delta = None
    if pos32 is not None:
        diff = np.abs(pos - np.asarray(pos32, D))
        diff = diff[np.isfinite(diff).all(axis=1)]
        delta = float(diff.max()) if diff.size else 0.0
    return pos, decode_normal(words), delta


# ---- stage 3: the light bits ----------------------------------------------------------------------------------------------------------

class Bits:
    """bool [P][L]: in_range, occluded (meaningful where in range), robust_in, robust_occ."""


def light_bits(pos, nor, scene, lights, ray_range, margin=0.0, shared=None):
    """src/bin/raytraced_shadows.wgsl:93-102 per (receiver, light): dist - radius > 0 skips the light; the shadow ray starts at
    pos + nor * 0.0001 and its direction is light_vec = light - pos, not normalised, so t = 1 is the light.  The reference's
    traverse_tlas walks t > 0; with the ray range on the walk ends at the light: 0 < t < 1.  Rays are traced for the pairs in
    range only.  shared: a dict in which the triangle tests are kept for a second call with the other ray_range."""
    sc = scene if isinstance(scene, _Scene) else _Scene(scene)
    pos, nor = np.asarray(pos, D), np.asarray(nor, D)
    P, L = len(pos), len(lights)
    out = Bits()
    with np.errstate(all="ignore"):
        light_vec = np.asarray(lights["position"], D)[None, :, :] - pos[:, None, :]      # :93
        dist = _norm(light_vec)                                                         # :94
        gap = dist - np.asarray(lights["radius"], D)[None, :]
        out.in_range = ~(gap > 0.0)                                                     # :95
        out.robust_in = ~(np.abs(gap) <= margin)              # the rule's only bound; a NaN gap is in range on both sides
    out.dist = dist
    out.occluded = np.zeros((P, L), bool)
    out.robust_occ = np.ones((P, L), bool)
    p, l = np.nonzero(out.in_range & np.isfinite(pos).all(axis=1)[:, None] & np.isfinite(nor).all(axis=1)[:, None])
    if len(p):
        origin = pos[p] + nor[p] * BIAS                                                 # :98
        shared = {} if shared is None else shared
        if "tests" not in shared:
            shared["tests"] = _triangle_tests(sc, origin, light_vec[p, l], margin, True)
        out.occluded[p, l], out.robust_occ[p, l] = shared["tests"].any_hit(1.0 if ray_range else None)      # :99-102
    return out


# ---- stage 4: the light loop -----------------------------------------------------------------------------------------------------------

def attenuation(dist, radius):
    """raytraced_shadows.wgsl:48-55 with max_intensity = falloff = 1 (:104)."""
    with np.errstate(all="ignore"):
        s = dist / radius
        s2 = s * s
        return np.where(s >= 1.0, 0.0, (1.0 - s2) ** 2 / (1.0 + s2))


def shade(pos, nor, material, table, lights, in_range_bits, occluded_bits, eye):
    """src/bin/raytraced_shadows.wgsl:73-118 with the bits GIVEN (bool [N][L]) in place of the range test and the walk, the
    material table's rows in place of the textures (albedo, metallic_roughness.z = specular, emissive) -> (rgba [N][4], S [N][3]):
    S = |base| + the sum over the visited lights of |(diff + spec) * occlusion * atten| per channel."""
    pos, nor, material = np.asarray(pos, D), np.asarray(nor, D), np.asarray(material).reshape(-1).astype(np.int64)
    M = np.asarray(table)[material]
    albedo, specular, emissive = M["albedo"].astype(D), M["specular"].astype(D), M["emissive"].astype(D)
    n = len(pos)
    with np.errstate(all="ignore"):
        rd = np.asarray(eye, D).reshape(-1)[None, :3] - pos
        rd = rd / _norm(rd)[:, None]                                                    # :75
        color = albedo * 0.3 + emissive                                                 # :79
        is_light = material == LIGHT_MATERIAL
        color[is_light] = (albedo + emissive)[is_light]                                 # :83-85
        S = np.abs(color)
        covr = np.maximum(0.0, _dot(-rd, nor))                                          # :111
        for i in range(len(lights)):                                                    # :88, ascending
            visit = in_range_bits[:, i] & ~is_light & (material != NO_MATERIAL)         # :89, :95
            at = np.flatnonzero(visit)
            if not len(at):
                continue
            light_vec = np.asarray(lights["position"][i], D)[None, :] - pos[at]         # :93
            dist = _norm(light_vec)                                                     # :94
            occlusion = np.where(occluded_bits[at, i], 0.5, 1.0)                        # :97-102
            atten = attenuation(dist, D(lights["radius"][i]))                           # :104
            light_dir = light_vec / dist[:, None]                                       # :106
            shd = np.maximum(0.0, _dot(nor[at], light_dir))                             # :107
            lc = np.asarray(lights["color"][i], D)[None, :]
            diff = lc * albedo[at] * shd[:, None]                                       # :108
            spec = lc * specular[at][:, None] * (covr[at] ** 16)[:, None]               # :112
            term = (diff + spec) * occlusion[:, None] * atten[:, None]                  # :114
            color[at] += term
            S[at] += np.abs(term)
        out = np.ones((n, 4))
        out[:, :3] = np.where(color > 0.0, color, 0.0)                                  # :117 (a NaN leaves as 0)
        out[material == NO_MATERIAL] = (1.0, 0.0, 1.0, 1.0)                             # :80-82
    return out, S
