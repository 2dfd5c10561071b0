"""Scenes, intervals and the expected records of the ray-interval tests (VD_OPT_TRACE_RAY_RANGE: include/voidin_abi.h, "Ray intervals").
Shared by tests/test_trace_range_cases.py (CPU: the restatement is checked against the oracle, the classes are populated) and
tests/test_gpu_trace_range.py; a helper module, no tests in it.

The oracle walks the half-line t > 0 and is not edited, so the expected records of an interval come from a BRUTE FORCE: for every
ray, every instance and every triangle of its mesh, the instance-space ray (the `inv_transform` rows as oracle/np_restate.py's
trace takes them) and the Moeller-Trumbore t in float32 with the operation order of np_restate._tri, vectorised over rays.
Every accepted (t, instance, triangle) with 0 < t < 1e30 is kept, sorted per ray; the answer of an interval is the minimum t
with t_lo < t < t_hi.  The brute force knows no visit order, so of a record `dist` and `hit` are always expected bit for bit and
`instance` / `triangle` only where exactly one triangle attains the minimum (Expected.unique).

The only shortcut: a ray is not tested against an instance whose mesh it cannot reach - the distance, in float64, from the centre
of the mesh's vertex box to the instance-space line exceeds the box's half diagonal by more than a thousandth of it.  Every
triangle lies inside that box, so nothing a ray truly intersects is dropped (rays with a zero or non-finite direction skip the
shortcut)."""
import numpy as np

from chain_scenes import chain_rays, chain_scene
from conftest import golden
from voidin_amd import abi, synth

F = np.float32
MAX_DIST = F(1e30)
NONE = np.uint32(0xFFFFFFFF)
SEED = synth.SEED_BASE + 20


# ---- scenes -------------------------------------------------------------------------------------------------------------------

def _golden_scene():
    g = golden("trace_40.npz")
    return (g["tlas"], g["instances"], g["meshes"], g["bvh_nodes"], g["vertices"], g["indices"]), g["rays"].copy()


def _seeded_scene(oracle):
    """300 instances of three meshes (vertex_offset / base_index / bvh_index all non-zero), 64 x 64 primary rays."""
    meshes_src = [synth.uv_sphere(1.0, 4), synth.knot_mesh(96, 24), synth.triangle_soup(64)]
    V, I, B = [], [], []
    infos = np.zeros(len(meshes_src), dtype=abi.MESH_INFO)
    vo = bo = no = 0
    for k, (v, i) in enumerate(meshes_src):
        v = np.asarray(v, F).reshape(-1, 3)
        nodes, idx = oracle.bvh_build(v, i)
        infos[k]["min"], infos[k]["max"] = synth.mesh_bounds(v)
        infos[k]["index_count"], infos[k]["base_index"] = len(idx), bo
        infos[k]["vertex_offset"], infos[k]["bvh_index"] = vo, no
        V.append(v); I.append(idx); B.append(nodes)
        vo += len(v); bo += len(idx); no += len(nodes)
    inst = synth.instances(300, n_mesh=3, seed=synth.SEED_BASE + 18, extent=50.0, scale_range=(0.5, 3.0))
    tl = oracle.tlas_build(inst, infos)
    rays = synth.primary_rays(synth.camera_uniform(eye=(0, 2.5, 40), pitch_deg=0), 64, 64)
    return (tl, inst, infos, np.concatenate(B), np.concatenate(V), np.concatenate(I).astype(np.uint32)), rays


def _chain(oracle):
    """200 spheres behind one another: a ray along +x holds 199 pending entries when it reaches the first - more than the 128 a
    lane keeps - and one from the far end, or one that leaves at once, holds next to none."""
    rays, _, _ = chain_rays(768, far_x=250.0, seed=SEED + 1)
    return chain_scene(oracle, 200), rays


def shadow_scene(oracle):
    """What the option is for: two unit spheres, a light at L = (0, 5, 0) and two points with their normals.  Point 0 lies next to
    the origin (off the sphere's axis: the pole is a vertex): nothing lies between it and the light, and sphere 0 (centre
    (0, 10, 0)) lies on the same line BEHIND the light, at t = 1.8 of the shadow ray (t = 1 is the light).  Point 1 = (20, 0, 0): sphere 1 sits halfway between it and the light.
    -> (scene, positions, normals, light)."""
    v, i = synth.uv_sphere(1.0, 8)
    v = np.asarray(v, F).reshape(-1, 3)
    nodes, idx = oracle.bvh_build(v, i)
    infos = np.zeros(1, dtype=abi.MESH_INFO)
    infos[0]["min"], infos[0]["max"] = synth.mesh_bounds(v)
    infos[0]["index_count"] = len(idx)
    inst = np.zeros(2, dtype=abi.INSTANCE)
    for k, c in enumerate(((0.0, 10.0, 0.0), (10.0, 2.5, 0.0))):
        T = np.eye(4, dtype=F); T[3, :3] = c                # column-major storage: translation in elements 12..14
        Ti = np.eye(4, dtype=F); Ti[3, :3] = -np.asarray(c, F)
        inst[k]["transform"], inst[k]["inv_transform"] = T.reshape(16), Ti.reshape(16)
    scene = (oracle.tlas_build(inst, infos), inst, infos, nodes, v, np.asarray(idx, np.uint32))
    pos = np.array([[0.2, 0, 0.1], [20, 0, 0]], F)
    nor = np.array([[0, 1, 0], [0, 1, 0]], F)
    return scene, pos, nor, np.array([0, 5, 0], F)


_CACHE = {}
NAMES = ("golden", "seeded", "chain")


class Case:
    """One scene with its rays: the oracle's records over the half-line (`want`, its deepest stack `deepest`), every intersection
    of every ray (`hits`), and one fixed set of intervals around each ray's first two intersections (`t_min`, `t_max`)."""

    def __init__(self, name, oracle):
        self.name = name
        self.scene, self.rays = {"golden": lambda: _golden_scene(), "seeded": lambda: _seeded_scene(oracle), "chain": lambda: _chain(oracle)}[name]()
        self.want, self.deepest = oracle.trace(self.scene, self.rays, threads=8)
        self.want = np.ascontiguousarray(self.want)
        self.hits = brute_force(self.scene, self.rays)
        # (the golden fixture's own rays: 47 of 1024 meet two triangles at all, so every one of them has its first hit cut away)
        self.t_min, self.t_max = intervals(self.hits, len(self.rays), SEED + 2 + NAMES.index(name), cut_share=1.0 if name == "golden" else 0.6)

    def miss_record(self):
        """Today's miss record, from the oracle (every scene has rays that miss)."""
        miss = self.want[self.want["hit"] == 0]
        assert len(miss) and len(set(miss.tobytes()[k * 16:(k + 1) * 16] for k in range(len(miss)))) == 1
        return miss[0]


def case(name, oracle):
    """Computed once per process and shared: nobody changes what it returns."""
    if name not in _CACHE:
        _CACHE[name] = Case(name, oracle)
    return _CACHE[name]


# ---- the brute force ----------------------------------------------------------------------------------------------------------

class Hits:
    """Every intersection of every ray, as rows sorted by (ray, t): `start[r] : start[r + 1]` are ray r's, and the last row of
    each ray is a sentinel at t = +inf."""

    def __init__(self, ray, t, inst, tri, n_rays):
        sent = np.arange(n_rays, dtype=np.int64)
        ray = np.concatenate([ray, sent]); t = np.concatenate([t, np.full(n_rays, np.inf, F)])
        inst = np.concatenate([inst, np.full(n_rays, NONE)]); tri = np.concatenate([tri, np.full(n_rays, NONE)])
        order = np.lexsort((t, ray))
        self.ray, self.t, self.inst, self.tri = ray[order], t[order], inst[order], tri[order]
        self.start = np.searchsorted(self.ray, np.arange(n_rays + 1))
        self.n_rays = n_rays

    def nth(self, k):
        """t of each ray's k-th intersection (0 = the first), +inf where it has fewer."""
        at = self.start[:-1] + k
        ok = at < self.start[1:]
        return np.where(ok, self.t[np.minimum(at, len(self.t) - 1)], F(np.inf)).astype(F)


def _mesh_triangles(mesh, verts, idx):
    n_tri = int(mesh["index_count"]) // 3
    base, vo = int(mesh["base_index"]), int(np.uint32(mesh["vertex_offset"]))
    sel = idx[base: base + 3 * n_tri].astype(np.int64).reshape(n_tri, 3) + vo
    return verts[sel]                                      # [T][3][3]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _tri_all(eye, d, tri):
    """np_restate._tri for rays [R][3] x triangles [T][3][3], without the `t < hit` bound -> (t [R][T], accepted [R][T])."""
    v0, v1, v2 = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    eye, d = eye[:, None, :], d[:, None, :]
    e1, e2 = v1 - v0, v2 - v0
    uvec = _cross(d, e2)
    det = _dot(e1, uvec)
    ok = ~(det < F(1e-10))
    inv_det = F(1.0) / det
    o = eye - v0
    u = inv_det * _dot(o, uvec)
    ok &= ~((u < 0) | (u > 1))
    vvec = _cross(o, e1)
    v = inv_det * _dot(d, vvec)
    ok &= ~((v < 0) | ((u + v) > 1))
    t = inv_det * _dot(e2, vvec)
    assert t.dtype == F
    return t, ok & (t > 0) & (t < MAX_DIST)


def brute_force(scene, rays, chunk=1 << 22):
    tl, inst, meshes, bn, verts, idx = scene
    verts = np.asarray(verts, F).reshape(-1, 3)
    idx = np.asarray(idx, np.uint32).reshape(-1)
    eye, d = np.ascontiguousarray(rays["eye"], F), np.ascontiguousarray(rays["dir"], F)
    tris = [_mesh_triangles(m, verts, idx) for m in meshes]
    boxes = [(t.reshape(-1, 3).min(axis=0).astype(np.float64), t.reshape(-1, 3).max(axis=0).astype(np.float64)) for t in tris]
    out = ([], [], [], [])
    with np.errstate(all="ignore"):
        for i in range(len(inst)):
            m = min(int(inst[i]["mesh"]), len(meshes) - 1)
            M = inst[i]["inv_transform"].reshape(4, 4).astype(F)
            e2 = np.stack([((M[0, r] * eye[:, 0] + M[1, r] * eye[:, 1]) + M[2, r] * eye[:, 2]) + M[3, r] * F(1) for r in range(3)], axis=1)
            d2 = np.stack([((M[0, r] * d[:, 0] + M[1, r] * d[:, 1]) + M[2, r] * d[:, 2]) + M[3, r] * F(0) for r in range(3)], axis=1)
            assert e2.dtype == F and d2.dtype == F
            # the shortcut of the module's docstring, in float64
            c, half = (boxes[m][0] + boxes[m][1]) / 2, np.linalg.norm(boxes[m][1] - boxes[m][0]) / 2
            e64, d64 = e2.astype(np.float64), d2.astype(np.float64)
            dd = (d64 * d64).sum(axis=1)
            w = c[None, :] - e64
            perp = w - d64 * ((w * d64).sum(axis=1) / dd)[:, None]
            far = np.sqrt((perp * perp).sum(axis=1)) > half * 1.001 + 1e-6
            keep = np.flatnonzero(~(far & np.isfinite(dd) & (dd > 0) & np.isfinite(perp).all(axis=1)))
            step = max(1, chunk // max(1, len(tris[m])))
            for a in range(0, len(keep), step):
                sel = keep[a: a + step]
                t, ok = _tri_all(e2[sel], d2[sel], tris[m])
                r, k = np.nonzero(ok)
                out[0].append(sel[r]); out[1].append(t[r, k]); out[2].append(np.full(len(r), i, np.uint32)); out[3].append(k.astype(np.uint32))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return Hits(cat(out[0], np.int64), cat(out[1], F), cat(out[2], np.uint32), cat(out[3], np.uint32), len(rays))


# ---- what an interval gives ---------------------------------------------------------------------------------------------------

def normalise(t_min, t_max):
    """voidin_abi.h "Ray intervals": t_lo = fmaxf(_pad0, 0), t_hi = fminf(_pad1, VD_MAX_DIST) (fmaxf / fminf: a NaN operand is ignored)."""
    return np.fmax(np.asarray(t_min, F), F(0)).astype(F), np.fmin(np.asarray(t_max, F), MAX_DIST).astype(F)


class Expected:
    """records: HIT array (dist, hit of every ray; instance / triangle meaningful where `unique`); unique: exactly one triangle
    attains the minimum, or the ray misses (then the whole miss record is expected)."""

    def __init__(self, records, unique):
        self.records, self.unique = records, unique


def expected(hits, t_min, t_max, miss_record, ray_of=None):
    """The brute force's answer for one interval per ray.  ray_of: row k of the call is ray ray_of[k] of `hits` (default: itself)."""
    n = len(np.asarray(t_min))
    ray_of = np.arange(n) if ray_of is None else np.asarray(ray_of)
    t_lo, t_hi = normalise(t_min, t_max)
    rec = np.empty(n, dtype=abi.HIT)
    rec[:] = miss_record
    # rows are sorted by (ray, t) and a positive float orders as its bit pattern: one search over the key {ray, bits of t} finds
    # each ray's first row above t_lo (its sentinel at +inf when there is none); it counts when it lies below t_hi
    key = (hits.ray.astype(np.uint64) << np.uint64(32)) | hits.t.view(np.uint32).astype(np.uint64)
    lo_bits = np.where(t_lo > 0, t_lo, F(0)).astype(F).view(np.uint32).astype(np.uint64)
    at = np.searchsorted(key, (ray_of.astype(np.uint64) << np.uint64(32)) | lo_bits, side="right")
    at = np.minimum(at, len(hits.t) - 1)                   # (t_lo = +inf lands behind the ray's sentinel: nothing is above it)
    t = hits.t[at]
    ok = (hits.ray[at] == ray_of) & (t < t_hi)
    rec["dist"][ok], rec["hit"][ok], rec["instance"][ok], rec["triangle"][ok] = t[ok], 1, hits.inst[at][ok], hits.tri[at][ok]
    nxt = np.minimum(at + 1, len(hits.t) - 1)
    unique = ~(ok & (hits.ray[nxt] == hits.ray[at]) & (nxt != at) & (hits.t[nxt] == t))
    return Expected(rec, unique)


def intervals(hits, n_rays, seed, cut_share=0.6):
    """One interval per ray, placed around its first two intersections t1 <= t2 (a ray with fewer takes 8, or twice t1, in their
    place), by class: 0 (t1 inside, ends before t2), 1 (first hit cut away, t2 inside, no upper end), 2 (as 1, upper end behind t2),
    3 (ends before t1), 4 (between t1 and t2: nothing inside), 5 (t_min = t1 exactly, no upper end), 6 (t_max = t2 exactly).
    Of the rays with two intersections a share `cut_share` falls into 1, 2 and 5 - the ones t_min cuts the first hit of while a
    later one stays inside; the other rays mostly into 0 and 3."""
    rng = np.random.default_rng(seed)
    t1, t2 = hits.nth(0), hits.nth(1)
    two = np.isfinite(t2)
    t1 = np.where(np.isfinite(t1), t1, F(8)).astype(F)
    t2 = np.where(two, t2, t1 * F(2)).astype(F)
    rest = (1.0 - cut_share) / 4
    cls = np.where(two, rng.choice(7, size=n_rays, p=[rest, 0.4 * cut_share, 0.35 * cut_share, rest, rest, 0.25 * cut_share, rest]),
                   rng.choice(7, size=n_rays, p=[0.3, 0.02, 0.02, 0.5, 0.02, 0.07, 0.07]))
    u, v = rng.random(n_rays).astype(F), rng.random(n_rays).astype(F)
    below, between, behind = (t1 * u).astype(F), (t1 + (t2 - t1) * u).astype(F), (t2 * (F(1) + v) + F(1e-3)).astype(F)
    between2 = (between + (t2 - between) * v).astype(F)
    is_ = [cls == k for k in range(7)]
    t_min = np.select(is_, [below, between, between, F(0) * u, between, t1, below]).astype(F)
    t_max = np.select(is_, [between, np.full(n_rays, MAX_DIST), behind, (t1 * v).astype(F), between2, np.full(n_rays, MAX_DIST), t2]).astype(F)
    return t_min, t_max


def big_call(c, copies, seed):
    """A call large enough to fan out, whose expected records still come from the brute force: the case's rays `copies` times over,
    every copy with intervals of its own.  -> (rays, t_min, t_max, ray_of)."""
    n = len(c.rays)
    parts = [intervals(c.hits, n, seed + k) for k in range(copies)]
    return (np.tile(c.rays, copies), np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
            np.tile(np.arange(n), copies))


def with_range(rays, t_min, t_max):
    """A copy of the rays with the two fields filled."""
    from voidin_amd.runtime import set_ray_range
    return set_ray_range(rays.copy(), t_min, t_max)


def populations(c, t_min, t_max):
    """-> (share of rays whose first hit t_min cuts away while a later one stays inside, share that t_max turns into misses,
    share left out of the instance / triangle comparison)."""
    e = expected(c.hits, t_min, t_max, c.miss_record())
    t_lo, t_hi = normalise(t_min, t_max)
    first = c.hits.nth(0)
    had = np.isfinite(first)
    cut = had & (first <= t_lo) & (e.records["hit"] == 1)
    ended = had & (first > t_lo) & (first >= t_hi) & (e.records["hit"] == 0)
    return cut.mean(), ended.mean(), (~e.unique).mean()
