"""Random cases for the shading chain and what the twins expect of them: vd_lighting_dev (part "lighting"), vd_gbuffer_points_dev and
vd_shadow_gbuffer*_dev (part "shadow"), vd_gbuffer_trace*_dev into vd_shade_gbuffer*_dev (part "chain").  Shared by
tests/test_fuzz_shading_cases.py (CPU: the populations of the suite's slice, the replay), tools/fuzz_shading.py (the campaigns) and
tests/test_gpu_fuzz_shading.py (the slice); a helper module, no tests in it, no GPU, and not the library under test.

Everything expected comes from twins that are there: gbuffer_cases (points, scatter), shadow_pass_cases (lights, in_range, pack, Want),
lighting_cases (shade, rule_words, subset_words, materials), gbuffer_trace_cases (resolve, rays, same_image) and the oracle's walk.

A case is a pure function of (seed, part, case number): its generator is np.random.default_rng([seed, part, number]), so case k of a
campaign is made alone, without the cases in front of it.  Two inputs are not drawn but DEALT, so that a slice cannot miss them by
chance: the light count of case k is entry k of a seeded shuffle of the part's list (every block of len(list) cases holds every
count once), and every twelfth shadow case (k % 12 == LARGE_AT) is the large one - 131 x 97 pixels, 256 or 257 lights: enough cells
(n_lights * ceil(points / 512)) for a second round of the one-workgroup scan.

Where a generator has to see something it looks: a camera is drawn up to CAMERA_TRIES times until between a tenth and nine tenths of
its pixels hit the scene (the oracle's answer; the last draw stays when none does), lights up to LIGHT_TRIES times until a pair is in
range and one is not.  Both loops consume the case's own generator only.

The occluded bit of a pair in range is the oracle's record of the pair's shadow ray (origin pos + nor * 0.0001, direction light - pos,
so the light sits at t = 1): `hit` of the walk over the half-line with VD_OPT_TRACE_RAY_RANGE off, and with it on `hit` of the same walk
over the ray's interval (0, 1) - oracle.trace_range, which restates "Ray intervals" of include/voidin_abi.h word for word: the result
starts at dist = t_hi and the box tests prune by it.  The form tests/test_gpu_trace_range.py derives such answers by, `hit and dist < 1`
of the half-line's closest hit, was tried first and checked on the CPU against the brute force over the open segment
(shadow_pass_cases.segment_hits) on a small case - shadow case 2 of seed 606 made at 17 x 5 pixels with 33 lights: every ray agrees, and
tests/test_fuzz_shading_cases.py repeats it.  The first campaign then found 29 pairs in six cases where the device reports no occluder
and that form reports one, all of them at depth 1e-40: a point 1e37 away, whose shadow ray is so long that the whole scene lies within
an ulp of t = 1.  There a triangle's t comes out just below 1 while the entry distance of a box around it comes out AT 1, and a walk
that starts at dist = 1 does not enter the box.  The header defines the record by the walk, so the device is right and the form (and
the brute force, which knows no boxes) is not the definition there; the interval walk of the oracle gives the device's bits in all 29.
Words.near keeps the form, and the CPU tests hold that it equals the walk wherever a point is nearer than 1e30.  Only pairs in range are walked."""
import math

import numpy as np

import gbuffer_cases as G
import gbuffer_trace_cases as T
import lighting_cases as L
import shadow_pass_cases as S
import trace_range_cases as cases
from voidin_amd import abi, synth

F, U = np.float32, np.uint32
PARTS = ("lighting", "shadow", "chain")
SEED = 606
SLICE = {"lighting": 48, "shadow": 12, "chain": 8}          # what tests/test_gpu_fuzz_shading.py runs
SHAPES = ((1, 1), (63, 1), (64, 1), (65, 1), (127, 1), (129, 1), (256, 1), (17, 31), (64, 9), (65, 3), (7, 73), (129, 5), (193, 3), (33, 33))
# W = 0, 1, 2, 3, both parities inside 4 .. 31, and 32 - with counts at 32 W - 1, 32 W and 32 W + 1
LIGHT_COUNTS = {"lighting": (0, 1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 160, 161, 193, 255, 256, 257, 320, 352, 500, 511, 512, 513, 700,
                             900, 992, 993, 1000, 1023, 1024),
                "shadow": (0, 1, 2, 31, 32, 33, 64, 65, 96, 97, 129, 257),
                "campaign shadow": (0, 1, 2, 31, 32, 33, 64, 65, 96, 97, 129, 160, 257, 352, 512, 1000, 1024),
                "chain": (0, 1, 31, 32, 33, 64, 65)}
MATERIAL_VALUES, MATERIAL_P = (0, 1, 2, 3, 7, 255), (0.1, 0.25, 0.1, 0.2, 0.15, 0.2)        # 0 and 2 - no receiver - together 20 %
DEPTH_EDGES = np.array([0.0, -0.0, np.nan, np.inf, 1.0, -1.0, 1e-40], np.float64)
RADIUS_EDGES = np.array([0.0, np.nan, np.inf, -1.0], F)
CHUNKS = (0, 1, 97, 1500, 20000)
SHADOW_FORMS = ("scene", "prepared", "wide", "tight")       # test_gpu_shadow_gbuffer.FORMS
CHAIN_FORMS = ("scene", "prepared", "wide")                 # not tight: its ties may report another triangle
LARGE_AT, LARGE_SHAPE, LARGE_LIGHTS = 7, (131, 97), (256, 257)
CAMERA_TRIES, LIGHT_TRIES = 8, 6
UV_EDGES = np.array([65504.0, 65520.0, 1e9, 1e-8, 3e-6, np.nan], F)       # 3e-6: a subnormal half (1e-8 alone rounds to zero)


def rng_of(seed, part, k):
    return np.random.default_rng([int(seed), PARTS.index(part), int(k)])


def dealt(seed, part, k, values):
    """Entry k of the seeded shuffles of `values`, one shuffle per block of len(values) cases."""
    n = len(values)
    return values[int(np.random.default_rng([int(seed), PARTS.index(part), k // n, 77]).permutation(n)[k % n])]


# ---- inputs common to the parts -----------------------------------------------------------------------------------------------------

def look(eye, target):
    """synth.camera_uniform at `eye`, its forward axis through `target`."""
    d = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    d /= np.linalg.norm(d)
    return synth.camera_uniform(eye=tuple(float(x) for x in eye), yaw_deg=math.degrees(math.atan2(-d[0], -d[2])), pitch_deg=math.degrees(math.asin(d[1])))


def forward(cam):
    V = cam["view"].reshape(4, 4).astype(np.float64)          # [column][row]
    return -V[:3, 2]


def pitches(rng, w):
    """-> ((depth, normal_uv, material) pitches, the colour target's): each image packed or padded, the material pitch odd in half
    the cases, the colour rows always further apart than they are long."""
    d = 4 * w + (4 * int(rng.integers(1, 9)) if rng.random() < 0.5 else 0)
    n = 8 * w + (8 * int(rng.integers(1, 9)) if rng.random() < 0.5 else 0)
    m = w + (int(rng.integers(1, 9)) if rng.random() < 0.5 else 0)
    odd = rng.random() < 0.5
    if (m & 1) != int(odd):
        m += 1
    return (d, n, m), 16 * w + 16 * int(rng.integers(1, 5))


def images(rng, cam, w, h):
    """The three images of part (a) -> (depth [h][w], normal_uv [h][w][2], material [h][w])."""
    n = w * h
    depth = (float(cam["znear"]) / rng.uniform(5.0, 60.0, n)).astype(F)
    edges = rng.random() < 1 / 3
    at, which = rng.random(n) < 1 / 16, rng.integers(0, len(DEPTH_EDGES), n)
    if edges:
        depth[at] = DEPTH_EDGES[which[at]].astype(F)
    words = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(U)
    material = np.asarray(MATERIAL_VALUES, np.uint8)[rng.choice(len(MATERIAL_VALUES), n, p=MATERIAL_P)]
    return depth.reshape(h, w), words.reshape(h, w, 2), material.reshape(h, w)


def lights(rng, n, centre, edges=True):
    """shadow_pass_cases.lights in a random box about `centre`, radii from {2, 10, 25} to {30, 60, 200}, colours in [0, 2); in a
    quarter of the cases three radii from {0, NaN, +inf, -1}."""
    half = float(rng.choice([10.0, 30.0, 60.0]))
    radii = (float(rng.choice([2.0, 10.0, 25.0])), float(rng.choice([30.0, 60.0, 200.0])))
    seed = int(rng.integers(1 << 30))
    colour = (2.0 * rng.random((n, 3))).astype(F)
    special, where, what = rng.random() < 0.25, rng.integers(0, max(n, 1), 3), rng.integers(0, len(RADIUS_EDGES), 3)
    out = S.lights(n=n, seed=seed, box=tuple((float(c) - half, float(c) + half) for c in centre), radii=radii)
    out["color"] = colour
    if special and edges and n:
        out["radius"][where] = RADIUS_EDGES[what]
    return out


def fed_words(rng, gb, lts):
    """The bit words a lighting call is fed -> (in-range words [pixels][W], occluded words): the rule's; in a fifth of the cases with
    a random 10 % of the bits flipped on receivers and every bit set elsewhere; the bits at and above n_lights random; the occluded
    words a seeded subset of the in-range ones."""
    n, n_lights = gb.width * gb.height, len(lts)
    W = (n_lights + 31) // 32
    flip, noise = rng.random() < 0.2, rng.random((n, W * 32)) < 0.1
    tail = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    seed, stream = int(rng.integers(1 << 30)), int(rng.integers(0, 16))
    if not n_lights:
        return None, None
    inr = L.rule_words(gb, lts).copy()
    if flip:
        recv = G.receivers(gb.material.reshape(-1))
        inr[recv] ^= S.pack(noise)[recv]
        inr[~recv] = U(0xffffffff)
    if n_lights & 31:
        keep = U((1 << (n_lights & 31)) - 1)
        inr[:, W - 1] = (inr[:, W - 1] & keep) | (tail & ~keep)
    occ = L.subset_words(inr, seed, stream=stream)
    if flip:
        occ[~G.receivers(gb.material.reshape(-1))] = U(0xffffffff)
    return inr, occ


def lights_only(words, n_lights):
    """The words with the bits at and above n_lights cleared, as test_the_bits_decide (d) hands them to the twin."""
    out = words.copy()
    if n_lights & 31:
        out[:, -1] &= U((1 << (n_lights & 31)) - 1)
    return out


# ---- (a) lighting -------------------------------------------------------------------------------------------------------------------

class LightingCase:
    part = "lighting"

    def __init__(self, seed, k):
        rng = rng_of(seed, "lighting", k)
        self.seed, self.k = seed, k
        self.n_lights = dealt(seed, "lighting", k, LIGHT_COUNTS["lighting"])
        self.w, self.h = SHAPES[int(rng.integers(len(SHAPES)))]
        self.pitches, self.colour_pitch = pitches(rng, self.w)
        eye = rng.uniform(-50.0, 50.0, 3)
        self.cam = synth.camera_uniform(eye=tuple(float(x) for x in eye), yaw_deg=float(rng.random() * 360), pitch_deg=float(rng.random() * 120 - 60))
        self.gb = G.GBuffer(self.cam, *images(rng, self.cam, self.w, self.h))
        self.lts = lights(rng, self.n_lights, eye + forward(self.cam) * rng.uniform(10.0, 40.0))
        self.inr, self.occ = fed_words(rng, self.gb, self.lts)
        self.table = L.materials()
        self.W = (self.n_lights + 31) // 32

    def want(self, **wrong):
        if not self.n_lights:
            return L.shade(self.gb, self.lts, None, None, self.table)
        return L.shade(self.gb, self.lts, lights_only(self.inr, self.n_lights), lights_only(self.occ, self.n_lights), self.table, **wrong)

    def describe(self):
        return f"lighting case {self.k} (seed {self.seed}): {self.w} x {self.h}, {self.n_lights} lights, pitches {self.pitches} / {self.colour_pitch}"


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------

class Scene:
    """scene: the six arrays of a trace scene; centres: the world centres of the instances' boxes; extent: the cube they lie in."""

    def __init__(self, scene, extent, name):
        self.scene, self.extent, self.name = scene, extent, name
        inst, meshes = scene[1], scene[2]
        mid = ((meshes["min"] + meshes["max"]) * F(0.5)).astype(np.float64)[inst["mesh"]]
        M = inst["transform"].reshape(-1, 4, 4).astype(np.float64)          # [column][row]
        self.centres = np.einsum("nc,ncr->nr", mid, M[:, :3, :3]) + M[:, 3, :3]
        half = ((meshes["max"] - meshes["min"]) * F(0.5)).astype(np.float64)[inst["mesh"]]
        self.radii = np.linalg.norm(half * np.linalg.norm(M[:, :3, :3], axis=2), axis=1)      # of a sphere about the instance's box


def random_scene(rng, oracle, seeded_share=0.5):
    """Either the `seeded` scene of trace_range_cases or one made the way tools/fuzz_trace.py makes them: 1 to 4 meshes, 1 to 300
    instances, mirrored ones in a third of the cases, BLAS and TLAS by the oracle."""
    use_seeded = rng.random() < seeded_share
    n_mesh = int(rng.integers(1, 5))
    srcs = []
    for _ in range(n_mesh):
        kind, a, b, s = int(rng.integers(0, 3)), int(rng.integers(1, 8)), int(rng.integers(4, 16)), int(rng.integers(1 << 30))
        radius, n_u, n_tri = float(rng.choice([0.5, 1.0, 3.0])), int(rng.integers(8, 64)), int(rng.integers(1, 200))
        srcs.append((kind, a, b, s, radius, n_u, n_tri))
    n_inst = int(rng.choice([1, 2, 7, 63, 64, 65, 300]))
    ext = float(rng.choice({1: [3.0, 6.0], 2: [4.0, 8.0], 7: [6.0, 15.0]}.get(n_inst, [30.0, 60.0] if n_inst < 300 else [50.0, 100.0])))
    inst_seed, big = int(rng.integers(1 << 30)), float(rng.choice([1.0, 4.0]))
    mirror, m = rng.random() < 1 / 3, rng.integers(0, n_inst, max(1, n_inst // 10))
    if use_seeded:
        return Scene(cases.case("seeded", oracle).scene, 50.0, "seeded")
    V, I, B = [], [], []
    infos = np.zeros(n_mesh, dtype=abi.MESH_INFO)
    vo = bo = no = 0
    for j, (kind, a, b, s, radius, n_u, n_tri) in enumerate(srcs):
        v, i = (synth.uv_sphere(radius, a), synth.knot_mesh(n_u, b, seed=s), synth.triangle_soup(n_tri, seed=s))[kind]
        v = np.asarray(v, F).reshape(-1, 3)
        nodes, idx = oracle.bvh_build(v, i)
        infos[j]["min"], infos[j]["max"] = synth.mesh_bounds(v)
        infos[j]["index_count"], infos[j]["base_index"] = len(idx), bo
        infos[j]["vertex_offset"], infos[j]["bvh_index"] = vo, no
        V.append(v); I.append(idx); B.append(nodes)
        vo += len(v); bo += len(idx); no += len(nodes)
    inst = synth.instances(n_inst, n_mesh=n_mesh, seed=inst_seed, extent=ext, scale_range=(0.2, big))
    if mirror:                                              # a negative determinant: backface culling flips
        Tm = inst["transform"].reshape(-1, 4, 4).copy()
        Tm[m, 0, :3] *= F(-1)
        inst["transform"] = Tm.reshape(-1, 16)
        inst["inv_transform"] = np.linalg.inv(Tm.astype(np.float64).transpose(0, 2, 1)).transpose(0, 2, 1).reshape(-1, 16).astype(F)
    scene = (oracle.tlas_build(inst, infos), inst, infos, np.concatenate(B), np.concatenate(V), np.concatenate(I).astype(U))
    return Scene(scene, ext, f"random: {n_mesh} meshes, {n_inst} instances{', mirrored' if mirror else ''}, extent {ext:g}")


def camera_on(rng, oracle, sc, w, h, rays_of):
    """A camera outside the middle of the scene that looks at one of its instances -> (camera, the oracle's records of rays_of(camera)).
    Drawn again until between a tenth and nine tenths of the rays hit."""
    for attempt in range(CAMERA_TRIES):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        d[1] = abs(d[1]) * 0.5
        d /= np.linalg.norm(d)
        j = int(rng.integers(len(sc.centres)))
        far, near, off = rng.uniform(0.3, 1.1), rng.uniform(2.0, 8.0), rng.normal(size=3)
        if attempt % 2 == 0:                                # from the outside, towards an instance ...
            eye, aim = d * sc.extent * far, sc.centres[j] + off * 0.05 * sc.extent
        else:                                               # ... or from a few of its radii away
            eye, aim = sc.centres[j] + d * sc.radii[j] * near, sc.centres[j] + off * 0.2 * sc.radii[j]
        cam = look(eye, aim)
        rec = np.ascontiguousarray(oracle.trace(sc.scene, rays_of(cam), threads=8)[0])
        if 0.1 <= (rec["hit"] == 1).mean() <= 0.9:
            break
    return cam, rec


def lights_on(rng, gb, n_lights, edges=True):
    """Lights about one of the G-buffer's finite points, drawn again until a pair is in range and one is not (when there are two pairs)."""
    pos = gb.points()[0]
    finite = pos[np.isfinite(pos).all(axis=1)]
    for _ in range(LIGHT_TRIES):
        centre = finite[int(rng.integers(len(finite)))] if len(finite) else np.zeros(3)
        lts = lights(rng, n_lights, np.asarray(centre, np.float64), edges)
        if not n_lights or len(pos) * n_lights < 2:
            break
        reach = S.in_range(pos, lts)
        if reach.any() and not reach.all():
            break
    return lts


def surface_depth(cam, rays, rec, depth):
    """`depth` with the clip z / w of the hit point wherever a record of `rays` (gbuffer_cases.centre_rays) hits - float64, rounded:
    input data, as gbuffer_cases.seeded_gbuffer makes it."""
    at = np.flatnonzero(rec["hit"] == 1)
    p = rays["eye"][at].astype(np.float64) + rays["dir"][at].astype(np.float64) * rec["dist"][at].astype(np.float64)[:, None]
    PV = cam["projection"].reshape(4, 4).astype(np.float64).T @ cam["view"].reshape(4, 4).astype(np.float64).T
    clip = (PV @ np.concatenate([p, np.ones((len(p), 1))], axis=1).T).T
    out = depth.reshape(-1).copy()
    with np.errstate(all="ignore"):
        out[at] = (clip[:, 2] / clip[:, 3]).astype(F)
    return out.reshape(depth.shape)


def occluded_pairs(oracle, scene, pos, nor, lts, reach):
    """The oracle's records of the shadow rays of the pairs in range -> (hit [P][L], hit inside (0, 1) [P][L], hit and dist < 1
    [P][L]): the walk over the half-line, the walk over the ray's interval (oracle.trace_range), and the form the interval's answer
    was first derived by; a pair out of range is False in all three."""
    hit, inside, near = np.zeros(reach.shape, bool), np.zeros(reach.shape, bool), np.zeros(reach.shape, bool)
    sel = [np.flatnonzero(reach[:, l]) for l in range(len(lts))]
    rays = [oracle.shadow_rays(pos[s], nor[s], lts["position"][l]) for l, s in enumerate(sel) if len(s)]
    if rays:
        rays = np.concatenate(rays)
        rec = oracle.trace(scene, rays, threads=8)[0]
        rays["_pad0"], rays["_pad1"] = F(0), F(1)              # what vd_shadow_rays_dev writes under the option
        ranged = oracle.trace_range(scene, rays, threads=8)
        at = 0
        for l, s in enumerate(sel):
            r = rec[at: at + len(s)]
            hit[s, l] = r["hit"] == 1
            inside[s, l] = ranged["hit"][at: at + len(s)] == 1
            near[s, l] = (r["hit"] == 1) & (r["dist"] < F(1))
            at += len(s)
    return hit, inside, near


class Words:
    """What vd_shadow_gbuffer*_dev writes for a G-buffer, from the CPU: reach / hit [ray_range] / near (hit and dist < 1) as bool [P][L], want[ray_range]
    (shadow_pass_cases.Want), the per-pixel words inr and occ[ray_range], and the info record."""

    def __init__(self, oracle, scene, gb, lts):
        pos, nor, _ = gb.points()
        self.reach = S.in_range(pos, lts) if len(lts) else np.zeros((len(pos), 0), bool)
        h0, h1, self.near = occluded_pairs(oracle, scene, pos, nor, lts, self.reach)
        self.hit = {0: h0, 1: h1}
        self.want = {r: S.Want(self.reach, h) for r, h in self.hit.items()}
        self.inr = G.scatter(gb, self.want[0].in_range_words)
        self.occ = {r: G.scatter(gb, w.occluded_words) for r, w in self.want.items()}
        L_ = len(lts)
        self.info = {"n_points": len(pos) if L_ else 0, "n_rays": int(self.reach.sum()), "words_per_point": (L_ + 31) // 32}


# ---- (b) the G-buffer shadow pass -----------------------------------------------------------------------------------------------------

class ShadowCase:
    part = "shadow"

    def __init__(self, seed, k, oracle, campaign=False, shape=None, n_lights=None):
        rng = rng_of(seed, "shadow", k)
        self.seed, self.k, self.oracle = seed, k, oracle
        large = k % 12 == LARGE_AT
        self.n_lights = dealt(seed, "shadow", k, LIGHT_COUNTS["campaign shadow" if campaign else "shadow"])
        self.w, self.h = SHAPES[1 + int(rng.integers(len(SHAPES) - 1))]         # not 1 x 1: one pair cannot be both in range and out of it
        big = LARGE_LIGHTS[int(rng.integers(2))]
        if large:
            (self.w, self.h), self.n_lights = LARGE_SHAPE, big
        if shape is not None:                               # a cut of the case, for the small check of the module's docstring
            (self.w, self.h), self.n_lights = shape, n_lights
        self.max_chunk_rays, self.ray_range = int(rng.choice(CHUNKS)), int(rng.integers(2))
        self.pitches, _ = pitches(rng, self.w)
        self.sc = random_scene(rng, oracle)
        self.cam, rec = camera_on(rng, oracle, self.sc, self.w, self.h, lambda cam: G.centre_rays(cam, self.w, self.h))
        depth, words, material = images(rng, self.cam, self.w, self.h)
        self.gb = G.GBuffer(self.cam, surface_depth(self.cam, G.centre_rays(self.cam, self.w, self.h), rec, depth), words, material)
        self.lts = lights_on(rng, self.gb, self.n_lights, edges=not large)
        self._words = None

    def words(self):
        if self._words is None:
            self._words = Words(self.oracle, self.sc.scene, self.gb, self.lts)
        return self._words

    def describe(self):
        return (f"shadow case {self.k} (seed {self.seed}): {self.w} x {self.h}, {self.n_lights} lights, max_chunk_rays {self.max_chunk_rays}, "
                f"ray_range {self.ray_range}, pitches {self.pitches}, scene {self.sc.name}")


# ---- (c) the whole chain ----------------------------------------------------------------------------------------------------------------

def attributes(rng, n_vertices):
    """Per-vertex normals (random unit vectors, some zero, some NaN) and uvs (uniform in [-2, 2], runs of vertices at 65504, 65520, 1e9,
    1e-8, 3e-6 and NaN - runs, so that all three corners of some triangles hold the value and it survives the interpolation)."""
    n = rng.normal(size=(n_vertices, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    kind = rng.random(n_vertices)
    n[kind < 0.03] = 0.0
    n[kind > 0.97] = np.nan
    uv = rng.uniform(-2.0, 2.0, (n_vertices, 2))
    run = max(3, n_vertices // 12)
    for value in UV_EDGES:
        at, comp = int(rng.integers(0, max(1, n_vertices - run))), int(rng.integers(0, 3))
        uv[at: at + run, ([0], [1], [0, 1])[comp]] = value
    return n.astype(F), uv.astype(F)


class ChainCase:
    part = "chain"

    def __init__(self, seed, k, oracle):
        rng = rng_of(seed, "chain", k)
        self.seed, self.k, self.oracle = seed, k, oracle
        self.n_lights = dealt(seed, "chain", k, LIGHT_COUNTS["chain"])
        self.w, self.h = SHAPES[int(rng.integers(len(SHAPES)))]
        self.ray_range, self.max_chunk_rays = int(rng.integers(2)), int(rng.choice(CHUNKS))
        self.colour_pitch = pitches(rng, self.w)[1]
        self.sc = random_scene(rng, oracle, seeded_share=0.25)
        tl, inst, meshes, bn, verts, idx = self.sc.scene
        inst = np.array(inst, dtype=abi.INSTANCE, copy=True)
        inst["material"] = np.asarray((1, 3, 7, 255, 0x105, 2, 0x100, 0), U)[rng.choice(8, len(inst), p=(0.3, 0.2, 0.1, 0.15, 0.1, 0.05, 0.05, 0.05))]
        self.scene = (tl, inst, meshes, bn, verts, idx)
        self.sc.scene = self.scene
        nv = len(np.asarray(verts).reshape(-1, 3))
        normals, uvs = attributes(rng, nv)
        drop = int(rng.integers(4))                         # 0, 1: both attributes; 2: no normals; 3: no uvs
        self.full_geo = T.Geometry(inst, meshes, verts, idx, normals, uvs)
        self.geo = self.full_geo.without(normals=drop == 2, tex_coords=drop == 3)
        self.cam, self.rec = camera_on(rng, oracle, self.sc, self.w, self.h, lambda cam: T.rays(cam, self.w, self.h))
        self.img = T.resolve(self.cam, self.geo, self.rec, self.w, self.h)
        self.gb = self.img.gbuffer()
        self.lts = lights_on(rng, self.gb, self.n_lights)
        self.table = L.materials()
        self._words = None

    def words(self):
        if self._words is None:
            self._words = Words(self.oracle, self.scene, self.gb, self.lts)
        return self._words

    def colour(self):
        w = self.words()
        if not self.n_lights:
            return L.shade(self.gb, self.lts, None, None, self.table)
        return L.shade(self.gb, self.lts, w.inr, w.occ[self.ray_range], self.table)

    def describe(self):
        return (f"chain case {self.k} (seed {self.seed}): {self.w} x {self.h}, {self.n_lights} lights, max_chunk_rays {self.max_chunk_rays}, ray_range {self.ray_range}, "
                f"normals {self.geo.normals is not None}, uvs {self.geo.tex_coords is not None}, scene {self.sc.name}")


def make(part, seed, k, oracle=None, campaign=False):
    if part == "lighting":
        return LightingCase(seed, k)
    return ShadowCase(seed, k, oracle, campaign) if part == "shadow" else ChainCase(seed, k, oracle)
