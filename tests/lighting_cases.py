"""The float32 twin of the lighting pass (vd_lighting_dev, vd_shade_gbuffer*_dev: include/voidin_lighting.h), its material table and
its G-buffers.  Shared by tests/test_lighting_cases.py (CPU: the twin against hand values, the populations) and
tests/test_gpu_lighting.py; a helper module, no tests in it.

The twin restates the header's definition in numpy float32 with an explicit .astype(F) after every operation.  It is built on the
twins that are there: gbuffer_cases.world_position / decode_normal / receivers give `pos`, `nor` and which pixels run the loop,
shadow_pass_cases.dist is the loop's `dist`, shadow_pass_cases.in_range / pack and gbuffer_cases.scatter make the bit words a call
is fed.  The lights are visited one after the other in ascending order, every pixel whose bit is set at once.

materials(): 256 seeded VdFlatMaterial rows - albedo and specular in [0, 1), emissive in [0, 0.1), a pad word that is not zero.
flipped_gbuffer: the seeded G-buffer of gbuffer_cases with the normal word of every third receiver replaced by the code of the
opposite normal.  The seeded image's normals all face the eye, so covr = pos0(dot(-rd, nor)) is 0 on every pixel and the specular
term is never anything but 0; a flipped normal looks away from the eye and makes it count.
Everything is computed once per process and shared: nobody changes what these functions return."""
import numpy as np

import gbuffer_cases as G
import shadow_pass_cases as S
from voidin_amd import abi, synth

F = np.float32
SEED = synth.SEED_BASE + 113
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- inputs -------------------------------------------------------------------------------------------------------------------

def materials(seed=SEED):
    """256 FLAT_MATERIAL rows: one per value of the material byte."""
    def make():
        t = np.zeros(abi.LIGHTING_MATERIALS, dtype=abi.FLAT_MATERIAL)
        t["albedo"] = synth.uniform01(seed, 0, 3 * len(t)).reshape(-1, 3).astype(F)
        t["specular"] = synth.uniform01(seed, 1, len(t)).astype(F)
        t["emissive"] = (0.1 * synth.uniform01(seed, 2, 3 * len(t))).reshape(-1, 3).astype(F)
        t["_pad"] = 0xFACE0000 + np.arange(len(t))
        return t
    return _once(("materials", seed), make)


def flipped_gbuffer(oracle):
    """-> (scene, GBuffer 64 x 64): seeded_gbuffer with every third receiver's normal turned round."""
    def make():
        scene, gb, _ = G.seeded_gbuffer(oracle)
        words = gb.normal_uv.reshape(-1, 2).copy()
        turn = gb.points()[2][::3]
        words[turn, 0] = G.encode_normal((-G.decode_normal(words[turn, 0])).astype(F))
        return scene, G.GBuffer(gb.cam, gb.depth, words.reshape(gb.height, gb.width, 2), gb.material)
    return _once("flipped", make)


def rule_words(gb, lts):
    """The in-range words [pixels][W] of a G-buffer as vd_shadow_gbuffer_dev writes them: the twin of the rule on the twin's points."""
    return G.scatter(gb, S.pack(S.in_range(gb.points()[0], lts)))


def subset_words(words, seed, stream=0):
    """A seeded random subset of the set bits of `words`: occlusion bits that need no walk."""
    n = words.size
    r = (synth.uniform01(seed, 16 + stream, n) * 65536.0).astype(np.uint32) | ((synth.uniform01(seed, 48 + stream, n) * 65536.0).astype(np.uint32) << np.uint32(16))
    return words & r.reshape(words.shape)


# ---- the twin -----------------------------------------------------------------------------------------------------------------

def dot(a, b):
    return (((a[:, 0] * b[:, 0]).astype(F) + (a[:, 1] * b[:, 1]).astype(F)).astype(F) + (a[:, 2] * b[:, 2]).astype(F)).astype(F)


def pos0(x):
    return np.where(x > F(0), x, F(0)).astype(F)


def view(gb):
    """-> (pos [N][3], nor [N][3], covr [N]) of EVERY pixel of a G-buffer, in pixel order."""
    n = gb.width * gb.height
    i = np.arange(n, dtype=np.uint32)
    pos = G.world_position(gb.cam, i % np.uint32(gb.width), i // np.uint32(gb.width), gb.width, gb.height, gb.depth.reshape(-1))
    nor = G.decode_normal(gb.normal_uv.reshape(-1, 2)[:, 0])
    with np.errstate(all="ignore"):
        v = (np.asarray(gb.cam["view_position"], F).reshape(-1)[None, :3] - pos).astype(F)
        rd = (v / np.sqrt(dot(v, v)).astype(F)[:, None]).astype(F)
        covr = pos0(dot((-rd).astype(F), nor))
    return pos, nor, covr


def pow16(covr):
    c = np.asarray(covr, F)
    with np.errstate(all="ignore"):
        for _ in range(4):
            c = (c * c).astype(F)
    return c


def attenuation(dist, radius):
    """raytraced_shadows.wgsl:48-55 with max_intensity = falloff = 1."""
    with np.errstate(all="ignore"):
        s = (np.asarray(dist, F) / F(radius)).astype(F)
        s2 = (s * s).astype(F)
        q = (F(1) - s2).astype(F)
        return np.where(s >= F(1), F(0), ((q * q).astype(F) / (F(1) + s2).astype(F)).astype(F)).astype(F)


def shade(gb, lts, in_range_words, occluded_words, table, descending=False, ignore_occlusion=False):
    """The definition for a whole image -> float32 [pixels][4].  in_range_words / occluded_words: uint32 [pixels][W] (ignored when
    there is no light).  descending / ignore_occlusion: the two ways of being wrong the populations are counted for."""
    n, L = gb.width * gb.height, len(lts)
    mat = gb.material.reshape(-1)
    M = np.asarray(table)[mat]
    alb, spec, emi = M["albedo"].astype(F), M["specular"].astype(F), M["emissive"].astype(F)
    lit = G.receivers(mat)
    pos, nor, covr = view(gb)
    c16 = pow16(covr)
    with np.errstate(all="ignore"):
        c = np.where(lit[:, None], ((alb * F(0.3)).astype(F) + emi).astype(F), (alb + emi).astype(F)).astype(F)
        for l in (range(L - 1, -1, -1) if descending else range(L)):
            bit = np.uint32(1) << np.uint32(l & 31)
            at = np.flatnonzero(lit & ((in_range_words[:, l >> 5] & bit) != 0))
            if at.size == 0:
                continue
            p = pos[at]
            d = (np.asarray(lts["position"][l], F)[None, :] - p).astype(F)
            dist = S.dist(p, lts["position"][l])
            occluded = ((occluded_words[at, l >> 5] & bit) != 0) & (not ignore_occlusion)
            occlusion = np.where(occluded, F(0.5), F(1)).astype(F)
            atten = attenuation(dist, lts["radius"][l])
            ldir = (d / dist[:, None]).astype(F)
            shd = pos0(dot(nor[at], ldir))
            for k in range(3):
                col = F(lts["color"][l][k])
                diff = ((col * alb[at, k]).astype(F) * shd).astype(F)
                sp = ((col * spec[at]).astype(F) * c16[at]).astype(F)
                c[at, k] = (c[at, k] + (((diff + sp).astype(F) * occlusion).astype(F) * atten).astype(F)).astype(F)
        out = np.ones((n, 4), F)
        out[:, :3] = pos0(c)
        out[mat == G.NO_MATERIAL] = (1, 0, 1, 1)
    return out


def pass_words(oracle, key, scene, gb, lts, ray_range=False):
    """What vd_shadow_gbuffer*_dev writes, from the CPU: -> (occluded words [pixels][W], in-range words, S.Want of the points) - the
    twin's points, the twin of the range rule and the oracle's any-hit answer, scattered to pixels (`key` names the inputs in the
    cache of shadow_pass_cases; ("gbuffer", "seeded") is the expectation tests/test_gpu_shadow_gbuffer.py computes)."""
    pos, nor, _ = gb.points()
    w = S.Want(S.in_range(pos, lts), S.any_hit(oracle, ("gbuffer", key), scene, pos, nor, lts, ray_range))
    return G.scatter(gb, w.occluded_words), G.scatter(gb, w.in_range_words), w


def changed(a, b):
    """bool per pixel: the two images differ in a bit of the pixel (two NaNs count as equal: none leaves the twin anyway)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all(axis=1)
