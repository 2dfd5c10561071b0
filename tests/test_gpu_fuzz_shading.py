"""A fixed-seed slice of tools/fuzz_shading.py inside the gpu suite - random G-buffers, lights, bit words, scenes and cameras through
vd_lighting_dev, vd_gbuffer_points_dev / vd_shadow_gbuffer*_dev and vd_gbuffer_trace*_dev into vd_shade_gbuffer*_dev against the float32
twins, byte for byte (tests/test_fuzz_shading_cases.py holds, without a GPU, what this very slice visits) - and one deterministic
walk through every word count W = 3 .. 32, whatever happens to the slice's seed.  The campaigns with fresh seeds are recorded in
profiles/fuzz_shading.md."""
import os
import sys

import numpy as np
import pytest

import fuzz_shading_cases as Z
import gbuffer_cases as G
import lighting_cases as L
import shadow_pass_cases as S
from test_gpu_lighting import MANY, same, step
from test_gpu_shadow_gbuffer import Case, shapes
from test_gpu_shadow_gbuffer import same as same_words

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))


def _slice(ctx, ctx_options, part):
    import fuzz_shading
    ctx_options("trace.ray_range", None)                   # the option the cases set: back to its default after the test, whatever happens
    out = []
    bad = fuzz_shading.run(Z.SLICE[part], seed=Z.SEED, ctx=ctx, log=out.append, parts=(part,))
    assert bad[part] == 0, "\n".join(out[:10])


def test_fuzz_slice_lighting(ctx, oracle, ctx_options):
    _slice(ctx, ctx_options, "lighting")


def test_fuzz_slice_shadow_gbuffer(ctx, oracle, ctx_options):
    _slice(ctx, ctx_options, "shadow")


def test_fuzz_slice_chain(ctx, oracle, ctx_options):
    _slice(ctx, ctx_options, "chain")


def test_a_point_too_far_for_float32_follows_the_interval_walk(ctx, oracle, ctx_options):
    """Shadow case 124 of seed 731, the smallest the first campaign listed (tests/test_fuzz_shading_cases.py has its anatomy): with the
    ray range on, three pairs of a point 1e37 away are clear on the device and by the oracle's interval walk, occluded by `hit and
    dist < 1`."""
    import fuzz_shading
    from test_fuzz_shading_cases import FAR
    ctx_options("trace.ray_range", None)
    c = Z.ShadowCase(FAR[0], FAR[1], oracle, campaign=True)
    assert c.ray_range == 1 and (c.words().near != c.words().hit[1]).sum() == 3
    out = []
    bad = fuzz_shading.run(FAR[1] + 1, seed=FAR[0], ctx=ctx, log=out.append, parts=("shadow",), only=[FAR[1]], campaign=True)
    assert bad["shadow"] == 0, "\n".join(out[:10])


def test_every_word_count(ctx, oracle):
    """The 65 x 3 crop of the seeded G-buffer - 195 pixels: two workgroups of the lighting kernel, three full waves and a wave of three
    lanes - under the first 32 W - 1 and 32 W of 1024 lights for every W = 3 .. 32: vd_lighting_dev against the twin fed the same words,
    and the in-range words of vd_shadow_gbuffer_dev against the twin of the rule."""
    scene, gb, _ = G.seeded_gbuffer(oracle)
    lts = S.lights(**MANY)
    case = Case(ctx, scene, gb, lts)
    try:
        im = dict(shapes(ctx, case.im))[(65, 3)]
        assert im.n_pixels == 195 and len(im.gb.points()[2]) > 64
        reach = L.rule_words(im.gb, lts)
        assert reach.shape == (195, 32) and all(reach[:, w].any() for w in range(32))
        d_table, table = ctx.upload(L.materials()), L.materials()
        pairs = S.in_range(im.gb.points()[0], lts)
        for W in range(3, 33):
            for n_lights in (32 * W - 1, 32 * W):
                inr = reach[:, :W].copy()
                if n_lights & 31:
                    inr[:, W - 1] &= np.uint32((1 << (n_lights & 31)) - 1)
                occ = L.subset_words(inr, L.SEED, stream=W)
                same(step(ctx, im, case.d_lts, n_lights, inr, occ, d_table), L.shade(im.gb, lts[:n_lights], inr, occ, table), ("lighting", W, n_lights))
                _, got, info = case.run("scene", im, n_lights, max_chunk_rays=0)
                same_words(got, inr, ("in range", W, n_lights))
                assert info["n_points"] == len(im.gb.points()[2]) and info["n_rays"] == int(pairs[:, :n_lights].sum())
    finally:
        case.close()
