"""The rounds of the shading chain's kernels that no other test reaches.

a. gbuffer_scan_kernel (voidin_amd/csrc/gbuffer.hip) scans 4 096 tile counts a round and carries a total from round to round; a
   tile is 512 pixels.  A 2047 x 1025 image has 4 098 tiles, the last one partial: round 2 holds two counts and its guard is live.
b. gbuffer_scatter_kernel writes W words a pixel, owner = j / words: vd_shadow_gbuffer*_dev at W = 4, 5, 8, 31, 32.
c. lighting_kernel stages the bit words of a wave through LDS when W > 2, 256 words a round, at stride W | 1: vd_lighting_dev at
   W = 4, 5, 8, 9, 31, 32 on shapes whose last wave is partial.
d. Bit arrays and lights that start 4 bytes (one 32-byte record) past a 256-byte boundary: legal pointers of their element types.
Everything is compared byte for byte with the twins of tests/*_cases.py, between canaries."""
import numpy as np
import pytest

import gbuffer_cases as G
import lighting_cases as L
import shadow_pass_cases as S
from test_gpu_lighting import Target, same as same_colour
from test_gpu_shadow_gbuffer import Case, Images, check_points, same, shapes
from voidin_amd import synth
from write_set import FILL

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
SEED = synth.SEED_BASE + 131
N_LIGHTS_SHADOW = (97, 129, 225, 961, 1024)                 # W = 4, 5, 8, 31, 32
N_LIGHTS_LIGHTING = (97, 129, 225, 257, 961, 1024)          # W = 4, 5, 8, 9, 31, 32
CROPS = ((1, 1), (65, 3), (17, 31), (64, 9))
SHAPES = ((1, 1), (63, 1), (65, 3), (17, 31), (64, 9))


def many_lights(n):
    """tests/test_gpu_shadow_pass.py's test_the_most_lights_a_call_takes: the 65 seeded lights over and over, every copy with its radii
    scaled differently - the any-hit answer of light l is that of seeded light l % 65."""
    lts = S.lights()[np.arange(n) % S.N_LIGHTS].copy()
    lts["radius"] = (lts["radius"] * (F(0.55) + F(0.06) * (np.arange(n) // S.N_LIGHTS).astype(F))).astype(F)
    return lts


@pytest.fixture(scope="module")
def seeded(ctx, oracle):
    scene, gb, _ = G.seeded_gbuffer(oracle)
    c = Case(ctx, scene, gb, many_lights(1024))
    yield c
    c.close()


@pytest.fixture(scope="module")
def d_table(ctx):
    return ctx.upload(L.materials())


@pytest.fixture(scope="module")
def crops(ctx, seeded):
    """The layouts of test_gpu_shadow_gbuffer.shapes() that these tests name, uploaded once: every one of CROPS and SHAPES is there."""
    offered = dict(shapes(ctx, seeded.im))
    wanted = sorted(set(CROPS) | set(SHAPES))
    assert set(wanted) <= set(offered), sorted(set(wanted) - set(offered))
    return {name: offered[name] for name in wanted}


# ---- a. the tile scan's second round -----------------------------------------------------------------------------------------------------

BIG_W, BIG_H = 2047, 1025
BIG_PITCHES = (4 * BIG_W + 12, 8 * BIG_W + 24, BIG_W + 4)
N_BIG = 3000


def big_gbuffer(oracle):
    """2047 x 1025 pixels of material 0 but for 3 000 receivers, each with the (depth, normal word, material) of a receiver of the
    seeded G-buffer, placed by a fixed seed: 2 740 anywhere before tile 4 096 (one each forced into tiles 0 and 4 095), 260 in the
    1 023 pixels of tiles 4 096 and 4 097 (the first and the last pixel of the image's tail among them)."""
    _, small, _ = G.seeded_gbuffer(oracle)
    src = small.points()[2]
    n = BIG_W * BIG_H
    tail = 4096 * G.TILE
    order = lambda stream, count: np.argsort(synth.uniform01(SEED, stream, count), kind="stable")
    head = order(0, tail)[: N_BIG - 260 - 2]
    at = np.unique(np.concatenate([head, [5, 4095 * G.TILE + 17], tail + order(1, n - tail)[:258], [tail, n - 1]]))
    take = src[(np.arange(len(at)) * 7) % len(src)]
    depth, words, material = np.zeros(n, F), np.zeros((n, 2), U), np.zeros(n, np.uint8)
    depth[at], words[at], material[at] = small.depth.reshape(-1)[take], small.normal_uv.reshape(-1, 2)[take], small.material.reshape(-1)[take]
    return G.GBuffer(small.cam, depth.reshape(BIG_H, BIG_W), words.reshape(BIG_H, BIG_W, 2), material.reshape(BIG_H, BIG_W))


def test_the_tile_scans_second_round(ctx, oracle, seeded):
    """vd_gbuffer_points_dev equals GBuffer.points() - count, pixel ids, positions, normals - between canaries; vd_shadow_gbuffer_dev
    with 33 lights: the in-range words are the twin's, the occluded words the composition's (the GPU's points, vd_shadow_pass_dev, a
    scatter in numpy) and, on every 16th receiver, the oracle's any-hit answer."""
    gb = big_gbuffer(oracle)
    assert gb.width * gb.height == 2098175 and -(-gb.width * gb.height // G.TILE) == 4098
    pos, nor, pix = gb.points()
    tile = pix // G.TILE
    assert {0, 4095, 4096, 4097} <= set(tile.tolist()) and (tile < 4096).sum() > 2000 and (tile >= 4096).sum() >= 200, np.bincount(tile >= 4096)
    assert len(pix) > 2900 and pix[-1] == gb.width * gb.height - 1
    big = Case.__new__(Case)
    big.ctx, big.rig, big.lts, big.d_lts = ctx, seeded.rig, S.lights()[:33], ctx.upload(S.lights()[:33])
    big.im = Images(ctx, gb, BIG_PITCHES)
    assert check_points(ctx, big.im, "2047 x 1025") == len(pix)
    occ, inr, info = big.run("scene", big.im, 33)
    reach = S.in_range(pos, big.lts)
    same(inr, G.scatter(gb, S.pack(reach)), "in range")
    c_occ, c_inr, c_info = big.composition("scene", big.im, 33)
    same(occ, c_occ, "occluded, against the composition")
    same(inr, c_inr, "in range, against the composition")
    assert info["n_points"] == c_info["n_points"] == len(pix) and info["n_rays"] == c_info["n_rays"] == int(reach.sum()), (info, c_info)
    k = np.arange(0, len(pix), 16)
    hit = S.any_hit(oracle, ("rounds", "big"), seeded.rig.scene, pos[k], nor[k], big.lts, False)
    same(occ[pix[k]], S.pack(reach[k] & hit), "occluded, every 16th receiver against the oracle")
    assert (reach[k] & hit).sum() > 500


# ---- b. W words a pixel through the scatter ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_lights", N_LIGHTS_SHADOW)
def test_the_pass_at_more_than_three_words_a_pixel(ctx, oracle, seeded, crops, n_lights):
    """Crops 1 x 1, 65 x 3, 17 x 31 and 64 x 9 of the seeded G-buffer: both outputs against the CPU expectation (the twin's reach, the
    oracle's any-hit answer of light l % 65) and against the composition on the GPU."""
    lts = seeded.lts[:n_lights]
    W = (n_lights + 31) // 32
    assert W > 3
    forms = ("scene", "prepared", "wide", "tight")
    for j, name in enumerate(CROPS):
        im = crops[name]
        form = forms[(j + W) % 4]
        pos, nor, pix = im.gb.points()
        base = S.any_hit(oracle, ("rounds",) + name, seeded.rig.scene, pos, nor, S.lights(), False) if len(pix) else np.zeros((0, S.N_LIGHTS), bool)
        w = S.Want(S.in_range(pos, lts), base[:, np.arange(n_lights) % S.N_LIGHTS])
        occ, inr, info = seeded.run(form, im, n_lights)
        same(inr, G.scatter(im.gb, w.in_range_words), (form, name, n_lights, "in range"))
        same(occ, G.scatter(im.gb, w.occluded_words), (form, name, n_lights, "occluded"))
        c_occ, c_inr, c_info = seeded.composition(form, im, n_lights)
        same(occ, c_occ, (form, name, n_lights, "occluded, against the composition"))
        same(inr, c_inr, (form, name, n_lights, "in range, against the composition"))
        assert info["words_per_point"] == W and (info["n_points"], info["n_rays"]) == (c_info["n_points"], c_info["n_rays"]) == (len(pix), w.n_rays)


# ---- c. the staging rounds of the lighting kernel ------------------------------------------------------------------------------------------

def staging(W, pixels):
    """-> (rounds of the image's last wave, its last round is ragged, the wave is partial): the wave stages min(64, pixels left) * W
    words, 256 a round."""
    left = pixels - 64 * ((pixels - 1) // 64)
    run = left * W
    return -(-run // 256), run % 256 != 0, left < 64


def lighting_inputs(im, lts, stream):
    inr = L.rule_words(im.gb, lts)
    return inr, L.subset_words(inr, L.SEED, stream=stream)


def offset_upload(a, offset):
    """The bytes of `a` on the device `offset` bytes past a 256-byte boundary, over a prefill -> (the view, the whole allocation)."""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    whole = torch.full((offset + len(raw) + 256,), FILL, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 256 == 0
    whole[offset: offset + len(raw)].copy_(torch.from_numpy(raw.copy()))
    return whole[offset: offset + len(raw)], whole


def fill_intact(whole, offset, nbytes):
    host = whole.cpu().numpy()
    return bool((host[:offset] == FILL).all() and (host[offset + nbytes:] == FILL).all())


@pytest.mark.parametrize("n_lights", N_LIGHTS_LIGHTING)
def test_the_lighting_step_at_more_than_three_words_a_pixel(ctx, oracle, seeded, crops, d_table, n_lights):
    """vd_lighting_dev byte for byte against lighting_cases.shade, fed the rule's bit words and a seeded subset of them as occlusion.
    Staging rounds of the LAST wave (rounds, r = its last round is ragged, p = the wave is partial):

        W    1 x 1    63 x 1    65 x 3    17 x 31    64 x 9
        4    1 r p    1 r p     1 r p     1 r p      1
        5    1 r p    2 r p     1 r p     1 r p      2 r
        8    1 r p    2 r p     1 r p     1 r p      2
        9    1 r p    3 r p     1 r p     1 r p      3 r
       31    1 r p    8 r p     1 r p     2 r p      8 r
       32    1 r p    8 r p     1 r p     2 r p      8

    (63 x 1 is one partial wave of 63 pixels; 65 x 3 ends on 3 pixels, 17 x 31 on 15; the full waves in front of a last one stage
    64 W words: 1, 2, 2, 3, 8 and 8 rounds, ragged at W = 5, 9 and 31.)"""
    lts = seeded.lts[:n_lights]
    W = (n_lights + 31) // 32
    table = L.materials()
    rounds = {name: staging(W, name[0] * name[1]) for name in SHAPES}
    assert rounds[(1, 1)] == (1, True, True) and rounds[(64, 9)] == (-(-64 * W // 256), (64 * W) % 256 != 0, False)
    if W in (5, 8, 9, 31, 32):
        assert rounds[(63, 1)][0] >= 2 and rounds[(63, 1)][1:] == (True, True)        # several rounds, a ragged last one, a partial wave
    d_lts = ctx.upload(lts)
    lit = 0
    for name in SHAPES:
        im = crops[name]
        assert (im.gb.width, im.gb.height) == name
        inr, occ = lighting_inputs(im, lts, stream=n_lights)
        assert inr.shape == (name[0] * name[1], W)
        tg = Target(im.gb.width, im.gb.height)
        ctx.lighting_dev(im.gb.cam, im.c, d_lts, n_lights, ctx.upload(occ), ctx.upload(inr), d_table, tg.t)
        same_colour(tg.read(), L.shade(im.gb, lts, inr, occ, table), (name, n_lights))
        lit += int(inr[:, 3:].any())
    assert lit >= 3                                           # the words beyond the third held bits


# ---- d. element alignment ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_lights", (33, 129))
def test_the_lighting_step_takes_arrays_at_their_elements_alignment(ctx, oracle, seeded, crops, d_table, n_lights):
    """W = 2 and W = 5 on the 17 x 31 crop: both bit arrays 4 bytes past a 256-byte boundary, the lights one 32-byte record past one -
    the bytes of the aligned call, and nothing around the arrays written."""
    im = crops[(17, 31)]
    lts = seeded.lts[:n_lights]
    inr, occ = lighting_inputs(im, lts, stream=n_lights + 1)
    tg = Target(17, 31)
    ctx.lighting_dev(im.gb.cam, im.c, ctx.upload(lts), n_lights, ctx.upload(occ), ctx.upload(inr), d_table, tg.t)
    aligned = tg.read()
    same_colour(aligned, L.shade(im.gb, lts, inr, occ, L.materials()), ("aligned", n_lights))
    (d_inr, w_inr), (d_occ, w_occ), (d_lts, w_lts) = offset_upload(inr, 4), offset_upload(occ, 4), offset_upload(lts, 32)
    assert d_inr.data_ptr() % 256 == 4 and d_occ.data_ptr() % 256 == 4 and d_lts.data_ptr() % 256 == 32
    tg = Target(17, 31)
    ctx.lighting_dev(im.gb.cam, im.c, d_lts, n_lights, d_occ, d_inr, d_table, tg.t)
    same_colour(tg.read(), aligned, ("4 bytes past a 256-byte boundary", n_lights))
    assert fill_intact(w_inr, 4, inr.nbytes) and fill_intact(w_occ, 4, occ.nbytes) and fill_intact(w_lts, 32, lts.nbytes)
    assert d_inr.cpu().numpy().tobytes() == inr.tobytes() and d_occ.cpu().numpy().tobytes() == occ.tobytes()


def test_the_pass_writes_arrays_at_their_elements_alignment(ctx, oracle, seeded, crops):
    """vd_shadow_gbuffer_dev at W = 5 on the 17 x 31 crop: both outputs 4 bytes past a 256-byte boundary, the lights one record past
    one - the words of the aligned call; the bytes in front of and behind the outputs keep their prefill."""
    import torch
    n_lights, W = 129, 5
    im = crops[(17, 31)]
    occ, inr, info = seeded.run("scene", im, n_lights)
    words = im.n_pixels * W
    outs = [torch.full((4 + words * 4 + 256,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_lts, w_lts = offset_upload(seeded.lts[:n_lights], 32)
    assert all(o.data_ptr() % 256 == 0 for o in outs) and d_lts.data_ptr() % 256 == 32
    info2 = ctx.shadow_gbuffer_dev(seeded.rig.ds, im.gb.cam, im.c, d_lts, n_lights, outs[0][4:], outs[1][4:])
    torch.cuda.synchronize()
    for o, wanted, what in zip(outs, (occ, inr), ("occluded", "in range")):
        assert fill_intact(o, 4, words * 4), what
        same(o.cpu().numpy()[4: 4 + words * 4].copy().view(U).reshape(im.n_pixels, W), wanted, what)
    assert info2 == info and fill_intact(w_lts, 32, 32 * n_lights)
