"""tests/lighting_cases.py without a GPU: the float32 twin of include/voidin_lighting.h's definition against values worked out by hand
in float64, and the populations of its inputs - what tests/test_gpu_lighting.py relies on when it compares the kernel with the twin
bit for bit: that the order of the lights, the occlusion bit and the specular term each change the bits of most pixels they touch."""
import numpy as np

import gbuffer_cases as G
import lighting_cases as L
import shadow_pass_cases as S
from voidin_amd import abi

F = np.float32


def _one_pixel(eye, word, material=1, depth=1.0):
    """A 1 x 1 G-buffer under clip_to_world with columns (2,0,0,0), (0,4,0,0), (0,0,8,1), (1,2,3,0): its pixel centre is ndc (0, 0), so
    w4 = (1, 2, 8 z + 3, z) and depth 1 puts the point at exactly (1, 2, 11)."""
    cam = np.zeros((), dtype=abi.CAMERA)
    cam["clip_to_world"] = np.asarray([2, 0, 0, 0, 0, 4, 0, 0, 0, 0, 8, 1, 1, 2, 3, 0], F)
    cam["view_position"] = (*eye, 1)
    return G.GBuffer(cam, np.full((1, 1), depth, F), np.array([[[word, 0x1234]]], np.uint32), np.full((1, 1), material, np.uint8))


def _light(position, radius, color):
    lt = np.zeros(1, dtype=abi.LIGHT)
    lt["position"], lt["radius"], lt["color"] = position, radius, color
    return lt


def test_one_light_along_the_normal_at_half_its_radius_against_float64():
    """pos = (1, 2, 11); the normal is the decoded word's; the light stands at pos + nor * 4 with radius 8: s = 0.5, atten = 0.5625 / 1.25,
    shade = 1.  The eye stands at pos - 5 (0.8 nor - 0.6 t) for a tangent t: covr = 0.8.  Occluded and not, for three materials."""
    word = G.AXIS_WORDS[2]
    nor = G.decode_normal([word])[0].astype(np.float64)
    t = np.cross(nor, [1.0, 0.0, 0.0])
    t /= np.linalg.norm(t)
    pos = np.array([1.0, 2.0, 11.0])
    eye = pos - 5.0 * (0.8 * nor - 0.6 * t)
    table = L.materials()
    color = np.array([0.75, 1.5, 0.125])
    lt = _light(pos + nor * 4.0, 8.0, color)
    one = np.ones((1, 1), np.uint32)
    for material in (1, 3, 255):
        gb = _one_pixel(eye, word, material)
        p, n, covr = L.view(gb)
        assert p.tobytes() == np.array([[1, 2, 11]], F).tobytes() and abs(float(covr[0]) - 0.8) < 1e-6
        M = table[material]
        alb, spec, emi = (M[f].astype(np.float64) for f in ("albedo", "specular", "emissive"))
        for occluded, occlusion in ((0, 1.0), (1, 0.5)):
            want = alb * 0.3 + emi + (color * alb * 1.0 + color * spec * 0.8 ** 16) * occlusion * (0.5625 / 1.25)
            got = L.shade(gb, lt, one, one * occluded, table)
            assert got.dtype == F and got.shape == (1, 4) and got[0, 3] == 1
            assert np.abs(got[0, :3] - want).max() < 2e-6 * want.max(), (material, occluded, got, want)
        # the bit decides: without it the base colour, whatever the occluded word says
        base = L.shade(gb, lt, one * 0, one, table)
        assert base[0, :3].tobytes() == ((M["albedo"] * F(0.3)).astype(F) + M["emissive"]).astype(F).tobytes()
        assert L.shade(gb, lt[:0], None, None, table).tobytes() == base.tobytes()


def test_the_materials_that_run_no_loop():
    table = L.materials()
    lt = _light((1, 2, 12), 8.0, (1, 1, 1))
    ones = np.full((1, 1), 0xffffffff, np.uint32)
    assert L.shade(_one_pixel((0, 0, 0), 0x80008000, material=0), lt, ones, ones, table).tobytes() == np.array([[1, 0, 1, 1]], F).tobytes()
    got = L.shade(_one_pixel((0, 0, 0), 0x80008000, material=2), lt, ones, ones, table)
    assert got[0, :3].tobytes() == (table[2]["albedo"] + table[2]["emissive"]).astype(F).tobytes() and got[0, 3] == 1


def test_a_light_at_exactly_its_radius_adds_nothing_and_an_infinite_colour_there_gives_zero():
    assert L.attenuation(F(7.3), F(7.3)) == 0 and L.attenuation(np.nextafter(F(7.3), F(0)), F(7.3)) > 0
    assert L.attenuation(F(1), F(0)) == 0 and np.isnan(L.attenuation(F(1), F(np.nan)))           # s = inf; a NaN stays one
    table = L.materials()
    gb = _one_pixel((1, 2, 30), 0x80008000)                # the point (1, 2, 11), the light 4 above it with radius 4: dist == radius
    one = np.ones((1, 1), np.uint32)
    base = L.shade(gb, _light((1, 2, 15), 4.0, (1, 1, 1))[:0], None, None, table)
    assert L.shade(gb, _light((1, 2, 15), 4.0, (3, 2, 1)), one, one * 0, table).tobytes() == base.tobytes()
    assert (base[0, :3] > 0).all()
    inf = L.shade(gb, _light((1, 2, 15), 4.0, (np.inf, 2, 1)), one, one * 0, table)
    assert inf[0, 0] == 0 and inf[0, 1:].tobytes() == base[0, 1:].tobytes()      # inf * 0 is a NaN, and the clamp makes it 0
    assert np.isfinite(L.shade(gb, _light((1, 2, 15), np.nan, (1, 1, 1)), one, one, table)).all()


def test_c16_against_the_sixteenth_power():
    """Four squarings, each rounded once: the relative error at most doubles and gains half an ulp per step - 15 * 2^-24 in all."""
    x = np.linspace(0.2, 1.0, 4001).astype(F)
    got = L.pow16(x).astype(np.float64)
    want = x.astype(np.float64) ** 16
    assert (np.abs(got - want) <= 16 * 2.0 ** -24 * want).all() and L.pow16(F(1)) == 1 and L.pow16(F(0)) == 0
    assert L.pow16(F(0.5)) == F(2.0 ** -16)


def test_populations_of_the_seeded_image(oracle):
    """65 lights on the seeded 64 x 64 G-buffer, the bits the pass gives (the twin of the rule, the oracle's any-hit): summing in
    descending order, and ignoring the occlusion bit, each change the bits of at least half of the receivers' colours."""
    scene, gb, _ = G.seeded_gbuffer(oracle)
    lts, table = S.lights(), L.materials()
    occ, inr, w = L.pass_words(oracle, "seeded", scene, gb, lts)
    recv = G.receivers(gb.material).reshape(-1)
    n = int(recv.sum())
    assert n > 1500 and w.n_rays > 30 * n and 2 * int(w.occluded.sum()) > w.n_rays
    got = L.shade(gb, lts, inr, occ, table)
    assert np.isfinite(got).all() and (got >= 0).all() and (got[:, 3] == 1).all()
    assert (got[gb.material.reshape(-1) == 0] == (1, 0, 1, 1)).all()
    down = L.changed(got, L.shade(gb, lts, inr, occ, table, descending=True))
    free = L.changed(got, L.shade(gb, lts, inr, occ, table, ignore_occlusion=True))
    assert not down[~recv].any() and not free[~recv].any()
    print(f"receivers {n}, pairs in range {w.n_rays}, occluded {int(w.occluded.sum())}; changed by descending order {int(down.sum())}, by ignoring occlusion {int(free.sum())}")
    assert 2 * int(down.sum()) >= n and 2 * int(free.sum()) >= n, (n, int(down.sum()), int(free.sum()))
    # the seeded image's normals face the eye: the specular factor is 0 on every pixel
    assert (L.view(gb)[2][recv] == 0).all()


def test_populations_of_the_flipped_image(oracle):
    """With every third receiver's normal turned round, at least a quarter of the receivers have covr > 0, and zeroing `specular`
    changes the bits of at least half of those."""
    scene, gb = L.flipped_gbuffer(oracle)
    _, seeded, _ = G.seeded_gbuffer(oracle)
    assert gb.material.tobytes() == seeded.material.tobytes() and gb.depth.tobytes() == seeded.depth.tobytes()
    assert int((gb.normal_uv[:, :, 0] != seeded.normal_uv[:, :, 0]).sum()) > 500 and gb.normal_uv[:, :, 1].tobytes() == seeded.normal_uv[:, :, 1].tobytes()
    lts, table = S.lights(), L.materials()
    recv = G.receivers(gb.material).reshape(-1)
    n = int(recv.sum())
    covr = L.view(gb)[2]
    facing = recv & (covr > 0)
    inr = L.rule_words(gb, lts)
    occ = L.subset_words(inr, L.SEED)
    got = L.shade(gb, lts, inr, occ, table)
    dull = table.copy()
    dull["specular"] = 0
    diff = L.changed(got, L.shade(gb, lts, inr, occ, dull))
    assert not diff[~facing].any()
    print(f"receivers {n}, covr > 0 on {int(facing.sum())}, changed by specular = 0: {int(diff.sum())}")
    assert 4 * int(facing.sum()) >= n and 2 * int(diff.sum()) >= int(facing.sum()), (n, int(facing.sum()), int(diff.sum()))
    assert (occ & ~inr == 0).all() and 0 < int((occ != 0).sum()) and occ.tobytes() != inr.tobytes()      # a proper subset of the bits
