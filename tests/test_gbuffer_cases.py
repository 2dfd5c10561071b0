"""tests/gbuffer_cases.py without a GPU: the float32 twin of include/voidin_gbuffer.h's definition against values worked out by hand,
the octahedral encoding's round trip, and the populations of the seeded and the hand-made G-buffer - what tests/test_gpu_shadow_gbuffer.py
relies on when it compares the kernels with the twin."""
import numpy as np

import gbuffer_cases as G
from voidin_amd import abi, synth

F = np.float32


def _camera(clip_to_world):
    cam = np.zeros((), dtype=abi.CAMERA)
    cam["clip_to_world"] = np.asarray(clip_to_world, F).reshape(16)
    return cam


def test_position_against_hand_values():
    """clip_to_world with columns (2,0,0,0), (0,4,0,0), (0,0,8,1), (1,2,3,0): w4 = (2x + 1, 4y + 2, 8z + 3, z).  A 2 x 2 image has its
    pixel centres at uv 0.25 / 0.75, ndc -0.5 / 0.5 with y flipped; every value below is exact in float32."""
    cam = _camera([2, 0, 0, 0, 0, 4, 0, 0, 0, 0, 8, 1, 1, 2, 3, 0])
    pos = G.world_position(cam, [0, 1, 0, 1], [0, 0, 1, 1], 2, 2, [0.5, 0.25, 2.0, 1.0])
    want = np.array([[(2 * -0.5 + 1) / 0.5, (4 * 0.5 + 2) / 0.5, (8 * 0.5 + 3) / 0.5],
                     [(2 * 0.5 + 1) / 0.25, (4 * 0.5 + 2) / 0.25, (8 * 0.25 + 3) / 0.25],
                     [(2 * -0.5 + 1) / 2.0, (4 * -0.5 + 2) / 2.0, (8 * 2.0 + 3) / 2.0],
                     [(2 * 0.5 + 1) / 1.0, (4 * -0.5 + 2) / 1.0, (8 * 1.0 + 3) / 1.0]], F)
    assert pos.dtype == F and pos.tobytes() == want.tobytes(), (pos, want)
    # 3 x 5: centres that are not dyadic - the float32 steps one by one, in Python floats rounded after every operation
    x, y, d = 2, 3, F(0.3)
    ux, uy = F(F(x + 0.5) / F(3)), F(F(y + 0.5) / F(5))
    nx, ny = F(F(ux * F(2)) - F(1)), F(F(F(F(1) - uy) * F(2)) - F(1))
    w = [F(F(F(F(2) * nx) + F(F(0) * ny)) + F(F(0) * d)) + F(1), F(F(F(F(0) * nx) + F(F(4) * ny)) + F(F(0) * d)) + F(2),
         F(F(F(F(0) * nx) + F(F(0) * ny)) + F(F(8) * d)) + F(3), F(F(F(F(0) * nx) + F(F(0) * ny)) + F(F(1) * d)) + F(0)]
    want = np.array([[F(w[0] / w[3]), F(w[1] / w[3]), F(w[2] / w[3])]], F)
    assert G.world_position(cam, [x], [y], 3, 5, [d]).tobytes() == want.tobytes()
    # depth 0 under this matrix: w = 0 - the divisions give infinities and, where the numerator is 0 too, a NaN
    with np.errstate(all="ignore"):
        p = G.world_position(cam, [0], [0], 2, 2, [0.0])[0]
    assert np.isnan(p[0]) and p[1] == np.inf and p[2] == np.inf


def _decode64(word):
    d = np.array([word & 0xffff, (word >> 16) & 0xffff], np.float64) / 65535.0 * 2 - 1
    n = np.array([d[0], d[1], 1 - abs(d[0]) - abs(d[1])])
    t = max(-n[2], 0.0)
    n[0] += -t if n[0] > 0 else t
    n[1] += -t if n[1] > 0 else t
    return n / np.linalg.norm(n)


def test_normal_against_hand_values():
    # the corners of the code square all fold onto the south pole: v = (+-1, +-1), n.z = -1, t = 1, x and y fall to 0
    for word in (0, 0xffffffff, 0x0000ffff, 0xffff0000):
        assert G.decode_normal([word]).tobytes() == np.array([[0, 0, -1]], F).tobytes(), hex(word)
    # the codes next to the centre: v = (+-1, -+1) / 65535 up to rounding, n.z = 1 - 2 / 65535
    for word, sx, sy in ((0x7fff8000, 1, -1), (0x80007fff, -1, 1)):
        n = G.decode_normal([word])[0]
        e = 1 / 65535
        want = np.array([sx * e, sy * e, 1 - 2 * e]) / np.sqrt(2 * e * e + (1 - 2 * e) ** 2)
        assert np.abs(n - want).max() < 1e-7 and np.sign(n[0]) == sx and np.sign(n[1]) == sy, (hex(word), n, want)
    # the four normals of the equator: n.z one code step below zero, the fold taken with every sign
    for word, want in zip(G.AXIS_WORDS, ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0))):
        n = G.decode_normal([word])[0]
        assert np.abs(n - np.array(want)).max() < 2e-5 and n[2] < 0, (hex(word), n)
    assert G.encode_normal(np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)], F)).tolist() == list(G.AXIS_WORDS)
    # 2 000 seeded words against the same steps in float64
    words = (synth.uniform01(G.SEED, 7, 2000) * 2.0 ** 32).astype(np.uint64).astype(np.uint32)
    got = G.decode_normal(words)
    assert got.dtype == F and max(np.abs(got[k] - _decode64(int(w))).max() for k, w in enumerate(words)) < 1e-6


def test_no_word_decodes_to_nz_exactly_zero():
    """n.z = (1 - |v.x|) - |v.y| over all 65 536 x 65 536 code pairs in the twin's float32 steps: never 0 (the exact sum would need a
    half-integer code).  So the hand-made G-buffer takes the equator's four encodings for `the words where n.z == 0`."""
    code = np.arange(65536, dtype=np.uint32)
    v = np.abs((((code.astype(F) / F(65535)).astype(F) * F(2)).astype(F) - F(1)).astype(F))
    assert not np.isin((F(1) - v).astype(F), v).any()
    assert (G.decode_normal(code << np.uint32(16) | code[::-1])[:, 2] != 0).all()


def test_encoding_round_trip():
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], F)
    u = synth.uniform01(G.SEED, 5, 3000).reshape(1000, 3)
    z, phi = 2 * u[:, 0] - 1, 2 * np.pi * u[:, 1]
    r = np.sqrt(1 - z * z)
    n = np.concatenate([axes, np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(F)])
    back = G.decode_normal(G.encode_normal(n))
    assert np.abs(back - n).max() < 2e-4, float(np.abs(back - n).max())
    assert (n[:, 2] < -0.5).sum() > 100 and (n[:, 2] > 0.5).sum() > 100       # both hemispheres: the fold and the plain half


def test_seeded_populations(oracle):
    scene, gb, hit = G.seeded_gbuffer(oracle)
    assert (gb.width, gb.height) == (64, 64)
    recv = G.receivers(gb.material).reshape(-1)
    assert 0.25 * 4096 < recv.sum() < 0.75 * 4096, int(recv.sum())
    material, depth = gb.material.reshape(-1), gb.depth.reshape(-1)
    assert (material[hit] == G.LIGHT_MATERIAL).sum() >= 50                                    # a light's own surface
    assert ((material == G.NO_MATERIAL) & hit & (depth != 0)).sum() >= 50                     # no material over a real depth
    assert ((material == G.NO_MATERIAL) & ~hit & (depth == 0)).sum() >= 50                    # the sky
    per_tile = recv.reshape(-1, G.TILE).sum(axis=1)
    assert per_tile[G.FULL_TILE] == G.TILE and per_tile[G.EMPTY_TILE] == 0, per_tile
    assert set(np.unique(material)) == {0, 1, 2, 3, 255}
    assert (gb.normal_uv[:, :, 1] != 0).all()
    # the points: in pixel order, and where a pixel hit something its position is the hit point again (the depth is that point's,
    # rounded to float32: at 15-60 units from the eye under znear = 0.001 the round trip keeps about 1e-5)
    pos, nor, pix = gb.points()
    assert len(pix) == recv.sum() and (np.diff(pix.astype(np.int64)) > 0).all() and pos.dtype == nor.dtype == F
    rays = G.centre_rays(gb.cam, 64, 64)
    rec, _ = oracle.trace(scene, rays, threads=8)
    at = hit[pix]
    want = rays["eye"][pix[at]].astype(np.float64) + rays["dir"][pix[at]].astype(np.float64) * rec["dist"][pix[at]].astype(np.float64)[:, None]
    assert np.abs(pos[at] - want).max() < 1e-3, float(np.abs(pos[at] - want).max())
    assert np.isinf(pos[~at]).any(axis=1).all() and not np.isnan(pos).any()                   # depth 0: at infinity
    assert np.abs(np.linalg.norm(nor[at].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert ((nor[at] * (rays["eye"][pix[at]] - pos[at])).sum(axis=1) > 0).all()               # facing the eye


def test_seeded_rows_and_crops(oracle):
    _, gb, _ = G.seeded_gbuffer(oracle)
    d, n, m, pitches = gb.rows(G.DEPTH_PITCH, G.NORMAL_UV_PITCH, G.MATERIAL_PITCH)
    assert pitches == (512, 768, 77) and (len(d), len(n), len(m)) == (64 * 512, 64 * 768, 64 * 77)
    assert d.reshape(64, 512)[:, :256].tobytes() == gb.depth.tobytes() and (d.reshape(64, 512)[:, 256:] == 0xC3).all()
    assert m.reshape(64, 77)[:, :64].tobytes() == gb.material.tobytes()
    c = gb.crop(17, 31)
    cd, cn, cm, _ = c.rows(G.DEPTH_PITCH, G.NORMAL_UV_PITCH, G.MATERIAL_PITCH)
    assert cd.reshape(31, 512)[:, : 4 * 17].tobytes() == d.reshape(64, 512)[:31, : 4 * 17].tobytes()      # the same pixels at the same pitches
    assert cm.reshape(31, 77)[:, :17].tobytes() == m.reshape(64, 77)[:31, :17].tobytes() and len(cn) == 31 * 768
    pos, nor, pix = c.points()
    full = gb.points()
    x, y = pix % 17, pix // 17
    keep = np.isin(full[2], y * 64 + x)
    assert keep.sum() == len(pix) and nor.tobytes() == full[1][keep].tobytes()              # the same words decode the same
    assert G.scatter(c, np.arange(len(pix), dtype=np.uint32)[:, None] + 1).reshape(31, 17)[y, x].tolist() == list(range(1, len(pix) + 1))


def test_hand_made_has_every_case(oracle):
    _, gb, lts = G.hand_gbuffer(oracle)
    assert (gb.width, gb.height) == (4, 3) and len(lts) == 13
    depth, words, material = gb.depth.reshape(-1), gb.normal_uv.reshape(-1, 2)[:, 0], gb.material.reshape(-1)
    recv = G.receivers(material)
    assert recv.sum() == 10 and set(material.tolist()) == {0, 1, 2, 3, 255}
    d = depth[recv]
    assert (d == 0).sum() == 1 and np.isnan(d).sum() == 1 and np.isposinf(d).sum() == 1 and (d == 1).sum() == 1
    assert {0, 0xffffffff, 0x7fff8000, 0x80007fff, *G.AXIS_WORDS} <= set(words[recv].tolist())
    pos, nor, pix = gb.points()
    assert pix.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]
    assert np.isinf(pos[0]).all() and np.isnan(pos[1]).all() and np.isnan(pos[2]).all() and np.isfinite(pos[3:]).all()
    assert np.abs(pos[4:, 2]).max() < 1e-4 and not np.isnan(nor).any()                        # the ordinary depths: about the z = 0 plane
