"""The twin of tests/gbuffer_trace_cases.py, without a GPU: against hand values, its octahedral encoder against
gbuffer_cases.encode_normal, its f16 packing against numpy.float16, its restated Moeller-Trumbore against the oracle's distances; the
populations the GPU tests rely on; and the round trip depth -> world position that bounds the end-to-end test.
(With a device: tests/test_gpu_gbuffer_trace.py.)"""
import numpy as np

import gbuffer_cases as G
import gbuffer_trace_cases as T
from voidin_amd import abi, synth

F, U = np.float32, np.uint32

# The round trip of test_depth_round_trips_to_the_hit_point: the twin's maximum over the hit pixels of the seeded 64 x 64 image,
# measured on the CPU, and the bound the tests assert - 4 x that maximum (the margin covers the smaller crops, whose pixel centres
# differ).
ROUND_TRIP_MEASURED = 4.54e-7
ROUND_TRIP_BOUND = 4 * ROUND_TRIP_MEASURED


def round_trip_error(img, eye):
    """max over the hit pixels of |world_position(depth) - p| / |p - eye| (float64 arithmetic on the float32 values)."""
    k = np.flatnonzero(img.branch == T.HIT)
    pos = G.world_position(img.cam, k % img.width, k // img.width, img.width, img.height, img.depth[k]).astype(np.float64)
    p, e = img.p[k].astype(np.float64), eye[k].astype(np.float64)
    return float((np.linalg.norm(pos - p, axis=1) / np.linalg.norm(p - e, axis=1)).max())


def test_the_hand_rays_are_the_hand_values():
    """Every pixel of the hand-made camera has eye = (0, 0, 5), dir = (0, 0, -1) exactly, the pads 0 and VD_MAX_DIST; under a real
    camera the centre ray of an odd image points along the view direction and the rays of a row are mirror images."""
    r = T.rays(T.hand_camera(), 7, 3)
    assert (r["eye"] == (0, 0, 5)).all() and (r["dir"] == (0, 0, -1)).all() and (r["_pad0"] == 0).all() and (r["_pad1"] == F(1e30)).all()
    cam = synth.camera_uniform(**G.CAMERA)
    r = T.rays(cam, 5, 5)
    np.testing.assert_allclose(r["dir"][12], (0, 0, -1), atol=1e-6)
    np.testing.assert_allclose(r["eye"][12], (0, 2.5, 40 - 0.001), atol=1e-4)
    np.testing.assert_allclose(r["dir"][10] * (-1, 1, 1), r["dir"][14], atol=1e-6)
    assert r["dir"][2][1] > 0 > r["dir"][22][1]                      # row 0 is the top
    np.testing.assert_allclose(np.linalg.norm(r["dir"].astype(np.float64), axis=1), 1, atol=1e-6)


def test_every_hand_case_takes_its_branch_and_gives_its_hand_values():
    geo, cam, rec, C = T.hand()
    n = len(C)
    img, geom = T.resolve(cam, geo, rec, n, 1), T.resolve(cam, geo.without(), rec, n, 1)
    for i, c in enumerate(C):
        assert img.branch[i] == geom.branch[i] == c.branch, (c.name, img.branch[i])
        if c.branch != T.HIT:
            for im in (img, geom):
                assert im.depth[i].view(U) == 0 and (im.words[i] == 0).all() and im.material[i] == 0, c.name
            continue
        e = c.expect
        assert geom.words[i, 1] == 0, c.name                           # no uvs: word 1 is 0
        assert img.t[i] == c.record["dist"], (c.name, img.t[i])          # the records' distances are the triangles' own
        if "u" in e:
            assert (img.u[i], img.v[i]) == (e["u"], e["v"]), c.name
        if "material" in e:
            assert img.material[i] == geom.material[i] == e["material"], c.name
        if "word0" in e:
            assert img.words[i, 0] == e["word0"], (c.name, hex(img.words[i, 0]))
        if "geometric" in e:
            assert geom.words[i, 0] == e["geometric"], (c.name, hex(geom.words[i, 0]))
        if "x_code" in e:
            assert (img.words[i, 0] & 0xffff, img.words[i, 0] >> 16) == (e["x_code"], e["y_code"]), (c.name, hex(img.words[i, 0]))
        if e.get("depth_not_finite"):
            assert not np.isfinite(img.depth[i]) and not np.isfinite(geom.depth[i]), c.name
        else:
            assert img.depth[i] == F(T.ZNEAR / (c.record["dist"] - T.EYE_Z)), (c.name, img.depth[i])      # clip.z / clip.w = ZNEAR / -z
        if e.get("skew"):
            mat3 = T.encode(T.normalise(np.array([[0, 4, 1]], F)))[0]
            inverse_transpose = T.encode(T.normalise(np.array([[0, 0.25, 1]], F)))[0]
            assert img.words[i, 0] == mat3 != inverse_transpose, c.name
        if "uv" in e:
            value, rne, rtz = e["uv"]
            lo, hi = int(img.words[i, 1]) & 0xffff, int(img.words[i, 1]) >> 16
            if rne is None:
                assert lo & 0x7fff > 0x7c00 and hi & 0x7fff > 0x7c00, c.name
            else:
                assert lo == rne and hi == rne ^ 0x8000, (c.name, hex(lo), hex(hi))
    # the plain hit's uv: (1/4, 1/2) * 1/4 = (1/16, 1/8)
    i = [c.name for c in C].index("plain hit, u = 1/4, v = 1/2")
    assert img.words[i, 1] == (int(np.float16(0.125).view(np.uint16)) << 16 | int(np.float16(0.0625).view(np.uint16)))
    # the list holds halfway cases that tell the two roundings apart
    assert sum(1 for c in C if "uv" in c.expect and c.expect["uv"][1] is not None and c.expect["uv"][1] != c.expect["uv"][2]) >= 4
    assert {c.branch for c in C} == set(range(7))


def test_the_encoder_equals_the_g_buffer_helpers_bit_for_bit():
    """10^5 seeded unit normals, the poles and the axes: the twin's encoder (which clamps and sends a NaN to 0) and
    gbuffer_cases.encode_normal (which does neither) give the same word; a normal of length zero, and a NaN, encode as 0."""
    u = synth.uniform01(T.SEED, 7, 300000).reshape(-1, 3) * 2 - 1
    n = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(F)
    n = np.concatenate([n, np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0.6, -0.8], [-0.6, 0, -0.8]], F)])
    assert (T.encode(n) == G.encode_normal(n)).all()
    assert T.encode(np.array([[0, 0, 1]], F))[0] == 0x80008000 and T.encode(np.array([[0, 0, -1]], F))[0] == 0xffffffff
    # 0 / 0 and a NaN sum make every quotient a NaN; inf / inf makes x alone one: its code is 0, y's the code of 0
    assert (T.encode(np.array([[0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0]], F)) == (0, 0, 0x80000000)).all()


def test_the_f16_packing_equals_numpy_float16():
    edge = np.array([e[0] for e in T.UV_EDGES if e[1] is not None], F)
    u = synth.uniform01(T.SEED, 8, 200000)
    many = np.concatenate([edge, -edge, (u * 131072 - 65536).astype(F), ((u - 0.5) * 2.0 ** -13).astype(F), (u * 4 - 2).astype(F),
                           np.array([65519.996, 65520.004, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12), 6.1e-5, 5.96e-8, 2.98e-8, 2.9e-8], F)])
    with np.errstate(over="ignore"):
        want = many.astype(np.float16).view(np.uint16).astype(U)
    got = T.f16_bits(many)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (many[bad[:4]].tolist(), [hex(int(x)) for x in got[bad[:4]]], [hex(int(x)) for x in want[bad[:4]]])
    for value, rne, _ in T.UV_EDGES:
        bits = int(T.f16_bits(np.array([value], F))[0])
        assert bits == rne if rne is not None else bits & 0x7fff > 0x7c00, value
    assert T.pack_uv(np.array([[1.0, -2.0]], F))[0] == 0xc0003c00


def test_the_restated_intersection_gives_the_walks_distance_bits(oracle):
    """For every hit pixel of the seeded image the twin's own t = inv_det * dot(edge2, vvec) has the bits of the oracle's dist: the
    instance-space ray and the expressions the barycentrics come from are the walk's."""
    _, _, _, rec = T.seeded(oracle)
    img = T.seeded_image(oracle)
    k = np.flatnonzero(rec["hit"] == 1)
    assert len(k) > 1000 and (img.branch[k] == T.HIT).all() and (img.branch[rec["hit"] == 0] == T.NO_HIT).all()
    assert img.t[k].view(U).tobytes() == np.ascontiguousarray(rec["dist"][k]).view(U).tobytes()
    u, v = img.u[k], img.v[k]
    assert (u >= 0).all() and (v >= 0).all() and (u + v <= F(1)).all()                # what intersect_trig accepted


def test_populations(oracle):
    """Both octahedral hemispheres, with attributes and without; hits and misses in every 64-pixel run of a row (the rows are 64
    pixels wide: one run each); every material of the table, 0x100 reading as 0; both attribute modes differ."""
    _, geo, _, rec = T.seeded(oracle)
    img, geom = T.seeded_image(oracle), T.seeded_image(oracle, attributes=False)
    hit = (rec["hit"] == 1).reshape(T.H, T.W)
    assert (hit.any(axis=1) & (~hit).any(axis=1)).sum() >= 32
    k = np.flatnonzero(hit.reshape(-1))
    for im in (img, geom):
        z = G.decode_normal(im.words[k, 0])[:, 2]
        assert (z > 0.05).sum() > 100 and (z < -0.05).sum() > (100 if im is img else 0), ((z > 0).sum(), (z < 0).sum())
    assert (img.words[k, 0] != geom.words[k, 0]).mean() > 0.9 and (geom.words[:, 1] == 0).all() and (img.words[k, 1] != 0).all()
    assert set(np.unique(img.material[k]).tolist()) == {0, 1, 2, 3, 5, 255}
    assert (img.material == geom.material).all() and img.depth.tobytes() == geom.depth.tobytes()
    assert (img.depth[k] > 0).all() and (img.depth[~hit.reshape(-1)] == 0).all()


def test_depth_round_trips_to_the_hit_point(oracle):
    """|world_position_from_depth(depth) - p| / |p - eye| over the hit pixels of the seeded 64 x 64 image, p = eye + dir * dist:
    the twin's maximum, measured here on the CPU, is 4.533e-07 (ROUND_TRIP_MEASURED = 4.54e-7 rounds it up) - a few float32 roundings
    of a depth of about 2.5e-5.  The bound the tests assert is 4 x that, 1.816e-6, which covers the crops of the GPU test, whose pixel
    centres differ; three of them are measured here too: 17 x 31 2.592e-07, 64 x 9 2.322e-07, 65 x 3 1.497e-07."""
    _, geo, cam, _ = T.seeded(oracle)
    worst = round_trip_error(T.seeded_image(oracle), T.pixel_rays(cam, T.W, T.H)[0])
    print(f"round trip, 64 x 64: {worst:.3e}")
    assert 0.9 * ROUND_TRIP_MEASURED <= worst <= ROUND_TRIP_MEASURED, worst
    for w, h in ((17, 31), (64, 9), (65, 3)):
        _, _, _, rec = T.seeded(oracle, w, h)
        e = round_trip_error(T.resolve(cam, geo, rec, w, h), T.pixel_rays(cam, w, h)[0])
        print(f"round trip, {w} x {h}: {e:.3e}")
        assert e <= ROUND_TRIP_BOUND, (w, h, e)
