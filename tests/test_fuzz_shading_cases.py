"""tests/fuzz_shading_cases.py without a GPU: the slice that tests/test_gpu_fuzz_shading.py runs (same seed, same counts) visits what it
is there to visit, a wrong summation order or a dropped occlusion bit would show in most of its lighting cases, the `hit and dist < 1`
form of the occluded bit agrees with the brute force over the open segment, the oracle's interval walk (vd_ref_trace_range) agrees with
both on ordinary rays and parts from them where the first campaign found the device to, and a case made alone is the case a campaign makes."""
import numpy as np
import pytest

import fuzz_shading_cases as Z
import gbuffer_cases as G
import gbuffer_trace_cases as T
import lighting_cases as L
import shadow_pass_cases as S

U = np.uint32
SCAN_CELLS = 1024 * 4            # kScanThreads * kScanItems of voidin_amd/csrc/vd_shade.hpp: the cells one round of shadow.hip's one-workgroup scan takes


@pytest.fixture(scope="module")
def lighting():
    return [Z.LightingCase(Z.SEED, k) for k in range(Z.SLICE["lighting"])]


@pytest.fixture(scope="module")
def shadow(oracle):
    return [Z.ShadowCase(Z.SEED, k, oracle) for k in range(Z.SLICE["shadow"])]


@pytest.fixture(scope="module")
def chain(oracle):
    return [Z.ChainCase(Z.SEED, k, oracle) for k in range(Z.SLICE["chain"])]


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------

def test_the_lighting_slice_visits_every_kind_of_word_count(lighting):
    Ws = {c.W for c in lighting}
    assert {0, 1, 2, 3, 32} <= Ws, sorted(Ws)
    inside = sorted(w for w in Ws if 4 <= w <= 31)
    assert len([w for w in inside if w % 2 == 0]) >= 3 and len([w for w in inside if w % 2 == 1]) >= 3, inside
    # a later trip of the LDS staging that is only partly filled, together with a ragged last wave
    assert [c.k for c in lighting if c.W > 4 and c.W % 4 and (c.w * c.h) % 64], "no case with W > 4, W % 4 != 0 and a ragged last wave"
    shapes = {(c.w, c.h) for c in lighting}
    assert len(shapes) >= 10, sorted(shapes)
    assert any(c.pitches[2] & 1 for c in lighting) and any(not c.pitches[2] & 1 for c in lighting)
    assert all(c.colour_pitch > 16 * c.w for c in lighting)
    assert any(c.pitches[0] == 4 * c.w for c in lighting) and any(c.pitches[0] > 4 * c.w for c in lighting)


def test_a_wrong_order_or_a_dropped_occlusion_bit_would_show(lighting):
    """Of the lighting cases with at least two lights and a receiver, at least two thirds give another image when the lights are
    summed in descending order, and at least two thirds when the occlusion bits are ignored."""
    live = [c for c in lighting if c.n_lights >= 2 and G.receivers(c.gb.material).any()]
    assert len(live) >= 30, len(live)
    order = sum(bool(L.changed(c.want(), c.want(descending=True)).any()) for c in live)
    occlusion = sum(bool(L.changed(c.want(), c.want(ignore_occlusion=True)).any()) for c in live)
    print(f"descending order shows in {order} of {len(live)} cases, ignored occlusion in {occlusion}")
    assert 3 * order >= 2 * len(live), (order, len(live))
    assert 3 * occlusion >= 2 * len(live), (occlusion, len(live))


def test_the_lighting_inputs_hold_the_classes_they_are_drawn_for(lighting):
    depth = np.concatenate([c.gb.depth.reshape(-1) for c in lighting])
    assert np.isnan(depth).any() and np.isinf(depth).any() and (depth < 0).any() and (depth == 0).any() and ((depth > 0) & (depth < 1e-38)).any()
    assert any(np.isnan(c.lts["radius"]).any() for c in lighting) and any(np.isinf(c.lts["radius"]).any() for c in lighting)
    mats = set(np.concatenate([c.gb.material.reshape(-1) for c in lighting]).tolist())
    assert mats == {0, 1, 2, 3, 7, 255}
    tails = [c for c in lighting if c.n_lights & 31]
    assert any((c.inr[:, -1] >> U(c.n_lights & 31)).any() for c in tails), "no bit at or above n_lights is ever set"
    assert any((c.inr[~G.receivers(c.gb.material.reshape(-1))] == U(0xffffffff)).all() and c.n_lights for c in lighting if not G.receivers(c.gb.material).all())


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------

def test_the_shadow_slice(shadow):
    occluded = clear = differs = 0
    for c in shadow:
        if not c.n_lights:
            continue
        w = c.words()
        assert w.reach.any() and not w.reach.all(), c.describe()
        occluded += int(w.hit[0].sum())
        clear += int((w.reach & ~w.hit[0]).sum())
        differs += int(c.ray_range and (w.hit[0] != w.hit[1]).any())
        assert w.info["n_points"] == len(c.gb.points()[2]) and w.info["n_rays"] == w.reach.sum()
        near = (np.abs(c.gb.points()[0]) < 1e30).all(axis=1)
        assert np.array_equal(w.hit[1][near], w.near[near]), c.describe()          # the interval walk is `hit and dist < 1` of the half-line's
    assert occluded > 0 and clear > 0, (occluded, clear)
    assert differs > 0, "no ray-range case in which something lies beyond a light"
    cells = [c.n_lights * -(-len(c.gb.points()[2]) // G.TILE) for c in shadow]
    assert max(cells) > SCAN_CELLS, cells
    assert {c.ray_range for c in shadow} == {0, 1} and len({c.max_chunk_rays for c in shadow}) >= 3
    assert len({c.sc.name == "seeded" for c in shadow}) == 2


def test_hit_and_dist_below_one_is_the_brute_force_over_the_open_segment(oracle):
    """The small check of the module's docstring: shadow case 2 at 17 x 5 pixels with 33 lights, every ray in range."""
    c = Z.ShadowCase(Z.SEED, 2, oracle, shape=(17, 5), n_lights=33)
    pos, nor, _ = c.gb.points()
    w = c.words()
    assert 100 < w.reach.sum() and w.hit[1].any() and (w.hit[0] != w.hit[1]).any(), (w.reach.sum(), w.hit[1].sum())
    brute = S.segment_hits(c.sc.scene, S.shadow_rays(oracle, pos, nor, c.lts)).reshape(len(c.lts), len(pos)).T
    assert np.array_equal(brute & w.reach, w.near) and np.array_equal(w.hit[1], w.near)


FAR = (731, 124, 34)             # (seed, case, pixel) of the campaign's lists: depth 1e-40


def test_where_float32_cannot_tell_the_light_from_the_scene_the_walk_decides(oracle):
    """The finding of the first campaign (profiles/fuzz_shading.md): pixel 34 of shadow case 124 of seed 731 has depth 1e-40, its point
    lies 1e37 away, and three lights reach it (radius NaN or +inf).  The half-line's closest hit lies at t = 0.9999992, so `hit and
    dist < 1` and the brute force say occluded; the walk over (0, 1) never enters the boxes - their entry distance is not below 1 -
    and says clear, which is the header's definition and what the device answers.  With (0, MAX_DIST) the interval walk gives the
    bytes of the plain one."""
    seed, k, pixel = FAR
    c = Z.ShadowCase(seed, k, oracle, campaign=True)
    pos, nor, pix = c.gb.points()
    p = int(np.flatnonzero(pix == pixel)[0])
    w = c.words()
    assert c.gb.depth.reshape(-1)[pixel] == np.float32(1e-40) and (np.abs(pos[p]) > 1e35).any()
    assert w.near[p].sum() == 3 and not w.hit[1][p].any() and w.hit[0][p].sum() == 3
    assert np.array_equal(np.delete(w.hit[1], p, axis=0), np.delete(w.near, p, axis=0))
    rays = np.concatenate([oracle.shadow_rays(pos, nor, c.lts["position"][l]) for l in np.flatnonzero(w.near[p])])
    plain = oracle.trace(c.sc.scene, rays)[0]
    rays["_pad0"], rays["_pad1"] = 0.0, 1e30
    assert oracle.trace_range(c.sc.scene, rays).tobytes() == plain.tobytes()
    rays["_pad0"], rays["_pad1"] = np.nan, np.nan           # both read as the default's
    assert oracle.trace_range(c.sc.scene, rays).tobytes() == plain.tobytes()


def test_the_oracles_interval_walk_is_the_brute_force_on_ordinary_rays(oracle):
    """oracle.trace_range on the `seeded` case of tests/trace_range_cases.py under its fixed intervals (both ends set, around each ray's
    first two intersections): dist and hit of the brute force bit for bit, instance and triangle where one triangle decides."""
    import trace_range_cases as cases
    c = cases.case("seeded", oracle)
    e = cases.expected(c.hits, c.t_min, c.t_max, c.miss_record())
    got = oracle.trace_range(c.scene, cases.with_range(c.rays, c.t_min, c.t_max), threads=8)
    assert got["dist"].tobytes() == e.records["dist"].tobytes() and np.array_equal(got["hit"], e.records["hit"])
    same = (got["instance"] == e.records["instance"]) & (got["triangle"] == e.records["triangle"])
    assert same[e.unique].all() and (got["hit"] != c.want["hit"]).sum() > 100
    assert oracle.trace_range(c.scene, cases.with_range(c.rays, 0.0, 1e30), threads=8).tobytes() == c.want.tobytes()


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------

def test_the_chain_slice(chain):
    halves = []
    for c in chain:
        hit = c.img.branch == T.HIT
        if c.w * c.h > 64:
            assert hit.any() and not hit.all(), c.describe()
        if c.geo.tex_coords is not None:
            word = c.img.words[hit, 1]
            halves.append(np.concatenate([word & U(0xffff), word >> U(16)]))
    halves = np.concatenate(halves)
    assert ((halves & U(0x7fff)) == U(0x7c00)).any(), "no uv half overflows to infinity"
    assert (((halves & U(0x7c00)) == 0) & ((halves & U(0x3ff)) != 0)).any(), "no uv half is subnormal"
    assert any(c.geo.normals is None for c in chain) and any(c.geo.tex_coords is None for c in chain) and any(c.geo.normals is not None and c.geo.tex_coords is not None for c in chain)
    assert max(c.n_lights for c in chain) <= 65 and any(c.n_lights for c in chain)


# ---- replay -----------------------------------------------------------------------------------------------------------------------------

def _arrays(c):
    out = [c.gb.depth, c.gb.normal_uv, c.gb.material, c.lts, np.asarray(c.cam).reshape(1)]
    if c.part == "lighting" and c.n_lights:
        out += [c.inr, c.occ]
    if c.part == "chain":
        out += [c.rec, c.geo.instances] + [a for a in (c.geo.normals, c.geo.tex_coords) if a is not None]
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out) + c.describe().encode()


def test_a_case_made_alone_is_the_case_of_a_run_from_case_zero(oracle, lighting, shadow, chain):
    """The slices above were made in order from case 0; here single cases are made again, alone and out of order."""
    for k in (37, 5, 20):
        assert _arrays(Z.make("lighting", Z.SEED, k)) == _arrays(lighting[k]), k
    for k in (9, 3):
        assert _arrays(Z.make("shadow", Z.SEED, k, oracle)) == _arrays(shadow[k]), k
    for k in (6, 1):
        assert _arrays(Z.make("chain", Z.SEED, k, oracle)) == _arrays(chain[k]), k
    assert _arrays(Z.make("lighting", Z.SEED + 1, 5)) != _arrays(lighting[5])
