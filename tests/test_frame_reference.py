"""The float32 twin chain of a whole frame - gbuffer_trace_cases.resolve over the oracle's hits, .gbuffer(), lighting_cases.pass_words,
lighting_cases.shade (tests/frame_cases.chain) - against the plain float64 renderer of tests/frame_reference.py, without a GPU: the
primary stage, the light bits with the ray range off and on, the colour; the caps on what the renderer's robust flags exclude; the
measured tolerances; and five deliberately wrong variants of the chain that the comparison must catch.
(With a device: tests/test_gpu_frame.py runs the device's own outputs through the same stages.)  Figures: profiles/frame_reference.md."""
import numpy as np
import pytest

import frame_cases as FC
import frame_reference as R
import gbuffer_cases as G
import gbuffer_trace_cases as T
import lighting_cases as L
import shadow_pass_cases as S

F, U = np.float32, np.uint32
CASES = [(name, form) for name in ("room", "seeded") for form in FC.FORMS]
MEASURED = {"depth": FC.DEPTH_MEASURED, "uv": FC.UV_MEASURED, "normal": FC.NORMAL_MEASURED, "colour": FC.COLOUR_MEASURED}

def frame_of(oracle, name, form):
    return FC.frames(oracle)[name].form(*form)


def stages(oracle, fr, c=None, report=None):
    """Stages a, b (ray range off and on) and c of the twin chain -> {stage: what disagrees}."""
    c = FC.chain(oracle, fr) if c is None else c
    ref = FC.reference_of_chain(fr, c)
    out = {"a": FC.stage_a(fr, ref, c.img.branch == T.HIT, c.rec["instance"], c.rec["triangle"], c.img.depth, c.img.words, c.img.material, report)}
    for r in (False, True):
        out["b", r] = FC.stage_b(fr, ref, c.reach, c.want[r].occluded, r, report)
        out["c", r] = FC.stage_c(fr, c.img.depth, c.img.words, c.img.material, c.inr, c.occ[r], c.colour[r], report)
    return out


@pytest.mark.parametrize("name,form", CASES)
def test_the_twin_chain_is_the_float64_frame(oracle, name, form):
    """Stage a: on robust pixels the branch and the (instance, triangle) of the oracle's record are the renderer's, depth, normal, uv
    and material within their bounds.  Stage b: on robust bits the twin's in_range and the oracle's any-hit answer are the
    renderer's, ray range off and on.  Stage c: |twin - float64| <= COLOUR_TOL * S per channel, no NaN, alpha 1, material 0 magenta.
    The caps on the excluded pixels and bits are part of the stages."""
    fr = frame_of(oracle, name, form)
    report = {}
    out = stages(oracle, fr, report=report)
    print(name, form, "delta", FC.reference_of_chain(fr, FC.chain(oracle, fr)).delta, report)
    assert all(v == [] for v in out.values()), out
    assert all(report[k] <= m * 1.0001 for k, m in MEASURED.items()), \
        ("a measured value of frame_cases.py is out of date", report)


def test_the_measured_values_are_attained(oracle):
    """Each *_MEASURED is the maximum over both frames and all forms.  No case may exceed it (a constant that is out of date); that
    some case comes within a factor of two of it keeps a constant from standing far above what is measured, without tying the suite
    to the last digit of the twins' float32 rounding."""
    worst = dict.fromkeys(MEASURED, 0.0)
    for name, form in CASES:
        report = {}
        stages(oracle, frame_of(oracle, name, form), report=report)
        for k in worst:
            worst[k] = max(worst[k], report[k])
    for k, m in MEASURED.items():
        assert 0.5 * m <= worst[k] <= 1.0001 * m, (k, worst[k], m)
    assert FC.DEPTH_BOUND == 4 * FC.DEPTH_MEASURED and FC.UV_BOUND == 4 * FC.UV_MEASURED and FC.COLOUR_TOL == 4 * FC.COLOUR_MEASURED
    # the normal: the quantisation bound alone, but for the seeded frame with its vertex normals
    for name, form in CASES:
        extra = 4 * FC.NORMAL_MEASURED if (name, form[0]) == ("seeded", True) else 0.0
        assert FC.normal_bound(frame_of(oracle, name, form)) == FC.NORMAL_QUANT + extra, (name, form)


def test_populations(oracle):
    """What the frames are said to hold (frame_cases.py's docstring, and the counts measured for `seeded`)."""
    fr = FC.seeded(oracle)
    c = FC.chain(oracle, fr)
    assert (c.img.branch == T.HIT).sum() == 2163 and len(c.gb.points()[2]) == 1612
    assert set(np.unique(c.img.material)) == {0, 1, 2, 3, 5, 255}
    assert 0.5 < c.reach.mean() < 0.65
    covr = L.view(c.gb)[2][c.gb.points()[2]]
    assert 0.4 < (covr > 0).mean() < 0.65
    fr = FC.room(oracle)
    c = FC.chain(oracle, fr)
    assert fr.w * fr.h == 1850 and fr.w * fr.h % 64 != 0
    hit = c.img.branch == T.HIT
    assert 0 < (~hit).sum() < 200 and set(np.unique(c.rec["instance"][hit])) == set(range(len(FC.ROOM_INSTANCES)))      # every instance is seen, and the void
    assert {0, 1, G.LIGHT_MATERIAL, 3, 5, 7, 255} == set(np.unique(c.img.material))
    pix = c.gb.points()[2]
    covr = L.view(c.gb)[2]
    box2 = hit & (c.rec["instance"] == 6)
    assert box2.sum() > 20 and (covr[box2] > 0).all() and (covr[pix] > 0).sum() == box2.sum()      # the inside-out box alone looks away
    geometric = L.view(FC.chain(oracle, fr.form(False, True)).gb)[2]
    assert (geometric[box2] == 0).all()                                                             # ... and its geometric normals face the eye
    reach, off, on = c.reach, c.want[False].occluded, c.want[True].occluded
    floor = (c.rec["instance"][pix] == 0)
    assert reach[:, 0].all() and 50 < off[floor, 0].sum() < floor.sum() // 2                        # overhead: shadows on the floor, most of it lit
    assert 0.1 < reach[floor, 1].mean() < 0.6                                                       # its radius ends in mid-floor
    assert reach[:, 2].all() and off[:, 2].all() and on[:, 2].all()                                 # behind the wall
    assert off[reach[:, 3], 3].all() and on[reach[:, 3], 3].all()                                   # inside a box
    assert (off[:, 4] & ~on[:, 4]).sum() > 200 and not (on & ~off).any()                            # sphere 0 behind light 4: the range clears bits


def test_the_seeded_record_is_the_closest_hit_rule(oracle):
    """tests/golden/frame_seeded_range.npz (the brute force over the open segment (0, 1)) against the rule the oracle's closest hit
    gives for a segment that has only an upper end - hit and dist < 1 - on every ray of both forms of the normals."""
    for normals in (True, False):
        fr = FC.seeded(oracle).form(normals, True)
        c = FC.chain(oracle, fr)
        pos, nor, _ = c.gb.points()
        rule = np.stack([(lambda rec: (rec["hit"] == 1) & (rec["dist"] < 1))(oracle.trace(fr.scene, oracle.shadow_rays(pos, nor, fr.lights["position"][l]), threads=8)[0])
                         for l in range(len(fr.lights))], axis=1)
        assert (rule == c.hit[True]).all(), (normals, int((rule != c.hit[True]).sum()))
        assert 50 < (c.hit[False] & ~c.hit[True]).sum()                      # the segment ends at the light: some bits clear (measured: 84)


# ---- the renderer must be able to fail ------------------------------------------------------------------------------------------------

def broken(out):
    return sorted(k[0] if isinstance(k, tuple) else k for k, v in out.items() if v)


def test_y_not_flipped_in_the_pixel_ray_breaks_the_primary_stage(oracle, monkeypatch):
    fr = FC.room(oracle)
    proper = T.pixel_rays

    def unflipped(cam, width, height):                  # ndc.y = uv.y * 2 - 1: the ray of pixel (x, y) is that of (x, height - 1 - y)
        eye, d = proper(cam, width, height)
        flip = lambda a: np.ascontiguousarray(a.reshape(height, width, 3)[::-1].reshape(-1, 3))
        return flip(eye), flip(d)
    monkeypatch.setattr(T, "pixel_rays", unflipped)
    c = FC.chain(oracle, fr, tag=("y not flipped",))
    monkeypatch.undo()
    ref = FC.reference_of_chain(fr, FC.chain(oracle, fr))
    bad = FC.stage_a(fr, ref, c.img.branch == T.HIT, c.rec["instance"], c.rec["triangle"], c.img.depth, c.img.words, c.img.material)
    assert {b[0] for b in bad} >= {"hit / miss", "instance / triangle"}, bad


def test_clip_to_world_transposed_breaks_the_primary_stage(oracle):
    fr = FC.room(oracle)
    cam = np.array(fr.cam, dtype=fr.cam.dtype, copy=True)
    cam["clip_to_world"] = np.asarray(fr.cam["clip_to_world"]).reshape(4, 4).T.reshape(16)
    c = FC.chain(oracle, fr, cam=cam, tag=("transposed",))
    ref = FC.reference_of_chain(fr, FC.chain(oracle, fr))
    bad = FC.stage_a(fr, ref, c.img.branch == T.HIT, c.rec["instance"], c.rec["triangle"], c.img.depth, c.img.words, c.img.material)
    assert {b[0] for b in bad} & {"hit / miss", "instance / triangle"}, bad


def test_occlusion_swapped_breaks_the_colour(oracle):
    """occlusion = 1 for an occluded pair and 0.5 for a free one: the twin's shade fed the complement of the occlusion bits."""
    fr = FC.room(oracle)
    c = FC.chain(oracle, fr)
    swapped = L.shade(c.gb, fr.lights, c.inr, c.inr & ~c.occ[False], fr.table)
    assert FC.stage_c(fr, c.img.depth, c.img.words, c.img.material, c.inr, c.occ[False], c.colour[False]) == []
    bad = FC.stage_c(fr, c.img.depth, c.img.words, c.img.material, c.inr, c.occ[False], swapped)
    assert [b[0] for b in bad] == ["colour"] and bad[0][1] > 500, bad


def test_shade_from_the_opposite_normal_breaks_the_colour(oracle):
    fr = FC.room(oracle)
    c = FC.chain(oracle, fr)
    words = c.img.words.copy()
    k = np.flatnonzero(c.img.branch == T.HIT)
    words[k, 0] = G.encode_normal((-G.decode_normal(words[k, 0])).astype(F))
    turned = G.GBuffer(fr.cam, c.gb.depth, words.reshape(fr.h, fr.w, 2), c.gb.material)
    wrong = L.shade(turned, fr.lights, c.inr, c.occ[False], fr.table)
    bad = FC.stage_c(fr, c.img.depth, c.img.words, c.img.material, c.inr, c.occ[False], wrong)
    assert [b[0] for b in bad] == ["colour"] and bad[0][1] > 500, bad


def test_the_range_rule_with_greater_or_equal_breaks_the_bits(oracle):
    """A light placed exactly at a receiver's radius distance - in BOTH arithmetics: light = (p.x, 2 * p.y, p.z) and radius = |p.y|
    for the float32 position p of a receiver of the wall, so that light - p = (0, p.y, 0) and dist = sqrt(p.y * p.y) = |p.y| without
    a rounding in float32 and in float64 alike.  Such a pair is borderline by the flag's own definition (|dist - radius| = 0), and
    only there do `>` and `>=` differ - so for this one light stage b is run over the renderer's bits on the float32 positions
    themselves with the flag of that one pair set: the twin's bits pass the stage, the wrong rule's break it at exactly that pair."""
    fr = FC.room(oracle)
    c = FC.chain(oracle, fr)
    pos, nor, pix = c.gb.points()
    q = int(np.flatnonzero(c.rec["instance"][pix] == 1)[7])              # a receiver of the wall: p.y is some metres
    p = pos[q]
    lts = np.zeros(1, dtype=fr.lights.dtype)
    lts["position"][0], lts["radius"][0] = (p[0], F(2) * p[1], p[2]), abs(p[1])
    b = R.light_bits(pos.astype(np.float64), nor.astype(np.float64), fr.scene, lts, False, margin=0.0)
    assert b.dist[q, 0] == float(lts["radius"][0]) and b.in_range[q, 0] and not b.robust_in[q, 0]
    assert b.robust_in.sum() == b.robust_in.size - 1
    b.robust_in[q, 0] = True                                  # the tie is exact on both sides: compared, flag or no flag

    class OnTheFloat32Positions:                              # stage b's view of the renderer, for this one light
        def bits(self, ray_range):
            return b
    tie = FC.Frame("room tie", fr.scene, fr.full_geo, fr.cam, fr.w, fr.h, lts, fr.table)
    twin = S.in_range(pos, lts)
    with np.errstate(all="ignore"):
        wrong = ~((S.dist(pos, lts["position"][0]) - lts["radius"][0]).astype(F) >= F(0))[:, None]
    assert twin[q, 0] and not wrong[q, 0]
    assert FC.stage_b(tie, OnTheFloat32Positions(), twin, twin & b.occluded, False) == []
    assert FC.stage_b(tie, OnTheFloat32Positions(), wrong, wrong & b.occluded, False) == [("in range", 1, [[q, 0]])]


def test_the_stages_pass_for_the_room_the_variants_are_made_from(oracle):
    assert broken(stages(oracle, FC.room(oracle))) == []
