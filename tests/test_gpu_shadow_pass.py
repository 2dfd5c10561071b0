"""vd_shadow_pass_dev / vd_shadow_pass_prepared_dev (include/voidin_shadow.h): one bit per (point, light) - in range, and in range and
occluded - from one call.  Every byte is checked twice: against the CPU expectation of tests/shadow_pass_cases.py (the float32 twin of
the range rule; the oracle's any-hit answer, the brute force's under VD_OPT_TRACE_RAY_RANGE) and against the COMPOSITION on the GPU,
the loop the pass replaces - per light vd_shadow_rays_dev and the matching any-hit call, masked by the twin.  Every call here writes
between canary words, which must survive it."""
import ctypes as C

import numpy as np
import pytest

import shadow_pass_cases as S
from test_gpu_trace_range import Rig
from voidin_amd import abi
from voidin_amd.runtime import VoidinError
from write_set import FILL, Fences

pytestmark = pytest.mark.gpu

PAD = 8                                                    # canary words in front of and behind every output
FORMS = ("scene", "prepared", "wide", "tight")
POINTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2142)
LIGHTS = (1, 31, 32, 33, 65)


class Inputs:
    """One case on the device: its rig (the scene in every shape a call takes), points, normals, lights."""

    def __init__(self, ctx, scene, pos, nor, lts):
        self.ctx, self.rig = ctx, Rig(ctx, scene)
        self.pos, self.nor, self.lts = pos, nor, lts
        self.d_pos, self.d_nor, self.d_lts = ctx.upload(pos), ctx.upload(nor), ctx.upload(lts)

    def close(self):
        self.rig.close()

    def call(self, form, n_points, n_lights, d_occ, d_inr, max_chunk_rays=0):
        ctx, rig = self.ctx, self.rig
        if form == "scene":
            return ctx.shadow_pass_dev(rig.ds, self.d_pos, self.d_nor, n_points, self.d_lts, n_lights, d_occ, d_inr, max_chunk_rays)
        accel = {"prepared": rig.acc, "wide": rig.acc_wide, "tight": rig.acc_tight}[form]
        return ctx.shadow_pass_prepared_dev(accel, self.d_pos, self.d_nor, n_points, self.d_lts, n_lights, d_occ, d_inr, max_chunk_rays)

    def run(self, form, n_points, n_lights, fill=0xEE, max_chunk_rays=0, with_in_range=True):
        """-> (occluded words [P][W], in-range words or None, info); the canary words around both outputs are checked."""
        import torch
        W = (n_lights + 31) // 32
        n = n_points * W
        bufs = [torch.full(((n + 2 * PAD) * 4,), fill, dtype=torch.uint8, device="cuda") for _ in range(2 if with_in_range else 1)]
        info = self.call(form, n_points, n_lights, bufs[0][PAD * 4:], bufs[1][PAD * 4:] if with_in_range else None, max_chunk_rays)
        torch.cuda.synchronize()
        out = []
        for b in bufs:
            raw = b.cpu().numpy()
            assert (raw[: PAD * 4] == fill).all() and (raw[(PAD + n) * 4:] == fill).all(), f"{form}: a word outside the call's {n}"
            out.append(raw[PAD * 4: (PAD + n) * 4].view(np.uint32).reshape(n_points, W).copy())
        assert info["words_per_point"] == W
        return out[0], (out[1] if with_in_range else None), info

    def composition(self, form, ray_range):
        """bool [P][L]: per light vd_shadow_rays_dev + the any-hit call of `form` over ALL points, on the context as it is set."""
        import torch
        ctx, rig, P = self.ctx, self.rig, len(self.pos)
        d_rays = ctx.empty(P * 32)
        d_flag = torch.empty((P,), dtype=torch.int32, device="cuda")
        out = np.zeros((P, len(self.lts)), bool)
        for l in range(len(self.lts)):
            ctx.shadow_rays_dev(self.d_pos, self.d_nor, P, self.lts["position"][l], d_rays)
            if form == "scene":
                ctx.trace_any_dev(rig.ds, d_rays, P, d_flag)
            else:
                ctx.trace_any_prepared_dev({"prepared": rig.acc, "wide": rig.acc_wide, "tight": rig.acc_tight}[form], d_rays, P, d_flag)
            torch.cuda.synchronize()
            out[:, l] = d_flag.cpu().numpy() != 0
        return out


@pytest.fixture(scope="module")
def seeded(ctx, oracle):
    scene, pos, nor = S.points(oracle)
    i = Inputs(ctx, scene, pos, nor, S.lights())
    yield i
    i.close()


@pytest.fixture(scope="module")
def hand(ctx, oracle):
    i = Inputs(ctx, *S.hand_made(oracle))
    yield i
    i.close()


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [hex(int(got[tuple(b)])) for b in bad[:4]], [hex(int(want[tuple(b)])) for b in bad[:4]])


# ---- 1. every shape, every form, option off and on ------------------------------------------------------------------------------

@pytest.mark.parametrize("ray_range", (0, 1))
@pytest.mark.parametrize("form", FORMS)
def test_shapes(ctx, ctx_options, oracle, seeded, form, ray_range):
    """Prefixes of the points x prefixes of the lights: the tile edges (512 points a wave), the word edges (32 lights), one point,
    one light.  Both outputs equal the CPU expectation and the composition on the GPU; n_rays is the twin's count."""
    ctx_options("trace.ray_range", ray_range)
    reach = S.in_range(seeded.pos, seeded.lts)
    comp = seeded.composition(form, ray_range)
    full = S.seeded_want(oracle, S.N_POINTS, S.N_LIGHTS, ray_range)
    assert np.array_equal(comp & reach, full.occluded), (form, "the composition itself differs from the CPU expectation", int((comp & reach != full.occluded).sum()))
    for n_lights in LIGHTS:
        for n_points in POINTS:
            want = S.seeded_want(oracle, n_points, n_lights, ray_range)
            occ, inr, info = seeded.run(form, n_points, n_lights)
            what = (form, ray_range, n_points, n_lights)
            same(inr, want.in_range_words, what + ("in range",))
            same(occ, want.occluded_words, what + ("occluded",))
            same(occ, S.pack(comp[:n_points, :n_lights] & reach[:n_points, :n_lights]), what + ("occluded, against the composition",))
            assert info["n_rays"] == want.n_rays and info["n_chunks"] >= 1, (what, info)


@pytest.mark.parametrize("ray_range", (0, 1))
def test_hand_made_lights(ctx, ctx_options, oracle, hand, ray_range):
    """Radii on the edges of the rule - 0, exactly the distance, one float below it, +inf, NaN, negative, -0.0 - on shadow_scene:
    by default the sphere behind the light shadows point 0, on the segment to the light it does not; point 1 is shadowed either way."""
    ctx_options("trace.ray_range", ray_range)
    want = S.hand_want(oracle, ray_range)
    reach = S.in_range(hand.pos, hand.lts)
    P, L = reach.shape
    for form in FORMS:
        occ, inr, info = hand.run(form, P, L)
        same(inr, want.in_range_words, (form, "in range"))
        same(occ, want.occluded_words, (form, "occluded"))
        same(occ, S.pack(hand.composition(form, ray_range) & reach), (form, "occluded, against the composition"))
        assert info == {"n_rays": want.n_rays, "n_chunks": 1, "words_per_point": 1}
        assert [(int(occ[p, 0]) >> 5) & 1 for p in (0, 1)] == ([0, 1] if ray_range else [1, 1]), form      # light 5: shadow_scene's, radius +inf


# ---- 2. chunks, what the buffers held, no in-range output, twice ----------------------------------------------------------------

@pytest.mark.parametrize("ray_range", (0, 1))
def test_chunks_do_not_change_a_byte(ctx, ctx_options, oracle, seeded, ray_range):
    """max_chunk_rays 1 500 on the full shape and 1 on 257 x 33 (every cell its own chunk: each word is folded in many launches):
    more than one chunk, and the bytes of one chunk - whatever the outputs held before."""
    ctx_options("trace.ray_range", ray_range)
    for n_points, n_lights, max_chunk in ((S.N_POINTS, S.N_LIGHTS, 1500), (257, 33, 1)):
        want = S.seeded_want(oracle, n_points, n_lights, ray_range)
        for form in ("scene", "prepared"):
            occ1, inr1, info1 = seeded.run(form, n_points, n_lights)
            assert info1["n_chunks"] == 1
            same(occ1, want.occluded_words, (form, n_points, "one chunk"))
            for fill in (0xEE, 0xFF, 0x00):
                occ, inr, info = seeded.run(form, n_points, n_lights, fill=fill, max_chunk_rays=max_chunk)
                assert info["n_chunks"] > 1 and info["n_rays"] == info1["n_rays"] == want.n_rays, (form, info, info1)
                assert occ.tobytes() == occ1.tobytes() and inr.tobytes() == inr1.tobytes(), (form, n_points, max_chunk, fill)
            if max_chunk == 1:
                cells = n_lights * ((n_points + 511) // 512)
                assert info["n_chunks"] <= cells, info


def test_what_the_outputs_held_does_not_matter(ctx, oracle, seeded):
    want = S.seeded_want(oracle, 1025, 33, 0)
    for fill in (0xFF, 0x00):
        occ, inr, _ = seeded.run("prepared", 1025, 33, fill=fill)
        same(occ, want.occluded_words, fill)
        same(inr, want.in_range_words, fill)


def test_without_the_in_range_output_and_twice(ctx, oracle, seeded):
    want = S.seeded_want(oracle, S.N_POINTS, S.N_LIGHTS, 0)
    for form in ("scene", "wide"):
        occ, none, info = seeded.run(form, S.N_POINTS, S.N_LIGHTS, with_in_range=False)
        assert none is None and info["n_rays"] == want.n_rays
        same(occ, want.occluded_words, (form, "d_in_range == NULL"))
        first = seeded.run(form, S.N_POINTS, S.N_LIGHTS, max_chunk_rays=20000)
        second = seeded.run(form, S.N_POINTS, S.N_LIGHTS, max_chunk_rays=20000)
        assert first[0].tobytes() == second[0].tobytes() == occ.tobytes() and first[1].tobytes() == second[1].tobytes() and first[2] == second[2]


def test_the_most_lights_a_call_takes(ctx, ctx_options, oracle, seeded):
    """VD_SHADOW_MAX_LIGHTS = 1024 lights, 32 words a point, 5 x 1024 = 5 120 cells: more than the 4 096 the scan's one workgroup takes
    in a round, so its carry from round to round is in the result.  The lights are the 65 seeded ones over and over, every copy with
    its radii scaled differently: the twin gives the reach, the any-hit answer of light l is that of seeded light l % 65."""
    import torch
    L = abi.SHADOW_MAX_LIGHTS
    lts = seeded.lts[np.arange(L) % S.N_LIGHTS].copy()
    lts["radius"] = (lts["radius"] * (np.float32(0.55) + np.float32(0.06) * (np.arange(L) // S.N_LIGHTS).astype(np.float32))).astype(np.float32)
    reach = S.in_range(seeded.pos, lts)
    assert 0.25 < reach.mean() < 0.75
    many = Inputs.__new__(Inputs)
    many.ctx, many.rig, many.pos, many.nor, many.lts = ctx, seeded.rig, seeded.pos, seeded.nor, lts
    many.d_pos, many.d_nor, many.d_lts = seeded.d_pos, seeded.d_nor, ctx.upload(lts)
    for ray_range in (0, 1):
        ctx_options("trace.ray_range", ray_range)
        hit = S.any_hit(oracle, "seeded", S.points(oracle)[0], seeded.pos, seeded.nor, seeded.lts, ray_range)[:, np.arange(L) % S.N_LIGHTS]
        want = S.Want(reach, hit)
        for form, max_chunk in (("prepared", 0), ("scene", 50000)):
            occ, inr, info = many.run(form, S.N_POINTS, L, max_chunk_rays=max_chunk)
            same(inr, want.in_range_words, (form, ray_range, "in range"))
            same(occ, want.occluded_words, (form, ray_range, "occluded"))
            assert info["n_rays"] == want.n_rays and info["words_per_point"] == 32 and (info["n_chunks"] > 1) == (max_chunk != 0), info


# ---- 3. the write set ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_chunk", (0, 700))
def test_write_set(ctx, oracle, seeded, max_chunk):
    """Inputs and outputs between the 64 KiB guards of tests/write_set.py: the inputs come back unchanged, no guard is touched, and
    of buffers one word per point too long nothing past n_points * W words is written."""
    import torch
    n_points, n_lights, W = 1025, 65, 3
    want = S.seeded_want(oracle, n_points, n_lights, 0)
    f = Fences()
    pos, nor = f.inp("positions", seeded.pos[:n_points]), f.inp("normals", seeded.nor[:n_points])
    lts = f.inp("lights", seeded.lts[:n_lights])
    scene_in = [f.inp(name, a) for name, a in zip(("tlas", "instances", "meshes", "bvh", "vertices", "indices"), seeded.rig.scene)]
    nbytes = n_points * W * 4
    occ, inr = f.out("occluded", nbytes + 4 * n_points), f.out("in_range", nbytes + 4 * n_points)
    s = abi.TraceScene()
    for k, name in enumerate(("tlas_nodes", "instances", "meshes", "bvh_nodes", "vertices", "indices")):
        setattr(s, name, scene_in[k].ptr)
        setattr(s, "n_" + name, getattr(seeded.rig.ds.struct, "n_" + name))
    info = abi.ShadowPassInfo()
    ctx._chk(ctx.lib.vd_shadow_pass_dev(ctx.h, C.byref(s), pos.ptr, nor.ptr, n_points, lts.ptr, n_lights, max_chunk, occ.ptr, inr.ptr, C.byref(info)))
    torch.cuda.synchronize()
    f.check()
    occ.check_fill(nbytes)
    inr.check_fill(nbytes)
    same(occ.read(np.uint32, n_points * W).reshape(n_points, W), want.occluded_words, "occluded")
    same(inr.read(np.uint32, n_points * W).reshape(n_points, W), want.in_range_words, "in range")
    assert info.n_rays == want.n_rays and (info.n_chunks > 1) == (max_chunk != 0)


# ---- 4. stream order -------------------------------------------------------------------------------------------------------------

def test_stream_order(oracle):
    """tests/test_gpu_stream_order.py's method for this call: warmed up on lights A; then on a side stream, behind its delay, the
    upload of lights B and the call through the context of that stream.  A clone taken on the stream in front of the upload holds the
    fill - nothing ran ahead of its place - and the clone behind the call holds expected(B), which differs from expected(A)."""
    import torch
    from test_gpu_stream_order import Side
    scene, pos, nor = S.points(oracle)
    n_points, n_lights, W = 1025, 33, 2
    pos, nor = pos[:n_points], nor[:n_points]
    A, B = S.lights()[:n_lights], S.lights(seed=S.SEED + 1)[:n_lights]
    want = {}
    for key, lts in (("A", A), ("B", B)):
        reach = S.in_range(pos, lts)
        want[key] = S.Want(reach, S.any_hit(oracle, ("stream", key), scene, pos, nor, lts, False))
    assert want["A"].occluded_words.tobytes() != want["B"].occluded_words.tobytes()
    assert want["A"].in_range_words.tobytes() != want["B"].in_range_words.tobytes()
    side = Side()
    try:
        c = side.ctx
        ds = c.device_scene(scene)
        d_pos, d_nor, d_lts = c.upload(pos), c.upload(nor), c.upload(A)
        d_B = c.upload(B)
        outs = [torch.full((n_points * W * 4,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        c.shadow_pass_dev(ds, d_pos, d_nor, n_points, d_lts, n_lights, outs[0], outs[1])            # a. warmed up, on A
        side.stream.synchronize()
        for o, w in zip(outs, (want["A"].occluded_words, want["A"].in_range_words)):
            assert o.cpu().numpy().tobytes() == w.tobytes(), "warm-up call on A"
            o.fill_(FILL)
        torch.cuda.synchronize()
        side.delay(side.stream)                                                                      # b. the delay, `before`, the upload of B
        with torch.cuda.stream(side.stream):
            before = [o.clone() for o in outs]
            d_lts.copy_(d_B, non_blocking=True)
        assert not side.stream.query(), f"the delay had ended before the call was made (measured {side.delay_ms:.1f} ms)"
        info = c.shadow_pass_dev(ds, d_pos, d_nor, n_points, d_lts, n_lights, outs[0], outs[1])      # c. the call (it blocks)
        with torch.cuda.stream(side.stream):
            after = [o.clone() for o in outs]
        side.stream.synchronize()
        for b in before:
            assert bool((b == FILL).all().item()), f"before holds results: written ahead of the call's place in the stream (delay measured {side.delay_ms:.1f} ms)"
        for a, w in zip(after, (want["B"].occluded_words, want["B"].in_range_words)):
            assert a.cpu().numpy().tobytes() == w.tobytes(), f"after != expected(B) (delay measured {side.delay_ms:.1f} ms)"
        assert info["n_rays"] == want["B"].n_rays != want["A"].n_rays
    finally:
        side.close()


# ---- 5. arguments ----------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_empty_calls(ctx, seeded):
    import torch
    lib, rig = ctx.lib, seeded.rig
    p, n, l = seeded.d_pos.data_ptr(), seeded.d_nor.data_ptr(), seeded.d_lts.data_ptr()
    out = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    o = out.data_ptr()
    scene, accel = C.byref(rig.ds.struct), rig.acc.h

    def refused(rc, word):
        assert rc == abi.VD_ERR_INVALID_ARG and word in lib.vd_last_error(ctx.h).decode(), (rc, lib.vd_last_error(ctx.h))

    refused(lib.vd_shadow_pass_dev(ctx.h, None, p, n, 4, l, 4, 0, o, None, None), "null scene")
    refused(lib.vd_shadow_pass_prepared_dev(ctx.h, None, p, n, 4, l, 4, 0, o, None, None), "null accel")
    for args in ((None, n, 4, l, 4, 0, o), (p, None, 4, l, 4, 0, o), (p, n, 4, None, 4, 0, o), (p, n, 4, l, 4, 0, None)):
        refused(lib.vd_shadow_pass_dev(ctx.h, scene, *args, None, None), "null pointer")
        refused(lib.vd_shadow_pass_prepared_dev(ctx.h, accel, *args, None, None), "null pointer")
    refused(lib.vd_shadow_pass_dev(ctx.h, scene, p, n, 4, l, abi.SHADOW_MAX_LIGHTS + 1, 0, o, None, None), "VD_SHADOW_MAX_LIGHTS")
    refused(lib.vd_shadow_pass_dev(ctx.h, scene, p, n, 0xf0000000 // 1024 + 1, l, 1024, 0, o, None, None), "0xf0000000")
    broken = abi.TraceScene.from_buffer_copy(rig.ds.struct)
    broken.bvh_nodes = None
    refused(lib.vd_shadow_pass_dev(ctx.h, C.byref(broken), p, n, 4, l, 4, 0, o, None, None), "incomplete scene")     # what the walk refuses
    with pytest.raises(VoidinError):
        ctx.shadow_pass_dev(rig.ds, None, seeded.d_nor, 4, seeded.d_lts, 4, out)
    # nothing to do: VD_OK, the info zeroed, nothing written - whatever the pointers say
    for n_points, n_lights in ((0, 4), (4, 0), (0, 0)):
        info = abi.ShadowPassInfo(7, 7, 7, 7)
        assert lib.vd_shadow_pass_dev(ctx.h, scene, None, None, n_points, None, n_lights, 0, o, o, C.byref(info)) == abi.VD_OK
        assert (info.n_rays, info.n_chunks, info.words_per_point) == (0, 0, 0)
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all().item())
