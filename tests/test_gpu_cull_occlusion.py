"""vd_cull_compact_hiz*, vd_cull_early_dev, vd_cull_late_dev - the occlusion-culled draw lists from ONE read of the instances -
against their pin, bit for bit:

    F = the bits vd_cull_mask_dev writes        V = vd_occlusion_mask_dev(F)        P = the caller's visible-last-frame bits
    hiz: list of V        early: list of E = F & P        late: list of L = V & ~P, d_visible_out = V

Expected values come from the CPU oracle alone (tests/cull_occlusion_cases.py: oracle.cull_emit -> F, oracle.occlusion_mask -> V,
rows of the oracle's draws); the GPU composition vd_cull_mask_dev -> vd_occlusion_mask_dev -> vd_expand_mask_dev must give the
same bytes.  Every comparison is tobytes() ==; output buffers are pre-filled with 0xAB and whatever the contract says is not
written must still be 0xAB afterwards.  Every case of 5 000 instances or more asserts on the ORACLE's sets, before a GPU
result is looked at, that the frustum culls something and the pyramid hides and leaves at least 5 % of the frustum set each."""
import os
import subprocess

import numpy as np
import pytest

import cull_occlusion_cases as K
from voidin_amd import abi, synth
from voidin_amd.runtime import EmitDraws, OcclusionState

pytestmark = pytest.mark.gpu

COUNT_SENTINEL = 0x7B7B7B7B
W, H = 1920, 1080


class Scene:
    """One scene on the host and on the device, with the oracle's sets."""

    def __init__(self, ctx, oracle, n, w=W, h=H, n_mesh=16, inst=None, cam=None, depth=None, check=True):
        import torch
        self.ctx, self.oracle, self.n, self.w, self.h = ctx, oracle, n, w, h
        self.cam = K.camera() if cam is None else cam
        self.meshes = K.meshes_for(n_mesh)
        self.inst = K.cloud(n, n_mesh=n_mesh) if inst is None else inst
        self.pyr = oracle.hiz_build(K.depth(w, h) if depth is None else depth)
        self.draws, self.F, self.V = K.oracle_sets(oracle, self.cam, self.meshes, self.inst, self.pyr, w, h)
        if check:
            K.assert_not_vacuous(n, self.F, self.V)
        self.d_m, self.d_i = ctx.upload(self.meshes), ctx.upload(self.inst)
        self.d_pyr = torch.from_numpy(self.pyr).to(ctx.torch_device)
        self.n_mesh = len(self.meshes)

    def expected(self, flags, pad):
        """bytes of the n-command output region: the list, then zeroes (pad_tail) or untouched 0xAB"""
        rows = K.select(self.draws, flags)
        assert (rows["instance_count"] == 1).all()
        k = len(rows)
        return rows.tobytes() + (b"\x00" if pad else b"\xab") * ((self.n - k) * 20), k

    def call(self, mode, pad=False, prev=None, alias=False):
        """-> (bytes of the whole output buffer = n commands + 64 bytes, the 4 count words, visible_out words or None, the
        words of prev after the call)"""
        import torch
        ctx, n = self.ctx, self.n
        d_out = ctx.empty(n * 20 + 64)
        d_out.fill_(0xAB)
        d_cnt = torch.full((4,), COUNT_SENTINEL, dtype=torch.int32, device=ctx.torch_device)
        d_prev = None if prev is None else ctx.upload(prev.view(np.int64)).view(torch.int64)
        d_vis = None
        if mode == "hiz":
            ctx.cull_compact_hiz_dev(self.cam, self.d_m, self.n_mesh, self.d_i, n, self.d_pyr, self.w, self.h, d_out, d_cnt, pad)
        elif mode == "early":
            ctx.cull_early_dev(self.cam, self.d_m, self.n_mesh, self.d_i, n, d_prev, d_out, d_cnt, pad)
        else:
            d_vis = d_prev if alias else torch.full_like(d_prev, 0x5A5A5A5A5A5A5A5A)
            ctx.cull_late_dev(self.cam, self.d_m, self.n_mesh, self.d_i, n, self.d_pyr, self.w, self.h, d_prev, d_vis, d_out, d_cnt, pad)
        torch.cuda.synchronize()
        vis = None if d_vis is None else d_vis.cpu().numpy().view(np.uint64)
        prev_after = None if d_prev is None else d_prev.cpu().numpy().view(np.uint64)
        return d_out.cpu().numpy().tobytes(), d_cnt.cpu().numpy().view(np.uint32), vis, prev_after

    def check(self, got, flags, pad, tag):
        out, cnt = got[0], got[1]
        want, k = self.expected(flags, pad)
        assert int(cnt[0]) == k, (tag, int(cnt[0]), k)
        assert (cnt[1:] == COUNT_SENTINEL).all(), tag                     # one count word is written
        assert out[: self.n * 20] == want, tag
        assert out[self.n * 20:] == b"\xab" * 64, tag                     # nothing behind the n commands

    def composition(self, prev=None, late=False):
        """The parent's four-launch composition on the GPU: mask -> occlusion mask [-> and / and-not with P] -> expansion
        with a caller-built id table.  -> (list bytes, count)"""
        import torch
        ctx, n = self.ctx, self.n
        d_mask = torch.zeros((n + 63) // 64, dtype=torch.int64, device=ctx.torch_device)
        ctx.cull_mask_dev(self.cam, self.d_m, self.n_mesh, self.d_i, n, d_mask)
        if prev is None or late:
            ctx.occlusion_mask_dev(self.cam, self.d_m, self.n_mesh, self.d_i, n, self.d_pyr, self.w, self.h, d_mask, d_mask)
        if prev is not None:
            d_p = ctx.upload(prev.view(np.int64)).view(torch.int64)
            d_mask = (d_mask & ~d_p) if late else (d_mask & d_p)
        id_t = np.uint8 if self.n_mesh <= 256 else (np.uint16 if self.n_mesh <= 65536 else np.uint32)
        ids = torch.from_numpy(np.minimum(self.inst["mesh"], self.n_mesh - 1).astype(id_t).view(np.uint8)).to(ctx.torch_device)
        d_draws, d_cnt = ctx.empty(n * 20), torch.zeros(4, dtype=torch.int32, device=ctx.torch_device)
        ctx.expand_mask_dev(d_mask, n, n, ids, self.d_m, self.n_mesh, d_draws, d_cnt, id_bytes=np.dtype(id_t).itemsize)
        torch.cuda.synchronize()
        k = int(d_cnt[0].item())
        return d_draws.cpu().numpy()[: k * 20].tobytes(), k


def check_all_modes(s, pads=(False, True), tag=""):
    """hiz, early and late (aliased and separate visible_out) with a random P whose padding bits are all ones; the P = 0 and
    P = all ones identities; the GPU composition."""
    n = s.n
    prev = K.random_prev(n)
    P = K.bits(prev, n)
    E, L = s.F & P, s.V & ~P
    K.assert_not_vacuous(n, s.F, s.V, E, L)                                # on the oracle's sets, before any GPU result
    assert not (E & L).any() and (E | L)[s.V].all()
    vis_want = K.pack(s.V)
    for pad in pads:
        s.check(s.call("hiz", pad), s.V, pad, (tag, "hiz", pad))
        s.check(s.call("early", pad, prev), E, pad, (tag, "early", pad))
        for alias in (False, True):
            got = s.call("late", pad, prev, alias)
            s.check(got, L, pad, (tag, "late", pad, alias))
            assert np.array_equal(got[2], vis_want), (tag, "visible_out", pad, alias)      # V, padding bits 0
            if not alias:
                assert np.array_equal(got[3], prev), (tag, "prev is read-only", pad)
    zero, ones = np.zeros_like(prev), np.full_like(prev, np.uint64(0xFFFFFFFFFFFFFFFF))
    s.check(s.call("late", False, zero), s.V, False, (tag, "late, P = 0 == hiz"))
    s.check(s.call("early", False, zero), np.zeros(n, bool), False, (tag, "early, P = 0 is empty"))
    s.check(s.call("early", True, ones), s.F, True, (tag, "early, P = ones == vd_cull_compact"))
    got = s.call("late", True, ones, True)
    s.check(got, np.zeros(n, bool), True, (tag, "late, P = ones is empty"))
    assert np.array_equal(got[2], vis_want), tag
    # the same bytes from the building blocks on the GPU
    for flags, kw in ((s.V, {}), (E, dict(prev=prev)), (L, dict(prev=prev, late=True))):
        want, k = s.expected(flags, False)
        comp, ck = s.composition(**kw)
        assert ck == k and comp == want[: k * 20], (tag, kw.keys())


@pytest.mark.parametrize("n", K.SIZES)
def test_every_seam_size(ctx, oracle, n):
    s = Scene(ctx, oracle, n)
    check_all_modes(s, tag=n)
    if n >= abi.CULL_SPLIT_MIN:                                              # early with P = ones against the GPU's own plain step
        import torch
        d_out, d_cnt = ctx.empty(n * 20), torch.zeros(4, dtype=torch.int32, device=ctx.torch_device)
        ctx.cull_compact_dev(s.cam, s.d_m, s.n_mesh, s.d_i, n, d_out, d_cnt, True)
        torch.cuda.synchronize()
        ones = np.full((n + 63) // 64, np.uint64(0xFFFFFFFFFFFFFFFF))
        got = s.call("early", True, ones)
        assert int(got[1][0]) == int(d_cnt[0].item()) and got[0][: n * 20] == d_out.cpu().numpy()[: n * 20].tobytes()


@pytest.mark.parametrize("n_mesh", K.MESH_COUNTS)
def test_every_id_width(ctx, oracle, n_mesh):
    check_all_modes(Scene(ctx, oracle, 200_000, n_mesh=n_mesh), tag=n_mesh)


@pytest.mark.parametrize("w,h", K.PYRAMIDS)
def test_every_pyramid_shape(ctx, oracle, w, h):
    import torch
    s = Scene(ctx, oracle, 200_000, w, h)
    # the pyramid the library builds from the same depth is the oracle's
    L = ctx.hiz_layout(w, h)
    d_pyr = torch.full((L.total_texels,), -1.0, dtype=torch.float32, device=ctx.torch_device)
    ctx.hiz_build_dev(ctx.upload(K.depth(w, h)), w, h, d_pyr)
    assert d_pyr.cpu().numpy().tobytes() == s.pyr.tobytes()
    s.d_pyr = d_pyr
    check_all_modes(s, tag=(w, h))


def test_poisoned_and_near_plane_instances_are_never_culled(ctx, oracle):
    """NaN, inf, zero scale, at and behind the eye, straddling the near plane - behind a wall 5 units away."""
    inst = K.poisoned_cloud()
    n, w, h = len(inst), 160, 120
    depth = np.full((h, w), np.float32(0.001 / 5.0), dtype=np.float32)
    s = Scene(ctx, oracle, n, w, h, inst=inst, cam=synth.camera_uniform(eye=(0, 0, 50), pitch_deg=0), depth=depth, check=False)
    assert s.V[10] and s.V[11] and s.V[13] and s.V[14]
    assert 0 < s.V.sum() < s.F.sum()
    prev = K.random_prev(n)
    P = K.bits(prev, n)
    for pad in (False, True):
        s.check(s.call("hiz", pad), s.V, pad, ("poison hiz", pad))
        s.check(s.call("early", pad, prev), s.F & P, pad, ("poison early", pad))
        got = s.call("late", pad, prev, True)
        s.check(got, s.V & ~P, pad, ("poison late", pad))
        assert np.array_equal(got[2], K.pack(s.V))
    listed = np.frombuffer(s.call("hiz")[0][: int(s.V.sum()) * 20], dtype=abi.DRAW)["base_instance"]
    assert {10, 11, 13, 14} <= set(listed.tolist())


def test_full_size_10m(ctx, oracle):
    """Beside tests/test_gpu_full_size.py's sizes: the bench's instance count."""
    n = K.FULL_SIZE
    s = Scene(ctx, oracle, n)
    prev = K.random_prev(n)
    P = K.bits(prev, n)
    E, L = s.F & P, s.V & ~P
    K.assert_not_vacuous(n, s.F, s.V, E, L)
    s.check(s.call("hiz", True), s.V, True, "10M hiz")
    s.check(s.call("early", False, prev), E, False, "10M early")
    got = s.call("late", True, prev, True)
    s.check(got, L, True, "10M late")
    assert np.array_equal(got[2], K.pack(s.V))
    want, k = s.expected(s.V, False)
    comp, ck = s.composition()
    assert ck == k and comp == want[: k * 20]


def _frames(oracle, meshes, inst, w, h, n_frames=3):
    """The oracle recurrence of the two-pass scheme: per frame (camera, pyramid, draws, E, L, V); P0 = 0, P(k+1) = V(k)."""
    n = len(inst)
    P = np.zeros(n, bool)
    out = []
    for k in range(n_frames):
        cam = K.camera(k)
        pyr = oracle.hiz_build(K.depth(w, h, seed=synth.SEED_BASE + 70 + k))
        draws, F, V = K.oracle_sets(oracle, cam, meshes, inst, pyr, w, h)
        E, L = F & P, V & ~P
        K.assert_not_vacuous(n, F, V)
        if k:
            assert E.sum() > 0 and L.sum() > 0 and (F & P & ~V).sum() > 0      # something drawn early is hidden now and leaves
        out.append((cam, pyr, draws, E, L, V))
        P = V
    return out


def test_three_frame_loop_with_a_moving_camera(ctx, oracle):
    """Frame k's d_visible_out is frame k+1's P (in place, owned by an OcclusionState); a vd_cull_compact_dev and a
    vd_cull_compact_views_dev call run between early and late of every frame."""
    import torch
    n, w, h = 300_000, 640, 360
    meshes, inst = K.meshes_for(16), K.cloud(n, seed=synth.SEED_BASE + 63)
    frames = _frames(oracle, meshes, inst, w, h)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    state = OcclusionState(ctx, n)
    assert state.visible.dtype == torch.int64 and len(state.visible) == (n + 63) // 64 and not state.visible.any().item()
    emit = EmitDraws(ctx)
    L_ = ctx.hiz_layout(w, h)
    d_pyr = torch.zeros(L_.total_texels, dtype=torch.float32, device=ctx.torch_device)
    d_e, d_l, d_x = ctx.empty(n * 20), ctx.empty(n * 20), ctx.empty(2 * n * 20)
    d_cnt = torch.full((8,), COUNT_SENTINEL, dtype=torch.int32, device=ctx.torch_device)
    for k, (cam, pyr, draws, E, L, V) in enumerate(frames):
        d_e.fill_(0xAB)
        d_l.fill_(0xAB)
        emit.record_early(cam, d_m, len(meshes), d_i, n, state, d_e, d_cnt[0:1], pad_tail=True)
        ctx.cull_compact_dev(cam, d_m, len(meshes), d_i, n, d_x, d_cnt[2:3])
        ctx.hiz_build_dev(ctx.upload(K.depth(w, h, seed=synth.SEED_BASE + 70 + k)), w, h, d_pyr)
        ctx.cull_compact_views_dev(np.concatenate([K.camera(1).reshape(1), K.camera(2).reshape(1)]), d_m, len(meshes), d_i, n, d_x, d_cnt[4:6])
        emit.record_late(cam, d_m, len(meshes), d_i, n, d_pyr, w, h, state, d_l, d_cnt[1:2])
        torch.cuda.synchronize()
        c = d_cnt.cpu().numpy().view(np.uint32)
        assert d_pyr.cpu().numpy().tobytes() == pyr.tobytes()
        we, wl = K.select(draws, E), K.select(draws, L)
        assert (int(c[0]), int(c[1])) == (len(we), len(wl)), (k, c)
        assert d_e.cpu().numpy()[: n * 20].tobytes() == we.tobytes() + b"\x00" * ((n - len(we)) * 20), k
        assert d_l.cpu().numpy()[: n * 20].tobytes() == wl.tobytes() + b"\xab" * ((n - len(wl)) * 20), k
        assert np.array_equal(state.visible.cpu().numpy().view(np.uint64), K.pack(V)), k


def test_frame_loop_replays_from_a_hip_graph(ctx, oracle):
    """early -> vd_hiz_build_dev -> late captured ONCE (single stream, linear) and replayed for three frames whose depth
    buffer changes in place; the camera is baked in, so the recurrence is frame 0's camera with moving depth."""
    import torch
    n, w, h = 300_000, 640, 360
    meshes, inst, cam = K.meshes_for(16), K.cloud(n, seed=synth.SEED_BASE + 63), K.camera(0)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    state = OcclusionState(ctx, n)
    L_ = ctx.hiz_layout(w, h)
    d_depth = torch.zeros(w * h, dtype=torch.float32, device=ctx.torch_device)
    d_pyr = torch.zeros(L_.total_texels, dtype=torch.float32, device=ctx.torch_device)
    d_e, d_l = ctx.empty(n * 20), ctx.empty(n * 20)
    d_cnt = torch.full((4,), COUNT_SENTINEL, dtype=torch.int32, device=ctx.torch_device)

    def frame():
        ctx.cull_early_dev(cam, d_m, len(meshes), d_i, n, state.visible, d_e, d_cnt[0:1], True)
        ctx.hiz_build_dev(d_depth, w, h, d_pyr)
        ctx.cull_late_dev(cam, d_m, len(meshes), d_i, n, d_pyr, w, h, state.visible, state.visible, d_l, d_cnt[1:2], True)

    frame()                                                  # warm-up: sizes the context's scratch
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    main_stream = torch.cuda.current_stream().cuda_stream
    try:
        with torch.cuda.graph(graph):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            frame()
    finally:
        ctx.set_stream(main_stream)
    state.reset()
    P = np.zeros(n, bool)
    for k in range(3):
        depth = K.depth(w, h, seed=synth.SEED_BASE + 70 + k)
        d_depth.copy_(torch.from_numpy(depth.reshape(-1)))
        d_e.fill_(0xAB)
        d_l.fill_(0xAB)
        d_cnt.fill_(COUNT_SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        draws, F, V = K.oracle_sets(oracle, cam, meshes, inst, oracle.hiz_build(depth), w, h)
        K.assert_not_vacuous(n, F, V)
        E, L = F & P, V & ~P
        if k:
            assert E.sum() > 0 and L.sum() > 0
        we, wl = K.select(draws, E), K.select(draws, L)
        c = d_cnt.cpu().numpy().view(np.uint32)
        assert (int(c[0]), int(c[1])) == (len(we), len(wl)), (k, c)
        assert d_e.cpu().numpy()[: n * 20].tobytes() == we.tobytes() + b"\x00" * ((n - len(we)) * 20), k
        assert d_l.cpu().numpy()[: n * 20].tobytes() == wl.tobytes() + b"\x00" * ((n - len(wl)) * 20), k
        assert np.array_equal(state.visible.cpu().numpy().view(np.uint64), K.pack(V)), k
        P = V


def test_id_table_is_shared_and_follows_scene_edits(ctx, oracle):
    """early, then late on the same scene (the id rows late finds are early's); then EVERY mesh id changes between an early and
    a late call, and again for a hiz call on a smaller scene: each list carries the ids of the instances it was called with."""
    a = Scene(ctx, oracle, 200_000, n_mesh=600)
    prev = K.random_prev(a.n)
    P = K.bits(prev, a.n)
    a.check(a.call("early", False, prev), a.F & P, False, "a early")
    a.check(a.call("late", False, prev, True), a.V & ~P, False, "a late")
    edited = a.inst.copy()
    edited["mesh"] = (a.inst["mesh"] + 7) % 600
    assert (edited["mesh"] != a.inst["mesh"]).all()
    b = Scene(ctx, oracle, 200_000, n_mesh=600, inst=edited)
    assert K.select(b.draws, b.V)["vertex_count"].tobytes() != K.select(a.draws, a.V)["vertex_count"].tobytes()
    a.check(a.call("early", False, prev), a.F & P, False, "a early again")
    b.check(b.call("late", False, prev, True), b.V & ~P, False, "b late after a early")
    a.check(a.call("hiz", True), a.V, True, "a hiz after b late")
    c = Scene(ctx, oracle, 70_001, n_mesh=600, inst=edited[:70_001].copy())
    c.check(c.call("hiz", True), c.V, True, "c hiz, smaller")
    b.check(b.call("hiz", False), b.V, False, "b hiz")


def test_host_pointer_form(ctx, oracle):
    s = Scene(ctx, oracle, 100_000)
    for pad in (False, True):
        out, cnt = ctx.cull_compact_hiz(s.cam, s.meshes, s.inst, s.pyr, s.w, s.h, pad_tail=pad)
        want, k = s.expected(s.V, pad)
        assert cnt == k and out.tobytes() == want, pad
    with pytest.raises(ValueError):
        ctx.cull_compact_hiz(s.cam, s.meshes, s.inst, s.pyr[:-1], s.w, s.h)
    # EmitDraws.record_hiz
    import torch
    d_out = ctx.empty(s.n * 20)
    d_out.fill_(0xAB)
    d_cnt = torch.zeros(4, dtype=torch.int32, device=ctx.torch_device)
    EmitDraws(ctx).record_hiz(s.cam, s.d_m, s.n_mesh, s.d_i, s.n, s.d_pyr, s.w, s.h, d_out, d_cnt, pad_tail=True)
    torch.cuda.synchronize()
    want, k = s.expected(s.V, True)
    assert int(d_cnt[0].item()) == k and d_out.cpu().numpy()[: s.n * 20].tobytes() == want


def test_stage_timing(ctx, oracle):
    s = Scene(ctx, oracle, 200_000)
    ctx.set_timing(True)
    try:
        s.call("hiz")
        a, b, total = ctx.last_gpu_ms_stage(0), ctx.last_gpu_ms_stage(1), ctx.last_gpu_ms()
        assert a > 0 and b > 0 and total >= max(a, b)
    finally:
        ctx.set_timing(False)


def test_invalid_arguments_and_empty_input(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    cam = np.ascontiguousarray(K.camera(), dtype=abi.CAMERA).reshape(1)
    meshes, inst = K.meshes_for(16), K.cloud(1000)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    L = ctx.hiz_layout(8, 4)
    d_pyr = torch.zeros(L.total_texels, dtype=torch.float32, device=ctx.torch_device)
    d_prev = torch.zeros(16, dtype=torch.int64, device=ctx.torch_device)
    d_out = ctx.empty(1000 * 20)
    d_out.fill_(0xAB)
    d_cnt = torch.full((4,), COUNT_SENTINEL, dtype=torch.int32, device=ctx.torch_device)
    c, m, i, p, v, o, k = cam.ctypes.data, d_m.data_ptr(), d_i.data_ptr(), d_pyr.data_ptr(), d_prev.data_ptr(), d_out.data_ptr(), d_cnt.data_ptr()
    bad_proj = cam.copy()
    bad_proj["projection"][0][15] = 1.0
    calls = {
        "vd_cull_compact_hiz": (lib.vd_cull_compact_hiz_dev, [c, m, 16, i, 1000, p, 8, 4, o, k, 0],
                                [(0, None), (1, None), (2, 0), (3, None), (5, None), (6, 0), (7, 65537), (8, None), (9, None), (0, bad_proj.ctypes.data)]),
        "vd_cull_early": (lib.vd_cull_early_dev, [c, m, 16, i, 1000, v, o, k, 0],
                          [(0, None), (1, None), (2, 0), (3, None), (5, None), (6, None), (7, None)]),
        "vd_cull_late": (lib.vd_cull_late_dev, [c, m, 16, i, 1000, p, 8, 4, v, v, o, k, 0],
                         [(0, None), (1, None), (2, 0), (3, None), (5, None), (6, 0), (7, 65537), (8, None), (9, None), (10, None), (11, None),
                          (0, bad_proj.ctypes.data)]),
    }
    for name, (fn, good, bads) in calls.items():
        for pos, bad in bads:
            args = list(good)
            args[pos] = bad
            assert fn(h, *args) == abi.VD_ERR_INVALID_ARG, (name, pos)
            assert name.encode() in lib.vd_last_error(h), (name, pos, lib.vd_last_error(h))
        if name != "vd_cull_early":
            args = list(good)
            args[0] = bad_proj.ctypes.data
            assert fn(h, *args) == abi.VD_ERR_INVALID_ARG and b"perspective" in lib.vd_last_error(h)
    torch.cuda.synchronize()
    assert (d_cnt.cpu().numpy().view(np.uint32) == COUNT_SENTINEL).all()          # a refused call writes nothing
    assert d_out.cpu().numpy().tobytes() == b"\xab" * len(d_out)
    assert not d_prev.any().item()
    # n_inst == 0: the count becomes 0 and nothing else is touched; null instances / out / masks are fine then
    for fn, args in ((lib.vd_cull_compact_hiz_dev, [c, m, 16, None, 0, p, 8, 4, None, k, 1]),
                     (lib.vd_cull_early_dev, [c, m, 16, None, 0, None, None, k, 1]),
                     (lib.vd_cull_late_dev, [c, m, 16, None, 0, p, 8, 4, None, None, None, k, 1])):
        d_cnt.fill_(COUNT_SENTINEL)
        assert fn(h, *args) == abi.VD_OK
        torch.cuda.synchronize()
        got = d_cnt.cpu().numpy().view(np.uint32)
        assert got[0] == 0 and (got[1:] == COUNT_SENTINEL).all()
    # the host-pointer form
    out, cnt = np.zeros(1000, abi.DRAW), np.full(1, 7, np.uint32)
    pyr = np.zeros(L.total_texels, np.float32)
    m_ = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
    hgood = [c, m_.ctypes.data, 16, inst.ctypes.data, 1000, pyr.ctypes.data, 8, 4, out.ctypes.data, cnt.ctypes.data, 0]
    for pos, bad in [(0, None), (1, None), (2, 0), (3, None), (5, None), (6, 0), (8, None), (9, None), (0, bad_proj.ctypes.data)]:
        args = list(hgood)
        args[pos] = bad
        assert lib.vd_cull_compact_hiz(h, *args) == abi.VD_ERR_INVALID_ARG, pos
        assert cnt[0] == 7 and not out.view(np.uint8).any(), pos
    assert lib.vd_cull_compact_hiz(h, c, m_.ctypes.data, 16, None, 0, pyr.ctypes.data, 8, 4, None, cnt.ctypes.data, 0) == abi.VD_OK and cnt[0] == 0


def test_cpp_mirror_runs_a_frame(ctx, oracle, tmp_path):
    """tests/cpp/occlusion_mirror_test.cpp: record_early -> HizPyramid::build -> record_late -> record_hiz through
    include/voidin.hpp, in a process of its own; its output file against the oracle."""
    from test_cull_occlusion_abi import build_mirror
    n, w, h = 50_000, 320, 200
    cam, meshes, inst = np.ascontiguousarray(K.camera(), dtype=abi.CAMERA).reshape(1), K.meshes_for(16), K.cloud(n)
    depth = K.depth(w, h)
    prev = K.random_prev(n)
    draws, F, V = K.oracle_sets(oracle, cam, meshes, inst, oracle.hiz_build(depth), w, h)
    P = K.bits(prev, n)
    K.assert_not_vacuous(n, F, V, F & P, V & ~P)
    src, dst = str(tmp_path / "scene.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(meshes), n, w, h], np.uint32).tobytes() + cam.tobytes() + meshes.tobytes() + inst.tobytes() +
                depth.tobytes() + prev.tobytes())
    exe = build_mirror(str(tmp_path))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    blob = open(dst, "rb").read()
    want = [K.select(draws, F & P), K.select(draws, V & ~P), K.select(draws, V)]
    assert np.frombuffer(blob[:12], np.uint32).tolist() == [len(x) for x in want]
    assert blob[12:] == b"".join(x.tobytes() for x in want) + K.pack(V).tobytes()
    assert os.path.getsize(dst) == len(blob)
