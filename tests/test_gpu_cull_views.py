"""vd_cull_compact_views* - the ordered draw lists of several cameras from ONE read of the instances - against the pin

    views(cameras)[v]  ==  vd_cull_compact(cameras[v])        bit for bit: list, count and padded tail,

through the C ABI.  Expected bytes come from the CPU oracle exactly as tests/test_gpu_cull.py gets them (cull_emit, then
compact, per view); every comparison is tobytes() ==, output buffers are pre-filled with 0xAB and every byte the contract
says is not written must still be 0xAB afterwards."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from voidin_amd import abi, synth
from voidin_amd.runtime import EmitDraws

pytestmark = pytest.mark.gpu

# the clouds of tests/test_gpu_cull.py (CLOUDS), copied
CLOUDS = {"wide": dict(scale_range=(0.25, 4.0)), "small": dict(scale_range=(0.02, 0.6), extent=600.0),
          "mid": dict(scale_range=(0.5, 1.2), extent=1500.0)}
N = 300_000
COUNT_SENTINEL = 0x7B7B7B7B


def eight_cameras():
    return [synth.camera_uniform(),
            synth.camera_uniform(yaw_deg=90.0, pitch_deg=0.0), synth.camera_uniform(yaw_deg=180.0, pitch_deg=0.0),
            synth.camera_uniform(yaw_deg=270.0, pitch_deg=0.0),
            synth.camera_uniform(pitch_deg=89.0), synth.camera_uniform(pitch_deg=-89.0),
            synth.camera_uniform(eye=(100.0, 50.0, -200.0), yaw_deg=45.0, pitch_deg=-30.0),
            synth.camera_uniform(jitter=(0.001, -0.001))]


def stack(cams):
    return np.concatenate([np.ascontiguousarray(c, dtype=abi.CAMERA).reshape(1) for c in cams])


def cloud(name, n=N):
    return synth.instances(n, seed=synth.SEED_BASE + 2, with_inverse=False, **CLOUDS[name])


def expected(oracle, cam, meshes, inst, pad_tail):
    """(region bytes of one view = n commands, count): the oracle's list, then zeroes (pad_tail) or untouched 0xAB."""
    want = oracle.cull_emit(cam, meshes, inst, threads=8)
    wc, wn = oracle.compact(want, pad_tail=pad_tail)
    if pad_tail:
        return wc.tobytes(), wn, want
    return wc[:wn].tobytes() + b"\xab" * ((len(inst) - wn) * 20), wn, want


def run_views(ctx, cams, d_m, n_mesh, d_i, n, pad_tail, stride=None):
    """-> (bytes of the whole output buffer: K * stride commands + 64 bytes, the 16 count words)"""
    import torch
    stride = n if stride is None else stride
    k = len(cams)
    d_out = ctx.empty(k * stride * 20 + 64)
    d_out.fill_(0xAB)
    d_cnt = torch.full((16,), COUNT_SENTINEL, dtype=torch.int32, device=ctx.torch_device)
    ctx.cull_compact_views_dev(stack(cams), d_m, n_mesh, d_i, n, d_out, d_cnt, pad_tail, stride)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().tobytes(), d_cnt.cpu().numpy().view(np.uint32)


def check_views(got, counts, want_regions, want_counts, n, stride, tag):
    k = len(want_regions)
    assert [int(c) for c in counts[:k]] == list(want_counts), tag
    assert (counts[k:] == COUNT_SENTINEL).all(), tag                    # only n_views count words are written
    for v in range(k):
        lo = v * stride * 20
        assert got[lo: lo + n * 20] == want_regions[v], (tag, v)
        if v + 1 < k:                                                   # the slots [n_inst, out_stride) of a view
            assert got[lo + n * 20: lo + stride * 20] == b"\xab" * ((stride - n) * 20), (tag, v)
    assert got[((k - 1) * stride + n) * 20:] == b"\xab" * (len(got) - ((k - 1) * stride + n) * 20), tag


def compare_with_oracle(ctx, oracle, cams, meshes, inst, pads=(False, True), strides=(0,), tag="", d_i=None):
    n = len(inst)
    d_m = ctx.upload(meshes)
    d_i = ctx.upload(inst) if d_i is None else d_i
    for pad in pads:
        exp = [expected(oracle, c, meshes, inst, pad) for c in cams]
        for extra in strides:
            got, counts = run_views(ctx, cams, d_m, len(meshes), d_i, n, pad, n + extra)
            check_views(got, counts, [e[0] for e in exp], [e[1] for e in exp], n, n + extra, (tag, pad, extra))


@pytest.mark.parametrize("name", ["wide", "small", "mid"])
def test_eight_different_views_each_equal_the_oracle(ctx, oracle, name):
    """K = 2, 3, 4, 5, 8 (the first K cameras; for K = 4 also the last four), with and without pad_tail, packed and with a gap
    between the lists.  The oracle's survivor sets of any two cameras differ (asserted), so a list written under the wrong
    camera, or one camera used twice, cannot pass."""
    cams, meshes, inst = eight_cameras(), synth.mesh_infos(), cloud(name)
    n = len(inst)
    vis = [oracle.cull_emit(c, meshes, inst, threads=8)["instance_count"] == 1 for c in cams]
    for a in range(8):
        for b in range(a + 1, 8):
            assert int((vis[a] != vis[b]).sum()) > 0, (name, a, b)
    assert all(0 < int(v.sum()) < n for v in vis)
    exp = {pad: [expected(oracle, c, meshes, inst, pad) for c in cams] for pad in (False, True)}
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    for sel in (range(0, 2), range(0, 3), range(0, 4), range(4, 8), range(0, 5), range(0, 8)):
        sel = list(sel)
        for pad in (False, True):
            for stride in (n, n + 1000):
                got, counts = run_views(ctx, [cams[v] for v in sel], d_m, len(meshes), d_i, n, pad, stride)
                check_views(got, counts, [exp[pad][v][0] for v in sel], [exp[pad][v][1] for v in sel], n, stride, (name, sel, pad, stride))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 100_000])
@pytest.mark.parametrize("name", ["wide", "small"])
def test_ragged_sizes(ctx, oracle, name, n):
    cams = eight_cameras()[:3]
    compare_with_oracle(ctx, oracle, cams, synth.mesh_infos(), cloud(name, n), strides=(0, 7), tag=(name, n))


@pytest.mark.parametrize("n_mesh", [1, 257, 600, 66_000])
def test_every_id_width_and_table_size(ctx, oracle, n_mesh):
    """1-byte ids (<= 256 meshes), 2-byte ids with the LDS table (<= 512) and without, 4-byte ids (> 65536 meshes): built as
    test_split_forms_with_every_id_width_and_table_size builds them."""
    meshes = synth.mesh_infos(n_mesh, seed=synth.SEED_BASE + 50)
    if n_mesh > 60_000:                                   # base_index would overflow u32 with the default index counts
        meshes["index_count"] = 36
        meshes["base_index"] = np.arange(n_mesh, dtype=np.uint32) * 36
        meshes["vertex_offset"] = np.arange(n_mesh, dtype=np.int32) * 12
    inst = synth.instances(N, n_mesh=n_mesh, seed=synth.SEED_BASE + 51, with_inverse=False, **CLOUDS["small"])
    cams = eight_cameras()
    compare_with_oracle(ctx, oracle, [cams[0], cams[6], cams[2]], meshes, inst, tag=n_mesh)


def test_reference_demo_scene_three_times_over(ctx, oracle):
    g = golden("cull_model_scene_x3.npz")                 # 327 meshes: 2-byte ids
    cams = eight_cameras()
    own = np.ascontiguousarray(g["camera"], dtype=abi.CAMERA).reshape(1)
    views = [own, cams[1], cams[6]]
    meshes, inst = g["meshes"], g["instances"]
    assert oracle.compact(oracle.cull_emit(own, meshes, inst))[1] == int(g["count"])
    compare_with_oracle(ctx, oracle, views, meshes, inst, strides=(0, 5), tag="scene_x3")


def test_every_view_has_its_own_near_and_far_plane(ctx, oracle):
    """Only the middle view has zfar = 50, znear = 1: the third return of is_visible is taken in that view alone."""
    meshes, inst = synth.mesh_infos(), cloud("mid")
    cam = synth.camera_uniform()
    mid = cam.copy()
    mid["zfar"], mid["znear"] = np.float32(50.0), np.float32(1.0)
    culled_by_far = int(oracle.cull_emit(cam, meshes, inst, threads=8)["instance_count"].sum()) - \
        int(oracle.cull_emit(mid, meshes, inst, threads=8)["instance_count"].sum())
    assert culled_by_far > 0, "the far-plane return is not exercised by this case"
    compare_with_oracle(ctx, oracle, [cam, mid, cam], meshes, inst, tag="planes")


def test_equal_cameras_give_equal_lists(ctx):
    import torch
    meshes, inst = synth.mesh_infos(), cloud("small")
    cam = eight_cameras()[6]
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    d_one = ctx.empty(N * 20)
    d_one.fill_(0xAB)
    d_cnt = torch.zeros(4, dtype=torch.int32, device=ctx.torch_device)
    for pad in (False, True):
        ctx.cull_compact_dev(cam, d_m, len(meshes), d_i, N, d_one, d_cnt, pad)
        torch.cuda.synchronize()
        one, cnt = d_one.cpu().numpy()[: N * 20].tobytes(), int(d_cnt[0].item())
        assert 0 < cnt < N
        got, counts = run_views(ctx, [cam] * 4, d_m, len(meshes), d_i, N, pad)
        check_views(got, counts, [one] * 4, [cnt] * 4, N, N, pad)
        d_one.fill_(0xAB)


def test_views_and_single_view_calls_share_a_context(ctx, ctx_options, oracle):
    """views (K = 4) -> vd_cull_compact_dev in its split form -> views on a buffer in which EVERY mesh id differs -> views on the
    first buffer again: the id table keeps only rows that differ from one call to the next, and every call stays exact."""
    import torch
    cams, meshes = eight_cameras()[:4], synth.mesh_infos()
    a = cloud("small")
    b = cloud("mid")
    b["mesh"] = (a["mesh"] + 5) % len(meshes)
    assert (a["mesh"] != b["mesh"]).all()
    d_m, d_a, d_b = ctx.upload(meshes), ctx.upload(a), ctx.upload(b)
    compare_with_oracle(ctx, oracle, cams, meshes, a, pads=(True,), tag="a", d_i=d_a)
    ctx_options("cull.split_min", 1)
    d_out, d_cnt = ctx.empty(N * 20), torch.zeros(4, dtype=torch.int32, device=ctx.torch_device)
    for inst, d_i in ((b, d_b), (a, d_a)):
        want, wn = oracle.compact(oracle.cull_emit(cams[1], meshes, inst, threads=8))
        ctx.cull_compact_dev(cams[1], d_m, len(meshes), d_i, N, d_out, d_cnt)
        torch.cuda.synchronize()
        assert int(d_cnt[0].item()) == wn and d_out.cpu().numpy()[: wn * 20].tobytes() == want[:wn].tobytes()
    compare_with_oracle(ctx, oracle, cams, meshes, b, pads=(True,), tag="b", d_i=d_b)
    compare_with_oracle(ctx, oracle, cams, meshes, a, pads=(False,), tag="a again", d_i=d_a)
    compare_with_oracle(ctx, oracle, cams[:3], meshes, b[:200_001], pads=(True,), tag="b, fewer views, smaller")
    compare_with_oracle(ctx, oracle, cams, meshes, a, pads=(True,), tag="a, third time", d_i=d_a)


def test_views_call_replays_from_a_hip_graph(ctx, oracle):
    """Captured the way tests/test_gpu_frame_loop.py captures its frame; the instance buffer is then overwritten in place
    with another cloud and the replay must give that cloud's lists (cameras are baked in by value, pointers stay)."""
    import torch
    cams, meshes = [eight_cameras()[v] for v in (0, 6, 3)], synth.mesh_infos()
    first, second = cloud("small"), cloud("mid")
    second["mesh"] = (second["mesh"] + 3) % len(meshes)
    d_m, d_i = ctx.upload(meshes), ctx.upload(first)
    stride = N + 11
    d_out = ctx.empty(3 * stride * 20 + 64)
    d_cnt = torch.full((16,), COUNT_SENTINEL, dtype=torch.int32, device=ctx.torch_device)
    camera_block = stack(cams)

    def step():
        ctx.cull_compact_views_dev(camera_block, d_m, len(meshes), d_i, N, d_out, d_cnt, True, stride)

    step()                                                 # warm-up: sizes the context's scratch
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    main_stream = torch.cuda.current_stream().cuda_stream
    try:
        with torch.cuda.graph(graph):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            step()
    finally:
        ctx.set_stream(main_stream)
    camera_block[:] = stack([eight_cameras()[1]] * 3)      # the host copy may change after capture
    d_i.copy_(torch.from_numpy(second.view(np.uint8).reshape(-1)))
    d_out.fill_(0xAB)
    d_cnt.fill_(COUNT_SENTINEL)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    exp = [expected(oracle, c, meshes, second, True) for c in cams]
    check_views(d_out.cpu().numpy().tobytes(), d_cnt.cpu().numpy().view(np.uint32), [e[0] for e in exp], [e[1] for e in exp], N, stride, "replay")


def test_full_size_10m_four_views(ctx, oracle):
    """The bench's cloud: every view bit-equal to vd_cull_compact_dev of that camera on the GPU, view 0 to the oracle."""
    import torch
    meshes = synth.mesh_infos()
    cams = [eight_cameras()[v] for v in (0, 1, 6, 7)]
    n = 10_000_000
    inst = synth.instances(n, seed=synth.SEED_BASE + 3, with_inverse=False)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    d_views = ctx.empty(4 * n * 20)
    d_views.fill_(0xAB)
    d_counts = torch.full((16,), COUNT_SENTINEL, dtype=torch.int32, device=ctx.torch_device)
    ctx.cull_compact_views_dev(stack(cams), d_m, len(meshes), d_i, n, d_views, d_counts, True)
    d_one = ctx.empty(n * 20)
    d_cnt = torch.zeros(4, dtype=torch.int32, device=ctx.torch_device)
    counts = []
    for v, cam in enumerate(cams):
        d_one.fill_(0xAB)
        ctx.cull_compact_dev(cam, d_m, len(meshes), d_i, n, d_one, d_cnt, True)
        torch.cuda.synchronize()
        counts.append(int(d_cnt[0].item()))
        assert int(d_counts[v].item()) == counts[v], v
        assert torch.equal(d_views[v * n * 20: (v + 1) * n * 20], d_one[: n * 20]), v
    assert len(set(counts)) == 4 and all(0 < c < n for c in counts)
    assert (d_counts[4:].cpu().numpy().view(np.uint32) == COUNT_SENTINEL).all()
    want, wn = oracle.compact(oracle.cull_emit(cams[0], meshes, inst, threads=8), pad_tail=True)
    assert counts[0] == wn and d_views[: n * 20].cpu().numpy().tobytes() == want.tobytes()


def test_host_pointer_form_and_record_views(ctx, oracle):
    import torch
    cams, meshes, inst = eight_cameras()[:3], synth.mesh_infos(), cloud("small")
    for pad in (False, True):
        exp = [expected(oracle, c, meshes, inst, pad) for c in cams]
        out, cnt = ctx.cull_compact_views(stack(cams), meshes, inst, pad_tail=pad)
        assert [int(c) for c in cnt] == [e[1] for e in exp]
        for v in range(3):
            assert out[v].tobytes() == exp[v][0], (pad, v)
    # out_stride > n_inst through the raw entry point
    stride = N + 3
    out = np.zeros(3 * stride, dtype=abi.DRAW)
    out.view(np.uint8)[:] = 0xAB
    cnt = np.full(16, COUNT_SENTINEL, np.uint32)
    block = stack(cams)
    m_, i_ = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO), np.ascontiguousarray(inst, dtype=abi.INSTANCE)
    assert ctx.lib.vd_cull_compact_views(ctx.h, block.ctypes.data, 3, m_.ctypes.data, len(m_), i_.ctypes.data, N, out.ctypes.data, stride,
                                         cnt.ctypes.data, 0) == abi.VD_OK
    exp = [expected(oracle, c, meshes, inst, False) for c in cams]
    check_views(out.tobytes() + b"\xab" * 64, cnt, [e[0] for e in exp], [e[1] for e in exp], N, stride, "host stride")
    # EmitDraws.record_views
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    d_out = ctx.empty(3 * N * 20 + 64)
    d_out.fill_(0xAB)
    d_cnt = torch.full((16,), COUNT_SENTINEL, dtype=torch.int32, device=ctx.torch_device)
    EmitDraws(ctx).record_views(stack(cams), d_m, len(meshes), d_i, N, d_out, d_cnt, pad_tail=True)
    torch.cuda.synchronize()
    exp = [expected(oracle, c, meshes, inst, True) for c in cams]
    check_views(d_out.cpu().numpy().tobytes(), d_cnt.cpu().numpy().view(np.uint32), [e[0] for e in exp], [e[1] for e in exp], N, N, "record_views")


def test_one_view_forwards_to_the_single_view_call(ctx, oracle):
    cam, meshes, inst = eight_cameras()[6], synth.mesh_infos(), cloud("small")
    compare_with_oracle(ctx, oracle, [cam], meshes, inst, strides=(0, 9), tag="K = 1")


def test_invalid_arguments_and_empty_input(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    cams, meshes, inst = stack(eight_cameras()), synth.mesh_infos(), cloud("small", 1000)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    d_out = ctx.empty(8 * 1000 * 20)
    d_cnt = torch.full((16,), COUNT_SENTINEL, dtype=torch.int32, device=ctx.torch_device)
    good = [cams.ctypes.data, 3, d_m.data_ptr(), len(meshes), d_i.data_ptr(), 1000, d_out.data_ptr(), 1000, d_cnt.data_ptr(), 0]
    for pos, bad in [(0, None), (1, 0), (1, abi.MAX_VIEWS + 1), (2, None), (3, 0), (4, None), (6, None), (7, 999), (8, None)]:
        args = list(good)
        args[pos] = bad
        assert lib.vd_cull_compact_views_dev(h, *args) == abi.VD_ERR_INVALID_ARG, pos
        assert b"vd_cull_compact_views" in lib.vd_last_error(h)
    out, cnt = np.zeros(3000, abi.DRAW), np.zeros(3, np.uint32)
    m_ = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
    hgood = [cams.ctypes.data, 3, m_.ctypes.data, len(m_), inst.ctypes.data, 1000, out.ctypes.data, 1000, cnt.ctypes.data, 0]
    for pos, bad in [(0, None), (1, 0), (1, abi.MAX_VIEWS + 1), (2, None), (3, 0), (4, None), (6, None), (7, 999), (8, None)]:
        args = list(hgood)
        args[pos] = bad
        cnt[:] = 7
        assert lib.vd_cull_compact_views(h, *args) == abi.VD_ERR_INVALID_ARG, pos
        assert (cnt == 7).all() and not out.view(np.uint8).any(), pos             # a refused call writes nothing
    torch.cuda.synchronize()
    assert (d_cnt.cpu().numpy().view(np.uint32) == COUNT_SENTINEL).all()          # a refused call writes nothing
    # n_inst == 0: all n_views counts become 0, nothing else; null instances / out are fine then
    assert lib.vd_cull_compact_views_dev(h, cams.ctypes.data, 5, d_m.data_ptr(), len(meshes), None, 0, None, 0, d_cnt.data_ptr(), 1) == abi.VD_OK
    torch.cuda.synchronize()
    c = d_cnt.cpu().numpy().view(np.uint32)
    assert (c[:5] == 0).all() and (c[5:] == COUNT_SENTINEL).all()
    cnt[:] = 7
    assert lib.vd_cull_compact_views(h, cams.ctypes.data, 3, m_.ctypes.data, len(m_), None, 0, None, 0, cnt.ctypes.data, 0) == abi.VD_OK
    assert (cnt == 0).all()
