"""The host-pointer forms of the cull family against each other's leftovers: every one of them stages through the same three
buffers of the context (instances; a count header + tables; the lists), so they run here one after the other on ONE fresh
context, at sizes that make the buffers regrow under another form's layout, and each result is compared byte for byte with
the matching _dev form on a second context with uploaded inputs.  Half of the cases set cull.split_min = 1, so the staged
split path runs at these sizes; the other half keeps the fused path."""

import numpy as np
import pytest

import cull_occlusion_cases as K
import lod_cases as LC
from voidin_amd import abi
from voidin_amd.runtime import Context

pytestmark = pytest.mark.gpu

SIZES = [1, 65, 1025, 3000, 40_000]      # the last one regrows every staging buffer
PYR_W, PYR_H = 160, 90
FILL = 0xC3
SLACK = 7                                # commands / id words behind every host output that no call may touch
SENTINEL = 0xC3C3C3C3


@pytest.fixture(scope="module")
def ref_ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pyramid(ref_ctx):
    import torch
    L = ref_ctx.hiz_layout(PYR_W, PYR_H)
    d_pyr = torch.zeros(L.total_texels, dtype=torch.float32, device=ref_ctx.torch_device)
    ref_ctx.hiz_build_dev(ref_ctx.upload(K.depth(PYR_W, PYR_H)), PYR_W, PYR_H, d_pyr)
    torch.cuda.synchronize()
    return d_pyr.cpu().numpy()


_inputs, _refs = {}, {}


def inputs(oracle, n):
    """One scene per size: the occlusion cases' cloud over 16 meshes, three cameras, and the LOD cases' tables over the same
    cloud (64 rows, 16 groups)."""
    if n not in _inputs:
        cam, P, _base, rows, groups, inst = LC.scene(oracle, n, n_rows=64)
        cams = np.concatenate([np.ascontiguousarray(K.camera(f), dtype=abi.CAMERA).reshape(1) for f in range(3)])
        _inputs[n] = dict(cams=cams, meshes=np.ascontiguousarray(K.meshes_for(16), dtype=abi.MESH_INFO),
                          inst=np.ascontiguousarray(inst, dtype=abi.INSTANCE), lod_cam=np.ascontiguousarray(cam, dtype=abi.CAMERA).reshape(1),
                          P=P, rows=np.ascontiguousarray(rows, dtype=abi.MESH_INFO), groups=np.ascontiguousarray(groups, dtype=abi.LOD_GROUP))
    return _inputs[n]


def reference(ref_ctx, oracle, pyramid, n, pad):
    """{form: (counts, lists [K, n])} from the _dev forms, computed once per (size, pad_tail) and never written again."""
    if (n, pad) in _refs:
        return _refs[(n, pad)]
    import torch
    s = inputs(oracle, n)
    c = ref_ctx
    d_m, d_i, d_rows, d_g, d_pyr = c.upload(s["meshes"]), c.upload(s["inst"]), c.upload(s["rows"]), c.upload(s["groups"]), c.upload(pyramid)
    out = {}

    def lists(k, fn):
        d_out = c.empty(k * n * 20)
        d_out.fill_(FILL)
        d_cnt = torch.full((4,), -1, dtype=torch.int32, device=c.torch_device)
        fn(d_out, d_cnt)
        torch.cuda.synchronize()
        return d_cnt.cpu().numpy().view(np.uint32)[:k].copy(), d_out.cpu().numpy()[: k * n * 20].view(abi.DRAW).reshape(k, n).copy()

    out["compact"] = lists(1, lambda o, k: c.cull_compact_dev(s["cams"][:1], d_m, 16, d_i, n, o, k, pad_tail=pad))
    out["views3"] = lists(3, lambda o, k: c.cull_compact_views_dev(s["cams"], d_m, 16, d_i, n, o, k, pad_tail=pad))
    out["views1"] = lists(1, lambda o, k: c.cull_compact_views_dev(s["cams"][:1], d_m, 16, d_i, n, o, k, pad_tail=pad))
    out["hiz"] = lists(1, lambda o, k: c.cull_compact_hiz_dev(s["cams"][:1], d_m, 16, d_i, n, d_pyr, PYR_W, PYR_H, o, k, pad_tail=pad))
    out["lod"] = lists(1, lambda o, k: c.cull_compact_lod_dev(s["lod_cam"], s["P"], d_g, 16, d_rows, 64, d_i, n, o, k, pad_tail=pad))
    d_e = c.empty(n * 20)
    c.cull_emit_dev(s["cams"][:1], d_m, 16, d_i, n, d_e)
    d_cmds, d_ids = c.empty(16 * 20), torch.full((n,), -1, dtype=torch.int32, device=c.torch_device)
    d_cnt = torch.full((4,), -1, dtype=torch.int32, device=c.torch_device)
    c.cull_batch_dev(s["cams"][:1], d_m, 16, d_i, n, d_cmds, d_ids, d_cnt)
    torch.cuda.synchronize()
    out["emit"] = d_e.cpu().numpy()[: n * 20].view(abi.DRAW).copy()
    out["batch"] = (int(d_cnt.cpu().numpy().view(np.uint32)[0]), d_cmds.cpu().numpy()[: 16 * 20].view(abi.DRAW).copy(),
                    d_ids.cpu().numpy().view(np.uint32).copy())
    if n >= K.NON_VACUOUS_FROM:              # the forms differ from each other and none keeps or drops everything
        v3, hiz, lod = out["views3"][0], int(out["hiz"][0][0]), out["lod"]
        assert 0 < hiz < int(out["compact"][0][0]) < n and len(set(int(x) for x in v3)) == 3 and 0 < out["batch"][0] < n
        assert len(np.unique(lod[1][0][: int(lod[0][0])]["vertex_count"])) > 16      # more rows than there are groups: LODs were chosen
    _refs[(n, pad)] = out
    return out


def filled(count, dtype):
    a = np.zeros(count, dtype=dtype)
    a.view(np.uint8)[:] = FILL
    return a


def check_lists(what, got, got_counts, stride, want, n, pad):
    """got: the host output, K lists `stride` commands apart; want = (counts, lists [K, n])."""
    w_cnt, w_lists = want
    assert list(got_counts) == list(w_cnt), (what, got_counts, w_cnt)
    for v, k in enumerate(int(x) for x in w_cnt):
        row = got[v * stride: (v + 1) * stride]
        assert k <= n, (what, v, k)
        assert row[:k].tobytes() == w_lists[v][:k].tobytes(), (what, v, "list")
        end = k
        if pad:
            assert row[k:n].tobytes() == w_lists[v][k:n].tobytes() == b"\x00" * ((n - k) * 20), (what, v, "padded tail")
            end = n
        assert (row[end:].view(np.uint8) == FILL).all(), (what, v, "bytes behind the list were written")


def run_sequence(ctx, s, pyramid, want, n, pad):
    lib, h = ctx.lib, ctx.h
    cams, meshes, inst = s["cams"], s["meshes"], s["inst"]
    c0, m, i = cams.ctypes.data, meshes.ctypes.data, inst.ctypes.data

    def compact(tag):
        out, cnt = filled(n + SLACK, abi.DRAW), filled(2, np.uint32)
        assert lib.vd_cull_compact(h, c0, m, 16, i, n, out.ctypes.data, cnt.ctypes.data, pad) == abi.VD_OK, lib.vd_last_error(h)
        assert cnt[1] == SENTINEL
        check_lists(tag, out, cnt[:1], n + SLACK, want["compact"], n, pad)

    def views(k, tag):
        stride = n + SLACK
        out, cnt = filled(k * stride, abi.DRAW), filled(k + 1, np.uint32)
        assert lib.vd_cull_compact_views(h, c0, k, m, 16, i, n, out.ctypes.data, stride, cnt.ctypes.data, pad) == abi.VD_OK, lib.vd_last_error(h)
        assert cnt[k] == SENTINEL
        check_lists(tag, out, cnt[:k], stride, want[tag], n, pad)

    compact("compact")
    views(3, "views3")
    out, cnt = filled(n + SLACK, abi.DRAW), filled(2, np.uint32)
    assert lib.vd_cull_compact_hiz(h, c0, m, 16, i, n, pyramid.ctypes.data, PYR_W, PYR_H, out.ctypes.data, cnt.ctypes.data, pad) == abi.VD_OK, lib.vd_last_error(h)
    assert cnt[1] == SENTINEL
    check_lists("hiz", out, cnt[:1], n + SLACK, want["hiz"], n, pad)
    out, cnt = filled(n + SLACK, abi.DRAW), filled(2, np.uint32)
    assert lib.vd_cull_compact_lod(h, s["lod_cam"].ctypes.data, abi.lod_params(s["P"]), s["groups"].ctypes.data, 16, s["rows"].ctypes.data, 64, i, n,
                                   out.ctypes.data, cnt.ctypes.data, pad) == abi.VD_OK, lib.vd_last_error(h)
    assert cnt[1] == SENTINEL
    check_lists("lod", out, cnt[:1], n + SLACK, want["lod"], n, pad)
    cmds, ids, cnt = filled(16 + SLACK, abi.DRAW), filled(n + SLACK, np.uint32), filled(2, np.uint32)
    assert lib.vd_cull_batch(h, c0, m, 16, i, n, cmds.ctypes.data, ids.ctypes.data, cnt.ctypes.data) == abi.VD_OK, lib.vd_last_error(h)
    w_cnt, w_cmds, w_ids = want["batch"]
    assert (int(cnt[0]), int(cnt[1])) == (w_cnt, SENTINEL)
    assert cmds[:16].tobytes() == w_cmds.tobytes() and (cmds[16:].view(np.uint8) == FILL).all()
    assert ids[:w_cnt].tobytes() == w_ids[:w_cnt].tobytes() and (ids[w_cnt:] == SENTINEL).all()
    out = filled(n + SLACK, abi.DRAW)
    assert lib.vd_cull_emit(h, c0, m, 16, i, n, out.ctypes.data) == abi.VD_OK, lib.vd_last_error(h)
    assert out[:n].tobytes() == want["emit"].tobytes() and (out[n:].view(np.uint8) == FILL).all()
    views(1, "views1")
    compact("compact again")


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
def test_host_forms_share_the_staging_buffers(ref_ctx, oracle, pyramid, split, pad):
    ctx = Context(0)
    try:
        if split:
            ctx.set_option("cull.split_min", 1)
        for n in SIZES:
            run_sequence(ctx, inputs(oracle, n), pyramid, reference(ref_ctx, oracle, pyramid, n, bool(pad)), n, pad)
    finally:
        ctx.close()


def test_refusals_name_the_form_and_leave_the_outputs(ref_ctx, oracle, pyramid):
    """A null in each pointer position in turn: VD_ERR_INVALID_ARG, the form's name in the message, no byte of an output
    written - and the caller's count word as the forms have always left it: vd_cull_compact zeroes it before it looks at the
    instances and the list, the others refuse first."""
    n = 65
    s = inputs(oracle, n)
    ctx = Context(0)
    try:
        lib, h = ctx.lib, ctx.h
        out, ids, cnt = filled(3 * n, abi.DRAW), filled(n, np.uint32), filled(4, np.uint32)
        c0, m, i, o, k = s["cams"].ctypes.data, s["meshes"].ctypes.data, s["inst"].ctypes.data, out.ctypes.data, cnt.ctypes.data
        P = abi.lod_params(s["P"])
        # name: (function, good arguments, pointer positions, positions after which the first count word is 0)
        forms = {
            "vd_cull_compact": (lib.vd_cull_compact, [c0, m, 16, i, n, o, k, 0], [0, 1, 3, 5, 6], [3, 5]),
            "vd_cull_compact_views": (lib.vd_cull_compact_views, [c0, 3, m, 16, i, n, o, n, k, 0], [0, 2, 4, 6, 8], []),
            "vd_cull_compact_hiz": (lib.vd_cull_compact_hiz, [c0, m, 16, i, n, pyramid.ctypes.data, PYR_W, PYR_H, o, k, 0], [0, 1, 3, 5, 8, 9], []),
            "vd_cull_compact_lod": (lib.vd_cull_compact_lod, [s["lod_cam"].ctypes.data, P, s["groups"].ctypes.data, 16, s["rows"].ctypes.data, 64, i, n, o, k, 0],
                                    [0, 2, 4, 6, 8, 9], []),
            "vd_cull_batch": (lib.vd_cull_batch, [c0, m, 16, i, n, o, ids.ctypes.data, k], [0, 1, 3, 5, 6, 7], []),
            "vd_cull_emit": (lib.vd_cull_emit, [c0, m, 16, i, n, o], [0, 1, 3, 5], []),
        }
        for name, (fn, good, positions, zeroed) in forms.items():
            for pos in positions:
                args = list(good)
                count_passed = args[pos] != k
                args[pos] = None
                out.view(np.uint8)[:] = FILL
                ids[:], cnt[:] = SENTINEL, SENTINEL
                assert fn(h, *args) == abi.VD_ERR_INVALID_ARG, (name, pos)
                assert name.encode() + b":" in lib.vd_last_error(h), (name, pos, lib.vd_last_error(h))
                first = 0 if (pos in zeroed and count_passed) else SENTINEL
                assert cnt[0] == first and (cnt[1:] == SENTINEL).all(), (name, pos, cnt)
                assert (out.view(np.uint8) == FILL).all() and (ids == SENTINEL).all(), (name, pos)
            assert fn(h, *good) == abi.VD_OK, (name, lib.vd_last_error(h))       # the context still works after the refusals
    finally:
        ctx.close()
