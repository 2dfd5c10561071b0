"""Per-instance LOD selection on the GPU: vd_cull_compact_lod_dev / vd_cull_batch_lod_dev / vd_lod_ids_dev / vd_cull_compact_lod
(include/voidin_abi.h, "Level of detail") against tests/lod_cases.py - the oracle's frustum set and a numpy float32 twin of
the definition.  Every comparison is tobytes() ==; output buffers are pre-filled with 0xAB, the count word with a sentinel,
and what the contract says is not written must still hold its fill afterwards.

Sizes: a single instance, the seams of a 64-instance round, of a 1024-instance tile and of an 8192-instance chunk of the
expansion, 200 000 for every id width, and ONE size above 3 x 256 x 4 x 1024 instances, where pass 1's grid-stride loop is
first taken on 256 CUs.  Row counts 64 / 600 / 66 000 give 1-, 2- and 4-byte ids."""
import functools

import numpy as np
import pytest

import lod_cases as L
from voidin_amd import abi
from voidin_amd.runtime import EmitDraws

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EEDC0DE
GUARD = 64                  # bytes of 0xAB behind each output that must survive


@functools.lru_cache(maxsize=None)
def case(oracle_mod, n, n_rows=64, q=0.2):
    """(cam, P, base, meshes, groups, inst, expected): computed once, shared, never modified."""
    cam, P, base, meshes, groups, inst = L.scene(oracle_mod, n, n_rows, q)
    return cam, P, base, meshes, groups, inst, L.expect(oracle_mod, cam, P, base, meshes, groups, inst)


class Scene:
    """The device copies of one case."""

    def __init__(self, ctx, cam, P, base, meshes, groups, inst):
        self.cam, self.P, self.n, self.n_group, self.n_mesh = cam, P, len(inst), len(groups), len(meshes)
        self.d_g, self.d_m, self.d_b, self.d_i = ctx.upload(groups), ctx.upload(meshes), ctx.upload(base), ctx.upload(inst)


def count_words(ctx):
    import torch
    return torch.from_numpy(np.full(4, SENTINEL, np.uint32).view(np.int32)).to(ctx.torch_device)


def run_list(ctx, s, pad_tail=False, P=None):
    import torch
    d_out = torch.full((s.n * 20 + GUARD,), 0xAB, dtype=torch.uint8, device=ctx.torch_device)
    d_cnt = count_words(ctx)
    EmitDraws(ctx).record_lod(s.cam, s.P if P is None else P, s.d_g, s.n_group, s.d_m, s.n_mesh, s.d_i, s.n, d_out, d_cnt, pad_tail)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().tobytes(), d_cnt.cpu().numpy().view(np.uint32).copy()


def assert_list(got, want, n, pad_tail=False, tag=""):
    out, cnt = got
    k = len(want)
    print(f"{tag}: count {int(cnt[0])} (want {k}) of {n}")
    assert cnt[0] == k and (cnt[1:] == SENTINEL).all(), tag
    assert out[: 20 * k] == want.tobytes(), tag
    fill = b"\x00" if pad_tail else b"\xab"                                  # padded: zeroed up to n; else nothing behind the count
    assert out[20 * k: 20 * n] == fill * (20 * (n - k)), tag
    assert out[20 * n:] == b"\xab" * GUARD, tag


def run_batch(ctx, s, P=None):
    import torch
    d_cmds = torch.full((s.n_mesh * 20 + GUARD,), 0xAB, dtype=torch.uint8, device=ctx.torch_device)
    d_ids = torch.full((s.n * 4 + GUARD,), 0xAB, dtype=torch.uint8, device=ctx.torch_device)
    d_cnt = count_words(ctx)
    EmitDraws(ctx).record_batched_lod(s.cam, s.P if P is None else P, s.d_g, s.n_group, s.d_m, s.n_mesh, s.d_i, s.n, d_cmds, d_ids, d_cnt)
    torch.cuda.synchronize()
    return d_cmds.cpu().numpy().tobytes(), d_ids.cpu().numpy().tobytes(), d_cnt.cpu().numpy().view(np.uint32).copy()


def assert_batch(got, e, n, tag=""):
    cmds, ids, cnt = got
    k = len(e["ids"])
    assert cnt[0] == k and (cnt[1:] == SENTINEL).all(), tag
    assert cmds == e["cmds"].tobytes() + b"\xab" * GUARD, tag                # exactly one command per row
    assert int(np.frombuffer(cmds[:-GUARD], abi.DRAW)["instance_count"].sum()) == k, tag
    assert ids[: 4 * k] == e["ids"].tobytes(), tag
    assert ids[4 * k:] == b"\xab" * (4 * (n - k) + GUARD), tag


def run_ids(ctx, s, id_bytes):
    import torch
    d_ids = torch.full((s.n * id_bytes + GUARD,), 0xAB, dtype=torch.uint8, device=ctx.torch_device)
    ctx.lod_ids_dev(s.cam, s.P, s.d_g, s.n_group, s.n_mesh, s.d_i, s.n, d_ids, id_bytes)
    torch.cuda.synchronize()
    return d_ids


def assert_ids(d_ids, rows, id_bytes, n):
    got = d_ids.cpu().numpy().tobytes()
    assert got[: n * id_bytes] == rows.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[id_bytes]).tobytes()
    assert got[n * id_bytes:] == b"\xab" * GUARD


@pytest.mark.parametrize("n", L.SIZES)
def test_sizes(ctx, oracle, n):
    """A ragged round, a ragged tile, the seam of two expansion chunks, every workgroup with work: list, padded list,
    instanced form and the rows alone."""
    cam, P, base, meshes, groups, inst, e = case(oracle, n)
    s = Scene(ctx, cam, P, base, meshes, groups, inst)
    assert_list(run_list(ctx, s), e["list"], n, tag=f"{n}")
    assert_list(run_list(ctx, s, pad_tail=True), e["list"], n, pad_tail=True, tag=f"{n} padded")
    assert_batch(run_batch(ctx, s), e, n, tag=f"{n} batched")
    assert_ids(run_ids(ctx, s, 1), e["row"], 1, n)


@pytest.mark.parametrize("n_rows,id_bytes", [(600, 2), (66_000, 4)])
def test_id_widths(ctx, oracle, n_rows, id_bytes):
    n = 200_000
    cam, P, base, meshes, groups, inst, e = case(oracle, n, n_rows)
    assert len(np.unique(e["row"][e["drawn"]])) > 256 and e["row"].max() > (255 if id_bytes == 2 else 65535)
    s = Scene(ctx, cam, P, base, meshes, groups, inst)
    assert_list(run_list(ctx, s), e["list"], n, tag=f"{n_rows} rows")
    assert_list(run_list(ctx, s, pad_tail=True), e["list"], n, pad_tail=True, tag=f"{n_rows} rows padded")
    assert_ids(run_ids(ctx, s, id_bytes), e["row"], id_bytes, n)
    assert_ids(run_ids(ctx, s, 4), e["row"], 4, n)                          # a wider table than the rows need is allowed
    if n_rows <= abi.BATCH_MAX_MESHES:
        assert_batch(run_batch(ctx, s), e, n, tag=f"{n_rows} rows batched")
    else:
        with pytest.raises(Exception) as err:                                # VD_BATCH_MAX_MESHES applies to rows
            run_batch(ctx, s)
        assert getattr(err.value, "code", None) == abi.VD_ERR_INVALID_ARG


def test_grid_stride_loop(ctx, oracle):
    """More tiles than 3 workgroups per CU hold: some waves take a second tile."""
    import torch
    n = L.STRIDE_SIZE
    assert n > 3 * torch.cuda.get_device_properties(0).multi_processor_count * 4 * 1024
    cam, P, base, meshes, groups, inst, e = case(oracle, n)
    s = Scene(ctx, cam, P, base, meshes, groups, inst)
    assert_list(run_list(ctx, s), e["list"], n, tag="grid stride")
    assert_ids(run_ids(ctx, s, 1), e["row"], 1, n)


@pytest.mark.parametrize("n", [1025, 200_000])
def test_without_lods_it_is_the_plain_list(ctx, oracle, n):
    """min_size = 0: the survivors and their order are vd_cull_compact_dev's on the groups' boxes; with one LOD per group and
    first_row = g the bytes are."""
    import torch
    cam, P, base, meshes, groups, inst, e = case(oracle, n, 64, None)
    assert P["min_size"] == 0
    s = Scene(ctx, cam, P, base, meshes, groups, inst)
    d_plain, d_cnt = ctx.empty(n * 20), count_words(ctx)
    ctx.cull_compact_dev(cam, s.d_b, len(base), s.d_i, n, d_plain, d_cnt)
    torch.cuda.synchronize()
    k = int(d_cnt.cpu().numpy().view(np.uint32)[0])
    plain = d_plain.cpu().numpy()[: 20 * k].view(abi.DRAW)
    out, cnt = run_list(ctx, s)
    assert cnt[0] == k == int(e["F"].sum())
    assert np.frombuffer(out[: 20 * k], abi.DRAW)["base_instance"].tobytes() == plain["base_instance"].tobytes()
    flat = np.zeros(len(base), abi.LOD_GROUP)
    flat["min"], flat["max"], flat["n_lods"] = base["min"], base["max"], 1
    flat["first_row"] = np.arange(len(base))
    flat["switch_size"] = np.inf
    one = Scene(ctx, cam, P, base, base, flat, inst)
    out, cnt = run_list(ctx, one)
    assert cnt[0] == k and out[: 20 * k] == plain.tobytes()


@pytest.mark.parametrize("n_rows,id_bytes", [(64, 1), (600, 2), (66_000, 4)])
def test_composition(ctx, oracle, n_rows, id_bytes):
    """vd_lod_ids_dev + vd_cull_mask_dev on the groups' boxes + vd_expand_mask_dev == the fused call with min_size = 0."""
    import torch
    n = 200_000
    cam, P, base, meshes, groups, inst, e = case(oracle, n, n_rows, None)
    s = Scene(ctx, cam, P, base, meshes, groups, inst)
    fused, fused_cnt = run_list(ctx, s)
    d_ids = run_ids(ctx, s, id_bytes)
    d_mask = torch.zeros((n + 63) // 64, dtype=torch.int64, device=ctx.torch_device)
    ctx.cull_mask_dev(cam, s.d_b, len(base), s.d_i, n, d_mask)
    d_out = torch.full((n * 20 + GUARD,), 0xAB, dtype=torch.uint8, device=ctx.torch_device)
    d_cnt = count_words(ctx)
    ctx.expand_mask_dev(d_mask, n, n, d_ids, s.d_m, s.n_mesh, d_out, d_cnt, id_bytes=id_bytes)
    torch.cuda.synchronize()
    assert d_cnt.cpu().numpy().view(np.uint32)[0] == fused_cnt[0] == len(e["list"])
    assert d_out.cpu().numpy().tobytes() == fused
    assert fused[: 20 * len(e["list"])] == e["list"].tobytes()


def test_interleaved_with_the_plain_call_on_one_context(ctx, ctx_options, oracle):
    """The LOD pass and vd_cull_compact_dev share the context's id table: LOD with 1-byte ids, plain, LOD with 2-byte ids,
    plain - all above the split size of the plain call, so that it runs its own pass 1 into the same arena."""
    import torch
    n = 200_000
    a = case(oracle, n, 64)
    b = case(oracle, n, 600)
    sa, sb = Scene(ctx, *a[:6]), Scene(ctx, *b[:6])
    ctx_options("cull.split_min", 1)

    def plain(s, base, inst):
        d_out, d_cnt = ctx.empty(n * 20), count_words(ctx)
        ctx.cull_compact_dev(s.cam, s.d_b, len(base), s.d_i, n, d_out, d_cnt)
        torch.cuda.synchronize()
        k = int(d_cnt.cpu().numpy().view(np.uint32)[0])
        want, wn = oracle.compact(oracle.cull_emit(s.cam, base, inst, threads=8))
        assert k == wn and d_out.cpu().numpy()[: 20 * k].tobytes() == want[:wn].tobytes()

    for _ in range(2):
        assert_list(run_list(ctx, sa), a[6]["list"], n, tag="u8 ids")
        plain(sb, b[2], b[5])
        assert_list(run_list(ctx, sb), b[6]["list"], n, tag="u16 ids")
        plain(sa, a[2], a[5])


def test_replays_from_a_hip_graph_after_the_instances_moved(ctx, oracle):
    """One capture of vd_cull_compact_lod_dev; vd_compute_update_dev moves the instances between the replays.  Camera and
    parameters are baked in; every replay equals the twin on the moved instances."""
    import torch
    n = 200_000
    cam, P, base, meshes, groups, inst, e = case(oracle, n)
    s = Scene(ctx, cam, P, base, meshes, groups, inst)
    s.d_i = s.d_i.clone()
    d_out = torch.full((n * 20 + GUARD,), 0xAB, dtype=torch.uint8, device=ctx.torch_device)
    d_cnt = count_words(ctx)

    def frame():
        ctx.cull_compact_lod_dev(cam, P, s.d_g, s.n_group, s.d_m, s.n_mesh, s.d_i, n, d_out, d_cnt)

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
    idx = np.arange(n, dtype=np.uint32)
    d_idx = torch.from_numpy(idx.view(np.int32)).to(ctx.torch_device)
    host, lists = inst, [e["list"].tobytes()]
    for k in range(2):
        t, dt = 1.0 + k, 0.35
        ctx.compute_update_dev(d_idx, n, s.d_i, n, t, dt)
        host = oracle.compute_update(idx, host, t, dt)
        d_out.fill_(0xAB)
        d_cnt.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert s.d_i.cpu().numpy().tobytes() == host.tobytes()
        want = L.expect(oracle, cam, P, base, meshes, groups, host)
        assert_list((d_out.cpu().numpy().tobytes(), d_cnt.cpu().numpy().view(np.uint32)), want["list"], n, tag=f"replay {k}")
        lists.append(want["list"].tobytes())
    assert len(set(lists)) == 3                              # the instances did move: three different lists


def test_hand_made_instances(ctx, oracle):
    cam, P, base, meshes, groups, inst, where = L.hand_scene(oracle)
    e = L.expect(oracle, cam, P, base, meshes, groups, inst)
    n = len(inst)
    s = Scene(ctx, cam, P, base, meshes, groups, inst)
    assert_ids(run_ids(ctx, s, 1), e["row"], 1, n)           # every case, drawn or not
    assert_list(run_list(ctx, s), e["list"], n, tag="hand")
    assert_batch(run_batch(ctx, s), e, n, tag="hand batched")
    got = np.frombuffer(run_list(ctx, s)[0][: 20 * len(e["list"])], abi.DRAW)
    for name, i in where.items():
        if e["drawn"][i]:
            cmd = got[np.searchsorted(got["base_instance"], i)]
            assert cmd["base_instance"] == i and cmd["base_index"] == meshes["base_index"][e["row"][i]], name


def test_host_pointer_form(ctx, oracle):
    cam, P, base, meshes, groups, inst, e = case(oracle, 8193)
    for pad in (False, True):
        out, k = ctx.cull_compact_lod(cam, P, groups, meshes, inst, pad_tail=pad)
        assert k == len(e["list"]) and out[:k].tobytes() == e["list"].tobytes()
        tail = out[k:].tobytes()
        assert tail == (b"\x00" if pad else b"\xab") * len(tail)
