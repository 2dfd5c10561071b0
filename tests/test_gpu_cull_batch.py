"""Instanced draw lists on the GPU: vd_cull_batch_dev / vd_batch_mask_dev / vd_cull_batch (include/voidin_abi.h, "Instanced
draw lists") against the CPU oracle's emit_draws output, regrouped in numpy:

    S = the instances the oracle keeps, ascending;  mid = min(mesh, n_mesh - 1)
    ids = S stably sorted by mid;  cmds[m] = {index_count, |S_m|, base_index, vertex_offset, sum of |S_k| over k < m}

and, as a second and independent pin, against the GPU's own vd_cull_compact_dev: its base_instance column, stably sorted by
mesh, is the id list.  Every comparison is tobytes() ==; output buffers are pre-filled with 0xAB, the count word with a
sentinel, and every byte the contract says is not written (ids behind the count, anything behind the n_mesh commands, the
words next to the count) must still hold its fill afterwards.

Survivor shares by the oracle at 300 007 instances, 16 meshes, the default camera narrowed to a 30 degree field of view
(asserted below, 5 % .. 95 % each): wide 94.4 %, small 13.4 %, mid 87.1 %.  (emit_draws' bounding radius is generous -
shaders/emit_draws.wgsl:19 - so only small instances are ever culled; under the default 90 degrees wide keeps 95.5 %.)"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from conftest import golden
from voidin_amd import abi, synth
from voidin_amd.runtime import EmitDraws

pytestmark = pytest.mark.gpu

CLOUDS = {"wide": dict(scale_range=(0.25, 4.0)), "small": dict(scale_range=(0.02, 0.6), extent=600.0),
          "mid": dict(scale_range=(0.5, 1.2), extent=1500.0)}        # tests/test_gpu_cull.py's three
SENTINEL = 0x5EEDC0DE
FOVY = math.pi / 6          # under the default 90 degrees the wide cloud keeps 95.5 %: too few culled
GUARD = 64                  # bytes of 0xAB behind each output that must survive
FRONT = dict(centre=(2.0, -2.0, -10.0), extent=6.0, scale_range=(0.5, 1.0))      # a cluster the default camera sees whole


def regroup(vis, mesh_col, meshes):
    """(cmds, ids) of the contract from a visibility vector and the instances' mesh ids."""
    n_mesh = len(meshes)
    S = np.flatnonzero(vis)
    mid = np.minimum(mesh_col, n_mesh - 1)[S].astype(np.int64)
    ids = S[np.argsort(mid, kind="stable")].astype(np.uint32)
    cnt = np.bincount(mid, minlength=n_mesh)
    base = np.cumsum(cnt) - cnt
    cmds = np.zeros(n_mesh, abi.DRAW)
    cmds["vertex_count"], cmds["instance_count"], cmds["base_index"] = meshes["index_count"], cnt, meshes["base_index"]
    cmds["vertex_offset"], cmds["base_instance"] = meshes["vertex_offset"], base
    return cmds, ids


@functools.lru_cache(maxsize=None)
def scene(cloud, n, n_mesh=16, edit=None):
    """(camera, meshes, instances): computed once, shared, never modified."""
    cam, meshes = synth.camera_uniform(fovy=FOVY), synth.mesh_infos(n_mesh)
    kw = FRONT if cloud == "front" else CLOUDS[cloud]
    inst = synth.instances(n, n_mesh=n_mesh, seed=synth.SEED_BASE + 2, with_inverse=False, **kw)
    i = np.arange(n, dtype=np.uint32)
    if edit == "clamp":                      # a tenth of the instances beyond the table: they belong to mesh n_mesh - 1
        inst["mesh"][i % 10 == 3] = n_mesh
        inst["mesh"][i % 20 == 7] = 0xFFFFFFFF
    elif edit == "distinct":                 # every round of 64 holds 64 distinct ids
        inst["mesh"] = (i + i // 64) % 64
    elif edit == "one":                      # every round holds one id
        inst["mesh"] = (i // 64 * 37) % 64
    elif edit == "runs":                     # sorted ids in runs of 1000
        inst["mesh"] = i // 1000
    elif edit == "two":                      # only meshes 3 and 200 occur among 256
        inst["mesh"] = np.where(synth.uniform01(synth.SEED_BASE + 5, 3, n) < 0.3, 3, 200)
    elif edit == "shift":                    # every mesh id differs from the unedited scene's
        inst["mesh"] = (inst["mesh"] + 1) % n_mesh
    return cam, meshes, inst


@functools.lru_cache(maxsize=None)
def expected(oracle_mod, cloud, n, n_mesh=16, edit=None, away=False):
    cam, meshes, inst = scene(cloud, n, n_mesh, edit)
    if away:        # turned round, with a finite far plane: behind the camera the generous radius of emit_draws.wgsl:19 passes
        cam = synth.camera_uniform(yaw_deg=180.0, pitch_deg=0.0, fovy=FOVY).copy()      # the side planes, the far test does not
        cam["zfar"] = np.float32(-1e6)
    vis = oracle_mod.cull_emit(cam, meshes, inst, threads=8)["instance_count"] == 1
    cmds, ids = regroup(vis, inst["mesh"], meshes)
    return cam, vis, cmds, ids


class Buffers:
    """Device outputs with their fills: n_mesh commands + guard, n ids + guard, four count words."""

    def __init__(self, ctx, n, n_mesh):
        import torch
        self.n, self.n_mesh = n, n_mesh
        self.cmds = torch.full((n_mesh * 20 + GUARD,), 0xAB, dtype=torch.uint8, device=ctx.torch_device)
        self.ids = torch.full((n * 4 + GUARD,), 0xAB, dtype=torch.uint8, device=ctx.torch_device)
        self.cnt = torch.from_numpy(np.full(4, SENTINEL, np.uint32).view(np.int32)).to(ctx.torch_device)

    def read(self):
        import torch
        torch.cuda.synchronize()
        return self.cmds.cpu().numpy().tobytes(), self.ids.cpu().numpy().tobytes(), self.cnt.cpu().numpy().view(np.uint32).copy()

    def untouched(self):
        cmds, ids, cnt = self.read()
        return cmds == b"\xab" * len(cmds) and ids == b"\xab" * len(ids) and (cnt == SENTINEL).all()


def assert_contract(got, cmds, ids, n, tag=""):
    g_cmds, g_ids, g_cnt = got
    k = len(ids)
    print(f"{tag}: count {int(g_cnt[0])} (want {k}) of {n}")
    assert g_cnt[0] == k and (g_cnt[1:] == SENTINEL).all(), tag
    assert g_cmds == cmds.tobytes() + b"\xab" * GUARD, tag                       # exactly n_mesh commands
    assert g_ids[: 4 * k] == ids.tobytes(), tag
    assert g_ids[4 * k:] == b"\xab" * (4 * (n - k) + GUARD), tag                   # words [|S|, n_inst) are not written


def run(ctx, cam, meshes, inst, d_m=None, d_i=None):
    n = len(inst)
    d_m = ctx.upload(meshes) if d_m is None else d_m
    d_i = ctx.upload(inst) if d_i is None else d_i
    b = Buffers(ctx, n, len(meshes))
    ctx.cull_batch_dev(cam, d_m, len(meshes), d_i, n, b.cmds, b.ids, b.cnt)
    return b.read()


def compact_ids(ctx, cam, meshes, inst):
    """The independent pin: vd_cull_compact_dev's base_instance column, stably sorted by clamped mesh id."""
    import torch
    n = len(inst)
    d_out, d_cnt = ctx.empty(n * 20), torch.zeros(4, dtype=torch.int32, device=ctx.torch_device)
    ctx.cull_compact_dev(cam, ctx.upload(meshes), len(meshes), ctx.upload(inst), n, d_out, d_cnt)
    torch.cuda.synchronize()
    k = int(d_cnt[0].item())
    S = d_out.cpu().numpy()[: k * 20].view(abi.DRAW)["base_instance"].astype(np.int64)
    mid = np.minimum(inst["mesh"], len(meshes) - 1)[S].astype(np.int64)
    return S[np.argsort(mid, kind="stable")].astype(np.uint32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 300_007])
@pytest.mark.parametrize("cloud", ["wide", "small", "mid"])
def test_sizes(ctx, oracle, cloud, n):
    """A ragged round, a ragged pass-1 tile, the seams between two waves' ranges, every wave with work."""
    cam, meshes, inst = scene(cloud, n)
    _, vis, cmds, ids = expected(oracle, cloud, n)
    if n == 300_007:
        share = vis.mean()
        print(f"{cloud}: {100 * share:.1f} % survive")
        assert 0.05 <= share <= 0.95
    assert_contract(run(ctx, cam, meshes, inst), cmds, ids, n, f"{cloud}/{n}")
    assert compact_ids(ctx, cam, meshes, inst).tobytes() == ids.tobytes()


@pytest.mark.parametrize("n_mesh", [1, 2, 256, 257, 4096])
def test_id_widths_and_the_mesh_limit(ctx, oracle, n_mesh):
    """1-byte rows up to 256 meshes, 2-byte rows beyond, the 16 KB table at 4096 (4-byte rows: test_batch_mask_*)."""
    n = 300_007
    cam, meshes, inst = scene("wide", n, n_mesh)
    _, vis, cmds, ids = expected(oracle, "wide", n, n_mesh)
    assert 0.05 <= vis.mean() <= 0.95
    assert_contract(run(ctx, cam, meshes, inst), cmds, ids, n, f"n_mesh={n_mesh}")


def test_one_mesh_more_than_the_limit_is_refused(ctx):
    n, n_mesh = 1000, abi.BATCH_MAX_MESHES + 1
    cam, meshes = synth.camera_uniform(), synth.mesh_infos(n_mesh)
    inst = synth.instances(n, n_mesh=n_mesh, with_inverse=False)
    b = Buffers(ctx, n, n_mesh)
    rc = ctx.lib.vd_cull_batch_dev(ctx.h, cam.ctypes.data, ctx.upload(meshes).data_ptr(), n_mesh, ctx.upload(inst).data_ptr(), n,
                                   b.cmds.data_ptr(), b.ids.data_ptr(), b.cnt.data_ptr())
    assert rc == abi.VD_ERR_INVALID_ARG
    msg = ctx.lib.vd_last_error(ctx.h).decode()
    assert "one-digit counting sort" in msg and "second sort digit is future work" in msg, msg
    assert b.untouched()


def test_mesh_ids_beyond_the_table_land_in_the_last_group(ctx, oracle):
    n = 300_007
    cam, meshes, inst = scene("wide", n, 16, "clamp")
    _, vis, cmds, ids = expected(oracle, "wide", n, 16, "clamp")
    beyond = vis & (inst["mesh"] >= 16)
    assert beyond.sum() > 1000                                              # visible instances with an id to clamp exist
    got = run(ctx, cam, meshes, inst)
    assert_contract(got, cmds, ids, n, "clamp")
    last = ids[cmds["base_instance"][15]: cmds["base_instance"][15] + cmds["instance_count"][15]]
    assert set(np.flatnonzero(beyond)) <= set(last.tolist())
    assert compact_ids(ctx, cam, meshes, inst).tobytes() == ids.tobytes()


@pytest.mark.parametrize("edit", ["distinct", "one", "runs"])
def test_rank_within_a_round(ctx, oracle, edit):
    """All 4096 instances survive; 64 distinct ids per round (the longest walk of a loop over distinct ids), one id per
    round, and sorted runs of 1000 that straddle rounds and wave ranges."""
    n, n_mesh = 4096, 64
    cam, meshes, inst = scene("front", n, n_mesh, edit)
    _, vis, cmds, ids = expected(oracle, "front", n, n_mesh, edit)
    assert vis.all()
    if edit == "distinct":
        assert all(len(set(inst["mesh"][r: r + 64].tolist())) == 64 for r in range(0, n, 64))
    if edit == "one":
        assert all(len(set(inst["mesh"][r: r + 64].tolist())) == 1 for r in range(0, n, 64))
    assert_contract(run(ctx, cam, meshes, inst), cmds, ids, n, edit)


def test_empty_groups_and_extremes(ctx, oracle):
    n = 100_003
    cam, meshes, inst = scene("wide", n, 256, "two")                        # only ids 3 and 200 occur among 256
    _, vis, cmds, ids = expected(oracle, "wide", n, 256, "two")
    assert set(np.flatnonzero(cmds["instance_count"]).tolist()) == {3, 200}
    assert (cmds["base_instance"][201:] == len(ids)).all()
    assert_contract(run(ctx, cam, meshes, inst), cmds, ids, n, "two meshes of 256")
    n = 20_001
    cam, meshes, inst = scene("front", n)                                    # wholly visible ...
    _, vis, cmds, ids = expected(oracle, "front", n)
    assert vis.all()
    assert_contract(run(ctx, cam, meshes, inst), cmds, ids, n, "all visible")
    away, vis, cmds, ids = expected(oracle, "front", n, away=True)            # ... and, with the camera turned round, not at all
    assert not vis.any() and not cmds["instance_count"].any() and not cmds["base_instance"].any()
    assert_contract(run(ctx, away, meshes, inst), cmds, ids, n, "none visible")


def _mask_of(ctx, cam, d_m, n_mesh, d_i, n):
    import torch
    d_mask = torch.zeros((n + 63) // 64, dtype=torch.int64, device=ctx.torch_device)
    ctx.cull_mask_dev(cam, d_m, n_mesh, d_i, n, d_mask)
    return d_mask


@pytest.mark.parametrize("width", [np.uint8, np.uint16, np.uint32])
def test_batch_mask_equals_cull_batch(ctx, oracle, width):
    """vd_batch_mask_dev on vd_cull_mask_dev's bits with a caller-supplied id table of each width (the 4-byte table holds the
    RAW ids, beyond-the-table ones included: the clamp is the call's)."""
    n = 300_007
    cam, meshes, inst = scene("wide", n, 16, "clamp")
    _, _, cmds, ids = expected(oracle, "wide", n, 16, "clamp")
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    table = inst["mesh"].copy() if width is np.uint32 else np.minimum(inst["mesh"], 15).astype(width)
    d_mask = _mask_of(ctx, cam, d_m, 16, d_i, n)
    b = Buffers(ctx, n, 16)
    ctx.batch_mask_dev(d_mask, n, ctx.upload(table), d_m, 16, b.cmds, b.ids, b.cnt, id_bytes=table.itemsize)
    got = b.read()
    assert_contract(got, cmds, ids, n, f"mask, {table.itemsize}-byte ids")
    ref = run(ctx, cam, meshes, inst, d_m, d_i)
    assert got[0] == ref[0] and got[1] == ref[1] and (got[2] == ref[2]).all()


def test_batch_mask_groups_an_occlusion_refined_mask(ctx):
    import torch
    g = golden("occlusion_1500.npz")
    h, w = g["depth"].shape
    meshes, inst = g["meshes"], g["instances"]
    n, n_mesh = len(inst), len(meshes)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    d_pyr = torch.zeros(len(g["pyramid"]), dtype=torch.float32, device="cuda")
    ctx.hiz_build_dev(ctx.upload(g["depth"]), w, h, d_pyr)
    d_in = ctx.upload(g["mask_in"].view(np.int64))
    d_out = torch.zeros_like(d_in)
    ctx.occlusion_mask_dev(g["camera"], d_m, n_mesh, d_i, n, d_pyr, w, h, d_in, d_out)
    mask = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(mask, g["mask_out"])
    vis = np.unpackbits(mask.view(np.uint8), bitorder="little")[:n].astype(bool)
    assert 0 < vis.sum() < np.unpackbits(g["mask_in"].view(np.uint8)).sum()  # the pyramid removed something, not everything
    cmds, ids = regroup(vis, inst["mesh"], meshes)
    b = Buffers(ctx, n, n_mesh)
    ctx.batch_mask_dev(d_out, n, ctx.upload(np.ascontiguousarray(inst["mesh"])), d_m, n_mesh, b.cmds, b.ids, b.cnt, id_bytes=4)
    assert_contract(b.read(), cmds, ids, n, "occlusion mask")


def test_state_between_calls(ctx, oracle):
    """Same bytes twice; a scene whose every mesh id changed (the id rows are rewritten); a smaller and then a larger scene and
    more meshes on the same context (scratch regrowth); a vd_cull_compact_dev call in between keeps its own bytes."""
    n = 300_007
    cam, meshes, inst = scene("wide", n)
    _, _, cmds, ids = expected(oracle, "wide", n)
    first = run(ctx, cam, meshes, inst)
    second = run(ctx, cam, meshes, inst)
    assert first[0] == second[0] and first[1] == second[1] and (first[2] == second[2]).all()
    assert_contract(second, cmds, ids, n, "repeat")
    _, meshes2, inst2 = scene("wide", n, 16, "shift")
    assert (inst2["mesh"] != inst["mesh"]).all()
    _, _, cmds2, ids2 = expected(oracle, "wide", n, 16, "shift")
    assert_contract(run(ctx, cam, meshes2, inst2), cmds2, ids2, n, "every id changed")
    want_compact = oracle.compact(oracle.cull_emit(cam, meshes, inst, threads=8))
    for cloud, m, n_mesh in (("small", 1025, 16), ("mid", 300_007, 16), ("wide", 300_007, 4096), ("wide", 300_007, 16)):
        c, ms, it = scene(cloud, m, n_mesh)
        _, _, cm, ii = expected(oracle, cloud, m, n_mesh)
        assert_contract(run(ctx, c, ms, it), cm, ii, m, f"after resize: {cloud}/{m}/{n_mesh}")
        # the compacted list of the first scene in between: ctx->scratch is rewritten by it, the batch arena is not
        import torch
        d_out, d_cnt = ctx.empty(n * 20), torch.zeros(4, dtype=torch.int32, device=ctx.torch_device)
        d_out.fill_(0xAB)
        ctx.cull_compact_dev(cam, ctx.upload(meshes), 16, ctx.upload(inst), n, d_out, d_cnt)
        torch.cuda.synchronize()
        k = int(d_cnt[0].item())
        assert k == want_compact[1] and d_out.cpu().numpy()[: k * 20].tobytes() == want_compact[0][:k].tobytes()
        assert (d_out.cpu().numpy()[k * 20: n * 20] == 0xAB).all()


def test_replays_from_a_hip_graph(ctx, oracle):
    """After a warm-up call sized the scratch, one vd_cull_batch_dev is only kernel launches: captured once, replayed twice
    into cleared buffers, the bytes are the eager call's."""
    import torch
    n = 300_007
    cam, meshes, inst = scene("mid", n)
    _, _, cmds, ids = expected(oracle, "mid", n)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    eager = run(ctx, cam, meshes, inst, d_m, d_i)                            # warm-up
    assert_contract(eager, cmds, ids, n, "eager")
    b = Buffers(ctx, n, 16)
    emit = EmitDraws(ctx)
    graph = torch.cuda.CUDAGraph()
    main_stream = torch.cuda.current_stream().cuda_stream
    try:
        with torch.cuda.graph(graph):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            emit.record_batched(cam, d_m, 16, d_i, n, b.cmds, b.ids, b.cnt)
    finally:
        ctx.set_stream(main_stream)
    for _ in range(2):
        b.cmds.fill_(0xAB); b.ids.fill_(0xAB); b.cnt.fill_(int(np.uint32(SENTINEL).view(np.int32)))
        graph.replay()
        got = b.read()
        assert got[0] == eager[0] and got[1] == eager[1] and (got[2] == eager[2]).all()


def test_three_million_instances_4096_meshes(ctx, oracle):
    """Many rounds per wave range, the column scan at full width, random ids."""
    n, n_mesh = 3_000_001, 4096
    cam, meshes, inst = scene("wide", n, n_mesh)
    _, vis, cmds, ids = expected(oracle, "wide", n, n_mesh)
    assert (cmds["instance_count"] > 0).sum() > 4000
    assert_contract(run(ctx, cam, meshes, inst), cmds, ids, n, "3 M / 4096")


def test_host_pointer_form_and_stage_timing(ctx, oracle):
    n = 100_003
    cam, meshes, inst = scene("small", n)
    _, _, cmds, ids = expected(oracle, "small", n)
    g_cmds, g_ids, k = ctx.cull_batch(cam, meshes, inst)
    assert k == len(ids) and g_cmds.tobytes() == cmds.tobytes() and g_ids.tobytes() == ids.tobytes()
    raw = np.full(n + 16, 0xABABABAB, np.uint32)                             # behind the count the host buffer is untouched too
    cnt, out = C.c_uint32(SENTINEL), np.zeros(16, abi.DRAW)
    assert ctx.lib.vd_cull_batch(ctx.h, cam.ctypes.data, meshes.ctypes.data, 16, inst.ctypes.data, n, out.ctypes.data, raw.ctypes.data,
                                 C.addressof(cnt)) == abi.VD_OK
    assert cnt.value == k and raw[:k].tobytes() == ids.tobytes() and (raw[k:] == 0xABABABAB).all()
    ctx.set_timing(True)
    try:
        run(ctx, cam, meshes, inst)
        s0, s1, total = ctx.last_gpu_ms_stage(0), ctx.last_gpu_ms_stage(1), ctx.last_gpu_ms()
        assert s0 > 0 and s1 > 0 and abs(s0 + s1 - total) < 0.05 * total + 0.02   # the same three events, (s0, s1, total)
    finally:
        ctx.set_timing(False)


def test_invalid_arguments_and_empty_input(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    n, n_mesh = 1000, 16
    cam, meshes = synth.camera_uniform(), synth.mesh_infos(n_mesh)
    inst = synth.instances(n, with_inverse=False)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    d_mask = torch.zeros(16, dtype=torch.int64, device=ctx.torch_device)
    d_tab = torch.zeros(n, dtype=torch.int32, device=ctx.torch_device)
    b = Buffers(ctx, n, n_mesh)
    P = lambda t: t.data_ptr()
    good_cull = [cam.ctypes.data, P(d_m), n_mesh, P(d_i), n, P(b.cmds), P(b.ids), P(b.cnt)]
    good_mask = [P(d_mask), n, P(d_tab), 4, P(d_m), n_mesh, P(b.cmds), P(b.ids), P(b.cnt)]

    def bad(fn, good, **change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        assert fn(h, *args) == abi.VD_ERR_INVALID_ARG, change
        assert lib.vd_last_error(h), change
        assert b.untouched(), change

    for k in (0, 1, 5, 7):                                                   # camera, meshes, cmds, count
        bad(lib.vd_cull_batch_dev, good_cull, **{f"a{k}": None})
    bad(lib.vd_cull_batch_dev, good_cull, a2=0)
    bad(lib.vd_cull_batch_dev, good_cull, a2=abi.BATCH_MAX_MESHES + 1)
    bad(lib.vd_cull_batch_dev, good_cull, a3=None)                           # instances, n_inst > 0
    bad(lib.vd_cull_batch_dev, good_cull, a6=None)                           # instance ids, n_inst > 0
    for k in (4, 6, 8):                                                      # meshes, cmds, count
        bad(lib.vd_batch_mask_dev, good_mask, **{f"a{k}": None})
    bad(lib.vd_batch_mask_dev, good_mask, a5=0)
    bad(lib.vd_batch_mask_dev, good_mask, a5=abi.BATCH_MAX_MESHES + 1)
    assert "one-digit counting sort" in lib.vd_last_error(h).decode()
    for width in (0, 3, 8):
        bad(lib.vd_batch_mask_dev, good_mask, a3=width)
        bad(lib.vd_batch_mask_dev, good_mask, a1=0, a3=width)                # ... also with nothing to group
    for k in (0, 2, 7):                                                      # mask, ids, instance ids with n_inst > 0
        bad(lib.vd_batch_mask_dev, good_mask, **{f"a{k}": None})
    # host form: null camera / meshes / cmds / count, the limit, null instances / ids with n_inst > 0
    out, ids, cnt = np.full(n_mesh * 20, 0xAB, np.uint8), np.full(n, 0xABABABAB, np.uint32), np.full(1, SENTINEL, np.uint32)
    good_host = [cam.ctypes.data, meshes.ctypes.data, n_mesh, inst.ctypes.data, n, out.ctypes.data, ids.ctypes.data, cnt.ctypes.data]
    for change in ({"a0": None}, {"a1": None}, {"a5": None}, {"a7": None}, {"a2": 0}, {"a2": abi.BATCH_MAX_MESHES + 1}, {"a3": None}, {"a6": None}):
        bad(lib.vd_cull_batch, good_host, **change)
        assert (out == 0xAB).all() and (ids == 0xABABABAB).all() and cnt[0] == SENTINEL, change
    # n_inst == 0: n_mesh commands with instance_count = 0 and base_instance = 0, count 0 - null instances / ids allowed
    want = np.zeros(n_mesh, abi.DRAW)
    want["vertex_count"], want["base_index"], want["vertex_offset"] = meshes["index_count"], meshes["base_index"], meshes["vertex_offset"]
    for call in (lambda e: lib.vd_cull_batch_dev(h, cam.ctypes.data, P(d_m), n_mesh, None, 0, P(e.cmds), None, P(e.cnt)),
                 lambda e: lib.vd_batch_mask_dev(h, None, 0, None, 4, P(d_m), n_mesh, P(e.cmds), None, P(e.cnt))):
        e = Buffers(ctx, 0, n_mesh)
        assert call(e) == abi.VD_OK
        assert_contract(e.read(), want, np.zeros(0, np.uint32), 0, "empty")
    cnt[0] = SENTINEL
    assert lib.vd_cull_batch(h, cam.ctypes.data, meshes.ctypes.data, n_mesh, None, 0, out.ctypes.data, None, cnt.ctypes.data) == abi.VD_OK
    assert cnt[0] == 0 and out.tobytes() == want.tobytes()
