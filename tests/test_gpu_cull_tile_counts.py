"""The two-launch split form of vd_cull_compact: pass 1 leaves the survivors of every 1024-instance tile in scratch and
the expansion places its chunks from that table (no scan launch).  Everything is compared with the CPU oracle byte for
byte: the ordered list, the count and - with pad_tail - the whole buffer.

Sizes sit around the boundaries of pass 1's grid: W = 12 x CU count waves, one 1024-instance tile per wave and sweep.
With rem = n_tiles mod W tiles in the last sweep, the cases cover n_tiles = 1, < W, = W, W + 1, 2W - 1 and the rem
ranges (W/4, W/2], (W/8, W/4], (W/16, W/8] (a last sweep that fills a half, a quarter, an eighth of the grid), each with
n not a multiple of 64, a multiple of 64 but not of 1024, and a whole number of tiles."""
import numpy as np
import pytest

from voidin_amd import synth

pytestmark = pytest.mark.gpu

TILE = 1024
SMALL = dict(scale_range=(0.02, 0.6), extent=600.0)
BASELINE = dict(scale_range=(0.25, 4.0))


def grid_waves():
    import torch
    return 12 * torch.cuda.get_device_properties(0).multi_processor_count


def tile_groups(W):
    return {"one": 1, "below_W": W - 5, "W": W, "W_plus_1": W + 1, "2W_minus_1": 2 * W - 1,
            "rem_P2": W + W // 2 - 3, "rem_P4": W + W // 4 - 5, "rem_P8": W + W // 8 - 1}


def ragged(n_tiles):
    return {"not64": (n_tiles - 1) * TILE + 1000, "not1024": (n_tiles - 1) * TILE + 960, "whole": n_tiles * TILE}


def compact_dev(ctx, cam, d_m, n_mesh, inst, pad_tail=False, first_instance=0, d_out=None, d_cnt=None, fill=0xAB):
    import torch
    n = len(inst)
    d_i = ctx.upload(inst)
    if d_out is None:
        d_out = ctx.empty(n * 20 + 64)
    d_out.fill_(fill)
    if d_cnt is None:
        d_cnt = torch.zeros(4, dtype=torch.int32, device=ctx.torch_device)
    ctx.cull_compact_dev(cam, d_m, n_mesh, d_i, n, d_out, d_cnt, pad_tail, first_instance)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), int(d_cnt[0].item()) & 0xFFFFFFFF


def check(ctx, oracle, cam, meshes, inst, first_instance=0, d_m=None, tag=""):
    """List + count, then the padded buffer; bytes past the written part keep the fill pattern."""
    n = len(inst)
    want = oracle.cull_emit(cam, meshes, inst, threads=8)
    want["base_instance"] += np.uint32(first_instance)
    wc, wn = oracle.compact(want)
    wp, wpn = oracle.compact(want, pad_tail=True)
    d_m = ctx.upload(meshes) if d_m is None else d_m
    got, cnt = compact_dev(ctx, cam, d_m, len(meshes), inst, False, first_instance)
    print(f"{tag} n={n} survivors={wn} got={cnt}")
    assert cnt == wn, tag
    assert got[: wn * 20].tobytes() == wc[:wn].tobytes(), tag
    assert (got[wn * 20:] == 0xAB).all(), tag                  # nothing written past the list
    got, cnt = compact_dev(ctx, cam, d_m, len(meshes), inst, True, first_instance)
    assert cnt == wpn == wn, tag
    assert got[: n * 20].tobytes() == wp.tobytes(), tag
    assert (got[n * 20:] == 0xAB).all(), tag
    return wn


@pytest.mark.parametrize("shape", ["not64", "not1024", "whole"])
@pytest.mark.parametrize("group", ["one", "below_W", "W", "W_plus_1", "2W_minus_1", "rem_P2", "rem_P4", "rem_P8"])
def test_sizes_around_the_grid_boundaries(ctx, ctx_options, oracle, group, shape):
    n = ragged(tile_groups(grid_waves())[group])[shape]
    cam, meshes = synth.camera_uniform(), synth.mesh_infos()
    inst = synth.instances(n, seed=synth.SEED_BASE + 80, with_inverse=False, **SMALL)
    ctx_options("cull.split_min", 1)
    wn = check(ctx, oracle, cam, meshes, inst, tag=f"{group}/{shape}")
    assert 0 < wn < n


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 70_000])
def test_small_inputs_through_the_split_form(ctx, ctx_options, oracle, n):
    cam, meshes = synth.camera_uniform(), synth.mesh_infos()
    inst = synth.instances(n, seed=synth.SEED_BASE + 81, with_inverse=False, **BASELINE)
    ctx_options("cull.split_min", 1)
    check(ctx, oracle, cam, meshes, inst, tag=f"small {n}")


@pytest.mark.parametrize("n", [70_001, 3_200_123])
@pytest.mark.parametrize("n_mesh", [16, 300, 70_000])
def test_three_id_widths(ctx, ctx_options, oracle, n_mesh, n):
    """1-byte ids run expand_mask_u8_kernel, 2- and 4-byte ids expand_mask_kernel (LDS mesh table up to 512 entries, global beyond)."""
    cam = synth.camera_uniform()
    meshes = synth.mesh_infos(n_mesh, seed=synth.SEED_BASE + 82)
    if n_mesh > 60_000:                                   # base_index would overflow u32 with the default index counts
        meshes["index_count"] = 36
        meshes["base_index"] = np.arange(n_mesh, dtype=np.uint32) * 36
        meshes["vertex_offset"] = np.arange(n_mesh, dtype=np.int32) * 12
    inst = synth.instances(n, n_mesh=n_mesh, seed=synth.SEED_BASE + 83, with_inverse=False, **SMALL)
    ctx_options("cull.split_min", 1)
    check(ctx, oracle, cam, meshes, inst, tag=f"n_mesh {n_mesh}")


@pytest.mark.parametrize("n", [5_000, 3_200_123])
def test_nothing_everything_and_the_baseline_cloud(ctx, ctx_options, oracle, n):
    meshes = synth.mesh_infos()
    ctx_options("cull.split_min", 1)
    # nothing visible: a camera that looks away from a cloud that lies wholly behind it
    cam = synth.camera_uniform(eye=(0.0, 0.0, 0.0), pitch_deg=0.0)
    inst = synth.instances(n, seed=synth.SEED_BASE + 84, scale_range=(0.01, 0.02), extent=10.0, with_inverse=False)
    t = inst["transform"].reshape(n, 16)
    t[:, 14] = np.float32(5000.0)                          # +z = behind an unrotated camera at the origin
    assert check(ctx, oracle, cam, meshes, inst, tag="nothing") == 0
    t[:, 12:14] = np.float32(0.0)
    t[:, 14] = np.float32(-50.0)                           # straight ahead, on the axis
    assert check(ctx, oracle, cam, meshes, inst, tag="everything") == n
    inst = synth.instances(n, seed=synth.SEED_BASE + 2, with_inverse=False, **BASELINE)
    assert 0 < check(ctx, oracle, synth.camera_uniform(), meshes, inst, tag="baseline") < n


def test_first_instance_offset(ctx, ctx_options, oracle):
    cam, meshes = synth.camera_uniform(), synth.mesh_infos()
    inst = synth.instances(3_150_001, seed=synth.SEED_BASE + 85, with_inverse=False, **SMALL)
    ctx_options("cull.split_min", 1)
    check(ctx, oracle, cam, meshes, inst, first_instance=7_654_321, tag="first_instance")


def test_consecutive_calls_on_one_context(ctx, ctx_options, oracle):
    """Other mesh assignments, then a smaller and a larger n (scratch regrown, table moved): what an earlier call left in
    the table must not reach a count.  Own context, so that the scratch starts small."""
    import torch
    from voidin_amd.runtime import Context
    cam, meshes = synth.camera_uniform(), synth.mesh_infos()
    own = Context(0)
    try:
        own.set_option("cull.split_min", 1)
        d_m = own.upload(meshes)
        a = synth.instances(400_000, seed=synth.SEED_BASE + 86, with_inverse=False, **BASELINE)    # many survivors per tile
        b = a.copy(); b["mesh"] = (b["mesh"] + 3) % len(meshes)
        c = synth.instances(90_000, seed=synth.SEED_BASE + 87, with_inverse=False, **SMALL)        # fewer tiles, few survivors
        d = synth.instances(3_300_000, seed=synth.SEED_BASE + 88, with_inverse=False, **SMALL)     # scratch regrown
        for name, inst in [("a", a), ("b", b), ("c", c), ("a", a), ("d", d), ("c", c), ("b", b)]:
            check(own, oracle, cam, meshes, inst, d_m=d_m, tag=f"sequence {name}")
    finally:
        own.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [9_000, 2_500_000])
def test_foreign_mask_still_goes_through_the_scan(ctx, oracle, n):
    """vd_expand_mask_dev and vd_mask_to_indices_dev get a mask without tile counts: mask_scan_kernel places their chunks."""
    import torch
    cam, meshes = synth.camera_uniform(), synth.mesh_infos()
    inst = synth.instances(n, seed=synth.SEED_BASE + 89, with_inverse=False, **SMALL)
    want = oracle.cull_emit(cam, meshes, inst, threads=8)
    wc, wn = oracle.compact(want)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    d_mask = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    ctx.cull_mask_dev(cam, d_m, len(meshes), d_i, n, d_mask)
    d_ids = ctx.upload(inst["mesh"].astype(np.uint8))
    d_out, d_cnt = ctx.empty(n * 20), torch.zeros(4, dtype=torch.int32, device="cuda")
    for _ in range(2):                                     # twice: the scan's epoch advances between launches
        d_cnt.zero_()
        ctx.expand_mask_dev(d_mask, n, n, d_ids, d_m, len(meshes), d_out, d_cnt, id_bytes=1)
        torch.cuda.synchronize()
        assert int(d_cnt[0].item()) == wn
        assert d_out.cpu().numpy()[: wn * 20].tobytes() == wc[:wn].tobytes()
    d_idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_cnt.zero_()
    ctx.mask_to_indices_dev(d_mask, n, 100, d_idx, d_cnt)
    torch.cuda.synchronize()
    assert int(d_cnt[0].item()) == wn
    want_idx = (np.nonzero(want["instance_count"] == 1)[0] + 100).astype(np.uint32)
    assert d_idx.cpu().numpy()[:wn].view(np.uint32).tobytes() == want_idx.tobytes()
