"""The mask -> draw-list expansion of voidin_amd/csrc/cull.hip on hand-made masks (tests/mask_cases.py): launch_expand and
its kernels, mask_scan_kernel, the indices wire format, pad_tail_kernel and the C3 compaction, byte for byte against the
numpy references, with a canary behind everything a call may write.

Every output buffer is allocated at its full contractual size plus a guard, filled with 0xC3 on the device before the
call, and checked afterwards: the count, the bytes of [0, count), and that every other byte of the allocation - behind
the count, behind the buffer, and in front of a buffer that does not start at the allocation - is still 0xC3 (with
pad_tail [count, n) is zero instead).  The untouched part is compared on the device; only [0, count) is copied back.

Which instantiation of launch_expand a group of cases reaches is noted at each test."""
import ctypes as C

import numpy as np
import pytest

import mask_cases as mc
from voidin_amd import abi

pytestmark = pytest.mark.gpu

CANARY = 0xC3
GUARD = 4096                                   # canary bytes behind the contractual size
SEAM_SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 16385, 24577]
ID_TYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}
BASES = [0, 4, 8, 12]                          # bytes past a 16-byte boundary


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded:
    """`nbytes` bytes that start `base` bytes past a 16-byte boundary, inside an allocation filled with the canary."""

    def __init__(self, nbytes, base=0):
        import torch
        self.raw = torch.empty(16 + int(nbytes) + GUARD, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.raw.fill_(CANARY)
        self.base, self.nbytes = base, int(nbytes)
        self.t = self.raw[base:]
        assert self.t.data_ptr() % 16 == base

    def check(self, want, tag, item=20):
        """The first len(want) bytes are `want`; every other byte of the allocation is untouched."""
        want = bytes(want)
        assert len(want) <= self.nbytes, tag
        got = self.t[: len(want)].cpu().numpy().tobytes()
        if got != want:
            a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
            k = int(np.nonzero(a != b)[0][0])
            lo = k // item * item
            raise AssertionError(f"{tag}: byte {k} (item {k // item} of {len(want) // item}): got {a[lo:lo + item].tolist()} want {b[lo:lo + item].tolist()}")
        assert bool((self.raw[: self.base] == CANARY).all().item()), f"{tag}: bytes in front of the buffer were written"
        rest = self.t[len(want):]
        if not bool((rest == CANARY).all().item()):
            k = int((rest != CANARY).nonzero()[0].item()) + len(want)
            raise AssertionError(f"{tag}: byte {k} was written: {len(want)} bytes are defined, the buffer holds {self.nbytes}")


def check_count(cnt, want, tag):
    got = int(cnt.t[:4].cpu().numpy().view(np.uint32)[0])
    assert got == want, f"{tag}: count {got} (0x{got:08x}), want {want}"
    cnt.check(np.uint32(want).tobytes(), tag + " [count word]", item=4)


def upload_at(ctx, arr, offset):
    """A device copy of arr that starts `offset` bytes past a 16-byte boundary."""
    import torch
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    raw = torch.zeros(len(a) + 32, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    t = raw[offset: offset + len(a)]
    t.copy_(torch.from_numpy(a))
    return t


def cheap_ids(n, dtype=np.uint8):
    """Ids for the large sizes (a seeded draw of 67 M values costs seconds): 0 .. 18 in a fixed rotation, so some are clamped."""
    return (np.arange(n, dtype=np.uint32) * 7 % 19).astype(dtype)


def expand_case(ctx, bits, S, ids, meshes, d_m, tag, d_ids=None, base=0, words=None):
    """vd_expand_mask_dev on pack_mask(bits, S) against expand_reference."""
    n = len(bits)
    words = mc.pack_mask(bits, S) if words is None else words
    want, wn = mc.expand_reference(words, n, S, ids, meshes)
    assert wn == int(np.asarray(bits).sum()), tag
    d_mask = ctx.upload(words)
    d_ids = ctx.upload(ids) if d_ids is None else d_ids
    out, cnt = Guarded(n * 20, base), Guarded(4)
    ctx.expand_mask_dev(d_mask, n, S, d_ids, d_m, len(meshes), out.t, cnt.t, id_bytes=ids.dtype.itemsize)
    check_count(cnt, wn, tag)
    out.check(want.tobytes(), tag)
    return wn


# ---- foreign-mask path: vd_expand_mask_dev, one shard ---------------------------------------------------------------

@pytest.mark.parametrize("n", SEAM_SIZES)
def test_expand_every_pattern_at_the_seam_sizes(ctx, n):
    """1-byte aligned ids, 16 meshes, one shard: mask_scan_kernel + expand_mask_u8_kernel<direct, no tile counts>.  Ids of 255
    (and 16, 17) are clamped to mesh 15."""
    meshes = mc.mesh_table(16)
    d_m = ctx.upload(meshes)
    ids = mc.mesh_ids(n, 16, seed=n, dtype=np.uint8)
    assert n < 64 or (ids == 255).any()
    for name, bits in mc.patterns(n, seed=n).items():
        expand_case(ctx, bits, n, ids, meshes, d_m, f"n={n} {name}")


@pytest.mark.parametrize("n_mesh", [1, 256, 257, 512, 513])
@pytest.mark.parametrize("id_bytes", [1, 2, 4])
def test_expand_id_widths_and_table_sizes(ctx, id_bytes, n_mesh):
    """id_bytes 1 with <= 256 meshes: expand_mask_u8_kernel<direct, no tile counts>; everything else expand_mask_kernel<IdT, TAB,
    no tile counts> with IdT by id_bytes and TAB = (n_mesh <= 512): all six of them.  The wider types carry ids above n_mesh."""
    meshes = mc.mesh_table(n_mesh, seed=id_bytes)
    d_m = ctx.upload(meshes)
    for n in (257, 8193, 24577):
        ids = mc.mesh_ids(n, n_mesh, seed=n + id_bytes, dtype=ID_TYPES[id_bytes])
        if n > 257 and (id_bytes > 1 or n_mesh < 256):
            assert (ids.astype(np.int64) >= n_mesh).any()
        for name, bits in mc.patterns(n, seed=n_mesh).items():
            expand_case(ctx, bits, n, ids, meshes, d_m, f"n={n} id_bytes={id_bytes} n_mesh={n_mesh} {name}")


# ---- the predicates of launch_expand's fast path, each flipped alone -------------------------------------------------

PREDICATE_N = 24577


def predicate_inputs():
    bits = mc.pattern("density_1_2", PREDICATE_N, seed=5)
    meshes = mc.mesh_table(16, seed=5)
    return bits, meshes, mc.mesh_ids(PREDICATE_N, 16, seed=5, dtype=np.uint8)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_predicate_id_table_alignment(ctx, offset):
    """d_mesh_ids 1, 2 and 3 bytes past a 16-byte boundary leaves the dword-fetching u8 kernel for expand_mask_kernel<u8, TAB,
    no tile counts>; offset 0 is the fast path on the same input."""
    bits, meshes, ids = predicate_inputs()
    d_ids = upload_at(ctx, ids, offset)
    assert d_ids.data_ptr() % 4 == offset
    expand_case(ctx, bits, PREDICATE_N, ids, meshes, ctx.upload(meshes), f"ids at +{offset}", d_ids=d_ids)


@pytest.mark.parametrize("shard_size", [
    8193, 8194, 8195,              # three shards, shard_size % 4 != 0: generic kernel
    8196,                          # three shards, % 4 == 0, short last shard: u8 kernel, groups of 4 words straddle shards
    64, 100, 192,                  # wps < 4 (1, 2, 3 words per shard): generic kernel
    256, 260,                      # wps == 4 and 5: the smallest shards of the u8 kernel
    PREDICATE_N + 1, 40000,        # shard_size > n_total: one shard with padding words behind the scene
    24000,                         # a short last shard of 577
])
def test_predicate_shard_shapes(ctx, shard_size):
    bits, meshes, ids = predicate_inputs()
    expand_case(ctx, bits, shard_size, ids, meshes, ctx.upload(meshes), f"shard_size={shard_size}")


def test_predicate_one_instance_per_shard(ctx):
    """shard_size = 1 at n = 130: 130 words with one valid bit each."""
    meshes = mc.mesh_table(16, seed=6)
    d_m = ctx.upload(meshes)
    for name, bits in mc.patterns(130, seed=6).items():
        expand_case(ctx, bits, 1, mc.mesh_ids(130, 16, seed=6, dtype=np.uint8), meshes, d_m, f"shard_size=1 {name}")


@pytest.mark.parametrize("base", BASES)
def test_expand_output_base(ctx, base):
    """d_out 0, 4, 8 and 12 bytes past a 16-byte boundary: the staged kernels store at the destination's 16-byte phase."""
    bits, meshes, ids = predicate_inputs()
    d_m = ctx.upload(meshes)
    expand_case(ctx, bits, PREDICATE_N, ids, meshes, d_m, f"u8 base={base}", base=base)
    wide = ids.astype(np.uint16)
    expand_case(ctx, bits, PREDICATE_N, wide, meshes, d_m, f"u16 base={base}", base=base)
    expand_case(ctx, mc.pattern("run_chunk_seam", PREDICATE_N), PREDICATE_N, wide, meshes, d_m, f"u16 run base={base}", base=base)


# ---- tile-count variants: vd_cull_compact_dev / vd_cull_compact_shard_dev / vd_cull_emit_shard_dev -------------------

def compact_case(ctx, cam, d_m, meshes, d_i, inst, bits, first, pad, tag, base=0):
    """first = None: vd_cull_compact_dev; else vd_cull_compact_shard_dev(first_instance = first)."""
    n = len(bits)
    want, wn = mc.expand_reference(mc.pack_mask(bits), n, n, inst["mesh"], meshes)
    want["base_instance"] = ((want["base_instance"].astype(np.int64) + (first or 0)) & 0xFFFFFFFF).astype(np.uint32)
    out, cnt = Guarded(n * 20, base), Guarded(4)
    if first is None:
        c = np.ascontiguousarray(cam, dtype=abi.CAMERA)
        ctx._chk(ctx.lib.vd_cull_compact_dev(ctx.h, c.ctypes.data, abi.ptr(d_m), len(meshes), abi.ptr(d_i), n, abi.ptr(out.t),
                                             abi.ptr(cnt.t), int(pad)))
    else:
        ctx.cull_compact_dev(cam, d_m, len(meshes), d_i, n, out.t, cnt.t, bool(pad), first)
    check_count(cnt, wn, tag)
    out.check(want.tobytes() + (bytes((n - wn) * 20) if pad else b""), tag)


def emit_case(ctx, cam, d_m, meshes, d_i, inst, bits, first, tag):
    n = len(bits)
    out = Guarded(n * 20)
    ctx.cull_emit_dev(cam, d_m, len(meshes), d_i, n, out.t, first)
    out.check(mc.emit_reference(bits, inst["mesh"], meshes, first).tobytes(), tag)


@pytest.mark.parametrize("form", ["fused", "two_launch"])
@pytest.mark.parametrize("n", [65, 2049, 8193, 24577])
def test_cull_compact_and_emit_on_pattern_scenes(ctx, ctx_options, n, form):
    """Scenes whose frustum cull gives the pattern (tests/test_mask_cases.py proves it on the oracle).  two_launch (forced with
    cull.split_min = 1): pass 1's tile counts place the chunks, expand_mask_u8_kernel<direct, tile counts>, and vd_cull_emit
    runs emit_all_u8_kernel; fused: cull_compact_kernel / emit_draws_kernel, the forms these sizes take by default."""
    if form == "two_launch":
        ctx_options("cull.split_min", 1)
    firsts = [None, 0, 100, 2**32 - n]
    for k, (name, bits) in enumerate(mc.patterns(n, seed=n + 1).items()):
        cam, meshes, inst = mc.instances_for_pattern(bits, 16, seed=k)
        d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
        for first in firsts:
            for pad in (0, 1):
                compact_case(ctx, cam, d_m, meshes, d_i, inst, bits, first, pad, f"{form} n={n} {name} first={first} pad={pad}")
        for first in firsts[1:]:
            emit_case(ctx, cam, d_m, meshes, d_i, inst, bits, first, f"{form} emit n={n} {name} first={first}")


@pytest.mark.parametrize("n_mesh", [300, 600, 66_000])
def test_cull_compact_tile_counts_with_wider_ids(ctx, ctx_options, n_mesh):
    """Pass 1 picks the id width by n_mesh: 2 bytes up to 65536 meshes (LDS table up to 512: expand_mask_kernel<u16, TAB, tile
    counts> at 300, <u16, no TAB, tile counts> at 600), 4 bytes beyond (<u32, no TAB, tile counts>)."""
    ctx_options("cull.split_min", 1)
    n = 24577
    for k, name in enumerate(["density_1_2", "chunks_alternating", "run_chunk_seam", "bit_last", "one"]):
        bits = mc.pattern(name, n, seed=n_mesh)
        cam, meshes, inst = mc.instances_for_pattern(bits, n_mesh, seed=k)
        d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
        for first, pad in ((None, 0), (100, 1)):
            compact_case(ctx, cam, d_m, meshes, d_i, inst, bits, first, pad, f"n_mesh={n_mesh} {name} first={first} pad={pad}")
        emit_case(ctx, cam, d_m, meshes, d_i, inst, bits, 100, f"emit n_mesh={n_mesh} {name}")


@pytest.mark.parametrize("n", [abi.CULL_SPLIT_MIN - 1, abi.CULL_SPLIT_MIN])
def test_cull_compact_on_each_side_of_the_library_s_switch(ctx, n):
    """Default options: the fused form one instance below VdCtx::split_min (abi.CULL_SPLIT_MIN), the two-launch form from it on."""
    import torch
    bits = mc.pattern("chunks_alternating", n)
    bits[n - 1] = 1
    cam, meshes, inst = mc.instances_for_pattern(bits, 16, seed=3)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    compact_case(ctx, cam, d_m, meshes, d_i, inst, bits, None, 0, f"n={n}")
    compact_case(ctx, cam, d_m, meshes, d_i, inst, bits, 2**32 - n, 1, f"n={n} shard, padded")
    del d_i
    torch.cuda.empty_cache()


# ---- pad_tail_kernel: head dwords, 16-byte body, tail dwords in all residues ------------------------------------------

@pytest.mark.parametrize("form", ["fused", "two_launch"])
@pytest.mark.parametrize("base", BASES)
def test_pad_tail_alignment(ctx, ctx_options, base, form):
    """The tail starts at d_out + 20 * count: counts 0 .. 5 walk its first byte through every 16-byte residue for each base;
    n - 3, n - 1 and n leave a tail of 15 dwords (no 16-byte body to speak of), 5 dwords, and none."""
    if form == "two_launch":
        ctx_options("cull.split_min", 1)
    n = 1031
    for count in (0, 1, 2, 3, 4, 5, n - 3, n - 1, n):
        bits = mc.with_count(n, count)
        cam, meshes, inst = mc.instances_for_pattern(bits, 16, seed=count)
        compact_case(ctx, cam, ctx.upload(meshes), meshes, ctx.upload(inst), inst, bits, 0, 1, f"{form} base={base} count={count}", base=base)


# ---- mask_scan_kernel's regimes, the LDS-staged u8 kernel ------------------------------------------------------------

def scan_sizes():
    return {"range_2": mc.CHUNK * 1025 + 1,                        # > 1024 chunks: two entries per thread of the scanning workgroup
            "grid_stride": mc.CHUNK * (32 * cu_count() + 1) + 77,  # one chunk more than the scan's grid holds: its grid-stride loop
            "staged": (12 << 20) + 8193}                           # > 12 Mi instances: expand_mask_u8_kernel<staged, ...>


def scan_masks(n):
    yield "density_1_1000", mc.pattern("density_1_1000", n, seed=9)
    yield "bit_last", mc.pattern("bit_last", n)
    yield "ends_full", mc.ends_full(n)


@pytest.mark.parametrize("size", ["range_2", "grid_stride", "staged"])
def test_scan_regimes_on_sparse_masks(ctx, size):
    """vd_mask_to_indices_dev and vd_expand_mask_dev (1-byte aligned ids: expand_mask_u8_kernel<direct, no tile counts> up to
    12 Mi instances, <staged, no tile counts> above)."""
    import torch
    n = scan_sizes()[size]
    meshes = mc.mesh_table(16, seed=7)
    d_m = ctx.upload(meshes)
    ids = cheap_ids(n)
    d_ids = ctx.upload(ids)
    for name, bits in scan_masks(n):
        words = mc.pack_mask(bits)
        wn = expand_case(ctx, bits, n, ids, meshes, d_m, f"{size} n={n} {name} expand", d_ids=d_ids, words=words)
        want = mc.indices_reference(words, n, 7)
        out, cnt = Guarded(n * 4), Guarded(4)
        ctx.mask_to_indices_dev(ctx.upload(words), n, 7, out.t, cnt.t)
        check_count(cnt, wn, f"{size} {name} indices")
        out.check(want.tobytes(), f"{size} n={n} {name} indices", item=4)
        del out
    torch.cuda.empty_cache()


def test_staged_expansion_from_tile_counts(ctx):
    """vd_cull_compact_dev above 12 Mi instances: expand_mask_u8_kernel<staged, tile counts>.  One case (1.8 GB of instances)."""
    import torch
    n = (12 << 20) + 8193
    bits = mc.pattern("density_1_1000", n, seed=11)
    cam, meshes, inst = mc.instances_for_pattern(bits, 16, seed=11)
    d_m, d_i = ctx.upload(meshes), ctx.upload(inst)
    compact_case(ctx, cam, d_m, meshes, d_i, inst, bits, None, 0, f"staged, tile counts n={n}")
    del d_i, inst
    torch.cuda.empty_cache()


# ---- indices wire format ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SEAM_SIZES)
def test_mask_to_indices_every_pattern_at_the_seam_sizes(ctx, n):
    for name, bits in mc.patterns(n, seed=n + 2).items():
        words = mc.pack_mask(bits)
        d_mask = ctx.upload(words)
        for first in (0, 100, 4097, 2**32 - n):
            want = mc.indices_reference(words, n, first)
            out, cnt = Guarded(n * 4), Guarded(4)
            ctx.mask_to_indices_dev(d_mask, n, first, out.t, cnt.t)
            check_count(cnt, len(want), f"n={n} {name} first={first}")
            out.check(want.tobytes(), f"n={n} {name} first={first}", item=4)


def index_lists(n_indices, n_total, seed):
    rng = np.random.default_rng([0x1D1C, seed, n_indices])
    asc = np.sort(rng.choice(n_total, n_indices, replace=False)).astype(np.uint32)
    yield "ascending", asc
    yield "shuffled", rng.permutation(asc)
    rep = rng.integers(0, n_total, n_indices).astype(np.uint32)
    rep[n_indices // 2:] = rep[: n_indices - n_indices // 2]       # the second half repeats the first
    rep[-1] = n_total - 1
    yield "repeats", rep


@pytest.mark.parametrize("n_mesh", [1, 512, 513])
@pytest.mark.parametrize("id_bytes", [1, 2, 4])
def test_indices_to_draws(ctx, id_bytes, n_mesh):
    """indices_to_draws_kernel<IdT>: both sides of its LDS table (kTab = 512), one block .. the grid-stride loop (more than
    16 x CUs x 256 indices), sorted, shuffled and repeating lists, every output phase.  Only indices below n_total."""
    meshes = mc.mesh_table(n_mesh, seed=20 + id_bytes)
    d_m = ctx.upload(meshes)
    big = 16 * cu_count() * 256 + 257
    for n_indices in (1, 255, 256, 257, big):
        n_total = n_indices + 1000
        ids = mc.mesh_ids(n_total, n_mesh, seed=n_indices, dtype=ID_TYPES[id_bytes])
        d_ids = ctx.upload(ids)
        for k, (name, lst) in enumerate(index_lists(n_indices, n_total, seed=n_mesh)):
            want = mc.draws_from_indices_reference(lst, ids, meshes).tobytes()
            d_lst = ctx.upload(lst)
            for base in (BASES if n_indices != big else [BASES[(k + id_bytes) % 4]]):
                out = Guarded(n_indices * 20, base)
                ctx.indices_to_draws_dev(d_lst, n_indices, d_ids, n_total, d_m, n_mesh, out.t, id_bytes=id_bytes)
                out.check(want, f"n_indices={n_indices} id_bytes={id_bytes} n_mesh={n_mesh} {name} base={base}")


@pytest.mark.parametrize("id_bytes", [1, 2])
def test_indices_round_trip_over_three_shards(ctx, id_bytes):
    """mask_to_indices per shard, concatenated, then indices_to_draws == expand_mask over the three shard masks (short last
    shard; shard_size % 4 == 0 and >= 4 words, so 1-byte ids stay on the u8 kernel across the shard seams)."""
    n, S = 24577, 8200
    meshes = mc.mesh_table(40, seed=30)
    d_m = ctx.upload(meshes)
    ids = mc.mesh_ids(n, 40, seed=30, dtype=ID_TYPES[id_bytes])
    d_ids = ctx.upload(ids)
    wps = mc.words_per_shard(S)
    for name, bits in mc.patterns(n, seed=31).items():
        words = mc.pack_mask(bits, S)
        want, wn = mc.expand_reference(words, n, S, ids, meshes)
        expand_case(ctx, bits, S, ids, meshes, d_m, f"round trip {name} expand", d_ids=d_ids)
        lst = Guarded(n * 4)
        done = 0
        for r in range(3):
            n_r = min(S, n - r * S)
            cnt = Guarded(4)
            ctx.mask_to_indices_dev(ctx.upload(words[r * wps: (r + 1) * wps]), n_r, r * S, lst.t[done * 4:], cnt.t)
            c = int(bits[r * S: r * S + n_r].sum())
            check_count(cnt, c, f"round trip {name} shard {r}")
            done += c
        assert done == wn
        lst.check(want["base_instance"].tobytes(), f"round trip {name} indices", item=4)
        out = Guarded(n * 20)
        if wn:
            ctx.indices_to_draws_dev(lst.t, wn, d_ids, n, d_m, len(meshes), out.t, id_bytes=id_bytes)
        out.check(want.tobytes(), f"round trip {name} draws")


# ---- C3 alone ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SEAM_SIZES)
def test_compact_draws_every_pattern_at_the_seam_sizes(ctx, oracle, n):
    meshes = mc.mesh_table(16, seed=40)
    ids = mc.mesh_ids(n, 16, seed=40)
    for name, bits in mc.patterns(n, seed=n + 3).items():
        emit = mc.emit_reference(bits, ids, meshes, first_instance=12345)
        want, wn = oracle.compact(emit)
        assert wn == int(bits.sum())
        out, cnt = Guarded(n * 20), Guarded(4)
        ctx.compact_draws_dev(ctx.upload(emit), n, out.t, cnt.t)
        check_count(cnt, wn, f"n={n} {name}")
        out.check(want[:wn].tobytes(), f"n={n} {name}")


# ---- state carried between launches -------------------------------------------------------------------------------------

def test_launches_back_to_back_on_a_fresh_context():
    """expand_mask at 24577 -> 65 -> 8192 * 1025 + 1 -> 8193 -> 24577 instances and mask_to_indices on the last mask, enqueued
    without a synchronize in between and read back at the end: the ScanState epoch advances per launch and the entries of
    earlier, larger launches stay behind.  expand_state starts at 64 KiB (8190 chunks), so two more steps follow: the size of
    the scan's grid-stride regime, whose chunk count outgrows it on a part with 256 CUs (the state is reallocated and its
    epoch restarted), and 24577 once more on the new state."""
    import torch
    from voidin_amd.runtime import Context
    own = Context(0)
    try:
        meshes = mc.mesh_table(16, seed=50)
        d_m = own.upload(meshes)
        steps = [(24577, "density_1_2"), (65, "bit_63_of_words"), (mc.CHUNK * 1025 + 1, "density_1_1000"), (8193, "chunks_alternating"),
                 (24577, "density_999_1000"), (scan_sizes()["grid_stride"], "density_1_1000"), (24577, "words_alternating")]
        jobs = []
        for k, (n, name) in enumerate(steps):
            bits = mc.pattern(name, n, seed=50 + k)
            ids = cheap_ids(n)
            words = mc.pack_mask(bits)
            jobs.append((n, name, words, ids, own.upload(words), own.upload(ids), Guarded(n * 20), Guarded(4)))
        idx_out, idx_cnt = Guarded(24577 * 4), Guarded(4)
        torch.cuda.synchronize()
        for n, name, words, ids, d_mask, d_ids, out, cnt in jobs:
            own.expand_mask_dev(d_mask, n, n, d_ids, d_m, 16, out.t, cnt.t, id_bytes=1)
        own.mask_to_indices_dev(jobs[-1][4], 24577, 3, idx_out.t, idx_cnt.t)
        torch.cuda.synchronize()
        for n, name, words, ids, d_mask, d_ids, out, cnt in jobs:
            want, wn = mc.expand_reference(words, n, n, ids, meshes)
            check_count(cnt, wn, f"sequence n={n} {name}")
            out.check(want.tobytes(), f"sequence n={n} {name}")
        want = mc.indices_reference(jobs[-1][2], 24577, 3)
        check_count(idx_cnt, len(want), "sequence indices")
        idx_out.check(want.tobytes(), "sequence indices", item=4)
    finally:
        own.close()
    torch.cuda.empty_cache()
