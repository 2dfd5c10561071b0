"""The hand-made masks and numpy references of tests/mask_cases.py check themselves against the CPU oracle: without this
the GPU tests that use them (tests/test_gpu_mask_patterns.py) could pass vacuously."""
import numpy as np
import pytest

import mask_cases as mc

SIZES = [1, 65, 8193, 20000]


@pytest.mark.parametrize("n", SIZES)
def test_pattern_scenes_reproduce_their_pattern_through_the_oracle(oracle, n):
    """oracle.cull_emit keeps exactly the instances whose bit is set, and the plain expansion of that mask is the oracle's
    compacted list."""
    pats = mc.patterns(n, seed=n)
    assert {"zero", "one", "bit_0", "bit_last", "density_1_2"} <= set(pats)
    for k, (name, bits) in enumerate(pats.items()):
        assert len(bits) == n and bits.dtype == np.uint8 and bits.max(initial=0) <= 1
        cam, meshes, inst = mc.instances_for_pattern(bits, n_mesh=16, seed=k)
        emit = oracle.cull_emit(cam, meshes, inst)
        assert emit["instance_count"].astype(np.uint8).tobytes() == bits.tobytes(), name
        assert emit.tobytes() == mc.emit_reference(bits, inst["mesh"], meshes).tobytes(), name
        want, wn = oracle.compact(emit)
        got, cnt = mc.expand_reference(mc.pack_mask(bits), n, n, inst["mesh"], meshes)
        assert cnt == wn == int(bits.sum()), name
        assert got.tobytes() == want[:wn].tobytes(), name


def test_patterns_that_do_not_exist_are_left_out():
    assert "run_chunk_seam" not in mc.patterns(8193) and "run_chunk_seam" in mc.patterns(8195)
    assert "chunks_alternating" not in mc.patterns(8192) and "chunks_alternating" in mc.patterns(8193)
    assert "bit_63_of_words" not in mc.patterns(63) and "words_alternating" not in mc.patterns(64)
    assert set(mc.patterns(24577)) == set(mc.NAMES)
    p = mc.patterns(24577)
    assert p["run_chunk_seam"].nonzero()[0].tolist() == [8190, 8191, 8192, 8193, 8194]
    assert p["run_wave_seam"].nonzero()[0].tolist() == [2046, 2047, 2048, 2049, 2050]
    assert p["run_group_seam"].nonzero()[0].tolist() == [254, 255, 256, 257, 258]
    assert p["bit_63_of_words"].nonzero()[0][-1] == 24575 and p["bit_last"].nonzero()[0].tolist() == [24576]
    assert p["chunks_alternating"][:8192].all() and not p["chunks_alternating"][8192:16384].any()
    assert p["chunks_alternating"][16384:24576].all() and p["chunks_alternating"][24576] == 0     # a fourth chunk of one instance
    for name, (num, den) in mc.DENSITIES.items():
        assert abs(int(p[name].sum()) - 24577 * num // den) < 400, name


@pytest.mark.parametrize("n", SIZES)
def test_padding_bits_are_zero_and_packing_round_trips(n):
    for name, bits in mc.patterns(n).items():
        for S in {n, 1, 64, 100, max(n // 3, 1) + 1, n + 37}:
            if S == 1 and n > 200:
                continue
            words = mc.pack_mask(bits, S)
            wps = mc.words_per_shard(S)
            assert len(words) == (n + S - 1) // S * wps
            assert int(np.unpackbits(words.view(np.uint8)).sum()) == int(bits.sum()), (name, S)     # nothing outside the shards' ranges
            assert mc.mask_bits(words, n, S).tobytes() == bits.tobytes(), (name, S)


@pytest.mark.parametrize("n", [65, 8193, 20000])
def test_sharded_reference_equals_the_one_shard_reference(n):
    """1, 3 and 5 shards, among them a shard size that is no multiple of 64 and a short last shard."""
    meshes = mc.mesh_table(16)
    ids = mc.mesh_ids(n, 16, dtype=np.uint8)
    for name, bits in mc.patterns(n).items():
        one, cnt = mc.expand_reference(mc.pack_mask(bits), n, n, ids, meshes)
        for shards in (1, 3, 5):
            S = n if shards == 1 else -(-n // shards) + 1  # one past the even split: the last shard is short
            if shards == 5 and n > 1000:
                S = (S + 63) // 64 * 64                    # whole words per shard
            assert (n + S - 1) // S == shards and (shards == 1 or n % S != 0)
            assert shards != 3 or S % 64 != 0
            got, c = mc.expand_reference(mc.pack_mask(bits, S), n, S, ids, meshes)
            assert c == cnt and got.tobytes() == one.tobytes(), (name, shards)


@pytest.mark.parametrize("n", SIZES)
def test_indices_wire_format_reference_equals_the_expansion(n):
    meshes = mc.mesh_table(513)
    ids = mc.mesh_ids(n, 513, dtype=np.uint16)
    for name, bits in mc.patterns(n).items():
        words = mc.pack_mask(bits)
        want, cnt = mc.expand_reference(words, n, n, ids, meshes)
        idx = mc.indices_reference(words, n, 0)
        assert idx.dtype == np.uint32 and len(idx) == cnt
        assert mc.draws_from_indices_reference(idx, ids, meshes).tobytes() == want.tobytes(), name
        off = mc.indices_reference(words, n, 2**32 - n)    # uint32 arithmetic: the last instance is 0xffffffff
        assert ((off.astype(np.int64) - (2**32 - n)) == idx).all() and (cnt == 0 or off.max() <= 0xFFFFFFFF)
    # unsorted and repeated lists are taken as they come
    lst = np.array([n - 1, 0, n - 1, n // 2], dtype=np.uint32)
    d = mc.draws_from_indices_reference(lst, ids, meshes)
    assert d["base_instance"].tolist() == lst.tolist() and (d["instance_count"] == 1).all()
    assert (d["vertex_count"] == meshes["index_count"][np.minimum(ids[lst].astype(np.int64), 512)]).all()


def test_out_of_range_ids_are_present_and_clamp_to_the_last_mesh():
    meshes = mc.mesh_table(16)
    for dtype in (np.uint8, np.uint16, np.uint32):
        ids = mc.mesh_ids(4096, 16, dtype=dtype)
        assert (ids == 255).any() and (ids == 16).any() and (ids == np.iinfo(dtype).max).any() and (ids < 16).sum() > 3000
        d = mc.commands(np.arange(4096), ids, meshes)
        assert (d["base_index"][ids >= 16] == meshes["base_index"][15]).all()
    ids = mc.mesh_ids(4096, 513, dtype=np.uint8)            # one-byte ids under a larger table: never clamped, all below 256
    assert ids.max() == 255
    assert len(set(meshes["index_count"].tolist())) == 16 and len(set(meshes["vertex_offset"].tolist())) == 16
