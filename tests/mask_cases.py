"""Hand-made visibility masks and plain references for the mask -> draw-list expansion (tests/test_mask_cases.py,
tests/test_gpu_mask_patterns.py).

The expansion is a pure function of (mask, mesh ids, mesh table): a set bit i gives the 20-byte command
{index_count, 1, base_index, vertex_offset of meshes[min(id[i], n_mesh - 1)], base_instance = i}, in ascending i.  The
references below state that in a few lines of numpy on integers and bytes; every comparison against them is bit for bit.

The seams the patterns are tied to are those of voidin_amd/csrc/cull.hip: a mask word (64 instances), a group of four
words that is staged and stored as one run (256), the 32 words of a wave (2048) and the 128 words of a workgroup's chunk
(8192)."""
import numpy as np

from voidin_amd import abi, synth

WORD, GROUP, WAVE, CHUNK = 64, 256, 2048, 8192

DENSITIES = {"density_1_1000": (1, 1000), "density_1_2": (1, 2), "density_999_1000": (999, 1000)}
RUNS = {"run_chunk_seam": (CHUNK - 2, CHUNK + 3), "run_wave_seam": (WAVE - 2, WAVE + 3), "run_group_seam": (GROUP - 2, GROUP + 3)}
NAMES = ["zero", "one", "bit_0", "bit_last", "bit_63_of_words", "bit_0_of_words", "words_alternating", "chunks_alternating",
         *RUNS, *DENSITIES]


def exists(name, n):
    """Whether pattern `name` can be built at length n without clamping it: a pattern that needs a seam n does not reach
    is left out."""
    if name in RUNS:
        return n >= RUNS[name][1]
    return n >= {"bit_63_of_words": WORD, "words_alternating": WORD + 1, "chunks_alternating": CHUNK + 1}.get(name, 1)


def pattern(name, n, seed=0):
    """One named pattern: n bits as a uint8 array of 0 / 1."""
    assert exists(name, n), (name, n)
    bits = np.zeros(n, dtype=np.uint8)
    i = np.arange(n, dtype=np.int64) if name.endswith(("_of_words", "alternating")) else None
    if name == "one":
        bits[:] = 1
    elif name == "bit_0":
        bits[0] = 1
    elif name == "bit_last":
        bits[n - 1] = 1
    elif name == "bit_63_of_words":
        bits[i % WORD == WORD - 1] = 1
    elif name == "bit_0_of_words":
        bits[i % WORD == 0] = 1
    elif name == "words_alternating":
        bits[(i // WORD) % 2 == 0] = 1
    elif name == "chunks_alternating":
        bits[(i // CHUNK) % 2 == 0] = 1
    elif name in RUNS:
        bits[RUNS[name][0]:RUNS[name][1]] = 1
    elif name in DENSITIES:
        num, den = DENSITIES[name]
        rng = np.random.default_rng([0x9A77, seed, num, den])
        bits[rng.integers(0, den, n) < num] = 1
    elif name != "zero":
        raise KeyError(name)
    return bits


def patterns(n, seed=0):
    """{name: bits} of every pattern that exists at length n."""
    return {name: pattern(name, n, seed) for name in NAMES if exists(name, n)}


def ends_full(n):
    """First and last chunk full, everything between empty: two runs of survivors with a long stretch of empty chunks in
    between (the scan's per-thread ranges and its grid-stride loop see nothing but zeros there)."""
    assert n > 2 * CHUNK
    bits = np.zeros(n, dtype=np.uint8)
    bits[:CHUNK] = 1
    bits[(n - 1) // CHUNK * CHUNK:] = 1
    return bits


def with_count(n, count):
    """`count` survivors among n, hand-placed: the first count - 1 instances and the last one (count == n: all)."""
    bits = np.zeros(n, dtype=np.uint8)
    if count > 0:
        bits[:count - 1] = 1
        bits[n - 1] = 1
    assert int(bits.sum()) == count
    return bits


def words_per_shard(shard_size):
    return (shard_size + WORD - 1) // WORD


def pack_mask(bits, shard_size=None):
    """The mask words of `bits` as the expansion reads them: shard r owns words [r * wps, (r + 1) * wps) and holds the
    instances [r * shard_size, (r + 1) * shard_size); padding bits are 0."""
    n = len(bits)
    S = n if shard_size is None else int(shard_size)
    wps, n_shards = words_per_shard(S), (n + S - 1) // S
    rows = np.zeros((n_shards, wps * WORD), dtype=np.uint8)
    flat = np.zeros(n_shards * S, dtype=np.uint8)
    flat[:n] = bits
    rows[:, :S] = flat.reshape(n_shards, S)
    return np.packbits(rows, axis=1, bitorder="little").reshape(-1).view("<u8").copy()


def mask_bits(mask_words, n_total, shard_size):
    """Inverse of pack_mask: the n_total bits the shards cover."""
    words = np.ascontiguousarray(mask_words, dtype="<u8")
    wps, n_shards = words_per_shard(shard_size), (n_total + shard_size - 1) // shard_size
    rows = np.unpackbits(words[: n_shards * wps].view(np.uint8), bitorder="little").reshape(n_shards, wps * WORD)
    return np.ascontiguousarray(rows[:, :shard_size]).reshape(-1)[:n_total]


def commands(index, ids, meshes, instance_count=1):
    """The command of every listed instance: mesh fields through the clamped id, base_instance = the index as given."""
    index = np.asarray(index)
    mid = np.minimum(np.asarray(ids)[index.astype(np.int64)].astype(np.int64), len(meshes) - 1)
    out = np.zeros(len(index), dtype=abi.DRAW)
    out["vertex_count"] = meshes["index_count"][mid]
    out["instance_count"] = instance_count
    out["base_index"] = meshes["base_index"][mid]
    out["vertex_offset"] = meshes["vertex_offset"][mid]
    out["base_instance"] = index.astype(np.uint32)
    return out


def expand_reference(mask_words, n_total, shard_size, ids, meshes):
    """(draws, count): one command per set bit, ascending instance index."""
    i = np.nonzero(mask_bits(mask_words, n_total, shard_size))[0]
    return commands(i, ids, meshes), len(i)


def indices_reference(mask_words, n_inst, first_instance):
    """Ascending first_instance + i of the set bits, in uint32 arithmetic."""
    i = np.nonzero(mask_bits(mask_words, n_inst, n_inst))[0]
    return ((i + int(first_instance)) & 0xFFFFFFFF).astype(np.uint32)


def draws_from_indices_reference(indices, ids, meshes):
    """The command of every listed index (unsorted, repeated: as listed), instance_count = 1."""
    return commands(np.asarray(indices, dtype=np.uint32), ids, meshes)


def emit_reference(bits, ids, meshes, first_instance=0):
    """Every slot written: instance_count = the bit, base_instance = first_instance + i (uint32)."""
    n = len(bits)
    out = commands(np.arange(n), ids, meshes, instance_count=np.asarray(bits, dtype=np.uint32))
    out["base_instance"] = ((np.arange(n, dtype=np.int64) + int(first_instance)) & 0xFFFFFFFF).astype(np.uint32)
    return out


def mesh_table(n_mesh, seed=0):
    """n_mesh MeshInfo records whose command fields are unrelated 32-bit values (a wrong row, or a field taken from a
    neighbouring row, shows) and whose boxes (half extent 0.25 .. 1) are centred near (0, 0, BOX_Z) in object space: see
    instances_for_pattern."""
    rng = np.random.default_rng([0x7AB1E, seed, n_mesh])
    m = np.zeros(n_mesh, dtype=abi.MESH_INFO)
    half = rng.uniform(0.25, 1.0, (n_mesh, 3))
    ctr = rng.uniform(-0.5, 0.5, (n_mesh, 3)) + np.array([0.0, 0.0, BOX_Z])
    m["min"], m["max"] = (ctr - half).astype(np.float32), (ctr + half).astype(np.float32)
    m["index_count"] = rng.integers(1, 1 << 32, n_mesh, dtype=np.uint64).astype(np.uint32)
    m["base_index"] = rng.integers(0, 1 << 32, n_mesh, dtype=np.uint64).astype(np.uint32)
    m["vertex_offset"] = rng.integers(-(1 << 31), 1 << 31, n_mesh, dtype=np.int64).astype(np.int32)
    m["bvh_index"] = np.arange(n_mesh, dtype=np.uint32)
    return m


def mesh_ids(n, n_mesh, seed=0, dtype=np.uint32):
    """Seeded mesh ids, about one in eight at or above n_mesh (the kernels clamp those to the last mesh): n_mesh itself,
    the largest value of the type, and - for one-byte ids - 255."""
    rng = np.random.default_rng([0x1D5, seed, n, n_mesh])
    top = int(np.iinfo(dtype).max)
    ids = rng.integers(0, min(n_mesh, top + 1), n, dtype=np.int64)
    over = np.array([min(n_mesh, top), top, min(255, top), min(n_mesh + 1, top)], dtype=np.int64)
    pick = rng.integers(0, 32, n)
    ids = np.where(pick < 4, over[pick & 3], ids)
    return ids.astype(dtype)


BOX_Z = 60.0        # view-space depth of the two clusters, and the object-space z of the mesh boxes


def instances_for_pattern(bits, n_mesh, seed=0):
    """(camera, meshes, instances) whose frustum cull keeps exactly the instances with bits[i] == 1.

    Unit scale, no rotation, seeded mesh ids (some out of range) and a seeded offset of up to 5 units per axis.  The
    visibility test measures its radius from the OBJECT-space box corners to the VIEW-space centre (emit_draws.wgsl, kept
    bug for bug), so at unit scale an instance behind the camera is dropped only if its box lies near its view-space
    centre: the boxes of mesh_table sit at object-space z = +BOX_Z.
      dropped: view-space centre (x, y, +BOX_Z + z), BEHIND the camera: radius < 11, and
               c.z * frustum[1] - |c.x| * frustum[0] < -42, so the first side plane rejects it;
      kept:    view-space centre (x, y, -BOX_Z + z), on the axis in FRONT: both side-plane terms are > 35, the radius is
               positive, and the far plane of synth.camera_uniform() is at infinity."""
    bits = np.asarray(bits)
    n = len(bits)
    cam = synth.camera_uniform()
    meshes = mesh_table(n_mesh, seed)
    ids = mesh_ids(n, n_mesh, seed)
    rng = np.random.default_rng([0x5CE9E, seed, n])
    c = rng.uniform(-5.0, 5.0, (n, 3))
    c[:, 2] += np.where(bits != 0, -BOX_Z, BOX_Z)
    # world position of the mesh centre = V^-1 * c; the translation puts the (clamped) mesh's box centre there
    V = cam["view"].reshape(4, 4).astype(np.float64).T
    Vinv = np.linalg.inv(V)
    world = c @ Vinv[:3, :3].T + Vinv[:3, 3]
    mid = np.minimum(ids.astype(np.int64), n_mesh - 1)
    centre = (meshes["max"].astype(np.float64) + meshes["min"].astype(np.float64)) / 2.0
    t = np.zeros((n, 16), dtype=np.float32)
    t[:, [0, 5, 10, 15]] = 1.0
    t[:, 12:15] = world - centre[mid]
    inst = np.zeros(n, dtype=abi.INSTANCE)
    inst["transform"] = t
    inst["mesh"] = ids
    inst["material"] = 1
    return cam, meshes, inst
