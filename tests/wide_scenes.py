"""Helpers of the wide-top-level tests (tests/test_gpu_trace_wide.py, tests/test_gpu_tlas_lbvh.py): a helper module, no tests in it.
Narrow TLAS nodes rewritten as VdTlasNodeWide, node arrays relocated through a seeded injective map, and scenes of pairwise
disjoint instances (where a ray's record cannot depend on the shape of the top level)."""
import numpy as np

from voidin_amd import abi, synth

SLOTS = 200_000          # relocated arrays: indices pass 16 bits


def widen(tl):
    """The same nodes as VdTlasNodeWide: left = left_right & 0xffff, right = left_right >> 16."""
    tl = np.asarray(tl, dtype=abi.TLAS_NODE)
    w = np.zeros(len(tl), dtype=abi.TLAS_NODE_WIDE)
    w["min"], w["max"], w["instance_idx"] = tl["min"], tl["max"], tl["instance_idx"]
    w["left"], w["right"] = tl["left_right"] & np.uint32(0xffff), tl["left_right"] >> np.uint32(16)
    return w


def relocate(wide, seed, n_slots=SLOTS):
    """(array of n_slots wide nodes, pos): node k of `wide` sits at pos[k]; the root stays at 0, the others are scattered by a
    seeded injective map, child ids follow, every unused slot is 0xff bytes.  The topology is unchanged."""
    n = len(wide)
    assert n <= n_slots
    rng = np.random.default_rng(seed)
    pos = np.zeros(n, dtype=np.uint32)
    pos[1:] = 1 + rng.choice(n_slots - 1, size=n - 1, replace=False).astype(np.uint32)
    assert len(set(pos.tolist())) == n and pos.max() > 0xffff
    moved = wide.copy()
    interior = (wide["left"] != 0) | (wide["right"] != 0)
    moved["left"][interior], moved["right"][interior] = pos[wide["left"][interior]], pos[wide["right"][interior]]
    out = np.frombuffer(b"\xff" * (n_slots * abi.TLAS_NODE_WIDE.itemsize), dtype=abi.TLAS_NODE_WIDE).copy()
    out[pos] = moved
    return out, pos


def reachable(wide):
    """bool per slot: reached from node 0 (children are followed only while they are inside the array)."""
    seen = np.zeros(len(wide), dtype=bool)
    todo = [0]
    while todo:
        k = todo.pop()
        if seen[k]:
            continue
        seen[k] = True
        l, r = int(wide["left"][k]), int(wide["right"][k])
        if l or r:
            todo += [c for c in (l, r) if c < len(wide)]
    return seen


def mesh_set(oracle, sources):
    """(infos, bvh_nodes, vertices, indices) of the meshes `sources` = [(vertices, indices), ...], BLAS by the oracle."""
    V, I, B = [], [], []
    infos = np.zeros(len(sources), dtype=abi.MESH_INFO)
    vo = bo = no = 0
    for k, (v, i) in enumerate(sources):
        v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
        nodes, idx = oracle.bvh_build(v, i)
        infos[k]["min"], infos[k]["max"] = synth.mesh_bounds(v)
        infos[k]["index_count"], infos[k]["base_index"], infos[k]["vertex_offset"], infos[k]["bvh_index"] = len(idx), bo, vo, no
        V.append(v); I.append(idx); B.append(nodes)
        vo += len(v); bo += len(idx); no += len(nodes)
    return infos, np.concatenate(B), np.concatenate(V), np.concatenate(I).astype(np.uint32)


def disjoint_instances(n, seed):
    """n instances of ONE unit-radius mesh, pairwise disjoint: centres on a cubic grid of spacing 1 jittered by less than 0.05,
    scale in [0.25, 0.44] (scaled radius < 0.45: two spheres are at least 1 - 0.1 - 0.9 > 0 apart - no two instances can tie),
    rotated about z.  Grid cells are handed out in a seeded random order, so instance order says nothing about position."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    cells = rng.permutation(side ** 3)[:n]
    c = np.stack([cells % side, (cells // side) % side, cells // (side * side)], axis=1).astype(np.float64)
    c += (rng.random((n, 3)) - 0.5) * 0.09
    s = 0.25 + 0.19 * rng.random(n)
    a = rng.random(n) * 2 * np.pi
    T = np.zeros((n, 4, 4))                                 # [column][row]: column-major storage
    T[:, 0, 0], T[:, 0, 1] = s * np.cos(a), s * np.sin(a)
    T[:, 1, 0], T[:, 1, 1] = -s * np.sin(a), s * np.cos(a)
    T[:, 2, 2], T[:, 3, 3] = s, 1.0
    T[:, 3, :3] = c
    M = np.transpose(T, (0, 2, 1))                          # [row][column]
    Mi = np.linalg.inv(M)
    inst = np.zeros(n, dtype=abi.INSTANCE)
    inst["transform"] = T.reshape(n, 16).astype(np.float32)
    inst["inv_transform"] = np.transpose(Mi, (0, 2, 1)).reshape(n, 16).astype(np.float32)
    return inst, side


def grid_rays(n, side, seed):
    """Seeded rays through a grid of `side`^3 cells: from points on a sphere around it towards points inside it."""
    rng = np.random.default_rng(seed)
    mid = (side - 1) / 2.0
    o = rng.normal(size=(n, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * (side * 1.2 + 2.0) + mid
    t = rng.random((n, 3)) * (side - 1)
    d = t - o
    rays = np.zeros(n, dtype=abi.RAY)
    rays["eye"], rays["dir"] = o, d / np.linalg.norm(d, axis=1, keepdims=True)
    return rays


def records_equal(got, want):
    """All four fields of every record, bit for bit."""
    a = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4)
    b = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 4)
    return a.shape == b.shape and bool((a == b).all())


def first_bad(got, want):
    a = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4)
    b = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 4)
    bad = np.nonzero((a != b).any(axis=1))[0]
    return (len(bad), int(bad[0]), got[bad[0]], want[bad[0]]) if len(bad) else None
