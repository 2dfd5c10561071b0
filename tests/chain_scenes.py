"""Hand-made trace scenes whose stack depth is set by a length: chains.  Shared by tests/test_gpu_tlas_trace.py,
tests/test_gpu_trace_deep.py and tests/test_trace_deep_references.py (a helper module, no tests in it).
Every scene is the tuple (tlas_nodes, instances, meshes, bvh_nodes, vertices, indices) that oracle.trace / Context.trace take."""
import numpy as np

from voidin_amd import abi, synth


def _sphere_mesh(oracle):
    v, i = synth.uv_sphere(0.4, 2)
    v = np.asarray(v, np.float32).reshape(-1, 3)
    nodes, idx = oracle.bvh_build(v, i)
    return nodes, v, idx


def _tlas_chain(leaf_min, leaf_max):
    """The chain over N leaf boxes in the reference's node layout (leaves at 1..N, interior nodes behind them, node 0 = a copy
    of the root): interior node k = {interior k - 1, leaf k}."""
    N = len(leaf_min)
    tl = np.zeros(2 * N, dtype=abi.TLAS_NODE)
    tl["min"][1:N + 1], tl["max"][1:N + 1] = leaf_min, leaf_max
    tl["left_right"][1:N + 1], tl["instance_idx"][1:N + 1] = 0, np.arange(N, dtype=np.uint32)
    if N > 1:
        k = np.arange(1, N, dtype=np.uint32)
        tl["min"][N + 1:] = np.minimum.accumulate(leaf_min, axis=0)[1:]
        tl["max"][N + 1:] = np.maximum.accumulate(leaf_max, axis=0)[1:]
        prev = np.concatenate([[1], N + k[:-1]]).astype(np.uint32)
        tl["left_right"][N + 1:], tl["instance_idx"][N + 1:] = prev | ((1 + k) << np.uint32(16)), 0xFFFFFFFF
    tl[0] = tl[2 * N - 1] if N > 1 else tl[1]
    return tl


def _x_instances(N):
    inst = np.zeros(N, dtype=abi.INSTANCE)
    T = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    T[:, 3, 0] = np.arange(N, dtype=np.float32)            # column-major storage: translation in elements 12..14
    inst["transform"] = T.reshape(N, 16)
    Ti = T.copy(); Ti[:, 3, 0] *= np.float32(-1)
    inst["inv_transform"] = Ti.reshape(N, 16)
    return inst


def chain_scene(oracle, n_leaves=200):
    """A TLAS that is one long chain - interior node k = {interior k - 1, leaf k}, spheres one unit apart along +x - in the
    reference's node layout (leaves at 1..N, interior nodes behind them, node 0 = a copy of the root).  A ray from x = -5
    along +x finds the chain as its NEAR child at every level and pushes the leaf: N - 1 pending entries when it reaches
    sphere 0.  N < 32 768: the layout's child fields are 16 bits wide."""
    nodes, v, idx = _sphere_mesh(oracle)
    infos = np.zeros(1, dtype=abi.MESH_INFO)
    infos[0]["min"], infos[0]["max"] = synth.mesh_bounds(v)
    infos[0]["index_count"] = len(idx)
    N = n_leaves
    assert 1 <= N < 32768
    inst = _x_instances(N)
    shift = np.zeros((N, 3), np.float32); shift[:, 0] = np.arange(N, dtype=np.float32)
    tl = _tlas_chain(infos[0]["min"] + shift, infos[0]["max"] + shift)
    return (tl, inst, infos, nodes, v, idx)


def chain_blas_mesh(n_tris):
    """(nodes, vertices, indices) of a hand-made BLAS chain in the reference's node layout (node 0 the root, node 1 unused, child
    pairs behind): n unit-spaced triangles facing -x; every interior node splits off the FARTHEST triangle (largest x) as a
    one-triangle leaf - its RIGHT child - and keeps the rest as its left child.  n - 3 interior levels above a 3-triangle leaf."""
    n = n_tris
    assert n >= 4
    tri = np.zeros((n, 3, 3), np.float32)
    tri[:, :, 0] = np.arange(n, dtype=np.float32)[:, None]
    tri[:, 0, 1:] = [-0.5, -0.5]; tri[:, 1, 1:] = [0.0, 0.6]; tri[:, 2, 1:] = [0.5, -0.5]
    verts, idx = tri.reshape(-1, 3).copy(), np.arange(3 * n, dtype=np.uint32)
    levels = n - 3
    nodes = np.zeros(2 + 2 * levels, dtype=abi.BVH_NODE)
    box = lambda a, b: (tri[a:b].reshape(-1, 3).min(axis=0), tri[a:b].reshape(-1, 3).max(axis=0))
    cur, hi = 0, n
    for j in range(levels):
        pair = 2 + 2 * j
        nodes[cur]["min"], nodes[cur]["max"] = box(0, hi)
        nodes[cur]["left_first"], nodes[cur]["count"] = pair, 0
        nodes[pair + 1]["min"], nodes[pair + 1]["max"] = box(hi - 1, hi)
        nodes[pair + 1]["left_first"], nodes[pair + 1]["count"] = hi - 1, 1
        cur, hi = pair, hi - 1
    nodes[cur]["min"], nodes[cur]["max"] = box(0, hi)
    nodes[cur]["left_first"], nodes[cur]["count"] = 0, hi
    return nodes, verts, idx


def chain_blas_scene(oracle, n_tris=190):
    """ONE instance whose BLAS is chain_blas_mesh(n_tris).  A ray from x = -1 along +x takes the rest as its near child at
    every level and pushes the leaf (bvh.wgsl:56-74 pushes the far child while nothing is hit): n - 3 pending BLAS entries
    before the first triangle test."""
    nodes, verts, idx = chain_blas_mesh(n_tris)
    infos = np.zeros(1, dtype=abi.MESH_INFO)
    infos[0]["min"], infos[0]["max"] = synth.mesh_bounds(verts)
    infos[0]["index_count"] = len(idx)
    inst = np.zeros(1, dtype=abi.INSTANCE)
    inst["transform"] = inst["inv_transform"] = np.eye(4, dtype=np.float32).reshape(16)
    return (oracle.tlas_build(inst, infos), inst, infos, nodes, verts, idx)


def chain_mixed_scene(oracle, n_leaves, n_tris):
    """chain_scene(n_leaves) whose NEAREST instance (x = 0) holds chain_blas_mesh(n_tris) as a second mesh; the others keep the
    small sphere.  A ray from x = -5 along +x enters that instance with n_leaves - 1 TLAS entries pending and piles n_tris - 3
    BLAS entries on top of them (blas_base > 0), pops them and goes on popping TLAS entries."""
    nodes0, v0, idx0 = _sphere_mesh(oracle)
    nodes1, v1, idx1 = chain_blas_mesh(n_tris)
    infos = np.zeros(2, dtype=abi.MESH_INFO)
    for m, (v, idx) in enumerate(((v0, idx0), (v1, idx1))):
        infos[m]["min"], infos[m]["max"] = synth.mesh_bounds(v)
        infos[m]["index_count"] = len(idx)
    infos[1]["base_index"], infos[1]["vertex_offset"], infos[1]["bvh_index"] = len(idx0), len(v0), len(nodes0)
    N = n_leaves
    assert 2 <= N < 32768
    inst = _x_instances(N)
    inst["mesh"][0] = 1
    shift = np.zeros((N, 3), np.float32); shift[:, 0] = np.arange(N, dtype=np.float32)
    leaf_min, leaf_max = infos[0]["min"] + shift, infos[0]["max"] + shift
    leaf_min[0], leaf_max[0] = infos[1]["min"], infos[1]["max"]
    tl = _tlas_chain(leaf_min, leaf_max)
    return (tl, inst, infos, np.concatenate([nodes0, nodes1]), np.concatenate([v0, v1]), np.concatenate([idx0, idx1]).astype(np.uint32))


def chain_rays(n_rays, far_x, seed=128, cheap=0.3, near_x=-5.0):
    """The rays of the deep tests: eyes spread over 0.6 x 0.6 in y, z; half start at near_x and look along +x (deep: the chain
    is the near child at every level), half start at far_x - beyond the chain's far end - and look along -x (the leaf is the
    near child: no depth at all); a share `cheap` of all looks along +y and leaves the scene at once.  Returns (rays, the masks
    far_side, cheap)."""
    rng = np.random.default_rng(seed)
    rays = np.zeros(n_rays, dtype=abi.RAY)
    rays["eye"] = (rng.random((n_rays, 3)).astype(np.float32) - np.float32(0.5)) * np.array([0.0, 0.6, 0.6], np.float32) + np.array([near_x, 0, 0], np.float32)
    rays["dir"] = np.array([1.0, 0.0, 0.0], np.float32)
    far_side = rng.random(n_rays) < 0.5
    rays["eye"][far_side, 0] = np.float32(far_x)
    rays["dir"][far_side] = np.array([-1.0, 0.0, 0.0], np.float32)
    is_cheap = rng.random(n_rays) < cheap
    rays["dir"][is_cheap] = np.array([0.0, 1.0, 0.0], np.float32)
    return rays, far_side, is_cheap
