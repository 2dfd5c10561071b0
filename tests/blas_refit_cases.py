"""CPU reference and inputs for the BLAS refit tests (tests/test_blas_refit_abi.py, tests/test_gpu_blas_refit.py).

The reference is plain numpy: leaf boxes from `vertices[indices_out]`, folded from (+1e30, -1e30); interior boxes as the
union of the two children, visiting node ids in DESCENDING order (children always follow their parent in the builder's
pre-order).  Every min / max runs on the order-preserving integer image of the float bits, with a NaN mapped to the
neutral element of the fold: that is Rust's f32::min / max (a NaN operand is ignored) with the oracle's tie rule
-0 < +0 (oracle/vd_oracle_math.h)."""
import numpy as np

I32_MAX, I32_MIN = np.int64(0x7fffffff), np.int64(-0x80000000)


def key(f):
    """float32 array -> int64 keys with the order of the floats, -0 below +0 (NaNs land outside the +-inf keys)."""
    i = np.ascontiguousarray(f, dtype=np.float32).view(np.int32).astype(np.int64)
    return i ^ ((i >> 31) & 0x7fffffff)


def unkey(k):
    k = np.asarray(k, dtype=np.int64)
    return (k ^ ((k >> 31) & 0x7fffffff)).astype(np.int32).view(np.float32)


def key_lo(f):
    """operand of a min: a NaN never wins"""
    f = np.ascontiguousarray(f, dtype=np.float32)
    return np.where(np.isnan(f), I32_MAX, key(f))


def key_hi(f):
    """operand of a max: a NaN never wins"""
    f = np.ascontiguousarray(f, dtype=np.float32)
    return np.where(np.isnan(f), I32_MIN, key(f))


def refit_reference(vertices, indices_out, nodes):
    """nodes with min / max recomputed for `vertices`; left_first / count (and node 1, and unreachable nodes) untouched."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    tri = np.ascontiguousarray(indices_out, dtype=np.uint32).reshape(-1, 3)
    out = np.array(nodes, copy=True)
    n = len(out)
    tv = v[tri]                                                   # (T, 3 corners, 3 axes)
    tmin, tmax = key_lo(tv).min(axis=1), key_hi(tv).max(axis=1)   # per triangle
    kmin = np.full((n, 3), key(np.float32(1e30)), dtype=np.int64)
    kmax = np.full((n, 3), key(np.float32(-1e30)), dtype=np.int64)
    count, first = out["count"].astype(np.int64), out["left_first"].astype(np.int64)
    reach = np.zeros(n, dtype=bool)
    reach[0] = True
    for k in range(n):                                            # parents come first: reachability in one ascending sweep
        if reach[k] and count[k] == 0:
            reach[first[k]] = reach[first[k] + 1] = True
    leaves = np.nonzero(reach & (count > 0))[0]
    for c in range(int(count[leaves].max()) if len(leaves) else 0):
        sel = leaves[count[leaves] > c]
        kmin[sel] = np.minimum(kmin[sel], tmin[first[sel] + c])
        kmax[sel] = np.maximum(kmax[sel], tmax[first[sel] + c])
    for k in range(n - 1, -1, -1):                                # children follow their parent: descending ids
        if reach[k] and count[k] == 0:
            l = first[k]
            kmin[k] = np.minimum(kmin[l], kmin[l + 1])
            kmax[k] = np.maximum(kmax[l], kmax[l + 1])
    mn, mx = out["min"].copy(), out["max"].copy()
    mn[reach], mx[reach] = unkey(kmin[reach]), unkey(kmax[reach])
    out["min"], out["max"] = mn, mx
    return out


def mesh_bounds_reference(vertices):
    """MeshPool::calculate_bounds (crates/pools/src/mesh/mod.rs:22-27): ALL vertices, from (+inf, -inf), NaN ignored."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    lo = np.minimum(key_lo(v).min(axis=0), key(np.float32(np.inf))) if len(v) else np.full(3, key(np.float32(np.inf)))
    hi = np.maximum(key_hi(v).max(axis=0), key(np.float32(-np.inf))) if len(v) else np.full(3, key(np.float32(-np.inf)))
    return unkey(lo), unkey(hi)


def bits(u32):
    return np.array([u32], dtype=np.uint32).view(np.float32)[0]


QUIET_NAN, SIGNALLING_NAN = bits(0x7fc00000), bits(0x7f800001)
SPECIALS = [QUIET_NAN, SIGNALLING_NAN, np.float32(0.0), np.float32(-0.0), np.float32(3e30)]


def deform(vertices, phase=0.0, specials=True):
    """A smooth displacement of every vertex; then a few coordinates overwritten with a quiet NaN, a signalling NaN, +0, -0
    and one value beyond 1e30 (as raw bits: a signalling NaN does not survive float arithmetic)."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    p = v.astype(np.float64)
    d = np.stack([0.35 * np.sin(1.3 * p[:, 1] + phase) + 0.1 * p[:, 0], 0.25 * np.cos(0.9 * p[:, 2] - phase),
                  0.3 * np.sin(0.7 * p[:, 0] + 2.0 * phase) - 0.05 * p[:, 2]], axis=1)
    out = (p + d).astype(np.float32)
    if specials:
        flat = out.reshape(-1).view(np.uint32)
        n = len(flat)
        for j, s in enumerate(SPECIALS):
            flat[(j * 7919 + 1) % n] = np.array([s], dtype=np.float32).view(np.uint32)[0]
    return out


def with_outlier(vertices):
    """One extra vertex no triangle refers to, far outside the mesh: the (+inf, -inf) fold over ALL vertices and the root
    box (referenced vertices only) then differ."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    return np.concatenate([v, np.array([[1234.5, -2345.5, 3456.5]], dtype=np.float32)])


def chain_mesh(n_tri, ratio):
    """The generator of tests/test_gpu_blas.py::test_chain_like_trees_vs_oracle: triangles at geometrically growing
    distances, so the tree is one long chain."""
    x = (ratio ** np.arange(n_tri, dtype=np.float64)).astype(np.float32)
    v = np.zeros((3 * n_tri, 3), dtype=np.float32)
    v[0::3, 0] = x; v[1::3, 0] = x * np.float32(1.01); v[2::3, 0] = x
    v[1::3, 1] = 0.5; v[2::3, 2] = 0.5
    return v, np.arange(3 * n_tri, dtype=np.uint32)


def tree_depth(nodes):
    depth = np.zeros(len(nodes), dtype=np.int64)
    for k in range(len(nodes)):
        if nodes["count"][k] == 0 and k != 1:
            l = int(nodes["left_first"][k]); depth[l] = depth[l + 1] = depth[k] + 1
    return int(depth.max())


FIXTURES = ["blas_plane.npz", "blas_sphere_1_1.npz", "blas_soup64.npz", "blas_knot_2k.npz", "blas_sphere_1_10.npz",
            "blas_plane_rot.npz", "blas_cube_obj.npz", "blas_soup_nan.npz",
            "blas_grid_24.npz", "blas_voxel_6.npz"]      # lattice meshes (tests/blas_lattice_cases.py): flat boxes, shared vertices
