"""CPU restatement and inputs for the LBVH bottom level (vd_bvh_build_lbvh*; tests/test_blas_lbvh_cases.py,
tests/test_gpu_blas_lbvh.py): a helper module, no tests in it.

The restatement follows the definition in include/voidin_abi.h with another algorithm than the kernels': the tree is built
TOP-DOWN over the 64-bit keys code << 32 | sorted position - the split of a range is the first position whose key has the
highest bit in which the range's end keys differ, found by searchsorted - recursing in the reference's order (the pair of
children is allocated when a node is subdivided, then the whole left subtree, then the right; blas.rs:105-128), and the
boxes come from blas_refit_cases.refit_reference.  The kernels build Karras' tree bottom-up and number it afterwards."""
import numpy as np

from blas_refit_cases import bits, key, key_hi, key_lo, refit_reference, unkey
from voidin_amd import abi, synth

BAD_CODE = 0x3fffffff
NAN = np.float32(np.nan)


def _with_nan_vertex(verts, indices):
    """(vertices + one NaN vertex, triples with every index >= n_vert pointing at it, number of such indices)."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    tri = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
    bad = tri >= len(v)
    return np.concatenate([v, np.full((1, 3), NAN, dtype=np.float32)]), np.where(bad, np.uint32(len(v)), tri), int(bad.sum())


def triangle_boxes(verts, indices):
    """(min (T,3), max (T,3), bad indices): three corners folded from (+1e30, -1e30), a NaN ignored, -0 < +0."""
    v, tri, n_bad = _with_nan_vertex(verts, indices)
    tv = v[tri]
    lo = np.minimum(key_lo(tv).min(axis=1), key(np.float32(1e30)))
    hi = np.maximum(key_hi(tv).max(axis=1), key(np.float32(-1e30)))
    return unkey(lo), unkey(hi), n_bad


def _spread10(v):
    v = (v | (v << 16)) & 0x030000ff
    v = (v | (v << 8)) & 0x0300f00f
    v = (v | (v << 4)) & 0x030c30c3
    return (v | (v << 2)) & 0x09249249


def codes_of_boxes(bmin, bmax):
    """The key of vd_tlas_build_lbvh*: centre 0.5 * (min + max) in float32, 10 bits per axis of the extent of the finite
    centres, x highest; a non-finite centre -> 0x3fffffff."""
    with np.errstate(all="ignore"):
        c = (np.float32(0.5) * (bmin + bmax).astype(np.float32)).astype(np.float32)
        fin = np.isfinite(c).all(axis=1)
        codes = np.full(len(c), BAD_CODE, dtype=np.uint32)
        if not fin.any():
            return codes
        lo, hi = c[fin].min(axis=0), c[fin].max(axis=0)
        q = np.zeros((len(c), 3), dtype=np.uint64)
        for k in range(3):
            if hi[k] > lo[k]:
                t = ((c[:, k] - lo[k]).astype(np.float32) / np.float32(hi[k] - lo[k])).astype(np.float32)
                s = np.fmin(np.fmax((t * np.float32(1024.0)).astype(np.float32), np.float32(0.0)), np.float32(1023.0))
                q[:, k] = np.where(fin, s, np.float32(0.0)).astype(np.uint64)
        m = (_spread10(q[:, 0]) << np.uint64(2)) | (_spread10(q[:, 1]) << np.uint64(1)) | _spread10(q[:, 2])
        codes[fin] = m[fin].astype(np.uint32)
    return codes


def lbvh_reference(verts, indices):
    """-> dict(nodes, indices, n_nodes, max_depth, n_bad_indices, codes (sorted), order)."""
    bmin, bmax, n_bad = triangle_boxes(verts, indices)
    tri = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
    T = len(tri)
    codes = codes_of_boxes(bmin, bmax)
    order = np.argsort(codes, kind="stable")
    keys = (codes[order].astype(np.uint64) << np.uint64(32)) | np.arange(T, dtype=np.uint64)
    nodes = np.zeros(max(2, 2 * T), dtype=abi.BVH_NODE)
    pool, max_depth = 2, 0
    todo = [(0, 0, T - 1, 0)]
    while todo:
        k, lo, hi, depth = todo.pop()
        if hi - lo + 1 <= 3:
            nodes["left_first"][k], nodes["count"][k] = lo, hi - lo + 1
            max_depth = max(max_depth, depth)
            continue
        a = int(keys[lo])
        b = (a ^ int(keys[hi])).bit_length() - 1                          # the highest bit in which the end keys differ
        first_with_bit = ((a >> b) | 1) << b
        s = lo + int(np.searchsorted(keys[lo:hi + 1], np.uint64(first_with_bit), side="left"))
        assert lo < s <= hi
        nodes["left_first"][k], nodes["count"][k] = pool, 0
        todo.append((pool + 1, s, hi, depth + 1))                         # popped second: the right subtree follows the whole left one
        todo.append((pool, lo, s - 1, depth + 1))
        pool += 2
    v_ext, tri_ext, _ = _with_nan_vertex(verts, indices)
    out = refit_reference(v_ext, tri_ext[order].reshape(-1), nodes[:pool])
    return {"nodes": out, "indices": np.ascontiguousarray(tri[order]).reshape(-1), "n_nodes": pool, "max_depth": max_depth,
            "n_bad_indices": n_bad, "codes": codes[order], "order": order}


def unit_radius(verts):
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    return (v / np.float32(np.linalg.norm(v.astype(np.float64), axis=1).max())).astype(np.float32)


def knot():
    """synth.knot_mesh(96, 48) scaled to unit radius: 9 216 triangles."""
    v, i = synth.knot_mesh(96, 48)
    return unit_radius(v), i


def sphere():
    """synth.uv_sphere(1.0, 24) scaled to unit radius: 36 672 triangles."""
    v, i = synth.uv_sphere(1.0, 24)
    return unit_radius(v), i


def point_triangles(xs):
    """One degenerate triangle per x: all three corners at (x, 0, 0) - its box and centre are that point."""
    xs = np.asarray(xs, dtype=np.float32)
    v = np.zeros((3 * len(xs), 3), dtype=np.float32)
    v[:, 0] = np.repeat(xs, 3)
    return v, np.arange(3 * len(xs), dtype=np.uint32)


def special_cases():
    """name -> (vertices, indices): what a total build must take."""
    out = {}
    v, i = synth.triangle_soup(1)
    out["identical_1000"] = (v, np.tile(i, 1000))
    t = np.arange(700, dtype=np.float32)
    base = np.stack([t * np.float32(0.25), t * np.float32(0.5), t * np.float32(-0.125)], axis=1)          # centres on one line
    lv = np.stack([base, base + np.float32([0.1, 0, 0]), base + np.float32([0, 0.1, 0])], axis=1).reshape(-1, 3).astype(np.float32)
    out["collinear_700"] = (lv, np.arange(3 * 700, dtype=np.uint32))
    v, i = synth.triangle_soup(300, seed=synth.SEED_BASE + 61)
    v = v.copy()
    v[np.abs(v) < 1.0] = 0.0
    z = v.reshape(-1)
    zero = np.nonzero(z == 0.0)[0]
    z[zero[::2]] = np.float32(-0.0)                                                                       # every other zero is -0
    out["signed_zeros_300"] = (v, i)
    v, i = synth.triangle_soup(200, seed=synth.SEED_BASE + 62)
    v = v.copy(); v[17, 1] = NAN
    out["nan_vertex_200"] = (v, i)
    v, i = synth.triangle_soup(200, seed=synth.SEED_BASE + 63)
    v = v.copy(); v[31, 0] = np.float32(np.inf); v[90, 2] = np.float32(-np.inf)
    out["inf_vertex_200"] = (v, i)
    v, i = synth.triangle_soup(200, seed=synth.SEED_BASE + 64)
    v = v.copy(); v[3 * 50: 3 * 51] = NAN; v[3 * 51, 0] = bits(0x7f800001)                                # one all-NaN triangle, one signalling NaN
    out["nan_triangle_200"] = (v, i)
    return out


def bad_index_case():
    v, i = synth.triangle_soup(100, seed=synth.SEED_BASE + 65)
    i = i.copy(); i[3 * 40 + 1] = len(v); i[3 * 77] = 0xffffffff
    return v, i
