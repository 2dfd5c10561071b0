"""CPU restatement of the depth-bounded LBVH bottom level (VD_OPT_BLAS_LBVH_MAX_DEPTH; tests/test_blas_lbvh_bounded_cases.py,
tests/test_gpu_blas_lbvh_bounded.py): a helper module, no tests in it.

The restatement follows the definition in include/voidin_abi.h TOP-DOWN, node by node with its depth and its mode, where the
kernels climb the unbounded radix tree, give every position under a switch node a new 64-bit key and build a second radix tree
over those keys.  Box, code and order come from blas_lbvh_cases, the boxes of the nodes from blas_refit_cases.refit_reference."""
import numpy as np

from blas_lbvh_cases import _with_nan_vertex, codes_of_boxes, triangle_boxes
from blas_refit_cases import refit_reference
from voidin_amd import abi, synth

MAX_BOUND = 62


def needr(k):
    """Depth of the radix tree over the integers 0 .. k - 1 cut off at nodes of <= 3 positions."""
    return 0 if k <= 3 else (k - 1).bit_length() - 1


def effective_bound(D):
    """The option's value as the library reads it: negative and 0 are unbounded (0), values above 62 are 62."""
    return 0 if D is None or D <= 0 else min(int(D), MAX_BOUND)


def lbvh_bounded_reference(verts, indices, D):
    """-> dict(nodes, indices, n_nodes, max_depth, n_bad_indices, codes (sorted), order, switches, switch_positions,
    switch_delta_below_32, switch_delta_from_32): the tree of the definition for the bound D (0: unbounded).  A ValueError when
    needr(T) > D, which the library refuses."""
    D = effective_bound(D)
    bmin, bmax, n_bad = triangle_boxes(verts, indices)
    tri = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
    T = len(tri)
    if D and needr(T) > D:
        raise ValueError(f"needr({T}) = {needr(T)} > {D}")
    codes = codes_of_boxes(bmin, bmax)
    order = np.argsort(codes, kind="stable")
    keys = (codes[order].astype(np.uint64) << np.uint64(32)) | np.arange(T, dtype=np.uint64)
    nodes = np.zeros(max(2, 2 * T), dtype=abi.BVH_NODE)
    pool, max_depth = 2, 0
    switches = switch_positions = below32 = from32 = 0
    todo = [(0, 0, T - 1, 0, None)]                                       # node id, lo, hi, depth, base (None: radix mode)
    while todo:
        k, lo, hi, depth, base = todo.pop()
        n = hi - lo + 1
        if n <= 3:
            nodes["left_first"][k], nodes["count"][k] = lo, n
            max_depth = max(max_depth, depth)
            continue
        if base is None:
            a, z = int(keys[lo]), int(keys[hi])
            b = (a ^ z).bit_length() - 1                                  # the highest bit in which the end keys differ
            s = lo + int(np.searchsorted(keys[lo:hi + 1], np.uint64(((a >> b) | 1) << b), side="left"))
            assert lo < s <= hi
            if D and depth + 1 + needr(max(s - lo, hi - s + 1)) > D:      # a switch node: position mode from here down
                base = lo
                switches += 1
                switch_positions += n
                if 63 - b < 32:
                    below32 += 1
                else:
                    from32 += 1
        if base is not None:
            a = lo - base
            b = (a ^ (hi - base)).bit_length() - 1
            s = base + (((a >> b) | 1) << b)
            assert lo < s <= hi
        if D:
            assert depth + needr(n) <= D                                  # the invariant of the definition
        nodes["left_first"][k], nodes["count"][k] = pool, 0
        todo.append((pool + 1, s, hi, depth + 1, base))                   # popped second: the right subtree follows the whole left one
        todo.append((pool, lo, s - 1, depth + 1, base))
        pool += 2
    v_ext, tri_ext, _ = _with_nan_vertex(verts, indices)
    out = refit_reference(v_ext, tri_ext[order].reshape(-1), nodes[:pool])
    return {"nodes": out, "indices": np.ascontiguousarray(tri[order]).reshape(-1), "n_nodes": pool, "max_depth": max_depth,
            "n_bad_indices": n_bad, "codes": codes[order], "order": order, "switches": switches, "switch_positions": switch_positions,
            "switch_delta_below_32": below32, "switch_delta_from_32": from32}


def duplicates_case():
    """300 soup triangles, each 7 times, in shuffled order: ranges of equal codes hold more positions than there are codes, so
    switch nodes occur both above (end codes differ) and inside (end codes equal) a run of equal codes."""
    v, i = synth.triangle_soup(300, seed=synth.SEED_BASE + 310)
    tri = np.tile(i.reshape(-1, 3), (7, 1))
    tri = tri[np.random.default_rng(311).permutation(len(tri))]
    return v, np.ascontiguousarray(tri, dtype=np.uint32).reshape(-1)


def random_cases(n=40, seed=312):
    """n fixed-seed soups of 1 .. 3000 triangles with vertices on a 1/8 grid (many equal codes), each with a bound of
    needr(T) + 0 .. 5: -> list of (vertices, indices, D)."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        T = int(rng.integers(1, 3001))
        v, i = synth.triangle_soup(T, seed=synth.SEED_BASE + 320 + c)
        v = (np.round(v * np.float32(8.0)) / np.float32(8.0)).astype(np.float32)
        out.append((v, i, max(1, needr(T) + int(rng.integers(0, 6)))))
    return out
