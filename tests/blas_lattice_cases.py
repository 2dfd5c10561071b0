"""Lattice meshes for the SAH BLAS build, and an instrumented numpy restatement that counts on them what random vertex
data never produces (tests/test_blas_lattice_cases.py, tests/test_gpu_blas_lattice.py): a helper module, no tests in it,
and neither HIP nor torch.

vd_bvh_build* emulates the reference's sequential recursion (crates/bvh/src/blas.rs:135-182): 21 trial shuffles per node,
`cost < optimal_cost` keeps the FIRST minimum in (axis, bin) order, the predicate is `centroid[axis] < pos`, one element
per shuffle is never examined.  With vertices on a lattice two things happen in nodes of every size that a soup shows only
in its smallest nodes: two different splits with exactly the same cost, and centroids exactly on a split plane.  Census
counts both per node; Mutant is the restatement with `<=` in one of the two places, in nodes of one size class only."""
import numpy as np

from oracle import np_restate as npr
from voidin_amd import synth

F = np.float32

# The node-size classes, one per implementation of the reduction over the 21 costs and of the predicate in the kernels.
# Stated here as data, not read from the kernel source: 32 is the largest node a lane group (8, 16 or 32 lanes) takes inside
# phase B, 512 is VD_SMALL_MAX (the largest subtree of phase B, one wave each), 2048 is VD_MID_MAX (the largest segment of
# the mid tier, one workgroup out of LDS); everything above goes through the level-synchronous rounds of phase A.
LANE_GROUP_MAX, VD_SMALL_MAX, VD_MID_MAX = 32, 512, 2048
SIZE_CLASSES = {"<=32": (4, LANE_GROUP_MAX), "33..512": (LANE_GROUP_MAX + 1, VD_SMALL_MAX),
                "513..2048": (VD_SMALL_MAX + 1, VD_MID_MAX), ">2048": (VD_MID_MAX + 1, 1 << 32)}      # inclusive; a node of <= 3 is a leaf


def size_class(count):
    for name, (lo, hi) in SIZE_CLASSES.items():
        if lo <= count <= hi:
            return name
    return "leaf"


# ------------------------------------------------------------------ generators -------------------------------------------
def grid(nx, ny, sx, sy, height=None, diagonals="same"):
    """nx x ny cells, vertices at (i * sx, j * sy, height(i, j)) (flat when height is None), two triangles per cell.
    diagonals: "same" cuts every cell from its (i, j) corner to its (i + 1, j + 1) corner, "alternating" flips the cut
    where i + j is odd."""
    assert diagonals in ("same", "alternating")
    jj, ii = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    z = np.zeros_like(ii) if height is None else height(ii, jj)
    v = np.stack([ii * sx, jj * sy, z], axis=-1).reshape(-1, 3).astype(F)
    cj, ci = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    v00 = (cj * (nx + 1) + ci).reshape(-1)
    v10, v01, v11 = v00 + 1, v00 + nx + 1, v00 + nx + 2
    same = np.stack([v00, v10, v11, v00, v11, v01], axis=1)
    if diagonals == "alternating":
        flip = ((ci + cj) % 2 == 1).reshape(-1, 1)
        same = np.where(flip, np.stack([v00, v10, v01, v10, v11, v01], axis=1), same)
    return v, same.reshape(-1).astype(np.uint32)


def voxel_surface(n, seed, fill):
    """The boundary quads (two triangles each) of a random occupancy grid of n^3 cells, a cell filled with probability
    `fill`: every face between a filled cell and an empty one or the outside.  Vertices are shared and sit at multiples of 3."""
    occ = np.zeros((n + 2,) * 3, dtype=bool)
    occ[1:-1, 1:-1, 1:-1] = (synth.uniform01(seed, 7, n ** 3) < fill).reshape(n, n, n)
    ids = -np.ones((n + 1,) * 3, dtype=np.int64)
    verts, tris = [], []

    def vid(p):
        if ids[p] < 0:
            ids[p] = len(verts)
            verts.append(p)
        return ids[p]

    for cell in np.argwhere(occ):
        for axis in range(3):
            for side in (0, 1):
                nb = cell.copy(); nb[axis] += 2 * side - 1
                if occ[tuple(nb)]:
                    continue
                u, w = [a for a in range(3) if a != axis]
                base = cell - 1                                  # lattice corner of the cell
                base[axis] += side
                q = []
                for du, dw in ((0, 0), (1, 0), (1, 1), (0, 1)):
                    p = base.copy(); p[u] += du; p[w] += dw
                    q.append(vid(tuple(p)))
                if side == 0:
                    q = q[::-1]
                tris += [q[0], q[1], q[2], q[0], q[2], q[3]]
    return (np.asarray(verts, dtype=F) * F(3.0)).astype(F), np.asarray(tris, dtype=np.uint32)


def with_repeats(v, i, tri, times):
    """The mesh with triangle `tri` appended `times` more times: times + 1 >= 4 equal centroids end in one node below the
    root that no candidate can split - the reference crashes there, the oracle and the library say VD_ERR_DEGENERATE."""
    i = np.asarray(i, dtype=np.uint32)
    return v, np.concatenate([i, np.tile(i[3 * tri: 3 * tri + 3], times)])


_CASES = {
    "grid_48x48": lambda: grid(48, 48, 3, 3),                                   # 4608: two levels of phase A
    "grid_33x32": lambda: grid(33, 32, 3, 3),                                   # 2112: just past the mid tier's limit
    "grid_24x24": lambda: grid(24, 24, 3, 3),                                   # 1152: the root is a mid-tier segment
    "grid_16x16": lambda: grid(16, 16, 3, 3),                                   # 512: the root is exactly a phase-B subtree
    "grid_37x29_alt": lambda: grid(37, 29, 3, 6, diagonals="alternating"),      # 2146: not square, unequal spacing
    "grid_23x23_height": lambda: grid(23, 23, 3, 3, height=lambda i, j: 3 * ((i * j) % 5)),      # 1058: h(i, j) = h(j, i)
    "grid_32x32_unit": lambda: grid(32, 32, 1, 1),                              # 2048 = VD_MID_MAX; centroids are thirds: ties through rounding
    "voxel_10": lambda: voxel_surface(10, synth.SEED_BASE + 900, 0.45),
    "voxel_6": lambda: voxel_surface(6, synth.SEED_BASE + 901, 0.45),
}
NAMES = list(_CASES)
_made = {}


def case(name):
    """(vertices, indices) of one named case, made once, read-only."""
    if name not in _made:
        v, i = _CASES[name]()
        v.setflags(write=False); i.setflags(write=False)
        _made[name] = (v, i)
    return _made[name]


def deep_degenerate():
    """The 24 x 24 grid with triangle 700 four more times: five equal centroids, far below the root."""
    v, i = case("grid_24x24")
    return with_repeats(v, i, 700, 4)


# ------------------------------------------------------------------ the instrument ---------------------------------------
class Census(npr._Blas):
    """np_restate._Blas with `partition` recording, per interior node, what the docstring of this module names.  The tree
    is the restatement's: the same shuffles in the same order on the same id list."""
    record = True
    le_cost = le_pred = None                                     # Mutant: the size class in which `<` becomes `<=`

    def __init__(self, verts, indices):
        super().__init__(verts, indices)
        self.rows = []

    def _in(self, cls, count):
        return cls is not None and SIZE_CLASSES[cls][0] <= count <= SIZE_CLASSES[cls][1]

    def shuffle_le(self, axis, pos, start, count):
        """shuffle with `centroid <= pos`."""
        ids, key = self.ids, self.cent_cols[axis]
        pos = float(pos)
        i, e = start, start + count - 1
        while i < e:
            if key[ids[i]] <= pos:
                i += 1
            else:
                ids[i], ids[e] = ids[e], ids[i]
                e -= 1
        return i

    def partition(self, start, count):
        shuffle = self.shuffle_le if self._in(self.le_pred, count) else self.shuffle
        le_cost = self._in(self.le_cost, count)
        best = (0, F(0), 0, np.finfo(F).max)
        ok = False
        cmn, cmx = self.bounds(start, count, True)
        costs, lefts = [], []
        on_plane = on_plane_flat = 0
        if self.record:
            members = np.asarray(self.ids[start:start + count], dtype=np.int64)
        with np.errstate(over="ignore", invalid="ignore"):
            for axis in range(3):
                for k in range(1, 8):
                    scale = F(k) / F(8)
                    pos = F(cmn[axis] + F(F(cmx[axis] - cmn[axis]) * scale))
                    piv = shuffle(axis, pos, start, count)
                    n1 = piv - start
                    n2 = count - n1
                    a1 = npr._area(*self.bounds(start, n1, False))
                    a2 = npr._area(*self.bounds(piv, n2, False))
                    cost = F(F(a1 * F(n1)) + F(a2 * F(n2)))
                    if self.record:
                        costs.append(cost)
                        lefts.append(frozenset(self.ids[start:piv]))          # the arrangement itself: the unexamined element is right
                        hits = int((self.cent[members, axis] == pos).sum())
                        if cmx[axis] != cmn[axis]:
                            on_plane += hits
                        else:
                            on_plane_flat += hits
                    if (cost <= best[3]) if le_cost else (cost < best[3]):
                        best = (axis, pos, piv, cost)
                        ok = True
        shuffle(best[0], best[1], start, count)
        if not ok:
            raise ValueError("degenerate")
        if self.record:
            c = np.asarray(costs, dtype=F)
            winners = np.flatnonzero(c == best[3])                              # a NaN or rejected cost never equals the minimum
            sets = {lefts[w] for w in winners}
            cross = any(lefts[a] != lefts[b] and a // 7 != b // 7 for a in winners for b in winners)
            self.rows.append({"count": count, "costs": c, "lefts": lefts, "on_plane": on_plane, "on_plane_flat": on_plane_flat,
                              "tied": len(sets) >= 2, "tied_across_axes": cross})
        return best[2]

    def table(self):
        """class -> dict(nodes, tied, tied_across_axes, on_plane, on_plane_flat) over the interior nodes recorded."""
        out = {c: dict(nodes=0, tied=0, tied_across_axes=0, on_plane=0, on_plane_flat=0) for c in SIZE_CLASSES}
        for r in self.rows:
            t = out[size_class(r["count"])]
            t["nodes"] += 1
            for k in ("tied", "tied_across_axes", "on_plane", "on_plane_flat"):
                t[k] += int(r[k])
        return out


class Mutant(Census):
    """The restatement with ONE change, applied only in nodes whose count lies in `size_class`:
    kind="tie": `cost <= best`, the last minimum wins; kind="predicate": `centroid <= pos` in the shuffles."""
    record = False

    def __init__(self, kind, size_class, verts, indices):
        assert kind in ("tie", "predicate") and size_class in SIZE_CLASSES
        super().__init__(verts, indices)
        if kind == "tie":
            self.le_cost = size_class
        else:
            self.le_pred = size_class


def census(verts, indices):
    """-> (Census after its build, (nodes, indices))."""
    c = Census(verts, indices)
    return c, c.build()


def mutant_build(kind, size_class, verts, indices):
    """-> (nodes, indices), or None where the mutant finds no split at all in some node."""
    try:
        return Mutant(kind, size_class, verts, indices).build()
    except ValueError:
        return None


def format_table(name, n_tri, table):
    lines = [f"{name} ({n_tri} triangles)", "  class       nodes   tied  across-axes  on-plane  on-plane(zero extent)"]
    for c, t in table.items():
        lines.append(f"  {c:<10} {t['nodes']:6d} {t['tied']:6d} {t['tied_across_axes']:12d} {t['on_plane']:9d} {t['on_plane_flat']:9d}")
    return "\n".join(lines)


# ------------------------------------------------------------------ reading a tree ----------------------------------------
def subtree_counts(nodes):
    """Primitive count under every node of a BLAS array (0 for the unused node 1)."""
    n = len(nodes)
    out = np.zeros(n, dtype=np.int64)
    for k in range(n - 1, -1, -1):                               # children come after their parent
        if k == 1:
            continue
        c = int(nodes["count"][k])
        l = int(nodes["left_first"][k])
        out[k] = c if c > 0 else out[l] + out[l + 1]
    return out


def preorder(nodes):
    """Node ids in pre-order (a pair is allocated when its parent is subdivided, so array order is not pre-order)."""
    out, todo = [], [0]
    while todo:
        k = todo.pop()
        out.append(k)
        if nodes["count"][k] == 0:
            l = int(nodes["left_first"][k])
            todo += [l + 1, l]
    return out


def first_difference(got, want):
    """One line naming the first node, in pre-order of the expected tree, in which `got` differs from it: its primitive
    count in the expected tree and that count's size class - which tier of the builder to open."""
    if len(got) != len(want):
        head = f"node count {len(got)} != {len(want)}; "
        got = np.concatenate([got, np.zeros(max(0, len(want) - len(got)), dtype=want.dtype)])[: len(want)]
    else:
        head = ""
    counts = subtree_counts(want)
    for k in preorder(want):
        if got[k: k + 1].tobytes() != want[k: k + 1].tobytes():
            return (f"{head}first differing node {k} (pre-order): {counts[k]} primitives, size class {size_class(int(counts[k]))}; "
                    f"got {got[k]} want {want[k]}")
    return head + "all nodes equal"
