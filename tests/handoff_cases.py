"""Inputs for the in-launch hand-offs (tests/test_handoff_cases.py, tests/test_gpu_handoffs.py, tests/test_gpu_stress.py): a helper
module, no tests in it.

A kernel that hands a box from one workgroup to another inside a launch and gets the visibility wrong reads a STALE word: the
copy of the previous launch, or a cache line fetched earlier in this one.  Repeating ONE input cannot show that - the stale word
holds the bytes the fresh one would.  So every family here gives two or three inputs of one shape (same counts, same buffers),
to be alternated on the same device buffers, with their expected outputs from what the family's parity tests already trust:

  A    the base input
  B1   the same topology, every box different (a refit: every vertex / instance moved; a build whose tree is a function of
       normalised positions: A scaled by a power of two, which changes no code and every box)
  B2   builds only: another input of the same size, so links, ranges and counts change too

`teeth` states what the alternation relies on - between two expected outputs every interior box differs in at least one word -
and `meta_teeth` what A / B2 rely on.  They are conditions on the references, asserted, not measured."""
import functools

import numpy as np

from blas_lbvh_bounded_cases import lbvh_bounded_reference
from blas_lbvh_cases import lbvh_reference
from blas_refit_cases import deform, mesh_bounds_reference, refit_reference
from conftest import golden
from voidin_amd import abi, synth

SEED = synth.SEED_BASE + 900
LINEAR = [0, 1, 2, 4, 5, 6, 8, 9, 10]          # rows 0..2 of columns 0..2 of a column-major 4x4: rotation * scale
TRANSLATION = [12, 13, 14]


# ---- what the alternation relies on ---------------------------------------------------------------------------------------------

def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)


def box_changed(a, b):
    """Per node: min or max differs in at least one WORD (bits, not values: -0 / +0 and NaN payloads count)."""
    return (_words(a["min"]) != _words(b["min"])).any(axis=1) | (_words(a["max"]) != _words(b["max"])).any(axis=1)


def blas_interior(nodes):
    """Interior nodes of a VdBvhNode array: count == 0, except the reserved slot 1 nobody refers to."""
    m = nodes["count"] == 0
    if len(nodes) > 1 and not (nodes["left_first"][m] == 1).any():
        m[1] = False
    return m


def tlas_interior(nodes):
    n = (len(nodes) - 1) // 2
    m = np.zeros(len(nodes), dtype=bool)
    m[n + 1:] = True                            # n+1 .. 2n-1, and the closing self-merge 2n
    m[0] = n > 1                                # node 0 copies the root
    return m


def teeth(a, b, interior):
    """Every interior box changes between the two outputs -> (holds, number of interior nodes that keep all six words)."""
    same = interior & ~box_changed(a, b)
    return not same.any(), int(same.sum())


def meta_teeth(a, b):
    """Share of A's interior nodes whose left_first / count differ in B (a node B does not have differs)."""
    inner = np.nonzero(blas_interior(a))[0]
    k = inner[inner < len(b)]
    differ = (a["left_first"][k] != b["left_first"][k]) | (a["count"][k] != b["count"][k])
    return (int(differ.sum()) + int((inner >= len(b)).sum())) / max(len(inner), 1)


# ---- TLAS refit -----------------------------------------------------------------------------------------------------------------

def moved(inst, seed=SEED):
    """Every translation and every scale changed: the linear part times 1.25 .. 1.75, the translation by up to +-40 per axis."""
    n = len(inst)
    out = np.array(inst, copy=True)
    u = np.stack([synth.uniform01(seed, s, n) for s in range(4)], axis=1)
    t = out["transform"].astype(np.float64)
    t[:, LINEAR] *= (1.25 + 0.5 * u[:, 3:4])
    t[:, TRANSLATION] += (u[:, 0:3] - 0.5) * 80.0 + 0.125
    out["transform"] = t.astype(np.float32)
    assert (out["transform"][:, TRANSLATION] != inst["transform"][:, TRANSLATION]).all() and (out["transform"][:, [0, 5, 10]] != inst["transform"][:, [0, 5, 10]]).any(axis=1).all()
    M = np.transpose(out["transform"].reshape(n, 4, 4).astype(np.float64), (0, 2, 1))
    out["inv_transform"] = np.transpose(np.linalg.inv(M), (0, 2, 1)).reshape(n, 16).astype(np.float32)
    return out


def scaled_instances(inst, factor=2.0):
    """The scene times a power of two about the origin: rows 0..2 of every column (translation included), exactly."""
    out = np.array(inst, copy=True)
    out["transform"][:, LINEAR + TRANSLATION] *= np.float32(factor)
    out["inv_transform"][:, LINEAR] /= np.float32(factor)
    return out


def tlas_children(nodes):
    if nodes.dtype == abi.TLAS_NODE_WIDE:
        return nodes["left"].astype(np.int64), nodes["right"].astype(np.int64)
    return (nodes["left_right"] & 0xffff).astype(np.int64), (nodes["left_right"] >> 16).astype(np.int64)


def _set_children(nodes, left, right):
    if nodes.dtype == abi.TLAS_NODE_WIDE:
        nodes["left"], nodes["right"] = left.astype(np.uint32), right.astype(np.uint32)
    else:
        nodes["left_right"] = (left | (right << 16)).astype(np.uint32)


def children_first(nodes):
    """An LBVH top level renumbered so that every interior node's id is above its children's: the same tree, leaves where they
    were, the root still 2n - 1.  vd_tlas_refit* takes any numbering (it follows the links); the oracle's refit sweeps
    n+1 .. 2n in ascending order, as the reference's chain numbers its merges, and the LBVH numbers nodes by split position."""
    n = (len(nodes) - 1) // 2
    if n < 2:
        return np.array(nodes, copy=True)
    left, right = tlas_children(nodes)
    order, stack = [], [(2 * n - 1, False)]
    while stack:
        k, done = stack.pop()
        if k <= n:
            continue
        if done:
            order.append(k)
        else:
            stack += [(k, True), (int(left[k]), False), (int(right[k]), False)]
    order = np.asarray(order, dtype=np.int64)
    assert len(order) == n - 1 and order[-1] == 2 * n - 1
    new = np.arange(2 * n + 1, dtype=np.int64)
    new[order] = n + 1 + np.arange(n - 1)
    out = np.array(nodes, copy=True)
    out[new] = nodes
    _set_children(out, new[left][np.argsort(new)], new[right][np.argsort(new)])
    l2, r2 = tlas_children(out)
    inner = np.arange(n + 1, 2 * n)
    assert (l2[inner] < inner).all() and (r2[inner] < inner).all() and l2[2 * n] == 2 * n - 1 and l2[0] == l2[2 * n - 1] and r2[0] == r2[2 * n - 1]
    return out


def pairwise_topology(n, wide):
    """A valid top level made without a GPU, for the CPU checks: leaf i + 1 is instance i, neighbours are merged level by level
    (ids ascend from children to parents), 2n - 1 is the root, 2n its self-merge, node 0 its copy.  Boxes: zero until refitted."""
    nodes = np.zeros(2 * n + 1, dtype=abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE)
    nodes["instance_idx"] = 0xffffffff
    nodes["instance_idx"][1:n + 1] = np.arange(n, dtype=np.uint32)
    left, right = np.zeros(2 * n + 1, dtype=np.int64), np.zeros(2 * n + 1, dtype=np.int64)
    level, nxt = list(range(1, n + 1)), n + 1
    while len(level) > 1:
        up = []
        for j in range(0, len(level) - 1, 2):
            left[nxt], right[nxt] = level[j], level[j + 1]
            up.append(nxt); nxt += 1
        if len(level) & 1:
            up.append(level[-1])
        level = up
    assert nxt == 2 * n
    left[2 * n] = right[2 * n] = 2 * n - 1
    left[0], right[0] = left[2 * n - 1], right[2 * n - 1]
    _set_children(nodes, left, right)
    return nodes


@functools.lru_cache(maxsize=None)
def tlas_refit_inputs(n):
    """-> (meshes, [("A", instances), ("B1", moved instances)])"""
    meshes = synth.mesh_infos()
    a = synth.instances(n, seed=SEED + 1, extent=300.0 + n / 64.0)
    return meshes, [("A", a), ("B1", moved(a))]


def tlas_refit_expected(oracle, topology, meshes, inputs):
    """oracle.tlas_refit of every instance set over ONE topology (children-first numbering)."""
    return [oracle.tlas_refit(inst, meshes, topology) for _, inst in inputs]


@functools.lru_cache(maxsize=None)
def tlas_lbvh_inputs(n):
    """-> (meshes, [A, B1 = A times two, B2 = another cloud])"""
    meshes = synth.mesh_infos()
    a = synth.instances(n, seed=SEED + 2, extent=200.0 + n / 50.0)
    return meshes, [("A", a), ("B1", scaled_instances(a)), ("B2", synth.instances(n, seed=SEED + 3, extent=150.0 + n / 40.0))]


# ---- BLAS: refit and the builds ---------------------------------------------------------------------------------------------------

def _helmet():
    g = golden("helmet.npz")
    return np.ascontiguousarray(g["vertices"], dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(g["indices"], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices, indices) by name: knot2k (2 048 triangles), sphere (6 320), soup<T>, helmet (15 452), knot32k, and with a
    trailing '*': ANOTHER mesh of the same vertex and triangle counts."""
    if name.endswith("*"):
        v, i = mesh(name[:-1])
        if name.startswith("soup"):
            return synth.triangle_soup(len(i) // 3, seed=SEED + 50 + len(i) // 3)
        # a mesh file has no second seed: axes rotated and stretched unequally, triangles in reverse order - other codes, another tree
        v2 = (v[:, [2, 0, 1]].astype(np.float64) * np.array([1.0, 0.37, 2.9]) + np.array([0.3, -1.1, 0.05])).astype(np.float32)
        return v2, np.ascontiguousarray(i.reshape(-1, 3)[::-1]).reshape(-1)
    if name == "knot2k":
        return synth.knot_mesh(32, 32)
    if name == "knot32k":
        return synth.knot_mesh(256, 64)
    if name == "sphere":
        return synth.uv_sphere(1.0, 10)
    if name == "helmet":
        return _helmet()
    assert name.startswith("soup"), name
    return synth.triangle_soup(int(name[4:]), seed=SEED + 10 + int(name[4:]))


def doubled(v):
    return (np.ascontiguousarray(v, dtype=np.float32) * np.float32(2.0)).astype(np.float32)


REFIT_PLANS = {"three": ("knot2k", "sphere", "soup4097"), "helmet": ("helmet",)}


@functools.lru_cache(maxsize=None)
def blas_refit_inputs(plan, oracle):
    """One plan's meshes, each built once by the oracle's builder -> [(vertices, permuted indices, nodes)] and per input
    ("A": as built, "B1": every vertex displaced) the vertices of every mesh."""
    built = []
    for name in REFIT_PLANS[plan]:
        v, i = mesh(name)
        nodes, idx = oracle.bvh_build(v, i)
        built.append((v, idx, nodes))
    inputs = [("A", [v for v, _, _ in built]), ("B1", [deform(v, phase=0.7 + 0.3 * m, specials=False) for m, (v, _, _) in enumerate(built)])]
    return built, inputs


def blas_refit_expected(built, verts):
    """-> [(nodes of refit_reference, (MeshInfo min, max) of mesh_bounds_reference)] per mesh"""
    return [(refit_reference(v, idx, nodes), mesh_bounds_reference(v)) for v, (_, idx, nodes) in zip(verts, built)]


def lbvh_inputs(name):
    """-> [("A", v, i), ("B1", 2 v, i), ("B2", another mesh of the same counts)]"""
    v, i = mesh(name)
    v2, i2 = mesh(name + "*")
    assert v2.shape == v.shape and i2.shape == i.shape
    return [("A", v, i), ("B1", doubled(v), i), ("B2", v2, i2)]


@functools.lru_cache(maxsize=None)
def lbvh_expected(name, bound):
    """The restatement of every input of lbvh_inputs(name): lbvh_reference (bound 0) or lbvh_bounded_reference."""
    return [lbvh_reference(v, i) if not bound else lbvh_bounded_reference(v, i, bound) for _, v, i in lbvh_inputs(name)]


PLAN_CAPS = [3, 4, 300, 1025, 4097]
PLAN_COUNTS = {"A": [3, 4, 300, 1025, 4097], "B1": [0, 3, 4, 1025, 2000], "B2": [3, 4, 300, 1000, 4097]}


@functools.lru_cache(maxsize=None)
def lbvh_plan_inputs():
    """Five meshes of PLAN_CAPS triangles; per input the vertices of every mesh and the count vector: A, B1 (vertices times two AND
    other counts), B2 (other soups, a third count vector) -> {input: (vertices per mesh, indices per mesh, counts)}"""
    a = [synth.triangle_soup(c, seed=SEED + 100 + c) for c in PLAN_CAPS]
    b2 = [synth.triangle_soup(c, seed=SEED + 200 + c) for c in PLAN_CAPS]
    return {"A": ([v for v, _ in a], [i for _, i in a], PLAN_COUNTS["A"]),
            "B1": ([doubled(v) for v, _ in a], [i for _, i in a], PLAN_COUNTS["B1"]),
            "B2": ([v for v, _ in b2], [i for _, i in b2], PLAN_COUNTS["B2"])}


@functools.lru_cache(maxsize=None)
def lbvh_plan_expected():
    """Per input, per mesh: the restatement of the single build of its first min(count, cap) triangles (None when that is 0)."""
    out = {}
    for tag, (vs, idx, counts) in lbvh_plan_inputs().items():
        out[tag] = [None if min(c, cap) == 0 else lbvh_reference(v, i[: 3 * min(c, cap)]) for v, i, c, cap in zip(vs, idx, counts, PLAN_CAPS)]
    return out


BUILD_MESHES = ("soup3000", "soup9000", "knot32k")


@functools.lru_cache(maxsize=None)
def bvh_build_inputs(name):
    """vd_bvh_build_dev: A, B1 = A times two, B2 = another mesh of the same counts -> [(tag, vertices, indices)]"""
    return lbvh_inputs(name)


def bvh_build_expected(oracle, name):
    """oracle.bvh_build of every input -> [(nodes, permuted indices)]"""
    return [oracle.bvh_build(v, i) for _, v, i in bvh_build_inputs(name)]
