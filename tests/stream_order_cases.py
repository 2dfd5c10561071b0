"""Inputs for the stream-order test (tests/test_stream_order_cases.py, tests/test_gpu_stream_order.py): a helper module, no tests
in it, nothing here touches the GPU.

A launch, memset or copy that the library puts on the wrong stream, or a blocking copy it makes without waiting for the context's
stream, runs AHEAD of work the caller queued on that stream.  The GPU test queues a long delay and then the upload of input B on
a side stream while the buffers still hold input A, and calls the entry point: whatever runs out of order sees A (or a mixture),
or writes its result before the delay has ended.  So every case gives two inputs A and B of ONE shape with their expected outputs
from what the family's parity tests already trust, such that

  * any mixture of A's and B's buffers (or words) is a legal input: every index of either is in range for both, a tree of one is
    a tree over the arrays of the other;
  * expected(A) != expected(B) for every output buffer; for lists the counts differ or more than half of the records do.

A case is a builder `build(oracle, which, parameter) -> Spec` and a `run(e, p, h)`: the plain call sequence, with `p[name]` the
address of every buffer of the Spec (device memory, or host memory for the host-pointer forms) and `h` the Spec's host arguments.
`e` is the GPU test's environment: e.ok(name, *args) calls through the side-stream context and asserts VD_OK, e.opt sets a context
option for the case, e.state lives from the warm-up call to the real one (plans, prepared scenes), e.armed tells the real call from
the warm-up, e.later(fn) runs fn once the stream has drained (e.released: the handles a call has released itself), e.put(name,
array) hands back what a call wrote through a host pointer.

A call that may wait for its stream drains the delay, and whatever is called behind it in the same case runs as it would on the
null stream.  So every entry point is, in at least one case, called with nothing but enqueue-only calls in front of it
(tests/test_stream_order_cases.py holds that with a recording environment); the host-pointer forms get a delay of their own each."""
import ctypes as C
import functools

import numpy as np

import cull_occlusion_cases as K
import handoff_cases as H
import lod_cases
import mask_cases as mc
from blas_lbvh_bounded_cases import lbvh_bounded_reference
from blas_lbvh_cases import lbvh_reference
from blas_refit_cases import deform, mesh_bounds_reference, refit_reference
from chain_scenes import chain_scene
from conftest import golden
from voidin_amd import abi, synth
from wide_scenes import widen
from write_set import FILL

SEED = synth.SEED_BASE + 1300

# Entry points whose declaration promises that a call only enqueues (once the context's scratch exists), with the line of
# include/voidin_abi.h that says so.  The GPU test holds each to it: the side stream must still be busy when the call returns.
ENQUEUE_ONLY = {
    **{n: 12 for n in ("vd_cull_emit_dev", "vd_cull_emit_shard_dev", "vd_cull_compact_dev", "vd_cull_compact_shard_dev", "vd_cull_mask_dev",
                       "vd_expand_mask_dev", "vd_mask_to_indices_dev", "vd_indices_to_draws_dev", "vd_compact_draws_dev", "vd_compute_update_dev",
                       "vd_tlas_refit_dev", "vd_tlas_refit_wide_dev", "vd_primary_rays_dev", "vd_shadow_rays_dev")},
    "vd_write_value32_async": 309,
    "vd_cull_compact_views_dev": 386,
    "vd_batch_mask_dev": 473, "vd_cull_batch_dev": 473,
    "vd_bvh_build_lbvh_dev": 564,
    "vd_bvh_build_lbvh_planned_dev": 612,
    "vd_bvh_refit_planned_dev": 699,
    "vd_tlas_build_dev": 730, "vd_tlas_build_wide_dev": 730,
    "vd_tlas_build_lbvh_dev": 769, "vd_tlas_build_lbvh_wide_dev": 769,
    "vd_trace_accel_update_geometry_dev": 870,
    "vd_hiz_build_dev": 1101, "vd_occlusion_mask_dev": 1101, "vd_cull_compact_hiz_dev": 1101, "vd_cull_early_dev": 1101, "vd_cull_late_dev": 1101,
    "vd_lod_ids_dev": 1181, "vd_cull_compact_lod_dev": 1181, "vd_cull_batch_lod_dev": 1181,
}

# Entry points that must drain the context's stream before they free what a queued call still uses, with the header line that says
# so (vd_trace_release does it too, in accel_free).  Called right behind an enqueue-only call, they return with the stream idle.
RELEASE_SYNCS = {"vd_bvh_lbvh_plan_release": 619, "vd_bvh_refit_plan_release": 705}

RANKS = "Needs several ranks."                    # tests/test_gpu_rccl.py runs world = 1 on a set stream
REFUSED = "Refused by this runtime."              # the external-semaphore import
NO_DEVICE_MEMORY = "Touches no device memory."
MEMORY_WAIT = "A wait on a memory word."          # nothing may be left waiting on the device: not part of this file
ADMISSIBLE = (RANKS, REFUSED, NO_DEVICE_MEMORY, MEMORY_WAIT)
EXCLUDED = {
    **{n: NO_DEVICE_MEMORY for n in (
        "vd_ctx_create", "vd_ctx_destroy", "vd_ctx_set_stream", "vd_ctx_reset_stream", "vd_ctx_synchronize", "vd_ctx_set_option", "vd_last_error",
        "vd_version", "vd_ctx_set_timing", "vd_last_gpu_ms", "vd_last_gpu_ms_stage", "vd_bvh_last_build_stats", "vd_trace_accel_info",
        "vd_trace_accel_info_wide", "vd_hiz_layout", "vd_import_external_buffer", "vd_release_external_buffer", "vd_host_callback_async")},
    **{n: REFUSED for n in ("vd_import_external_semaphore", "vd_wait_external_semaphore_async", "vd_signal_external_semaphore_async",
                            "vd_release_external_semaphore")},
    "vd_wait_value32_async": MEMORY_WAIT,
    **{n: RANKS for n in ("vd_dist_unique_id", "vd_dist_create", "vd_dist_destroy", "vd_dist_info", "vd_dist_set_scene_dev", "vd_dist_step_full_dev",
                          "vd_dist_step_draws_dev", "vd_dist_step_indices_dev", "vd_dist_allgather_dev")},
}


# ---- what a case is made of ------------------------------------------------------------------------------------------------------

def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()


class Spec:
    """One input of a case.  dev / inout: {name: array} of device inputs and of in/out arguments (their initial contents); out:
    {name: bytes} of outputs, pre-filled with write_set.FILL; host: the host arguments; want: {name: expectation}; ranges:
    [(what, values, bound)] for every index-bearing field - all values must be < bound, and the bounds of A and B must agree."""

    def __init__(self, dev=None, inout=None, out=None, host=None, want=None, ranges=()):
        self.dev = {k: _u8(v) for k, v in (dev or {}).items()}
        self.inout = {k: _u8(v) for k, v in (inout or {}).items()}
        self.host = {k: np.ascontiguousarray(v).reshape(-1).copy() if isinstance(v, np.ndarray) else v for k, v in (host or {}).items()}   # one owner per address
        self.out, self.want, self.ranges = dict(out or {}), dict(want or {}), list(ranges)

    def shape(self):
        """Names and sizes of every buffer, and the host arguments that are counts."""
        sizes = {k: len(v) for k, v in {**self.dev, **self.inout}.items()}
        sizes.update(self.out)
        return sizes, {k: v for k, v in self.host.items() if k.startswith("n_")}


def exact(a):
    """The whole buffer."""
    return {"kind": "exact", "data": _u8(a)}


def prefix(a):
    """The first bytes of the buffer; every byte behind them keeps the fill."""
    return {"kind": "prefix", "data": _u8(a)}


def records(a, size):
    """A list of `size`-byte records at the front of the buffer, the fill behind it."""
    return {"kind": "list", "data": _u8(a), "size": size}


def hits(a, exact_dist=True):
    """VdHit records; with a private tight top level the distances are held to 1e-5 (tests/test_gpu_trace_tight.py ABS_TOL)."""
    return {"kind": "hits", "data": np.array(a, dtype=abi.HIT), "exact": exact_dist}


def lbvh_top(inst, meshes, leaves, wide):
    """An LBVH top level has no byte-level restatement: the check of tests/test_gpu_write_set.py::tlas_lbvh.  `leaves`: the exact
    builder's nodes, whose leaf boxes the array must hold in some order."""
    return {"kind": "lbvh_top", "inst": inst, "meshes": meshes, "leaves": leaves, "wide": wide}


def compare(got, w, oracle=None):
    """None, or what is wrong with the bytes `got` of a buffer against the expectation `w`."""
    got = np.ascontiguousarray(got).view(np.uint8).reshape(-1)
    kind = w["kind"]
    if kind in ("exact", "prefix", "list"):
        want = w["data"]
        if kind == "exact" and len(got) != len(want):
            return f"{len(got)} bytes, want {len(want)}"
        if len(got) < len(want):
            return f"{len(got)} bytes, want at least {len(want)}"
        d = np.flatnonzero(got[: len(want)] != want)
        if d.size:
            return f"first difference at byte {int(d[0])} of {len(want)}, {d.size} bytes differ"
        d = np.flatnonzero(got[len(want):] != FILL)
        if d.size:
            return f"byte {len(want) + int(d[0])}, behind the {len(want)} bytes of the result, was written"
        return None
    if kind == "hits":
        g, want = got.view(abi.HIT), w["data"]
        if w["exact"]:
            return None if g.tobytes() == want.tobytes() else f"record {int(np.flatnonzero(g.view(np.uint8).reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16))[0] // 16)} differs"
        if not np.array_equal(g["hit"], want["hit"]):
            return f"hit flag of ray {int(np.flatnonzero(g['hit'] != want['hit'])[0])} differs"
        hit = want["hit"] == 1
        if not np.all(np.abs(g["dist"][hit].astype(np.float64) - want["dist"][hit]) <= 1e-5) or not (g["dist"][~hit] == np.float32(1e30)).all():
            return "a distance is off by more than 1e-5"
        return None
    assert kind == "lbvh_top"
    inst, meshes, exact_nodes, n = w["inst"], w["meshes"], w["leaves"], len(w["inst"])
    dt = abi.TLAS_NODE_WIDE if w["wide"] else abi.TLAS_NODE
    if len(got) != (2 * n + 1) * dt.itemsize:
        return f"{len(got)} bytes, want {(2 * n + 1) * dt.itemsize}"
    nodes = got.view(dt)
    order = nodes["instance_idx"][1:n + 1].astype(np.int64)
    if sorted(order.tolist()) != list(range(n)):
        return "the leaves are not a permutation of the instances"
    if nodes["min"][1:n + 1].tobytes() != exact_nodes["min"][1 + order].tobytes() or nodes["max"][1:n + 1].tobytes() != exact_nodes["max"][1 + order].tobytes():
        return "a leaf box is not the exact builder's"
    left, right = H.tlas_children(nodes)
    if (left >= 2 * n + 1).any() or (right >= 2 * n + 1).any():
        return "a child index is out of range"
    seen, todo, steps = [], [0], 0
    while todo and steps <= 4 * n + 4:
        k = todo.pop(); steps += 1
        if left[k] == 0 and right[k] == 0:
            seen.append(int(nodes["instance_idx"][k]))
        else:
            todo += [int(left[k]), int(right[k])]
    if sorted(seen) != list(range(n)):
        return "node 0 does not reach every instance once"
    if oracle.tlas_refit(inst, meshes, nodes).tobytes() != nodes.tobytes():
        return "a box is not the union of its children's"
    return None


def differs(a, b):
    """Teeth: could an output that is right for A pass as right for B?  -> True when it could not."""
    kind = a["kind"]
    assert kind == b["kind"]
    if kind in ("exact", "prefix"):
        return len(a["data"]) != len(b["data"]) or a["data"].tobytes() != b["data"].tobytes()
    if kind == "list":
        if len(a["data"]) != len(b["data"]):
            return True
        ra, rb = a["data"].reshape(-1, a["size"]), b["data"].reshape(-1, a["size"])
        return len(ra) > 0 and int((ra != rb).any(axis=1).sum()) * 2 > len(ra)
    if kind == "hits":
        return bool((a["data"]["hit"] != b["data"]["hit"]).any()) and a["data"].tobytes() != b["data"].tobytes()
    n = len(a["inst"])
    boxes = lambda w: np.sort(np.concatenate([w["leaves"]["min"][1:n + 1], w["leaves"]["max"][1:n + 1]], axis=1).view(np.uint32), axis=0)
    return len(b["inst"]) != n or bool((boxes(a) != boxes(b)).any())


class Case:
    def __init__(self, build, entry_points, param, options, host):
        self.build_fn, self.entry_points, self.param, self.options, self.host, self.run_fn = build, entry_points, param, options or {}, host, None
        self.__doc__ = build.__doc__

    def build(self, oracle, which):
        return _build(self, oracle, which)

    def run(self, e, p, h):
        return self.run_fn(e, p, h)


@functools.lru_cache(maxsize=None)
def _build(c, oracle, which):
    """Computed once per input, shared by the CPU and the GPU test, never modified (the tests copy what they change)."""
    return c.build_fn(oracle, which, c.param)


CASES = {}       # case id -> Case
COVERS = {}      # entry point -> the case ids that run it


def case(*entry_points, params=(None,), options=None, host=False):
    """options: {parameter: {context option: value}}."""
    def deco(fn):
        made = []
        for prm in params:
            cid = fn.__name__ if prm is None else f"{fn.__name__}[{prm}]"
            CASES[cid] = c = Case(fn, entry_points, prm, (options or {}).get(prm, {}), host)
            made.append(c)
            for ep in entry_points:
                COVERS.setdefault(ep, []).append(cid)

        def run(rfn):
            for c in made:
                c.run_fn = rfn
            return rfn
        fn.run = run
        return fn
    return deco


def B(which):
    return which == "B"


def _cam_ptr(cam):
    return np.ascontiguousarray(cam, dtype=abi.CAMERA).reshape(-1).ctypes.data


def _count(k):
    return exact(np.array([k], np.uint32))


# ---- cull / emit -----------------------------------------------------------------------------------------------------------------

_FRONT = dict(centre=(2.0, -2.0, -10.0), extent=6.0, scale_range=(0.5, 1.0))      # a cluster the default camera sees whole


@functools.lru_cache(maxsize=None)
def cull_scene(n, which):
    """tests/test_gpu_write_set.py::_cull_scene; A: the EVEN instances sit in the cluster the camera sees, B: the ODD ones, from
    other seeds, seen from a camera moved a little and through another mesh table - visibility, mesh ids and commands all differ."""
    b = B(which)
    cam = synth.camera_uniform(eye=(2.5, 5.0, 12.5)) if b else synth.camera_uniform()
    meshes = synth.mesh_infos(16, seed=SEED + 1) if b else synth.mesh_infos()
    inst = synth.instances(n, seed=SEED + 2 if b else synth.SEED_BASE + 2, scale_range=(0.02, 0.6), extent=600.0, with_inverse=False)
    inst[int(b)::2] = synth.instances(n, seed=SEED + 3 if b else synth.SEED_BASE + 3, with_inverse=False, **_FRONT)[int(b)::2]
    inst["mesh"][n // 2 if b else n // 3] = 0xFFFFFFFF            # clamped to the last mesh
    return cam, meshes, inst


def _vis(oracle, cam, meshes, inst):
    return oracle.cull_emit(cam, meshes, inst)["instance_count"] != 0


N_CULL = 2049


@case("vd_cull_emit_dev", "vd_cull_emit_shard_dev")
def cull_emit(o, w, _):
    """n commands each."""
    cam, meshes, inst = cull_scene(N_CULL, w)
    want = o.cull_emit(cam, meshes, inst)
    shard = want.copy(); shard["base_instance"] += np.uint32(1000)
    return Spec(dev={"meshes": meshes, "instances": inst}, out={"out": N_CULL * 20, "out_shard": N_CULL * 20}, host={"cam": cam, "n_mesh": len(meshes)},
                want={"out": exact(want), "out_shard": exact(shard)})


@cull_emit.run
def _(e, p, h):
    e.ok("vd_cull_emit_dev", _cam_ptr(h["cam"]), p["meshes"], h["n_mesh"], p["instances"], N_CULL, p["out"])
    e.ok("vd_cull_emit_shard_dev", _cam_ptr(h["cam"]), p["meshes"], h["n_mesh"], p["instances"], N_CULL, 1000, p["out_shard"])


@case("vd_cull_mask_dev")
def cull_mask(o, w, _):
    """ceil(n / 64) words.  Also the end-to-end control of the GPU test."""
    cam, meshes, inst = cull_scene(N_CULL, w)
    return Spec(dev={"meshes": meshes, "instances": inst}, out={"mask": (N_CULL + 63) // 64 * 8}, host={"cam": cam, "n_mesh": len(meshes)},
                want={"mask": exact(K.pack(_vis(o, cam, meshes, inst)))})


@cull_mask.run
def _(e, p, h):
    e.ok("vd_cull_mask_dev", _cam_ptr(h["cam"]), p["meshes"], h["n_mesh"], p["instances"], N_CULL, p["mask"])


@case("vd_compact_draws_dev")
def compact_draws(o, w, _):
    """[0, count) and the count."""
    cam, meshes, inst = cull_scene(N_CULL, w)
    draws = o.cull_emit(cam, meshes, inst)
    wc, k = o.compact(draws)
    return Spec(dev={"d_in": draws}, out={"out": N_CULL * 20, "count": 4}, want={"out": records(wc[:k], 20), "count": _count(k)})


@compact_draws.run
def _(e, p, h):
    e.ok("vd_compact_draws_dev", p["d_in"], N_CULL, p["out"], p["count"])


_YAWS = (0.0, 25.0, -25.0)


@case("vd_cull_compact_dev", "vd_cull_compact_shard_dev", "vd_cull_compact_views_dev", params=["fused", "split"], options={"split": {"cull.split_min": 1}})
def cull_compact(o, w, _):
    """The list and the count, without and with pad_tail (zeroes up to n_inst); shard: base_instance + 1000; three views, stride n + 5."""
    n = N_CULL
    cam, meshes, inst = cull_scene(n, w)
    wc, k = o.compact(o.cull_emit(cam, meshes, inst))
    shard = wc[:k].copy(); shard["base_instance"] += np.uint32(1000)
    padded = np.zeros(n, abi.DRAW); padded[:k] = wc[:k]
    eye = cam["view_position"].reshape(-1)[:3]
    cams = np.stack([synth.camera_uniform(eye=tuple(float(x) for x in eye), yaw_deg=y) for y in _YAWS]).reshape(-1)
    stride = n + 5
    want = {"out": records(wc[:k], 20), "count": _count(k), "out_pad": exact(padded), "count_pad": _count(k), "out_shard": records(shard, 20), "count_shard": _count(k)}
    counts = []
    for v in range(3):
        wv, kv = o.compact(o.cull_emit(cams[v], meshes, inst))
        want[f"view{v}"] = records(wv[:kv], 20)
        counts.append(kv)
    want["counts_views"] = exact(np.array(counts, np.uint32))
    out = {"out": n * 20, "count": 4, "out_pad": n * 20, "count_pad": 4, "out_shard": n * 20, "count_shard": 4, "views": 3 * stride * 20, "counts_views": 12}
    return Spec(dev={"meshes": meshes, "instances": inst}, out=out, host={"cam": cam, "cams": cams, "n_mesh": len(meshes)}, want=want)


@cull_compact.run
def _(e, p, h):
    n, c = N_CULL, _cam_ptr(h["cam"])
    e.ok("vd_cull_compact_dev", c, p["meshes"], h["n_mesh"], p["instances"], n, p["out"], p["count"], 0)
    e.ok("vd_cull_compact_dev", c, p["meshes"], h["n_mesh"], p["instances"], n, p["out_pad"], p["count_pad"], 1)
    e.ok("vd_cull_compact_shard_dev", c, p["meshes"], h["n_mesh"], p["instances"], n, 1000, p["out_shard"], p["count_shard"], 0)
    e.ok("vd_cull_compact_views_dev", _cam_ptr(h["cams"]), 3, p["meshes"], h["n_mesh"], p["instances"], n, p["views"], n + 5, p["counts_views"], 0)


VIEWS = {"cull_compact[fused]": ("views", 3, (N_CULL + 5) * 20), "cull_compact[split]": ("views", 3, (N_CULL + 5) * 20)}   # buffers checked in slices: view<v>


N_LIST = 1024


@case("vd_mask_to_indices_dev", "vd_indices_to_draws_dev", "vd_expand_mask_dev")
def mask_wire_formats(o, w, _):
    """indices: the count and [0, count); draws: n_indices commands; expansion: [0, count) and the count.  The index list is the first
    N_LIST survivors of either input: one count for A and B."""
    n = N_CULL
    cam, meshes, inst = cull_scene(n, w)
    words = K.pack(_vis(o, cam, meshes, inst))
    ids = np.minimum(inst["mesh"], 255).astype(np.uint8)
    idx = mc.indices_reference(words, n, 7)
    k = len(idx)
    assert k >= N_LIST
    lst = (idx[:N_LIST] - np.uint32(7)).astype(np.uint32)
    wd, wk = mc.expand_reference(words, n, n, ids, meshes)
    assert wk == k
    return Spec(dev={"mask": words, "ids": ids, "meshes": meshes, "list": lst}, out={"indices": n * 4, "count": 4, "draws": N_LIST * 20, "out": n * 20, "count_x": 4},
                host={"n_mesh": len(meshes)},
                want={"indices": records(idx, 4), "count": _count(k), "draws": records(mc.draws_from_indices_reference(lst, ids, meshes), 20),
                      "out": records(wd[:k], 20), "count_x": _count(k)},
                ranges=[("index list", lst, n)])


@mask_wire_formats.run
def _(e, p, h):
    n = N_CULL
    e.ok("vd_mask_to_indices_dev", p["mask"], n, 7, p["indices"], p["count"])
    e.ok("vd_indices_to_draws_dev", p["list"], N_LIST, p["ids"], 1, n, p["meshes"], h["n_mesh"], p["draws"])
    e.ok("vd_expand_mask_dev", p["mask"], n, n, p["ids"], 1, p["meshes"], h["n_mesh"], p["out"], p["count_x"])


def regroup(vis, mesh_col, meshes):
    """(cmds, ids) of "Instanced draw lists" (tests/test_gpu_write_set.py::_regroup)."""
    n_mesh = len(meshes)
    S = np.flatnonzero(vis)
    mid = np.minimum(mesh_col, n_mesh - 1)[S].astype(np.int64)
    ids = S[np.argsort(mid, kind="stable")].astype(np.uint32)
    cnt = np.bincount(mid, minlength=n_mesh)
    cmds = np.zeros(n_mesh, abi.DRAW)
    cmds["vertex_count"], cmds["instance_count"], cmds["base_index"] = meshes["index_count"], cnt, meshes["base_index"]
    cmds["vertex_offset"], cmds["base_instance"] = meshes["vertex_offset"], np.cumsum(cnt) - cnt
    return cmds, ids


@case("vd_cull_batch_dev", "vd_batch_mask_dev")
def instanced_lists(o, w, _):
    """n_mesh commands, [0, |S|) of the ids, the count - from the instances, and from a mask with an id table."""
    n = N_CULL
    cam, meshes, inst = cull_scene(n, w)
    vis = _vis(o, cam, meshes, inst)
    cmds, ids = regroup(vis, inst["mesh"], meshes)
    want = {}
    for s in ("", "_m"):
        want.update({"cmds" + s: exact(cmds), "ids" + s: records(ids, 4), "count" + s: _count(len(ids))})
    return Spec(dev={"meshes": meshes, "instances": inst, "mask": K.pack(vis), "table": inst["mesh"].astype(np.uint32)},
                out={"cmds": len(meshes) * 20, "ids": n * 4, "count": 4, "cmds_m": len(meshes) * 20, "ids_m": n * 4, "count_m": 4},
                host={"cam": cam, "n_mesh": len(meshes)}, want=want)


@instanced_lists.run
def _(e, p, h):
    n = N_CULL
    e.ok("vd_cull_batch_dev", _cam_ptr(h["cam"]), p["meshes"], h["n_mesh"], p["instances"], n, p["cmds"], p["ids"], p["count"])
    e.ok("vd_batch_mask_dev", p["mask"], n, p["table"], 4, p["meshes"], h["n_mesh"], p["cmds_m"], p["ids_m"], p["count_m"])


# ---- occlusion -------------------------------------------------------------------------------------------------------------------

HIZ_W, HIZ_H = 4097, 3


@case("vd_hiz_build_dev")
def hiz_build(o, w, _):
    """total_texels floats."""
    depth = synth.uniform01(SEED + 44 + B(w), 0, HIZ_W * HIZ_H).reshape(HIZ_H, HIZ_W).astype(np.float32)
    want = o.hiz_build(depth)
    return Spec(dev={"depth": depth}, out={"pyramid": len(want) * 4}, want={"pyramid": exact(want)})


@hiz_build.run
def _(e, p, h):
    e.ok("vd_hiz_build_dev", p["depth"], HIZ_W, HIZ_H, p["pyramid"])


N_OCC, OCC_W, OCC_H = 5000, 100, 37


@case("vd_occlusion_mask_dev", "vd_cull_compact_hiz_dev", "vd_cull_early_dev", "vd_cull_late_dev")
def occlusion(o, w, _):
    """mask: separate and in place; the three lists with their counts; late: also d_visible_out."""
    n, b = N_OCC, B(w)
    cam, meshes = K.camera(frame=int(b)), K.meshes_for(16)
    inst = K.cloud(n, seed=SEED + 60) if b else K.cloud(n)
    pyr = o.hiz_build(K.depth(OCC_W, OCC_H, seed=SEED + 61) if b else K.depth(OCC_W, OCC_H))
    draws, F, V = K.oracle_sets(o, cam, meshes, inst, pyr, OCC_W, OCC_H)
    P = K.random_prev(n, seed=SEED + 62) if b else K.random_prev(n)
    Pb = K.bits(P, n)
    lists = {"hiz": V, "early": F & Pb, "late": V & ~Pb}
    want = {"mask_out": exact(K.pack(V)), "mask_io": exact(K.pack(V)), "visible": exact(K.pack(V))}
    out = {"mask_out": len(P) * 8, "visible": len(P) * 8}
    for name, sel in lists.items():
        lst = K.select(draws, sel)
        want["out_" + name], want["count_" + name] = records(lst, 20), _count(len(lst))
        out["out_" + name], out["count_" + name] = n * 20, 4
    return Spec(dev={"meshes": meshes, "instances": inst, "pyramid": pyr, "mask_in": K.pack(F), "prev": P}, inout={"mask_io": K.pack(F)}, out=out,
                host={"cam": cam, "n_mesh": len(meshes)}, want=want)


@occlusion.run
def _(e, p, h):
    n, c, m, k, i, w_, h_ = N_OCC, _cam_ptr(h["cam"]), p["meshes"], h["n_mesh"], p["instances"], OCC_W, OCC_H
    e.ok("vd_occlusion_mask_dev", c, m, k, i, n, p["pyramid"], w_, h_, p["mask_in"], p["mask_out"])
    e.ok("vd_occlusion_mask_dev", c, m, k, i, n, p["pyramid"], w_, h_, p["mask_io"], p["mask_io"])
    e.ok("vd_cull_compact_hiz_dev", c, m, k, i, n, p["pyramid"], w_, h_, p["out_hiz"], p["count_hiz"], 0)
    e.ok("vd_cull_early_dev", c, m, k, i, n, p["prev"], p["out_early"], p["count_early"], 0)
    e.ok("vd_cull_late_dev", c, m, k, i, n, p["pyramid"], w_, h_, p["prev"], p["visible"], p["out_late"], p["count_late"], 0)


# ---- level of detail -------------------------------------------------------------------------------------------------------------

def lod_scene(o, n, w):
    """tests/lod_cases.py's scene; B: another cloud, and the smallest 30 % of what is in the frustum dropped by min_size."""
    return lod_cases.scene(o, n, min_size_quantile=0.3, seed=SEED + 70) if B(w) else lod_cases.scene(o, n)


@case("vd_lod_ids_dev", "vd_cull_compact_lod_dev", "vd_cull_batch_lod_dev")
def level_of_detail(o, w, _):
    """n ids of 1 and 4 bytes; the list and its count; n_mesh commands, the grouped ids, the count."""
    n = N_CULL
    cam, P, base, meshes, groups, inst = lod_scene(o, n, w)
    x = lod_cases.expect(o, cam, P, base, meshes, groups, inst)
    return Spec(dev={"groups": groups, "meshes": meshes, "instances": inst},
                out={"ids1": n, "ids4": n * 4, "out": n * 20, "count": 4, "cmds": len(meshes) * 20, "ids": n * 4, "count_b": 4},
                host={"cam": cam, "P": P, "n_group": len(groups), "n_mesh": len(meshes)},
                want={"ids1": exact(x["row"].astype(np.uint8)), "ids4": exact(x["row"].astype(np.uint32)), "out": records(x["list"], 20), "count": _count(len(x["list"])),
                      "cmds": exact(x["cmds"]), "ids": records(x["ids"], 4), "count_b": _count(len(x["list"]))},
                ranges=[("first_row + n_lods", groups["first_row"].astype(np.int64) + groups["n_lods"], len(meshes) + 1)])


@level_of_detail.run
def _(e, p, h):
    n, c, lp, g, ng, m, nm, i = N_CULL, _cam_ptr(h["cam"]), abi.lod_params(h["P"]), p["groups"], h["n_group"], p["meshes"], h["n_mesh"], p["instances"]
    e.ok("vd_lod_ids_dev", c, lp, g, ng, nm, i, n, p["ids1"], 1)
    e.ok("vd_lod_ids_dev", c, lp, g, ng, nm, i, n, p["ids4"], 4)
    e.ok("vd_cull_compact_lod_dev", c, lp, g, ng, m, nm, i, n, p["out"], p["count"], 0)
    e.ok("vd_cull_batch_lod_dev", c, lp, g, ng, m, nm, i, n, p["cmds"], p["ids"], p["count_b"])


# ---- BLAS ------------------------------------------------------------------------------------------------------------------------

def _mesh(name, w):
    """handoff_cases.mesh(name), and for B its other mesh of the same counts; a soup's index buffer counts 0, 1, 2, ... for every
    seed, so B lists its triangles last to first: the bytes differ even where a build leaves the order alone."""
    v, i = H.mesh(name + "*" if B(w) else name)
    v, i = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(i, dtype=np.uint32).reshape(-1)
    return (v, np.ascontiguousarray(i.reshape(-1, 3)[::-1]).reshape(-1)) if B(w) and name.startswith("soup") else (v, i)


SPARE = 37                                   # nodes of capacity nobody may write (tests/test_gpu_write_set.py)
# The builder starts mid-tier roots on the context's SECOND stream (launch_mid_early, blas.hip) when, after a level of the level
# loop that leaves segments behind, at least kMidEarlyMin = 256 new roots of 513 .. 2048 triangles are listed.  One mesh alone needs
# more than 256 * 513 = 131 328 triangles for that: none of handoff_cases.BUILD_MESHES (the largest, knot32k, has 32 768) gets there,
# and the oracle takes tens of seconds for one that does.  The batch reaches it at once: its meshes of 513 .. 2048 triangles are listed
# as mid-tier roots before the first level, so 256 of them beside ONE mesh that the level loop has to split twice (soup9000, the
# smallest of BUILD_MESHES with two levels) start on the second stream after level 0: sah_batch[second stream].
BUILD_MESH = "knot32k"
SECOND_STREAM_MESH, N_MID, T_MID = "soup9000", 256, 513


@case("vd_bvh_build_dev", params=[BUILD_MESH])
def sah_build(o, w, name):
    """nodes [0, n_nodes), the permuted indices, the host's n_nodes word."""
    v, i = _mesh(name, w)
    wn, wi = o.bvh_build(v, i)
    T = len(i) // 3
    return Spec(dev={"verts": v}, inout={"indices": i}, out={"nodes": (2 * T + SPARE) * 32}, host={"n_vert": len(v), "n_tri": T},
                want={"nodes": prefix(wn), "indices": exact(wi), "host:n_nodes": _count(len(wn))}, ranges=[("vertex index", i, len(v))])


@sah_build.run
def _(e, p, h):
    nn = C.c_uint32(0xEEEEEEEE)
    e.ok("vd_bvh_build_dev", p["verts"], h["n_vert"], p["indices"], h["n_tri"], p["nodes"], 2 * h["n_tri"] + SPARE, C.addressof(nn))
    e.put("host:n_nodes", np.array([nn.value], np.uint32))


BATCH_MESHES = ("soup3", "soup513", "soup2049")


@case("vd_bvh_build_batch_dev", params=["own", "packed"])
def sah_batch(o, w, form):
    """Three meshes: own node arrays, or packed behind 11 nodes of one array; of the items the three written fields."""
    meshes = [_mesh(m, w) for m in BATCH_MESHES]
    want, dev, inout, out, ranges = {}, {}, {}, {}, []
    at, first, fields = 11, [], []
    for m, (v, i) in enumerate(meshes):
        wn, wi = o.bvh_build(v, i)
        dev[f"verts{m}"], inout[f"indices{m}"] = v, i
        want[f"indices{m}"] = exact(wi)
        ranges.append((f"vertex index of mesh {m}", i, len(v)))
        if form == "own":
            out[f"nodes{m}"] = (len(i) // 3 * 2 + SPARE) * 32
            want[f"nodes{m}"] = prefix(wn)
            fields += [len(wn), 0, 0]
        else:
            first.append(wn)
            fields += [len(wn), at, 0]
            at += len(wn)
    if form == "packed":
        out["packed"] = (11 + sum(2 * (len(i) // 3) for _, i in meshes) + SPARE) * 32
        want["packed:fill"], want["packed:from 11"] = prefix(np.zeros(0, np.uint8)), prefix(np.concatenate(first))
        want["host:end"] = _count(at)
    want["host:items"] = exact(np.array(fields, np.int64))
    return Spec(dev=dev, inout=inout, out=out, host={"n_vert": [len(v) for v, _ in meshes], "n_tri": [len(i) // 3 for _, i in meshes], "form": form}, want=want, ranges=ranges)


@sah_batch.run
def _(e, p, h):
    K_, own = len(BATCH_MESHES), h["form"] == "own"
    items = (abi.BvhBatchItem * K_)()
    for m in range(K_):
        items[m].verts_xyz, items[m].indices_inout, items[m].out_nodes = p[f"verts{m}"], p[f"indices{m}"], p[f"nodes{m}"] if own else None
        items[m].n_vert, items[m].n_tri, items[m].node_cap = h["n_vert"][m], h["n_tri"][m], 2 * h["n_tri"][m] + SPARE if own else 0
        items[m].out_n_nodes, items[m].out_first_node, items[m].status = 0xEEEEEEEE, 0xEEEEEEEE, -99
    end = C.c_uint32(0xEEEEEEEE)
    pcap = 11 + sum(2 * t for t in h["n_tri"]) + SPARE
    e.ok("vd_bvh_build_batch_dev", C.addressof(items), K_, None if own else p["packed"], 0 if own else pcap, 0 if own else 11, C.addressof(end))
    e.put("host:items", np.array([x for m in range(K_) for x in (items[m].out_n_nodes, 0 if own else items[m].out_first_node, items[m].status)], np.int64))
    if not own:
        e.put("host:end", np.array([end.value], np.uint32))


@case("vd_bvh_build_batch_dev", params=["second stream"])
def sah_batch_second_stream(o, w, _):
    """N_MID meshes of T_MID triangles - consecutive chunks of one soup, in one vertex, one index and one packed node buffer - and
    SECOND_STREAM_MESH: the mid tier of the small ones runs on the context's second stream beside the level loop of the large one."""
    v, i = H.mesh(f"soup{N_MID * T_MID}" + ("*" if B(w) else ""))
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(N_MID, 3 * T_MID, 3)
    local = np.arange(3 * T_MID, dtype=np.uint32) if not B(w) else np.ascontiguousarray(np.arange(3 * T_MID, dtype=np.uint32).reshape(-1, 3)[::-1]).reshape(-1)
    vb, ib = _mesh(SECOND_STREAM_MESH, w)
    nodes, idx, fields, at = [], [], [], 0
    for m in range(N_MID + 1):
        wn, wi = o.bvh_build(v[m], local) if m < N_MID else o.bvh_build(vb, ib)
        nodes.append(wn); idx.append(wi); fields += [len(wn), at, 0]; at += len(wn)
    cap = 2 * (N_MID * T_MID + len(ib) // 3) + SPARE
    return Spec(dev={"verts": v, "verts_big": vb}, inout={"indices": np.tile(local, N_MID), "indices_big": ib}, out={"packed0": cap * 32},
                host={"n_vert_big": len(vb), "n_tri_big": len(ib) // 3},
                want={"packed0": prefix(np.concatenate(nodes)), "indices": exact(np.concatenate(idx[:-1])), "indices_big": exact(idx[-1]), "host:end": _count(at),
                      "host:items": exact(np.array(fields, np.int64))}, ranges=[("vertex index", local, 3 * T_MID), ("vertex index of the large mesh", ib, len(vb))])


@sah_batch_second_stream.run
def _(e, p, h):
    items = (abi.BvhBatchItem * (N_MID + 1))()
    for m in range(N_MID + 1):
        big = m == N_MID
        items[m].verts_xyz, items[m].indices_inout, items[m].out_nodes = (p["verts_big"], p["indices_big"], None) if big else (p["verts"] + m * 3 * T_MID * 12, p["indices"] + m * 3 * T_MID * 4, None)
        items[m].n_vert, items[m].n_tri, items[m].node_cap = (h["n_vert_big"], h["n_tri_big"], 0) if big else (3 * T_MID, T_MID, 0)
        items[m].out_n_nodes, items[m].out_first_node, items[m].status = 0xEEEEEEEE, 0xEEEEEEEE, -99
    end = C.c_uint32(0xEEEEEEEE)
    e.ok("vd_bvh_build_batch_dev", C.addressof(items), N_MID + 1, p["packed0"], 2 * (N_MID * T_MID + h["n_tri_big"]) + SPARE, 0, C.addressof(end))
    e.put("host:items", np.array([x for m in range(N_MID + 1) for x in (items[m].out_n_nodes, items[m].out_first_node, items[m].status)], np.int64))
    e.put("host:end", np.array([end.value], np.uint32))
    e.put("stats", e.build_stats())                  # the GPU test holds n_mid_roots and levels_phase_a against the rule above


N_LBVH = 2049


@case("vd_bvh_build_lbvh_dev", params=["unbounded", "depth 12"], options={"depth 12": {"blas.lbvh_max_depth": 12}})
def lbvh_build(o, w, form):
    """nodes [0, n_nodes), the permuted indices, the 16 bytes of d_result."""
    v, i = _mesh(f"soup{N_LBVH}", w)
    ref = lbvh_reference(v, i) if form == "unbounded" else lbvh_bounded_reference(v, i, 12)
    res = np.array([(ref["n_nodes"], ref["n_bad_indices"], ref["max_depth"], 0)], dtype=abi.BVH_LBVH_RESULT)
    return Spec(dev={"verts": v}, inout={"indices": i}, out={"nodes": (2 * N_LBVH + SPARE) * 32, "result": 16}, host={"n_vert": len(v)},
                want={"nodes": prefix(ref["nodes"][: ref["n_nodes"]]), "indices": exact(ref["indices"]), "result": exact(res)}, ranges=[("vertex index", i, len(v))])


@lbvh_build.run
def _(e, p, h):
    e.ok("vd_bvh_build_lbvh_dev", p["verts"], h["n_vert"], p["indices"], N_LBVH, p["nodes"], 2 * N_LBVH + SPARE, p["result"])


PLAN_CAPS = (65, 513, 4)
PLAN_COUNTS = {"A": (65, 100, 0), "B": (30, 513, 4)}


def _info(seed):
    info = np.zeros(1, dtype=abi.MESH_INFO)
    info["min"], info["max"], info["index_count"], info["base_index"], info["vertex_offset"], info["bvh_index"], info["junk"] = 77.0 + seed, -77.0 - seed, 9, 11, 22, 33, (44, 55)
    return info


def _with_bounds(info, v):
    out = info.copy()
    out["min"][0], out["max"][0] = mesh_bounds_reference(v)
    return out


@case("vd_bvh_lbvh_plan_dev", "vd_bvh_build_lbvh_planned_dev", "vd_bvh_lbvh_plan_release", params=["planned", "plan, then planned"])
def lbvh_planned(o, w, form):
    """Three meshes, the counts in device memory: per mesh nodes [0, n_nodes), the first 3 T indices, the result records; min / max
    of the second mesh's mesh_info.  planned: the plan is made by the warm-up call and reused; the other form plans in the call."""
    meshes = [_mesh(f"soup{c}", w) for c in PLAN_CAPS]
    counts = np.array(PLAN_COUNTS[w], np.uint32)
    dev, inout, out, want, ranges = {"counts": counts}, {"info": _info(int(B(w)))}, {"results": 16 * len(meshes)}, {}, []
    results = np.zeros(len(meshes), dtype=abi.BVH_LBVH_RESULT)
    for m, (v, i) in enumerate(meshes):
        T = int(counts[m])
        dev[f"verts{m}"], inout[f"indices{m}"], out[f"nodes{m}"] = v, i, (2 * PLAN_CAPS[m] + SPARE) * 32
        ranges.append((f"vertex index of mesh {m}", i, len(v)))
        if T == 0:
            want[f"nodes{m}"], want[f"indices{m}"] = prefix(np.zeros(0, np.uint8)), exact(i)
            continue
        ref = lbvh_reference(v, i[: 3 * T])
        results[m] = (ref["n_nodes"], 0, ref["max_depth"], 0)
        want[f"nodes{m}"], want[f"indices{m}"] = prefix(ref["nodes"][: ref["n_nodes"]]), exact(np.concatenate([ref["indices"], i[3 * T:]]))
    want["results"], want["info"] = exact(results), exact(_with_bounds(inout["info"], meshes[1][0]))
    ranges.append(("count, read as the capacity when above it", np.minimum(counts, PLAN_CAPS), max(PLAN_CAPS) + 1))
    return Spec(dev=dev, inout=inout, out=out, host={"n_vert": [len(v) for v, _ in meshes], "form": form}, want=want, ranges=ranges)


@lbvh_planned.run
def _(e, p, h):
    if "plan" not in e.state or h["form"] != "planned":
        items = (abi.BvhLbvhBatchItem * len(PLAN_CAPS))()
        for m, cap in enumerate(PLAN_CAPS):
            items[m].verts_xyz, items[m].indices_inout, items[m].nodes = p[f"verts{m}"], p[f"indices{m}"], p[f"nodes{m}"]
            items[m].mesh_info = p["info"] if m == 1 else None
            items[m].n_vert, items[m].tri_cap, items[m].node_cap = h["n_vert"][m], cap, 2 * cap + SPARE
        plan = C.c_void_p()
        e.ok("vd_bvh_lbvh_plan_dev", C.addressof(items), len(PLAN_CAPS), C.byref(plan))
        e.later(lambda: plan.value in e.released or e.ok("vd_bvh_lbvh_plan_release", plan))
        e.state["plan"] = plan
    e.ok("vd_bvh_build_lbvh_planned_dev", e.state["plan"], p["counts"], p["results"])
    if h["form"] == "planned" and e.armed:                        # the release finds the build queued behind the delay, and waits for it
        e.ok("vd_bvh_lbvh_plan_release", e.state["plan"])
        e.released.add(e.state["plan"].value)


def swapped_children(nodes):
    """The same tree with the two children of every interior node in each other's slots: same counts, every child id still above its
    parent's, other parents and other leaf ids - ANOTHER valid topology over the same arrays."""
    out = np.array(nodes, copy=True)
    reach = np.zeros(len(nodes), dtype=bool)
    reach[0] = True
    for k in range(len(nodes)):                                   # parents come first; the reserved slot 1 is not reached
        if reach[k] and nodes["count"][k] == 0:
            l = int(nodes["left_first"][k])
            reach[l] = reach[l + 1] = True
            out[l], out[l + 1] = nodes[l + 1], nodes[l]
    return out


N_REFIT = 2049


@case("vd_bvh_refit_plan_dev", "vd_bvh_refit_planned_dev", "vd_bvh_refit_plan_release", params=["planned", "plan, then planned"])
def blas_refit(o, w, form):
    """min / max of every node and of the mesh_info.  planned: the plan is made by the warm-up call, B is A's topology over moved
    vertices; plan, then planned: B is the tree with every pair of children swapped - a plan made from stale nodes climbs A's links."""
    v, i = _mesh(f"soup{N_REFIT}", "A")
    nodes, idx = o.bvh_build(v, i)
    v2 = deform(v, phase=0.9 if B(w) else 0.4, specials=False)
    if B(w):
        nodes = refit_reference(deform(v, phase=0.2, specials=False), idx, swapped_children(nodes) if form != "planned" else nodes)
    info = _info(int(B(w)))
    leaf = nodes["count"] > 0
    return Spec(dev={"verts": v2, "indices": idx}, inout={"nodes": nodes, "info": info}, host={"n_vert": len(v2), "n_nodes": len(nodes), "form": form},
                want={"nodes": exact(refit_reference(v2, idx, nodes)), "info": exact(_with_bounds(info, v2))},
                ranges=[("vertex index", idx, len(v2)), ("leaf range", (nodes["left_first"].astype(np.int64) + nodes["count"])[leaf], N_REFIT + 1),
                        ("child pair", nodes["left_first"][~leaf].astype(np.int64) + 1, len(nodes))])


@blas_refit.run
def _(e, p, h):
    if "plan" not in e.state or h["form"] != "planned":
        items = (abi.BvhRefitItem * 1)()
        items[0].verts_xyz, items[0].indices, items[0].nodes, items[0].mesh_info = p["verts"], p["indices"], p["nodes"], p["info"]
        items[0].n_vert, items[0].n_tri, items[0].n_nodes = h["n_vert"], N_REFIT, h["n_nodes"]
        plan = C.c_void_p()
        e.ok("vd_bvh_refit_plan_dev", C.addressof(items), 1, C.byref(plan))
        e.later(lambda: plan.value in e.released or e.ok("vd_bvh_refit_plan_release", plan))
        e.state["plan"] = plan
    e.ok("vd_bvh_refit_planned_dev", e.state["plan"])
    if h["form"] == "planned" and e.armed:                        # the release finds the refit queued behind the delay, and waits for it
        e.ok("vd_bvh_refit_plan_release", e.state["plan"])
        e.released.add(e.state["plan"].value)


# ---- TLAS ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tlas_scene(n, which, seed=50):
    """tests/test_gpu_write_set.py::_tlas_scene, and for B every instance of it moved and rescaled, under another mesh table."""
    a = synth.instances(n, seed=synth.SEED_BASE + seed + n % 97, extent=120.0)
    return (H.moved(a), synth.mesh_infos(16, seed=SEED + 1)) if B(which) else (a, synth.mesh_infos())


# The chain shared by 16 workgroups (a memset of its exchange words, tlas_build_mw_kernel, two conditional redo launches) starts by
# itself at 12 288 instances, where the oracle's sequential chain takes 8 s per input.  VD_OPT_TLAS_GROUPS selects it at any n: the
# kernel deals slot PAIRS to the workgroups (a workgroup whose share is empty scans nothing), reads at most slot cnt <= n < cap, its
# exchanged slot field holds 20 bits, and every spin is bounded, with the redo on one workgroup behind it - so n = 1000 is a valid
# input of that path; tlas.spin_limit = 0 forces the redo, as tests/test_gpu_write_set.py does at 12 288.
TLAS_PATHS = {"plain": (1000, {}), "chain from memory": (700, {"tlas.chain_lds": 0}),
              "indexed": (257, {"tlas.index_min": 65, "tlas.phase2": 64, "tlas.refresh": 37}),
              "several workgroups": (1000, {"tlas.groups": 16}),
              "several workgroups, redone on one": (1000, {"tlas.groups": 16, "tlas.spin_limit": 0})}


@case("vd_tlas_build_dev", "vd_tlas_build_wide_dev", params=list(TLAS_PATHS), options={k: v[1] for k, v in TLAS_PATHS.items()})
def tlas_build(o, w, path):
    """(2n + 1) nodes of 32 and of 48 bytes."""
    n = TLAS_PATHS[path][0]
    inst, meshes = tlas_scene(n, w)
    want = o.tlas_build(inst, meshes)
    return Spec(dev={"instances": inst, "meshes": meshes}, out={"nodes": (2 * n + 1) * 32, "wide": (2 * n + 1) * 48}, host={"n": n, "n_mesh": len(meshes)},
                want={"nodes": exact(want), "wide": exact(widen(want))})


@tlas_build.run
def _(e, p, h):
    e.ok("vd_tlas_build_dev", p["instances"], h["n"], p["meshes"], h["n_mesh"], p["nodes"])
    e.ok("vd_tlas_build_wide_dev", p["instances"], h["n"], p["meshes"], h["n_mesh"], p["wide"])


N_TLAS = 1000


def _nudged(inst):
    out = inst.copy()
    out["transform"][::3, 12:15] += np.float32(0.37)
    return out


@case("vd_tlas_refit_dev", "vd_tlas_refit_wide_dev")
def tlas_refit(o, w, _):
    """The same nodes in place.  B's tree is the exact builder's over B's instances: another topology of the same counts."""
    inst, meshes = tlas_scene(N_TLAS, w)
    built, now = o.tlas_build(inst, meshes), _nudged(inst)
    l, r = H.tlas_children(built)
    return Spec(dev={"instances": now, "meshes": meshes}, inout={"nodes": built, "wide": widen(built)}, host={"n_mesh": len(meshes)},
                want={"nodes": exact(o.tlas_refit(now, meshes, built)), "wide": exact(o.tlas_refit(now, meshes, widen(built)))},
                ranges=[("child", np.concatenate([l, r]), 2 * N_TLAS + 1), ("instance of a leaf", built["instance_idx"][1:N_TLAS + 1], N_TLAS)])


@tlas_refit.run
def _(e, p, h):
    e.ok("vd_tlas_refit_dev", p["instances"], N_TLAS, p["meshes"], h["n_mesh"], p["nodes"])
    e.ok("vd_tlas_refit_wide_dev", p["instances"], N_TLAS, p["meshes"], h["n_mesh"], p["wide"])


@case("vd_tlas_build_lbvh_dev", "vd_tlas_build_lbvh_wide_dev")
def tlas_lbvh(o, w, _):
    """(2n + 1) nodes of 32 and of 48 bytes, held against the header's layout."""
    inst, meshes = tlas_scene(N_TLAS, w)
    leaves = o.tlas_build(inst, meshes)
    return Spec(dev={"instances": inst, "meshes": meshes}, out={"nodes": (2 * N_TLAS + 1) * 32, "wide": (2 * N_TLAS + 1) * 48}, host={"n_mesh": len(meshes)},
                want={"nodes": lbvh_top(inst, meshes, leaves, False), "wide": lbvh_top(inst, meshes, leaves, True)})


@tlas_lbvh.run
def _(e, p, h):
    e.ok("vd_tlas_build_lbvh_dev", p["instances"], N_TLAS, p["meshes"], h["n_mesh"], p["nodes"])
    e.ok("vd_tlas_build_lbvh_wide_dev", p["instances"], N_TLAS, p["meshes"], h["n_mesh"], p["wide"])


# ---- trace -----------------------------------------------------------------------------------------------------------------------

SCENE_NAMES = ("tlas_nodes", "instances", "meshes", "bvh_nodes", "vertices", "indices")
N_RAYS = 4097


@functools.lru_cache(maxsize=None)
def trace_scene(oracle, which):
    """A: tests/golden/trace_40.npz with hits and misses alternating (tests/test_gpu_write_set.py::_trace40).  B: the same 40
    instances moved and rescaled, the top level refitted to them (A's topology), every mesh twice as large - vertices, BLAS boxes
    and mesh bounds times two, exactly - and the rays from the other side.  Same counts, same index ranges, other hits."""
    g = golden("trace_40.npz")
    scene = [g["tlas"], g["instances"], g["meshes"], g["bvh_nodes"], np.ascontiguousarray(g["vertices"], dtype=np.float32), g["indices"]]
    hit, miss = np.flatnonzero(g["hit"] == 1), np.flatnonzero(g["hit"] == 0)
    k = min(len(hit), len(miss))
    rays = g["rays"][np.concatenate([np.stack([hit[:k], miss[:k]], axis=1).reshape(-1), hit[k:], miss[k:]])]
    if B(which):
        inst, meshes, nodes = H.moved(scene[1]), scene[2].copy(), scene[3].copy()
        for a in (meshes, nodes):
            a["min"] *= np.float32(2.0); a["max"] *= np.float32(2.0)
        scene = [oracle.tlas_refit(inst, meshes, scene[0]), inst, meshes, nodes, scene[4] * np.float32(2.0), scene[5]]
        rays = rays[::-1].copy()
        rays["eye"] += np.float32(0.25)
    return tuple(scene), np.resize(rays, N_RAYS)


N_DEEP, N_DEEP_RAYS = 123, 65


@functools.lru_cache(maxsize=None)
def deep_scene(oracle, which):
    """tests/test_gpu_write_set.py's scene for the global-memory stack pass: chain_scene of 123 leaves, the shortest chain past a
    lane's 128 entries, five rays down the chain and three past it.  B: the whole scene twice as large - translations, vertices and
    every box times two, exactly - the rays from twice as far and dealt in another order: same depths, other distances, other flags."""
    tl, inst, infos, nodes, v, idx = chain_scene(oracle, N_DEEP)
    pool = np.zeros(8, dtype=abi.RAY)
    pool["eye"], pool["dir"] = (-5.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    pool["eye"][:, 1] = np.linspace(-0.2, 0.2, 8, dtype=np.float32)
    pool["dir"][5:] = (0.0, 1.0, 0.0)
    if B(which):
        two = np.float32(2.0)
        tl, inst, infos, nodes = tl.copy(), inst.copy(), infos.copy(), nodes.copy()
        for a in (tl, infos, nodes):
            a["min"] *= two; a["max"] *= two
        inst["transform"][:, 12:15] *= two; inst["inv_transform"][:, 12:15] *= two
        v = v * two
        pool["eye"] *= two
        pool = np.roll(pool, 3)
    scene = (tl, inst, infos, nodes, v, idx)
    assert int(oracle.trace(scene, pool, depths=True)[2].max()) > 128          # the oracle's shared far-only depth: the unit of the header's 128
    return scene, np.resize(pool, N_DEEP_RAYS)


def _scene_ranges(scene):
    tl, inst, meshes, nodes, verts, idx = scene
    n = len(inst)
    l, r = H.tlas_children(tl)
    leaf = nodes["count"] > 0
    return [("top-level child", np.concatenate([l, r]), len(tl)), ("instance of a leaf", tl["instance_idx"][(l == 0) & (r == 0)], n),
            ("mesh of an instance", inst["mesh"], len(meshes)), ("BLAS root", meshes["bvh_index"], len(nodes)),
            ("mesh-local vertex index", idx.reshape(-1), len(verts.reshape(-1, 3))), ("mesh-local leaf range", (nodes["left_first"].astype(np.int64) + nodes["count"])[leaf], len(idx.reshape(-1)) // 3 + 1),
            ("child pair", nodes["left_first"][~leaf].astype(np.int64) + 1, len(nodes) + 1)]


def _scene_struct(p, h, wide):
    s = abi.TraceSceneWide() if wide else abi.TraceScene()
    for name in SCENE_NAMES:
        setattr(s, name, p["tlas_wide" if wide and name == "tlas_nodes" else name])
        setattr(s, "n_" + name, h["n_" + name])
    return s


def _trace_spec(o, w, tight=0, deep=False):
    scene, rays = deep_scene(o, w) if deep else trace_scene(o, w)
    want, _ = o.trace(scene, rays)
    dts = [abi.TLAS_NODE, abi.INSTANCE, abi.MESH_INFO, abi.BVH_NODE, np.float32, np.uint32]
    dev = {name: np.ascontiguousarray(a, dtype=d).reshape(-1) for name, a, d in zip(SCENE_NAMES, scene, dts)}
    host = {"n_" + name: len(a) // (3 if name == "vertices" else 1) for name, a in dev.items()}
    dev["tlas_wide"], dev["rays"], host["n_rays"] = widen(scene[0]), rays, len(rays)
    return Spec(dev=dev, out={"hits": len(rays) * 16, "flags": len(rays) * 4}, host=host,
                want={"hits": hits(want, tight == 0), "flags": exact(want["hit"].astype(np.uint32))}, ranges=_scene_ranges(scene))


TRACE_FORMS = {"plain": {}, "plain, auto_prepare 0": {"trace.auto_prepare": 0}, "plain, one launch": {"trace.fan": 1}, "wide": {}, "wide, auto_prepare 0": {"trace.auto_prepare": 0},
               "plain, any first": {}, "wide, any first": {}}      # the walks block: whichever comes second finds the stream drained, so each gets to be first


@case("vd_trace_dev", "vd_trace_any_dev", "vd_trace_wide_dev", "vd_trace_any_wide_dev", params=list(TRACE_FORMS), options=TRACE_FORMS)
def trace(o, w, form):
    """n_rays records of 16 bytes and n_rays flags."""
    s = _trace_spec(o, w)
    s.host["wide"], s.host["any_first"] = form.startswith("wide"), form.endswith("any first")
    return s


@trace.run
def _(e, p, h):
    s = _scene_struct(p, h, h["wide"])
    calls = [("vd_trace_wide_dev" if h["wide"] else "vd_trace_dev", "hits"), ("vd_trace_any_wide_dev" if h["wide"] else "vd_trace_any_dev", "flags")]
    for name, out in calls[::-1] if h["any_first"] else calls:
        e.ok(name, C.byref(s), p["rays"], h["n_rays"], p[out])


@case("vd_trace_dev", "vd_trace_any_dev", "vd_trace_prepare_dev", "vd_trace_prepared_dev", "vd_trace_any_prepared_dev", "vd_trace_release", params=["plain", "prepared"])
def trace_deep(o, w, form):
    """The second pass, whose stack goes on in global memory: records and flags of 65 rays over the 123-leaf chain."""
    s = _trace_spec(o, w, deep=True)
    s.host["form"] = form
    return s


@trace_deep.run
def _(e, p, h):
    if h["form"] == "plain":
        s = _scene_struct(p, h, False)
        e.ok("vd_trace_dev", C.byref(s), p["rays"], h["n_rays"], p["hits"])
        e.ok("vd_trace_any_dev", C.byref(s), p["rays"], h["n_rays"], p["flags"])
    else:
        acc = _prepare(e, p, h, False, 0)
        e.ok("vd_trace_prepared_dev", acc, p["rays"], h["n_rays"], p["hits"])
        e.ok("vd_trace_any_prepared_dev", acc, p["rays"], h["n_rays"], p["flags"])


PREPARED_FORMS = {"narrow": (False, 0), "narrow, tight 1": (False, 1), "narrow, tight 2": (False, 2), "wide": (True, 0), "wide, tight": (True, 2)}


def _prepare(e, p, h, wide, tight):
    s, acc = _scene_struct(p, h, wide), C.c_void_p()
    e.opt("trace.tight_tlas", tight)
    e.ok("vd_trace_prepare_wide_dev" if wide else "vd_trace_prepare_dev", C.byref(s), C.byref(acc))
    e.opt("trace.tight_tlas", 0)
    e.later(lambda: acc.value in e.released or e.ok("vd_trace_release", acc))
    return acc


@case("vd_trace_prepare_dev", "vd_trace_prepare_wide_dev", "vd_trace_prepared_dev", "vd_trace_any_prepared_dev", "vd_trace_release", params=list(PREPARED_FORMS))
def trace_prepared(o, w, form):
    """Prepare, then both prepared walks: the prepare's validation and its private top level read the scene as the stream has it."""
    s = _trace_spec(o, w, PREPARED_FORMS[form][1])
    s.host["wide"], s.host["tight"] = PREPARED_FORMS[form]
    return s


@trace_prepared.run
def _(e, p, h):
    acc = _prepare(e, p, h, h["wide"], h["tight"])
    e.ok("vd_trace_prepared_dev", acc, p["rays"], h["n_rays"], p["hits"])
    e.ok("vd_trace_any_prepared_dev", acc, p["rays"], h["n_rays"], p["flags"])


MAINTENANCE = {"update_geometry": (False, 0), "update_geometry, any first": (False, 0), "update_geometry, release, prepare": (False, 0), "update, tight 1": (False, 1), "update, tight 2": (False, 2), "refit, tight 1": (False, 1), "refit, tight 2": (False, 2),
               "update, wide": (True, 2), "refit, wide": (True, 2)}


@case("vd_trace_accel_update_dev", "vd_trace_accel_refit_dev", "vd_trace_accel_update_geometry_dev", "vd_trace_prepare_dev", "vd_trace_prepare_wide_dev",
      "vd_trace_prepared_dev", "vd_trace_any_prepared_dev", "vd_trace_release", params=list(MAINTENANCE))
def trace_accel_maintenance(o, w, form):
    """The accel is prepared by the warm-up call over A; the call brings it up to B - the triangles with update_geometry, then
    the private top level with update or refit - and walks it."""
    s = _trace_spec(o, w, MAINTENANCE[form][1])
    s.host["wide"], s.host["tight"], s.host["form"] = MAINTENANCE[form] + (form,)
    return s


@trace_accel_maintenance.run
def _(e, p, h):
    if "acc" not in e.state:
        e.state["acc"] = _prepare(e, p, h, h["wide"], h["tight"])
    acc = e.state["acc"]
    e.ok("vd_trace_accel_update_geometry_dev", acc)
    if h["form"].startswith("update,"):
        e.ok("vd_trace_accel_update_dev", acc)
    elif h["form"].startswith("refit"):
        e.ok("vd_trace_accel_refit_dev", acc)
    elif h["form"].endswith("release, prepare") and e.armed:      # the release finds the update queued behind the delay, and waits for it
        e.ok("vd_trace_release", acc)
        e.released.add(acc.value)
        acc = e.state["acc"] = _prepare(e, p, h, h["wide"], h["tight"])
    calls = [("vd_trace_prepared_dev", "hits"), ("vd_trace_any_prepared_dev", "flags")]
    for name, out in calls[::-1] if h["form"].endswith("any first") else calls:
        e.ok(name, acc, p["rays"], h["n_rays"], p[out])


# ---- ray generators and the one-mesh walks ---------------------------------------------------------------------------------------

RAYS_W, RAYS_H = 65, 1


@case("vd_primary_rays_dev")
def primary_rays(o, w, _):
    """width * height rays.  No device input: a launch ahead of its place shows as a result where the fill should still be."""
    cam = synth.camera_uniform(eye=(1, 2, 14), pitch_deg=-5) if B(w) else synth.camera_uniform(eye=(0, 0, 15), pitch_deg=0)
    return Spec(out={"rays": RAYS_W * RAYS_H * 32}, host={"cam": cam}, want={"rays": exact(o.primary_rays(cam, RAYS_W, RAYS_H))})


@primary_rays.run
def _(e, p, h):
    e.ok("vd_primary_rays_dev", _cam_ptr(h["cam"]), RAYS_W, RAYS_H, p["rays"])


N_WALK = 257


@case("vd_shadow_rays_dev")
def shadow_rays(o, w, _):
    """32 bytes per point."""
    n = N_WALK
    u = synth.uniform01(SEED + 33 + B(w), 0, 6 * n).reshape(n, 6).astype(np.float32)
    pos, nor = np.ascontiguousarray(u[:, :3] * 10), np.ascontiguousarray(u[:, 3:] - np.float32(0.5))
    light = np.array([-5.0, 30.0, 25.0] if B(w) else [3.0, 40.0, 20.0], np.float32)
    return Spec(dev={"positions": pos, "normals": nor}, out={"rays": n * 32}, host={"light": light}, want={"rays": exact(o.shadow_rays(pos, nor, light))})


@shadow_rays.run
def _(e, p, h):
    e.ok("vd_shadow_rays_dev", p["positions"], p["normals"], N_WALK, h["light"].ctypes.data_as(C.POINTER(C.c_float)), p["rays"])


@case("vd_traverse_iter_dev", "vd_traverse_dev", params=["iterative first", "recursive first"])
def one_mesh_walks(o, w, order):
    """4 bytes per ray.  B: the mesh of tests/golden/harness_soup64.npz twice as large (vertices and boxes times two, exactly), the rays
    from twice as far: every hit distance doubles."""
    g = golden("harness_soup64.npz")
    nodes, v, idx = g["nodes"].copy(), g["vertices"].astype(np.float32), g["indices"].astype(np.uint32)
    hit, miss = np.flatnonzero(g["dist"] >= 0), np.flatnonzero(g["dist"] < 0)          # few rays of the fixture hit: they alternate with misses
    rays = np.resize(g["rays"][np.stack([hit, miss[: len(hit)]], axis=1).reshape(-1)], N_WALK)
    t0 = 14.0
    if B(w):
        nodes["min"] *= np.float32(2.0); nodes["max"] *= np.float32(2.0)
        v = v * np.float32(2.0)
        rays = rays.copy(); rays["eye"] *= np.float32(2.0)
        t0 = 29.0
    leaf = nodes["count"] > 0
    return Spec(dev={"nodes": nodes, "verts": v, "indices": idx, "rays": rays}, out={"iter": N_WALK * 4, "rec": N_WALK * 4}, host={"n_nodes": len(nodes), "t0": t0, "order": order},
                want={"iter": exact(o.traverse_iter(nodes, v, idx, rays)), "rec": exact(o.traverse_recursive(nodes, v, idx, rays, t0=t0))},
                ranges=[("vertex index", idx, len(v.reshape(-1, 3))), ("leaf range", (nodes["left_first"].astype(np.int64) + nodes["count"])[leaf], len(idx) // 3 + 1),
                        ("child pair", nodes["left_first"][~leaf].astype(np.int64) + 1, len(nodes))])


@one_mesh_walks.run
def _(e, p, h):
    for which in ("iter", "rec") if h["order"] == "iterative first" else ("rec", "iter"):      # both block: each gets to be first
        if which == "iter":
            e.ok("vd_traverse_iter_dev", p["nodes"], h["n_nodes"], p["verts"], p["indices"], p["rays"], N_WALK, p["iter"])
        else:
            e.ok("vd_traverse_dev", p["nodes"], h["n_nodes"], p["verts"], p["indices"], p["rays"], N_WALK, C.c_float(h["t0"]), p["rec"])


# ---- instance animation, the stream-side store -----------------------------------------------------------------------------------

N_UPDATE, N_UPDATE_INST = 1667, 5000


@case("vd_compute_update_dev")
def compute_update(o, w, _):
    """The listed records of the instance array, in place; an index out of range is dropped."""
    b = B(w)
    inst = synth.instances(N_UPDATE_INST, seed=SEED + 9 if b else synth.SEED_BASE + 9, extent=60.0)
    ids = np.arange(1 if b else 0, N_UPDATE_INST, 3, dtype=np.uint32)[:N_UPDATE].copy()
    ids[7 if b else 5] = 999_999
    t, dt = (2.9, 0.033) if b else (1.7, 0.016)
    return Spec(dev={"ids": ids}, inout={"instances": inst}, host={"time": t, "dt": dt}, want={"instances": exact(o.compute_update(ids, inst, t, dt, True))})


@compute_update.run
def _(e, p, h):
    e.ok("vd_compute_update_dev", p["ids"], N_UPDATE, p["instances"], N_UPDATE_INST, C.c_float(h["time"]), C.c_float(h["dt"]), 1)


@case("vd_write_value32_async")
def write_value32(o, w, _):
    """Four bytes."""
    v = 0x0BADF00D if B(w) else 0x12345678
    return Spec(out={"word": 4}, host={"value": v}, want={"word": _count(v)})


@write_value32.run
def _(e, p, h):
    e.ok("vd_write_value32_async", p["word"], h["value"])


# ---- host-pointer forms: every buffer in host memory, the call made while the delay holds the context's stream ----------------------

N_HOST = 1237


@case("vd_cull_emit", "vd_cull_compact", "vd_cull_compact_views", "vd_cull_batch", host=True)
def host_cull_forms(o, w, _):
    """As the device forms write."""
    n = N_HOST
    cam, meshes, inst = cull_scene(n, w)
    draws = o.cull_emit(cam, meshes, inst)
    wc, k = o.compact(draws)
    eye = cam["view_position"].reshape(-1)[:3]
    cams = np.stack([synth.camera_uniform(eye=tuple(float(x) for x in eye), yaw_deg=y) for y in _YAWS[:2]]).reshape(-1)
    want = {"emit": exact(draws), "out": records(wc[:k], 20), "count": _count(k)}
    counts = []
    for v in range(2):
        wv, kv = o.compact(o.cull_emit(cams[v], meshes, inst))
        want[f"view{v}"] = records(wv[:kv], 20)
        counts.append(kv)
    cmds, ids = regroup(draws["instance_count"] != 0, inst["mesh"], meshes)
    want.update({"counts_views": exact(np.array(counts, np.uint32)), "cmds": exact(cmds), "ids": records(ids, 4), "count_b": _count(len(ids))})
    return Spec(dev={"meshes": meshes, "instances": inst},
                out={"emit": n * 20, "out": n * 20, "count": 4, "views": 2 * (n + 3) * 20, "counts_views": 8, "cmds": len(meshes) * 20, "ids": n * 4, "count_b": 4},
                host={"cam": cam, "cams": cams, "n_mesh": len(meshes)}, want=want)


VIEWS["host_cull_forms"] = ("views", 2, (N_HOST + 3) * 20)


@host_cull_forms.run
def _(e, p, h):
    n, c, m, k, i = N_HOST, _cam_ptr(h["cam"]), p["meshes"], h["n_mesh"], p["instances"]
    e.ok("vd_cull_emit", c, m, k, i, n, p["emit"])
    e.ok("vd_cull_compact", c, m, k, i, n, p["out"], p["count"], 0)
    e.ok("vd_cull_compact_views", _cam_ptr(h["cams"]), 2, m, k, i, n, p["views"], n + 3, p["counts_views"], 0)
    e.ok("vd_cull_batch", c, m, k, i, n, p["cmds"], p["ids"], p["count_b"])


@case("vd_cull_compact_hiz", "vd_cull_compact_lod", host=True)
def host_occlusion_lod_forms(o, w, _):
    """The occlusion-culled list and the LOD list, with their counts."""
    n, b = N_HOST, B(w)
    cam, meshes = K.camera(frame=int(b)), K.meshes_for(16)
    inst = K.cloud(n, seed=SEED + 60) if b else K.cloud(n)
    pyr = o.hiz_build(K.depth(OCC_W, OCC_H, seed=SEED + 61) if b else K.depth(OCC_W, OCC_H))
    draws, F, V = K.oracle_sets(o, cam, meshes, inst, pyr, OCC_W, OCC_H)
    lst = K.select(draws, V)
    lcam, P, base, lmeshes, groups, linst = lod_scene(o, n, w)
    x = lod_cases.expect(o, lcam, P, base, lmeshes, groups, linst)
    return Spec(dev={"meshes": meshes, "instances": inst, "pyramid": pyr, "groups": groups, "lmeshes": lmeshes, "linstances": linst},
                out={"out": n * 20, "count": 4, "lout": n * 20, "lcount": 4},
                host={"cam": cam, "n_mesh": len(meshes), "lcam": lcam, "P": P, "n_group": len(groups), "n_lmesh": len(lmeshes)},
                want={"out": records(lst, 20), "count": _count(len(lst)), "lout": records(x["list"], 20), "lcount": _count(len(x["list"]))})


@host_occlusion_lod_forms.run
def _(e, p, h):
    n = N_HOST
    e.ok("vd_cull_compact_hiz", _cam_ptr(h["cam"]), p["meshes"], h["n_mesh"], p["instances"], n, p["pyramid"], OCC_W, OCC_H, p["out"], p["count"], 0)
    e.ok("vd_cull_compact_lod", _cam_ptr(h["lcam"]), abi.lod_params(h["P"]), p["groups"], h["n_group"], p["lmeshes"], h["n_lmesh"], p["linstances"], n, p["lout"], p["lcount"], 0)


T_HOST = 77


@case("vd_bvh_build", "vd_bvh_build_lbvh", "vd_bvh_refit", host=True)
def host_blas_forms(o, w, _):
    """One small mesh through the exact build, the LBVH build and the refit (B's tree: the children swapped)."""
    v, i = _mesh(f"soup{T_HOST}", w)
    wn, wi = o.bvh_build(v, i)
    ref = lbvh_reference(v, i)
    va, ia = _mesh(f"soup{T_HOST}", "A")
    rn, ri = o.bvh_build(va, ia)
    v2 = deform(va, phase=0.9 if B(w) else 0.4, specials=False)
    if B(w):
        rn = swapped_children(rn)
    cap = (2 * T_HOST + SPARE) * 32
    return Spec(dev={"verts": v, "verts2": v2, "refit_indices": ri}, inout={"indices": i, "indices_l": i, "refit_nodes": rn}, out={"nodes": cap, "n_nodes": 4, "nodes_l": cap, "n_nodes_l": 4},
                host={"n_vert": len(v), "n_refit_nodes": len(rn)},
                want={"nodes": prefix(wn), "indices": exact(wi), "n_nodes": _count(len(wn)), "nodes_l": prefix(ref["nodes"][: ref["n_nodes"]]), "indices_l": exact(ref["indices"]),
                      "n_nodes_l": _count(ref["n_nodes"]), "refit_nodes": exact(refit_reference(v2, ri, rn))},
                ranges=[("vertex index", i, len(v)), ("vertex index of the refit", ri, len(v2))])


@host_blas_forms.run
def _(e, p, h):
    cap = 2 * T_HOST + SPARE
    e.ok("vd_bvh_build", p["verts"], h["n_vert"], p["indices"], T_HOST, p["nodes"], cap, p["n_nodes"])
    e.ok("vd_bvh_build_lbvh", p["verts"], h["n_vert"], p["indices_l"], T_HOST, p["nodes_l"], cap, p["n_nodes_l"])
    e.ok("vd_bvh_refit", p["verts2"], h["n_vert"], p["refit_indices"], T_HOST, p["refit_nodes"], h["n_refit_nodes"])


@case("vd_bvh_build_batch", "vd_bvh_build_lbvh_batch", host=True)
def host_blas_batches(o, w, _):
    """Three meshes packed behind 11 nodes by the exact builder; the same three through the batched LBVH with host counts."""
    meshes = [_mesh(m, w) for m in ("soup3", "soup77", "soup513")]
    counts = np.array((3, 50, 0) if not B(w) else (2, 77, 500), np.uint32)
    dev, inout, out, want, first, fields, at = {"counts": counts}, {}, {"results": 48}, {}, [], [], 11
    results = np.zeros(3, dtype=abi.BVH_LBVH_RESULT)
    for m, (v, i) in enumerate(meshes):
        wn, wi = o.bvh_build(v, i)
        dev[f"verts{m}"], inout[f"indices{m}"], inout[f"indices_l{m}"] = v, i, i
        want[f"indices{m}"] = exact(wi)
        first.append(wn); fields += [len(wn), at, 0]; at += len(wn)
        T = int(counts[m])
        out[f"nodes_l{m}"] = (2 * (len(i) // 3) + SPARE) * 32
        if T == 0:
            want[f"nodes_l{m}"], want[f"indices_l{m}"] = prefix(np.zeros(0, np.uint8)), exact(i)
            continue
        ref = lbvh_reference(v, i[: 3 * T])
        results[m] = (ref["n_nodes"], 0, ref["max_depth"], 0)
        want[f"nodes_l{m}"], want[f"indices_l{m}"] = prefix(ref["nodes"][: ref["n_nodes"]]), exact(np.concatenate([ref["indices"], i[3 * T:]]))
    out["packed"] = (11 + sum(2 * (len(i) // 3) for _, i in meshes) + SPARE) * 32
    want.update({"packed:fill": prefix(np.zeros(0, np.uint8)), "packed:from 11": prefix(np.concatenate(first)), "host:end": _count(at), "host:items": exact(np.array(fields, np.int64)), "results": exact(results)})
    return Spec(dev=dev, inout=inout, out=out, host={"n_vert": [len(v) for v, _ in meshes], "n_tri": [len(i) // 3 for _, i in meshes]}, want=want,
                ranges=[(f"vertex index of mesh {m}", i, len(v)) for m, (v, i) in enumerate(meshes)])


@host_blas_batches.run
def _(e, p, h):
    items, lit = (abi.BvhBatchItem * 3)(), (abi.BvhLbvhBatchItem * 3)()
    for m in range(3):
        items[m].verts_xyz, items[m].indices_inout, items[m].out_nodes = p[f"verts{m}"], p[f"indices{m}"], None
        items[m].n_vert, items[m].n_tri, items[m].node_cap = h["n_vert"][m], h["n_tri"][m], 0
        items[m].out_n_nodes, items[m].out_first_node, items[m].status = 0xEEEEEEEE, 0xEEEEEEEE, -99
        lit[m].verts_xyz, lit[m].indices_inout, lit[m].nodes, lit[m].mesh_info = p[f"verts{m}"], p[f"indices_l{m}"], p[f"nodes_l{m}"], None
        lit[m].n_vert, lit[m].tri_cap, lit[m].node_cap = h["n_vert"][m], h["n_tri"][m], 2 * h["n_tri"][m] + SPARE
    end = C.c_uint32(0xEEEEEEEE)
    e.ok("vd_bvh_build_batch", C.addressof(items), 3, p["packed"], 11 + sum(2 * t for t in h["n_tri"]) + SPARE, 11, C.addressof(end))
    e.put("host:items", np.array([x for m in range(3) for x in (items[m].out_n_nodes, items[m].out_first_node, items[m].status)], np.int64))
    e.put("host:end", np.array([end.value], np.uint32))
    e.ok("vd_bvh_build_lbvh_batch", C.addressof(lit), 3, p["counts"], p["results"])


@case("vd_tlas_build", "vd_tlas_build_wide", "vd_tlas_refit", "vd_tlas_build_lbvh", "vd_tlas_build_lbvh_wide", host=True)
def host_tlas_forms(o, w, _):
    """(2n + 1) nodes of 32 / 48 bytes from both builders; the refit in place."""
    n = T_HOST
    inst, meshes = tlas_scene(n, w)
    built, now = o.tlas_build(inst, meshes), _nudged(inst)
    return Spec(dev={"instances": inst, "moved": now, "meshes": meshes}, inout={"refit": built},
                out={"nodes": (2 * n + 1) * 32, "wide": (2 * n + 1) * 48, "lbvh": (2 * n + 1) * 32, "lbvh_wide": (2 * n + 1) * 48}, host={"n_mesh": len(meshes)},
                want={"nodes": exact(built), "wide": exact(widen(built)), "lbvh": lbvh_top(inst, meshes, built, False), "lbvh_wide": lbvh_top(inst, meshes, built, True),
                      "refit": exact(o.tlas_refit(now, meshes, built))})


@host_tlas_forms.run
def _(e, p, h):
    n, i, m, k = T_HOST, p["instances"], p["meshes"], h["n_mesh"]
    e.ok("vd_tlas_build", i, n, m, k, p["nodes"])
    e.ok("vd_tlas_build_wide", i, n, m, k, p["wide"])
    e.ok("vd_tlas_build_lbvh", i, n, m, k, p["lbvh"])
    e.ok("vd_tlas_build_lbvh_wide", i, n, m, k, p["lbvh_wide"])
    e.ok("vd_tlas_refit", p["moved"], n, m, k, p["refit"])


@case("vd_trace", "vd_trace_wide", "vd_primary_rays", "vd_traverse_iter", "vd_traverse", host=True)
def host_trace_forms(o, w, _):
    """n_rays records through both top levels; 11 x 7 primary rays; the two one-mesh walks."""
    s, walk = _trace_spec(o, w), _build(CASES["one_mesh_walks[iterative first]"], o, w)
    n = T_HOST
    cam = synth.camera_uniform(eye=(1, 2, 14), pitch_deg=-5) if B(w) else synth.camera_uniform(eye=(0, 0, 15), pitch_deg=0)
    rays, wrays = s.dev["rays"].view(abi.RAY)[:n], walk.dev["rays"].view(abi.RAY)[:n]
    scene = trace_scene(o, w)[0]
    nodes, v, idx = walk.dev["nodes"].view(abi.BVH_NODE), walk.dev["verts"].view(np.float32), walk.dev["indices"].view(np.uint32)
    dev = dict(s.dev, rays=rays, w_nodes=nodes, w_verts=v, w_indices=idx, w_rays=wrays)
    want, _ = o.trace(scene, rays)
    return Spec(dev=dev, out={"hits": n * 16, "hits_wide": n * 16, "primary": 11 * 7 * 32, "iter": n * 4, "rec": n * 4},
                host=dict(s.host, cam=cam, n_w_nodes=len(nodes), n_w_vert=len(v) // 3, n_w_tri=len(idx) // 3, t0=walk.host["t0"]),
                want={"hits": hits(want), "hits_wide": hits(want), "primary": exact(o.primary_rays(cam, 11, 7)), "iter": exact(o.traverse_iter(nodes, v, idx, wrays)),
                      "rec": exact(o.traverse_recursive(nodes, v, idx, wrays, t0=walk.host["t0"]))}, ranges=s.ranges + walk.ranges)


@host_trace_forms.run
def _(e, p, h):
    n = T_HOST
    for wide in (False, True):
        s = _scene_struct(p, h, wide)
        e.ok("vd_trace_wide" if wide else "vd_trace", C.byref(s), p["rays"], n, p["hits_wide" if wide else "hits"])
    e.ok("vd_primary_rays", _cam_ptr(h["cam"]), 11, 7, p["primary"])
    e.ok("vd_traverse_iter", p["w_nodes"], h["n_w_nodes"], p["w_verts"], h["n_w_vert"], p["w_indices"], h["n_w_tri"], p["w_rays"], n, p["iter"])
    e.ok("vd_traverse", p["w_nodes"], h["n_w_nodes"], p["w_verts"], h["n_w_vert"], p["w_indices"], h["n_w_tri"], p["w_rays"], n, C.c_float(h["t0"]), p["rec"])


# ---- what the GPU test compares ----------------------------------------------------------------------------------------------------

def slices(cid, name, nbytes):
    """How the bytes of buffer `name` are cut up for `want`: [(want key, lo, hi)].  Plain buffers: themselves; the views' buffer: one
    slice per view; a packed node array: the nodes in front of the first one keep their fill."""
    if cid in VIEWS and VIEWS[cid][0] == name:
        _, k, stride = VIEWS[cid]
        return [(f"view{v}", v * stride, (v + 1) * stride) for v in range(k)]
    if name == "packed":
        return [("packed:fill", 0, 11 * 32), ("packed:from 11", 11 * 32, nbytes)]
    return [(name, 0, nbytes)]


NO_TEETH = ("packed:fill",)      # the 11 nodes in front of a packed array keep their fill for either input; the array behind them has teeth
