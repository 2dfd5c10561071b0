"""Which bytes of the caller's memory an entry point may touch: every pointer argument of every case sits in a tests/write_set.py
fence - [64 KiB guard | 256-byte aligned payload | 64 KiB guard], inputs included - the call runs once, the payload is compared
with the oracle or restatement the entry point's own parity tests use, and then every guard, every byte of an output that the
header does not promise, and every input must be as they were.

ONE table-driven test.  A case names the entry points it covers (tests/test_write_set_harness.py requires every function of
include/voidin_abi.h to be covered here or listed in EXCLUDED with its reason) and loops over the smallest shapes on both sides
of the entry point's seams.  Inputs that may change are the ones the header names: indices_inout, the instances listed for
vd_compute_update_dev, min / max of a refit's nodes and of its mesh_info, a visibility mask passed in place.

All payloads are 256-byte aligned, no case tries to make a kernel fault or hang; guards see stray stores only."""
import ctypes as C
import functools

import numpy as np
import pytest

import cull_occlusion_cases as K
import lod_cases
import mask_cases as mc
from blas_lbvh_cases import lbvh_reference
from blas_refit_cases import deform, mesh_bounds_reference, refit_reference
from chain_scenes import chain_scene
from conftest import fields_equal, first_difference, golden
from voidin_amd import abi, synth
from wide_scenes import widen
from write_set import Fences

pytestmark = pytest.mark.gpu

NO_BUFFER = "No caller buffer is written."
RANKS = "Needs several ranks."
EXCLUDED = {
    "vd_ctx_create": NO_BUFFER, "vd_ctx_destroy": NO_BUFFER, "vd_ctx_set_stream": NO_BUFFER, "vd_ctx_reset_stream": NO_BUFFER,
    "vd_ctx_synchronize": NO_BUFFER, "vd_ctx_set_option": NO_BUFFER, "vd_last_error": NO_BUFFER, "vd_version": NO_BUFFER,
    "vd_ctx_set_timing": NO_BUFFER, "vd_last_gpu_ms": NO_BUFFER, "vd_last_gpu_ms_stage": NO_BUFFER, "vd_bvh_last_build_stats": NO_BUFFER,
    "vd_trace_accel_info": NO_BUFFER, "vd_trace_accel_info_wide": NO_BUFFER, "vd_hiz_layout": NO_BUFFER,
    "vd_bvh_lbvh_plan_dev": NO_BUFFER, "vd_bvh_lbvh_plan_release": NO_BUFFER, "vd_bvh_refit_plan_dev": NO_BUFFER,
    "vd_bvh_refit_plan_release": NO_BUFFER, "vd_trace_prepare_dev": NO_BUFFER, "vd_trace_prepare_wide_dev": NO_BUFFER,
    "vd_trace_release": NO_BUFFER,
    "vd_import_external_buffer": NO_BUFFER, "vd_release_external_buffer": NO_BUFFER, "vd_import_external_semaphore": NO_BUFFER,
    "vd_wait_external_semaphore_async": NO_BUFFER, "vd_signal_external_semaphore_async": NO_BUFFER,
    "vd_release_external_semaphore": NO_BUFFER, "vd_wait_value32_async": NO_BUFFER, "vd_host_callback_async": NO_BUFFER,
    "vd_dist_unique_id": RANKS, "vd_dist_create": RANKS, "vd_dist_destroy": RANKS, "vd_dist_info": RANKS, "vd_dist_set_scene_dev": RANKS,
    "vd_dist_step_full_dev": RANKS, "vd_dist_step_draws_dev": RANKS, "vd_dist_step_indices_dev": RANKS, "vd_dist_allgather_dev": RANKS,
}

CASES = {}       # case id -> (function, parameter)
COVERS = {}      # entry point -> the case functions that run it

SEAMS = [1, 63, 64, 65, 1023, 1024, 1025, 2049]


def case(*entry_points, params=(None,)):
    def deco(fn):
        for ep in entry_points:
            COVERS.setdefault(ep, []).append(fn.__name__)
        for p in params:
            CASES[fn.__name__ if p is None else f"{fn.__name__}[{p}]"] = (fn, p)
        return fn
    return deco


class Env:
    def __init__(self, ctx, oracle, ctx_options):
        self.ctx, self.oracle, self.opt, self.lib, self.h = ctx, oracle, ctx_options, ctx.lib, ctx.h

    def call(self, name, *args):
        """The entry point with the context in front, then a wait for its stream: the status."""
        rc = getattr(self.lib, name)(self.h, *args)
        self.ctx.synchronize()
        return rc

    def ok(self, name, *args):
        rc = self.call(name, *args)
        if rc == abi.VD_ERR_HIP:                 # the device may have faulted: start nothing more on it
            pytest.exit(f"{name}: VD_ERR_HIP: {self.lib.vd_last_error(self.h)}", returncode=3)
        assert rc == abi.VD_OK, (name, abi.STATUS_NAMES.get(rc, rc), self.lib.vd_last_error(self.h))


def _eq(got, want, tag):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.tobytes() != want.tobytes():
        a, b = np.frombuffer(got.tobytes(), np.uint8), np.frombuffer(want.tobytes(), np.uint8)
        assert len(a) == len(b), f"{tag}: {len(a)} bytes, want {len(b)}"
        k = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"{tag}: first difference at byte {k} of {len(a)}")


def _u32(f):
    return int(f.read(np.uint32)[0])


def _cam(fs, cam, name="camera"):
    return fs.inp(name, np.ascontiguousarray(cam, dtype=abi.CAMERA).reshape(-1), host=True)


# ---- cull / emit ----------------------------------------------------------------------------------------------------------------

_FRONT = dict(centre=(2.0, -2.0, -10.0), extent=6.0, scale_range=(0.5, 1.0))      # a cluster the default camera sees whole


def _cull_scene(n):
    """Every other instance in a cluster the camera sees, the rest spread far beyond the frustum: survivors and culled ones."""
    cam, meshes = synth.camera_uniform(), synth.mesh_infos()
    inst = synth.instances(n, seed=synth.SEED_BASE + 2, scale_range=(0.02, 0.6), extent=600.0, with_inverse=False)
    inst[::2] = synth.instances(n, seed=synth.SEED_BASE + 3, with_inverse=False, **_FRONT)[::2]
    inst["mesh"][n // 3] = 0xFFFFFFFF            # clamped to the last mesh
    return cam, meshes, inst


def _mask_words(flags):
    return K.pack(np.asarray(flags, dtype=bool))


@case("vd_cull_emit_dev", "vd_cull_emit_shard_dev", "vd_cull_mask_dev", "vd_compact_draws_dev", params=SEAMS)
def cull_emit_mask_compact(e, n):
    """emit: exactly n commands; mask: exactly ceil(n / 64) words, padding bits 0; C3 alone: [0, count) and the count word."""
    cam, meshes, inst = _cull_scene(n)
    want = e.oracle.cull_emit(cam, meshes, inst)
    assert n < 63 or 0 < int(want["instance_count"].sum()) < n
    for first in (None, 1000):
        fs = Fences()
        c, m, i, out = _cam(fs, cam), fs.inp("meshes", meshes), fs.inp("instances", inst), fs.out("d_out", n * 20)
        if first is None:
            e.ok("vd_cull_emit_dev", c.ptr, m.ptr, len(meshes), i.ptr, n, out.ptr)
            w = want
        else:
            e.ok("vd_cull_emit_shard_dev", c.ptr, m.ptr, len(meshes), i.ptr, n, first, out.ptr)
            w = want.copy(); w["base_instance"] += np.uint32(first)
        _eq(out.read(), w, f"emit n={n} first={first}")
        fs.check()
    fs = Fences()
    c, m, i, mask = _cam(fs, cam), fs.inp("meshes", meshes), fs.inp("instances", inst), fs.out("d_mask", (n + 63) // 64 * 8)
    e.ok("vd_cull_mask_dev", c.ptr, m.ptr, len(meshes), i.ptr, n, mask.ptr)
    _eq(mask.read(), _mask_words(want["instance_count"] != 0), f"mask n={n}")          # K.pack leaves the padding bits 0
    fs.check()
    fs = Fences()
    wc, k = e.oracle.compact(want)
    d_in, out, cnt = fs.inp("d_in", want), fs.out("d_out", n * 20), fs.out("d_out_count", 4)
    e.ok("vd_compact_draws_dev", d_in.ptr, n, out.ptr, cnt.ptr)
    assert _u32(cnt) == k
    _eq(out.read()[: k * 20], wc[:k], f"compact_draws n={n}")
    out.check_fill(k * 20)
    fs.check()


@case("vd_cull_compact_dev", "vd_cull_compact_shard_dev", "vd_cull_compact_views_dev", params=SEAMS)
def cull_compact(e, n):
    """[0, count) and the count; with pad_tail zeroes up to n_inst; views: nothing in [n_inst, out_stride) of a view either."""
    cam, meshes, inst = _cull_scene(n)
    want = e.oracle.cull_emit(cam, meshes, inst)
    wc, k = e.oracle.compact(want)
    for first, pad in ((None, 0), (None, 1), (1000, 0), (1000, 1)):
        fs = Fences()
        c, m, i = _cam(fs, cam), fs.inp("meshes", meshes), fs.inp("instances", inst)
        out, cnt = fs.out("d_out", n * 20), fs.out("d_out_count", 4)
        w = wc[:k].copy()
        if first is None:
            e.ok("vd_cull_compact_dev", c.ptr, m.ptr, len(meshes), i.ptr, n, out.ptr, cnt.ptr, pad)
        else:
            e.ok("vd_cull_compact_shard_dev", c.ptr, m.ptr, len(meshes), i.ptr, n, first, out.ptr, cnt.ptr, pad)
            w["base_instance"] += np.uint32(first)
        tag = f"compact n={n} first={first} pad={pad}"
        assert _u32(cnt) == k, tag
        _eq(out.read()[: k * 20], w, tag)
        if pad:
            assert not out.read()[k * 20:].any(), tag + ": the padded tail is not zero"
        else:
            out.check_fill(k * 20)
        fs.check()
    cams = np.stack([synth.camera_uniform(yaw_deg=y) for y in (0.0, 90.0, 180.0)]).reshape(-1)
    stride = n + 5
    for pad in (0, 1):
        fs = Fences()
        c, m, i = _cam(fs, cams, "cameras"), fs.inp("meshes", meshes), fs.inp("instances", inst)
        out, cnt = fs.out("d_out", 3 * stride * 20), fs.out("d_out_counts", 12)
        e.ok("vd_cull_compact_views_dev", c.ptr, 3, m.ptr, len(meshes), i.ptr, n, out.ptr, stride, cnt.ptr, pad)
        raw, counts = out.read(), cnt.read(np.uint32)
        for v in range(3):
            wv, kv = e.oracle.compact(e.oracle.cull_emit(cams[v], meshes, inst))
            tag = f"views n={n} view {v} pad={pad}"
            assert counts[v] == kv, tag
            at = v * stride * 20
            _eq(raw[at: at + kv * 20], wv[:kv], tag)
            if pad:
                assert not raw[at + kv * 20: at + n * 20].any(), tag
                out.check_fill(at + n * 20, at + stride * 20)
            else:
                out.check_fill(at + kv * 20, at + stride * 20)
        fs.check()


@case("vd_mask_to_indices_dev", "vd_indices_to_draws_dev", "vd_expand_mask_dev", params=SEAMS)
def mask_wire_formats(e, n):
    """indices: the count word and [0, count) of the n_inst words (words past the count keep their bytes: the header says so since
    this file found it true at every size); draws: exactly n_indices commands; expansion: [0, count) and the count."""
    cam, meshes, inst = _cull_scene(n)
    vis = e.oracle.cull_emit(cam, meshes, inst)["instance_count"] != 0
    words = _mask_words(vis)
    ids = np.minimum(inst["mesh"], 255).astype(np.uint8)                      # the table clamps again to n_mesh - 1
    fs = Fences()
    mask, out, cnt = fs.inp("d_mask", words), fs.out("d_out_indices", n * 4), fs.out("d_out_count", 4)
    e.ok("vd_mask_to_indices_dev", mask.ptr, n, 7, out.ptr, cnt.ptr)
    want = mc.indices_reference(words, n, 7)
    k = len(want)
    assert _u32(cnt) == k
    _eq(out.read()[: 4 * k], want, f"mask_to_indices n={n}")
    out.check_fill(4 * k)
    fs.check()
    lst = (want - np.uint32(7)).astype(np.uint32)
    fs = Fences()
    d_l, d_ids, m, out = fs.inp("d_indices", lst if k else np.zeros(1, np.uint32)), fs.inp("d_mesh_ids", ids), fs.inp("meshes", meshes), fs.out("d_out", max(k, 1) * 20)
    e.ok("vd_indices_to_draws_dev", d_l.ptr, k, d_ids.ptr, 1, n, m.ptr, len(meshes), out.ptr)
    _eq(out.read()[: k * 20], mc.draws_from_indices_reference(lst, ids, meshes), f"indices_to_draws n={n}")
    out.check_fill(k * 20)
    fs.check()
    fs = Fences()
    mask, d_ids, m, out, cnt = fs.inp("d_mask", words), fs.inp("d_mesh_ids", ids), fs.inp("meshes", meshes), fs.out("d_out", n * 20), fs.out("d_out_count", 4)
    e.ok("vd_expand_mask_dev", mask.ptr, n, n, d_ids.ptr, 1, m.ptr, len(meshes), out.ptr, cnt.ptr)
    wd, wk = mc.expand_reference(words, n, n, ids, meshes)
    assert _u32(cnt) == wk == k
    _eq(out.read()[: k * 20], wd, f"expand n={n}")
    out.check_fill(k * 20)
    fs.check()


def _regroup(vis, mesh_col, meshes):
    """(cmds, ids) of "Instanced draw lists" from a visibility vector and the instances' mesh ids (tests/test_gpu_cull_batch.py)."""
    n_mesh = len(meshes)
    S = np.flatnonzero(vis)
    mid = np.minimum(mesh_col, n_mesh - 1)[S].astype(np.int64)
    ids = S[np.argsort(mid, kind="stable")].astype(np.uint32)
    cnt = np.bincount(mid, minlength=n_mesh)
    cmds = np.zeros(n_mesh, abi.DRAW)
    cmds["vertex_count"], cmds["instance_count"], cmds["base_index"] = meshes["index_count"], cnt, meshes["base_index"]
    cmds["vertex_offset"], cmds["base_instance"] = meshes["vertex_offset"], np.cumsum(cnt) - cnt
    return cmds, ids


@case("vd_cull_batch_dev", "vd_batch_mask_dev", params=[1, 63, 65, 1025, 2049])
def instanced_lists(e, n):
    """exactly n_mesh commands, [0, |S|) of the id words - words [|S|, n_inst) are NOT written - and the count."""
    cam, meshes, inst = _cull_scene(n)
    vis = e.oracle.cull_emit(cam, meshes, inst)["instance_count"] != 0
    cmds, ids = _regroup(vis, inst["mesh"], meshes)
    k = len(ids)
    for name in ("vd_cull_batch_dev", "vd_batch_mask_dev"):
        fs = Fences()
        m = fs.inp("meshes", meshes)
        o_c, o_i, cnt = fs.out("d_out_cmds", len(meshes) * 20), fs.out("d_out_instance_ids", n * 4), fs.out("d_out_count", 4)
        if name == "vd_cull_batch_dev":
            c, i = _cam(fs, cam), fs.inp("instances", inst)
            e.ok(name, c.ptr, m.ptr, len(meshes), i.ptr, n, o_c.ptr, o_i.ptr, cnt.ptr)
        else:
            mask, t = fs.inp("d_mask", _mask_words(vis)), fs.inp("d_mesh_ids", inst["mesh"].astype(np.uint32))
            e.ok(name, mask.ptr, n, t.ptr, 4, m.ptr, len(meshes), o_c.ptr, o_i.ptr, cnt.ptr)
        assert _u32(cnt) == k, name
        _eq(o_c.read(), cmds, f"{name} n={n} commands")
        _eq(o_i.read()[: 4 * k], ids, f"{name} n={n} ids")
        o_i.check_fill(4 * k)
        fs.check()


# ---- occlusion -------------------------------------------------------------------------------------------------------------------

@case("vd_hiz_build_dev", params=["1x1", "2x1", "5x3", "100x37", "4097x3"])
def hiz_build(e, shape):
    """exactly total_texels floats; the depth buffer comes back unchanged."""
    w, h = (int(x) for x in shape.split("x"))
    depth = synth.uniform01(synth.SEED_BASE + 44, 0, w * h).reshape(h, w).astype(np.float32)
    want = e.oracle.hiz_build(depth)
    assert len(want) == e.ctx.hiz_layout(w, h).total_texels
    fs = Fences()
    d, p = fs.inp("d_depth", depth), fs.out("d_pyramid", len(want) * 4)
    e.ok("vd_hiz_build_dev", d.ptr, w, h, p.ptr)
    _eq(p.read(), want, f"pyramid {shape}")
    fs.check()


@case("vd_occlusion_mask_dev", "vd_cull_compact_hiz_dev", "vd_cull_early_dev", "vd_cull_late_dev", params=[1, 63, 64, 65, 5000])
def occlusion(e, n):
    """mask: ceil(n / 64) words, separate and in place; lists: [0, count) + the count (pad_tail: zero up to n_inst); late: also the
    ceil(n / 64) words of d_visible_out, separate and in place.  Pyramid, instances, meshes unchanged."""
    w, h = 100, 37
    cam, meshes, inst = K.camera(), K.meshes_for(16), K.cloud(n)
    pyr = e.oracle.hiz_build(K.depth(w, h))
    draws, F, V = K.oracle_sets(e.oracle, cam, meshes, inst, pyr, w, h)
    wF, wV = K.pack(F), K.pack(V)
    for in_place in (False, True):
        fs = Fences()
        c, m, i, p = _cam(fs, cam), fs.inp("meshes", meshes), fs.inp("instances", inst), fs.inp("d_pyramid", pyr)
        if in_place:
            mi = mo = fs.inout("d_mask (in place)", wF)
        else:
            mi, mo = fs.inp("d_mask_in", wF), fs.out("d_mask_out", len(wF) * 8)
        e.ok("vd_occlusion_mask_dev", c.ptr, m.ptr, len(meshes), i.ptr, n, p.ptr, w, h, mi.ptr, mo.ptr)
        _eq(mo.read(), wV, f"occlusion mask n={n} in_place={in_place}")
        fs.check()
    P = K.random_prev(n)
    Pb = K.bits(P, n)
    for name, sel in (("vd_cull_compact_hiz_dev", V), ("vd_cull_early_dev", F & Pb), ("vd_cull_late_dev", V & ~Pb), ("vd_cull_late_dev in place", V & ~Pb)):
        for pad in (0, 1):
            fs = Fences()
            c, m, i = _cam(fs, cam), fs.inp("meshes", meshes), fs.inp("instances", inst)
            out, cnt = fs.out("d_out", n * 20), fs.out("d_out_count", 4)
            if name == "vd_cull_compact_hiz_dev":
                p = fs.inp("d_pyramid", pyr)
                e.ok(name, c.ptr, m.ptr, len(meshes), i.ptr, n, p.ptr, w, h, out.ptr, cnt.ptr, pad)
            elif name == "vd_cull_early_dev":
                pv = fs.inp("d_prev_visible", P)
                e.ok(name, c.ptr, m.ptr, len(meshes), i.ptr, n, pv.ptr, out.ptr, cnt.ptr, pad)
            else:
                p = fs.inp("d_pyramid", pyr)
                if name.endswith("in place"):
                    pv = vo = fs.inout("d_prev_visible = d_visible_out", P)
                else:
                    pv, vo = fs.inp("d_prev_visible", P), fs.out("d_visible_out", len(P) * 8)
                e.ok("vd_cull_late_dev", c.ptr, m.ptr, len(meshes), i.ptr, n, p.ptr, w, h, pv.ptr, vo.ptr, out.ptr, cnt.ptr, pad)
                _eq(vo.read(), wV, f"{name} n={n}: d_visible_out")
            lst = K.select(draws, sel)
            k = len(lst)
            tag = f"{name} n={n} pad={pad}"
            assert _u32(cnt) == k, tag
            _eq(out.read()[: k * 20], lst, tag)
            if pad:
                assert not out.read()[k * 20:].any(), tag
            else:
                out.check_fill(k * 20)
            fs.check()


# ---- level of detail -------------------------------------------------------------------------------------------------------------

@case("vd_lod_ids_dev", "vd_cull_compact_lod_dev", "vd_cull_batch_lod_dev", params=[64, 1025, 2049])
def level_of_detail(e, n):
    """ids: exactly n_inst ids of id_bytes; list: [0, count) + the count; instanced: n_mesh commands, [0, count) ids, the count."""
    cam, P, base, meshes, groups, inst = lod_cases.scene(e.oracle, n)
    x = lod_cases.expect(e.oracle, cam, P, base, meshes, groups, inst)
    lp = abi.lod_params(P)
    for id_bytes, dt in ((1, np.uint8), (2, np.uint16), (4, np.uint32)):
        fs = Fences()
        c, g, i, out = _cam(fs, cam), fs.inp("d_groups", groups), fs.inp("instances", inst), fs.out("d_out_ids", n * id_bytes)
        e.ok("vd_lod_ids_dev", c.ptr, lp, g.ptr, len(groups), len(meshes), i.ptr, n, out.ptr, id_bytes)
        _eq(out.read(), x["row"].astype(dt), f"lod ids n={n} id_bytes={id_bytes}")
        fs.check()
    k = len(x["list"])
    for pad in (0, 1):
        fs = Fences()
        c, g, m, i = _cam(fs, cam), fs.inp("d_groups", groups), fs.inp("meshes", meshes), fs.inp("instances", inst)
        out, cnt = fs.out("d_out", n * 20), fs.out("d_out_count", 4)
        e.ok("vd_cull_compact_lod_dev", c.ptr, lp, g.ptr, len(groups), m.ptr, len(meshes), i.ptr, n, out.ptr, cnt.ptr, pad)
        assert _u32(cnt) == k
        _eq(out.read()[: k * 20], x["list"], f"lod list n={n} pad={pad}")
        if pad:
            assert not out.read()[k * 20:].any()
        else:
            out.check_fill(k * 20)
        fs.check()
    fs = Fences()
    c, g, m, i = _cam(fs, cam), fs.inp("d_groups", groups), fs.inp("meshes", meshes), fs.inp("instances", inst)
    o_c, o_i, cnt = fs.out("d_out_cmds", len(meshes) * 20), fs.out("d_out_instance_ids", n * 4), fs.out("d_out_count", 4)
    e.ok("vd_cull_batch_lod_dev", c.ptr, lp, g.ptr, len(groups), m.ptr, len(meshes), i.ptr, n, o_c.ptr, o_i.ptr, cnt.ptr)
    assert _u32(cnt) == k
    _eq(o_c.read(), x["cmds"], f"lod batch n={n} commands")
    _eq(o_i.read()[: 4 * k], x["ids"], f"lod batch n={n} ids")
    o_i.check_fill(4 * k)
    fs.check()


# ---- BLAS ------------------------------------------------------------------------------------------------------------------------

def _soup(n_tri):
    v, i = synth.triangle_soup(n_tri, seed=synth.SEED_BASE + 100 + n_tri)
    return np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(i, dtype=np.uint32).reshape(-1)


@case("vd_bvh_build_dev", params=[1, 3, 4, 64, 65, 512, 513, 2048, 2049])
def sah_build(e, n_tri):
    """nodes [0, n_nodes) of a node_cap = 2 n_tri + 37 array - the bytes of [n_nodes, node_cap) are NOT written (the header says so
    since this file found it true at every size) - exactly 3 n_tri indices, the host's n_nodes word; vertices unchanged."""
    v, i = _soup(n_tri)
    wn, wi = e.oracle.bvh_build(v, i)
    cap = 2 * n_tri + 37
    fs = Fences()
    d_v, d_i, d_n, nn = fs.inp("verts_xyz", v), fs.inout("indices_inout", i), fs.out("out_nodes", cap * 32), fs.out("out_n_nodes", 4, host=True)
    e.ok("vd_bvh_build_dev", d_v.ptr, len(v), d_i.ptr, n_tri, d_n.ptr, cap, nn.ptr)
    k = _u32(nn)
    assert k == len(wn) and k < cap
    got = d_n.read(abi.BVH_NODE, k)
    assert fields_equal(got, wn), first_difference(got, wn)
    _eq(d_i.read(), wi, f"indices n_tri={n_tri}")
    d_n.check_fill(k * 32)
    fs.check()


@case("vd_bvh_build_dev", params=["degenerate", "bad index"])
def sah_build_errors(e, kind):
    """An error return: nothing outside the three buffers is written and the vertices are unchanged.  What is written inside them is
    printed (pytest -s), not asserted - the header leaves the outputs of a failed build open; when this case was written both
    inputs left nodes, indices and the n_nodes word untouched."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    i = np.tile(np.array([0, 1, 2], np.uint32), 5) if kind == "degenerate" else np.array([0, 1, 2, 0, 1, 7], np.uint32)
    n_tri, cap = len(i) // 3, 2 * (len(i) // 3) + 37
    fs = Fences()
    d_v, d_i, d_n, nn = fs.inp("verts_xyz", v), fs.inout("indices_inout", i), fs.out("out_nodes", cap * 32), fs.out("out_n_nodes", 4, host=True)
    rc = e.call("vd_bvh_build_dev", d_v.ptr, len(v), d_i.ptr, n_tri, d_n.ptr, cap, nn.ptr)
    assert rc == (abi.VD_ERR_DEGENERATE if kind == "degenerate" else abi.VD_ERR_INVALID_ARG)
    print(f"vd_bvh_build_dev ({kind}): nodes written: {not d_n.fill_intact(0)}, indices changed: {d_i.read().tobytes() != i.tobytes()}, "
          f"n_nodes word written: {not nn.fill_intact(0)}")
    fs.check()


def _batch_items(fs, meshes, own, extra=37):
    items = (abi.BvhBatchItem * len(meshes))()
    bufs = []
    for m, (v, i) in enumerate(meshes):
        n_tri = len(i) // 3
        d_v, d_i = fs.inp(f"verts_xyz[{m}]", v), fs.inout(f"indices_inout[{m}]", i)
        d_n = fs.out(f"out_nodes[{m}]", (2 * n_tri + extra) * 32) if own else None
        items[m].verts_xyz, items[m].indices_inout, items[m].out_nodes = d_v.ptr, d_i.ptr, d_n.ptr if own else None
        items[m].n_vert, items[m].n_tri, items[m].node_cap = len(v), n_tri, 2 * n_tri + extra if own else 0
        items[m].out_n_nodes, items[m].out_first_node, items[m].status = 0xEEEEEEEE, 0xEEEEEEEE, -99
        bufs.append((d_v, d_i, d_n))
    return items, bufs


def _batch_items_check(before, after, K_):
    """The item array: only out_n_nodes, out_first_node and status of every item may change."""
    for m in range(K_):
        for f in ("verts_xyz", "indices_inout", "out_nodes", "n_vert", "n_tri", "node_cap"):
            assert getattr(before[m], f) == getattr(after[m], f), (m, f)


@case("vd_bvh_build_batch_dev", params=["own", "packed"])
def sah_batch(e, form):
    """Three meshes (3, 513, 2049 triangles).  own: as vd_bvh_build_dev per mesh; packed with packed_first = 11: nothing before node 11,
    nothing at or after *out_packed_end; of the item array only the three written fields."""
    meshes = [_soup(t) for t in (3, 513, 2049)]
    want = [e.oracle.bvh_build(v, i) for v, i in meshes]
    fs = Fences()
    items, bufs = _batch_items(fs, meshes, own=(form == "own"))
    first, pcap = 11, 11 + sum(2 * (len(i) // 3) for _, i in meshes) + 37
    packed = fs.out("d_packed_nodes", pcap * 32) if form == "packed" else None
    raw = bytes(items)
    h_items, end = fs.inout("items", np.frombuffer(raw, np.uint8), host=True), fs.out("out_packed_end", 4, host=True)
    if form == "own":
        e.ok("vd_bvh_build_batch_dev", h_items.ptr, 3, None, 0, 0, end.ptr)
    else:
        e.ok("vd_bvh_build_batch_dev", h_items.ptr, 3, packed.ptr, pcap, first, end.ptr)
    after = (abi.BvhBatchItem * 3).from_buffer_copy(h_items.read().tobytes())
    _batch_items_check(items, after, 3)
    at = first
    for m, (wn, wi) in enumerate(want):
        d_v, d_i, d_n = bufs[m]
        assert after[m].status == 0 and after[m].out_n_nodes == len(wn), m
        if form == "own":
            got = d_n.read(abi.BVH_NODE, len(wn))
            d_n.check_fill(len(wn) * 32)
        else:
            assert after[m].out_first_node == at
            got = packed.read(abi.BVH_NODE)[at: at + len(wn)]
            at += len(wn)
        assert fields_equal(got, wn), (m, first_difference(got, wn))
        _eq(d_i.read(), wi, f"mesh {m}: indices")
    if form == "packed":
        assert _u32(end) == at
        packed.check_fill(0, first * 32)
        packed.check_fill(at * 32)
    fs.check()


@case("vd_bvh_build_lbvh_dev", params=[1, 3, 4, 64, 65, 513, 2049])
def lbvh_build(e, n_tri):
    """nodes [0, n_nodes) - "No byte of out_nodes past n_nodes is written" - the 3 n_tri indices, the 16 bytes of d_result."""
    v, i = _soup(n_tri)
    ref = lbvh_reference(v, i)
    cap = max(2, 2 * n_tri) + 37
    fs = Fences()
    d_v, d_i, d_n, res = fs.inp("verts_xyz", v), fs.inout("indices_inout", i), fs.out("out_nodes", cap * 32), fs.out("d_result", 16)
    e.ok("vd_bvh_build_lbvh_dev", d_v.ptr, len(v), d_i.ptr, n_tri, d_n.ptr, cap, res.ptr)
    r = res.read(abi.BVH_LBVH_RESULT)[0]
    assert (int(r["n_nodes"]), int(r["n_bad_indices"]), int(r["max_depth"]), int(r["_pad"])) == (ref["n_nodes"], 0, ref["max_depth"], 0)
    got = d_n.read(abi.BVH_NODE, ref["n_nodes"])
    assert fields_equal(got, ref["nodes"]), first_difference(got, ref["nodes"])
    _eq(d_i.read(), ref["indices"], f"lbvh indices n_tri={n_tri}")
    d_n.check_fill(ref["n_nodes"] * 32)
    fs.check()


@case("vd_bvh_build_lbvh_planned_dev")
def lbvh_batch(e, _):
    """Three meshes with device counts {all, 100 of 513, 0}: per mesh nodes [0, n_nodes), the first 3 T indices, 16 result bytes; "No byte
    of nodes past n_nodes and no index past 3 * T_m is written"; min / max of the one mesh_info and no other field; counts unchanged."""
    meshes = [_soup(t) for t in (65, 513, 4)]
    counts = np.array([65, 100, 0], np.uint32)
    info = np.zeros(1, dtype=abi.MESH_INFO)
    info["min"], info["max"], info["index_count"], info["base_index"], info["vertex_offset"], info["bvh_index"], info["junk"] = 77.0, -77.0, 9, 11, 22, 33, (44, 55)
    fs = Fences()
    items = (abi.BvhLbvhBatchItem * 3)()
    bufs = []
    d_info = fs.inp("mesh_info[1]", info)
    for m, (v, i) in enumerate(meshes):
        cap = len(i) // 3
        d_v, d_i, d_n = fs.inp(f"verts_xyz[{m}]", v), fs.inout(f"indices_inout[{m}]", i), fs.out(f"nodes[{m}]", (2 * cap + 37) * 32)
        items[m].verts_xyz, items[m].indices_inout, items[m].nodes = d_v.ptr, d_i.ptr, d_n.ptr
        items[m].mesh_info = d_info.ptr if m == 1 else None
        items[m].n_vert, items[m].tri_cap, items[m].node_cap = len(v), cap, 2 * cap + 37
        bufs.append((d_i, d_n))
    plan = e.ctx.bvh_lbvh_plan(items)
    try:
        d_c, res = fs.inp("d_n_tri", counts), fs.out("d_results", 48)
        e.ok("vd_bvh_build_lbvh_planned_dev", plan.h, d_c.ptr, res.ptr)
    finally:
        plan.close()
    results = res.read(abi.BVH_LBVH_RESULT)
    for m, (v, i) in enumerate(meshes):
        T = int(counts[m])
        d_i, d_n = bufs[m]
        if T == 0:
            assert not results[m:m + 1].view(np.uint8).any() and d_n.fill_intact(0)
            _eq(d_i.read(), i, f"mesh {m}: T == 0 writes no index")
            continue
        ref = lbvh_reference(v, i[: 3 * T])
        assert (int(results[m]["n_nodes"]), int(results[m]["n_bad_indices"]), int(results[m]["max_depth"]), int(results[m]["_pad"])) == (ref["n_nodes"], 0, ref["max_depth"], 0)
        got = d_n.read(abi.BVH_NODE, ref["n_nodes"])
        assert fields_equal(got, ref["nodes"]), (m, first_difference(got, ref["nodes"]))
        d_n.check_fill(ref["n_nodes"] * 32)
        _eq(d_i.read(), np.concatenate([ref["indices"], i[3 * T:]]), f"mesh {m}: indices")
    lo, hi = mesh_bounds_reference(meshes[1][0])
    got = d_info.read(abi.MESH_INFO)
    assert got["min"][0].tobytes() == lo.tobytes() and got["max"][0].tobytes() == hi.tobytes()
    box = np.zeros(48, bool); box[0:12] = box[16:28] = True
    fs.check(allowed={"mesh_info[1]": box})


@case("vd_bvh_refit_planned_dev", params=[1, 4, 65, 513, 2049])
def blas_refit(e, n_tri):
    """REWRITTEN: min / max of the reachable nodes and of the mesh_info; NOT rewritten: left_first, count, every byte past n_nodes,
    the indices, the vertices, every other field of the VdMeshInfo."""
    v, i = _soup(n_tri)
    nodes, idx = e.oracle.bvh_build(v, i)
    v2 = deform(v, phase=0.4)
    info = np.zeros(1, dtype=abi.MESH_INFO)
    info["min"], info["max"], info["index_count"], info["base_index"], info["vertex_offset"], info["bvh_index"], info["junk"] = 77.0, -77.0, 9, 11, 22, 33, (44, 55)
    fs = Fences()
    d_v, d_i, d_n, d_info = fs.inp("verts_xyz", v2), fs.inp("indices", idx), fs.inp("nodes", nodes), fs.inp("mesh_info", info)
    items = (abi.BvhRefitItem * 1)()
    items[0].verts_xyz, items[0].indices, items[0].nodes, items[0].mesh_info = d_v.ptr, d_i.ptr, d_n.ptr, d_info.ptr
    items[0].n_vert, items[0].n_tri, items[0].n_nodes = len(v2), n_tri, len(nodes)
    plan = e.ctx.bvh_refit_plan(items)
    try:
        e.ok("vd_bvh_refit_planned_dev", plan.h)
    finally:
        plan.close()
    want = refit_reference(v2, idx, nodes)
    got = d_n.read(abi.BVH_NODE)
    assert fields_equal(got, want), first_difference(got, want)
    assert not fields_equal(got, nodes), "the refit changed no box"
    lo, hi = mesh_bounds_reference(v2)
    gi = d_info.read(abi.MESH_INFO)
    assert gi["min"][0].tobytes() == lo.tobytes() and gi["max"][0].tobytes() == hi.tobytes()
    box = np.zeros(32, bool); box[0:12] = box[16:28] = True
    ibox = np.zeros(48, bool); ibox[0:12] = ibox[16:28] = True
    fs.check(allowed={"nodes": np.tile(box, len(nodes)), "mesh_info": ibox})


# ---- TLAS ------------------------------------------------------------------------------------------------------------------------

def _tlas_scene(n, seed=50):
    return synth.instances(n, seed=synth.SEED_BASE + seed + n % 97, extent=120.0), synth.mesh_infos()


def _tlas_builds(e, inst, meshes, tag, want=None):
    """vd_tlas_build_dev / _wide_dev into exactly 2n + 1 nodes of 32 / 48 bytes; instances and meshes unchanged."""
    n = len(inst)
    want = e.oracle.tlas_build(inst, meshes) if want is None else want
    for name, dt in (("vd_tlas_build_dev", abi.TLAS_NODE), ("vd_tlas_build_wide_dev", abi.TLAS_NODE_WIDE)):
        fs = Fences()
        i, m, out = fs.inp("instances", inst), fs.inp("meshes", meshes), fs.out("d_out_nodes", (2 * n + 1) * dt.itemsize)
        e.ok(name, i.ptr, n, m.ptr, len(meshes), out.ptr)
        got = out.read(dt)
        if dt == abi.TLAS_NODE:
            assert fields_equal(got, want), (tag, name, first_difference(got, want))
        else:
            assert fields_equal(got, widen(want)), (tag, name)          # same chain, children as two u32, _pad 0
        fs.check()
    return want


@case("vd_tlas_build_dev", "vd_tlas_build_wide_dev", "vd_tlas_refit_dev", "vd_tlas_refit_wide_dev", params=[1, 2, 3, 64, 65, 1000])
def tlas_build_and_refit(e, n):
    """build: exactly (2n + 1) nodes; refit: the same nodes in place, topology fields as they were; instances and meshes unchanged."""
    inst, meshes = _tlas_scene(n)
    built = _tlas_builds(e, inst, meshes, f"n={n}")
    moved = inst.copy()
    moved["transform"][::3, 12:15] += np.float32(0.37)
    for name, nodes in (("vd_tlas_refit_dev", built), ("vd_tlas_refit_wide_dev", widen(built))):
        fs = Fences()
        i, m, d_n = fs.inp("instances", moved), fs.inp("meshes", meshes), fs.inout("d_nodes_inout", nodes)
        e.ok(name, i.ptr, n, m.ptr, len(meshes), d_n.ptr)
        want = e.oracle.tlas_refit(moved, meshes, nodes)
        got = d_n.read(nodes.dtype)
        assert fields_equal(got, want), (name, first_difference(got, want))
        for f in ("left_right", "instance_idx") if nodes.dtype == abi.TLAS_NODE else ("left", "right", "instance_idx", "_pad"):
            assert np.array_equal(got[f], nodes[f]), (name, f)
        fs.check()


@functools.lru_cache(maxsize=None)
def _several_workgroups_scene(oracle):
    """(instances, meshes, the oracle's nodes) at the smallest n the chain shares among 16 workgroups; computed once, never modified."""
    inst, meshes = synth.instances(12288, seed=synth.SEED_BASE + 14, extent=700.0), synth.mesh_infos()
    return inst, meshes, oracle.tlas_build(inst, meshes)


@case("vd_tlas_build_dev", "vd_tlas_build_wide_dev", params=["chain from memory", "indexed", "several workgroups", "several workgroups, redone on one"])
def tlas_build_further_paths(e, path):
    """One n on each further path of the agglomerative build, selected as tests/test_gpu_tlas_trace.py selects them."""
    if path == "chain from memory":
        e.opt("tlas.chain_lds", 0)
        inst, meshes = _tlas_scene(700)
    elif path == "indexed":                                  # test_indexed_build_on_ties_nesting_and_stale_slots
        e.opt("tlas.index_min", 65); e.opt("tlas.phase2", 64); e.opt("tlas.refresh", 37)
        inst, meshes = _tlas_scene(257)
    else:                                                    # test_tlas_build_on_several_workgroups_vs_oracle: from 12288 instances on
        if path.endswith("one"):
            e.opt("tlas.spin_limit", 0)
        inst, meshes, want = _several_workgroups_scene(e.oracle)
        _tlas_builds(e, inst, meshes, path, want)
        return
    _tlas_builds(e, inst, meshes, path)


def _lbvh_children(nodes):
    if nodes.dtype == abi.TLAS_NODE_WIDE:
        return nodes["left"].astype(np.int64), nodes["right"].astype(np.int64)
    return (nodes["left_right"] & 0xffff).astype(np.int64), (nodes["left_right"] >> 16).astype(np.int64)


@case("vd_tlas_build_lbvh_dev", "vd_tlas_build_lbvh_wide_dev", params=[1, 2, 3, 64, 65, 1000])
def tlas_lbvh(e, n):
    """exactly (2n + 1) nodes of 32 / 48 bytes.  The array is held against the header's layout: the leaves are the exact builder's leaf
    boxes in some order, every instance is reached once from node 0, and the oracle's refit changes no byte (so every box is the
    union it should be); tests/test_gpu_tlas_lbvh.py checks the code order."""
    inst, meshes = _tlas_scene(n)
    exact = e.oracle.tlas_build(inst, meshes)
    for name, dt in (("vd_tlas_build_lbvh_dev", abi.TLAS_NODE), ("vd_tlas_build_lbvh_wide_dev", abi.TLAS_NODE_WIDE)):
        fs = Fences()
        i, m, out = fs.inp("instances", inst), fs.inp("meshes", meshes), fs.out("d_out_nodes", (2 * n + 1) * dt.itemsize)
        e.ok(name, i.ptr, n, m.ptr, len(meshes), out.ptr)
        nodes = out.read(dt)
        order = nodes["instance_idx"][1:n + 1].astype(np.int64)
        assert sorted(order.tolist()) == list(range(n)), name
        assert nodes["min"][1:n + 1].tobytes() == exact["min"][1 + order].tobytes() and nodes["max"][1:n + 1].tobytes() == exact["max"][1 + order].tobytes(), name
        left, right = _lbvh_children(nodes)
        seen, todo = [], [0]
        while todo:
            k = todo.pop()
            if left[k] == 0 and right[k] == 0:
                seen.append(int(nodes["instance_idx"][k]))
            else:
                todo += [int(left[k]), int(right[k])]
        assert sorted(seen) == list(range(n)), name
        assert e.oracle.tlas_refit(inst, meshes, nodes).tobytes() == nodes.tobytes(), f"{name}: a box is not the union of its children's"
        fs.check()


# ---- trace -----------------------------------------------------------------------------------------------------------------------

SCENE_NAMES = ("tlas_nodes", "instances", "meshes", "bvh_nodes", "vertices", "indices")
N_RAYS = [1, 63, 64, 65, 4097]


def _fenced_scene(fs, scene, wide):
    """The six buffers of a trace scene as inputs, and the struct that names them in a host fence."""
    dts = [abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE, abi.INSTANCE, abi.MESH_INFO, abi.BVH_NODE, np.float32, np.uint32]
    arrs = [np.ascontiguousarray(a, dtype=d).reshape(-1) for a, d in zip(scene, dts)]
    s = abi.TraceSceneWide() if wide else abi.TraceScene()
    bufs = []
    for name, a in zip(SCENE_NAMES, arrs):
        f = fs.inp(name, a)
        setattr(s, name, f.ptr)
        setattr(s, "n_" + name, len(a) // (3 if name == "vertices" else 1))
        bufs.append(f)
    h = fs.inp("scene struct", np.frombuffer(bytes(s), np.uint8), host=True)
    return C.cast(h.ptr, C.POINTER(type(s))), bufs


def _trace40(e):
    g = golden("trace_40.npz")
    scene = (g["tlas"], g["instances"], g["meshes"], g["bvh_nodes"], g["vertices"], g["indices"])
    assert len(g["instances"]) == 40
    hit, miss = np.flatnonzero(g["hit"] == 1), np.flatnonzero(g["hit"] == 0)
    k = min(len(hit), len(miss))
    order = np.concatenate([np.stack([hit[:k], miss[:k]], axis=1).reshape(-1), hit[k:], miss[k:]])      # hits and misses alternate from ray 0 on
    return scene, g["rays"][order]


def _check_hits(got, want, exact, tag):
    if exact:
        _eq(got, want, tag)
        return
    assert np.array_equal(got["hit"], want["hit"]), tag
    hit = want["hit"] == 1
    assert np.all(np.abs(got["dist"][hit].astype(np.float64) - want["dist"][hit]) <= 1e-5), tag      # tests/test_gpu_trace_tight.py ABS_TOL
    assert (got["dist"][~hit] == np.float32(1e30)).all(), tag


TRACE_FORMS = ["plain", "plain, trace.auto_prepare = 0", "wide", "prepared", "prepared, tight 1", "prepared, tight 2", "prepared wide", "prepared wide, tight",
               "plain, global-memory stack pass", "prepared, global-memory stack pass"]


@case("vd_trace_dev", "vd_trace_any_dev", "vd_trace_wide_dev", "vd_trace_any_wide_dev", "vd_trace_prepared_dev", "vd_trace_any_prepared_dev", params=TRACE_FORMS)
def trace(e, form):
    """n_rays * 16 bytes of records / n_rays * 4 bytes of flags; all six scene buffers, the scene struct and the rays unchanged."""
    deep = "stack pass" in form
    if deep:
        scene = chain_scene(e.oracle, 123)          # depth N + 6 (tests/test_gpu_trace_deep.py): the shortest chain past a lane's 128 entries
        pool = np.zeros(8, dtype=abi.RAY)
        pool["eye"], pool["dir"] = (-5.0, 0.0, 0.0), (1.0, 0.0, 0.0)
        pool["eye"][:, 1] = np.linspace(-0.2, 0.2, 8, dtype=np.float32)
        pool["dir"][5:] = (0.0, 1.0, 0.0)
        deepest = int(e.oracle.trace(scene, pool, depths=True)[2].max())
        below = int(e.oracle.trace(chain_scene(e.oracle, 122), pool, depths=True)[2].max())
        assert below <= 128 < deepest, (below, deepest)          # the oracle's shared far-only depth: the unit of the header's 128
    else:
        scene, pool = _trace40(e)
    wide, narrow = "wide" in form, scene                       # the oracle walks the narrow nodes: same records (include/voidin_abi.h)
    if wide:
        scene = (widen(scene[0]),) + tuple(scene[1:])
    tight = 1 if "tight 1" in form else 2 if "tight" in form else 0
    if "auto_prepare = 0" in form:
        e.opt("trace.auto_prepare", 0)
    for n in ([65] if deep else N_RAYS):
        rays = np.resize(pool, n)
        want, _ = e.oracle.trace(narrow, rays)
        assert deep or n < 2 or 0 < int(want["hit"].sum()) < n
        fs = Fences()
        s, _ = _fenced_scene(fs, scene, wide)
        r, hits, flags = fs.inp("rays", rays), fs.out("d_out", n * 16), fs.out("d_out_hit", n * 4)
        tag = f"{form} n_rays={n}"
        if "prepared" in form:
            acc = C.c_void_p()
            e.opt("trace.tight_tlas", tight)
            e.ok("vd_trace_prepare_wide_dev" if wide else "vd_trace_prepare_dev", s, C.byref(acc))
            e.opt("trace.tight_tlas", 0)
            try:
                e.ok("vd_trace_prepared_dev", acc, r.ptr, n, hits.ptr)
                e.ok("vd_trace_any_prepared_dev", acc, r.ptr, n, flags.ptr)
            finally:
                e.lib.vd_trace_release(e.h, acc)
        else:
            e.ok("vd_trace_wide_dev" if wide else "vd_trace_dev", s, r.ptr, n, hits.ptr)
            e.ok("vd_trace_any_wide_dev" if wide else "vd_trace_any_dev", s, r.ptr, n, flags.ptr)
        _check_hits(hits.read(abi.HIT), want, tight == 0, tag)
        assert np.array_equal(flags.read(np.uint32), want["hit"]), tag
        fs.check()


@case("vd_trace_accel_update_dev", "vd_trace_accel_refit_dev", "vd_trace_accel_update_geometry_dev", params=["narrow, tight 1", "narrow, tight 2", "wide, tight"])
def trace_accel_maintenance(e, form):
    """update / refit / update_geometry write the accel's private memory: every buffer of the scene is unchanged by each call, and the
    accel still gives the oracle's hits afterwards."""
    scene, pool = _trace40(e)
    wide = form.startswith("wide")
    if wide:
        scene = (widen(scene[0]),) + tuple(scene[1:])
    rays = np.resize(pool, 257)
    want, _ = e.oracle.trace(_trace40(e)[0], rays)
    fs = Fences()
    s, _ = _fenced_scene(fs, scene, wide)
    r, hits = fs.inp("rays", rays), fs.out("d_out", len(rays) * 16)
    acc = C.c_void_p()
    e.opt("trace.tight_tlas", 1 if form.endswith("1") else 2)
    e.ok("vd_trace_prepare_wide_dev" if wide else "vd_trace_prepare_dev", s, C.byref(acc))
    e.opt("trace.tight_tlas", 0)
    try:
        for name in ("vd_trace_accel_refit_dev", "vd_trace_accel_update_dev", "vd_trace_accel_update_geometry_dev"):
            e.ok(name, acc)
            fs.check()
            assert hits.fill_intact(0), name
        e.ok("vd_trace_prepared_dev", acc, r.ptr, len(rays), hits.ptr)
    finally:
        e.lib.vd_trace_release(e.h, acc)
    _check_hits(hits.read(abi.HIT), want, False, form)
    fs.check()


# ---- ray generators and the one-mesh walks ---------------------------------------------------------------------------------------

@case("vd_primary_rays_dev", params=["1x1", "5x3", "65x1"])
def primary_rays(e, shape):
    """exactly width * height rays of 32 bytes."""
    w, h = (int(x) for x in shape.split("x"))
    cam = synth.camera_uniform(eye=(0, 0, 15), pitch_deg=0)
    fs = Fences()
    c, out = _cam(fs, cam), fs.out("d_rays", w * h * 32)
    e.ok("vd_primary_rays_dev", c.ptr, w, h, out.ptr)
    _eq(out.read(), e.oracle.primary_rays(cam, w, h), f"primary rays {shape}")
    fs.check()


@case("vd_shadow_rays_dev", "vd_traverse_iter_dev", "vd_traverse_dev", params=[1, 63, 64, 65, 257])
def rays_and_walks(e, n):
    """32 bytes per shadow ray; 4 bytes per distance of the two one-mesh walks; every input unchanged."""
    u = synth.uniform01(synth.SEED_BASE + 33, 0, 6 * n).reshape(n, 6).astype(np.float32)
    pos, nor, light = np.ascontiguousarray(u[:, :3] * 10), np.ascontiguousarray(u[:, 3:] - np.float32(0.5)), np.array([3.0, 40.0, 20.0], np.float32)
    fs = Fences()
    p, q, l, out = fs.inp("d_positions", pos), fs.inp("d_normals", nor), fs.inp("light_position", light, host=True), fs.out("d_rays", n * 32)
    e.ok("vd_shadow_rays_dev", p.ptr, q.ptr, n, C.cast(l.ptr, C.POINTER(C.c_float)), out.ptr)
    _eq(out.read(), e.oracle.shadow_rays(pos, nor, light), f"shadow rays n={n}")
    fs.check()
    g = golden("harness_soup64.npz")
    nodes, v, idx = g["nodes"], g["vertices"].astype(np.float32), g["indices"].astype(np.uint32)
    rays = np.resize(g["rays"], n)
    for name in ("vd_traverse_iter_dev", "vd_traverse_dev"):
        fs = Fences()
        d_n, d_v, d_i, d_r, out = fs.inp("d_nodes", nodes), fs.inp("d_verts_xyz", v), fs.inp("d_indices", idx), fs.inp("d_rays", rays), fs.out("d_out_dist", n * 4)
        if name == "vd_traverse_iter_dev":
            e.ok(name, d_n.ptr, len(nodes), d_v.ptr, d_i.ptr, d_r.ptr, n, out.ptr)
            want = e.oracle.traverse_iter(nodes, v, idx, rays)
        else:
            e.ok(name, d_n.ptr, len(nodes), d_v.ptr, d_i.ptr, d_r.ptr, n, C.c_float(14.0), out.ptr)
            want = e.oracle.traverse_recursive(nodes, v, idx, rays, t0=14.0)
        _eq(out.read(), want, f"{name} n={n}")
        fs.check()


# ---- instance animation, the stream-side store -----------------------------------------------------------------------------------

@case("vd_compute_update_dev", params=[1, 1667])
def compute_update(e, n_indices):
    """Only the listed records change (an index out of range is dropped): transform, and inv_transform with fix_inverse only."""
    inst = synth.instances(5000, seed=synth.SEED_BASE + 9, extent=60.0)
    ids = np.arange(0, 5000, 3, dtype=np.uint32)[:n_indices].copy()
    assert len(ids) == n_indices
    if n_indices > 5:
        ids[5] = 999_999
    for fix in (0, 1):
        want = e.oracle.compute_update(ids, inst, 1.7, 0.016, bool(fix))
        fs = Fences()
        d_ids, d_i = fs.inp("d_indices", ids), fs.inp("d_instances", inst)
        e.ok("vd_compute_update_dev", d_ids.ptr, n_indices, d_i.ptr, 5000, C.c_float(1.7), C.c_float(0.016), fix)
        got = d_i.read(abi.INSTANCE)
        _eq(got, want, f"compute_update n_indices={n_indices} fix_inverse={fix}")
        assert got.tobytes() != inst.tobytes()
        if not fix:
            assert got["inv_transform"].tobytes() == inst["inv_transform"].tobytes()
        may = np.zeros((5000, 144), bool)
        may[ids[ids < 5000], : 128 if fix else 64] = True
        fs.check(allowed={"d_instances": may.reshape(-1)})


@case("vd_write_value32_async")
def write_value32(e, _):
    """four bytes."""
    fs = Fences()
    w = fs.out("d_word", 4)
    e.ok("vd_write_value32_async", w.ptr, 0x12345678)
    assert _u32(w) == 0x12345678
    fs.check()


# ---- host-pointer forms: one small ragged size each, every argument in a host fence ----------------------------------------------

def _host(fs):
    """Fences whose buffers all live in host memory."""
    fs.device = "host"
    return fs


@case("vd_cull_emit", "vd_cull_compact", "vd_cull_compact_views", "vd_cull_batch", "vd_cull_compact_hiz", "vd_cull_compact_lod")
def host_cull_forms(e, _):
    """As the device forms write: n commands / [0, count) + the count (pad_tail: zeroes up to n_inst) / n_mesh commands and [0, count) ids."""
    n = 1237
    cam, meshes, inst = _cull_scene(n)
    want = e.oracle.cull_emit(cam, meshes, inst)
    wc, k = e.oracle.compact(want)
    fs = _host(Fences())
    c, m, i, out = _cam(fs, cam), fs.inp("meshes", meshes), fs.inp("instances", inst), fs.out("out", n * 20)
    e.ok("vd_cull_emit", c.ptr, m.ptr, len(meshes), i.ptr, n, out.ptr)
    _eq(out.read(), want, "vd_cull_emit")
    fs.check()
    for pad in (0, 1):
        fs = _host(Fences())
        c, m, i, out, cnt = _cam(fs, cam), fs.inp("meshes", meshes), fs.inp("instances", inst), fs.out("out", n * 20), fs.out("out_count", 4)
        e.ok("vd_cull_compact", c.ptr, m.ptr, len(meshes), i.ptr, n, out.ptr, cnt.ptr, pad)
        assert _u32(cnt) == k
        _eq(out.read()[: k * 20], wc[:k], f"vd_cull_compact pad={pad}")
        if pad:
            assert not out.read()[k * 20:].any()
        else:
            out.check_fill(k * 20)
        fs.check()
    cams = np.stack([synth.camera_uniform(yaw_deg=y) for y in (0.0, 90.0)]).reshape(-1)
    stride = n + 3
    fs = _host(Fences())
    c, m, i, out, cnt = _cam(fs, cams, "cameras"), fs.inp("meshes", meshes), fs.inp("instances", inst), fs.out("out", 2 * stride * 20), fs.out("out_counts", 8)
    e.ok("vd_cull_compact_views", c.ptr, 2, m.ptr, len(meshes), i.ptr, n, out.ptr, stride, cnt.ptr, 0)
    for v in range(2):
        wv, kv = e.oracle.compact(e.oracle.cull_emit(cams[v], meshes, inst))
        assert cnt.read(np.uint32)[v] == kv
        _eq(out.read()[v * stride * 20: (v * stride + kv) * 20], wv[:kv], f"vd_cull_compact_views view {v}")
        out.check_fill((v * stride + kv) * 20, (v + 1) * stride * 20)
    fs.check()
    cmds, ids = _regroup(want["instance_count"] != 0, inst["mesh"], meshes)
    fs = _host(Fences())
    c, m, i = _cam(fs, cam), fs.inp("meshes", meshes), fs.inp("instances", inst)
    o_c, o_i, cnt = fs.out("out_cmds", len(meshes) * 20), fs.out("out_instance_ids", n * 4), fs.out("out_count", 4)
    e.ok("vd_cull_batch", c.ptr, m.ptr, len(meshes), i.ptr, n, o_c.ptr, o_i.ptr, cnt.ptr)
    assert _u32(cnt) == len(ids)
    _eq(o_c.read(), cmds, "vd_cull_batch commands")
    _eq(o_i.read()[: 4 * len(ids)], ids, "vd_cull_batch ids")
    o_i.check_fill(4 * len(ids))
    fs.check()
    # occlusion-culled list
    w, h = 100, 37
    ocam, omeshes, oinst = K.camera(), K.meshes_for(16), K.cloud(n)
    pyr = e.oracle.hiz_build(K.depth(w, h))
    draws, F, V = K.oracle_sets(e.oracle, ocam, omeshes, oinst, pyr, w, h)
    lst = K.select(draws, V)
    fs = _host(Fences())
    c, m, i, p = _cam(fs, ocam), fs.inp("meshes", omeshes), fs.inp("instances", oinst), fs.inp("pyramid", pyr)
    out, cnt = fs.out("out", n * 20), fs.out("out_count", 4)
    e.ok("vd_cull_compact_hiz", c.ptr, m.ptr, len(omeshes), i.ptr, n, p.ptr, w, h, out.ptr, cnt.ptr, 0)
    assert _u32(cnt) == len(lst)
    _eq(out.read()[: len(lst) * 20], lst, "vd_cull_compact_hiz")
    out.check_fill(len(lst) * 20)
    fs.check()
    # level of detail
    lcam, P, base, lmeshes, groups, linst = lod_cases.scene(e.oracle, n)
    x = lod_cases.expect(e.oracle, lcam, P, base, lmeshes, groups, linst)
    fs = _host(Fences())
    c, g, m, i = _cam(fs, lcam), fs.inp("groups", groups), fs.inp("meshes", lmeshes), fs.inp("instances", linst)
    out, cnt = fs.out("out", n * 20), fs.out("out_count", 4)
    e.ok("vd_cull_compact_lod", c.ptr, abi.lod_params(P), g.ptr, len(groups), m.ptr, len(lmeshes), i.ptr, n, out.ptr, cnt.ptr, 0)
    assert _u32(cnt) == len(x["list"])
    _eq(out.read()[: len(x["list"]) * 20], x["list"], "vd_cull_compact_lod")
    out.check_fill(len(x["list"]) * 20)
    fs.check()


@case("vd_bvh_build", "vd_bvh_build_batch", "vd_bvh_build_lbvh", "vd_bvh_build_lbvh_batch", "vd_bvh_refit")
def host_blas_forms(e, _):
    """A staging copy sized by a capacity instead of a count shows up here: node arrays with 37 spare nodes keep their fill."""
    n_tri = 77
    v, i = _soup(n_tri)
    wn, wi = e.oracle.bvh_build(v, i)
    cap = 2 * n_tri + 37
    fs = _host(Fences())
    d_v, d_i, d_n, nn = fs.inp("verts_xyz", v), fs.inout("indices_inout", i), fs.out("out_nodes", cap * 32), fs.out("out_n_nodes", 4)
    e.ok("vd_bvh_build", d_v.ptr, len(v), d_i.ptr, n_tri, d_n.ptr, cap, nn.ptr)
    assert _u32(nn) == len(wn)
    got = d_n.read(abi.BVH_NODE, len(wn))
    assert fields_equal(got, wn), first_difference(got, wn)
    _eq(d_i.read(), wi, "vd_bvh_build indices")
    d_n.check_fill(len(wn) * 32)
    fs.check()
    # batch, packed behind 11 nodes
    meshes = [_soup(t) for t in (3, 77, 513)]
    want = [e.oracle.bvh_build(a, b) for a, b in meshes]
    fs = _host(Fences())
    items, bufs = _batch_items(fs, meshes, own=False)
    first, pcap = 11, 11 + sum(2 * (len(b) // 3) for _, b in meshes) + 37
    packed = fs.out("packed_nodes", pcap * 32)
    h_items, end = fs.inout("items", np.frombuffer(bytes(items), np.uint8)), fs.out("out_packed_end", 4)
    e.ok("vd_bvh_build_batch", h_items.ptr, 3, packed.ptr, pcap, first, end.ptr)
    after = (abi.BvhBatchItem * 3).from_buffer_copy(h_items.read().tobytes())
    _batch_items_check(items, after, 3)
    at = first
    for m, (xn, xi) in enumerate(want):
        assert after[m].status == 0 and after[m].out_n_nodes == len(xn) and after[m].out_first_node == at
        got = packed.read(abi.BVH_NODE)[at: at + len(xn)]
        assert fields_equal(got, xn), (m, first_difference(got, xn))
        _eq(bufs[m][1].read(), xi, f"vd_bvh_build_batch mesh {m}: indices")
        at += len(xn)
    assert _u32(end) == at
    packed.check_fill(0, first * 32)
    packed.check_fill(at * 32)
    fs.check()
    # LBVH, single and batched
    ref = lbvh_reference(v, i)
    fs = _host(Fences())
    d_v, d_i, d_n, nn = fs.inp("verts_xyz", v), fs.inout("indices_inout", i), fs.out("out_nodes", cap * 32), fs.out("out_n_nodes", 4)
    e.ok("vd_bvh_build_lbvh", d_v.ptr, len(v), d_i.ptr, n_tri, d_n.ptr, cap, nn.ptr)
    assert _u32(nn) == ref["n_nodes"]
    got = d_n.read(abi.BVH_NODE, ref["n_nodes"])
    assert fields_equal(got, ref["nodes"]), first_difference(got, ref["nodes"])
    _eq(d_i.read(), ref["indices"], "vd_bvh_build_lbvh indices")
    d_n.check_fill(ref["n_nodes"] * 32)
    fs.check()
    fs = _host(Fences())
    counts = np.array([3, 50, 0], np.uint32)
    lit = (abi.BvhLbvhBatchItem * 3)()
    lb = []
    for m, (a, b) in enumerate(meshes):
        tcap = len(b) // 3
        f_v, f_i, f_n = fs.inp(f"verts_xyz[{m}]", a), fs.inout(f"indices_inout[{m}]", b), fs.out(f"nodes[{m}]", (2 * tcap + 37) * 32)
        lit[m].verts_xyz, lit[m].indices_inout, lit[m].nodes, lit[m].mesh_info = f_v.ptr, f_i.ptr, f_n.ptr, None
        lit[m].n_vert, lit[m].tri_cap, lit[m].node_cap = len(a), tcap, 2 * tcap + 37
        lb.append((f_i, f_n))
    h_items, h_c, res = fs.inout("items", np.frombuffer(bytes(lit), np.uint8)), fs.inp("n_tri", counts), fs.out("results", 48)
    e.ok("vd_bvh_build_lbvh_batch", h_items.ptr, 3, h_c.ptr, res.ptr)
    results = res.read(abi.BVH_LBVH_RESULT)
    for m, (a, b) in enumerate(meshes):
        T = int(counts[m])
        f_i, f_n = lb[m]
        if T == 0:
            assert int(results[m]["n_nodes"]) == 0 and f_n.fill_intact(0)
            _eq(f_i.read(), b, f"vd_bvh_build_lbvh_batch mesh {m}: T == 0")
            continue
        r = lbvh_reference(a, b[: 3 * T])
        assert int(results[m]["n_nodes"]) == r["n_nodes"] and int(results[m]["max_depth"]) == r["max_depth"]
        got = f_n.read(abi.BVH_NODE, r["n_nodes"])
        assert fields_equal(got, r["nodes"]), (m, first_difference(got, r["nodes"]))
        f_n.check_fill(r["n_nodes"] * 32)
        _eq(f_i.read(), np.concatenate([r["indices"], b[3 * T:]]), f"vd_bvh_build_lbvh_batch mesh {m}: indices")
    fs.check()
    # refit
    v2 = deform(v, phase=0.4)
    fs = _host(Fences())
    d_v, d_i, d_n = fs.inp("verts_xyz", v2), fs.inp("indices", wi), fs.inp("nodes_inout", wn)
    e.ok("vd_bvh_refit", d_v.ptr, len(v2), d_i.ptr, n_tri, d_n.ptr, len(wn))
    want_r = refit_reference(v2, wi, wn)
    got = d_n.read(abi.BVH_NODE)
    assert fields_equal(got, want_r), first_difference(got, want_r)
    box = np.zeros(32, bool); box[0:12] = box[16:28] = True
    fs.check(allowed={"nodes_inout": np.tile(box, len(wn))})


@case("vd_tlas_build", "vd_tlas_build_wide", "vd_tlas_refit", "vd_tlas_build_lbvh", "vd_tlas_build_lbvh_wide")
def host_tlas_forms(e, _):
    """exactly (2n + 1) nodes of 32 / 48 bytes; the refit rewrites the same nodes in place; instances and meshes unchanged."""
    n = 77
    inst, meshes = _tlas_scene(n)
    want = e.oracle.tlas_build(inst, meshes)
    for name, dt in (("vd_tlas_build", abi.TLAS_NODE), ("vd_tlas_build_wide", abi.TLAS_NODE_WIDE), ("vd_tlas_build_lbvh", abi.TLAS_NODE), ("vd_tlas_build_lbvh_wide", abi.TLAS_NODE_WIDE)):
        fs = _host(Fences())
        i, m, out = fs.inp("instances", inst), fs.inp("meshes", meshes), fs.out("out_nodes", (2 * n + 1) * dt.itemsize)
        e.ok(name, i.ptr, n, m.ptr, len(meshes), out.ptr)
        got = out.read(dt)
        if "lbvh" in name:
            order = got["instance_idx"][1:n + 1].astype(np.int64)
            assert sorted(order.tolist()) == list(range(n)) and got["min"][1:n + 1].tobytes() == want["min"][1 + order].tobytes(), name
            assert e.oracle.tlas_refit(inst, meshes, got).tobytes() == got.tobytes(), name
        else:
            assert fields_equal(got, e.oracle.tlas_build(inst, meshes, wide=(dt == abi.TLAS_NODE_WIDE))), name
        fs.check()
    moved = inst.copy()
    moved["transform"][::3, 12:15] += np.float32(0.37)
    fs = _host(Fences())
    i, m, d_n = fs.inp("instances", moved), fs.inp("meshes", meshes), fs.inout("nodes_inout", want)
    e.ok("vd_tlas_refit", i.ptr, n, m.ptr, len(meshes), d_n.ptr)
    _eq(d_n.read(abi.TLAS_NODE), e.oracle.tlas_refit(moved, meshes, want), "vd_tlas_refit")
    fs.check()


@case("vd_trace", "vd_trace_wide", "vd_primary_rays", "vd_traverse_iter", "vd_traverse")
def host_trace_forms(e, _):
    """n_rays records of 16 bytes / width * height rays of 32 bytes / n_rays distances of 4 bytes; every input unchanged."""
    scene, pool = _trace40(e)
    n = 77
    rays = np.resize(pool, n)
    want, _ = e.oracle.trace(scene, rays)
    for wide in (False, True):
        fs = _host(Fences())
        s, _ = _fenced_scene(fs, (widen(scene[0]),) + tuple(scene[1:]) if wide else scene, wide)
        r, out = fs.inp("rays", rays), fs.out("out", n * 16)
        e.ok("vd_trace_wide" if wide else "vd_trace", s, r.ptr, n, out.ptr)
        _eq(out.read(abi.HIT), want, "vd_trace_wide" if wide else "vd_trace")
        fs.check()
    cam = synth.camera_uniform(eye=(0, 0, 15), pitch_deg=0)
    fs = _host(Fences())
    c, out = _cam(fs, cam), fs.out("rays", 11 * 7 * 32)
    e.ok("vd_primary_rays", c.ptr, 11, 7, out.ptr)
    _eq(out.read(), e.oracle.primary_rays(cam, 11, 7), "vd_primary_rays")
    fs.check()
    g = golden("harness_soup64.npz")
    nodes, v, idx = g["nodes"], g["vertices"].astype(np.float32), g["indices"].astype(np.uint32)
    rays = np.resize(g["rays"], n)
    for name in ("vd_traverse_iter", "vd_traverse"):
        fs = _host(Fences())
        d_n, d_v, d_i, d_r, out = fs.inp("nodes", nodes), fs.inp("verts_xyz", v), fs.inp("indices", idx), fs.inp("rays", rays), fs.out("out_dist", n * 4)
        if name == "vd_traverse_iter":
            e.ok(name, d_n.ptr, len(nodes), d_v.ptr, len(v), d_i.ptr, len(idx) // 3, d_r.ptr, n, out.ptr)
            want_d = e.oracle.traverse_iter(nodes, v, idx, rays)
        else:
            e.ok(name, d_n.ptr, len(nodes), d_v.ptr, len(v), d_i.ptr, len(idx) // 3, d_r.ptr, n, C.c_float(14.0), out.ptr)
            want_d = e.oracle.traverse_recursive(nodes, v, idx, rays, t0=14.0)
        _eq(out.read(), want_d, name)
        fs.check()


# ---- "A refused call writes nothing" ---------------------------------------------------------------------------------------------

@case("vd_cull_emit_dev", "vd_cull_compact_dev", "vd_cull_mask_dev", "vd_cull_compact_views_dev", "vd_occlusion_mask_dev", "vd_expand_mask_dev",
      "vd_tlas_build_dev", "vd_bvh_build_lbvh_dev")
def refused_calls_write_nothing(e, _):
    """VD_ERR_INVALID_ARG with valid fenced outputs - n_mesh == 0, out_stride < n_inst, a depth bound the triangle count cannot meet -
    and every payload keeps its fill."""
    n = 130
    cam, meshes, inst = _cull_scene(n)
    fs = Fences()
    c, m, i = _cam(fs, cam), fs.inp("meshes", meshes), fs.inp("instances", inst)
    out, cnt, mask = fs.out("d_out", 3 * n * 20), fs.out("d_out_count", 12), fs.out("d_mask", (n + 63) // 64 * 8)
    words, ids = fs.inp("d_mask_in", _mask_words(np.ones(n, bool))), fs.inp("d_mesh_ids", np.zeros(n, np.uint8))
    pyr = fs.inp("d_pyramid", e.oracle.hiz_build(K.depth(5, 3)))
    nodes = fs.out("d_out_nodes", (2 * n + 1) * 32)
    cams = fs.inp("cameras", np.stack([cam, cam]).reshape(-1), host=True)
    refused = [
        ("vd_cull_emit_dev", (c.ptr, m.ptr, 0, i.ptr, n, out.ptr)),
        ("vd_cull_compact_dev", (c.ptr, m.ptr, 0, i.ptr, n, out.ptr, cnt.ptr, 1)),
        ("vd_cull_mask_dev", (c.ptr, m.ptr, 0, i.ptr, n, mask.ptr)),
        ("vd_cull_compact_views_dev", (cams.ptr, 2, m.ptr, len(meshes), i.ptr, n, out.ptr, n - 1, cnt.ptr, 1)),
        ("vd_occlusion_mask_dev", (c.ptr, m.ptr, 0, i.ptr, n, pyr.ptr, 5, 3, words.ptr, mask.ptr)),
        ("vd_expand_mask_dev", (words.ptr, n, n, ids.ptr, 1, m.ptr, 0, out.ptr, cnt.ptr)),
        ("vd_tlas_build_dev", (i.ptr, n, m.ptr, 0, nodes.ptr)),
    ]
    for name, args in refused:
        assert e.call(name, *args) == abi.VD_ERR_INVALID_ARG, name
        for f in (out, cnt, mask, nodes):
            f.check_fill(0)
        fs.check()
    v, idx = _soup(5)
    e.opt("blas.lbvh_max_depth", 1)                          # 5 triangles > 2^(1 + 1)
    d_v, d_i, d_n, res = fs.inp("verts_xyz", v), fs.inp("indices_inout", idx), fs.out("out_nodes", 47 * 32), fs.out("d_result", 16)
    assert e.call("vd_bvh_build_lbvh_dev", d_v.ptr, len(v), d_i.ptr, 5, d_n.ptr, 47, res.ptr) == abi.VD_ERR_INVALID_ARG
    d_n.check_fill(0); res.check_fill(0)
    fs.check()


@pytest.mark.parametrize("case_id", list(CASES))
def test_write_set(ctx, oracle, ctx_options, case_id):
    fn, param = CASES[case_id]
    fn(Env(ctx, oracle, ctx_options), param)
