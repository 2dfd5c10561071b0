"""Host-side mirror of the reference's pass-graph / builder API over the C ABI.

Names follow the reference:
  EmitDraws.record      <- crates/app/src/pass/visibility.rs:233-254 (`impl Pass for EmitDraws`)
  BvhBuilder(...).build <- crates/bvh/src/blas.rs:51-103
  Tlas.build            <- crates/bvh/src/tlas.rs:31-85
  traverse_tlas         <- shaders/utils/bvh.wgsl:89-123

torch is plumbing only (device memory + streams); all compute is in libvoidin_hip.so.
There is no CPU fallback: constructing a Context without the HIP library or a gfx950 GPU raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi


class VoidinError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        super().__init__(f"{abi.STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


def _as_u8_tensor(arr: np.ndarray, device):
    import torch
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(device)


def to_numpy(t, dtype: np.dtype) -> np.ndarray:
    """uint8 device tensor -> structured numpy array."""
    return t.detach().cpu().numpy().view(dtype)


def set_ray_range(rays: np.ndarray, t_min, t_max) -> np.ndarray:
    """Fill the interval fields of a RAY array in place (scalars or one value per ray) and return it: `_pad0` = t_min, `_pad1` = t_max,
    which every trace call reads under the option "trace.ray_range" (VD_OPT_TRACE_RAY_RANGE, include/voidin_abi.h, "Ray intervals") and
    ignores without it.  (0, abi.MAX_DIST) is the whole half-line: the bytes a call without the option gives."""
    if rays.dtype != abi.RAY:
        raise TypeError("set_ray_range takes an array of abi.RAY")
    rays["_pad0"] = t_min
    rays["_pad1"] = t_max
    return rays


class Context:
    """One VdCtx bound to a device and (by default) torch's current HIP stream."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        self.lib = abi.load()
        h = C.c_void_p()
        rc = self.lib.vd_ctx_create(device, C.byref(h))
        if rc != abi.VD_OK:
            raise VoidinError(rc, "vd_ctx_create failed (need a gfx950 GPU; there is no CPU fallback)")
        self.h = h
        self.device = device
        import torch
        self.torch_device = torch.device("cuda", device)
        if use_torch_stream:
            self.set_stream(torch.cuda.current_stream(self.torch_device).cuda_stream)
        self.apply_env_options()

    def set_option(self, name: str, value: int | None):
        """vd_ctx_set_option (include/voidin_abi.h VdOption) by name, e.g. "tlas.spin_limit"; None = default."""
        self._chk(self.lib.vd_ctx_set_option(self.h, abi.OPTIONS[name], -1 if value is None else int(value)))

    def apply_env_options(self):
        """A/B scripts under tools/ select variants with VD_* environment variables; the LIBRARY reads none of them -
        this harness forwards them as per-context options when a Context is made."""
        import os
        for env, name in abi.OPTION_ENV.items():
            if os.environ.get(env) not in (None, ""):
                self.set_option(name, int(os.environ[env]))

    # -- plumbing -------------------------------------------------------------------------
    def _chk(self, rc: int):
        if rc != abi.VD_OK:
            raise VoidinError(rc, self.lib.vd_last_error(self.h).decode())

    def set_stream(self, hip_stream: int | None):
        self._chk(self.lib.vd_ctx_set_stream(self.h, hip_stream))

    def synchronize(self):
        self._chk(self.lib.vd_ctx_synchronize(self.h))

    def set_timing(self, enabled: bool):
        self._chk(self.lib.vd_ctx_set_timing(self.h, int(enabled)))

    def last_gpu_ms(self) -> float:
        return float(self.lib.vd_last_gpu_ms(self.h))

    def last_gpu_ms_stage(self, stage: int) -> float:
        return float(self.lib.vd_last_gpu_ms_stage(self.h, stage))

    def close(self):
        if getattr(self, "h", None):
            self.lib.vd_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, arr: np.ndarray):
        return _as_u8_tensor(arr, self.torch_device)

    def empty(self, nbytes: int):
        import torch
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.torch_device)

    # -- cull / emit (device pointers) ------------------------------------------------------
    def cull_emit_dev(self, camera: np.ndarray, d_meshes, n_mesh, d_inst, n_inst, d_out, first_instance=0):
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        self._chk(self.lib.vd_cull_emit_shard_dev(self.h, cam.ctypes.data, abi.ptr(d_meshes), n_mesh,
                                                  abi.ptr(d_inst), n_inst, first_instance, abi.ptr(d_out)))

    def cull_compact_dev(self, camera: np.ndarray, d_meshes, n_mesh, d_inst, n_inst, d_out, d_count,
                         pad_tail: bool = False, first_instance=0):
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        self._chk(self.lib.vd_cull_compact_shard_dev(self.h, cam.ctypes.data, abi.ptr(d_meshes), n_mesh,
                                                     abi.ptr(d_inst), n_inst, first_instance, abi.ptr(d_out),
                                                     abi.ptr(d_count), int(pad_tail)))

    def cull_compact_views_dev(self, cameras, d_meshes, n_mesh, d_inst, n_inst, d_out, d_counts, pad_tail: bool = False,
                               out_stride: int | None = None):
        """vd_cull_compact_views_dev: the instances are read once for all cameras (1..abi.MAX_VIEWS of them); view v's
        list goes to d_out[v * out_stride ...) (in commands; default n_inst = packed), its count to d_counts[v]."""
        cams = np.ascontiguousarray(cameras, dtype=abi.CAMERA).reshape(-1)
        self._chk(self.lib.vd_cull_compact_views_dev(self.h, cams.ctypes.data, len(cams), abi.ptr(d_meshes), n_mesh,
                                                     abi.ptr(d_inst), n_inst, abi.ptr(d_out),
                                                     n_inst if out_stride is None else int(out_stride), abi.ptr(d_counts),
                                                     int(pad_tail)))

    def cull_mask_dev(self, camera: np.ndarray, d_meshes, n_mesh, d_inst, n_inst, d_mask):
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        self._chk(self.lib.vd_cull_mask_dev(self.h, cam.ctypes.data, abi.ptr(d_meshes), n_mesh, abi.ptr(d_inst), n_inst,
                                            abi.ptr(d_mask)))

    def expand_mask_dev(self, d_mask, n_total, shard_size, d_mesh_ids, d_meshes, n_mesh, d_out, d_count, id_bytes=None):
        if id_bytes is None:
            id_bytes = d_mesh_ids.element_size() if hasattr(d_mesh_ids, "element_size") else 4
        self._chk(self.lib.vd_expand_mask_dev(self.h, abi.ptr(d_mask), n_total, shard_size, abi.ptr(d_mesh_ids), id_bytes,
                                              abi.ptr(d_meshes), n_mesh, abi.ptr(d_out), abi.ptr(d_count)))

    def mask_to_indices_dev(self, d_mask, n_inst, first_instance, d_out_indices, d_count):
        self._chk(self.lib.vd_mask_to_indices_dev(self.h, abi.ptr(d_mask), n_inst, first_instance, abi.ptr(d_out_indices), abi.ptr(d_count)))

    def indices_to_draws_dev(self, d_indices, n_indices, d_mesh_ids, n_total, d_meshes, n_mesh, d_out, id_bytes=None):
        if id_bytes is None:
            id_bytes = d_mesh_ids.element_size() if hasattr(d_mesh_ids, "element_size") else 4
        self._chk(self.lib.vd_indices_to_draws_dev(self.h, abi.ptr(d_indices), n_indices, abi.ptr(d_mesh_ids), id_bytes, n_total,
                                                   abi.ptr(d_meshes), n_mesh, abi.ptr(d_out)))

    # instanced draw lists: one command per mesh + the survivors' ids grouped by mesh (voidin_abi.h "Instanced draw lists")
    def batch_mask_dev(self, d_mask, n_inst, d_mesh_ids, d_meshes, n_mesh, d_out_cmds, d_out_instance_ids, d_count, id_bytes=None):
        """vd_batch_mask_dev: group the set bits of any visibility mask by mesh through a caller-supplied id table."""
        if id_bytes is None:
            id_bytes = d_mesh_ids.element_size() if hasattr(d_mesh_ids, "element_size") else 4
        self._chk(self.lib.vd_batch_mask_dev(self.h, abi.ptr(d_mask), n_inst, abi.ptr(d_mesh_ids), id_bytes, abi.ptr(d_meshes), n_mesh,
                                             abi.ptr(d_out_cmds), abi.ptr(d_out_instance_ids), abi.ptr(d_count)))

    def cull_batch_dev(self, camera: np.ndarray, d_meshes, n_mesh, d_inst, n_inst, d_out_cmds, d_out_instance_ids, d_count):
        """vd_cull_batch_dev: cull + group in one read of the instances; n_mesh commands, |S| ids, the count."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        self._chk(self.lib.vd_cull_batch_dev(self.h, cam.ctypes.data, abi.ptr(d_meshes), n_mesh, abi.ptr(d_inst), n_inst,
                                             abi.ptr(d_out_cmds), abi.ptr(d_out_instance_ids), abi.ptr(d_count)))

    # level of detail: the row of the mesh table an instance is drawn with (voidin_abi.h "Level of detail")
    def lod_ids_dev(self, camera, params, d_groups, n_group, n_mesh, d_inst, n_inst, d_out_ids, id_bytes=None):
        """vd_lod_ids_dev: d_out_ids[i] = the d_meshes row of instance i, for every instance (no visibility test)."""
        if id_bytes is None:
            id_bytes = d_out_ids.element_size() if hasattr(d_out_ids, "element_size") else 4
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        self._chk(self.lib.vd_lod_ids_dev(self.h, cam.ctypes.data, abi.lod_params(params), abi.ptr(d_groups), n_group, n_mesh,
                                          abi.ptr(d_inst), n_inst, abi.ptr(d_out_ids), id_bytes))

    def cull_compact_lod_dev(self, camera, params, d_groups, n_group, d_meshes, n_mesh, d_inst, n_inst, d_out, d_count,
                             pad_tail: bool = False):
        """vd_cull_compact_lod_dev: the ordered list of the drawn instances, each with the command of its LOD row."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        self._chk(self.lib.vd_cull_compact_lod_dev(self.h, cam.ctypes.data, abi.lod_params(params), abi.ptr(d_groups), n_group,
                                                   abi.ptr(d_meshes), n_mesh, abi.ptr(d_inst), n_inst, abi.ptr(d_out),
                                                   abi.ptr(d_count), int(pad_tail)))

    def cull_batch_lod_dev(self, camera, params, d_groups, n_group, d_meshes, n_mesh, d_inst, n_inst, d_out_cmds,
                           d_out_instance_ids, d_count):
        """vd_cull_batch_lod_dev: one command per row of d_meshes (mesh x LOD), the drawn instances' ids grouped by row."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        self._chk(self.lib.vd_cull_batch_lod_dev(self.h, cam.ctypes.data, abi.lod_params(params), abi.ptr(d_groups), n_group,
                                                 abi.ptr(d_meshes), n_mesh, abi.ptr(d_inst), n_inst, abi.ptr(d_out_cmds),
                                                 abi.ptr(d_out_instance_ids), abi.ptr(d_count)))

    def compact_draws_dev(self, d_in, n, d_out, d_count):
        self._chk(self.lib.vd_compact_draws_dev(self.h, abi.ptr(d_in), n, abi.ptr(d_out), abi.ptr(d_count)))

    def compute_update_dev(self, d_indices, n_indices, d_instances, n_instances, time, dt, fix_inverse=False):
        self._chk(self.lib.vd_compute_update_dev(self.h, abi.ptr(d_indices), n_indices, abi.ptr(d_instances), n_instances,
                                                 float(time), float(dt), int(fix_inverse)))

    # -- ordering through a shared word / the host (voidin_abi.h: "Ordering that WORKS on this platform") ------
    def wait_value32(self, d_word_ptr: int, value: int):
        self._chk(self.lib.vd_wait_value32_async(self.h, d_word_ptr, value))

    def write_value32(self, d_word_ptr: int, value: int):
        self._chk(self.lib.vd_write_value32_async(self.h, d_word_ptr, value))

    def host_callback(self, fn, user=None):
        """fn: a ctypes CFUNCTYPE(None, c_void_p) object the CALLER keeps alive until it has run."""
        self._chk(self.lib.vd_host_callback_async(self.h, fn, user))

    # -- cull / emit (host arrays) ----------------------------------------------------------
    def cull_emit(self, camera, meshes, instances) -> np.ndarray:
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        meshes = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
        instances = np.ascontiguousarray(instances, dtype=abi.INSTANCE)
        out = np.zeros(len(instances), dtype=abi.DRAW)
        self._chk(self.lib.vd_cull_emit(self.h, cam.ctypes.data, meshes.ctypes.data, len(meshes),
                                        instances.ctypes.data, len(instances), out.ctypes.data))
        return out

    def cull_compact(self, camera, meshes, instances, pad_tail=False):
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        meshes = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
        instances = np.ascontiguousarray(instances, dtype=abi.INSTANCE)
        out = np.zeros(len(instances), dtype=abi.DRAW)
        out.view(np.uint8)[:] = 0xAB  # poison: only [0,count) (or everything with pad_tail) is defined
        cnt = C.c_uint32(0)
        self._chk(self.lib.vd_cull_compact(self.h, cam.ctypes.data, meshes.ctypes.data, len(meshes),
                                           instances.ctypes.data, len(instances), out.ctypes.data,
                                           C.addressof(cnt), int(pad_tail)))
        return out, cnt.value

    def cull_compact_lod(self, camera, params, groups, meshes, instances, pad_tail=False):
        """Host arrays in, (list, count) out; the group table is validated (VD_ERR_INVALID_ARG).  Only [0, count) is
        defined (everything with pad_tail)."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        groups = np.ascontiguousarray(groups, dtype=abi.LOD_GROUP)
        meshes = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
        instances = np.ascontiguousarray(instances, dtype=abi.INSTANCE)
        out = np.zeros(len(instances), dtype=abi.DRAW)
        out.view(np.uint8)[:] = 0xAB
        cnt = C.c_uint32(0)
        self._chk(self.lib.vd_cull_compact_lod(self.h, cam.ctypes.data, abi.lod_params(params), groups.ctypes.data, len(groups),
                                               meshes.ctypes.data, len(meshes), instances.ctypes.data, len(instances),
                                               out.ctypes.data, C.addressof(cnt), int(pad_tail)))
        return out, cnt.value

    def cull_batch(self, camera, meshes, instances):
        """Host arrays in; (cmds [n_mesh], ids[:count], count) out: one command per mesh, the survivors' ids grouped by mesh."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA)
        meshes = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
        instances = np.ascontiguousarray(instances, dtype=abi.INSTANCE)
        cmds = np.zeros(len(meshes), dtype=abi.DRAW)
        ids = np.full(max(len(instances), 1), 0xABABABAB, dtype=np.uint32)      # poison: only [0, count) is defined
        cnt = C.c_uint32(0)
        self._chk(self.lib.vd_cull_batch(self.h, cam.ctypes.data, meshes.ctypes.data, len(meshes), instances.ctypes.data,
                                         len(instances), cmds.ctypes.data, ids.ctypes.data, C.addressof(cnt)))
        return cmds, ids[:cnt.value], cnt.value

    def cull_compact_views(self, cameras, meshes, instances, pad_tail=False):
        """Host arrays in, (lists [n_views, n_inst], counts [n_views]) out; only [0, count) of a list is defined
        (everything with pad_tail)."""
        cams = np.ascontiguousarray(cameras, dtype=abi.CAMERA).reshape(-1)
        meshes = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
        instances = np.ascontiguousarray(instances, dtype=abi.INSTANCE)
        out = np.zeros((len(cams), len(instances)), dtype=abi.DRAW)
        out.view(np.uint8)[:] = 0xAB
        cnt = np.zeros(len(cams), dtype=np.uint32)
        self._chk(self.lib.vd_cull_compact_views(self.h, cams.ctypes.data, len(cams), meshes.ctypes.data, len(meshes),
                                                 instances.ctypes.data, len(instances), out.ctypes.data, len(instances),
                                                 cnt.ctypes.data, int(pad_tail)))
        return out, cnt

    # -- BLAS -------------------------------------------------------------------------------
    def bvh_build(self, verts, indices):
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        idx = np.array(indices, dtype=np.uint32).reshape(-1).copy()
        n_tri = len(idx) // 3
        nodes = np.zeros(max(2 * n_tri, 2), dtype=abi.BVH_NODE)
        n_nodes = C.c_uint32(0)
        self._chk(self.lib.vd_bvh_build(self.h, verts.ctypes.data, len(verts), idx.ctypes.data, n_tri,
                                        nodes.ctypes.data, len(nodes), C.addressof(n_nodes)))
        return nodes[:n_nodes.value].copy(), idx

    def bvh_build_dev(self, d_verts, n_vert, d_indices, n_tri, d_nodes, node_cap) -> int:
        n_nodes = C.c_uint32(0)
        self._chk(self.lib.vd_bvh_build_dev(self.h, abi.ptr(d_verts), n_vert, abi.ptr(d_indices), n_tri,
                                            abi.ptr(d_nodes), node_cap, C.addressof(n_nodes)))
        return n_nodes.value

    def bvh_build_lbvh(self, verts, indices):
        """vd_bvh_build_lbvh, host arrays: the LBVH bottom level (NOT the reference's tree; voidin_abi.h "LBVH bottom level")
        -> (nodes, indices in sorted code order)."""
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        idx = np.array(indices, dtype=np.uint32).reshape(-1).copy()
        n_tri = len(idx) // 3
        nodes = np.zeros(max(2 * n_tri, 2), dtype=abi.BVH_NODE)
        n_nodes = C.c_uint32(0)
        self._chk(self.lib.vd_bvh_build_lbvh(self.h, verts.ctypes.data, len(verts), idx.ctypes.data, n_tri,
                                             nodes.ctypes.data, len(nodes), C.addressof(n_nodes)))
        return nodes[:n_nodes.value].copy(), idx

    def bvh_build_lbvh_dev(self, d_verts, n_vert, d_indices, n_tri, d_nodes, node_cap, d_result):
        """vd_bvh_build_lbvh_dev: enqueues only; d_result: 16 bytes of DEVICE memory for {n_nodes, n_bad_indices, max_depth, _pad}."""
        self._chk(self.lib.vd_bvh_build_lbvh_dev(self.h, abi.ptr(d_verts), n_vert, abi.ptr(d_indices), n_tri,
                                                 abi.ptr(d_nodes), node_cap, abi.ptr(d_result)))

    # Batched LBVH bottom level: many meshes per call, the triangle counts on the device (voidin_abi.h "Batched LBVH bottom level")
    class BvhLbvhPlan:
        """vd_bvh_lbvh_plan_dev: the layout of K meshes - pointers and capacities - validated once, with all work memory of their
        build.  `items` is an (abi.BvhLbvhBatchItem * K) with device pointers (a failed plan leaves the offending item's status
        set); the plan keeps those pointers, so the caller keeps the tensors alive."""

        def __init__(self, ctx: "Context", items, n_items=None):
            self.ctx, self.items = ctx, items
            self.n_items = len(items) if n_items is None else int(n_items)
            h = C.c_void_p()
            ctx._chk(ctx.lib.vd_bvh_lbvh_plan_dev(ctx.h, C.addressof(items) if self.n_items else None, self.n_items, C.byref(h)))
            self.h = h

        def build(self, d_n_tri, d_results):
            self.ctx.bvh_build_lbvh_planned_dev(self, d_n_tri, d_results)

        def close(self):
            if getattr(self, "h", None):
                self.ctx.lib.vd_bvh_lbvh_plan_release(self.ctx.h, self.h)
                self.h = None

        def __del__(self):
            try:
                self.close()
            except Exception:
                pass

    def bvh_lbvh_plan(self, items, n_items=None) -> "Context.BvhLbvhPlan":
        return Context.BvhLbvhPlan(self, items, n_items)

    def bvh_build_lbvh_planned_dev(self, plan: "Context.BvhLbvhPlan", d_n_tri, d_results):
        """vd_bvh_build_lbvh_planned_dev: enqueues the build of every mesh of the plan.  d_n_tri: K uint32 counts in DEVICE memory
        (None = every tri_cap); d_results: 16 * K bytes of DEVICE memory."""
        self._chk(self.lib.vd_bvh_build_lbvh_planned_dev(self.h, plan.h, abi.ptr(d_n_tri) if d_n_tri is not None else None, abi.ptr(d_results)))

    def bvh_build_lbvh_batch(self, meshes, n_tri=None, mesh_infos=None):
        """vd_bvh_build_lbvh_batch, host arrays.  meshes: [(vertices (V,3) f32, indices (3 * tri_cap,) u32)]; n_tri: per mesh, the
        triangles to build from (None = all; above the capacity = all); mesh_infos: None, or per mesh None / a 1-element
        abi.MESH_INFO array whose min / max are refreshed in place.  -> [(nodes, indices with the first 3 T permuted, result)].
        A mesh with an index >= n_vert raises VD_ERR_INVALID_ARG; `.items` of the error names it by status."""
        K = len(meshes)
        items = (abi.BvhLbvhBatchItem * max(K, 1))()
        keep = []
        for m, (v, i) in enumerate(meshes):
            v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
            idx = np.array(i, dtype=np.uint32).reshape(-1).copy()
            cap = len(idx) // 3
            nodes = np.zeros(max(2 * cap, 2), dtype=abi.BVH_NODE)
            keep.append((v, idx, nodes))
            items[m].verts_xyz, items[m].indices_inout, items[m].nodes = v.ctypes.data, idx.ctypes.data, nodes.ctypes.data
            info = None if mesh_infos is None else mesh_infos[m]
            items[m].mesh_info = None if info is None else info.ctypes.data
            items[m].n_vert, items[m].tri_cap, items[m].node_cap = len(v), cap, len(nodes)
        counts = None if n_tri is None else np.ascontiguousarray(n_tri, dtype=np.uint32)
        assert counts is None or len(counts) == K
        results = np.zeros(max(K, 1), dtype=abi.BVH_LBVH_RESULT)
        try:
            self._chk(self.lib.vd_bvh_build_lbvh_batch(self.h, C.addressof(items), K, None if counts is None else counts.ctypes.data, results.ctypes.data))
        except VoidinError as e:
            e.items = items
            raise
        return [(keep[m][2][: int(results[m]["n_nodes"])].copy(), keep[m][1], results[m].copy()) for m in range(K)]

    def bvh_build_batch(self, meshes, packed=True):
        """K meshes in ONE build (vd_bvh_build_batch; MeshPool::add for a whole scene, mesh/mod.rs:309-351).
        meshes: [(vertices (V,3) f32, indices (3T,) u32)].  packed: one shared node array, each mesh's nodes behind the
        previous mesh's -> (nodes, [(first_node, n_nodes, permuted indices)]); else [(nodes, permuted indices)]."""
        K = len(meshes)
        items = (abi.BvhBatchItem * K)()
        keep = []
        for m, (v, i) in enumerate(meshes):
            v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
            idx = np.array(i, dtype=np.uint32).reshape(-1).copy()
            n_tri = len(idx) // 3
            own = None if packed else np.zeros(max(2 * n_tri, 2), dtype=abi.BVH_NODE)
            keep.append((v, idx, own))
            items[m].verts_xyz, items[m].indices_inout = v.ctypes.data, idx.ctypes.data
            items[m].out_nodes = None if packed else own.ctypes.data
            items[m].n_vert, items[m].n_tri, items[m].node_cap = len(v), n_tri, 0 if packed else len(own)
        cap = sum(max(2 * (len(k[1]) // 3), 2) for k in keep) if packed else 0
        shared = np.zeros(max(cap, 1), dtype=abi.BVH_NODE)
        end = C.c_uint32(0)
        self._chk(self.lib.vd_bvh_build_batch(self.h, C.addressof(items), K, shared.ctypes.data if packed else None, cap, 0, C.addressof(end)))
        if packed:
            return shared[: end.value].copy(), [(int(items[m].out_first_node), int(items[m].out_n_nodes), keep[m][1]) for m in range(K)]
        return [(keep[m][2][: items[m].out_n_nodes].copy(), keep[m][1]) for m in range(K)]

    def bvh_build_batch_dev(self, items, n_items, d_packed=None, packed_cap=0, packed_first=0) -> int:
        """items: (abi.BvhBatchItem * K) with device pointers; returns one past the last packed node."""
        end = C.c_uint32(0)
        self._chk(self.lib.vd_bvh_build_batch_dev(self.h, C.addressof(items), n_items, abi.ptr(d_packed) if d_packed is not None else None,
                                                  packed_cap, packed_first, C.addressof(end)))
        return end.value

    # BLAS refit: new boxes for deformed vertices, same topology (voidin_abi.h "BLAS refit")
    def bvh_refit(self, verts, indices, nodes) -> np.ndarray:
        """vd_bvh_refit, host arrays, one mesh: `indices` as the build permuted them; returns the nodes with min / max
        recomputed for `verts` (refit(build(x), x) == build(x) bit for bit)."""
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        nodes = np.array(nodes, dtype=abi.BVH_NODE, copy=True)
        self._chk(self.lib.vd_bvh_refit(self.h, verts.ctypes.data, len(verts), idx.ctypes.data, len(idx) // 3,
                                        nodes.ctypes.data, len(nodes)))
        return nodes

    class BvhRefitPlan:
        """vd_bvh_refit_plan_dev: what a refit needs from the topology of K meshes, derived and validated once.  `items` is an
        (abi.BvhRefitItem * K) with device pointers (a failed plan leaves the offending item's status set); the plan keeps
        those pointers, so the caller keeps the tensors alive."""

        def __init__(self, ctx: "Context", items, n_items=None):
            self.ctx, self.items = ctx, items
            self.n_items = len(items) if n_items is None else int(n_items)
            h = C.c_void_p()
            ctx._chk(ctx.lib.vd_bvh_refit_plan_dev(ctx.h, C.addressof(items) if self.n_items else None, self.n_items, C.byref(h)))
            self.h = h

        def refit(self):
            self.ctx.bvh_refit_planned(self)

        def close(self):
            if getattr(self, "h", None):
                self.ctx.lib.vd_bvh_refit_plan_release(self.ctx.h, self.h)
                self.h = None

        def __del__(self):
            try:
                self.close()
            except Exception:
                pass

    def bvh_refit_plan(self, items, n_items=None) -> "Context.BvhRefitPlan":
        return Context.BvhRefitPlan(self, items, n_items)

    def bvh_refit_planned(self, plan: "Context.BvhRefitPlan"):
        """vd_bvh_refit_planned_dev: one kernel for all meshes of the plan, enqueued on the context's stream."""
        self._chk(self.lib.vd_bvh_refit_planned_dev(self.h, plan.h))

    def bvh_refit_plan_release(self, plan: "Context.BvhRefitPlan"):
        plan.close()

    def bvh_last_build_stats(self) -> dict:
        st = abi.BvhBuildStats()
        self._chk(self.lib.vd_bvh_last_build_stats(self.h, C.byref(st)))
        return {k: (round(getattr(st, k), 3) if t is C.c_float else int(getattr(st, k))) for k, t in st._fields_}

    # -- TLAS -------------------------------------------------------------------------------
    def tlas_build(self, instances, meshes, wide=False) -> np.ndarray:
        instances = np.ascontiguousarray(instances, dtype=abi.INSTANCE)
        meshes = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
        out = np.zeros(2 * len(instances) + 1, dtype=abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE)
        fn = self.lib.vd_tlas_build_wide if wide else self.lib.vd_tlas_build
        self._chk(fn(self.h, instances.ctypes.data, len(instances), meshes.ctypes.data, len(meshes),
                     out.ctypes.data))
        return out

    def tlas_refit(self, instances, meshes, nodes) -> np.ndarray:
        instances = np.ascontiguousarray(instances, dtype=abi.INSTANCE)
        meshes = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
        nodes = np.array(nodes, dtype=abi.TLAS_NODE, copy=True)
        self._chk(self.lib.vd_tlas_refit(self.h, instances.ctypes.data, len(instances), meshes.ctypes.data,
                                         len(meshes), nodes.ctypes.data))
        return nodes

    def tlas_build_dev(self, d_inst, n, d_meshes, n_mesh, d_nodes, wide=False):
        fn = self.lib.vd_tlas_build_wide_dev if wide else self.lib.vd_tlas_build_dev
        self._chk(fn(self.h, abi.ptr(d_inst), n, abi.ptr(d_meshes), n_mesh, abi.ptr(d_nodes)))

    def tlas_refit_dev(self, d_inst, n, d_meshes, n_mesh, d_nodes, wide=False):
        fn = self.lib.vd_tlas_refit_wide_dev if wide else self.lib.vd_tlas_refit_dev
        self._chk(fn(self.h, abi.ptr(d_inst), n, abi.ptr(d_meshes), n_mesh, abi.ptr(d_nodes)))

    def tlas_build_lbvh(self, instances, meshes, wide=False) -> np.ndarray:
        """vd_tlas_build_lbvh[_wide]: the LBVH top level (2n + 1 nodes, layout in include/voidin_abi.h), host arrays."""
        instances = np.ascontiguousarray(instances, dtype=abi.INSTANCE)
        meshes = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
        out = np.zeros(2 * len(instances) + 1, dtype=abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE)
        fn = self.lib.vd_tlas_build_lbvh_wide if wide else self.lib.vd_tlas_build_lbvh
        self._chk(fn(self.h, instances.ctypes.data, len(instances), meshes.ctypes.data, len(meshes), out.ctypes.data))
        return out

    def tlas_build_lbvh_dev(self, d_inst, n, d_meshes, n_mesh, d_nodes, wide=False):
        fn = self.lib.vd_tlas_build_lbvh_wide_dev if wide else self.lib.vd_tlas_build_lbvh_dev
        self._chk(fn(self.h, abi.ptr(d_inst), n, abi.ptr(d_meshes), n_mesh, abi.ptr(d_nodes)))

    # -- traversal ----------------------------------------------------------------------------
    def trace(self, scene_arrays, rays) -> np.ndarray:
        """scene_arrays = (tlas_nodes, instances, meshes, bvh_nodes, vertices, indices), host."""
        dts = [abi.TLAS_NODE, abi.INSTANCE, abi.MESH_INFO, abi.BVH_NODE, np.float32, np.uint32]
        arrs = [np.ascontiguousarray(a, dtype=d).reshape(-1) for a, d in zip(scene_arrays, dts)]
        s = abi.TraceScene()
        s.tlas_nodes, s.n_tlas_nodes = arrs[0].ctypes.data, len(arrs[0])
        s.instances, s.n_instances = arrs[1].ctypes.data, len(arrs[1])
        s.meshes, s.n_meshes = arrs[2].ctypes.data, len(arrs[2])
        s.bvh_nodes, s.n_bvh_nodes = arrs[3].ctypes.data, len(arrs[3])
        s.vertices, s.n_vertices = arrs[4].ctypes.data, len(arrs[4]) // 3
        s.indices, s.n_indices = arrs[5].ctypes.data, len(arrs[5])
        rays = np.ascontiguousarray(rays, dtype=abi.RAY)
        out = np.zeros(len(rays), dtype=abi.HIT)
        self._chk(self.lib.vd_trace(self.h, C.byref(s), rays.ctypes.data, len(rays), out.ctypes.data))
        return out

    def trace_wide(self, scene_arrays, rays) -> np.ndarray:
        """vd_trace_wide: as trace(), with scene_arrays[0] an array of TLAS_NODE_WIDE."""
        dts = [abi.TLAS_NODE_WIDE, abi.INSTANCE, abi.MESH_INFO, abi.BVH_NODE, np.float32, np.uint32]
        arrs = [np.ascontiguousarray(a, dtype=d).reshape(-1) for a, d in zip(scene_arrays, dts)]
        s = abi.TraceSceneWide()
        for k, name in enumerate(("tlas_nodes", "instances", "meshes", "bvh_nodes", "vertices", "indices")):
            setattr(s, name, arrs[k].ctypes.data)
            setattr(s, "n_" + name, len(arrs[k]) // (3 if name == "vertices" else 1))
        rays = np.ascontiguousarray(rays, dtype=abi.RAY)
        out = np.zeros(len(rays), dtype=abi.HIT)
        self._chk(self.lib.vd_trace_wide(self.h, C.byref(s), rays.ctypes.data, len(rays), out.ctypes.data))
        return out

    class DeviceScene:
        """Device-resident copy of a trace scene; keeps the tensors alive next to the VdTraceScene.  A node array of
        dtype TLAS_NODE_WIDE makes it a VdTraceSceneWide (`wide`): what trace_wide_dev / trace_any_wide_dev take."""

        def __init__(self, ctx, scene_arrays):
            self.wide = getattr(scene_arrays[0], "dtype", None) == abi.TLAS_NODE_WIDE
            dts = [abi.TLAS_NODE_WIDE if self.wide else abi.TLAS_NODE, abi.INSTANCE, abi.MESH_INFO, abi.BVH_NODE, np.float32, np.uint32]
            arrs = [np.ascontiguousarray(a, dtype=d).reshape(-1) for a, d in zip(scene_arrays, dts)]
            self.tensors = [ctx.upload(a) for a in arrs]
            s = abi.TraceSceneWide() if self.wide else abi.TraceScene()
            s.tlas_nodes, s.n_tlas_nodes = self.tensors[0].data_ptr(), len(arrs[0])
            s.instances, s.n_instances = self.tensors[1].data_ptr(), len(arrs[1])
            s.meshes, s.n_meshes = self.tensors[2].data_ptr(), len(arrs[2])
            s.bvh_nodes, s.n_bvh_nodes = self.tensors[3].data_ptr(), len(arrs[3])
            s.vertices, s.n_vertices = self.tensors[4].data_ptr(), len(arrs[4]) // 3
            s.indices, s.n_indices = self.tensors[5].data_ptr(), len(arrs[5])
            self.struct = s

    def device_scene(self, scene_arrays) -> "Context.DeviceScene":
        return Context.DeviceScene(self, scene_arrays)

    def trace_dev(self, scene: "Context.DeviceScene", d_rays, n_rays, d_out):
        if scene.wide:
            raise TypeError("a scene whose top level is TLAS_NODE_WIDE goes through trace_wide_dev")
        self._chk(self.lib.vd_trace_dev(self.h, C.byref(scene.struct), abi.ptr(d_rays), n_rays, abi.ptr(d_out)))

    def trace_wide_dev(self, scene: "Context.DeviceScene", d_rays, n_rays, d_out):
        """vd_trace_wide_dev over a DeviceScene made from TLAS_NODE_WIDE nodes."""
        if not scene.wide:
            raise TypeError("trace_wide_dev needs a scene whose top level is TLAS_NODE_WIDE")
        self._chk(self.lib.vd_trace_wide_dev(self.h, C.byref(scene.struct), abi.ptr(d_rays), n_rays, abi.ptr(d_out)))

    def trace_any_wide_dev(self, scene: "Context.DeviceScene", d_rays, n_rays, d_out_hit):
        if not scene.wide:
            raise TypeError("trace_any_wide_dev needs a scene whose top level is TLAS_NODE_WIDE")
        self._chk(self.lib.vd_trace_any_wide_dev(self.h, C.byref(scene.struct), abi.ptr(d_rays), n_rays, abi.ptr(d_out_hit)))

    def trace_any_dev(self, scene: "Context.DeviceScene", d_rays, n_rays, d_out_hit):
        """Occlusion query: d_out_hit[i] (u32) = 1 iff ray i hits anything (raytraced_shadows.wgsl:97-102)."""
        if scene.wide:
            raise TypeError("a scene whose top level is TLAS_NODE_WIDE goes through trace_any_wide_dev")
        self._chk(self.lib.vd_trace_any_dev(self.h, C.byref(scene.struct), abi.ptr(d_rays), n_rays, abi.ptr(d_out_hit)))

    class TraceAccel:
        """vd_trace_prepare_dev / vd_trace_prepare_wide_dev (by the DeviceScene's node type): per-scene de-indexed leaf triangles
        and, with trace.tight_tlas, a private top level (include/voidin_abi.h); keeps the DeviceScene alive."""

        def __init__(self, ctx: "Context", scene: "Context.DeviceScene"):
            self.ctx, self.scene, self.wide = ctx, scene, scene.wide
            h = C.c_void_p()
            prepare = ctx.lib.vd_trace_prepare_wide_dev if scene.wide else ctx.lib.vd_trace_prepare_dev
            ctx._chk(prepare(ctx.h, C.byref(scene.struct), C.byref(h)))
            self.h = h

        def info(self) -> dict:
            """vd_trace_accel_info, or vd_trace_accel_info_wide for a wide accel (then with "refits_since_build"); "wide" says which."""
            st = abi.TraceAccelInfoWide() if self.wide else abi.TraceAccelInfo()
            fn = self.ctx.lib.vd_trace_accel_info_wide if self.wide else self.ctx.lib.vd_trace_accel_info
            self.ctx._chk(fn(self.h, C.byref(st)))
            d = {"tight_tlas": int(st.tight_tlas), "n_tlas_nodes": int(st.n_tlas_nodes), "tight_fallback_instances": int(st.tight_fallback_instances),
                 "triangle_bytes": int(st.triangle_bytes), "d_tlas_nodes": st.d_tlas_nodes, "wide": self.wide}
            if self.wide:
                d["refits_since_build"] = int(st.refits_since_build)
            return d

        def refit(self):
            """vd_trace_accel_refit_dev: new tight boxes into the private top level as it stands, topology kept (blocks)."""
            self.ctx._chk(self.ctx.lib.vd_trace_accel_refit_dev(self.ctx.h, self.h))

        def update(self):
            """vd_trace_accel_update_dev: rebuild the private top level from the instance buffer as it is now."""
            self.ctx._chk(self.ctx.lib.vd_trace_accel_update_dev(self.ctx.h, self.h))

        def update_geometry(self):
            """vd_trace_accel_update_geometry_dev: de-index the leaf triangles again from the vertex buffer as it is now
            (enqueues only; refit the BLAS first)."""
            self.ctx._chk(self.ctx.lib.vd_trace_accel_update_geometry_dev(self.ctx.h, self.h))

        def close(self):
            if getattr(self, "h", None):
                self.ctx.lib.vd_trace_release(self.ctx.h, self.h)
                self.h = None

        def __del__(self):
            try:
                self.close()
            except Exception:
                pass

    def trace_prepare(self, scene: "Context.DeviceScene") -> "Context.TraceAccel":
        return Context.TraceAccel(self, scene)

    def trace_prepared_dev(self, accel: "Context.TraceAccel", d_rays, n_rays, d_out):
        self._chk(self.lib.vd_trace_prepared_dev(self.h, accel.h, abi.ptr(d_rays), n_rays, abi.ptr(d_out)))

    def trace_any_prepared_dev(self, accel: "Context.TraceAccel", d_rays, n_rays, d_out_hit):
        self._chk(self.lib.vd_trace_any_prepared_dev(self.h, accel.h, abi.ptr(d_rays), n_rays, abi.ptr(d_out_hit)))

    def shadow_rays_dev(self, d_positions, d_normals, n_points, light_position, d_rays):
        lp = (C.c_float * 3)(*[float(x) for x in light_position])
        self._chk(self.lib.vd_shadow_rays_dev(self.h, abi.ptr(d_positions), abi.ptr(d_normals), n_points, lp, abi.ptr(d_rays)))

    def shadow_pass_dev(self, scene: "Context.DeviceScene", d_positions, d_normals, n_points, d_lights, n_lights, d_occluded, d_in_range=None,
                        max_chunk_rays=0) -> dict:
        """vd_shadow_pass_dev (include/voidin_shadow.h): the shadow loop of raytraced_shadows.wgsl:87-115 for n_points points and
        n_lights lights (abi.LIGHT records on the device).  Bit l & 31 of word p * W + (l >> 5), W = (n_lights + 31) // 32, of
        d_in_range (may be None) = point p is in range of light l; of d_occluded = it is, and its shadow ray hits something.
        Blocks.  -> {"n_rays", "n_chunks", "words_per_point"}."""
        if scene.wide:
            raise TypeError("a scene whose top level is TLAS_NODE_WIDE goes through trace_prepare and shadow_pass_prepared_dev")
        info = abi.ShadowPassInfo()
        self._chk(self.lib.vd_shadow_pass_dev(self.h, C.byref(scene.struct), abi.ptr(d_positions), abi.ptr(d_normals), n_points, abi.ptr(d_lights), n_lights,
                                              max_chunk_rays, abi.ptr(d_occluded), abi.ptr(d_in_range), C.byref(info)))
        return {"n_rays": int(info.n_rays), "n_chunks": int(info.n_chunks), "words_per_point": int(info.words_per_point)}

    def shadow_pass_prepared_dev(self, accel: "Context.TraceAccel", d_positions, d_normals, n_points, d_lights, n_lights, d_occluded, d_in_range=None,
                                 max_chunk_rays=0) -> dict:
        """vd_shadow_pass_prepared_dev: the same over a prepared scene - narrow, wide or with a private top level."""
        info = abi.ShadowPassInfo()
        self._chk(self.lib.vd_shadow_pass_prepared_dev(self.h, accel.h, abi.ptr(d_positions), abi.ptr(d_normals), n_points, abi.ptr(d_lights), n_lights,
                                                       max_chunk_rays, abi.ptr(d_occluded), abi.ptr(d_in_range), C.byref(info)))
        return {"n_rays": int(info.n_rays), "n_chunks": int(info.n_chunks), "words_per_point": int(info.words_per_point)}

    @staticmethod
    def gbuffer(d_depth, d_normal_uv, d_material, width, height, depth_pitch=None, normal_uv_pitch=None, material_pitch=None) -> "abi.GBuffer":
        """VdGBuffer (include/voidin_gbuffer.h) over three device images; a pitch (bytes per row) left out is the packed one."""
        return abi.GBuffer(abi.ptr(d_depth), 4 * width if depth_pitch is None else depth_pitch,
                           abi.ptr(d_normal_uv), 8 * width if normal_uv_pitch is None else normal_uv_pitch,
                           abi.ptr(d_material), width if material_pitch is None else material_pitch, width, height)

    def gbuffer_points_dev(self, camera, gb: "abi.GBuffer", d_positions, d_normals, d_pixels, d_n_points, read_back=True):
        """vd_gbuffer_points_dev: the receivers of a G-buffer (material neither 0 nor 2) in pixel order - world position from the
        depth image, normal from the octahedral word, pixel id - and their count in d_n_points.  read_back: the call blocks and
        returns the count; without it the call only enqueues and returns None."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        n = C.c_uint32(0)
        self._chk(self.lib.vd_gbuffer_points_dev(self.h, cam.ctypes.data, C.byref(gb), abi.ptr(d_positions), abi.ptr(d_normals), abi.ptr(d_pixels),
                                                 abi.ptr(d_n_points), C.byref(n) if read_back else None))
        return int(n.value) if read_back else None

    @staticmethod
    def _gbuffer_info(info) -> dict:
        return {"n_points": int(info.n_points), "n_rays": int(info.n_rays), "n_chunks": int(info.n_chunks), "words_per_point": int(info.words_per_point)}

    def shadow_gbuffer_dev(self, scene: "Context.DeviceScene", camera, gb: "abi.GBuffer", d_lights, n_lights, d_occluded, d_in_range=None,
                           max_chunk_rays=0) -> dict:
        """vd_shadow_gbuffer_dev (include/voidin_gbuffer.h): the shadow loop for every pixel of a G-buffer.  W = (n_lights + 31) // 32
        words per PIXEL in d_occluded and d_in_range (may be None): a receiver's are those of shadow_pass_dev for its point, every other
        pixel's are zero.  Blocks.  -> {"n_points", "n_rays", "n_chunks", "words_per_point"}."""
        if scene.wide:
            raise TypeError("a scene whose top level is TLAS_NODE_WIDE goes through trace_prepare and shadow_gbuffer_prepared_dev")
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        info = abi.ShadowGBufferInfo()
        self._chk(self.lib.vd_shadow_gbuffer_dev(self.h, C.byref(scene.struct), cam.ctypes.data, C.byref(gb), abi.ptr(d_lights), n_lights, max_chunk_rays,
                                                 abi.ptr(d_occluded), abi.ptr(d_in_range), C.byref(info)))
        return self._gbuffer_info(info)

    def shadow_gbuffer_prepared_dev(self, accel: "Context.TraceAccel", camera, gb: "abi.GBuffer", d_lights, n_lights, d_occluded, d_in_range=None,
                                    max_chunk_rays=0) -> dict:
        """vd_shadow_gbuffer_prepared_dev: the same over a prepared scene - narrow, wide or with a private top level."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        info = abi.ShadowGBufferInfo()
        self._chk(self.lib.vd_shadow_gbuffer_prepared_dev(self.h, accel.h, cam.ctypes.data, C.byref(gb), abi.ptr(d_lights), n_lights, max_chunk_rays,
                                                          abi.ptr(d_occluded), abi.ptr(d_in_range), C.byref(info)))
        return self._gbuffer_info(info)

    @staticmethod
    def gbuffer_target(d_depth, d_normal_uv, d_material, width, height, depth_pitch=None, normal_uv_pitch=None, material_pitch=None) -> "abi.GBufferTarget":
        """VdGBufferTarget (include/voidin_gbuffer_trace.h) over three writable device images; a pitch left out is the packed one."""
        return abi.GBufferTarget(abi.ptr(d_depth), 4 * width if depth_pitch is None else depth_pitch,
                                 abi.ptr(d_normal_uv), 8 * width if normal_uv_pitch is None else normal_uv_pitch,
                                 abi.ptr(d_material), width if material_pitch is None else material_pitch, width, height)

    @staticmethod
    def gbuffer_geometry(scene: "Context.DeviceScene", d_normals=None, d_tex_coords=None) -> "abi.GBufferGeometry":
        """VdGBufferGeometry: the instances, meshes, vertices and indices of a DeviceScene (narrow or wide) with per-vertex normals
        (3 floats) and uvs (2 floats) on the device, either of which may be None."""
        s = scene.struct
        return abi.GBufferGeometry(s.instances, s.n_instances, s.meshes, s.n_meshes, s.vertices, s.n_vertices, s.indices, s.n_indices,
                                   abi.ptr(d_normals), abi.ptr(d_tex_coords))

    def gbuffer_rays_dev(self, camera, width, height, d_rays):
        """vd_gbuffer_rays_dev: one ray through every pixel centre (bvh_trace.wgsl:227-231), the whole half-line.  Enqueues only."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        self._chk(self.lib.vd_gbuffer_rays_dev(self.h, cam.ctypes.data, width, height, abi.ptr(d_rays)))

    def gbuffer_resolve_dev(self, camera, geometry: "abi.GBufferGeometry", d_hits, target: "abi.GBufferTarget"):
        """vd_gbuffer_resolve_dev: width * height hit records into depth, normal + uv and material.  Enqueues only."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        self._chk(self.lib.vd_gbuffer_resolve_dev(self.h, cam.ctypes.data, C.byref(geometry), abi.ptr(d_hits), C.byref(target)))

    def gbuffer_trace_dev(self, scene: "Context.DeviceScene", camera, target: "abi.GBufferTarget", d_normals=None, d_tex_coords=None):
        """vd_gbuffer_trace_dev: rays -> trace_dev -> resolve over a narrow scene, the rays and records in the context's arena."""
        if scene.wide:
            raise TypeError("a scene whose top level is TLAS_NODE_WIDE goes through trace_prepare and gbuffer_trace_prepared_dev")
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        self._chk(self.lib.vd_gbuffer_trace_dev(self.h, C.byref(scene.struct), abi.ptr(d_normals), abi.ptr(d_tex_coords), cam.ctypes.data, C.byref(target)))

    def gbuffer_trace_prepared_dev(self, accel: "Context.TraceAccel", geometry: "abi.GBufferGeometry", camera, target: "abi.GBufferTarget"):
        """vd_gbuffer_trace_prepared_dev: the same over a prepared scene - narrow, wide or with a private top level."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        self._chk(self.lib.vd_gbuffer_trace_prepared_dev(self.h, accel.h, C.byref(geometry), cam.ctypes.data, C.byref(target)))

    @staticmethod
    def color_target(d_rgba, width, height, pitch=None) -> "abi.ColorTarget":
        """VdColorTarget (include/voidin_lighting.h) over a writable device image of four floats a pixel; a pitch left out is the
        packed one."""
        return abi.ColorTarget(abi.ptr(d_rgba), 16 * width if pitch is None else pitch, width, height)

    def lighting_dev(self, camera, gb: "abi.GBuffer", d_lights, n_lights, d_occluded, d_in_range, d_materials, target: "abi.ColorTarget"):
        """vd_lighting_dev: the shader's light loop summed per pixel over the set in-range bits, in ascending order, from the W words
        per pixel vd_shadow_gbuffer_dev writes; d_materials: abi.LIGHTING_MATERIALS rows of abi.FLAT_MATERIAL.  n_lights == 0: the
        base colours (the light and bit arrays may be None).  Enqueues only."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        self._chk(self.lib.vd_lighting_dev(self.h, cam.ctypes.data, C.byref(gb), abi.ptr(d_lights), n_lights, abi.ptr(d_occluded), abi.ptr(d_in_range),
                                           abi.ptr(d_materials), C.byref(target)))

    def shade_gbuffer_dev(self, scene: "Context.DeviceScene", camera, gb: "abi.GBuffer", d_lights, n_lights, d_materials, target: "abi.ColorTarget",
                          max_chunk_rays=0) -> dict:
        """vd_shade_gbuffer_dev: shadow_gbuffer_dev followed by lighting_dev, the bits in the context's arena.  Blocks.
        -> {"n_points", "n_rays", "n_chunks", "words_per_point"}, as the pass reports."""
        if scene.wide:
            raise TypeError("a scene whose top level is TLAS_NODE_WIDE goes through trace_prepare and shade_gbuffer_prepared_dev")
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        info = abi.ShadowGBufferInfo()
        self._chk(self.lib.vd_shade_gbuffer_dev(self.h, C.byref(scene.struct), cam.ctypes.data, C.byref(gb), abi.ptr(d_lights), n_lights, max_chunk_rays,
                                                abi.ptr(d_materials), C.byref(target), C.byref(info)))
        return self._gbuffer_info(info)

    def shade_gbuffer_prepared_dev(self, accel: "Context.TraceAccel", camera, gb: "abi.GBuffer", d_lights, n_lights, d_materials, target: "abi.ColorTarget",
                                   max_chunk_rays=0) -> dict:
        """vd_shade_gbuffer_prepared_dev: the same over a prepared scene - narrow, wide or with a private top level."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        info = abi.ShadowGBufferInfo()
        self._chk(self.lib.vd_shade_gbuffer_prepared_dev(self.h, accel.h, cam.ctypes.data, C.byref(gb), abi.ptr(d_lights), n_lights, max_chunk_rays,
                                                         abi.ptr(d_materials), C.byref(target), C.byref(info)))
        return self._gbuffer_info(info)

    def primary_rays_dev(self, camera, width, height, d_rays):
        """One ray per pixel from camera.clip_to_world (src/bin/bvh_cpu.rs:71-83); d_rays: width*height rays."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        self._chk(self.lib.vd_primary_rays_dev(self.h, cam.ctypes.data, width, height, abi.ptr(d_rays)))

    def traverse_iter_dev(self, d_nodes, n_nodes, d_verts, d_indices, d_rays, n_rays, d_out_dist):
        """Bvh::traverse_iter (crates/bvh/src/blas.rs:247-295) for a batch of rays against one mesh; -1 = Miss."""
        self._chk(self.lib.vd_traverse_iter_dev(self.h, abi.ptr(d_nodes), n_nodes, abi.ptr(d_verts), abi.ptr(d_indices),
                                                abi.ptr(d_rays), n_rays, abi.ptr(d_out_dist)))

    def traverse_dev(self, d_nodes, n_nodes, d_verts, d_indices, d_rays, n_rays, d_out_dist, t0=1e30):
        """Bvh::traverse (crates/bvh/src/blas.rs:211-245), the recursive walk, started as bvh_cpu.rs:86 would
        (`traverse(.., ray, 0, 1e30)`); Hit(t0) when the root box is entered and nothing is hit, -1 = Miss."""
        self._chk(self.lib.vd_traverse_dev(self.h, abi.ptr(d_nodes), n_nodes, abi.ptr(d_verts), abi.ptr(d_indices),
                                           abi.ptr(d_rays), n_rays, C.c_float(t0), abi.ptr(d_out_dist)))

    # -- occlusion extension (no reference counterpart; include/voidin_abi.h "Occlusion culling") ----------
    def hiz_layout(self, width, height) -> "abi.HizLayout":
        L = abi.HizLayout()
        self._chk(self.lib.vd_hiz_layout(width, height, C.byref(L)))
        return L

    def hiz_build_dev(self, d_depth, width, height, d_pyramid):
        self._chk(self.lib.vd_hiz_build_dev(self.h, abi.ptr(d_depth), width, height, abi.ptr(d_pyramid)))

    def occlusion_mask_dev(self, camera, d_meshes, n_mesh, d_inst, n, d_pyramid, width, height, d_mask_in, d_mask_out):
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        self._chk(self.lib.vd_occlusion_mask_dev(self.h, cam.ctypes.data, abi.ptr(d_meshes), n_mesh, abi.ptr(d_inst), n,
                                                 abi.ptr(d_pyramid), width, height, abi.ptr(d_mask_in), abi.ptr(d_mask_out)))

    # occlusion-culled draw lists: one read of the instances (frustum + pyramid and / or last frame's visibility bits)
    def cull_compact_hiz_dev(self, camera, d_meshes, n_mesh, d_inst, n_inst, d_pyramid, width, height, d_out, d_count,
                             pad_tail: bool = False):
        """vd_cull_compact_hiz_dev: the ordered list of the instances that pass the frustum test and are not occluded."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        self._chk(self.lib.vd_cull_compact_hiz_dev(self.h, cam.ctypes.data, abi.ptr(d_meshes), n_mesh, abi.ptr(d_inst), n_inst,
                                                   abi.ptr(d_pyramid), width, height, abi.ptr(d_out), abi.ptr(d_count), int(pad_tail)))

    def cull_early_dev(self, camera, d_meshes, n_mesh, d_inst, n_inst, d_prev_visible, d_out, d_count, pad_tail: bool = False):
        """vd_cull_early_dev: in the frustum AND visible last frame (d_prev_visible: one bit per instance, u64 words)."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        self._chk(self.lib.vd_cull_early_dev(self.h, cam.ctypes.data, abi.ptr(d_meshes), n_mesh, abi.ptr(d_inst), n_inst,
                                             abi.ptr(d_prev_visible), abi.ptr(d_out), abi.ptr(d_count), int(pad_tail)))

    def cull_late_dev(self, camera, d_meshes, n_mesh, d_inst, n_inst, d_pyramid, width, height, d_prev_visible, d_visible_out,
                      d_out, d_count, pad_tail: bool = False):
        """vd_cull_late_dev: unoccluded now and NOT visible last frame; d_visible_out (may be d_prev_visible) = the
        unoccluded set, next frame's d_prev_visible."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        self._chk(self.lib.vd_cull_late_dev(self.h, cam.ctypes.data, abi.ptr(d_meshes), n_mesh, abi.ptr(d_inst), n_inst,
                                            abi.ptr(d_pyramid), width, height, abi.ptr(d_prev_visible), abi.ptr(d_visible_out),
                                            abi.ptr(d_out), abi.ptr(d_count), int(pad_tail)))

    def cull_compact_hiz(self, camera, meshes, instances, pyramid, width, height, pad_tail=False):
        """Host arrays in (the pyramid as vd_hiz_layout lays it out), (list, count) out; only [0, count) is defined
        (everything with pad_tail)."""
        cam = np.ascontiguousarray(camera, dtype=abi.CAMERA).reshape(1)
        meshes = np.ascontiguousarray(meshes, dtype=abi.MESH_INFO)
        instances = np.ascontiguousarray(instances, dtype=abi.INSTANCE)
        pyramid = np.ascontiguousarray(pyramid, dtype=np.float32).reshape(-1)
        if len(pyramid) != self.hiz_layout(width, height).total_texels:
            raise ValueError("pyramid does not hold vd_hiz_layout(width, height).total_texels floats")
        out = np.zeros(len(instances), dtype=abi.DRAW)
        out.view(np.uint8)[:] = 0xAB
        cnt = C.c_uint32(0)
        self._chk(self.lib.vd_cull_compact_hiz(self.h, cam.ctypes.data, meshes.ctypes.data, len(meshes), instances.ctypes.data,
                                               len(instances), pyramid.ctypes.data, width, height, out.ctypes.data,
                                               C.addressof(cnt), int(pad_tail)))
        return out, cnt.value


# ------------------------------------------------------------------------------------------
# Reference-shaped façade
# ------------------------------------------------------------------------------------------
class EmitDraws:
    """`impl Pass for EmitDraws` (visibility.rs:230-255): record() leaves draw_cmd_buffer[0..N)
    valid on the ctx's stream before the consumer (Geometry::record) runs on the same stream."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def record(self, camera, mesh_info_buf, n_mesh, instances_buf, n_inst, draw_cmd_buffer):
        self.ctx.cull_emit_dev(camera, mesh_info_buf, n_mesh, instances_buf, n_inst, draw_cmd_buffer)

    def record_compacted(self, camera, mesh_info_buf, n_mesh, instances_buf, n_inst, draw_cmd_buffer,
                         draw_count_buf, pad_tail=False):
        self.ctx.cull_compact_dev(camera, mesh_info_buf, n_mesh, instances_buf, n_inst, draw_cmd_buffer,
                                  draw_count_buf, pad_tail)

    def record_views(self, cameras, mesh_info_buf, n_mesh, instances_buf, n_inst, draw_cmd_buffer, draw_count_buf,
                     pad_tail=False, out_stride=None):
        """record_compacted for several cameras of one scene in one read of the instances: view v's list starts at
        command v * out_stride of draw_cmd_buffer (default: n_inst), its count is word v of draw_count_buf."""
        self.ctx.cull_compact_views_dev(cameras, mesh_info_buf, n_mesh, instances_buf, n_inst, draw_cmd_buffer,
                                        draw_count_buf, pad_tail, out_stride)

    def record_batched(self, camera, mesh_info_buf, n_mesh, instances_buf, n_inst, draw_cmd_buffer, visible_ids_buf, draw_count_buf):
        """The instanced form: draw_cmd_buffer[0..n_mesh) = one command per mesh (instance_count = its visible instances),
        visible_ids_buf[0..count) = the survivors' instance ids grouped by mesh, which the vertex shader indexes with
        instance_index; the consumer is multi_draw_indexed_indirect(draw_cmd_buffer, 0, n_mesh)."""
        self.ctx.cull_batch_dev(camera, mesh_info_buf, n_mesh, instances_buf, n_inst, draw_cmd_buffer, visible_ids_buf, draw_count_buf)

    def record_lod(self, camera, lod_params, lod_group_buf, n_group, mesh_info_buf, n_mesh, instances_buf, n_inst, draw_cmd_buffer,
                   draw_count_buf, pad_tail=False):
        """record_compacted with a level of detail per instance: instances name a GROUP, the command comes from the row
        of mesh_info_buf the projected size picks; instances smaller than lod_params.min_size are dropped."""
        self.ctx.cull_compact_lod_dev(camera, lod_params, lod_group_buf, n_group, mesh_info_buf, n_mesh, instances_buf, n_inst,
                                      draw_cmd_buffer, draw_count_buf, pad_tail)

    def record_batched_lod(self, camera, lod_params, lod_group_buf, n_group, mesh_info_buf, n_mesh, instances_buf, n_inst,
                           draw_cmd_buffer, visible_ids_buf, draw_count_buf):
        """record_batched over LOD rows: draw_cmd_buffer[0..n_mesh) = one command per (mesh, LOD) row."""
        self.ctx.cull_batch_lod_dev(camera, lod_params, lod_group_buf, n_group, mesh_info_buf, n_mesh, instances_buf, n_inst,
                                    draw_cmd_buffer, visible_ids_buf, draw_count_buf)

    def record_hiz(self, camera, mesh_info_buf, n_mesh, instances_buf, n_inst, pyramid_buf, width, height, draw_cmd_buffer,
                   draw_count_buf, pad_tail=False):
        """record_compacted with the occlusion test against a depth pyramid folded into the same read of the instances."""
        self.ctx.cull_compact_hiz_dev(camera, mesh_info_buf, n_mesh, instances_buf, n_inst, pyramid_buf, width, height,
                                      draw_cmd_buffer, draw_count_buf, pad_tail)

    def record_early(self, camera, mesh_info_buf, n_mesh, instances_buf, n_inst, state: "OcclusionState", draw_cmd_buffer,
                     draw_count_buf, pad_tail=False):
        """Two-pass occlusion culling, first half: what was visible last frame and is still in the frustum."""
        self.ctx.cull_early_dev(camera, mesh_info_buf, n_mesh, instances_buf, n_inst, state.visible, draw_cmd_buffer,
                                draw_count_buf, pad_tail)

    def record_late(self, camera, mesh_info_buf, n_mesh, instances_buf, n_inst, pyramid_buf, width, height,
                    state: "OcclusionState", draw_cmd_buffer, draw_count_buf, pad_tail=False):
        """Second half, against the pyramid of the depth the early list produced: what it reveals; the state's bits become
        this frame's unoccluded set (in place)."""
        self.ctx.cull_late_dev(camera, mesh_info_buf, n_mesh, instances_buf, n_inst, pyramid_buf, width, height,
                               state.visible, state.visible, draw_cmd_buffer, draw_count_buf, pad_tail)


class OcclusionState:
    """The visibility bits the two-pass scheme carries from frame to frame: one bit per instance in 64-bit words, zeroed
    (nothing was visible before the first frame, so that frame's early list is empty and its late list is everything
    unoccluded)."""

    def __init__(self, ctx: Context, n_inst: int):
        import torch
        self.n_inst = int(n_inst)
        self.visible = torch.zeros(max((self.n_inst + 63) // 64, 1), dtype=torch.int64, device=ctx.torch_device)

    def reset(self):
        self.visible.zero_()


class Bvh:
    def __init__(self, nodes: np.ndarray):
        self.nodes = nodes

    def refit(self, ctx: Context, vertices: np.ndarray, indices: np.ndarray):
        """NEW (not in the reference): same topology, boxes recomputed for `vertices`; `indices` as build() left them."""
        self.nodes = ctx.bvh_refit(vertices, indices, self.nodes)


class BvhBuilder:
    """BvhBuilder::new(vertices, indices).build() (blas.rs:51-103).  `indices` is permuted in
    place, as the reference does to the caller's slice."""

    def __init__(self, ctx: Context, vertices: np.ndarray, indices: np.ndarray):
        self.ctx, self.vertices, self.indices = ctx, vertices, indices
        self.num_bins = 8

    def set_bin_number(self, num_bins: int):
        self.num_bins = num_bins  # stored and ignored, exactly like blas.rs:64-67 vs :136
        return self

    def build(self) -> Bvh:
        nodes, idx = self.ctx.bvh_build(self.vertices, self.indices)
        self.indices.reshape(-1)[:] = idx
        return Bvh(nodes)

    def build_fast(self) -> Bvh:
        """NEW (not in the reference): the LBVH bottom level (vd_bvh_build_lbvh) - for a mesh that is rebuilt every frame."""
        nodes, idx = self.ctx.bvh_build_lbvh(self.vertices, self.indices)
        self.indices.reshape(-1)[:] = idx
        return Bvh(nodes)


class Tlas:
    """Tlas::empty() / Tlas::build(&mut self, instances, meshes) (tlas.rs:27-85)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.nodes = np.zeros(0, dtype=abi.TLAS_NODE)

    @classmethod
    def empty(cls, ctx: Context):
        return cls(ctx)

    def build(self, instances, meshes):
        self.nodes = self.ctx.tlas_build(instances, meshes)

    def refit(self, instances, meshes):
        self.nodes = self.ctx.tlas_refit(instances, meshes, self.nodes)
