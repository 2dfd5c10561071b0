"""The host-pointer forms of the ray side and the top-level builders against each other's leftovers: vd_tlas_build*, vd_tlas_refit,
vd_tlas_build_lbvh*, vd_trace, vd_trace_wide, vd_traverse_iter, vd_traverse and vd_primary_rays all stage their inputs and results
through the context, so they run here one after the other on ONE fresh context, in an order that makes each of them find the
staging memory in another form's layout and at sizes that make it regrow several times, and every result is compared byte for
byte with the matching _dev form on a second context over uploaded inputs (the _dev forms are held against the oracle elsewhere:
tests/test_gpu_tlas_trace.py, test_gpu_trace_wide.py, test_gpu_tlas_lbvh.py, test_gpu_trace_deep.py).  Behind every host output
lie a few sentinel records that no call may touch.  The refusals of every entry point - status and exact text - close the file."""
import ctypes as C

import numpy as np
import pytest

from chain_scenes import chain_rays, chain_scene
from voidin_amd import abi, synth
from voidin_amd.runtime import Context
from wide_scenes import first_bad, mesh_set, records_equal, widen

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 65, 1025, 3000]           # instances; the staging memory starts at 64 KiB and regrows at 1025 and again at 3000
RAY_COUNTS = [1, 65, 4097]
FILL = 0xC3
SLACK = 5                                # records behind every host output that no call may touch


@pytest.fixture(scope="module")
def ref_ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def geometry(oracle):
    """(infos, bvh_nodes, vertices, indices) of two meshes for the trace scenes, and one mesh (nodes, vertices, indices) for the
    single-mesh walks."""
    scene_meshes = mesh_set(oracle, [synth.uv_sphere(1.0, 4), synth.knot_mesh(48, 12)])
    v, i = synth.knot_mesh(96, 24)
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
    nodes, idx = oracle.bvh_build(v, i)
    return scene_meshes, (np.ascontiguousarray(nodes, dtype=abi.BVH_NODE), v, np.ascontiguousarray(idx, dtype=np.uint32))


def filled(count, dtype):
    a = np.zeros(count, dtype=dtype)
    a.view(np.uint8)[:] = FILL
    return a


def untouched(a, n):
    return bool((a[n:].view(np.uint8) == FILL).all())


def rays_into(n, seed, radius, spread):
    """n seeded rays from a sphere of `radius` around the origin towards points of the cube [-spread, spread]^3."""
    u = synth.uniform01(seed, 0, 6 * n).reshape(n, 6).astype(np.float64)
    o = u[:, :3] * 2 - 1
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * radius
    t = (u[:, 3:] * 2 - 1) * spread
    rays = np.zeros(n, dtype=abi.RAY)
    rays["eye"], rays["dir"] = o, (t - o) / np.linalg.norm(t - o, axis=1, keepdims=True)
    return rays


def instances(n, moved=False):
    return synth.instances(n, n_mesh=2, seed=synth.SEED_BASE + 70 + n + (1000 if moved else 0), extent=40.0, scale_range=(0.5, 2.0))


def host_scene(arrays, wide):
    """(VdTraceScene / VdTraceSceneWide over host arrays, the arrays - kept alive by the caller)."""
    dts = [abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE, abi.INSTANCE, abi.MESH_INFO, abi.BVH_NODE, np.float32, np.uint32]
    arrs = [np.ascontiguousarray(a, dtype=d).reshape(-1) for a, d in zip(arrays, dts)]
    s = abi.TraceSceneWide() if wide else abi.TraceScene()
    for k, name in enumerate(("tlas_nodes", "instances", "meshes", "bvh_nodes", "vertices", "indices")):
        setattr(s, name, arrs[k].ctypes.data)
        setattr(s, "n_" + name, len(arrs[k]) // (3 if name == "vertices" else 1))
    return s, arrs


class Reference:
    """The _dev forms on the second context: every result is computed once, kept as bytes and never written again."""

    def __init__(self, ctx, geometry):
        self.ctx = ctx
        (self.infos, self.B, self.V, self.I), self.mesh = geometry
        self.d_meshes = ctx.upload(self.infos)
        self.d_mesh = tuple(ctx.upload(a) for a in self.mesh)
        self._tlas, self._hits, self._dist, self._rays = {}, {}, {}, {}

    def tlas(self, n):
        """{form: nodes} of n instances: build, build_wide, lbvh, lbvh_wide, and refit = the narrow build refitted to moved instances."""
        if n in self._tlas:
            return self._tlas[n]
        import torch
        c, out = self.ctx, {}
        inst, inst2 = instances(n), instances(n, moved=True)
        d_i, d_i2 = c.upload(inst), c.upload(inst2)
        for name, fn, wide in (("build", c.tlas_build_dev, False), ("build_wide", c.tlas_build_dev, True),
                               ("lbvh", c.tlas_build_lbvh_dev, False), ("lbvh_wide", c.tlas_build_lbvh_dev, True)):
            dt = abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE
            d_n = torch.full(((2 * n + 1) * dt.itemsize,), 0xCD, dtype=torch.uint8, device=c.torch_device)
            fn(d_i, n, self.d_meshes, len(self.infos), d_n, wide=wide)
            torch.cuda.synchronize()
            out[name] = d_n.cpu().numpy().view(dt).copy()
        d_n = c.upload(out["build"])
        c.tlas_refit_dev(d_i2, n, self.d_meshes, len(self.infos), d_n)
        torch.cuda.synchronize()
        out["refit"] = d_n.cpu().numpy().view(abi.TLAS_NODE).copy()
        assert out["refit"].tobytes() != out["build"].tobytes()
        self._tlas[n] = out
        return out

    def scene(self, n, wide):
        t = self.tlas(n)
        return (t["build_wide"] if wide else t["build"], instances(n), self.infos, self.B, self.V, self.I)

    def hits(self, key, scene, rays):
        """The records of vd_trace_dev / vd_trace_wide_dev (by the node type of scene[0]) over `scene`."""
        if key not in self._hits:
            import torch
            c, n = self.ctx, len(rays)
            ds = c.device_scene(scene)
            d_h = c.empty(n * 16)
            (c.trace_wide_dev if ds.wide else c.trace_dev)(ds, c.upload(rays), n, d_h)
            torch.cuda.synchronize()
            self._hits[key] = d_h.cpu().numpy()[: n * 16].view(abi.HIT).copy()
        return self._hits[key]

    def dist(self, recursive, rays):
        key = (recursive, len(rays))
        if key not in self._dist:
            import torch
            c, n = self.ctx, len(rays)
            d_out = torch.full((n,), 7.0, dtype=torch.float32, device=c.torch_device)
            d_n, d_v, d_i = self.d_mesh
            if recursive:
                c.traverse_dev(d_n, len(self.mesh[0]), d_v, d_i, c.upload(rays), n, d_out, t0=14.0)
            else:
                c.traverse_iter_dev(d_n, len(self.mesh[0]), d_v, d_i, c.upload(rays), n, d_out)
            torch.cuda.synchronize()
            self._dist[key] = d_out.cpu().numpy().copy()
        return self._dist[key]

    def primary(self, cam, w, h):
        if (w, h) not in self._rays:
            import torch
            d_r = torch.full((w * h * abi.RAY.itemsize,), 0xCD, dtype=torch.uint8, device=self.ctx.torch_device)
            self.ctx.primary_rays_dev(cam, w, h, d_r)
            torch.cuda.synchronize()
            self._rays[(w, h)] = d_r.cpu().numpy().view(abi.RAY).copy()
        return self._rays[(w, h)]


@pytest.fixture(scope="module")
def reference(ref_ctx, geometry):
    return Reference(ref_ctx, geometry)


SCENE_RAYS = {r: rays_into(r, synth.SEED_BASE + 91 + r, 50.0, 20.0) for r in RAY_COUNTS}
MESH_RAYS = {r: rays_into(r, synth.SEED_BASE + 95 + r, 6.0, 1.5) for r in RAY_COUNTS}
CAMERA = np.ascontiguousarray(synth.camera_uniform(eye=(0, 0, 15), pitch_deg=0), dtype=abi.CAMERA).reshape(1)


def host_trace(ctx, scene, rays, wide, what):
    s, keep = host_scene(scene, wide)
    n = len(rays)
    out = filled(n + SLACK, abi.HIT)
    fn = ctx.lib.vd_trace_wide if wide else ctx.lib.vd_trace
    assert fn(ctx.h, C.byref(s), rays.ctypes.data, n, out.ctypes.data) == abi.VD_OK, (what, ctx.lib.vd_last_error(ctx.h))
    assert untouched(out, n), (what, "records behind the output were written")
    return out[:n]


def run_sequence(ctx, ref, n):
    lib, h = ctx.lib, ctx.h
    inst, inst2, infos = instances(n), instances(n, moved=True), ref.infos
    want = ref.tlas(n)
    nodes_m, verts_m, idx_m = ref.mesh

    def build(name, fn, wide, start=None):
        dt = abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE
        out = filled(2 * n + 1 + SLACK, dt)
        if start is not None:
            out[: 2 * n + 1] = start
        src = inst2 if start is not None else inst
        assert fn(h, src.ctypes.data, n, infos.ctypes.data, len(infos), out.ctypes.data) == abi.VD_OK, (name, n, lib.vd_last_error(h))
        assert out[: 2 * n + 1].tobytes() == want[name].tobytes(), (name, n)
        assert untouched(out, 2 * n + 1), (name, n, "nodes behind the array were written")

    def trace(r, wide):
        rays = SCENE_RAYS[r]
        scene = ref.scene(n, wide)
        got = host_trace(ctx, scene, rays, wide, (n, r, wide))
        w = ref.hits((n, r, wide), scene, rays)
        assert records_equal(got, w), ("vd_trace_wide" if wide else "vd_trace", n, r, first_bad(got, w))

    def traverse(r, recursive):
        rays = MESH_RAYS[r]
        out = filled(r + SLACK, np.float32)
        if recursive:
            rc = lib.vd_traverse(h, nodes_m.ctypes.data, len(nodes_m), verts_m.ctypes.data, len(verts_m), idx_m.ctypes.data, len(idx_m) // 3,
                                 rays.ctypes.data, r, C.c_float(14.0), out.ctypes.data)
        else:
            rc = lib.vd_traverse_iter(h, nodes_m.ctypes.data, len(nodes_m), verts_m.ctypes.data, len(verts_m), idx_m.ctypes.data, len(idx_m) // 3,
                                      rays.ctypes.data, r, out.ctypes.data)
        assert rc == abi.VD_OK, (recursive, r, lib.vd_last_error(h))
        assert out[:r].tobytes() == ref.dist(recursive, rays).tobytes(), ("vd_traverse" if recursive else "vd_traverse_iter", n, r)
        assert untouched(out, r), (recursive, r, "distances behind the output were written")

    def primary(w, hgt):
        out = filled(w * hgt + SLACK, abi.RAY)
        assert lib.vd_primary_rays(h, CAMERA.ctypes.data, w, hgt, out.ctypes.data) == abi.VD_OK, lib.vd_last_error(h)
        assert out[: w * hgt].tobytes() == ref.primary(CAMERA, w, hgt).tobytes(), ("vd_primary_rays", w, hgt)
        assert untouched(out, w * hgt), ("vd_primary_rays", w, hgt, "rays behind the output were written")

    r0, r1, r2 = RAY_COUNTS
    build("build", lib.vd_tlas_build, False)
    trace(r0, False)
    build("build_wide", lib.vd_tlas_build_wide, True)
    traverse(r1, False)
    build("refit", lib.vd_tlas_refit, False, start=want["build"])
    trace(r2, True)
    build("lbvh", lib.vd_tlas_build_lbvh, False)
    primary(1, 1)
    traverse(r0, True)
    build("lbvh_wide", lib.vd_tlas_build_lbvh_wide, True)
    trace(r1, False)
    trace(r0, True)
    primary(97, 61)
    traverse(r2, False)
    trace(r2, False)
    build("refit", lib.vd_tlas_refit, False, start=want["build"])
    trace(r1, True)
    traverse(r1, True)
    traverse(r2, True)
    traverse(r0, False)
    build("build", lib.vd_tlas_build, False)


def test_host_forms_share_the_staging_memory(reference):
    ctx = Context(0)
    try:
        for n in SIZES + [2]:                # ... and a small call again in the memory the largest one left
            run_sequence(ctx, reference, n)
        # the results are not vacuous: rays hit and miss, on the scenes and on the mesh
        hits = reference.hits((3000, 4097, False), None, None)["hit"]
        assert 0 < hits.sum() < len(hits)
        d = reference.dist(False, MESH_RAYS[4097])
        assert (d >= 0).any() and (d < 0).any()
    finally:
        ctx.close()


def test_deep_rays_through_the_host_forms(reference, oracle):
    """A chain of 200 leaves: rays that run out of their 128 stack entries take the second pass - through the staged forms too."""
    scene = chain_scene(oracle, 200)
    rays, _far, _cheap = chain_rays(4097, 250.0, seed=79)
    ctx = Context(0)
    try:
        for wide in (False, True):
            sc = ((widen(scene[0]),) if wide else (scene[0],)) + tuple(scene[1:])
            want = reference.hits(("chain", wide), sc, rays)
            assert 0 < want["hit"].sum() < len(rays)
            got = host_trace(ctx, sc, rays, wide, ("chain", wide))
            assert records_equal(got, want), (wide, first_bad(got, want))
    finally:
        ctx.close()


def test_fan_out_through_the_host_forms(reference):
    """trace.waves = 1: a grid of one wave per CU, so 16 384 rays are one per lane and the call over 1 025 instances may fan out.
    The staged call with the fan-out, the same call as one launch (trace.fan = 1) and the _dev form give the same bytes."""
    n, rays = 1025, rays_into(16384, synth.SEED_BASE + 99, 50.0, 20.0)
    for wide in (False, True):
        ctx = Context(0)                     # a fresh one each: what a call remembers about the fan-out is per context
        try:
            ctx.set_option("trace.waves", 1)
            scene = reference.scene(n, wide)
            fanned = host_trace(ctx, scene, rays, wide, ("fan-out", wide)).copy()
            ctx.set_option("trace.fan", 1)
            single = host_trace(ctx, scene, rays, wide, ("one launch", wide)).copy()
            ctx.set_option("trace.fan", None)
            assert records_equal(fanned, single), (wide, first_bad(fanned, single))
            want = reference.hits((n, len(rays), wide), scene, rays)
            assert records_equal(fanned, want), (wide, first_bad(fanned, want))
            assert 0 < want["hit"].sum() < len(rays)
        finally:
            ctx.close()


# ---- refusals: status and exact text, as the entry points have always given them --------------------------------------
MARK = b"vd_ctx_set_option: unknown option"


def refused(ctx, fn, args, status, text):
    """Calls fn(ctx, *args) after leaving a known other message in the context; the call must return `status` and leave `text`."""
    assert ctx.lib.vd_ctx_set_option(ctx.h, 9999, 0) == abi.VD_ERR_INVALID_ARG and ctx.lib.vd_last_error(ctx.h) == MARK
    assert fn(ctx.h, *args) == status, (fn.__name__, args, ctx.lib.vd_last_error(ctx.h))
    assert ctx.lib.vd_last_error(ctx.h) == text, (fn.__name__, args, ctx.lib.vd_last_error(ctx.h))


def accepted_without_rays(ctx, fn, args):
    """n_rays == 0 with null rays / out: VD_OK, and no message is written."""
    assert ctx.lib.vd_ctx_set_option(ctx.h, 9999, 0) == abi.VD_ERR_INVALID_ARG
    assert fn(ctx.h, *args) == abi.VD_OK, (fn.__name__, ctx.lib.vd_last_error(ctx.h))
    assert ctx.lib.vd_last_error(ctx.h) == MARK, fn.__name__


def null_ctx(ctx, fn, args):
    """A null context: VD_ERR_INVALID_ARG, and nothing is written anywhere (the live context keeps its message)."""
    assert ctx.lib.vd_ctx_set_option(ctx.h, 9999, 0) == abi.VD_ERR_INVALID_ARG
    assert fn(None, *args) == abi.VD_ERR_INVALID_ARG, fn.__name__
    assert ctx.lib.vd_last_error(ctx.h) == MARK, fn.__name__


def incomplete(struct_type, s, field):
    t = struct_type()
    C.memmove(C.byref(t), C.byref(s), C.sizeof(struct_type))
    setattr(t, field, None if not field.startswith("n_") else 0)
    return t


def test_trace_refusals(reference):
    import torch
    n, r = 65, 65
    rays = SCENE_RAYS[r]
    ctx = Context(0)
    try:
        lib = ctx.lib
        d_rays, d_out = ctx.upload(rays), ctx.empty(r * 16)
        d_out.fill_(FILL)
        dr, do = d_rays.data_ptr(), d_out.data_ptr()
        h_out = filled(r, abi.HIT)
        hr, ho = rays.ctypes.data, h_out.ctypes.data
        ds_n, ds_w = ctx.device_scene(reference.scene(n, False)), ctx.device_scene(reference.scene(n, True))
        hs_n, keep_n = host_scene(reference.scene(n, False), False)
        hs_w, keep_w = host_scene(reference.scene(n, True), True)
        # entry point: (function, scene struct, its type, rays, out, name in "incomplete scene", name in "null rays/out")
        scene_forms = [
            (lib.vd_trace_dev, ds_n.struct, abi.TraceScene, dr, do, b"vd_trace", b"vd_trace"),
            (lib.vd_trace_any_dev, ds_n.struct, abi.TraceScene, dr, do, b"vd_trace_any", b"vd_trace_any"),
            (lib.vd_trace, hs_n, abi.TraceScene, hr, ho, b"vd_trace", b"vd_trace"),
            (lib.vd_trace_wide_dev, ds_w.struct, abi.TraceSceneWide, dr, do, b"vd_trace_wide", b"vd_trace_wide"),
            (lib.vd_trace_any_wide_dev, ds_w.struct, abi.TraceSceneWide, dr, do, b"vd_trace_wide", b"vd_trace_any_wide"),
            (lib.vd_trace_wide, hs_w, abi.TraceSceneWide, hr, ho, b"vd_trace_wide", b"vd_trace_wide"),
        ]
        for fn, s, st, pr, po, scene_name, rays_name in scene_forms:
            null_ctx(ctx, fn, (C.byref(s), pr, r, po))
            refused(ctx, fn, (None, pr, r, po), abi.VD_ERR_INVALID_ARG, scene_name + b": incomplete scene")
            for field in ("tlas_nodes", "instances", "meshes", "bvh_nodes", "vertices", "indices", "n_meshes", "n_tlas_nodes", "n_instances"):
                refused(ctx, fn, (C.byref(incomplete(st, s, field)), pr, r, po), abi.VD_ERR_INVALID_ARG, scene_name + b": incomplete scene")
            refused(ctx, fn, (C.byref(incomplete(st, s, "instances")), None, 0, None), abi.VD_ERR_INVALID_ARG, scene_name + b": incomplete scene")
            accepted_without_rays(ctx, fn, (C.byref(s), None, 0, None))
            refused(ctx, fn, (C.byref(s), None, r, po), abi.VD_ERR_INVALID_ARG, rays_name + b": null rays/out")
            refused(ctx, fn, (C.byref(s), pr, r, None), abi.VD_ERR_INVALID_ARG, rays_name + b": null rays/out")
            assert fn(ctx.h, C.byref(s), pr, r, po) == abi.VD_OK, (fn.__name__, lib.vd_last_error(ctx.h))      # the context still works
        for fn in (lib.vd_trace_wide_dev, lib.vd_trace_any_wide_dev, lib.vd_trace_wide):
            s = hs_w if fn is lib.vd_trace_wide else ds_w.struct
            many = incomplete(abi.TraceSceneWide, s, "n_tlas_nodes")
            many.n_tlas_nodes = 2 * abi.TLAS_WIDE_MAX_INSTANCES + 2
            pr, po = (hr, ho) if fn is lib.vd_trace_wide else (dr, do)
            refused(ctx, fn, (C.byref(many), pr, r, po), abi.VD_ERR_INVALID_ARG, b"vd_trace_wide: more than 2 * VD_TLAS_WIDE_MAX_INSTANCES + 1 top-level nodes")
        accel = ctx.trace_prepare(ds_n)
        try:
            for fn, name in ((lib.vd_trace_prepared_dev, b"vd_trace_prepared"), (lib.vd_trace_any_prepared_dev, b"vd_trace_any_prepared")):
                null_ctx(ctx, fn, (accel.h, dr, r, do))
                refused(ctx, fn, (None, dr, r, do), abi.VD_ERR_INVALID_ARG, name + b": null accel")
                refused(ctx, fn, (None, None, 0, None), abi.VD_ERR_INVALID_ARG, name + b": null accel")
                accepted_without_rays(ctx, fn, (accel.h, None, 0, None))
                refused(ctx, fn, (accel.h, None, r, do), abi.VD_ERR_INVALID_ARG, name + b": null rays/out")
                refused(ctx, fn, (accel.h, dr, r, None), abi.VD_ERR_INVALID_ARG, name + b": null rays/out")
                assert fn(ctx.h, accel.h, dr, r, do) == abi.VD_OK, (name, lib.vd_last_error(ctx.h))
        finally:
            accel.close()
        torch.cuda.synchronize()
    finally:
        ctx.close()


def test_traverse_refusals(reference):
    import torch
    r = 65
    rays = MESH_RAYS[r]
    nodes, verts, idx = reference.mesh
    ctx = Context(0)
    try:
        lib = ctx.lib
        d_n, d_v, d_i, d_r = (ctx.upload(a) for a in (nodes, verts, idx, rays))
        d_out = torch.zeros(r, dtype=torch.float32, device=ctx.torch_device)
        out = filled(r, np.float32)
        t0 = C.c_float(1e30)
        # (function, name in the messages, arguments before the rays, the rays, arguments between the count and the output, output)
        forms = [
            (lib.vd_traverse_iter_dev, b"vd_traverse_iter", [d_n.data_ptr(), len(nodes), d_v.data_ptr(), d_i.data_ptr()], d_r.data_ptr(), [], d_out.data_ptr()),
            (lib.vd_traverse_dev, b"vd_traverse", [d_n.data_ptr(), len(nodes), d_v.data_ptr(), d_i.data_ptr()], d_r.data_ptr(), [t0], d_out.data_ptr()),
            (lib.vd_traverse_iter, b"vd_traverse[_iter]", [nodes.ctypes.data, len(nodes), verts.ctypes.data, len(verts), idx.ctypes.data, len(idx) // 3],
             rays.ctypes.data, [], out.ctypes.data),
            (lib.vd_traverse, b"vd_traverse[_iter]", [nodes.ctypes.data, len(nodes), verts.ctypes.data, len(verts), idx.ctypes.data, len(idx) // 3],
             rays.ctypes.data, [t0], out.ctypes.data),
        ]
        for fn, name, mesh, pr, mid, po in forms:
            host = len(mesh) == 6
            null_ctx(ctx, fn, (*mesh, pr, r, *mid, po))
            for pos in ((0, 1, 2, 4) if host else (0, 1, 2, 3)):      # nodes, n_nodes, vertices, indices
                bad = list(mesh)
                bad[pos] = 0 if pos == 1 else None
                refused(ctx, fn, (*bad, pr, r, *mid, po), abi.VD_ERR_INVALID_ARG, name + b": incomplete mesh")
                refused(ctx, fn, (*bad, None, 0, *mid, None), abi.VD_ERR_INVALID_ARG, name + b": incomplete mesh")
            accepted_without_rays(ctx, fn, (*mesh, None, 0, *mid, None))
            refused(ctx, fn, (*mesh, None, r, *mid, po), abi.VD_ERR_INVALID_ARG, name + b": null rays/out")
            refused(ctx, fn, (*mesh, pr, r, *mid, None), abi.VD_ERR_INVALID_ARG, name + b": null rays/out")
            assert fn(ctx.h, *mesh, pr, r, *mid, po) == abi.VD_OK, (name, lib.vd_last_error(ctx.h))
        torch.cuda.synchronize()
        assert out.tobytes() == d_out.cpu().numpy().tobytes()       # the last host call and the last _dev call: the recursive walk from 1e30
        # vd_primary_rays: a null context, a null camera, a null output
        one = filled(4, abi.RAY)
        null_ctx(ctx, lib.vd_primary_rays, (CAMERA.ctypes.data, 2, 2, one.ctypes.data))
        refused(ctx, lib.vd_primary_rays, (CAMERA.ctypes.data, 2, 2, None), abi.VD_ERR_INVALID_ARG, b"vd_primary_rays: null rays")
        refused(ctx, lib.vd_primary_rays, (None, 2, 2, one.ctypes.data), abi.VD_ERR_INVALID_ARG, b"vd_primary_rays: null camera")
        assert untouched(one, 0)
        accepted_without_rays(ctx, lib.vd_primary_rays, (CAMERA.ctypes.data, 0, 7, None))
    finally:
        ctx.close()


def test_tlas_refusals(reference):
    n = 65
    inst, infos = instances(n), reference.infos
    want = reference.tlas(n)
    ctx = Context(0)
    try:
        lib = ctx.lib
        d_i, d_m = ctx.upload(inst), ctx.upload(infos)
        null_text = b"vd_tlas_*: null pointer or zero count"
        narrow_text = b"vd_tlas_*: n > 32768 does not fit the 16-bit left_right packing (tlas.rs:71); use the _wide variant"
        # (function, wide, host form, the nodes it starts from - a refit - or None, the result it must give)
        forms = [
            (lib.vd_tlas_build, False, True, None, "build"), (lib.vd_tlas_build_dev, False, False, None, "build"),
            (lib.vd_tlas_build_wide, True, True, None, "build_wide"), (lib.vd_tlas_build_wide_dev, True, False, None, "build_wide"),
            (lib.vd_tlas_refit, False, True, "build", "build"), (lib.vd_tlas_refit_dev, False, False, "build", "build"),
            (lib.vd_tlas_refit_wide_dev, True, False, "build_wide", "build_wide"),
            (lib.vd_tlas_build_lbvh, False, True, None, "lbvh"), (lib.vd_tlas_build_lbvh_dev, False, False, None, "lbvh"),
            (lib.vd_tlas_build_lbvh_wide, True, True, None, "lbvh_wide"), (lib.vd_tlas_build_lbvh_wide_dev, True, False, None, "lbvh_wide"),
        ]
        for fn, wide, host, start, result in forms:
            dt = abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE
            h_nodes = filled(2 * n + 1 + SLACK, dt)
            if start:
                h_nodes[: 2 * n + 1] = want[start]
            d_nodes = ctx.upload(h_nodes)
            pi, pm, pn = (inst.ctypes.data, infos.ctypes.data, h_nodes.ctypes.data) if host else (d_i.data_ptr(), d_m.data_ptr(), d_nodes.data_ptr())
            null_ctx(ctx, fn, (pi, n, pm, len(infos), pn))
            for bad in ((None, n, pm, len(infos), pn), (pi, 0, pm, len(infos), pn), (pi, n, None, len(infos), pn), (pi, n, pm, 0, pn),
                        (pi, n, pm, len(infos), None)):
                refused(ctx, fn, bad, abi.VD_ERR_INVALID_ARG, null_text)
            if not wide:
                refused(ctx, fn, (pi, abi.TLAS_MAX_INSTANCES + 1, pm, len(infos), pn), abi.VD_ERR_TLAS_OVERFLOW, narrow_text)
            elif b"lbvh" in fn.__name__.encode():
                refused(ctx, fn, (pi, abi.TLAS_WIDE_MAX_INSTANCES + 1, pm, len(infos), pn), abi.VD_ERR_INVALID_ARG,
                        b"vd_tlas_build_lbvh_wide: n > VD_TLAS_WIDE_MAX_INSTANCES")
            assert untouched(h_nodes, 2 * n + 1 if start else 0), fn.__name__
            assert fn(ctx.h, pi, n, pm, len(infos), pn) == abi.VD_OK, (fn.__name__, lib.vd_last_error(ctx.h))      # and then it works
            ctx.synchronize()
            got = h_nodes if host else d_nodes.cpu().numpy().view(dt)
            assert got[: 2 * n + 1].tobytes() == want[result].tobytes(), fn.__name__       # a refit to the instances of the build: the build
            assert untouched(got, 2 * n + 1), fn.__name__
    finally:
        ctx.close()
