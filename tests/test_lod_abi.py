"""The level-of-detail entry points (include/voidin_abi.h, "Level of detail") at the boundary: struct layouts of the header
and of the Python mirror, a null context is a return code that writes nothing, the emitted gfx950 code of the new pass-1
kernel (registers within three workgroups per CU, no private memory, no atomics, the group row fetched as four 16-byte
loads) - all without a GPU - and, with one, the argument checks that need a live context."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from voidin_amd import abi

CSRC = os.path.join(ROOT, "voidin_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-S", "--cuda-device-only"]
SYMBOLS = ("vd_lod_ids_dev", "vd_cull_compact_lod_dev", "vd_cull_batch_lod_dev", "vd_cull_compact_lod")


def test_struct_layouts():
    g, p = abi.LOD_GROUP, abi.LOD_PARAMS
    assert g.itemsize == 64 and p.itemsize == 16 and C.sizeof(abi.LodParams) == 16
    assert [g.fields[k][1] for k in ("min", "first_row", "max", "n_lods", "switch_size", "_pad")] == [0, 12, 16, 28, 32, 60]
    assert [p.fields[k][1] for k in ("scale", "min_distance", "min_size", "_pad")] == [0, 4, 8, 12]
    assert [getattr(abi.LodParams, k).offset for k in ("scale", "min_distance", "min_size", "_pad")] == [0, 4, 8, 12]
    assert abi.LOD_MAX == 8 and g.fields["switch_size"][0].shape == (7,)
    src = ('#include <stddef.h>\n#include "voidin_abi.h"\n'
           "_Static_assert(sizeof(VdLodGroup) == 64 && sizeof(VdLodParams) == 16 && VD_LOD_MAX == 8u, \"sizes\");\n"
           "_Static_assert(offsetof(VdLodGroup, first_row) == 12 && offsetof(VdLodGroup, max) == 16 && offsetof(VdLodGroup, n_lods) == 28, \"group\");\n"
           "_Static_assert(offsetof(VdLodGroup, switch_size) == 32 && offsetof(VdLodGroup, _pad) == 60, \"group\");\n"
           "_Static_assert(offsetof(VdLodParams, min_distance) == 4 && offsetof(VdLodParams, min_size) == 8, \"params\");\n"
           "int main(void) { return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "lod_abi.c")
        open(path, "w").write(src)
        r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_entry_points():
    lib = abi.load()
    for name in SYMBOLS:
        assert name in abi.PROTOTYPES and hasattr(lib, name), name


def _host_args():
    cam = np.zeros(1, abi.CAMERA)
    groups = np.zeros(2, abi.LOD_GROUP)
    groups["n_lods"], groups["first_row"] = 2, [0, 2]
    meshes, inst = np.zeros(4, abi.MESH_INFO), np.zeros(4, abi.INSTANCE)
    return cam, groups, meshes, inst, abi.LodParams(500.0, 0.1, 0.0, 0)


def test_null_context_is_an_error_not_a_crash():
    lib = abi.load()
    cam, groups, meshes, inst, P = _host_args()
    out, ids, cnt = np.full(4 * 20, 0xAB, np.uint8), np.full(4, 0xABABABAB, np.uint32), np.full(1, 7, np.uint32)
    I = abi.VD_ERR_INVALID_ARG
    assert lib.vd_lod_ids_dev(None, cam.ctypes.data, P, groups.ctypes.data, 2, 4, inst.ctypes.data, 4, ids.ctypes.data, 4) == I
    assert lib.vd_cull_compact_lod_dev(None, cam.ctypes.data, P, groups.ctypes.data, 2, meshes.ctypes.data, 4, inst.ctypes.data, 4, out.ctypes.data, cnt.ctypes.data, 0) == I
    assert lib.vd_cull_compact_lod(None, cam.ctypes.data, P, groups.ctypes.data, 2, meshes.ctypes.data, 4, inst.ctypes.data, 4, out.ctypes.data, cnt.ctypes.data, 1) == I
    assert lib.vd_cull_batch_lod_dev(None, cam.ctypes.data, P, groups.ctypes.data, 2, meshes.ctypes.data, 4, inst.ctypes.data, 4, out.ctypes.data, ids.ctypes.data, cnt.ctypes.data) == I
    assert lib.vd_cull_compact_lod(None, None, P, None, 0, None, 0, None, 0, None, None, 0) == I
    assert (cnt == 7).all() and (out == 0xAB).all() and (ids == 0xABABABAB).all()


# --- the emitted code ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cull_isa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isa") / "cull.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, os.path.join(CSRC, "cull.hip"), "-o", path], check=True, capture_output=True, timeout=600)
    return open(path).read()


def kernel_metadata(text, fragment):
    out = {}
    meta = text[text.index("amdhsa.kernels:"):]
    for entry in re.split(r"\n  - \.", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry)
        if name and fragment in name.group(1):
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return out


def kernel_bodies(text, fragment):
    out = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):\s*;.*$" % re.escape(fragment), text, re.M):
        end = text.index(".Lfunc_end", m.end())
        out[m.group(1)] = [l.strip() for l in text[m.end():end].splitlines() if l.strip() and not l.strip().startswith((";", "."))]
    return out


def test_the_lod_kernel_fits_three_workgroups_per_cu_without_private_memory(cull_isa):
    """__launch_bounds__(256, 3) = 12 waves per CU = 3 per SIMD: at most 512 / 3 -> 168 vector registers, and nothing spilled
    to reach that.  Six instantiations: three id widths, with and without the mask."""
    meta = kernel_metadata(cull_isa, "cull_mask_lod_kernel")
    assert len(meta) == 6, sorted(meta)
    for sym, m in meta.items():
        print(sym, {k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert m["vgpr_count"] <= 168, (sym, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (sym, m)
        assert m["group_segment_fixed_size"] == 0, (sym, m)             # no LDS beyond the skeleton's dynamic slab + id rows


def test_the_lod_kernel_has_no_atomics_and_loads_a_group_as_four_quads(cull_isa):
    bodies = kernel_bodies(cull_isa, "cull_mask_lod_kernel")
    assert len(bodies) == 6, sorted(bodies)
    for sym, body in bodies.items():
        bad = [l for l in body if l.startswith(("global_atomic", "flat_atomic", "buffer_atomic", "buffer_wbl2", "scratch_", "ds_add", "ds_cmpst"))]
        assert not bad, (sym, bad[:4])
        assert any(l.startswith("global_store") for l in body), sym
        # the 9 x 16 bytes of the instance slab are loaded twice in the text (prologue + prefetch); the group row adds 4
        quads = [l for l in body if l.startswith("global_load_dwordx4")]
        assert len(quads) >= 4, (sym, len(quads))


# --- with a live context ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_calls_write_nothing(ctx):
    import torch
    lib, I = ctx.lib, abi.VD_ERR_INVALID_ARG
    cam, groups, meshes, inst, P = _host_args()
    d_g, d_m, d_i = ctx.upload(groups), ctx.upload(meshes), ctx.upload(inst)
    d_out = torch.full((4 * 20,), 0xAB, dtype=torch.uint8, device=ctx.torch_device)
    d_ids = torch.full((64,), 0xAB, dtype=torch.uint8, device=ctx.torch_device)
    d_cnt = torch.full((4,), 7, dtype=torch.int32, device=ctx.torch_device)
    p = lambda t: t.data_ptr()
    camp = cam.ctypes.data

    def compact(camera=camp, params=P, g=p(d_g), ng=2, m=p(d_m), nm=4, i=p(d_i), n=4, out=p(d_out), cnt=p(d_cnt)):
        return lib.vd_cull_compact_lod_dev(ctx.h, camera, params, g, ng, m, nm, i, n, out, cnt, 1)

    def batch(camera=camp, params=P, g=p(d_g), ng=2, m=p(d_m), nm=4, i=p(d_i), n=4, cmds=p(d_out), ids=p(d_ids), cnt=p(d_cnt)):
        return lib.vd_cull_batch_lod_dev(ctx.h, camera, params, g, ng, m, nm, i, n, cmds, ids, cnt)

    def ids(camera=camp, params=P, g=p(d_g), ng=2, nm=4, i=p(d_i), n=4, out=p(d_ids), width=1):
        return lib.vd_lod_ids_dev(ctx.h, camera, params, g, ng, nm, i, n, out, width)

    for fn in (compact, batch, ids):
        assert fn(camera=None) == I and fn(g=None) == I and fn(ng=0) == I and fn(nm=0) == I and fn(i=None) == I, fn.__name__
        for bad in (abi.LodParams(float("nan"), 0.1, 0, 0), abi.LodParams(float("inf"), 0.1, 0, 0), abi.LodParams(-1.0, 0.1, 0, 0),
                    abi.LodParams(500, 0.0, 0, 0), abi.LodParams(500, -1.0, 0, 0), abi.LodParams(500, float("nan"), 0, 0),
                    abi.LodParams(500, float("inf"), 0, 0), abi.LodParams(500, 0.1, -1.0, 0), abi.LodParams(500, 0.1, float("nan"), 0),
                    abi.LodParams(500, 0.1, float("inf"), 0)):
            assert fn(params=bad) == I, (fn.__name__, bad.scale, bad.min_distance, bad.min_size)
    assert compact(m=None) == I and compact(out=None) == I and compact(cnt=None) == I
    assert batch(m=None) == I and batch(cmds=None) == I and batch(ids=None) == I and batch(cnt=None) == I
    assert batch(nm=abi.BATCH_MAX_MESHES + 1) == I
    assert ids(out=None) == I and ids(width=3) == I and ids(width=0) == I and ids(out=p(d_ids) + 4) == I
    assert ids(nm=257, width=1) == I and ids(nm=65537, width=2) == I
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xAB).all() and (d_ids.cpu().numpy() == 0xAB).all() and (d_cnt.cpu().numpy() == 7).all()
    assert b"vd_lod_ids" in lib.vd_last_error(ctx.h)
    # n_inst == 0: the count is set, nothing else is touched; the instanced form writes its empty commands
    assert compact(n=0, i=None, out=None) == abi.VD_OK and ids(n=0, i=None, out=None) == abi.VD_OK
    torch.cuda.synchronize()
    assert d_cnt.cpu().numpy().tolist() == [0, 7, 7, 7] and (d_out.cpu().numpy() == 0xAB).all()
    assert batch(n=0, i=None, ids=None) == abi.VD_OK
    torch.cuda.synchronize()
    cmds = d_out.cpu().numpy().view(abi.DRAW)
    assert (cmds["instance_count"] == 0).all() and (cmds["base_instance"] == 0).all()


@pytest.mark.gpu
def test_the_host_form_rejects_bad_tables(ctx):
    cam, groups, meshes, inst, P = _host_args()
    out, k = ctx.cull_compact_lod(cam, P, groups, meshes, inst)
    assert k <= 4
    for field, g, value in (("n_lods", 0, 0), ("n_lods", 1, 9), ("first_row", 1, 3), ("first_row", 0, 0xFFFFFFFF)):
        bad = groups.copy()
        bad[field][g] = value
        buf, cnt = np.full(4 * 20, 0xAB, np.uint8), np.full(1, 7, np.uint32)
        rc = ctx.lib.vd_cull_compact_lod(ctx.h, cam.ctypes.data, P, bad.ctypes.data, 2, meshes.ctypes.data, 4, inst.ctypes.data, 4,
                                         buf.ctypes.data, cnt.ctypes.data, 0)
        assert rc == abi.VD_ERR_INVALID_ARG, (field, g, value)
        assert (buf == 0xAB).all() and cnt[0] == 7
