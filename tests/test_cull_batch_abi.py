"""vd_batch_mask_dev / vd_cull_batch_dev / vd_cull_batch (instanced draw lists: one command per mesh, survivors grouped by
mesh) without a GPU: the library exports the three, a null context is a return code that writes nothing, the mesh limit of the
header is the mirror's, and the emitted gfx950 code of every new kernel keeps its state in registers and LDS - and, for the
scatter, decides no position with an atomic.  (tests/test_gpu_cull_batch.py is the run-time half; the argument checks that
need a live context are there.)"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from voidin_amd import abi

CSRC = os.path.join(ROOT, "voidin_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-S", "--cuda-device-only"]
SYMBOLS = ("vd_batch_mask_dev", "vd_cull_batch_dev", "vd_cull_batch")
# kernel -> instantiations (the walks over the instances exist once per id width)
KERNELS = {"batch_hist_kernel": 3, "batch_scan_kernel": 1, "batch_cmds_kernel": 1, "batch_scatter_kernel": 3}


def test_library_exports_the_three_entry_points():
    lib = abi.load()
    for name in SYMBOLS:
        assert name in abi.PROTOTYPES and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "voidin_abi.h")).read()
    assert int(re.search(r"#define VD_BATCH_MAX_MESHES (\d+)u", header).group(1)) == abi.BATCH_MAX_MESHES == 4096


def test_null_context_is_an_error_not_a_crash():
    """No context: refused, with arguments that are otherwise valid and with all of them null; nothing is written."""
    lib = abi.load()
    cam = np.zeros(1, abi.CAMERA)
    meshes, inst = np.zeros(2, abi.MESH_INFO), np.zeros(4, abi.INSTANCE)
    mask, table = np.full(1, 0xF, np.uint64), np.zeros(4, np.uint32)
    cmds, ids, cnt = np.full(2 * 20, 0xAB, np.uint8), np.full(4, 0xABABABAB, np.uint32), np.full(1, 7, np.uint32)
    assert lib.vd_batch_mask_dev(None, mask.ctypes.data, 4, table.ctypes.data, 4, meshes.ctypes.data, 2, cmds.ctypes.data, ids.ctypes.data,
                                 cnt.ctypes.data) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_batch_mask_dev(None, None, 0, None, 0, None, 0, None, None, None) == abi.VD_ERR_INVALID_ARG
    for fn in (lib.vd_cull_batch_dev, lib.vd_cull_batch):
        assert fn(None, cam.ctypes.data, meshes.ctypes.data, 2, inst.ctypes.data, 4, cmds.ctypes.data, ids.ctypes.data, cnt.ctypes.data) == abi.VD_ERR_INVALID_ARG
        assert fn(None, None, None, 0, None, 0, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert (cnt == 7).all() and (cmds == 0xAB).all() and (ids == 0xABABABAB).all()


@pytest.fixture(scope="module")
def batch_isa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isa") / "batch.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, os.path.join(CSRC, "batch.hip"), "-o", path], check=True, capture_output=True, timeout=600)
    return open(path).read()


def kernel_metadata(text, fragment):
    """{symbol: {key: int}} from the code-object metadata (amdhsa.kernels) of every kernel whose symbol contains `fragment`."""
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


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_new_kernel_uses_private_memory_or_spills(batch_isa, kernel):
    meta = kernel_metadata(batch_isa, kernel)
    assert len(meta) == KERNELS[kernel], sorted(meta)
    for sym, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (sym, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (sym, m)
    bodies = kernel_bodies(batch_isa, kernel)
    assert sorted(bodies) == sorted(meta)
    for sym, body in bodies.items():
        assert not [l for l in body if l.startswith("scratch_")], sym


def test_every_kernel_of_the_file_is_covered(batch_isa):
    names = set(re.findall(r"\.name:\s+(\S+)", batch_isa[batch_isa.index("amdhsa.kernels:"):]))
    assert len(names) == sum(KERNELS.values()) and all(any(k in n for k in KERNELS) for n in names), sorted(names)


def test_no_global_atomic_decides_where_an_id_lands(batch_isa):
    """The scatter's positions are cursor + ballot rank: no atomic on memory in any instantiation (and none on LDS either -
    the cursors are advanced by plain stores of the round's last peer); the ids leave as plain dword stores."""
    bodies = kernel_bodies(batch_isa, "batch_scatter_kernel")
    assert len(bodies) == 3, sorted(bodies)
    for sym, body in bodies.items():
        bad = [l for l in body if l.startswith(("global_atomic", "flat_atomic", "buffer_atomic", "ds_add", "ds_cmpst"))]
        assert not bad, (sym, bad[:4])
        assert any(l.startswith("global_store_dword ") for l in body), sym
        assert any(l.startswith("v_mbcnt") or l.startswith("s_bcnt1") or l.startswith("v_bcnt") for l in body), sym   # the rank is a popcount
    # the other kernels touch memory with plain loads and stores only; the histogram counts in LDS
    for kernel in ("batch_hist_kernel", "batch_scan_kernel", "batch_cmds_kernel"):
        for sym, body in kernel_bodies(batch_isa, kernel).items():
            assert not [l for l in body if l.startswith(("global_atomic", "flat_atomic", "buffer_atomic"))], sym
