"""vd_cull_compact_views / vd_cull_compact_views_dev (several cameras in one read of the instances) without a GPU: the
library exports both, a null context is a return code, and the emitted gfx950 code of every instantiation of the
multi-view pass 1 holds its cameras without spilling.  (tests/test_gpu_cull_views.py is the run-time half; the argument
checks that need a live context are there.)"""
import ctypes as C
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
KERNEL = "cull_mask_views_kernel"


def test_library_exports_both_entry_points():
    lib = abi.load()
    for name in ("vd_cull_compact_views_dev", "vd_cull_compact_views"):
        assert name in abi.PROTOTYPES and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "voidin_abi.h")).read()
    assert int(re.search(r"#define VD_MAX_VIEWS (\d+)", header).group(1)) == abi.MAX_VIEWS == 8


def test_null_context_is_an_error_not_a_crash():
    """No context: refused, with arguments that are otherwise valid and with all of them null.  (The other argument
    errors need a live context to be told apart: tests/test_gpu_cull_views.py::test_invalid_arguments_and_empty_input.)"""
    lib = abi.load()
    cams = np.zeros(2, abi.CAMERA)
    meshes, inst = np.zeros(2, abi.MESH_INFO), np.zeros(4, abi.INSTANCE)
    out, cnt = np.zeros(8, abi.DRAW), np.full(2, 7, np.uint32)
    for fn in (lib.vd_cull_compact_views_dev, lib.vd_cull_compact_views):
        assert fn(None, cams.ctypes.data, 2, meshes.ctypes.data, 2, inst.ctypes.data, 4, out.ctypes.data, 4, cnt.ctypes.data, 0) == abi.VD_ERR_INVALID_ARG
        assert fn(None, None, 0, None, 0, None, 0, None, 0, None, 0) == abi.VD_ERR_INVALID_ARG
    assert (cnt == 7).all() and not out.view(np.uint8).any()          # a refused call writes nothing


@pytest.fixture(scope="module")
def cull_isa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isa") / "cull.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, os.path.join(CSRC, "cull.hip"), "-o", path], check=True, capture_output=True, timeout=600)
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


def test_no_instantiation_of_the_multi_view_pass_spills(cull_isa):
    """Eight cameras are 176 dwords - more than a wave's scalar registers - and the view loop indexes them at run time:
    they must come from scalar loads of the kernel-argument segment, not from a private (scratch) copy."""
    meta = kernel_metadata(cull_isa, KERNEL)
    assert len(meta) == 3, sorted(meta)                      # one instantiation per id width (1, 2, 4 bytes) serves every view count
    for sym, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (sym, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (sym, m)
        assert m["vgpr_count"] <= 168, (sym, m)              # three waves per SIMD, as cull_mask_tiled_kernel (__launch_bounds__(256, 3))
    bodies = kernel_bodies(cull_isa, KERNEL)
    assert sorted(bodies) == sorted(meta)
    for sym, body in bodies.items():
        assert not [l for l in body if l.startswith(("scratch_", "buffer_"))], sym
        assert sum(l.startswith("s_load_dword") for l in body) >= 10, sym     # 22 camera dwords per view + the arguments


def test_multi_view_pass_has_no_atomics_and_no_l2_writeback(cull_isa):
    """Like the single-view pass 1 (tests/test_isa_cull_two_launch.py): the kernel boundary orders masks, counts and ids
    before the expansions; the counts leave as plain dword stores."""
    bodies = kernel_bodies(cull_isa, KERNEL)
    assert len(bodies) == 3, sorted(bodies)
    for sym, body in bodies.items():
        bad = [l for l in body if l.startswith(("global_atomic", "flat_atomic", "buffer_atomic", "buffer_wbl2", "ds_add", "ds_cmpst"))]
        assert not bad, (sym, bad[:4])
        dword = [l for l in body if l.startswith("global_store_dword ")]
        assert dword and not any("sc1" in l or "sc0" in l for l in dword), (sym, dword)
        assert any(l.startswith("global_store_dwordx2") for l in body), sym          # the ballot words
        assert sum(l.startswith("global_load_dwordx4") and " nt" in l for l in body) >= 9, sym   # the instance stream stays nontemporal
