"""The wide walk and the LBVH top level at the ABI, without a GPU: the struct the wide calls take, what they answer before the
device is touched, the registers of the wide kernels against their narrow counterparts (from the code object's metadata), and
the C++ mirror's new members."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from voidin_amd import abi

CSRC = os.path.join(ROOT, "voidin_amd", "csrc")


def test_trace_scene_wide_layout():
    """VdTraceSceneWide is VdTraceScene with another node type: six {pointer, u32} pairs, 16 bytes each."""
    S = abi.TraceSceneWide
    assert C.sizeof(S) == 96 == C.sizeof(abi.TraceScene)
    names = ["tlas_nodes", "instances", "meshes", "bvh_nodes", "vertices", "indices"]
    for k, name in enumerate(names):
        assert getattr(S, name).offset == 16 * k and getattr(S, "n_" + name).offset == 16 * k + 8, name
    assert abi.TLAS_NODE_WIDE.itemsize == 48 and abi.TLAS_NODE_WIDE.fields["left"][1] == 12 and abi.TLAS_NODE_WIDE.fields["right"][1] == 28
    assert abi.TLAS_NODE_WIDE.fields["instance_idx"][1] == 32
    src = open(os.path.join(ROOT, "include", "voidin_abi.h")).read()
    assert re.search(r"#define\s+VD_TLAS_WIDE_MAX_INSTANCES\s+\(1u << 24\)", src) and abi.TLAS_WIDE_MAX_INSTANCES == 1 << 24
    # the C compiler's view of the same struct
    prog = ('#include <stddef.h>\n#include "voidin_abi.h"\n'
            "_Static_assert(sizeof(VdTraceSceneWide) == 96 && offsetof(VdTraceSceneWide, n_tlas_nodes) == 8, \"wide scene\");\n"
            "_Static_assert(offsetof(VdTraceSceneWide, instances) == 16 && offsetof(VdTraceSceneWide, indices) == 80, \"wide scene\");\n"
            "_Static_assert(offsetof(VdTraceSceneWide, n_indices) == 88, \"wide scene\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_null_context_is_an_error():
    lib = abi.load()
    s = abi.TraceSceneWide()
    for fn in (lib.vd_trace_wide_dev, lib.vd_trace_any_wide_dev, lib.vd_trace_wide):
        assert fn(None, C.byref(s), None, 4, None) == abi.VD_ERR_INVALID_ARG
        assert fn(None, None, None, 0, None) == abi.VD_ERR_INVALID_ARG
    for fn in (lib.vd_tlas_build_lbvh, lib.vd_tlas_build_lbvh_dev, lib.vd_tlas_build_lbvh_wide, lib.vd_tlas_build_lbvh_wide_dev):
        assert fn(None, None, 0, None, 0, None) == abi.VD_ERR_INVALID_ARG
        assert fn(None, 1 << 12, 5, 1 << 12, 1, 1 << 12) == abi.VD_ERR_INVALID_ARG      # whatever the other arguments say
        assert fn(None, 1 << 12, abi.TLAS_WIDE_MAX_INSTANCES + 1, 1 << 12, 1, 1 << 12) == abi.VD_ERR_INVALID_ARG


def _kernel_metadata(text):
    """{kernel symbol: (vgpr_count, private_segment_fixed_size)} from the amdhsa.kernels metadata of a gfx950 assembly file."""
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - \.", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        vg, ps = re.search(r"vgpr_count:\s+(\d+)", blk), re.search(r"private_segment_fixed_size:\s+(\d+)", blk)
        if name and vg and ps:
            out[name.group(1)] = (int(vg.group(1)), int(ps.group(1)))
    return out


def test_wide_kernels_take_no_more_registers_than_their_narrow_counterparts(tmp_path):
    """Occupancy of the walk is set by its registers (6 waves per SIMD, 5 with the fan-out's code: trace.hip, __launch_bounds__):
    a wide kernel that needed more VGPRs or more scratch than the narrow kernel of the same {ANY, PREP, FAN} would run fewer."""
    path = str(tmp_path / "trace.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "-S", "--cuda-device-only"]
    subprocess.run(["/opt/rocm/bin/hipcc", *flags, os.path.join(CSRC, "trace.hip"), "-o", path], check=True, capture_output=True, timeout=900)
    md = _kernel_metadata(open(path).read())
    b = lambda x: "Lb1E" if x else "Lb0E"

    def find(fragment):
        hit = [k for k in md if fragment in k]
        assert len(hit) == 1, (fragment, hit)
        return md[hit[0]]

    pairs = 0
    for any_ in (0, 1):
        for prep in (0, 1):
            for fan in (0, 1):
                narrow = find(("trace_single_prep_kernelI" if prep else "trace_single_kernelI") + b(any_) + b(fan) + "EE")
                wide = find("trace_wide_kernelI" + b(any_) + b(prep) + b(fan) + "EE")
                assert wide[0] <= narrow[0] and wide[1] <= narrow[1], ("first pass", any_, prep, fan, wide, narrow)
                pairs += 1
            narrow, wide = find("trace_deep_kernelI" + b(any_) + b(prep) + "EE"), find("trace_deep_wide_kernelI" + b(any_) + b(prep) + "EE")
            assert wide[0] <= narrow[0] and wide[1] <= narrow[1], ("second pass", any_, prep, wide, narrow)
            pairs += 1
    assert pairs == 12


def _build_mirror():
    src = os.path.join(ROOT, "tests", "cpp", "trace_wide_mirror_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "trace_wide_mirror_test")
    newest = max(os.path.getmtime(src), os.path.getmtime(os.path.join(ROOT, "include", "voidin.hpp")),
                 os.path.getmtime(os.path.join(ROOT, "include", "voidin_abi.h")))
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), src,
               "-L", CSRC, "-lvoidin_hip", f"-Wl,-rpath,{CSRC}", "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_wide_mirror_compiles_and_links():
    """Tlas::build_fast, TlasWide and traverse_tlas(gpu, VdTraceSceneWide, rays) of include/voidin.hpp against the C ABI."""
    assert os.path.exists(_build_mirror())


@pytest.mark.gpu
def test_wide_mirror_gives_the_same_records_over_four_top_levels():
    out = subprocess.run(["timeout", "600", _build_mirror()], capture_output=True, text=True, timeout=700)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "trace_wide_mirror_test OK" in out.stdout, out.stdout
