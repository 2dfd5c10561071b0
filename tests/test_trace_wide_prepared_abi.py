"""vd_trace_prepare_wide_dev, vd_trace_accel_refit_dev and vd_trace_accel_info_wide at the ABI, without a GPU: declared, bound and
exported; what they answer before a device is touched; the layout of VdTraceAccelInfoWide as Python and as the C compiler see it."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT
from voidin_amd import abi

NEW = ("vd_trace_prepare_wide_dev", "vd_trace_accel_refit_dev", "vd_trace_accel_info_wide")


def test_the_three_symbols_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "voidin_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = abi.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in abi.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert "do not exist" not in src[src.index("typedef struct VdTraceSceneWide") - 1500: src.index("typedef struct VdTraceSceneWide")]


def test_null_arguments_are_errors_before_any_device_is_touched():
    lib = abi.load()
    scene, out, info = abi.TraceSceneWide(), C.c_void_p(), abi.TraceAccelInfoWide()
    # no context: whatever the other arguments say
    assert lib.vd_trace_prepare_wide_dev(None, C.byref(scene), C.byref(out)) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_trace_prepare_wide_dev(None, None, None) == abi.VD_ERR_INVALID_ARG
    assert out.value is None
    assert lib.vd_trace_accel_refit_dev(None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_trace_accel_refit_dev(None, 1 << 12) == abi.VD_ERR_INVALID_ARG          # the handle is not read without a context
    # no accel / nowhere to put the answer
    assert lib.vd_trace_accel_info_wide(None, C.byref(info)) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_trace_accel_info_wide(None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_trace_accel_info_wide(1 << 12, None) == abi.VD_ERR_INVALID_ARG          # ... nor without a place for the answer
    # the calls that now take either kind of handle still refuse none
    assert lib.vd_trace_prepared_dev(None, None, None, 4, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_trace_any_prepared_dev(None, None, None, 4, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_trace_accel_update_dev(None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_trace_accel_update_geometry_dev(None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_trace_release(None, None) == abi.VD_ERR_INVALID_ARG


def test_accel_info_wide_layout():
    S = abi.TraceAccelInfoWide
    assert C.sizeof(S) == 32 and S.d_tlas_nodes.offset == 24 and S.triangle_bytes.offset == 16 and S.refits_since_build.offset == 12
    assert [S.tight_tlas.offset, S.n_tlas_nodes.offset, S.tight_fallback_instances.offset] == [0, 4, 8]
    prog = ('#include <stddef.h>\n#include "voidin_abi.h"\n'
            "_Static_assert(sizeof(VdTraceAccelInfoWide) == 32 && offsetof(VdTraceAccelInfoWide, d_tlas_nodes) == 24, \"wide accel info\");\n"
            "_Static_assert(offsetof(VdTraceAccelInfoWide, refits_since_build) == 12 && offsetof(VdTraceAccelInfoWide, triangle_bytes) == 16, \"wide accel info\");\n"
            "_Static_assert(sizeof(VdTraceAccelInfo) == 32, \"the narrow one is unchanged\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_the_cpp_mirror_has_the_new_members():
    hpp = open(os.path.join(ROOT, "include", "voidin.hpp")).read()
    cls = hpp[hpp.index("class TraceScene {"):]
    cls = cls[: cls.index("\n};")]
    assert "const VdTraceSceneWide& d_scene" in cls and "vd_trace_prepare_wide_dev" in cls
    assert "void refit()" in cls and "vd_trace_accel_refit_dev" in cls
    assert "VdTraceAccelInfoWide info_wide() const" in cls and "vd_trace_accel_info_wide" in cls
