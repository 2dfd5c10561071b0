"""vd_shadow_pass_dev and vd_shadow_pass_prepared_dev at the ABI (include/voidin_shadow.h), without a GPU: the layout of VdLight and
VdShadowPassInfo as the C compiler and as Python see them; declared in the new header and nowhere in voidin_abi.h; bound by a table
of their own and exported; what they answer before a device is touched.  (With a device: tests/test_gpu_shadow_pass.py.)"""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT
from voidin_amd import abi

NEW = ("vd_shadow_pass_dev", "vd_shadow_pass_prepared_dev")
INCLUDE = os.path.join(ROOT, "include")


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def test_light_layout_as_c11_sees_it():
    prog = ('#include <stddef.h>\n#include "voidin_shadow.h"\n'
            "_Static_assert(sizeof(VdLight) == 32, \"light.rs:55-62\");\n"
            "_Static_assert(offsetof(VdLight, position) == 0 && offsetof(VdLight, radius) == 12, \"position, radius\");\n"
            "_Static_assert(offsetof(VdLight, color) == 16 && offsetof(VdLight, _pad) == 28, \"color, pad\");\n"
            "_Static_assert(sizeof(VdShadowPassInfo) == 16 && offsetof(VdShadowPassInfo, n_rays) == 0, \"info\");\n"
            "_Static_assert(offsetof(VdShadowPassInfo, n_chunks) == 4 && offsetof(VdShadowPassInfo, words_per_point) == 8, \"info\");\n"
            "_Static_assert(VD_SHADOW_MAX_LIGHTS == 1024u, \"lights per call\");\n"
            "int main(void) { return vd_shadow_pass_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == vd_shadow_pass_prepared_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-x", "c", "-"], input=prog,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_light_layout_as_python_sees_it():
    L = abi.LIGHT
    assert L.itemsize == 32 and [L.fields[f][1] for f in ("position", "radius", "color", "_pad")] == [0, 12, 16, 28]
    S = abi.ShadowPassInfo
    assert C.sizeof(S) == 16 and [S.n_rays.offset, S.n_chunks.offset, S.words_per_point.offset] == [0, 4, 8]
    assert abi.SHADOW_MAX_LIGHTS == 1024


def test_the_symbols_are_declared_in_the_new_header_bound_apart_and_exported():
    shadow, base = _code("voidin_shadow.h"), _code("voidin_abi.h")
    assert sorted(set(re.findall(r"\b(vd_[a-z_0-9]+)\s*\(", shadow))) == sorted(NEW) == sorted(abi.SHADOW_PROTOTYPES)
    assert '#include "voidin_abi.h"' in shadow
    lib = abi.load()
    for name in NEW:
        assert not (set(abi.SHADOW_PROTOTYPES) & set(abi.PROTOTYPES))
        assert hasattr(lib, name) and getattr(lib, name).argtypes == abi.SHADOW_PROTOTYPES[name][1], name
    # voidin_abi.h knows none of it: its tables (tests/test_abi_symbols.py, the write-set and stream-order inventories) are about it alone
    for word in NEW + ("VdLight", "VdShadowPassInfo", "VD_SHADOW_MAX_LIGHTS", "voidin_shadow"):
        assert word not in base, word


def test_null_context_is_an_error_before_any_device_is_touched():
    lib = abi.load()
    scene, info = abi.TraceScene(), abi.ShadowPassInfo(7, 7, 7, 7)
    assert lib.vd_shadow_pass_dev(None, None, None, None, 0, None, 0, 0, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shadow_pass_dev(None, C.byref(scene), 1 << 12, 1 << 12, 4, 1 << 12, 4, 0, 1 << 12, None, C.byref(info)) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shadow_pass_prepared_dev(None, None, None, None, 0, None, 0, 0, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shadow_pass_prepared_dev(None, 1 << 12, 1 << 12, 1 << 12, 4, 1 << 12, 4, 0, 1 << 12, None, C.byref(info)) == abi.VD_ERR_INVALID_ARG
    assert (info.n_rays, info.n_chunks, info.words_per_point) == (7, 7, 7)      # nothing is read or written without a context


def test_the_cpp_mirror_has_the_wrappers():
    hpp = open(os.path.join(INCLUDE, "voidin.hpp")).read()
    assert '#include "voidin_shadow.h"' in hpp and "inline VdShadowPassInfo shadow_pass(const Gpu& gpu" in hpp and "vd_shadow_pass_dev(" in hpp
    cls = hpp[hpp.index("class TraceScene {"):]
    cls = cls[: cls.index("\n};")]
    assert "VdShadowPassInfo shadow_pass(" in cls and "vd_shadow_pass_prepared_dev" in cls


def test_integration_md_has_the_rust_lines_outside_the_ffi_block():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = doc[doc.index("<!-- ffi:begin -->"): doc.index("<!-- ffi:end -->")]
    for name in NEW:
        assert f"pub fn {name}(" in doc and f"pub fn {name}(" not in block, name
