"""vd_lighting_dev, vd_shade_gbuffer_dev and vd_shade_gbuffer_prepared_dev at the ABI (include/voidin_lighting.h), without a GPU: the
layout of VdFlatMaterial and VdColorTarget as the C compiler and as Python see them; declared in the new header and in none of the
four older ones; bound by a table of their own and exported; what they answer before a device is touched; the mirrors, the Makefile
and the documents.  (With a device: tests/test_gpu_lighting.py.)"""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT
from voidin_amd import abi

NEW = ("vd_lighting_dev", "vd_shade_gbuffer_dev", "vd_shade_gbuffer_prepared_dev")
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "voidin_amd", "csrc")


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def test_layouts_as_c11_sees_them():
    prog = ('#include <stddef.h>\n#include "voidin_lighting.h"\n'
            "_Static_assert(sizeof(VdFlatMaterial) == 32 && offsetof(VdFlatMaterial, albedo) == 0 && offsetof(VdFlatMaterial, specular) == 12, \"albedo, specular\");\n"
            "_Static_assert(offsetof(VdFlatMaterial, emissive) == 16 && offsetof(VdFlatMaterial, _pad) == 28, \"emissive\");\n"
            "_Static_assert(sizeof(VdColorTarget) == 24 && offsetof(VdColorTarget, rgba) == 0 && offsetof(VdColorTarget, pitch) == 8, \"rgba, pitch\");\n"
            "_Static_assert(offsetof(VdColorTarget, width) == 12 && offsetof(VdColorTarget, height) == 16, \"sizes\");\n"
            "_Static_assert(VD_LIGHTING_MATERIALS == 256u && sizeof(VdGBuffer) == 56 && sizeof(VdLight) == 32, \"voidin_gbuffer.h and voidin_shadow.h come with it\");\n"
            "int main(void) { VdColorTarget t = {0}; float p; t.rgba = &p; *t.rgba = 1.0f;      /* writable */\n"
            "  return vd_lighting_dev(0, 0, 0, 0, 0, 0, 0, 0, &t) + vd_shade_gbuffer_dev(0, 0, 0, 0, 0, 0, 0, 0, &t, 0)\n"
            "       + vd_shade_gbuffer_prepared_dev(0, 0, 0, 0, 0, 0, 0, 0, &t, 0); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-x", "c", "-"], input=prog,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_layouts_as_python_sees_them():
    M = abi.FLAT_MATERIAL
    assert M.itemsize == 32 and [M.fields[f][1] for f in ("albedo", "specular", "emissive", "_pad")] == [0, 12, 16, 28]
    T = abi.ColorTarget
    assert C.sizeof(T) == 24 and [getattr(T, f).offset for f in ("rgba", "pitch", "width", "height")] == [0, 8, 12, 16]
    assert abi.LIGHTING_MATERIALS == 256


def test_the_symbols_are_declared_in_the_new_header_bound_apart_and_exported():
    new = _code("voidin_lighting.h")
    older = {n: _code(n) for n in ("voidin_gbuffer_trace.h", "voidin_gbuffer.h", "voidin_shadow.h", "voidin_abi.h")}
    assert sorted(set(re.findall(r"\b(vd_[a-z_0-9]+)\s*\(", new))) == sorted(NEW) == sorted(abi.LIGHTING_PROTOTYPES)
    assert '#include "voidin_gbuffer.h"' in new
    assert not (set(abi.LIGHTING_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.SHADOW_PROTOTYPES) | set(abi.GBUFFER_PROTOTYPES) | set(abi.GBUFFER_TRACE_PROTOTYPES)))
    lib = abi.load()
    for name in NEW:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == abi.LIGHTING_PROTOTYPES[name][1], name
    for word in NEW + ("VdFlatMaterial", "VdColorTarget", "voidin_lighting", "VD_LIGHTING_MATERIALS"):
        for name, text in older.items():
            assert word not in text, (word, name)


def test_null_context_is_an_error_before_any_device_is_touched():
    lib = abi.load()
    gb = abi.GBuffer(1 << 12, 256, 1 << 12, 512, 1 << 12, 64, 64, 64)
    tg = abi.ColorTarget(1 << 12, 1024, 64, 64)
    scene = abi.TraceScene()
    assert lib.vd_lighting_dev(None, None, None, None, 0, None, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_lighting_dev(None, 1 << 12, C.byref(gb), 1 << 12, 4, 1 << 12, 1 << 12, 1 << 12, C.byref(tg)) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shade_gbuffer_dev(None, None, None, None, None, 0, 0, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shade_gbuffer_dev(None, C.byref(scene), 1 << 12, C.byref(gb), 1 << 12, 4, 0, 1 << 12, C.byref(tg), None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shade_gbuffer_prepared_dev(None, None, None, None, None, 0, 0, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shade_gbuffer_prepared_dev(None, 1 << 12, 1 << 12, C.byref(gb), 1 << 12, 4, 0, 1 << 12, C.byref(tg), None) == abi.VD_ERR_INVALID_ARG


def test_the_python_mirror_has_the_calls():
    from voidin_amd.runtime import Context
    for name in ("color_target", "lighting_dev", "shade_gbuffer_dev", "shade_gbuffer_prepared_dev"):
        assert callable(getattr(Context, name)), name
    tg = Context.color_target(1 << 12, 17, 5)
    assert isinstance(tg, abi.ColorTarget) and (tg.rgba, tg.pitch, tg.width, tg.height) == (1 << 12, 272, 17, 5)      # packed by default
    tg = Context.color_target(1 << 12, 17, 5, 512)
    assert (tg.rgba, tg.pitch, tg.width, tg.height) == (1 << 12, 512, 17, 5)


def test_the_cpp_mirror_has_the_wrappers():
    hpp = open(os.path.join(INCLUDE, "voidin.hpp")).read()
    assert '#include "voidin_lighting.h"' in hpp
    for decl, call in (("inline void lighting(const Gpu& gpu", "vd_lighting_dev("), ("inline VdShadowGBufferInfo shade_gbuffer(const Gpu& gpu", "vd_shade_gbuffer_dev(")):
        assert decl in hpp and call in hpp, decl
    cls = hpp[hpp.index("class TraceScene {"):]
    cls = cls[: cls.index("\n};")]
    assert "VdShadowGBufferInfo shade_gbuffer(" in cls and "vd_shade_gbuffer_prepared_dev" in cls
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "lighting_mirror_test.cpp"))


def test_the_source_is_built_and_the_older_files_do_not_know_it():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\blighting\.hip\b", mk, re.M) and "../../include/voidin_lighting.h" in mk
    for older in ("shadow.hip", "trace.hip", "gbuffer.hip", "gbuffer_trace.hip"):
        assert "lighting" not in open(os.path.join(CSRC, older)).read().lower(), older
    src = open(os.path.join(CSRC, "lighting.hip")).read()
    assert "vd_shadow_gbuffer_dev(" in src and "vd_shadow_gbuffer_prepared_dev(" in src      # the pass is reached through its exported entry points
    assert len(re.findall(r"__global__", src)) == 1


def test_the_documents_name_it():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = doc[doc.index("<!-- ffi:begin -->"): doc.index("<!-- ffi:end -->")]
    for name in NEW:
        assert f"pub fn {name}(" in doc and f"pub fn {name}(" not in block, name
    assert "VdFlatMaterial" in doc and "VdColorTarget" in doc and "vd_gbuffer_trace_dev" in doc
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "vd_lighting_dev" in text and "vd_shade_gbuffer" in text, name
