"""vd_gbuffer_rays_dev, vd_gbuffer_resolve_dev, vd_gbuffer_trace_dev and vd_gbuffer_trace_prepared_dev at the ABI
(include/voidin_gbuffer_trace.h), without a GPU: the layout of VdGBufferTarget and VdGBufferGeometry as the C compiler and as Python see
them; declared in the new header and in none of the three older ones; bound by a table of their own and exported; what they answer
before a device is touched; the mirrors, the Makefile and the documents.  (With a device: tests/test_gpu_gbuffer_trace.py.)"""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT
from voidin_amd import abi

NEW = ("vd_gbuffer_rays_dev", "vd_gbuffer_resolve_dev", "vd_gbuffer_trace_dev", "vd_gbuffer_trace_prepared_dev")
INCLUDE = os.path.join(ROOT, "include")


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def test_layouts_as_c11_sees_them():
    prog = ('#include <stddef.h>\n#include "voidin_gbuffer_trace.h"\n'
            "_Static_assert(sizeof(VdGBufferTarget) == sizeof(VdGBuffer) && sizeof(VdGBufferTarget) == 56, \"VdGBuffer's layout\");\n"
            "_Static_assert(offsetof(VdGBufferTarget, depth) == offsetof(VdGBuffer, depth) && offsetof(VdGBufferTarget, depth_pitch) == offsetof(VdGBuffer, depth_pitch), \"depth\");\n"
            "_Static_assert(offsetof(VdGBufferTarget, normal_uv) == 16 && offsetof(VdGBufferTarget, normal_uv_pitch) == 24, \"normal_uv\");\n"
            "_Static_assert(offsetof(VdGBufferTarget, material) == 32 && offsetof(VdGBufferTarget, material_pitch) == 40, \"material\");\n"
            "_Static_assert(offsetof(VdGBufferTarget, width) == 44 && offsetof(VdGBufferTarget, height) == 48, \"sizes\");\n"
            "_Static_assert(sizeof(VdGBufferGeometry) == 80 && offsetof(VdGBufferGeometry, instances) == 0 && offsetof(VdGBufferGeometry, n_instances) == 8, \"instances\");\n"
            "_Static_assert(offsetof(VdGBufferGeometry, meshes) == 16 && offsetof(VdGBufferGeometry, n_meshes) == 24, \"meshes\");\n"
            "_Static_assert(offsetof(VdGBufferGeometry, vertices) == 32 && offsetof(VdGBufferGeometry, n_vertices) == 40, \"vertices\");\n"
            "_Static_assert(offsetof(VdGBufferGeometry, indices) == 48 && offsetof(VdGBufferGeometry, n_indices) == 56, \"indices\");\n"
            "_Static_assert(offsetof(VdGBufferGeometry, normals) == 64 && offsetof(VdGBufferGeometry, tex_coords) == 72, \"attributes\");\n"
            "_Static_assert(sizeof(VdShadowGBufferInfo) == 16, \"voidin_gbuffer.h comes with it\");\n"
            "int main(void) { VdGBufferTarget t = {0}; float d; t.depth = &d; *t.depth = 1.0f;      /* writable */\n"
            "  return vd_gbuffer_rays_dev(0, 0, 0, 0, 0) + vd_gbuffer_resolve_dev(0, 0, 0, 0, &t) + vd_gbuffer_trace_dev(0, 0, 0, 0, 0, 0)\n"
            "       + vd_gbuffer_trace_prepared_dev(0, 0, 0, 0, 0); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-x", "c", "-"], input=prog,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_layouts_as_python_sees_them():
    T, G = abi.GBufferTarget, abi.GBuffer
    names = ("depth", "depth_pitch", "normal_uv", "normal_uv_pitch", "material", "material_pitch", "width", "height")
    assert C.sizeof(T) == 56 and [getattr(T, f).offset for f in names] == [getattr(G, f).offset for f in names] == [0, 8, 16, 24, 32, 40, 44, 48]
    Q = abi.GBufferGeometry
    assert C.sizeof(Q) == 80
    assert [getattr(Q, f).offset for f in ("instances", "n_instances", "meshes", "n_meshes", "vertices", "n_vertices", "indices", "n_indices", "normals",
                                           "tex_coords")] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72]


def test_the_symbols_are_declared_in_the_new_header_bound_apart_and_exported():
    new = _code("voidin_gbuffer_trace.h")
    older = {n: _code(n) for n in ("voidin_gbuffer.h", "voidin_shadow.h", "voidin_abi.h")}
    assert sorted(set(re.findall(r"\b(vd_[a-z_0-9]+)\s*\(", new))) == sorted(NEW) == sorted(abi.GBUFFER_TRACE_PROTOTYPES)
    assert '#include "voidin_gbuffer.h"' in new
    assert not (set(abi.GBUFFER_TRACE_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.SHADOW_PROTOTYPES) | set(abi.GBUFFER_PROTOTYPES)))
    lib = abi.load()
    for name in NEW:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == abi.GBUFFER_TRACE_PROTOTYPES[name][1], name
    for word in NEW + ("VdGBufferTarget", "VdGBufferGeometry", "voidin_gbuffer_trace"):
        for name, text in older.items():
            assert word not in text, (word, name)


def test_null_context_is_an_error_before_any_device_is_touched():
    lib = abi.load()
    tg = abi.GBufferTarget(1 << 12, 256, 1 << 12, 512, 1 << 12, 64, 64, 64)
    geo = abi.GBufferGeometry(1 << 12, 1, 1 << 12, 1, 1 << 12, 3, 1 << 12, 3, None, None)
    scene = abi.TraceScene()
    assert lib.vd_gbuffer_rays_dev(None, None, 0, 0, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_gbuffer_rays_dev(None, 1 << 12, 64, 64, 1 << 12) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_gbuffer_resolve_dev(None, None, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_gbuffer_resolve_dev(None, 1 << 12, C.byref(geo), 1 << 12, C.byref(tg)) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_gbuffer_trace_dev(None, None, None, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_gbuffer_trace_dev(None, C.byref(scene), None, None, 1 << 12, C.byref(tg)) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_gbuffer_trace_prepared_dev(None, None, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_gbuffer_trace_prepared_dev(None, 1 << 12, C.byref(geo), 1 << 12, C.byref(tg)) == abi.VD_ERR_INVALID_ARG


def test_the_python_mirror_has_the_calls():
    from voidin_amd.runtime import Context
    for name in ("gbuffer_target", "gbuffer_geometry", "gbuffer_rays_dev", "gbuffer_resolve_dev", "gbuffer_trace_dev", "gbuffer_trace_prepared_dev"):
        assert callable(getattr(Context, name)), name
    tg = Context.gbuffer_target(1 << 12, 1 << 13, 1 << 14, 17, 5)
    assert isinstance(tg, abi.GBufferTarget)
    assert (tg.depth_pitch, tg.normal_uv_pitch, tg.material_pitch, tg.width, tg.height) == (68, 136, 17, 17, 5)      # packed by default
    tg = Context.gbuffer_target(1 << 12, 1 << 13, 1 << 14, 17, 5, 256, 512, 19)
    assert (tg.depth, tg.normal_uv, tg.material, tg.depth_pitch, tg.normal_uv_pitch, tg.material_pitch) == (1 << 12, 1 << 13, 1 << 14, 256, 512, 19)

    class Scene:
        struct = abi.TraceScene(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)
    g = Context.gbuffer_geometry(Scene, 13, None)
    assert (g.instances, g.n_instances, g.meshes, g.n_meshes, g.vertices, g.n_vertices, g.indices, g.n_indices, g.normals, g.tex_coords) == \
        (3, 4, 5, 6, 9, 10, 11, 12, 13, None)


def test_the_cpp_mirror_has_the_wrappers():
    hpp = open(os.path.join(INCLUDE, "voidin.hpp")).read()
    assert '#include "voidin_gbuffer_trace.h"' in hpp
    for decl, call in (("inline void gbuffer_rays(const Gpu& gpu", "vd_gbuffer_rays_dev("), ("inline void gbuffer_resolve(const Gpu& gpu", "vd_gbuffer_resolve_dev("),
                       ("inline void gbuffer_trace(const Gpu& gpu", "vd_gbuffer_trace_dev(")):
        assert decl in hpp and call in hpp, decl
    cls = hpp[hpp.index("class TraceScene {"):]
    cls = cls[: cls.index("\n};")]
    assert "void gbuffer_trace(" in cls and "vd_gbuffer_trace_prepared_dev" in cls
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "gbuffer_trace_mirror_test.cpp"))


def test_the_source_is_built_and_the_older_files_do_not_know_it():
    csrc = os.path.join(ROOT, "voidin_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\bgbuffer_trace\.hip\b", mk, re.M) and "../../include/voidin_gbuffer_trace.h" in mk
    for older in ("shadow.hip", "trace.hip"):
        assert "gbuffer" not in open(os.path.join(csrc, older)).read().lower(), older
    assert "gbuffer_trace" not in open(os.path.join(csrc, "gbuffer.hip")).read().lower()
    src = open(os.path.join(csrc, "gbuffer_trace.hip")).read()
    assert "vd_trace_dev(" in src and "vd_trace_prepared_dev(" in src          # the walk is reached through its exported entry points
    assert len(re.findall(r"__global__", src)) == 2


def test_the_documents_name_it():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = doc[doc.index("<!-- ffi:begin -->"): doc.index("<!-- ffi:end -->")]
    for name in NEW:
        assert f"pub fn {name}(" in doc and f"pub fn {name}(" not in block, name
    assert "MeshPool" in doc and "tex_coords" in doc and "vd_shadow_gbuffer" in doc
    for name in ("README.md", "DESIGN.md"):
        assert "vd_gbuffer_trace" in open(os.path.join(ROOT, name)).read(), name
