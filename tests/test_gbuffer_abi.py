"""vd_gbuffer_points_dev, vd_shadow_gbuffer_dev and vd_shadow_gbuffer_prepared_dev at the ABI (include/voidin_gbuffer.h), without a GPU:
the layout of VdGBuffer and VdShadowGBufferInfo as the C compiler and as Python see them; declared in the new header and in neither
voidin_shadow.h nor voidin_abi.h; bound by a table of their own and exported; what they answer before a device is touched.
(With a device: tests/test_gpu_shadow_gbuffer.py.)"""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT
from voidin_amd import abi

NEW = ("vd_gbuffer_points_dev", "vd_shadow_gbuffer_dev", "vd_shadow_gbuffer_prepared_dev")
INCLUDE = os.path.join(ROOT, "include")


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def test_layouts_as_c11_sees_them():
    prog = ('#include <stddef.h>\n#include "voidin_gbuffer.h"\n'
            "_Static_assert(sizeof(VdGBuffer) == 56, \"three images and the sizes\");\n"
            "_Static_assert(offsetof(VdGBuffer, depth) == 0 && offsetof(VdGBuffer, depth_pitch) == 8, \"depth\");\n"
            "_Static_assert(offsetof(VdGBuffer, normal_uv) == 16 && offsetof(VdGBuffer, normal_uv_pitch) == 24, \"normal_uv\");\n"
            "_Static_assert(offsetof(VdGBuffer, material) == 32 && offsetof(VdGBuffer, material_pitch) == 40, \"material\");\n"
            "_Static_assert(offsetof(VdGBuffer, width) == 44 && offsetof(VdGBuffer, height) == 48, \"sizes\");\n"
            "_Static_assert(sizeof(VdShadowGBufferInfo) == 16 && offsetof(VdShadowGBufferInfo, n_points) == 0, \"info\");\n"
            "_Static_assert(offsetof(VdShadowGBufferInfo, n_rays) == 4 && offsetof(VdShadowGBufferInfo, n_chunks) == 8, \"info\");\n"
            "_Static_assert(offsetof(VdShadowGBufferInfo, words_per_point) == 12, \"info\");\n"
            "_Static_assert(VD_GBUFFER_NO_MATERIAL == 0u && VD_GBUFFER_LIGHT_MATERIAL == 2u, \"raytraced_shadows.wgsl:80, shared.wgsl:1\");\n"
            "_Static_assert(sizeof(VdLight) == 32 && VD_SHADOW_MAX_LIGHTS == 1024u, \"voidin_shadow.h comes with it\");\n"
            "int main(void) { return vd_gbuffer_points_dev(0, 0, 0, 0, 0, 0, 0, 0) + vd_shadow_gbuffer_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)\n"
            "                        + vd_shadow_gbuffer_prepared_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-x", "c", "-"], input=prog,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_layouts_as_python_sees_them():
    G = abi.GBuffer
    assert C.sizeof(G) == 56
    assert [getattr(G, f).offset for f in ("depth", "depth_pitch", "normal_uv", "normal_uv_pitch", "material", "material_pitch", "width", "height")] == \
        [0, 8, 16, 24, 32, 40, 44, 48]
    S = abi.ShadowGBufferInfo
    assert C.sizeof(S) == 16 and [S.n_points.offset, S.n_rays.offset, S.n_chunks.offset, S.words_per_point.offset] == [0, 4, 8, 12]
    assert (abi.GBUFFER_NO_MATERIAL, abi.GBUFFER_LIGHT_MATERIAL) == (0, 2)


def test_the_symbols_are_declared_in_the_new_header_bound_apart_and_exported():
    gbuffer, shadow, base = _code("voidin_gbuffer.h"), _code("voidin_shadow.h"), _code("voidin_abi.h")
    assert sorted(set(re.findall(r"\b(vd_[a-z_0-9]+)\s*\(", gbuffer))) == sorted(NEW) == sorted(abi.GBUFFER_PROTOTYPES)
    assert '#include "voidin_shadow.h"' in gbuffer
    assert not (set(abi.GBUFFER_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.SHADOW_PROTOTYPES)))
    lib = abi.load()
    for name in NEW:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == abi.GBUFFER_PROTOTYPES[name][1], name
    # the two older headers know none of it: their tables and inventories are about them alone
    for word in NEW + ("VdGBuffer", "VdShadowGBufferInfo", "VD_GBUFFER_", "voidin_gbuffer"):
        assert word not in base and word not in shadow, word


def test_null_context_is_an_error_before_any_device_is_touched():
    lib = abi.load()
    gb = abi.GBuffer(1 << 12, 256, 1 << 12, 512, 1 << 12, 64, 64, 64)
    scene, info, n = abi.TraceScene(), abi.ShadowGBufferInfo(7, 7, 7, 7), C.c_uint32(7)
    assert lib.vd_gbuffer_points_dev(None, None, None, None, None, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_gbuffer_points_dev(None, 1 << 12, C.byref(gb), 1 << 12, 1 << 12, 1 << 12, 1 << 12, C.byref(n)) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shadow_gbuffer_dev(None, None, None, None, None, 0, 0, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shadow_gbuffer_dev(None, C.byref(scene), 1 << 12, C.byref(gb), 1 << 12, 4, 0, 1 << 12, None, C.byref(info)) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shadow_gbuffer_prepared_dev(None, None, None, None, None, 0, 0, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_shadow_gbuffer_prepared_dev(None, 1 << 12, 1 << 12, C.byref(gb), 1 << 12, 4, 0, 1 << 12, None, C.byref(info)) == abi.VD_ERR_INVALID_ARG
    assert (info.n_points, info.n_rays, info.n_chunks, info.words_per_point, n.value) == (7, 7, 7, 7, 7)      # nothing is written without a context


def test_the_python_mirror_has_the_calls():
    from voidin_amd.runtime import Context
    for name in ("gbuffer", "gbuffer_points_dev", "shadow_gbuffer_dev", "shadow_gbuffer_prepared_dev"):
        assert callable(getattr(Context, name)), name
    gb = Context.gbuffer(1 << 12, 1 << 13, 1 << 14, 17, 5)
    assert (gb.depth_pitch, gb.normal_uv_pitch, gb.material_pitch, gb.width, gb.height) == (68, 136, 17, 17, 5)      # packed by default


def test_the_cpp_mirror_has_the_wrappers():
    hpp = open(os.path.join(INCLUDE, "voidin.hpp")).read()
    assert '#include "voidin_gbuffer.h"' in hpp and "inline VdShadowGBufferInfo shadow_gbuffer(const Gpu& gpu" in hpp and "vd_shadow_gbuffer_dev(" in hpp
    assert "inline uint32_t gbuffer_points(const Gpu& gpu" in hpp and "vd_gbuffer_points_dev(" in hpp
    cls = hpp[hpp.index("class TraceScene {"):]
    cls = cls[: cls.index("\n};")]
    assert "VdShadowGBufferInfo shadow_gbuffer(" in cls and "vd_shadow_gbuffer_prepared_dev" in cls


def test_the_source_is_built_and_the_older_files_do_not_know_it():
    csrc = os.path.join(ROOT, "voidin_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\bgbuffer\.hip\b", mk, re.M) and "../../include/voidin_gbuffer.h" in mk
    for older in ("shadow.hip", "trace.hip"):
        assert "gbuffer" not in open(os.path.join(csrc, older)).read().lower(), older
    src = open(os.path.join(csrc, "gbuffer.hip")).read()
    assert "vd_shadow_pass_dev(" in src and "vd_shadow_pass_prepared_dev(" in src          # the pass is reached through its exported entry points


def test_integration_md_has_the_rust_lines_the_copies_and_the_bit_test():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = doc[doc.index("<!-- ffi:begin -->"): doc.index("<!-- ffi:end -->")]
    for name in NEW:
        assert f"pub fn {name}(" in doc and f"pub fn {name}(" not in block, name
    assert "copy_texture_to_buffer" in doc
    for image in ("copy(&gbuffer.depth,", "copy(&gbuffer.normal_uv,", "copy(&gbuffer.material,"):      # the buffer copies of the three images
        assert image in doc, image
    assert "occluded[pix * W + (i >> 5u)]" in doc and "traverse_tlas(ray).hit" in doc       # the two WGSL lines
