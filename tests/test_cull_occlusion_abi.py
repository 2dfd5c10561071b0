"""vd_cull_compact_hiz / vd_cull_compact_hiz_dev / vd_cull_early_dev / vd_cull_late_dev (occlusion-culled draw lists in one
read of the instances) without a GPU: the library exports and binds the four, a null context is a return code, every
instantiation of their pass 1 fits three waves per SIMD without spilling, the C++ mirror compiles - and every case of
tests/test_gpu_cull_occlusion.py is non-vacuous on the oracle's side (the GPU test asserts the same condition again before
it looks at a GPU result)."""
import os
import re
import subprocess

import numpy as np
import pytest

import cull_occlusion_cases as K
from conftest import ROOT
from test_cull_views_abi import FLAGS, CSRC, kernel_bodies, kernel_metadata
from voidin_amd import abi

KERNEL = "cull_mask_occ_kernel"
NAMES = ("vd_cull_compact_hiz_dev", "vd_cull_compact_hiz", "vd_cull_early_dev", "vd_cull_late_dev")


def test_library_exports_and_binds_the_four_entry_points():
    lib = abi.load()
    header = open(os.path.join(ROOT, "include", "voidin_abi.h")).read()
    for name in NAMES:
        assert name in abi.PROTOTYPES and hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, header), name
    from voidin_amd import runtime
    for method in ("cull_compact_hiz_dev", "cull_compact_hiz", "cull_early_dev", "cull_late_dev"):
        assert hasattr(runtime.Context, method), method
    for method in ("record_hiz", "record_early", "record_late"):
        assert hasattr(runtime.EmitDraws, method), method
    assert hasattr(runtime, "OcclusionState")


def test_null_context_is_an_error_not_a_crash():
    lib = abi.load()
    cam, meshes, inst = np.zeros(1, abi.CAMERA), np.zeros(2, abi.MESH_INFO), np.zeros(4, abi.INSTANCE)
    pyr, prev = np.zeros(1, np.float32), np.zeros(1, np.uint64)
    out, cnt = np.zeros(4, abi.DRAW), np.full(1, 7, np.uint32)
    c, m, i, p, v, o, k = (a.ctypes.data for a in (cam, meshes, inst, pyr, prev, out, cnt))
    assert lib.vd_cull_compact_hiz_dev(None, c, m, 2, i, 4, p, 1, 1, o, k, 0) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_cull_compact_hiz(None, c, m, 2, i, 4, p, 1, 1, o, k, 0) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_cull_early_dev(None, c, m, 2, i, 4, v, o, k, 0) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_cull_late_dev(None, c, m, 2, i, 4, p, 1, 1, v, v, o, k, 0) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_cull_late_dev(None, None, None, 0, None, 0, None, 0, 0, None, None, None, None, 0) == abi.VD_ERR_INVALID_ARG
    assert cnt[0] == 7 and not out.view(np.uint8).any()               # a refused call writes nothing


@pytest.fixture(scope="module")
def cull_isa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isa") / "cull.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, os.path.join(CSRC, "cull.hip"), "-o", path], check=True, capture_output=True, timeout=600)
    return open(path).read()


def test_every_instantiation_keeps_three_waves_per_simd_without_spilling(cull_isa):
    """{hiz, early, late} x {1-, 2-, 4-byte ids}: no scratch, no spill, and at most 168 vector registers - 512 / 3 rounded
    down to the allocation granule of 8 - which is what __launch_bounds__(256, 3) promises the launch."""
    meta = kernel_metadata(cull_isa, KERNEL)
    assert len(meta) == 9, sorted(meta)
    modes = sorted(re.search(r"I([htj])Lb([01])ELb([01])E", sym).groups() for sym in meta)
    assert modes == sorted((t, h, p) for t in "htj" for h, p in (("1", "0"), ("0", "1"), ("1", "1"))), modes
    for sym, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (sym, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (sym, m)
        assert m["vgpr_count"] <= 168, (sym, m)
    bodies = kernel_bodies(cull_isa, KERNEL)
    assert sorted(bodies) == sorted(meta)
    scratch_en = dict(re.findall(r"\.amdhsa_kernel (\S*%s\S*)[\s\S]*?\.amdhsa_enable_private_segment (\d)" % KERNEL, cull_isa))
    assert sorted(scratch_en) == sorted(meta) and set(scratch_en.values()) == {"0"}, scratch_en
    for sym, body in bodies.items():
        assert not [l for l in body if l.startswith(("scratch_", "buffer_"))], sym


def test_pass_one_streams_like_the_single_view_pass(cull_isa):
    """No atomics, no L2 write-back, plain count stores, the instance stream nontemporal - and the pyramid texels NOT:
    they are ordinary cached loads."""
    for sym, body in kernel_bodies(cull_isa, KERNEL).items():
        bad = [l for l in body if l.startswith(("global_atomic", "flat_atomic", "buffer_atomic", "buffer_wbl2", "ds_add", "ds_cmpst"))]
        assert not bad, (sym, bad[:4])
        dword = [l for l in body if l.startswith("global_store_dword ")]
        assert dword and not any("sc1" in l or "sc0" in l for l in dword), (sym, dword)
        assert any(l.startswith("global_store_dwordx2") for l in body), sym          # the ballot words
        assert sum(l.startswith("global_load_dwordx4") and " nt" in l for l in body) >= 9, sym
        texel = [l for l in body if l.startswith("global_load_dword ")]
        if "Lb1ELb" in sym:                                                          # a pyramid is bound
            assert len(texel) >= 4 and not any(" nt" in l for l in texel), (sym, texel)


def test_cpp_mirror_of_the_new_passes_compiles(tmp_path):
    """tests/cpp/occlusion_mirror_test.cpp drives record_early -> HizPyramid::build -> record_late through include/voidin.hpp
    (the GPU run of it: tests/test_gpu_cull_occlusion.py)."""
    exe = build_mirror(str(tmp_path))
    assert os.path.exists(exe)


def build_mirror(directory):
    src = os.path.join(ROOT, "tests", "cpp", "occlusion_mirror_test.cpp")
    exe = os.path.join(directory, "occlusion_mirror_test")
    lib_dir = os.path.join(ROOT, "voidin_amd", "csrc")
    abi.load()
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), src,
                    "-L", lib_dir, "-lvoidin_hip", f"-Wl,-rpath,{lib_dir}", "-o", exe], check=True, capture_output=True, timeout=900)
    return exe


def _check(oracle, n, w, h, n_mesh=16, frame=0):
    cam, meshes, inst = K.camera(frame), K.meshes_for(n_mesh), K.cloud(n, n_mesh=n_mesh)
    pyr = oracle.hiz_build(K.depth(w, h))
    _, F, V = K.oracle_sets(oracle, cam, meshes, inst, pyr, w, h)
    P = K.bits(K.random_prev(n), n)
    K.assert_not_vacuous(n, F, V, F & P, V & ~P)
    assert not ((F & P) & (V & ~P)).any() and ((F & P) | (V & ~P))[V].all()         # E and L disjoint, E | L covers V


@pytest.mark.parametrize("n", [n for n in K.SIZES if n >= K.NON_VACUOUS_FROM] + [K.FULL_SIZE])
def test_gpu_cases_are_not_vacuous_sizes(oracle, n):
    _check(oracle, n, 1920, 1080)


@pytest.mark.parametrize("w,h", K.PYRAMIDS)
def test_gpu_cases_are_not_vacuous_pyramids(oracle, w, h):
    _check(oracle, 200_000, w, h)


@pytest.mark.parametrize("n_mesh", K.MESH_COUNTS)
def test_gpu_cases_are_not_vacuous_id_widths(oracle, n_mesh):
    _check(oracle, 200_000, 1920, 1080, n_mesh=n_mesh)


@pytest.mark.parametrize("frame", [0, 1, 2])
def test_gpu_cases_are_not_vacuous_moving_camera(oracle, frame):
    _check(oracle, 200_000, 1920, 1080, frame=frame)


def test_prev_words_set_their_padding_bits():
    """The random P of the GPU tests has ones behind the last instance: 'padding bits are ignored on input' is exercised."""
    for n in (1, 63, 65, 1023, 8193):
        w = K.random_prev(n)
        assert int(w[-1] >> np.uint64(n % 64)) == (1 << (64 - n % 64)) - 1
        assert 0 < K.bits(K.random_prev(8193), 8193).sum() < 8193
