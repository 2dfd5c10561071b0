"""BvhBuilder::build_fast / MeshPool::add_fast / MeshPool::rebuild_fast of the C++ mirror (include/voidin.hpp): the host compiles
against the C ABI without a GPU and, with one, rebuilds a pooled mesh in place and compares against a fresh build_fast."""
import os
import subprocess

import pytest

from conftest import ROOT

NAME = "blas_lbvh_mirror_test"


def _build():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    exe = os.path.join(ROOT, "tests", "cpp", NAME)
    newest = max(os.path.getmtime(src), os.path.getmtime(os.path.join(ROOT, "include", "voidin.hpp")),
                 os.path.getmtime(os.path.join(ROOT, "include", "voidin_abi.h")))
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), src,
               "-L", os.path.join(ROOT, "voidin_amd", "csrc"), "-lvoidin_hip", f"-Wl,-rpath,{os.path.join(ROOT, 'voidin_amd', 'csrc')}",
               "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_blas_lbvh_mirror_compiles_and_links():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_rebuild_fast_rebuilds_the_pooled_mesh_in_place():
    exe = _build()
    out = subprocess.run(["timeout", "600", exe], capture_output=True, text=True, timeout=700)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "blas_lbvh_mirror_test OK" in out.stdout and "rebuilt: " in out.stdout, out.stdout
