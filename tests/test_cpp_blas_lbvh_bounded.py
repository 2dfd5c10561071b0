"""VD_OPT_BLAS_LBVH_MAX_DEPTH through the C++ mirror (include/voidin.hpp): the host compiles against the C ABI without a GPU and,
with one, adds the helmet with MeshPool::add_fast under a bound of 23 and walks it with a 24-entry stack
(tests/cpp/blas_lbvh_bounded_mirror_test.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden

NAME = "blas_lbvh_bounded_mirror_test"


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


def test_blas_lbvh_bounded_mirror_compiles_and_links():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_add_fast_under_the_bound_is_walked_with_24_entries(tmp_path):
    exe = _build()
    g = golden("helmet.npz")
    v = np.ascontiguousarray(g["vertices"], dtype=np.float32).reshape(-1, 3)
    i = np.ascontiguousarray(g["indices"], dtype=np.uint32).reshape(-1)
    mesh = tmp_path / "helmet.bin"
    with open(mesh, "wb") as f:
        f.write(np.array([len(v), len(i)], dtype=np.uint32).tobytes() + v.tobytes() + i.tobytes())
    out = subprocess.run(["timeout", "600", exe, str(mesh)], capture_output=True, text=True, timeout=700)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "blas_lbvh_bounded_mirror_test OK" in out.stdout and "max_depth: 24 unbounded, 23 under the bound of 23" in out.stdout, out.stdout
