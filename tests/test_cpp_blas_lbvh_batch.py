"""MeshPool::add_many_fast / rebuild_many_fast of the C++ mirror (include/voidin.hpp): the host compiles against the C ABI without
a GPU and, with one, compares the pool after one batched LBVH build with the pool after the same meshes one by one."""
import os
import subprocess

import pytest

from conftest import ROOT

NAME = "blas_lbvh_batch_mirror_test"


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


def test_blas_lbvh_batch_mirror_compiles_and_links():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_many_fast_equals_one_by_one():
    exe = _build()
    out = subprocess.run(["timeout", "600", exe], capture_output=True, text=True, timeout=700)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "blas_lbvh_batch_mirror_test OK" in out.stdout and "added: 5 meshes" in out.stdout and "rebuilt: 3 meshes" in out.stdout, out.stdout
