"""The pure host part of the SAH builder's copy-out (voidin_amd/csrc/blas_top.hpp: top_preorder, number_top, place_nodes) on
hand-made top trees - tests/cpp/blas_top_test.cpp, a stand-alone program built by the host compiler alone, once plainly and
once with the address and undefined-behaviour sanitizers.  No GPU and no library."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "blas_top_test.cpp")
HDR = os.path.join(ROOT, "voidin_amd", "csrc", "blas_top.hpp")


def _build(exe, extra=()):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra, SRC, "-o", exe], check=True, capture_output=True, timeout=900)
    return exe


@pytest.mark.parametrize("name,flags", [("blas_top_test", ()),
                                        ("blas_top_test_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))])
def test_top_tree_numbering_and_node_placement(name, flags):
    exe = _build(os.path.join(ROOT, "tests", "cpp", name), flags)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "blas_top_test OK" in out.stdout, out.stdout + out.stderr
