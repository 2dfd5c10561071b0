"""The pure host part of vd_bvh_lbvh_plan_dev (voidin_amd/csrc/blas_lbvh_plan.hpp: lbvh_judge_item, lbvh_place_item,
lbvh_plan_tables) on hand-made item lists - tests/cpp/blas_lbvh_plan_test.cpp, a stand-alone program built by the host compiler
alone, once plainly and once with the address and undefined-behaviour sanitizers.  No GPU and no library."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "blas_lbvh_plan_test.cpp")
HDRS = [os.path.join(ROOT, "voidin_amd", "csrc", h) for h in ("blas_lbvh_plan.hpp", "vd_plan.hpp")]


def _build(exe, extra=()):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC, *HDRS]):
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra, SRC, "-o", exe], check=True, capture_output=True, timeout=900)
    return exe


@pytest.mark.parametrize("name,flags", [("blas_lbvh_plan_test", ()),
                                        ("blas_lbvh_plan_test_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))])
def test_slot_layout_fold_chunks_and_refusals(name, flags):
    exe = _build(os.path.join(ROOT, "tests", "cpp", name), flags)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "blas_lbvh_plan_test OK" in out.stdout, out.stdout + out.stderr
