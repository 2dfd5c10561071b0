"""lighting, shade_gbuffer and TraceScene::shade_gbuffer of the C++ mirror (include/voidin.hpp, include/voidin_lighting.h): the host
compiles against the C ABI without a GPU and, with one, gets from one call the bytes of shadow_gbuffer + lighting over a traced
G-buffer (tests/cpp/lighting_mirror_test.cpp)."""
import os
import subprocess

import pytest

from conftest import ROOT
from voidin_amd import abi

NAME = "lighting_mirror_test"


def build_mirror(directory):
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    exe = os.path.join(directory, NAME)
    lib_dir = os.path.join(ROOT, "voidin_amd", "csrc")
    abi.load()
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), src,
                        "-L", lib_dir, "-lvoidin_hip", f"-Wl,-rpath,{lib_dir}", "-o", exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_lighting_mirror_compiles_and_links(tmp_path):
    assert os.path.exists(build_mirror(str(tmp_path)))


@pytest.mark.gpu
def test_lighting_mirror_gives_the_bytes_of_the_two_calls(tmp_path):
    exe = build_mirror(str(tmp_path))
    r = subprocess.run(["timeout", "300", exe], capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and NAME + " OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
