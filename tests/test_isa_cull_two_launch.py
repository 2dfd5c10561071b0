"""The two-launch split form of vd_cull_compact hands pass 1's per-tile survivor counts to the expansion across a kernel
boundary: plain stores on one side, plain loads on the other.  The emitted gfx950 code of every instantiation of the two
kernels is checked for what must NOT be there: no atomic, no L2 write-back fence.  (tests/test_gpu_cull_tile_counts.py is
the run-time half.)"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "voidin_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-S", "--cuda-device-only"]


@pytest.fixture(scope="module")
def cull_isa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isa") / "cull.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, os.path.join(CSRC, "cull.hip"), "-o", path], check=True, capture_output=True, timeout=600)
    return open(path).read()


def kernel_bodies(text, mangled_fragment):
    """{symbol: instructions} of every kernel whose symbol contains `mangled_fragment`."""
    out = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):\s*;.*$" % re.escape(mangled_fragment), text, re.M):
        end = text.index(".Lfunc_end", m.end())
        out[m.group(1)] = [l.strip() for l in text[m.end():end].splitlines() if l.strip() and not l.strip().startswith((";", "."))]
    return out


@pytest.mark.parametrize("fragment,at_least", [("cull_mask_tiled_kernel", 3), ("expand_mask_u8_kernel", 4), ("expand_mask_kernel", 12)])
def test_no_atomics_and_no_l2_writeback(cull_isa, fragment, at_least):
    bodies = kernel_bodies(cull_isa, fragment)
    assert len(bodies) >= at_least, sorted(bodies)
    for sym, body in bodies.items():
        assert any(l.startswith("global_store") for l in body), sym
        bad = [l for l in body if l.startswith(("global_atomic", "flat_atomic", "buffer_atomic", "buffer_wbl2"))]
        assert not bad, (sym, bad[:4])


def test_tile_counts_leave_pass_1_as_one_plain_dword_store(cull_isa):
    for sym, body in kernel_bodies(cull_isa, "cull_mask_tiled_kernel").items():
        dword = [l for l in body if l.startswith("global_store_dword ")]
        assert dword and not any("sc1" in l or "sc0" in l for l in dword), (sym, dword)
