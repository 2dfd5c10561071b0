"""The shadow pass (voidin_amd/csrc/shadow.hip) hands everything over between launches: counts to the scan, offsets to the ray writer
and to the fold, the fold's words from one chunk to the next.  The emitted gfx950 code of its kernels is checked for what that
allows: no atomic on memory anywhere, no private segment (every per-lane array stays in registers), and the rays leave the writer
as 16-byte stores.  (tests/test_gpu_shadow_pass.py is the run-time half.)"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "voidin_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-S", "--cuda-device-only"]
KERNELS = ("shadow_count_kernel", "shadow_scan_kernel", "shadow_write_kernel", "shadow_fold_kernel")


@pytest.fixture(scope="module")
def shadow_isa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isa") / "shadow.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, os.path.join(CSRC, "shadow.hip"), "-o", path], check=True, capture_output=True, timeout=600)
    return open(path).read()


def kernel_bodies(text):
    """{kernel name: instructions} of every kernel of the file."""
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        m = re.match(r"_Z(?:N12_GLOBAL__N_1)?(\d+)", sym)
        assert m, f"a kernel symbol of another shape: {sym}"
        start = re.search(r"^%s:.*$" % re.escape(sym), text, re.M)
        end = text.index(".Lfunc_end", start.end())
        out[sym[m.end(): m.end() + int(m.group(1))]] = [l.strip() for l in text[start.end():end].splitlines()
                                                        if l.strip() and not l.strip().startswith((";", "."))]
    return out


def test_the_file_holds_the_four_kernels(shadow_isa):
    assert sorted(kernel_bodies(shadow_isa)) == sorted(KERNELS)


def test_no_kernel_holds_an_atomic_on_memory(shadow_isa):
    for name, body in kernel_bodies(shadow_isa).items():
        assert len(body) > 20, name
        bad = [l for l in body if l.startswith(("global_atomic", "flat_atomic", "buffer_atomic"))]
        assert not bad, (name, bad[:4])


def test_no_kernel_has_a_private_segment(shadow_isa):
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", shadow_isa, re.M)
    assert len(sizes) == len(KERNELS) and all(int(s) == 0 for s in sizes), sizes
    meta = re.findall(r"^\s*\.private_segment_fixed_size:\s*(\d+)", shadow_isa, re.M)
    assert len(meta) == len(KERNELS) and all(int(s) == 0 for s in meta), meta


def test_the_ray_writer_stores_sixteen_bytes_at_a_time(shadow_isa):
    body = kernel_bodies(shadow_isa)["shadow_write_kernel"]
    stores = [l for l in body if re.match(r"(global|flat|buffer|scratch)_store", l)]
    assert len(stores) >= 2 and all(l.startswith("global_store_dwordx4") for l in stores), stores[:6]
