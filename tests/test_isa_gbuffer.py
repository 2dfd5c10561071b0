"""The G-buffer front end (voidin_amd/csrc/gbuffer.hip) puts its tiles in order between launches - counts to the scan, offsets to the
writer and to the scatter - and a receiver's rank inside a tile is ballots of one wave.  The emitted gfx950 code of its kernels is
checked for what that allows: the four kernels and no other, no atomic on memory anywhere, no private segment (the per-lane arrays
stay in registers), a point's position and normal leaving the writer as 12-byte stores, and the count kernel reading bytes alone.
(tests/test_gpu_shadow_gbuffer.py is the run-time half.)"""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_isa_shadow_pass import FLAGS, kernel_bodies

CSRC = os.path.join(ROOT, "voidin_amd", "csrc")
KERNELS = ("gbuffer_count_kernel", "gbuffer_scan_kernel", "gbuffer_write_kernel", "gbuffer_scatter_kernel")


@pytest.fixture(scope="module")
def gbuffer_isa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isa") / "gbuffer.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, os.path.join(CSRC, "gbuffer.hip"), "-o", path], check=True, capture_output=True, timeout=600)
    return open(path).read()


def test_the_file_holds_the_four_kernels(gbuffer_isa):
    assert sorted(kernel_bodies(gbuffer_isa)) == sorted(KERNELS)


def test_no_kernel_holds_an_atomic_on_memory(gbuffer_isa):
    for name, body in kernel_bodies(gbuffer_isa).items():
        assert len(body) > 20, name
        bad = [l for l in body if l.startswith(("global_atomic", "flat_atomic", "buffer_atomic"))]
        assert not bad, (name, bad[:4])


def test_no_kernel_has_a_private_segment(gbuffer_isa):
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", gbuffer_isa, re.M)
    assert len(sizes) == len(KERNELS) and all(int(s) == 0 for s in sizes), sizes
    meta = re.findall(r"^\s*\.private_segment_fixed_size:\s*(\d+)", gbuffer_isa, re.M)
    assert len(meta) == len(KERNELS) and all(int(s) == 0 for s in meta), meta


def test_the_count_kernel_reads_the_material_byte_alone(gbuffer_isa):
    body = kernel_bodies(gbuffer_isa)["gbuffer_count_kernel"]
    loads = [l for l in body if re.match(r"(global|flat|buffer)_load", l)]
    assert len(loads) == 8 and all(l.startswith("global_load_ubyte") for l in loads), loads


def test_the_writer_stores_a_point_as_twelve_bytes(gbuffer_isa):
    body = kernel_bodies(gbuffer_isa)["gbuffer_write_kernel"]
    stores = [l for l in body if re.match(r"(global|flat|buffer|scratch)_store", l)]
    assert stores and all(l.startswith(("global_store_dwordx3", "global_store_dword ")) for l in stores), stores[:8]
    assert sum(l.startswith("global_store_dwordx3") for l in stores) == 2 * sum(l.startswith("global_store_dword ") for l in stores) > 0, stores[:8]
