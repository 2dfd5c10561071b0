"""The G-buffer from primary rays (voidin_amd/csrc/gbuffer_trace.hip) is one pixel per lane from the record to the stores: nothing is
handed between lanes or launches but the rays and records themselves.  The emitted gfx950 code of its kernels is checked for what
that allows: the two kernels and no other, no atomic on memory, no private segment (the instance's matrices stay in registers), no LDS;
the resolve kernel converts the uv with the round-to-nearest-even v_cvt_f16_f32 - never the packed round-toward-zero convert, which
gives other bits - and its word pair leaves as one 8-byte store beside a 4-byte depth and a material byte; the ray kernel stores
16 bytes at a time.  (tests/test_gpu_gbuffer_trace.py is the run-time half.)"""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_isa_shadow_pass import FLAGS, kernel_bodies

CSRC = os.path.join(ROOT, "voidin_amd", "csrc")
KERNELS = ("gbuffer_rays_kernel", "gbuffer_resolve_kernel")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isa") / "gbuffer_trace.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, os.path.join(CSRC, "gbuffer_trace.hip"), "-o", path], check=True, capture_output=True, timeout=600)
    return open(path).read()


def stores(body):
    return [l for l in body if re.match(r"(global|flat|buffer|scratch)_store", l)]


def test_the_file_holds_the_two_kernels(isa):
    assert sorted(kernel_bodies(isa)) == sorted(KERNELS)


def test_no_kernel_holds_an_atomic_on_memory_or_touches_lds(isa):
    for name, body in kernel_bodies(isa).items():
        assert len(body) > 20, name
        bad = [l for l in body if l.startswith(("global_atomic", "flat_atomic", "buffer_atomic", "ds_"))]
        assert not bad, (name, bad[:4])


def test_no_kernel_has_a_private_segment(isa):
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, re.M)
    assert len(sizes) == len(KERNELS) and all(int(s) == 0 for s in sizes), sizes
    meta = re.findall(r"^\s*\.private_segment_fixed_size:\s*(\d+)", isa, re.M)
    assert len(meta) == len(KERNELS) and all(int(s) == 0 for s in meta), meta
    for name, body in kernel_bodies(isa).items():
        assert not [l for l in body if l.startswith("scratch_")], name


def test_the_resolve_kernel_converts_to_f16_with_round_to_nearest_even(isa):
    body = kernel_bodies(isa)["gbuffer_resolve_kernel"]
    assert sum(l.startswith("v_cvt_f16_f32") for l in body) >= 2, [l for l in body if "cvt" in l][:8]
    assert not [l for l in body if "cvt_pkrtz" in l]
    assert not [l for l in body if l.startswith("s_setreg")], "the rounding mode is the default one throughout"


def test_the_resolve_kernel_stores_the_word_pair_as_eight_bytes(isa):
    st = stores(kernel_bodies(isa)["gbuffer_resolve_kernel"])
    kinds = sorted({l.split()[0] for l in st})
    assert kinds == ["global_store_byte", "global_store_dword", "global_store_dwordx2"], st
    assert len(st) == 3, st                              # one of each: the miss and the hit meet before the stores


def test_the_resolve_kernel_loads_a_record_as_sixteen_bytes_and_the_mesh_words_together(isa):
    """The record is one 16-byte load; index_count and base_index are two loads with no wait between them; no load is a flat one."""
    body = kernel_bodies(isa)["gbuffer_resolve_kernel"]
    at = [i for i, l in enumerate(body) if re.match(r"(global|flat|buffer)_load", l)]
    loads = [body[i].split()[0] for i in at]
    assert loads[0] == "global_load_dwordx4" and not [l for l in loads if not l.startswith("global_load")], loads
    assert loads[1] == "global_load_dwordx2", loads                  # {mesh, material}
    assert loads[2:4] == ["global_load_dword", "global_load_dword"], loads
    assert not [l for l in body[at[2]: at[3]] if l.startswith("s_waitcnt")], body[at[2]: at[3]]


def test_the_ray_kernel_stores_sixteen_bytes_at_a_time(isa):
    st = stores(kernel_bodies(isa)["gbuffer_rays_kernel"])
    assert len(st) == 2 and all(l.startswith("global_store_dwordx4") for l in st), st
