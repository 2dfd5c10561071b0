"""The lighting pass (voidin_amd/csrc/lighting.hip) is one pixel per lane, and its cost follows the set bits: per 32-light word the wave
ORs its in-range words into one scalar mask and walks the mask's set bits, fetching each light record at a wave-uniform index.  The
emitted gfx950 code of its kernel is checked for what that design promises: the one kernel and no other; no atomic on memory; no
private segment and no scratch instruction; the colour leaves as exactly one 16-byte store; the rounding mode is never touched; the
OR is DPP inside the rows and v_readlane across them, never an LDS permute; the walk is a scalar loop (s_ff1 on the mask) and every
load inside it is a scalar one - the light record; the bit words of W > 2 come through LDS, which nothing else uses, and those of
W = 2 as one 8-byte load per array.  (tests/test_gpu_lighting.py is the run-time half.)"""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_isa_shadow_pass import FLAGS, kernel_bodies

CSRC = os.path.join(ROOT, "voidin_amd", "csrc")
KERNELS = ("lighting_kernel",)


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isa") / "lighting.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, os.path.join(CSRC, "lighting.hip"), "-o", path], check=True, capture_output=True, timeout=600)
    return open(path).read()


@pytest.fixture(scope="module")
def body(isa):
    return kernel_bodies(isa)["lighting_kernel"]


def walk(isa):
    """The instructions of the walk over one mask: the basic blocks of the loop whose header picks the lowest set bit with s_ff1, as the
    compiler's own block comments name them (`in Loop: Header=BBx_y`)."""
    sym = re.search(r"^\s*\.amdhsa_kernel\s+(\S+)", isa, re.M).group(1)
    text = isa[re.search(r"^%s:.*$" % re.escape(sym), isa, re.M).end():]
    lines = text[: text.index(".Lfunc_end")].splitlines()
    at = [i for i, l in enumerate(lines) if l.strip().startswith("s_ff1_i32_b32")]
    assert len(at) == 1, [lines[i] for i in at]
    header = next(m.group(1) for m in (re.match(r"\.L(BB\d+_\d+):", lines[i]) for i in range(at[0], -1, -1)) if m)
    out, inside = [], False
    for l in lines:
        m = re.match(r"(?:\.L(BB\d+_\d+):|; %bb\.\d+:)", l)
        if m:
            inside = m.group(1) == header or f"Header={header} " in l + " "
        elif inside and l.strip() and not l.strip().startswith((";", ".")):
            out.append(l.strip())
    return out


def test_the_file_holds_the_one_kernel(isa):
    assert sorted(kernel_bodies(isa)) == sorted(KERNELS)


def test_no_atomic_on_memory(body):
    assert len(body) > 100
    bad = [l for l in body if l.startswith(("global_atomic", "flat_atomic", "buffer_atomic", "ds_add", "ds_or", "ds_cmpst", "ds_wrxchg"))]
    assert not bad, bad[:4]


def test_no_private_segment_and_no_scratch_instruction(isa, body):
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, re.M)
    assert len(sizes) == len(KERNELS) and all(int(s) == 0 for s in sizes), sizes
    meta = re.findall(r"^\s*\.private_segment_fixed_size:\s*(\d+)", isa, re.M)
    assert len(meta) == len(KERNELS) and all(int(s) == 0 for s in meta), meta
    assert not [l for l in body if l.startswith("scratch_")]
    spills = re.findall(r"^\s*\.[sv]gpr_spill_count:\s*(\d+)", isa, re.M)
    assert len(spills) == 2 and all(int(s) == 0 for s in spills), spills


def test_the_colour_leaves_as_one_sixteen_byte_store(body):
    st = [l for l in body if re.match(r"(global|flat|buffer|scratch)_store", l)]
    assert len(st) == 1 and st[0].startswith("global_store_dwordx4"), st


def test_the_rounding_mode_is_the_default_one_throughout(body):
    assert not [l for l in body if l.startswith("s_setreg")]


def test_the_or_of_the_wave_is_dpp_and_readlane(body):
    dpp = [l for l in body if l.startswith("v_or_b32_dpp")]
    assert len(dpp) == 4 and sum("quad_perm" in l for l in dpp) == 2 and sum("row_half_mirror" in l for l in dpp) == 1 and sum("row_mirror" in l for l in dpp) == 1, dpp
    lanes = sorted(int(l.rsplit(",", 1)[1]) for l in body if l.startswith("v_readlane_b32"))
    assert lanes == [0, 16, 32, 48], lanes
    assert not [l for l in body if l.startswith(("ds_bpermute", "ds_permute", "ds_swizzle"))]


def test_the_walk_is_a_scalar_loop_and_its_loads_are_scalar_loads(isa, body):
    """Inside the walk: s_ff1 picks the bit, the light record (32 bytes) arrives through s_load_* alone - no vector load, no LDS read -
    and nothing is stored."""
    w = walk(isa)
    assert 40 < len(w) < len(body) // 2, len(w)
    loads = [l.split()[0] for l in w if re.match(r"(s|global|flat|buffer|scratch)_(buffer_)?load", l)]
    assert loads and all(l.startswith("s_load_dword") for l in loads), loads
    width = {"s_load_dword": 1, "s_load_dwordx2": 2, "s_load_dwordx4": 4, "s_load_dwordx8": 8}
    assert 7 <= sum(width[l] for l in loads) <= 8, loads                       # position, radius, colour (the pad word may come along)
    assert not [l for l in w if l.startswith(("ds_", "global_store", "flat_"))]
    assert [l for l in w if l.startswith("v_sqrt_f32")] and [l for l in w if l.startswith("v_div_fixup_f32")]      # the arithmetic is in there


def test_the_bit_words_come_through_lds_or_as_one_load_per_array(body):
    """W > 2: 64 consecutive words per load (global_load_dword at lane stride 4) into LDS - ds_write_b32 - and one ds_read_b32 per array and
    word in the loop over the words; W = 2: global_load_dwordx2, once per array.  No flat load anywhere."""
    assert not [l for l in body if l.startswith("flat_")]
    assert sum(l.startswith("global_load_dwordx2") for l in body) == 2
    ds = sorted({l.split()[0] for l in body if l.startswith("ds_")})
    assert ds == ["ds_read_b32", "ds_write_b32"], ds
    assert sum(l.startswith("ds_read_b32") for l in body) == 2
    assert sum(l.startswith("ds_write_b32") for l in body) == 8                # kStageSteps = 4 steps in flight, two arrays
