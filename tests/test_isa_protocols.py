"""The fence-free hand-offs between workgroups: the TLAS refit climb, the several-workgroup TLAS chain, the
BLAS refit climb and the fit of the LBVH bottom level publish data with relaxed agent-scope atomics and order them with
`s_waitcnt vmcnt(0)` instead of release / acquire fences (an agent-scope release writes back the whole L2 of the XCD: DESIGN.md 3.4).
Under the HIP memory model that rests on what the compiler EMITS, so the emitted gfx950 code is checked here, on every build:

  * published data leaves as write-through stores (`sc1`) and is re-read L2-coherently (`sc1` loads);
  * the arrival / "readable" atomic that follows the data is preceded by `s_waitcnt vmcnt(0)`;
  * the chunk counts of `mask_scan_kernel` travel as ONE 8-byte {epoch, count} word (self-validating, race-free);
  * the kernels that hand over with fences instead (`blas_refit_kernel<true>`, `lbvh_fit_kernel`) hold an agent-scope write-back
    before the counter add and an `sc1` invalidate after it.

And an inventory: EVERY kernel of csrc/*.hip whose body holds a global atomic or an `sc1` access is either a hand-off with a
run-time test that alternates or repeats it (HANDOFFS; DESIGN.md 3.4 is the readable copy), or is excused with a reason
(NOT_A_HANDOFF).  A new climb cannot arrive without both halves.

tests/test_gpu_handoffs.py and tests/test_gpu_stress.py are the run-time half."""
import glob
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "voidin_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-S", "--cuda-device-only"]


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """name -> gfx950 assembly of csrc/<name>.hip: every source, compiled once, side by side."""
    d = tmp_path_factory.mktemp("isa")
    names = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(CSRC, "*.hip")))

    def compile_one(name):
        path = str(d / f"{name}.s")
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, os.path.join(CSRC, f"{name}.hip"), "-o", path], check=True, capture_output=True, timeout=600)
        return open(path).read()

    with ThreadPoolExecutor(max_workers=8) as pool:
        return dict(zip(names, pool.map(compile_one, names)))


def kernel_body(text, mangled_fragment):
    """Instructions of the first kernel whose symbol contains `mangled_fragment`."""
    m = re.search(r"^(_Z\w*%s\w*):\s*;.*$" % re.escape(mangled_fragment), text, re.M)
    assert m, f"kernel {mangled_fragment} not found"
    end = text.index(".Lfunc_end", m.end())         # (a kernel may hold several s_endpgm: early exits)
    return [l.strip() for l in text[m.end():end].splitlines() if l.strip() and not l.strip().startswith((";", "."))]


def test_refit_climb_publishes_write_through_and_waits_before_the_handshake(isa):
    body = kernel_body(isa["tlas"], "tlas_refit_up_kernelI10VdTlasNode")
    atomics = [i for i, l in enumerate(body) if l.startswith("global_atomic_add")]
    assert len(atomics) == 2, "announce (+1) and readable (+2)"
    stores = [i for i, l in enumerate(body) if l.startswith("global_store_dword ") and i < atomics[1]]
    assert len(stores) >= 6 and all("sc1" in body[i] for i in stores), "the box must leave as agent-scope write-through stores"
    between = body[max(stores) + 1: atomics[1]]
    assert any(l.startswith("s_waitcnt vmcnt(0)") for l in between), "the box must have reached memory before 'readable' is counted"
    loads = [l for l in body[atomics[1] + 1:] if l.startswith("global_load_dword ")][:6]
    assert len(loads) == 6 and all("sc1" in l for l in loads), "the sibling's box must be read L2-coherently"


def test_several_workgroup_chain_exchanges_tagged_words(isa):
    body = kernel_body(isa["tlas"], "tlas_build_mw_kernelI10VdTlasNode")
    assert any(l.startswith("global_store_dwordx2") and "sc1" in l for l in body), "the {area, slot, tag} key is ONE 8-byte agent-scope store"
    assert any(l.startswith("global_load_dwordx2") and "sc1" in l for l in body), "... polled by agent-scope loads"
    # the merge: slot stores (sc1), then the explicit wait, then the merge counter
    waits = [i for i, l in enumerate(body) if l.startswith("s_waitcnt vmcnt(0)")]
    sc1_stores = [i for i, l in enumerate(body) if l.startswith("global_store_dword ") and "sc1" in l]
    assert sc1_stores and any(any(s < w for s in sc1_stores) and any(s > w for s in sc1_stores) for w in waits)


def test_mask_scan_counts_are_self_validating_words(isa):
    body = kernel_body(isa["cull"], "mask_scan_kernel")
    assert any(l.startswith("global_store_dwordx2") and "sc1" in l for l in body), "{epoch, count} leaves as one 8-byte agent-scope store"
    assert any(l.startswith("global_load_dwordx2") and "sc1" in l for l in body), "... and is accepted only when its tag is this launch's epoch"
    assert not any(l.startswith("buffer_wbl2") for l in body), "no agent-scope release fence (it writes back the XCD's whole L2)"


# ---- the climbs of blas_refit.hip and blas_lbvh.hip ---------------------------------------------------------------------------------

STORE, LOAD, ATOMIC = re.compile(r"(global|flat|buffer)_store_"), re.compile(r"(global|flat|buffer)_load_"), re.compile(r"(global|flat|buffer)_atomic_")
ENDS_A_PATH = ("s_branch", "s_endpgm")


def _offset(line):
    m = re.search(r"offset:(\d+)", line)
    return int(m.group(1)) if m else 0


def climb(body):
    """The announce of a climb and what surrounds it -> (index of the counter add, indices of the stores on the straight path that
    leads to it, indices of the loads on the straight path behind it).  The announce is the first `global_atomic_add` with a store
    on its path: the MeshInfo fold that shares blas_refit_kernel counts its blocks with an add that follows atomic min / max only.
    A straight path ends at an unconditional branch or the end of the program (conditional exits leave it, nothing enters)."""
    for add in (i for i, l in enumerate(body) if l.startswith("global_atomic_add")):
        start = max((i for i in range(add) if body[i].startswith(ENDS_A_PATH)), default=-1) + 1
        stores = [i for i in range(start, add) if STORE.match(body[i])]
        if stores:
            stop = min((i for i in range(add + 1, len(body)) if body[i].startswith(ENDS_A_PATH)), default=len(body))
            return add, stores, [i for i in range(add + 1, stop) if LOAD.match(body[i])]
    raise AssertionError("no counter add with stores on its path")


def _check_publish_and_read(body, words, what):
    """`words` payload words leave as global sc1 stores, the sibling's come back as global sc1 loads of the same offsets."""
    add, stores, loads = climb(body)
    assert len(stores) == words and all(body[i].startswith("global_store_dword ") and "sc1" in body[i] for i in stores), \
        f"{what}: the published words leave as `global_store_dword ... sc1`, never flat: {[body[i] for i in stores]}"
    sc1_loads = [i for i in loads if "sc1" in body[i]]
    assert len(sc1_loads) == words and all(body[i].startswith("global_load_dword ") for i in sc1_loads), \
        f"{what}: the sibling's words are read by `global_load_dword ... sc1`: {[body[i] for i in loads]}"
    assert not any(body[i].startswith("flat_") for i in loads), f"{what}: a flat load behind the counter add"
    assert sorted(_offset(body[i]) for i in sc1_loads) == sorted(_offset(body[i]) for i in stores), f"{what}: the words read are not the words published"
    return add, stores, sc1_loads


@pytest.mark.parametrize("source,kernel,words", [("blas_refit", "blas_refit_kernelILb0", 6), ("blas_lbvh", "blas_lbvh_fit_kernel", 7),
                                                 ("blas_lbvh", "blas_lbvh_batch_fit_kernel", 7)])
def test_blas_climbs_publish_write_through_and_drain_before_the_counter(isa, source, kernel, words):
    """The leaf climb of the BLAS refit (a box: six words) and fit_body of the LBVH bottom level (a box and the count / height word:
    seven) - no fence: write-through stores, the storing wave drained, a relaxed counter add, L1-bypassing loads."""
    body = kernel_body(isa[source], kernel)
    add, stores, loads = _check_publish_and_read(body, words, kernel)
    assert any(l.startswith("s_waitcnt vmcnt(0)") for l in body[max(stores) + 1: add]), "the words must have reached memory before the counter says so"
    assert not any(l.startswith(("buffer_wbl2", "buffer_inv")) for l in body[min(stores): max(loads) + 1]), "no fence on the climb's path"
    if source == "blas_lbvh":               # nothing but the climb stores in these kernels: the first box of a leaf pair leaves the same way
        every = [l for l in body if STORE.match(l)]
        assert every and all(l.startswith("global_store_dword ") and "sc1" in l for l in every)
        assert len([l for l in body if ATOMIC.match(l)]) == 1


def test_blas_refit_with_fences_holds_a_write_back_and_an_invalidate(isa):
    """VD_OPT_BLAS_REFIT_FENCES = 1: the same stores and loads, an agent-scope release before the add, an acquire behind it."""
    body = kernel_body(isa["blas_refit"], "blas_refit_kernelILb1")
    add, stores, loads = _check_publish_and_read(body, 6, "blas_refit_kernel<true>")
    before, after = body[max(stores) + 1: add], body[add + 1: min(loads)]
    wb = [i for i, l in enumerate(before) if l.startswith("buffer_wbl2") and "sc1" in l]
    assert wb and any(l.startswith("s_waitcnt vmcnt(0)") for l in before[wb[-1] + 1:]), "write-back, completed, before the counter add"
    assert any(l.startswith("buffer_inv") and "sc1" in l for l in after), "invalidate between the counter add and the sibling's loads"


@pytest.mark.parametrize("node", ["I10VdTlasNode", "I14VdTlasNodeWide"])
def test_tlas_lbvh_fit_hands_over_with_fences(isa, node):
    """lbvh_fit_kernel: the __threadfence() form.  One loop: [write-back, wait] add [invalidate] loads of BOTH children, stores."""
    body = kernel_body(isa["tlas"], "lbvh_fit_kernel" + node)
    adds = [i for i, l in enumerate(body) if ATOMIC.match(l)]
    assert len(adds) == 1 and body[adds[0]].startswith("global_atomic_add")
    add = adds[0]
    wb = [i for i in range(add) if body[i].startswith("buffer_wbl2") and "sc1" in body[i]]
    assert wb and any(l.startswith("s_waitcnt vmcnt(0)") for l in body[wb[-1] + 1: add]), "write-back, completed, before the counter add"
    box_loads = [i for i in range(add + 1, len(body)) if body[i].startswith("global_load_dword ") and "sc1" in body[i]]
    assert len(box_loads) == 12, "both children's boxes, L1-bypassing"
    assert any(l.startswith("buffer_inv") and "sc1" in l for l in body[add + 1: box_loads[0]]), "invalidate between the add and the boxes"
    stores = [l for l in body if STORE.match(l)]
    assert stores and all(l.startswith("global_store_dword ") and "sc1" in l for l in stores), "boxes leave as global write-through stores"
    assert not any(l.startswith("flat_") for l in body)


# ---- inventory ----------------------------------------------------------------------------------------------------------------------

HANDOFFS_FILE, STRESS_FILE = "tests/test_gpu_handoffs.py", "tests/test_gpu_stress.py"
# kernel (name without template arguments) -> the run-time test that alternates its inputs (test_gpu_handoffs) or repeats it (test_gpu_stress)
HANDOFFS = {
    "tlas_refit_up_kernel": f"{HANDOFFS_FILE}::test_handoff[tlas_refit[narrow-4096]-quiet]",
    "blas_refit_kernel": f"{HANDOFFS_FILE}::test_handoff[blas_refit[three-fences0]-quiet]",
    "blas_lbvh_fit_kernel": f"{HANDOFFS_FILE}::test_handoff[blas_lbvh[soup4097]-quiet]",
    "blas_lbvh_batch_fit_kernel": f"{HANDOFFS_FILE}::test_handoff[blas_lbvh_planned[caps-3-4-300-1025-4097]-quiet]",
    "blas_lbvh_batch_bounds_kernel": f"{HANDOFFS_FILE}::test_handoff[blas_lbvh_planned[caps-3-4-300-1025-4097]-quiet]",
    "lbvh_fit_kernel": f"{HANDOFFS_FILE}::test_handoff[tlas_lbvh[narrow-4096]-quiet]",
    "a_boundary_kernel": f"{HANDOFFS_FILE}::test_handoff[bvh_build[soup9000]-quiet]",
    "a_apply_kernel": f"{HANDOFFS_FILE}::test_handoff[bvh_build[soup9000]-quiet]",
    "mask_scan_kernel": f"{STRESS_FILE}::test_split_cull_scan_hand_off_repeats",
    "tlas_build_mw_kernel": f"{STRESS_FILE}::test_several_workgroup_tlas_chain_repeats",
    "tlas_build_indexed_kernel": f"{STRESS_FILE}::test_indexed_tlas_build_repeats",
}
NEXT_LAUNCH = "Counters, keys and lists that a LATER launch reads; nothing is read back inside the launch."
TRACE = "Ray-supply counter, job list, per-ray minimum and overflow marks: drawn from or read by the next launch; tuning counters."
LOOK_BACK = "Look-back granules are self-validating 8-byte {epoch, status, value} words: the datum is its own flag, no payload behind it."
NOT_A_HANDOFF = {
    "blas_precompute_kernel": NEXT_LAUNCH, "a_eval_kernel": NEXT_LAUNCH, "a_bin_kernel": NEXT_LAUNCH, "a_child_kernel": NEXT_LAUNCH,
    "blas_mid_kernel": NEXT_LAUNCH, "c_root_kernel": NEXT_LAUNCH, "lbvh_extent_kernel": NEXT_LAUNCH, "lbvh_extent_seg_kernel": NEXT_LAUNCH,
    "blas_small_kernel": "One workgroup per subtree: its records are re-read by the same workgroup only; an error word nobody reads in the launch.",
    "blas_lbvh_boxes_kernel": "n_bad_indices: a counter nobody reads in the launch.",
    "blas_lbvh_batch_boxes_kernel": "n_bad_indices: a counter nobody reads in the launch.",
    "compact_draws_kernel": LOOK_BACK, "cull_compact_kernel": LOOK_BACK,
    "ovf_list_kernel": TRACE, "traverse_iter_kernel": TRACE, "traverse_rec_kernel": TRACE, "pair_owner_kernel": TRACE, "prepare_tris_kernel": TRACE,
    "trace_single_prep_kernel": TRACE, "trace_single_kernel": TRACE, "trace_deep_kernel": TRACE, "trace_wide_kernel": TRACE,
    "trace_deep_wide_kernel": TRACE, "tight_boxes_kernel": TRACE,
}


def kernel_names(text):
    """Kernel symbols of one assembly file -> names without namespace and template arguments."""
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        m = re.match(r"_Z(?:N12_GLOBAL__N_1)?(\d+)", sym)
        assert m, f"a kernel symbol of another shape: {sym}"
        out[sym] = sym[m.end(): m.end() + int(m.group(1))]
    return out


def kernels_that_could_hand_over(isa):
    """-> {kernel name: source} for every kernel whose body holds a global atomic or an sc1 access"""
    found = {}
    for source, text in isa.items():
        for sym, name in kernel_names(text).items():
            body = kernel_body(text, sym[2:])                 # (kernel_body puts the _Z in front itself)
            if any(ATOMIC.match(l) or ((STORE.match(l) or LOAD.match(l)) and re.search(r"\bsc1\b", l)) for l in body):
                found[name] = source
    return found


def inventory_errors(found, handoffs, excused, case_ids, case_kernels):
    """Every kernel that could hand over is in exactly one table; no table names a kernel that is gone; every test named exists
    and, in tests/test_gpu_handoffs.py, names the kernel back."""
    errors = []
    for name in sorted(found):
        if (name in handoffs) == (name in excused):
            errors.append(f"{name} ({found[name]}.hip): " + ("in both tables" if name in handoffs else "in neither HANDOFFS nor NOT_A_HANDOFF"))
    for name in sorted((set(handoffs) | set(excused)) - set(found)):
        errors.append(f"{name}: no kernel of that name holds a global atomic or an sc1 access")
    for name, reason in sorted(excused.items()):
        if not reason.strip():
            errors.append(f"{name}: no reason")
    for name, test in sorted(handoffs.items()):
        path, _, rest = test.partition("::")
        if path == HANDOFFS_FILE:
            m = re.fullmatch(r"test_handoff\[(.+)\]", rest)
            if not m or m.group(1) not in case_ids:
                errors.append(f"{name}: no case {rest}")
            elif name not in case_kernels[m.group(1)]:
                errors.append(f"{name}: the case {m.group(1)} does not name it")
        elif not os.path.exists(os.path.join(ROOT, path)) or not re.search(rf"^def {re.escape(rest)}\(", open(os.path.join(ROOT, path)).read(), flags=re.M):
            errors.append(f"{name}: the test {test} does not exist")
    return errors


def _cases():
    import test_gpu_handoffs as t
    return set(t.CASES), {cid: kernels for cid, (_, _, kernels) in t.CASES.items()}


def test_every_kernel_that_could_hand_over_is_tested_or_excused(isa):
    found = kernels_that_could_hand_over(isa)
    assert inventory_errors(found, HANDOFFS, NOT_A_HANDOFF, *_cases()) == []
    for name in ("blas_refit_kernel", "blas_lbvh_fit_kernel", "blas_lbvh_batch_fit_kernel", "lbvh_fit_kernel", "a_boundary_kernel", "a_apply_kernel"):
        assert HANDOFFS[name].startswith(HANDOFFS_FILE), f"{name}: a case that ALTERNATES its inputs"


def test_the_inventory_can_fail(isa):
    found = kernels_that_could_hand_over(isa)
    ids, kernels = _cases()
    less = dict(HANDOFFS); less.pop("blas_lbvh_fit_kernel")
    assert inventory_errors(found, less, NOT_A_HANDOFF, ids, kernels) == ["blas_lbvh_fit_kernel (blas_lbvh.hip): in neither HANDOFFS nor NOT_A_HANDOFF"]
    assert inventory_errors(dict(found, new_climb_kernel="tlas"), HANDOFFS, NOT_A_HANDOFF, ids, kernels) == ["new_climb_kernel (tlas.hip): in neither HANDOFFS nor NOT_A_HANDOFF"]
    assert "in both tables" in inventory_errors(found, HANDOFFS, dict(NOT_A_HANDOFF, lbvh_fit_kernel="x"), ids, kernels)[0]
    assert "no case" in inventory_errors(found, dict(HANDOFFS, lbvh_fit_kernel=f"{HANDOFFS_FILE}::test_handoff[tlas_lbvh[narrow-1]-quiet]"), NOT_A_HANDOFF, ids, kernels)[0]
    assert "does not name it" in inventory_errors(found, dict(HANDOFFS, lbvh_fit_kernel=HANDOFFS["blas_refit_kernel"]), NOT_A_HANDOFF, ids, kernels)[0]
    assert "does not exist" in inventory_errors(found, dict(HANDOFFS, mask_scan_kernel=f"{STRESS_FILE}::test_that_is_not_there"), NOT_A_HANDOFF, ids, kernels)[0]
    assert "no kernel of that name" in inventory_errors(found, HANDOFFS, dict(NOT_A_HANDOFF, gone_kernel=NEXT_LAUNCH), ids, kernels)[0]
    assert "no reason" in inventory_errors(found, HANDOFFS, dict(NOT_A_HANDOFF, ovf_list_kernel=" "), ids, kernels)[0]
