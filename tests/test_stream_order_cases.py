"""The inputs of tests/test_gpu_stream_order.py (tests/stream_order_cases.py), held to their conditions on the CPU: A and B of every
case have one shape, any mixture of their buffers is a legal input, every output buffer has teeth - expected(A) != expected(B), for a
list other counts or more than half of the records - and every function of include/voidin_abi.h is run by a case or excluded with an
admitted reason.  No GPU is needed; the expected outputs come from the oracle and the restatements the parity tests trust."""
import numpy as np
import pytest

import stream_order_cases as S
from test_write_set_harness import HEADER, declared_symbols


@pytest.fixture(scope="module")
def specs(oracle):
    def get(cid):
        return S.CASES[cid].build(oracle, "A"), S.CASES[cid].build(oracle, "B")
    return get


@pytest.mark.parametrize("cid", list(S.CASES))
def test_a_and_b_have_one_shape(specs, cid):
    a, b = specs(cid)
    assert a.shape() == b.shape()
    assert set(a.want) == set(b.want) and {k: w["kind"] for k, w in a.want.items()} == {k: w["kind"] for k, w in b.want.items()}
    assert not set(a.dev) & set(a.inout) and not (set(a.dev) | set(a.inout)) & set(a.out)
    for s in (a, b):
        for name in list(s.out) + list(s.inout):                 # every buffer the call writes is compared with something
            keys = [k for k, _, _ in S.slices(cid, name, 1 << 30)]
            assert all(k in s.want for k in keys), (name, keys)
    assert S.CASES[cid].run_fn is not None and S.CASES[cid].__doc__


def range_errors(a, b):
    """Every index-bearing field of either input lies under the bound of BOTH: the bounds - the counts the other input's arrays
    have - agree, and every value of either is below them."""
    errors = []
    if [(what, bound) for what, _, bound in a.ranges] != [(what, bound) for what, _, bound in b.ranges]:
        errors.append("A and B do not state the same fields with the same bounds")
    for tag, s in (("A", a), ("B", b)):
        for what, values, bound in s.ranges:
            values = np.asarray(values).astype(np.int64)
            if values.size and not (0 <= values.min() and values.max() < bound):
                errors.append(f"{tag}: {what}: {int(values.min())} .. {int(values.max())} is not within [0, {bound})")
    return errors


@pytest.mark.parametrize("cid", list(S.CASES))
def test_any_mixture_is_a_legal_input(specs, cid):
    """The ranges, and no NaN, no infinity in a float argument (the parity files own those)."""
    a, b = specs(cid)
    assert range_errors(a, b) == []
    for s in (a, b):
        for k, v in s.host.items():
            if isinstance(v, np.ndarray) and v.dtype.kind == "f":
                assert np.isfinite(v).all(), k


def test_the_range_check_can_fail(oracle):
    a, b = (S.CASES["mask_wire_formats"].build(oracle, w) for w in "AB")
    assert a.ranges and range_errors(a, b) == []
    what, values, bound = a.ranges[0]
    bad = values.copy(); bad[3] = bound                          # one index of A that B's arrays do not have
    worse = S.Spec(ranges=[(what, bad, bound)])
    assert range_errors(worse, b) == [f"A: {what}: {int(bad.min())} .. {bound} is not within [0, {bound})"]
    shorter = S.Spec(ranges=[(what, values, bound - 1)])         # B's arrays one element shorter than A's
    assert range_errors(a, shorter)[0] == "A and B do not state the same fields with the same bounds"


@pytest.mark.parametrize("cid", list(S.CASES))
def test_every_output_has_teeth(specs, cid):
    a, b = specs(cid)
    for name in a.want:
        if name in S.NO_TEETH:
            continue
        assert S.differs(a.want[name], b.want[name]), f"{name}: a result that is right for A would pass for B"
    same = [name for name in list(a.dev) + list(a.inout) if a.dev.get(name, a.inout.get(name)).tobytes() == b.dev.get(name, b.inout.get(name)).tobytes()]
    # the upload of B changes every buffer but the tables that A's topology shares with B: a mesh table, the indices of a refit or a walk
    assert set(same) <= {"meshes", "lmeshes", "indices", "refit_indices", "w_indices"}, same


def test_teeth_and_compare_can_fail():
    x, y = np.arange(40, dtype=np.uint32), np.arange(40, dtype=np.uint32)
    y[:10] += 1                                                  # a quarter of ten 16-byte records... of 40 4-byte ones: not enough
    assert not S.differs(S.records(x, 4), S.records(y, 4)) and S.differs(S.records(x, 4), S.records(y[:39], 4))
    y[:21] += 1
    assert S.differs(S.records(x, 4), S.records(y, 4))
    assert not S.differs(S.exact(x), S.exact(x.copy())) and S.differs(S.exact(x), S.exact(y))
    buf = np.full(200, S.FILL, np.uint8)
    buf[:160] = x.view(np.uint8)
    assert S.compare(buf, S.records(x, 4)) is None
    assert "differ" in S.compare(buf, S.records(y, 4))
    buf[180] = 0
    assert "was written" in S.compare(buf, S.records(x, 4))
    assert S.compare(buf[:160], S.exact(x)) is None and S.compare(buf, S.exact(x)) == "200 bytes, want 160"


# ---- the order of the calls inside a case ---------------------------------------------------------------------------------------

class Recorder:
    """A case's run() against no library: the names of the entry points in the order they are called."""

    def __init__(self):
        self.calls, self.state, self.laters, self.released, self.armed = [], {}, [], set(), False

    def ok(self, name, *args):
        self.calls.append(name)

    def opt(self, name, value):
        pass

    def later(self, fn):
        self.laters.append(fn)

    def put(self, name, array):
        pass

    def build_stats(self):
        return {}


class _Addresses(dict):
    def __missing__(self, name):
        return 0x1000


def call_order(c, a, b):
    """-> (the calls of the warm-up round, the calls of the real round, the calls made once the stream has drained)"""
    e = Recorder()
    c.run(e, _Addresses(), a.host)
    warm, e.calls, e.armed = e.calls, [], True
    c.run(e, _Addresses(), b.host)
    real, e.calls = e.calls, []
    for fn in e.laters:
        fn()
    return warm, real, e.calls


def reached_behind_the_delay(orders):
    """Entry points that some case calls with the delay still in front of them: a host-pointer form always (every call gets its
    own delay), a device form when every call before it in the real round only enqueues."""
    out = set()
    for cid, (_, real, _) in orders.items():
        for k, name in enumerate(real):
            if S.CASES[cid].host or all(prev in S.ENQUEUE_ONLY for prev in real[:k]):
                out.add(name)
    return out


@pytest.fixture(scope="module")
def orders(specs):
    return {cid: call_order(c, *specs(cid)) for cid, c in S.CASES.items()}


def test_every_case_calls_what_it_says_it_covers(orders):
    """A form calls nothing its case does not list, and the forms of a case together call everything it lists."""
    called = {}
    for cid, (warm, real, late) in orders.items():
        c = S.CASES[cid]
        assert set(warm) | set(real) | set(late) <= set(c.entry_points), cid
        called.setdefault(c.build_fn, set()).update(warm + real + late)
    for c in S.CASES.values():
        assert called[c.build_fn] == set(c.entry_points), c.build_fn.__name__


def test_every_entry_point_is_reached_behind_the_delay(orders):
    """A call that may wait for its stream drains the delay: what runs behind it in the same case runs as on the null stream.  Every
    covered entry point must therefore come first - behind nothing but enqueue-only calls - in the real round of some case."""
    assert sorted(set(S.COVERS) - reached_behind_the_delay(orders)) == []


def test_the_order_check_can_fail(orders):
    cut = {cid: o for cid, o in orders.items() if not cid.endswith("any first]") and cid != "trace_deep[prepared]"}
    assert "vd_trace_any_prepared_dev" in set(S.COVERS) - reached_behind_the_delay(cut)
    cut = {cid: o for cid, o in orders.items() if cid != "one_mesh_walks[recursive first]"}
    assert sorted(set(S.COVERS) - reached_behind_the_delay(cut)) == ["vd_traverse_dev"]


# ---- completeness ---------------------------------------------------------------------------------------------------------------

def completeness_errors(header, covers, excluded):
    """The form of tests/test_write_set_harness.py::completeness_errors: every exported function is run by a case or excluded with
    an admitted reason - never both, never neither."""
    declared, errors = set(declared_symbols(header)), []
    for name in sorted(declared):
        if (name in covers) == (name in excluded):
            errors.append(f"{name}: " + ("both a case and an exclusion" if name in covers else "neither a case nor an exclusion"))
    for name in sorted((set(covers) | set(excluded)) - declared):
        errors.append(f"{name}: not declared by the header")
    for name, reason in sorted(excluded.items()):
        if reason not in S.ADMISSIBLE:
            errors.append(f"{name}: inadmissible reason {reason!r}")
        elif reason == S.RANKS and not name.startswith("vd_dist_"):
            errors.append(f"{name}: not a vd_dist_* function")
        elif reason == S.REFUSED and "external_semaphore" not in name:
            errors.append(f"{name}: not an external-semaphore function")
    for name in sorted(set(S.ENQUEUE_ONLY) - set(covers)):
        errors.append(f"{name}: promised to only enqueue, run by no case")
    return errors


def test_every_exported_function_is_run_on_the_side_stream_or_excluded():
    assert completeness_errors(HEADER, S.COVERS, S.EXCLUDED) == []


def test_the_completeness_check_can_fail(tmp_path):
    covers = dict(S.COVERS); covers.pop("vd_hiz_build_dev")
    assert completeness_errors(HEADER, covers, S.EXCLUDED) == ["vd_hiz_build_dev: neither a case nor an exclusion", "vd_hiz_build_dev: promised to only enqueue, run by no case"]
    excluded = dict(S.EXCLUDED); excluded.pop("vd_version")
    assert completeness_errors(HEADER, S.COVERS, excluded) == ["vd_version: neither a case nor an exclusion"]
    grown = tmp_path / "voidin_abi.h"
    grown.write_text(open(HEADER).read().replace("const char* vd_version(void);", "const char* vd_version(void);\nint vd_new_thing_dev(VdCtx* ctx, float* d_out);"))
    assert completeness_errors(str(grown), S.COVERS, S.EXCLUDED) == ["vd_new_thing_dev: neither a case nor an exclusion"]
    assert completeness_errors(HEADER, S.COVERS, dict(S.EXCLUDED, vd_trace_dev=S.NO_DEVICE_MEMORY))[0].startswith("vd_trace_dev: both")
    assert "inadmissible" in completeness_errors(HEADER, S.COVERS, dict(S.EXCLUDED, vd_version="Too slow."))[0]
    assert "not a vd_dist_*" in completeness_errors(HEADER, S.COVERS, dict(S.EXCLUDED, vd_version=S.RANKS))[0]


def test_the_enqueue_only_table_quotes_the_header():
    """Every line the table names says that the call only enqueues, or is the convention at the top of the header."""
    lines = open(HEADER).read().split("\n")
    for name, line in S.ENQUEUE_ONLY.items():
        text = " ".join(lines[line - 1: line + 1]).lower()
        assert "enqueue" in text, (name, line, text)
