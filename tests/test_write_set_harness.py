"""tests/write_set.py can fail - a one-byte stray store on either side of a payload, at either end of either guard, and a one-byte
change of an input are each reported with their side and offset, for a device-style fence (a CPU torch tensor) and a host fence
(numpy) - and tests/test_gpu_write_set.py states the write set of every function include/voidin_abi.h exports, or says why not.
No GPU is needed."""
import os
import re

import numpy as np
import pytest

import write_set as ws
from conftest import ROOT

DEVICES = ["cpu", "host"]


def _poke(f, raw_index, value=0x00):
    f.raw[raw_index] = value


def _fence(device, role="out", n=1000):
    if role == "out":
        return ws.Fenced("buf", device, nbytes=n, role="out", guard_byte=0xA7)
    return ws.Fenced("buf", device, data=np.arange(n, dtype=np.uint32).view(np.uint8)[:n], role=role, guard_byte=0xA7)


@pytest.mark.parametrize("device", DEVICES)
def test_layout(device):
    f = _fence(device)
    assert f.ptr % ws.ALIGN == 0 and f.front >= ws.GUARD and len(f.raw) - f.front - f.nbytes >= ws.GUARD
    assert (f.read() == ws.FILL).all() and len(f.read()) == 1000
    base = f.raw.ctypes.data if device == "host" else f.raw.data_ptr()
    assert f.ptr == base + f.front
    g = _fence(device, "in")
    assert g.read(np.uint32).tolist() == list(range(250))


@pytest.mark.parametrize("device", DEVICES)
def test_a_clean_call_passes(device):
    out, inp = _fence(device), _fence(device, "in")
    out.payload[:100] = 7                        # what a call is allowed to do
    out.check(); inp.check()
    out.check_fill(100)
    fs = ws.Fences(device)
    a, b, c = fs.inp("a", np.zeros(10, np.uint8)), fs.out("b", 33), fs.inp("c", np.ones(5, np.float32), host=True)
    assert len({a.guard_byte, b.guard_byte, c.guard_byte}) == 3 and ws.FILL not in (a.guard_byte, b.guard_byte, c.guard_byte)
    assert c.device == "host" and a.device == device
    fs.check()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("where", ["payload - 1", "payload + len", "far end of the front guard", "far end of the back guard"])
def test_one_stray_byte_is_reported_with_side_and_offset(device, where):
    f = _fence(device)
    total = len(f.raw)
    raw_index, side, offset = {"payload - 1": (f.front - 1, "front", -1),
                               "payload + len": (f.front + f.nbytes, "back", f.nbytes),
                               "far end of the front guard": (0, "front", -f.front),
                               "far end of the back guard": (total - 1, "back", total - 1 - f.front)}[where]
    _poke(f, raw_index)
    with pytest.raises(ws.WriteSetError) as err:
        f.check()
    assert (err.value.buffer, err.value.side, err.value.first, err.value.last) == ("buf", side, offset, offset)
    assert "buf" in str(err.value) and side in str(err.value) and str(offset) in str(err.value)


@pytest.mark.parametrize("device", DEVICES)
def test_first_and_last_changed_offset(device):
    f = _fence(device)
    _poke(f, f.front + f.nbytes + 3); _poke(f, f.front + f.nbytes + 40000)
    with pytest.raises(ws.WriteSetError) as err:
        f.check()
    assert (err.value.side, err.value.first, err.value.last) == ("back", f.nbytes + 3, f.nbytes + 40000)


@pytest.mark.parametrize("device", DEVICES)
def test_a_changed_input_is_reported(device):
    f = _fence(device, "in")
    f.payload[37] = 0xFF
    with pytest.raises(ws.WriteSetError) as err:
        f.check()
    assert (err.value.buffer, err.value.side, err.value.first, err.value.last) == ("buf", "payload", 37, 37)
    # bytes the header lets a call change are named by a mask; one byte outside it is still found, at its own offset
    allowed = np.zeros(1000, bool); allowed[32:44] = True
    f.check(allowed)
    f.payload[600] = 0xFF
    with pytest.raises(ws.WriteSetError) as err:
        f.check(allowed)
    assert (err.value.side, err.value.first, err.value.last) == ("payload", 600, 600)


@pytest.mark.parametrize("device", DEVICES)
def test_unpromised_bytes_of_an_output(device):
    f = _fence(device)
    f.payload[:400] = 1
    f.check_fill(400)
    assert f.fill_intact(400) and not f.fill_intact(399)
    f.payload[999] = 0
    with pytest.raises(ws.WriteSetError) as err:
        f.check_fill(400)
    assert (err.value.side, err.value.first, err.value.last) == ("payload", 999, 999)
    with pytest.raises(ws.WriteSetError):
        f.check_fill(0, 1)


# ---- completeness ---------------------------------------------------------------------------------------------------------------

HEADER = os.path.join(ROOT, "include", "voidin_abi.h")
ADMISSIBLE = ("No caller buffer is written.", "Needs several ranks.")
FENCED_ALREADY = re.compile(r"^Fenced already by `(tests/[a-z_0-9]+\.py)::([a-z_0-9]+)(\[.*\])?`\.$")


def declared_symbols(header=HEADER):
    """As tests/test_abi_symbols.py reads the header."""
    src = open(header).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vd_[a-z_0-9]+)\s*\(", src)))


def completeness_errors(header, covers, excluded):
    """Every exported function is a case or an exclusion with an admissible reason - never both, never neither."""
    declared, errors = set(declared_symbols(header)), []
    for name in sorted(declared):
        if (name in covers) == (name in excluded):
            errors.append(f"{name}: " + ("both a case and an exclusion" if name in covers else "neither a case nor an exclusion"))
    for name in sorted((set(covers) | set(excluded)) - declared):
        errors.append(f"{name}: not declared by the header")
    for name, reason in sorted(excluded.items()):
        if reason in ADMISSIBLE:
            continue
        m = FENCED_ALREADY.match(reason)
        if not m:
            errors.append(f"{name}: inadmissible reason {reason!r}")
        elif not os.path.exists(os.path.join(ROOT, m.group(1))) or not re.search(rf"^def {m.group(2)}\(", open(os.path.join(ROOT, m.group(1))).read(), flags=re.M):
            errors.append(f"{name}: the test {m.group(1)}::{m.group(2)} does not exist")
    return errors


def test_every_exported_function_states_its_write_set():
    import test_gpu_write_set as t
    assert completeness_errors(HEADER, t.COVERS, t.EXCLUDED) == []
    assert all(fn.__doc__ for fn, _ in t.CASES.values()), "every case declares its write set in its docstring"


def test_the_completeness_check_can_fail(tmp_path):
    import test_gpu_write_set as t
    covers = dict(t.COVERS); covers.pop("vd_hiz_build_dev")
    assert completeness_errors(HEADER, covers, t.EXCLUDED) == ["vd_hiz_build_dev: neither a case nor an exclusion"]
    excluded = dict(t.EXCLUDED); excluded.pop("vd_version")
    assert completeness_errors(HEADER, t.COVERS, excluded) == ["vd_version: neither a case nor an exclusion"]
    grown = tmp_path / "voidin_abi.h"
    grown.write_text(open(HEADER).read().replace("const char* vd_version(void);", "const char* vd_version(void);\nint vd_new_thing_dev(VdCtx* ctx, float* d_out);"))
    assert completeness_errors(str(grown), t.COVERS, t.EXCLUDED) == ["vd_new_thing_dev: neither a case nor an exclusion"]
    assert completeness_errors(HEADER, t.COVERS, dict(t.EXCLUDED, vd_trace_dev="No caller buffer is written."))[0].startswith("vd_trace_dev: both")
    bad = dict(t.EXCLUDED, vd_version="Too slow."); assert "inadmissible" in completeness_errors(HEADER, t.COVERS, bad)[0]
    gone = dict(t.EXCLUDED, vd_version="Fenced already by `tests/test_gpu_cull.py::test_that_is_not_there`.")
    assert "does not exist" in completeness_errors(HEADER, t.COVERS, gone)[0]
