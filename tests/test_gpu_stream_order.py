"""Stream order ("Stream order"): everything an entry point does runs on the context's stream, every blocking copy has a
wait for that stream in front of it, and the builder's second stream is joined by events.  On torch's current stream - the HIP null
stream, where almost every other GPU test runs - none of that can fail: the null stream orders a launch on the wrong stream, and a
blocking copy without a wait, for free.  Here every entry point runs through a context bound to a SIDE stream S, behind a delay:

  a.  the buffers hold input A, the outputs the fill byte; one warm-up call (scratch, plans, prepared scenes) is checked against
      expected(A), then the outputs are refilled and the device is idle;
  b.  on S: a delay of K_DELAY device-to-device copies, a clone of every output (`before`), the upload of input B;
  c.  the entry point, through the context of S, with B's host arguments;
  d.  where the header promises that the call only enqueues (stream_order_cases.ENQUEUE_ONLY): S is still busy when it returns;
  e.  on S a clone of every output (`after`); then `before` holds the fill - nothing ran ahead of its place - and `after` holds
      expected(B), which differs from expected(A) in every buffer (tests/test_stream_order_cases.py).

Whatever runs out of order sees A, or writes before the delay has ended.  A call that may wait for its stream drains the delay, so
what a case calls behind it runs as it would on the null stream: every entry point is therefore the first such call of some case
(tests/test_stream_order_cases.py holds that), the plan and accel releases are called right behind an enqueue-only call and must
return with the stream drained, and every host-pointer call gets a delay of its own.  ONE table-driven test over tests/stream_order_cases.py; a
probe shows first that the null stream really overtakes S on this machine, and a control shows a stale mask for a call that is made
on the null stream on purpose.  The delay is torch copies only: finite by construction, nothing waits on a word.

Sensitivity, recorded in profiles/stream_order.md: with cull_mask_kernel launched on stream 0 the case cull_mask, and no other, turns
red at step e."""
import time

import numpy as np
import pytest

import stream_order_cases as S
from voidin_amd import abi
from write_set import FILL

pytestmark = pytest.mark.gpu

K_DELAY = 400                 # each copy moves 2 x 256 MiB through HBM: at least 64 us at the part's 8 TB/s, so at least 25 ms in all
DELAY_BYTES = 256 << 20
CANDIDATES = 4                # side streams the probe may try
CHECKED, RAN = set(), set()   # enqueue-only promises held so far; cases run so far


class Side:
    """The side stream, its context, the delay and what the probe found."""

    def __init__(self):
        import torch
        from voidin_amd.runtime import Context
        self.torch = torch
        self.a = torch.empty(DELAY_BYTES, dtype=torch.uint8, device="cuda")
        self.b = torch.empty(DELAY_BYTES, dtype=torch.uint8, device="cuda")
        self.a.zero_(); self.b.zero_()
        torch.cuda.synchronize()
        self.stream, self.candidate, self.probes = None, None, []
        # torch's pool streams are made with hipStreamNonBlocking: no implicit ordering with the null stream.  The probe shows it.
        for k in range(CANDIDATES):
            s = torch.cuda.Stream()
            ok, why = self.probe(s)
            self.probes.append((k, ok, why))
            if ok:
                self.stream, self.candidate = s, k
                break
        if self.stream is None:
            pytest.fail(f"no teeth: every side stream is serialised with the null stream ({self.probes})", pytrace=False)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            start.record(); self.delay(self.stream); end.record()
        self.stream.synchronize()
        self.delay_ms = start.elapsed_time(end)
        self.ctx = Context(0, use_torch_stream=False)
        self.ctx.set_stream(self.stream.cuda_stream)
        print(f"\nstream order: side stream candidate {self.candidate}, probes {self.probes}, delay of {K_DELAY} copies measured {self.delay_ms:.1f} ms")

    def delay(self, stream):
        with self.torch.cuda.stream(stream):
            for _ in range(K_DELAY):
                self.b.copy_(self.a, non_blocking=True)

    def probe(self, s):
        """Work on the null stream overtakes work on `s`: -> (True, "") or (False, why)."""
        torch = self.torch
        bufs = [torch.full((1 << 20,), 0xA1, dtype=torch.uint8, device="cuda") for _ in range(3)]
        src = torch.full((1 << 20,), 0xB2, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.delay(s)
        with torch.cuda.stream(s):
            for t in bufs:
                t.copy_(src, non_blocking=True)
        null = torch.cuda.current_stream()
        clones = [t.clone() for t in bufs]                   # on the null stream
        null.synchronize()                                   # the null stream alone
        busy = not s.query()
        stale = all(bool((c == 0xA1).all().item()) for c in clones)
        s.synchronize()
        fresh = all(bool((t == 0xB2).all().item()) for t in bufs)
        assert fresh, "the probe's own upload did not arrive"
        if not busy:
            return False, "the side stream was idle once the null stream had been waited for"
        return (True, "") if stale else (False, "the null stream's clone saw the side stream's upload")

    def close(self):
        self.stream.synchronize()
        self.ctx.close()


@pytest.fixture(scope="module")
def side():
    s = Side()
    t0 = time.perf_counter()
    yield s
    s.close()
    print(f"\nstream order: {len(RAN)} cases in {time.perf_counter() - t0:.1f} s after setup; enqueue-only promises held: {len(CHECKED)} of {len(S.ENQUEUE_ONLY)}")


class Env:
    """What a case's run() sees (tests/stream_order_cases.py)."""

    def __init__(self, side, host=False):
        self.side, self.ctx, self.lib, self.h, self.host = side, side.ctx, side.ctx.lib, side.ctx.h, host
        self.state, self.laters, self.puts, self.options, self.released = {}, [], {}, [], set()
        self.armed = self.blocked = False

    def ok(self, name, *args):
        if self.armed and self.host:             # a host-pointer form ends with a wait for its stream: each call gets a delay of its own
            self.side.torch.cuda.synchronize()
            self.side.delay(self.side.stream)
            assert not self.side.stream.query(), f"{name}: the delay had ended before the call was made (measured {self.side.delay_ms:.1f} ms)"
        rc = getattr(self.lib, name)(self.h, *args)
        if rc == abi.VD_ERR_HIP:                 # the device may have faulted: start nothing more on it
            pytest.exit(f"{name}: VD_ERR_HIP: {self.lib.vd_last_error(self.h)}", returncode=3)
        assert rc == abi.VD_OK, (name, abi.STATUS_NAMES.get(rc, rc), self.lib.vd_last_error(self.h))
        if self.armed and not self.blocked and name in S.RELEASE_SYNCS:
            assert self.side.stream.query(), (f"{name} (include/voidin_abi.h:{S.RELEASE_SYNCS[name]} says it synchronises the stream first) returned while the "
                                              f"call queued in front of it was still behind the delay (measured {self.side.delay_ms:.1f} ms)")
        if not self.armed or self.blocked:
            return
        if name not in S.ENQUEUE_ONLY:
            self.blocked = True                  # a call that may wait for its stream: the delay can be over from here on
            return
        assert not self.side.stream.query(), (
            f"{name} (include/voidin_abi.h:{S.ENQUEUE_ONLY[name]} says it only enqueues): the side stream was idle when the call returned - "
            f"the call waited, or the delay was too short (measured {self.side.delay_ms:.1f} ms)")
        CHECKED.add(name)

    def opt(self, name, value):
        self.ctx.set_option(name, value)
        self.options.append(name)

    def later(self, fn):
        self.laters.append(fn)

    def put(self, name, array):
        self.puts[name] = array if isinstance(array, dict) else np.ascontiguousarray(array)

    def build_stats(self):
        return self.ctx.bvh_last_build_stats()

    def finish(self):
        self.side.stream.synchronize()
        self.armed = False
        for fn in self.laters:
            fn()
        for name in self.options:
            self.ctx.set_option(name, None)


def _check(cid, read, puts, want, oracle, what, delay_ms):
    """Every expectation of `want` against the bytes read(name) of its buffer, or what the call handed back through a host pointer."""
    for name, nbytes in read.sizes.items():
        cuts = [c for c in S.slices(cid, name, nbytes) if c[0] in want]
        if not cuts:
            continue                             # an input the call may not write: tests/test_gpu_write_set.py holds that
        data = read(name)
        for key, lo, hi in cuts:
            bad = S.compare(data[lo:hi], want[key], oracle)
            assert bad is None, f"{what}: {key}: {bad} (delay measured {delay_ms:.1f} ms)"
    for key, w in want.items():
        if key.startswith("host:"):
            assert key in puts, f"{what}: {key} was not handed back"
            bad = S.compare(puts[key], w, oracle)
            assert bad is None, f"{what}: {key}: {bad} (delay measured {delay_ms:.1f} ms)"


class Reader:
    def __init__(self, tensors, sizes):
        self.tensors, self.sizes = tensors, sizes

    def __call__(self, name):
        t = self.tensors[name]
        return (t if isinstance(t, np.ndarray) else t.cpu().numpy())[: self.sizes[name]]


def _second_stream_rule(cid, puts):
    """sah_batch_second_stream: the build listed at least kMidEarlyMin mid-tier roots and ran more than one level, which is when
    launch_mid_early (blas.hip) starts them on the context's second stream."""
    if "stats" in puts:
        st = puts["stats"]
        assert st["n_mid_roots"] >= S.N_MID and st["levels_phase_a"] >= 2, f"{cid}: the build did not reach the second stream: {st}"


def run_device_case(side, oracle, cid):
    import torch
    c = S.CASES[cid]
    A, B = c.build(oracle, "A"), c.build(oracle, "B")
    Sx, ms = side.stream, side.delay_ms
    inputs = {**A.dev, **A.inout}
    sizes = {**{k: len(v) for k, v in inputs.items()}, **A.out}
    written = list(A.out) + list(A.inout)
    buf = {k: torch.empty(max(n, 16), dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
    d_A = {k: torch.from_numpy(v).cuda() for k, v in inputs.items()}
    d_B = {k: torch.from_numpy(v).cuda() for k, v in {**B.dev, **B.inout}.items()}
    ptr = {k: t.data_ptr() for k, t in buf.items()}

    def refill():
        for k in A.out:
            buf[k].fill_(FILL)
        for k, t in d_A.items():
            buf[k][: len(t)].copy_(t)
        torch.cuda.synchronize()

    e = Env(side)
    try:
        for name, value in c.options.items():
            e.opt(name, value)
        # a. the warm-up call, on A
        refill()
        c.run(e, ptr, A.host)
        Sx.synchronize()
        _check(cid, Reader(buf, sizes), e.puts, A.want, oracle, "warm-up call on A", ms)
        _second_stream_rule(cid, e.puts)
        e.puts.clear()
        refill()
        # b. the delay, `before`, the upload of B - all on S
        side.delay(Sx)
        with torch.cuda.stream(Sx):
            before = {k: buf[k].clone() for k in written}
            for k, t in d_B.items():
                buf[k][: len(t)].copy_(t, non_blocking=True)
        # c. + d. the call, with B's host arguments
        e.armed = True
        c.run(e, ptr, B.host)
        e.armed = False
        # e.
        with torch.cuda.stream(Sx):
            after = {k: buf[k].clone() for k in written}
        Sx.synchronize()
        for k in A.out:
            stray = torch.nonzero(before[k][: sizes[k]] != FILL).reshape(-1)
            assert stray.numel() == 0, (f"before holds results: {k}, {stray.numel()} bytes from byte {int(stray[0])} on were written ahead of the call's place "
                                        f"in the stream (delay measured {ms:.1f} ms)")
        for k in A.inout:
            assert torch.equal(before[k][: sizes[k]], d_A[k]), f"before holds results: {k} changed ahead of the call's place in the stream (delay measured {ms:.1f} ms)"
        _check(cid, Reader(after, sizes), e.puts, B.want, oracle, "after != expected(B)", ms)
        _second_stream_rule(cid, e.puts)
    finally:
        e.finish()


def run_host_case(side, oracle, cid):
    """Host-pointer forms: a warm-up round on A's arrays leaves A's results in the context's staging buffers; then every call is made
    with B's arrays behind a delay of its own on S (Env.ok) - an upload, a fetch or a blocking copy that does not wait for the stream
    runs ahead of the delay and brings back stale bytes."""
    c = S.CASES[cid]
    A, B = c.build(oracle, "A"), c.build(oracle, "B")
    sizes = {**{k: len(v) for k, v in {**A.dev, **A.inout}.items()}, **A.out}
    buf = {k: np.empty(max(n, 16), dtype=np.uint8) for k, n in sizes.items()}
    ptr = {k: t.ctypes.data for k, t in buf.items()}

    def fill(X):
        for k in A.out:
            buf[k][:] = FILL
        for k, v in {**X.dev, **X.inout}.items():
            buf[k][: len(v)] = v

    e = Env(side, host=True)
    try:
        fill(A)
        c.run(e, ptr, A.host)
        _check(cid, Reader(buf, sizes), e.puts, A.want, oracle, "warm-up call on A", side.delay_ms)
        e.puts.clear()
        fill(B)
        e.armed = True
        c.run(e, ptr, B.host)
        _check(cid, Reader(buf, sizes), e.puts, B.want, oracle, "after != expected(B)", side.delay_ms)
    finally:
        e.finish()


@pytest.mark.parametrize("cid", list(S.CASES))
def test_stream_order(side, oracle, cid):
    (run_host_case if S.CASES[cid].host else run_device_case)(side, oracle, cid)
    RAN.add(cid)


def test_control_a_call_on_the_null_stream_sees_the_stale_input(side, ctx, oracle):
    """The one place that asserts a STALE result: step b, then vd_cull_mask_dev through the session's ordinary context - the null
    stream - with A's camera, and a wait for the null stream alone.  The mask is expected(A): the launch overtook the delay and the
    upload of B behind it, as a library launch on the wrong stream would.  (Legal: any mixture of A and B is a valid input.)"""
    import torch
    c = S.CASES["cull_mask"]
    A, B = c.build(oracle, "A"), c.build(oracle, "B")
    d = {k: torch.from_numpy(v).cuda() for k, v in A.dev.items()}
    d_B = {k: torch.from_numpy(v).cuda() for k, v in B.dev.items()}
    mask = torch.full((A.out["mask"],), FILL, dtype=torch.uint8, device="cuda")
    cam = A.host["cam"].view(abi.CAMERA)

    def call():
        ctx.cull_mask_dev(cam, d["meshes"], A.host["n_mesh"], d["instances"], S.N_CULL, mask)

    null = torch.cuda.current_stream()
    call()                                                       # warmed up
    null.synchronize()
    assert S.compare(mask.cpu().numpy(), A.want["mask"]) is None
    mask.fill_(FILL)
    torch.cuda.synchronize()
    side.delay(side.stream)
    with torch.cuda.stream(side.stream):
        for k, t in d_B.items():
            d[k].copy_(t, non_blocking=True)
    call()
    null.synchronize()                                           # the null stream alone
    busy = not side.stream.query()
    got = mask.cpu().numpy()
    side.stream.synchronize()
    assert busy, f"the delay had ended before the null stream was idle (measured {side.delay_ms:.1f} ms)"
    assert S.compare(got, A.want["mask"]) is None, "a launch on the null stream did not overtake the side stream: the method has no teeth"
    assert S.compare(got, B.want["mask"]) is not None
    assert all(torch.equal(d[k], d_B[k]) for k in d)


def test_every_enqueue_only_promise_was_held(side):
    """Every entry point of ENQUEUE_ONLY returned while the delay was still running, in at least one case (only meaningful when
    the whole table ran)."""
    if len(RAN) == len(S.CASES):
        assert sorted(set(S.ENQUEUE_ONLY) - CHECKED) == []
