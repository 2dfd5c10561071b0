"""Write-set harness of tests/test_gpu_write_set.py (a helper module, no tests in it; its own proof is
tests/test_write_set_harness.py, which runs without a GPU).

`Fenced` is ONE allocation laid out [front guard | payload | back guard]: a torch.uint8 tensor on a torch device ("cuda",
or "cpu" for the self-test), a numpy array for device="host" (the host-pointer entry points).  Both guards are at least
GUARD = 64 KiB - more than any unit a workgroup stores in one step (the largest: a 1024-command tile of 20 B) - and the payload
starts ALIGN = 256 bytes aligned.  Every buffer of a case gets its own guard byte, an output payload is pre-filled with FILL, an
input payload is snapshotted on its own device before the call.

check() compares guards, fills and snapshots where the buffer lives (nothing but a verdict and two offsets is copied back) and
raises WriteSetError naming the buffer, the side ("front", "payload", "back") and the first and last offset that changed.
Offsets are relative to the payload: -1 is the last byte of the front guard, nbytes the first byte of the back guard.
Guards see stray STORES only."""
import numpy as np

GUARD = 64 * 1024
ALIGN = 256
FILL = 0xEE                                   # an output payload before the call
_GUARD_BYTES = [b for b in range(0x91, 0xEE) if b not in (FILL, 0xAB, 0xC3, 0xCD)]


class WriteSetError(AssertionError):
    def __init__(self, buffer, side, first, last, what):
        super().__init__(f"{buffer}: {what}: {side}, offsets {first} .. {last} (relative to the payload)")
        self.buffer, self.side, self.first, self.last = buffer, side, first, last


def _changed(region, want):
    """(first, last) index where region != want (a byte value or a same-sized region), None when equal.  Runs where the data is."""
    if isinstance(region, np.ndarray):
        bad = np.flatnonzero(region != want)
        return (int(bad[0]), int(bad[-1])) if bad.size else None
    import torch
    ne = region != want
    if not bool(ne.any().item()):
        return None
    bad = torch.nonzero(ne).reshape(-1)
    return int(bad[0].item()), int(bad[-1].item())


class Fenced:
    """role "in": payload = data, must come back byte-equal (but for `allowed`); role "out": payload = FILL; role "inout": payload =
    data, no snapshot check (the case compares it with its reference)."""

    def __init__(self, name, device, nbytes=None, data=None, role="out", guard_byte=0xA7):
        assert role in ("in", "out", "inout") and guard_byte != FILL
        if data is not None:
            data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            nbytes = len(data)
        self.name, self.device, self.role, self.guard_byte, self.nbytes = name, device, role, guard_byte, int(nbytes)
        total = GUARD + self.nbytes + GUARD + ALIGN
        if device == "host":
            self.raw = np.full(total, guard_byte, dtype=np.uint8)
            base = self.raw.ctypes.data
        else:
            import torch
            self.raw = torch.full((total,), guard_byte, dtype=torch.uint8, device=device)
            base = self.raw.data_ptr()
        self.front = GUARD + (-(base + GUARD)) % ALIGN
        self.ptr = base + self.front
        assert self.ptr % ALIGN == 0 and self.front >= GUARD and total - self.front - self.nbytes >= GUARD
        self.payload = self.raw[self.front: self.front + self.nbytes]
        if data is None:
            self.payload[:] = FILL
        elif device == "host":
            self.payload[:] = data
        else:
            import torch
            self.payload.copy_(torch.from_numpy(data.copy()))
        self.snapshot = None
        if role == "in":
            self.snapshot = self.payload.copy() if device == "host" else self.payload.clone()

    def read(self, dtype=np.uint8, count=None):
        """The payload (its first `count` items) as a numpy array of `dtype`, copied to the host."""
        p = self.payload if self.device == "host" else self.payload.cpu().numpy()
        a = np.array(p, copy=True).view(dtype)
        return a if count is None else a[:count]

    def check_guards(self):
        bad = _changed(self.raw[: self.front], self.guard_byte)
        if bad:
            raise WriteSetError(self.name, "front", bad[0] - self.front, bad[1] - self.front, "bytes in front of the buffer were written")
        bad = _changed(self.raw[self.front + self.nbytes:], self.guard_byte)
        if bad:
            raise WriteSetError(self.name, "back", self.nbytes + bad[0], self.nbytes + bad[1], "bytes behind the buffer were written")

    def check_unchanged(self, allowed=None):
        """An input: every byte equals the snapshot; `allowed` (bool per payload byte) names the bytes the header lets a call change."""
        assert self.snapshot is not None, f"{self.name} is not an input"
        now, was = self.payload, self.snapshot
        if allowed is not None:
            keep = ~np.asarray(allowed, dtype=bool)
            assert keep.shape == (self.nbytes,)
            if self.device == "host":
                idx = np.flatnonzero(keep)
                bad = _changed(now[idx], was[idx])
            else:
                import torch
                idx = torch.from_numpy(np.flatnonzero(keep)).to(self.payload.device)
                bad = _changed(now[idx], was[idx])
            if bad:
                bad = (int(idx[bad[0]]), int(idx[bad[1]]))
        else:
            bad = _changed(now, was)
        if bad:
            raise WriteSetError(self.name, "payload", bad[0], bad[1], "an input was changed")

    def fill_intact(self, lo, hi=None):
        """True when payload[lo:hi) still holds FILL (for the "report whether" items)."""
        return _changed(self.payload[lo: self.nbytes if hi is None else hi], FILL) is None

    def check_fill(self, lo, hi=None):
        """An output: payload[lo:hi) is outside the declared write set and must still hold FILL."""
        hi = self.nbytes if hi is None else hi
        bad = _changed(self.payload[lo:hi], FILL)
        if bad:
            raise WriteSetError(self.name, "payload", lo + bad[0], lo + bad[1], f"bytes of [{lo}, {hi}) that the call may not write were written")

    def check(self, allowed=None):
        self.check_guards()
        if self.role == "in":
            self.check_unchanged(allowed)


class Fences:
    """The buffers of one case: hands every one its own guard byte; check() = all guards + all inputs."""

    def __init__(self, device="cuda"):
        self.device, self.all = device, []

    def _new(self, name, device, **kw):
        f = Fenced(name, device, guard_byte=_GUARD_BYTES[len(self.all) % len(_GUARD_BYTES)], **kw)
        self.all.append(f)
        return f

    def inp(self, name, data, host=False):
        return self._new(name, "host" if host else self.device, data=data, role="in")

    def out(self, name, nbytes, host=False):
        return self._new(name, "host" if host else self.device, nbytes=nbytes, role="out")

    def inout(self, name, data, host=False):
        return self._new(name, "host" if host else self.device, data=data, role="inout")

    def check(self, allowed=None):
        """allowed: {buffer name: bool mask} for the inputs a call may change in part."""
        allowed = allowed or {}
        for f in self.all:
            f.check(allowed.get(f.name))
