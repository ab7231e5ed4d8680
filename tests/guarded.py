"""Guarded buffers: one allocation per buffer, laid out [front guard | payload | back guard], so that a test sees WHERE an
entry point read and wrote and not only what it computed.

  * Both guards are mapped memory of the same allocation (never the edge of one): an overrun lands in a guard and is found
    by comparing bits afterwards, never by a fault.
  * Each guard is at least 2 MiB and at least 320 rows x K x 4 bytes (the widest macro-tile edge of any engine times a
    row of the operand), so that a whole mis-addressed tile still lands inside it.
  * The payload starts `offset` bytes after a 512-byte boundary, `offset` being the weakest alignment the interface
    accepts for that argument (include/bsmr_hip.h "Alignment"): OPERAND = 16 for A, B, X, Y, dA, dB, A16, B16 and
    VALUES = 4 for P, v, dP, the softmax arrays and both arrays of bsmr_batched_transpose.  torch hands out 512-byte
    aligned memory, which hides every assumption beyond that.
  * Guards, and the payload of an output, hold FILL: a NaN with a recognisable payload, compared as int32.  A guard value
    that is read into a stored result turns it into NaN; a write shows as changed bits; an output element that was never
    written still holds FILL.

check() asserts that both guards are bit-identical to FILL, that an input's payload is bit-identical to what was uploaded
and that no word of an output's payload still holds FILL; a failure names the side, the first and last changed byte
offset relative to the payload and the number of changed words.  Works on CPU tensors too (tests/test_guarded_host.py
plants the violations there)."""
import numpy as np
import torch

FILL = 0x7FC0DEAD            # a quiet NaN as fp32, (NaN, 0xDEAD) as two 16-bit halves; positive as int32
BOUNDARY = 512               # what torch's allocator aligns to
OPERAND, VALUES = 16, 4      # the offsets: weakest alignment accepted for operand matrices / value arrays
MIN_GUARD = 2 << 20
TILE_ROWS = 320              # widest macro-tile edge of any engine (GEMM engine: 16 panels / 20 column blocks)


def guard_bytes(K):
    """bytes of each guard for a call with inner dimension K, a whole number of BOUNDARY"""
    need = max(MIN_GUARD, TILE_ROWS * int(K) * 4)
    return -(-need // BOUNDARY) * BOUNDARY


class GuardError(AssertionError):
    pass


class Guarded:
    """kind: "input" (payload must stay as uploaded), "output" (payload prefilled with FILL, every word must be
    overwritten) or "inplace" (an input the call may overwrite: only the guards are checked)."""

    def __init__(self, name, kind, dtype, count, offset, K, device, data=None):
        assert kind in ("input", "output", "inplace") and offset % 4 == 0 and 0 < offset < BOUNDARY
        self.name, self.kind, self.offset = name, kind, offset
        self.dtype = np.dtype(dtype)
        self.count = int(count)
        self.nbytes = self.count * self.dtype.itemsize
        assert self.nbytes % 4 == 0, "payloads are whole 32-bit words"
        self.guard = guard_bytes(K)
        words = (2 * self.guard + self.nbytes + 2 * BOUNDARY) // 4
        self.raw = torch.empty(words, dtype=torch.int32, device=device)
        self.raw.fill_(FILL)
        base = self.raw.data_ptr()
        assert base % 4 == 0
        # first address >= base + guard that lies `offset` past a boundary
        start = base + self.guard
        start += (offset - start) % BOUNDARY
        self.first = (start - base) // 4                 # payload = raw[first : last]
        self.last = self.first + self.nbytes // 4
        self.ptr = start
        assert self.ptr % BOUNDARY == offset, (self.ptr, offset)
        assert self.first * 4 >= self.guard and (words - self.last) * 4 >= self.guard
        self.expect = None
        if kind != "output":
            a = np.ascontiguousarray(data, dtype=self.dtype).ravel()
            assert a.size == self.count, (name, a.size, self.count)
            if self.count:
                self.payload().copy_(torch.from_numpy(a.view(np.int32)).to(device))
            if kind == "input":
                self.expect = self.payload().clone()

    # ---- construction ----
    @classmethod
    def input(cls, name, data, offset, K, device, dtype=np.float32):
        data = np.asarray(data)
        return cls(name, "input", dtype, data.size, offset, K, device, data)

    @classmethod
    def inplace(cls, name, data, offset, K, device):
        data = np.asarray(data)
        return cls(name, "inplace", np.float32, data.size, offset, K, device, data)

    @classmethod
    def output(cls, name, count, offset, K, device, dtype=np.float32):
        return cls(name, "output", dtype, count, offset, K, device)

    # ---- access ----
    def payload(self):
        """the payload as an int32 view of the allocation"""
        return self.raw[self.first:self.last]

    def front(self):
        return self.raw[:self.first]

    def back(self):
        return self.raw[self.last:]

    def numpy(self):
        return self.payload().cpu().numpy().view(self.dtype)

    def freeze(self):
        """an output that was written becomes an input of the next call: its present bits must stay"""
        self.kind = "input"
        self.expect = self.payload().clone()

    # ---- the check ----
    def _changed(self, where):
        """(words, first byte, last byte) of the True elements of the int32-wise mask `where`, offsets within it"""
        idx = torch.nonzero(where).flatten()
        return int(idx.numel()), int(idx[0]) * 4, int(idx[-1]) * 4 + 3

    def check(self):
        front, back, pay = self.front() != FILL, self.back() != FILL, self.payload()
        flags = [front.any(), back.any()]
        if self.kind == "input":
            flags.append((pay != self.expect).any())
        elif self.kind == "output":
            flags.append((pay == FILL).any())
        bad = torch.stack(flags).cpu().tolist()         # one synchronisation for the common (clean) case
        if not any(bad):
            return
        msgs = []
        if bad[0]:
            n, lo, hi = self._changed(front)
            shift = self.first * 4
            msgs.append(f"front guard changed: {n} words, bytes [{lo - shift}, {hi - shift}] relative to the payload")
        if bad[1]:
            n, lo, hi = self._changed(back)
            msgs.append(f"back guard changed: {n} words, bytes [{lo + self.nbytes}, {hi + self.nbytes}] relative to the "
                        f"payload")
        if len(bad) > 2 and bad[2]:
            if self.kind == "input":
                n, lo, hi = self._changed(pay != self.expect)
                msgs.append(f"input payload modified: {n} words, bytes [{lo}, {hi}]")
            else:
                n, lo, hi = self._changed(pay == FILL)
                msgs.append(f"output payload not written: {n} words, bytes [{lo}, {hi}]")
        raise GuardError(f"{self.name} ({self.kind}, {self.nbytes} bytes at {self.offset} past a {BOUNDARY}-byte "
                         f"boundary): " + "; ".join(msgs))


def check_all(*buffers):
    for b in buffers:
        if b is not None:
            b.check()
