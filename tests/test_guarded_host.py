"""tests/guarded.py on CPU tensors: the layout and alignment arithmetic, and the proof that the harness bites - every
violation a wrong kernel could commit is planted here with plain torch indexing and must be reported with its side and
byte offsets.  No kernel is modified and none runs."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import guarded                                            # noqa: E402
from guarded import FILL, GuardError, Guarded             # noqa: E402

CPU = torch.device("cpu")


def _input(n=1000, offset=guarded.OPERAND, K=64):
    data = np.arange(n, dtype=np.float32) - 7
    return Guarded.input("A", data, offset, K, CPU), data


def _fails(buf):
    with pytest.raises(GuardError) as e:
        buf.check()
    return str(e.value)


def _span(msg, what):
    m = re.search(re.escape(what) + r": (\d+) words, bytes \[(-?\d+), (-?\d+)\]", msg)
    assert m, (what, msg)
    return tuple(int(g) for g in m.groups())


def test_guard_size_is_a_condition():
    assert guarded.guard_bytes(32) == 2 << 20 and guarded.guard_bytes(1024) == 2 << 20
    assert guarded.guard_bytes(4096) == 320 * 4096 * 4            # a macro-tile edge of rows outgrows 2 MiB
    for K in (32, 100, 1639, 5000):
        g = guarded.guard_bytes(K)
        assert g >= 2 << 20 and g >= 320 * K * 4 and g % guarded.BOUNDARY == 0


@pytest.mark.parametrize("offset", [guarded.VALUES, guarded.OPERAND])
@pytest.mark.parametrize("dtype,count", [(np.float32, 1), (np.float32, 999), (np.uint16, 64), (np.float32, 330 * 64)])
def test_layout_and_alignment(offset, dtype, count):
    for buf in (Guarded.output("P", count, offset, 128, CPU, dtype=dtype),
                Guarded.input("A", np.ones(count, dtype=dtype), offset, 128, CPU, dtype=dtype)):
        assert buf.ptr % guarded.BOUNDARY == offset                      # only as aligned as the interface asks for
        assert buf.ptr == buf.raw.data_ptr() + 4 * buf.first
        assert buf.nbytes == count * np.dtype(dtype).itemsize == 4 * (buf.last - buf.first)
        assert 4 * buf.front().numel() >= buf.guard and 4 * buf.back().numel() >= buf.guard
        assert buf.front().numel() + buf.payload().numel() + buf.back().numel() == buf.raw.numel()
        assert (buf.front() == FILL).all() and (buf.back() == FILL).all()
        assert buf.numpy().dtype == dtype and buf.numpy().size == count
    out = Guarded.output("P", count, offset, 128, CPU, dtype=dtype)
    assert (out.payload() == FILL).all()
    if dtype == np.float32:
        assert np.isnan(out.numpy()).all()                               # a guard value that reaches a result is NaN
        assert np.isnan(out.front()[-4:].numpy().view(np.float32)).all()


def test_untouched_buffers_pass():
    buf, data = _input()
    buf.check()
    assert np.array_equal(buf.numpy(), data)
    out = Guarded.output("P", 100, guarded.VALUES, 64, CPU)
    out.payload().copy_(torch.arange(100, dtype=torch.int32))            # "written"
    out.check()
    inplace = Guarded.inplace("X", data, guarded.VALUES, 64, CPU)
    inplace.payload().zero_()                                            # the call may overwrite it
    inplace.check()
    guarded.check_all(buf, None, out, inplace)


def test_last_word_of_the_front_guard():
    buf, _ = _input()
    buf.raw[buf.first - 1] = 0
    msg = _fails(buf)
    assert _span(msg, "front guard changed") == (1, -4, -1) and "back guard" not in msg and "payload modified" not in msg


def test_first_word_of_the_back_guard():
    buf, _ = _input()
    buf.raw[buf.last] = 0
    msg = _fails(buf)
    assert _span(msg, "back guard changed") == (1, buf.nbytes, buf.nbytes + 3) and "front guard" not in msg


def test_far_ends_of_both_guards():
    buf, _ = _input()
    buf.raw[0] = 1
    msg = _fails(buf)
    n, lo, hi = _span(msg, "front guard changed")
    assert (n, lo, hi) == (1, -4 * buf.first, -4 * buf.first + 3) and -lo >= buf.guard
    buf, _ = _input()
    buf.raw[-1] = 1
    n, lo, hi = _span(_fails(buf), "back guard changed")
    assert n == 1 and hi == 4 * (buf.raw.numel() - buf.first) - 1 and lo - buf.nbytes >= buf.guard - 4


def test_a_run_of_words_reports_first_last_and_count():
    buf, _ = _input()
    buf.raw[buf.last + 5:buf.last + 25] = 7
    buf.raw[buf.first - 300] = 7
    msg = _fails(buf)
    assert _span(msg, "back guard changed") == (20, buf.nbytes + 20, buf.nbytes + 99)
    assert _span(msg, "front guard changed") == (1, -1200, -1197)


def test_a_modified_input_word():
    buf, _ = _input()
    buf.payload()[123] ^= 1                                              # one bit of one operand element
    msg = _fails(buf)
    assert _span(msg, "input payload modified") == (1, 492, 495) and "guard changed" not in msg


def test_a_float_written_as_the_same_value_but_other_bits_is_seen():
    buf = Guarded.input("A", np.zeros(8, np.float32), guarded.OPERAND, 32, CPU)
    buf.payload()[3] = -2 ** 31                                          # -0.0 == +0.0 as floats
    assert _span(_fails(buf), "input payload modified") == (1, 12, 15)


def test_an_unwritten_output_word():
    out = Guarded.output("P", 100, guarded.VALUES, 64, CPU)
    out.payload().copy_(torch.arange(100, dtype=torch.int32))
    out.payload()[77] = FILL                                             # every element but one was written
    msg = _fails(out)
    assert _span(msg, "output payload not written") == (1, 308, 311) and "guard changed" not in msg
    fresh = Guarded.output("P", 100, guarded.VALUES, 64, CPU)
    assert _span(_fails(fresh), "output payload not written") == (100, 0, 399)


def test_frozen_output_becomes_an_input():
    out = Guarded.output("A16", 64, guarded.OPERAND, 32, CPU, dtype=np.uint16)
    out.payload().copy_(torch.arange(32, dtype=torch.int32))
    out.check()
    out.freeze()
    out.check()
    out.payload()[31] = 0
    assert _span(_fails(out), "input payload modified") == (1, 124, 127)


def test_the_message_names_the_buffer():
    buf, _ = _input(offset=guarded.VALUES)
    buf.raw[buf.last] = 0
    msg = _fails(buf)
    assert msg.startswith("A (input, 4000 bytes at 4 past a 512-byte boundary)")
