"""MX block scales on the fp8 operand without a GPU (include/bsmr_hip.h "MX block scales"): the four _mx entry
points are declared, exported and bound, the ABI revision did not move, the headers are still C99, and the argument checks
that need no device answer as documented - a NULL plan / handle first, then K, then compute_mode and fp8_format - before
the plan or handle is looked into; bsmr_widen_fp8_mx refuses a count that is no multiple of 32.

The CPU side of the contract is pinned here too, with torch as the reference: mx_dequantize is one fp32 multiplication by
torch.float8_e8m0fnu's value, the ranges in which the 16-bit copy of bsmr_sddmm_b8_mx is exact are the stated ones, and
mx_quantize follows the OCP rule.

As in tests/test_fp8_host.py, the K and mode cases hand the calls a block of zeroed host memory as "handle"."""
import ctypes as C

import numpy as np
import pytest

from test_fp8_host import FORMATS, MODES

torch = pytest.importorskip("torch")

NAMES = ("bsmr_widen_fp8_mx", "bsmr_sddmm_b8_mx", "bsmr_spmm_x8_mx", "bsmr_sparse_attention_x8_mx")
F8 = (torch.float8_e4m3fn, torch.float8_e5m2)
DT16 = (torch.float16, torch.bfloat16)
SCALE_CODES = (0, 1, 2, 3, 10, 126, 127, 128, 254, 255)


@pytest.fixture(scope="module")
def bt(engine):
    import bsmr_torch
    return bsmr_torch


def test_symbols_are_declared_and_bound(engine):
    from test_capi import INCLUDE, LIB, declared_functions, exported

    decl = declared_functions(INCLUDE / "bsmr_hip.h")
    exp = exported(LIB / "libbsmr_hip.so")
    for name in NAMES:
        assert name in decl and name in engine.HIP_SYMBOLS and name in exp, name
    for name in ("widen_fp8_mx", "sddmm_b8_mx", "spmm_x8_mx", "sparse_attention_x8_mx"):
        assert callable(getattr(engine, name)), name
    assert engine.hip().bsmr_abi_revision() == 5   # four functions added, no layout changed


def test_headers_still_compile_as_c(tmp_path):
    from test_capi import test_headers_compile_as_c

    test_headers_compile_as_c(tmp_path)


def test_null_handle_is_refused_without_a_device(engine):
    hip, bad = engine.hip(), engine.ERR_INVALID_ARG
    for mode in MODES:
        for fmt in FORMATS:
            for nb in (1, 0):                                                # num_batches 0 is no excuse
                assert hip.bsmr_sddmm_b8_mx(None, 32, 16, 16, 1, 16, nb, mode, fmt, None) == bad
                assert hip.bsmr_spmm_x8_mx(None, 32, 0, 16, 16, 1, 16, nb, mode, fmt, None) == bad
                assert hip.bsmr_sparse_attention_x8_mx(None, 32, 1.0, 16, 16, 1, 16, 16, 16, nb, mode, fmt, None) == bad
    # the handle is looked at first: a bad K on a NULL handle is still INVALID_ARG
    assert hip.bsmr_sddmm_b8_mx(None, 48, 16, 16, 1, 16, 1, 0, 0, None) == bad
    assert hip.bsmr_spmm_x8_mx(None, 48, 0, 16, 16, 1, 16, 1, 0, 0, None) == bad
    assert hip.bsmr_sparse_attention_x8_mx(None, 48, 1.0, 16, 16, 1, 16, 16, 16, 1, 0, 0, None) == bad


def test_k_and_modes_are_judged_before_the_handle_is_read(engine):
    hip = engine.hip()
    blank = C.create_string_buffer(1 << 16)                                  # zeroed host memory, never a real handle
    h = C.addressof(blank)
    for K in (48, 0, 16, 33):
        for mode in MODES:
            for fmt in FORMATS:                                              # K comes before both modes
                assert hip.bsmr_sddmm_b8_mx(h, K, 16, 16, 1, 16, 1, mode, fmt, None) == engine.ERR_UNSUPPORTED_K
                assert hip.bsmr_spmm_x8_mx(h, K, 0, 16, 16, 1, 16, 1, mode, fmt, None) == engine.ERR_UNSUPPORTED_K
                assert hip.bsmr_sparse_attention_x8_mx(h, K, 1.0, 16, 16, 1, 16, 16, 16, 1, mode, fmt,
                                                       None) == engine.ERR_UNSUPPORTED_K
    for mode in MODES:
        for fmt in FORMATS:
            if mode in (0, 1) and fmt in (0, 1):
                continue
            assert hip.bsmr_sddmm_b8_mx(h, 32, 16, 16, 1, 16, 1, mode, fmt, None) == engine.ERR_INVALID_ARG
            assert hip.bsmr_spmm_x8_mx(h, 32, 0, 16, 16, 1, 16, 1, mode, fmt, None) == engine.ERR_INVALID_ARG
            assert hip.bsmr_sparse_attention_x8_mx(h, 32, 1.0, 16, 16, 1, 16, 16, 16, 1, mode, fmt,
                                                   None) == engine.ERR_INVALID_ARG
    for scale in (float("nan"), float("inf")):                               # with the handle, before K
        assert hip.bsmr_sparse_attention_x8_mx(h, 48, scale, 16, 16, 1, 16, 16, 16, 1, 0, 0, None) == engine.ERR_INVALID_ARG
    assert bytes(blank) == bytes(1 << 16)


def test_widen_mx_count_and_pointer_rules(engine):
    """the modes first; a count that is no multiple of 32 is refused; count 0 is a no-op whatever the pointers; count > 0
    needs all three pointers, the codes and the output 16-byte aligned, the scales at any address"""
    hip, bad = engine.hip(), engine.ERR_INVALID_ARG
    for mode in (0, 1):
        for fmt in (0, 1):
            assert hip.bsmr_widen_fp8_mx(None, None, None, 0, mode, fmt, None) == engine.OK
            assert hip.bsmr_widen_fp8_mx(8, 3, 2, 0, mode, fmt, None) == engine.OK
            for count in (1, 16, 31, 33, 48, 256 + 16):
                assert hip.bsmr_widen_fp8_mx(4096, 4096, 4096, count, mode, fmt, None) == bad, count
                assert hip.bsmr_widen_fp8_mx(None, None, None, count, mode, fmt, None) == bad, count
            for src, sc, dst in ((None, None, None), (None, 4097, 4096), (4096, None, 4096), (4096, 4097, None),
                                 (4096 + 8, 4097, 4096), (4096, 4097, 4096 + 8)):
                assert hip.bsmr_widen_fp8_mx(src, sc, dst, 256, mode, fmt, None) == bad
    for mode in MODES:
        for fmt in FORMATS:
            if not (mode in (0, 1) and fmt in (0, 1)):
                assert hip.bsmr_widen_fp8_mx(None, None, None, 0, mode, fmt, None) == bad


def test_python_wrappers_raise(engine):
    for call in (lambda: engine.widen_fp8_mx(None, None, None, 32),
                 lambda: engine.widen_fp8_mx(4096, 4096, 4096, 48),
                 lambda: engine.widen_fp8_mx(None, None, None, 0, mode=engine.COMPUTE_F32),
                 lambda: engine.sddmm_b8_mx(None, 32, 16, 16, 1, 16, 1, engine.COMPUTE_F16, engine.FP8_E4M3),
                 lambda: engine.spmm_x8_mx(None, 32, False, 16, 16, 1, 16, mode=engine.COMPUTE_BF16, fmt=engine.FP8_E5M2),
                 lambda: engine.sparse_attention_x8_mx(None, 32, 1.0, 16, 16, 1, 16, 16, 16, mode=engine.COMPUTE_F16)):
        with np.testing.assert_raises(engine.BsmrError):
            call()
    engine.widen_fp8_mx(None, None, None, 0)                                 # the no-op does not raise


# ---- the CPU side of the contract --------------------------------------------------------------------------------------
def _table(f8):
    """all 256 codes x SCALE_CODES: codes (10, 256) fp8 with 8 blocks of 32 per row, scales (10, 8) uint8"""
    codes = torch.arange(256, dtype=torch.uint8).repeat(len(SCALE_CODES), 1).view(f8)
    scales = torch.tensor(SCALE_CODES, dtype=torch.uint8).unsqueeze(1).repeat(1, 8)
    return codes, scales


def _same(a, b):
    """equal as numbers, NaN by class, zeros by their sign"""
    a, b = a.to(torch.float64), b.to(torch.float64)
    nan = torch.isnan(a)
    return (torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan], b[~nan])
            and torch.equal(torch.signbit(a[~nan]), torch.signbit(b[~nan])))


@pytest.mark.parametrize("f8", F8)
def test_mx_dequantize_is_one_multiplication_by_the_e8m0_value(bt, f8):
    codes, scales = _table(f8)
    want = codes.float() * scales.view(torch.float8_e8m0fnu).float().repeat_interleave(32, dim=1)
    for sc in (scales, scales.view(torch.float8_e8m0fnu)):
        got = bt.mx_dequantize(codes, sc)
        assert got.dtype == torch.float32 and _same(got, want)
    row = {e: i for i, e in enumerate(SCALE_CODES)}
    one = torch.tensor([1.0]).to(f8).view(torch.uint8).item()
    assert want[row[0], one] == 2.0 ** -127 and want[row[254], one] == 2.0 ** 127       # subnormal kept; 2^127
    assert torch.isnan(want[row[255]]).all()                                               # scale code 255
    assert torch.isinf(want[row[254], torch.tensor([448.0]).to(f8).view(torch.uint8).item()])   # overflow: +inf
    assert torch.signbit(want[:-1, 0x80]).all() and (want[:-1, 0x80] == 0).all()             # -0 keeps its sign
    assert _same(bt.mx_dequantize(codes, scales, torch.bfloat16), want.to(torch.bfloat16))
    for bad in (lambda: bt.mx_dequantize(codes.float(), scales), lambda: bt.mx_dequantize(codes, scales[:, :7]),
                lambda: bt.mx_dequantize(codes, scales.float())):
        with pytest.raises(ValueError):
            bad()


# scale codes for which narrow(dq) is exact for every finite code, wherever dq is finite (include/bsmr_hip.h)
EXACT = {(torch.bfloat16, torch.float8_e4m3fn): range(3, 255), (torch.bfloat16, torch.float8_e5m2): range(10, 255),
         (torch.float16, torch.float8_e4m3fn): range(127 - 15, 127 + 7 + 1), (torch.float16, torch.float8_e5m2): range(127 - 8, 127 + 1)}


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("f8", F8)
def test_the_ranges_in_which_the_16_bit_copy_is_exact(bt, f8, dt):
    """every scale code 0 .. 254 on every finite code: inside the stated range the narrowing changes no finite value;
    directly outside it (one code below, one above where there is one) some value is rounded or overflows"""
    codes = torch.arange(256, dtype=torch.uint8).repeat(255, 1).view(f8)
    scales = torch.arange(255, dtype=torch.uint8).unsqueeze(1).repeat(1, 8)
    dq = bt.mx_dequantize(codes, scales)
    back = dq.to(dt).float()
    finite = torch.isfinite(dq)
    exact_rows = ((back == dq) | ~finite).all(dim=1)
    rng = EXACT[(dt, f8)]
    assert exact_rows[rng.start:rng.stop].all(), (dt, f8, torch.nonzero(~exact_rows[rng.start:rng.stop])[:4])
    assert not exact_rows[rng.start - 1]
    if rng.stop < 255:
        assert not exact_rows[rng.stop]


def _blocks_of_fp8_values(f8, gen, shifts, rows=64, K=128, top_mantissa=1.75):
    """x (rows, K) fp32: every block of 32 holds values of the format times one power of two, 2^shift; the block's largest
    magnitude has a mantissa of at most top_mantissa"""
    codes = torch.randint(0, 256, (rows, K), generator=gen, dtype=torch.uint8)
    special = (codes & 0x7F) == 0x7F if f8 == torch.float8_e4m3fn else (codes & 0x7C) == 0x7C
    codes[special] &= 0xBF
    vals = codes.view(f8).float().reshape(rows, K // 32, 32)
    amax = vals.abs().amax(dim=-1, keepdim=True)
    mant, exp = torch.frexp(amax)
    over = (2 * mant > top_mantissa).expand_as(vals) & (vals.abs() == amax)
    lowered = torch.ldexp(torch.tensor(0.75), exp).expand_as(vals)           # 1.5 2^p: still a value of the format
    vals = torch.where(over, torch.copysign(lowered, vals), vals)
    sh = shifts[torch.randint(0, len(shifts), (rows, K // 32, 1), generator=gen)]
    return (vals.double() * torch.exp2(sh.double())).float().reshape(rows, K)


@pytest.mark.parametrize("f8", F8)
def test_mx_quantize_round_trips_scaled_fp8_blocks(bt, f8):
    """a block that holds fp8 values times one power of two comes back exactly.  The OCP rule takes floor(log2 amax): the
    largest element is scaled to exponent emax, where e4m3 has the mantissas 1 .. 1.75 (1.875 2^8 is its NaN code) - so the
    blocks here keep the mantissa of their largest magnitude at or below 1.75, which every e5m2 value does by itself;
    test_mx_quantize_follows_the_ocp_rule shows the 1.875 case saturate."""
    gen = torch.Generator().manual_seed(5)
    x = _blocks_of_fp8_values(f8, gen, torch.arange(-60, 61))
    assert torch.isfinite(x).all()
    codes, scales = bt.mx_quantize(x, f8)
    assert codes.dtype == f8 and scales.dtype == torch.uint8 and tuple(scales.shape) == (64, 4)
    assert _same(bt.mx_dequantize(codes, scales), x)
    xb = x.reshape(2, 32, 128)                                               # a leading batch
    cb, sb = bt.mx_quantize(xb, f8)
    assert torch.equal(cb.view(torch.uint8).reshape(64, 128), codes.view(torch.uint8)) and torch.equal(sb.reshape(64, 4), scales)


@pytest.mark.parametrize("f8", F8)
def test_mx_quantize_follows_the_ocp_rule(bt, f8):
    emax, top = (8, 448.0) if f8 == torch.float8_e4m3fn else (15, 57344.0)
    x = torch.zeros(6, 32)
    x[0, 3] = 1.0                                                            # amax 1: e = 127 - emax, code 2^emax
    x[1, 0], x[1, 1] = -3.0, 0.75                                            # amax 3: floor(log2) = 1
    x[2] = 0                                                                 # an all-zero block
    x[3, 0], x[3, 1] = 1.9375, 1.0                                           # mantissa above 1.75: saturates
    x[4, 5] = torch.finfo(torch.float32).max                                 # the top of fp32
    x[5, 0], x[5, 1] = 2.0 ** -149, 2.0 ** -135                              # fp32 subnormals: e clamps at 0
    codes, scales = bt.mx_quantize(x, f8)
    assert scales[:, 0].tolist() == [127 - emax, 128 - emax, 0, 127 - emax, 254 - emax, 0]
    dq = bt.mx_dequantize(codes, scales)
    assert _same(dq[:3], x[:3])
    assert dq[3, 0] == 1.75 and dq[3, 1] == 1.0                              # the saturating cast: the largest finite value
    assert codes[3, 0].float() == top
    assert dq[4, 5] == 1.75 * 2.0 ** 127 and torch.isfinite(dq).all()
    assert dq[5, 1] == 2.0 ** -135 and dq[5, 0] == 0                         # 2^-135 2^127 = 2^-8: a value of both formats
    with pytest.raises(ValueError):
        bt.mx_quantize(torch.zeros(4, 48), f8)
    with pytest.raises(ValueError):
        bt.mx_quantize(x, torch.float16)


@pytest.mark.parametrize("f8", F8)
def test_mx_quantize_never_makes_a_finite_value_non_finite(bt, f8):
    gen = torch.Generator().manual_seed(9)
    m = torch.rand(256, 96, generator=gen) + 1.0
    e = torch.randint(-149, 128, (256, 96), generator=gen)
    s = torch.randint(0, 2, (256, 96), generator=gen) * 2.0 - 1.0
    x = (s.double() * m.double() * torch.exp2(e.double())).float()           # the whole fp32 range, subnormals included
    x[0, :32] = torch.finfo(torch.float32).max
    x[1, :32] = -torch.finfo(torch.float32).max
    assert torch.isfinite(x).all()
    codes, scales = bt.mx_quantize(x, f8)
    dq = bt.mx_dequantize(codes, scales)
    assert torch.isfinite(dq).all() and (scales <= 254).all()
    # rounding to nearest inside the block's range: within half a unit of the format at the block's largest exponent
    # (amax 2^-mbits / 2, mantissa bits 3 / 2), or clipped from [1.75, 2) 2^p to 1.75 2^p (at most amax / 8); where the
    # scale code clamps at 0, half the format's subnormal step times 2^-127 on top
    amax = x.abs().reshape(256, 3, 32).amax(dim=-1, keepdim=True).expand(256, 3, 32).reshape(256, 96).double()
    ulp, step = (2.0 ** -3, 2.0 ** -9) if f8 == torch.float8_e4m3fn else (2.0 ** -2, 2.0 ** -16)
    assert ((dq.double() - x.double()).abs() <= amax * max(ulp / 2, 1 / 8) + step / 2 * 2.0 ** -127).all()
    y = x.clone()
    y[2, 7], y[3, 40] = float("nan"), float("inf")                           # NaN stays NaN, inf saturates
    c2, s2 = bt.mx_quantize(y, f8)
    d2 = bt.mx_dequantize(c2, s2)
    assert torch.isnan(d2[2, 7]) and torch.isfinite(d2[3, 40]) and torch.isnan(d2).sum() == 1
