"""MXFP4 keys and values without a GPU (include/bsmr_hip.h "MXFP4 keys and values"): the four entry points are
declared, exported and bound, the ABI revision did not move, the headers are still C99, and the argument checks that need
no device answer as documented - a NULL plan / handle first, then K, then compute_mode - before the plan or handle is
looked into; bsmr_widen_fp4_mx refuses a count that is no multiple of 32.  SparseOperator's ValueErrors are raised before
any device work, so they are shown here on an operator without plan or handle.

The CPU side of the contract is pinned here too.  The reference is built in this file and shares nothing with
bsmr_torch: the eight magnitudes written out, the nibble order, and 2^(e-127) from math.ldexp.  mx_dequantize is checked
on all 256 bytes x all 256 scale codes; the exactness of the 16-bit copy is found, not assumed; mx_quantize follows the OCP
rule with ties to the even code.

As in tests/test_fp8_host.py, the K and mode cases hand the calls a block of zeroed host memory as "handle"."""
import ctypes as C
import math

import numpy as np
import pytest

from test_fp8_host import MODES

torch = pytest.importorskip("torch")

NAMES = ("bsmr_widen_fp4_mx", "bsmr_sddmm_b4_mx", "bsmr_spmm_x4_mx", "bsmr_sparse_attention_x4_mx")
F4 = torch.float4_e2m1fn_x2
DT16 = (torch.float16, torch.bfloat16)
MAG = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)        # OCP e2m1, magnitude codes 0 .. 7


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
    for name in ("widen_fp4_mx", "sddmm_b4_mx", "spmm_x4_mx", "sparse_attention_x4_mx"):
        assert callable(getattr(engine, name)), name
    assert "MXFP4 keys and values" in (INCLUDE / "bsmr_hip.h").read_text()
    assert engine.hip().bsmr_abi_revision() == 5   # four functions added, no layout changed


def test_headers_still_compile_as_c(tmp_path):
    from test_capi import test_headers_compile_as_c

    test_headers_compile_as_c(tmp_path)


def test_null_handle_is_refused_without_a_device(engine):
    hip, bad = engine.hip(), engine.ERR_INVALID_ARG
    for mode in (0, 1):
        for nb in (1, 0):                                                    # num_batches 0 is no excuse
            assert hip.bsmr_sddmm_b4_mx(None, 32, 16, 16, 1, 16, nb, mode, None) == bad
            assert hip.bsmr_spmm_x4_mx(None, 32, 0, 16, 16, 1, 16, nb, mode, None) == bad
            assert hip.bsmr_sparse_attention_x4_mx(None, 32, 1.0, 16, 16, 1, 16, 16, 16, nb, mode, None) == bad
    # the handle is looked at first: a bad K on a NULL handle is still INVALID_ARG
    assert hip.bsmr_sddmm_b4_mx(None, 48, 16, 16, 1, 16, 1, 0, None) == bad
    assert hip.bsmr_spmm_x4_mx(None, 48, 0, 16, 16, 1, 16, 1, 0, None) == bad
    assert hip.bsmr_sparse_attention_x4_mx(None, 48, 1.0, 16, 16, 1, 16, 16, 16, 1, 0, None) == bad


def test_k_and_mode_are_judged_before_the_handle_is_read(engine):
    hip = engine.hip()
    blank = C.create_string_buffer(1 << 16)                                  # zeroed host memory, never a real handle
    h = C.addressof(blank)
    for K in (48, 0, 16, 33):
        for mode in MODES:                                                   # K comes before the mode
            assert hip.bsmr_sddmm_b4_mx(h, K, 16, 16, 1, 16, 1, mode, None) == engine.ERR_UNSUPPORTED_K
            assert hip.bsmr_spmm_x4_mx(h, K, 0, 16, 16, 1, 16, 1, mode, None) == engine.ERR_UNSUPPORTED_K
            assert hip.bsmr_sparse_attention_x4_mx(h, K, 1.0, 16, 16, 1, 16, 16, 16, 1, mode, None) == engine.ERR_UNSUPPORTED_K
    for mode in MODES:
        if mode in (0, 1):
            continue
        assert hip.bsmr_sddmm_b4_mx(h, 32, 16, 16, 1, 16, 1, mode, None) == engine.ERR_INVALID_ARG
        assert hip.bsmr_spmm_x4_mx(h, 32, 0, 16, 16, 1, 16, 1, mode, None) == engine.ERR_INVALID_ARG
        assert hip.bsmr_sparse_attention_x4_mx(h, 32, 1.0, 16, 16, 1, 16, 16, 16, 1, mode, None) == engine.ERR_INVALID_ARG
    for scale in (float("nan"), float("inf")):                               # with the handle, before K
        assert hip.bsmr_sparse_attention_x4_mx(h, 48, scale, 16, 16, 1, 16, 16, 16, 1, 0, None) == engine.ERR_INVALID_ARG
    assert bytes(blank) == bytes(1 << 16)


def test_widen_count_and_pointer_rules(engine):
    """the mode first; a count that is no multiple of 32 is refused; count 0 is a no-op whatever the pointers; count > 0
    needs all three pointers, the codes and the output 16-byte aligned, the scales at any address"""
    hip, bad = engine.hip(), engine.ERR_INVALID_ARG
    for mode in (0, 1):
        assert hip.bsmr_widen_fp4_mx(None, None, None, 0, mode, None) == engine.OK
        assert hip.bsmr_widen_fp4_mx(8, 3, 2, 0, mode, None) == engine.OK
        for count in (1, 16, 31, 33, 48, 256 + 16):
            assert hip.bsmr_widen_fp4_mx(4096, 4096, 4096, count, mode, None) == bad, count
            assert hip.bsmr_widen_fp4_mx(None, None, None, count, mode, None) == bad, count
        for src, sc, dst in ((None, None, None), (None, 4097, 4096), (4096, None, 4096), (4096, 4097, None),
                             (4096 + 8, 4097, 4096), (4096, 4097, 4096 + 8)):
            assert hip.bsmr_widen_fp4_mx(src, sc, dst, 256, mode, None) == bad
    for mode in MODES:
        if mode not in (0, 1):
            assert hip.bsmr_widen_fp4_mx(None, None, None, 0, mode, None) == bad


def test_python_wrappers_raise(engine):
    for call in (lambda: engine.widen_fp4_mx(None, None, None, 32),
                 lambda: engine.widen_fp4_mx(4096, 4096, 4096, 48),
                 lambda: engine.widen_fp4_mx(None, None, None, 0, mode=engine.COMPUTE_F32),
                 lambda: engine.sddmm_b4_mx(None, 32, 16, 16, 1, 16, 1, engine.COMPUTE_F16),
                 lambda: engine.spmm_x4_mx(None, 32, False, 16, 16, 1, 16, mode=engine.COMPUTE_BF16),
                 lambda: engine.sparse_attention_x4_mx(None, 32, 1.0, 16, 16, 1, 16, 16, 16, mode=engine.COMPUTE_F16)):
        with np.testing.assert_raises(engine.BsmrError):
            call()
    engine.widen_fp4_mx(None, None, None, 0)                                 # the no-op does not raise


# ---- SparseOperator's ValueErrors: all raised before any device work ---------------------------------------------------
def _bare_operator(bt, M=6, N=5, nnz=9):
    """an operator without plan and handle, 'living' on the CPU: every check below fails before either would be used"""
    op = bt.SparseOperator.__new__(bt.SparseOperator)
    op.M, op.N, op.nnz, op.device, op.blocked = M, N, nnz, torch.device("cpu"), False
    op._plan = op._bw = None
    return op


def _z4(*shape):
    return torch.zeros(*shape, dtype=torch.uint8).view(F4)


def test_operator_value_errors(bt):
    op = _bare_operator(bt)
    M, N, nnz, K = op.M, op.N, op.nnz, 64
    A, v = torch.zeros(M, K, dtype=torch.bfloat16), torch.zeros(nnz)
    X4, E = _z4(N, K // 2), torch.full((N, K // 32), 127, dtype=torch.uint8)
    e8 = E.view(torch.float8_e8m0fnu)
    bad_scales = (None,                                                      # missing: the scales are mandatory
                  E.float(), E.to(torch.int8),                               # dtype
                  E[:, :1].contiguous(), E[:-1].contiguous(), E.repeat(1, 2),  # shape: blocks, rows, K/16
                  E.unsqueeze(0),                                            # a batch the operand has not
                  E.to("meta"),                                              # device
                  E.t().contiguous().t(),                                    # not contiguous
                  e8.clone().requires_grad_(True))                           # no gradient into scales
    for sc in bad_scales:
        with pytest.raises(ValueError):
            op.sddmm(A, X4, B_scale=sc)
        with pytest.raises(ValueError):
            op.spmm(v, X4, out_dtype=torch.bfloat16, X_scale=sc)
        with pytest.raises(ValueError):
            op.softmax_spmm(v, X4, 1.0, out_dtype=torch.bfloat16, X_scale=sc)
        with pytest.raises(ValueError):
            op.attention(A, X4, X4, Kt_scale=sc, V_scale=E)
        with pytest.raises(ValueError):
            op.attention(A, torch.zeros(N, K, dtype=torch.bfloat16), X4, V_scale=sc)
    g4 = _z4(N, K // 2).requires_grad_(True)                                 # no gradient into codes
    for call in (lambda: op.sddmm(A, g4, B_scale=E),
                 lambda: op.spmm(v, g4, out_dtype=torch.float16, X_scale=E),
                 lambda: op.softmax_spmm(v, g4, 1.0, out_dtype=torch.float16, X_scale=E),
                 lambda: op.spmm(v, _z4(M, K // 2), transpose=True, out_dtype=torch.float16,
                                 X_scale=torch.zeros(M, K // 32, dtype=torch.uint8)),
                 lambda: op.spmm(v, X4, X_scale=E),                          # out_dtype missing
                 lambda: op.spmm(v, X4, out_dtype=torch.float32, X_scale=E),
                 lambda: op.spmm(v, X4, out_dtype=F4, X_scale=E),
                 lambda: op.softmax_spmm(v, X4, 1.0, X_scale=E),
                 lambda: op.softmax_spmm(v, X4, 1.0, out_dtype=torch.float32, X_scale=E),
                 lambda: op.sddmm(torch.zeros(M, K), X4, B_scale=E),         # an fp32 A beside an fp4 B
                 lambda: op.sddmm(torch.zeros(M, 32, dtype=torch.bfloat16), X4, B_scale=E)):   # A and B disagree on K
        with pytest.raises(ValueError):
            call()
    # K / 2 = 24 bytes per row: K = 48 is no multiple of 32 (one block of scales, so the scale check lets it through)
    odd, e1 = _z4(N, 24), torch.zeros(N, 1, dtype=torch.uint8)
    for call in (lambda: op.sddmm(torch.zeros(M, 48, dtype=torch.bfloat16), odd, B_scale=e1),
                 lambda: op.spmm(v, odd, out_dtype=torch.bfloat16, X_scale=e1),
                 lambda: op.softmax_spmm(v, odd, 1.0, out_dtype=torch.bfloat16, X_scale=e1)):
        with pytest.raises(ValueError, match="multiple of 32"):
            call()
    # a scale beside an operand that is neither fp8 nor fp4 is still refused
    with pytest.raises(ValueError):
        op.sddmm(A, torch.zeros(N, K, dtype=torch.bfloat16), B_scale=E)


# ---- the CPU side of the contract --------------------------------------------------------------------------------------
def _value(nibble):
    m = MAG[nibble & 7]
    return -m if nibble & 8 else m


def _scale(e):
    """2^(e - 127) as a Python float (exact), NaN for 255"""
    return float("nan") if e == 255 else math.ldexp(1.0, e - 127)


def _table_reference():
    """(256 scale codes, 512 elements) fp32: row e holds byte 0's two elements, byte 1's, ... under scale code e - built from
    the format's definition in fp64 (every product is exact there), then cast to fp32 (exact wherever fp32 can hold it,
    +-inf beyond)"""
    vals = np.array([_value(b & 15) if k == 0 else _value(b >> 4) for b in range(256) for k in (0, 1)], np.float64)
    sc = np.array([_scale(e) for e in range(256)], np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy((vals[None, :] * sc[:, None]).astype(np.float32))


def _table_inputs():
    codes = torch.arange(256, dtype=torch.uint8).repeat(256, 1).view(F4)     # (256, 256 bytes): K = 512, 16 blocks
    scales = torch.arange(256, dtype=torch.int32).to(torch.uint8).unsqueeze(1).repeat(1, 16)
    return codes, scales


def _same(a, b):
    """equal as numbers, NaN by class, zeros by their sign"""
    a, b = a.to(torch.float64), b.to(torch.float64)
    nan = torch.isnan(a)
    return (torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan], b[~nan])
            and torch.equal(torch.signbit(a[~nan]), torch.signbit(b[~nan])))


def test_mx_dequantize_on_every_byte_and_every_scale_code(bt):
    codes, scales = _table_inputs()
    want = _table_reference()
    for sc in (scales, scales.view(torch.float8_e8m0fnu)):
        got = bt.mx_dequantize(codes, sc)
        assert got.dtype == torch.float32 and tuple(got.shape) == (256, 512) and _same(got, want)
    # what the contract states, on the reference: low nibble first, subnormals kept, the overflow from 253 on, NaN at 255
    assert want[127, 2 * 0x21].item() == 0.5 and want[127, 2 * 0x21 + 1].item() == 1.0
    assert want[0, 2 * 0x01].item() == 2.0 ** -128 and want[254, 2 * 0x02].item() == 2.0 ** 127
    fin = torch.isfinite(want)
    assert fin[:253].all() and not fin[253].all() and not fin[254].all() and fin[254, 2 * 0x02]
    assert want[253, 2 * 0x07].item() == math.inf and want[253, 2 * 0x0F].item() == -math.inf         # 6 2^126
    assert want[253, 2 * 0x06].item() == math.inf and want[253, 2 * 0x05].item() == 1.5 * 2.0 ** 127  # 4 2^126 = 2^128; 3 2^126
    assert torch.isnan(want[255]).all()                                      # the zeros included
    assert (want[:255, 2 * 0x08] == 0).all() and torch.signbit(want[:255, 2 * 0x08]).all()   # -0 keeps its sign
    assert _same(bt.mx_dequantize(codes, scales, torch.bfloat16), want.to(torch.bfloat16))
    for bad in (lambda: bt.mx_dequantize(codes.view(torch.uint8), scales), lambda: bt.mx_dequantize(codes, scales[:, :15]),
                lambda: bt.mx_dequantize(codes, scales.float()), lambda: bt.mx_dequantize(codes, scales.repeat(1, 2))):
        with pytest.raises(ValueError):
            bad()


def _exact_rows(dq, dt):
    back = dq.to(dt).float()
    return ((back == dq) | (torch.isnan(back) & torch.isnan(dq))).all(dim=1)


def test_the_16_bit_copy_bf16_always_fp16_in_a_window(bt):
    """narrow(dq) over all 16 codes x 256 scale codes: bf16 holds every element for every scale code (the overflows and
    the NaN row as themselves); fp16 only inside one window of shifts, which is found here and must be the one the header
    and DESIGN state; the code below it rounds an element, the code above it overflows"""
    dq = _table_reference()
    assert _exact_rows(dq, torch.bfloat16).all()
    ok = _exact_rows(dq[:255], torch.float16)
    inside = torch.nonzero(ok).ravel()
    lo, hi = int(inside.min()), int(inside.max())
    assert ok[lo:hi + 1].all() and int(ok.sum()) == hi - lo + 1              # one window
    assert (lo - 127, hi - 127) == (-23, 13)                                 # include/bsmr_hip.h, DESIGN.md 17
    below, above = dq[lo - 1], dq[hi + 1]
    assert torch.isfinite(below.half()).all() and (below.half().float() != below).any()      # rounded: 0.5 2^-24 -> 0
    assert torch.isfinite(above).all() and torch.isinf(above.half()).any()                   # 6 2^14 > 65504
    header = (__import__("test_capi").INCLUDE / "bsmr_hip.h").read_text()
    assert "[-23, 13]" in header and "104 .. 140" in header


def test_mx_quantize_ties_go_to_the_even_code(bt):
    ties = [(0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0)]
    x = torch.zeros(2, 32)
    x[0, 0], x[1, 0] = 4.0, -4.0                                             # amax 4: e = 127, the values as they are
    for i, (t, _) in enumerate(ties):
        x[0, i + 1], x[1, i + 1] = t, -t
    codes, scales = bt.mx_quantize(x, F4)
    assert codes.dtype == F4 and tuple(codes.shape) == (2, 16) and scales.dtype == torch.uint8 and scales.tolist() == [[127], [127]]
    dq = bt.mx_dequantize(codes, scales)
    want = torch.tensor([4.0] + [w for _, w in ties])
    assert _same(dq[0, :8], want) and _same(dq[1, :8], -want)                # -0.25 -> -0
    # a hair beside each tie goes to the nearer neighbour
    up = torch.zeros(1, 32)
    up[0, 0] = 4.0
    for i, (t, _) in enumerate(ties):
        up[0, 2 * i + 1], up[0, 2 * i + 2] = t * (1 + 2.0 ** -20), t * (1 - 2.0 ** -20)
    d = bt.mx_dequantize(*bt.mx_quantize(up, F4))[0]
    for i in range(7):
        assert d[2 * i + 1].item() == MAG[i + 1] and d[2 * i + 2].item() == MAG[i], i


def test_mx_quantize_follows_the_ocp_rule_and_saturates(bt):
    x = torch.zeros(8, 32)
    x[0, 3] = 1.0                                                            # amax 1: e = 127 - 2, the code of 4
    x[1, 0], x[1, 1] = -3.0, 0.75                                            # amax 3: floor(log2) = 1, e = 126
    x[2] = 0                                                                 # an all-zero block
    x[3, 0], x[3, 1], x[3, 2] = 7.5, -7.9, 5.5                               # amax 7.9: e = 127; beyond 6 saturates
    x[4, 5] = torch.finfo(torch.float32).max                                 # the top of fp32: e = 252
    x[5, 0], x[5, 1] = 2.0 ** -149, 2.0 ** -127                              # fp32 subnormals: e clamps at 0
    x[6, 0], x[6, 1] = float("inf"), 1.0                                     # inf is no amax and saturates
    x[7, 0], x[7, 1] = 1.75, 1.0                                             # a mantissa above 1.5: 7 saturates to 6
    codes, scales = bt.mx_quantize(x, F4)
    assert scales[:, 0].tolist() == [125, 126, 0, 127, 252, 0, 125, 125]
    raw = codes.view(torch.uint8)
    assert raw[0, 1].item() == 0x60 and raw[1, 0].item() == 0x3F             # element 3: a high nibble; (-6, 1.5) / 2
    dq = bt.mx_dequantize(codes, scales)
    assert _same(dq[:3], x[:3])
    assert dq[3, :3].tolist() == [6.0, -6.0, 6.0]                            # 5.5 is nearer 6 than 4
    assert dq[4, 5].item() == 6.0 * 2.0 ** 125 and torch.isfinite(dq).all()
    assert dq[5, 1].item() == 2.0 ** -127 and dq[5, 0].item() == 0
    assert dq[6, 0].item() == 6.0 * 2.0 ** -2 and dq[6, 1].item() == 1.0
    assert dq[7, 0].item() == 1.5 and dq[7, 1].item() == 1.0                 # the known clipping of the floor rule
    with pytest.raises(ValueError):
        bt.mx_quantize(torch.zeros(4, 48), F4)
    nan = torch.zeros(1, 32)
    nan[0, 9] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        bt.mx_quantize(nan, F4)


def test_mx_quantize_packs_the_low_nibble_first(bt):
    x = torch.zeros(1, 32)
    x[0, 0], x[0, 1], x[0, 2], x[0, 3], x[0, 31] = 6.0, -0.5, -0.0, 1.5, -6.0
    codes, scales = bt.mx_quantize(x, F4)
    raw = codes.view(torch.uint8)[0]
    assert scales.item() == 127
    assert raw[0].item() == 0x97 and raw[1].item() == 0x38 and raw[15].item() == 0xF0    # (6, -0.5), (-0, 1.5), (0, -6)


def test_mx_quantize_round_trips_scaled_e2m1_blocks(bt):
    """a block that holds e2m1 values times one power of two comes back exactly, -0 included, whenever its largest
    magnitude is 4 or 6 times that power (the floor rule then finds the power itself) - over the whole range of scale codes
    a quantiser can emit; with a leading batch the same codes"""
    gen = torch.Generator().manual_seed(5)
    rows, K = 64, 128
    nib = torch.randint(0, 16, (rows, K), generator=gen)
    nib.view(rows, K // 32, 32)[:, :, 0] = torch.randint(6, 8, (rows, K // 32), generator=gen)   # 4 or 6 in every block
    vals = torch.tensor([_value(n) for n in range(16)], dtype=torch.float64)[nib]
    e = torch.randint(0, 253, (rows, K // 32, 1), generator=gen)
    x = (vals.view(rows, K // 32, 32) * torch.exp2((e - 127).double())).float().view(rows, K)
    assert torch.isfinite(x).all()
    codes, scales = bt.mx_quantize(x, F4)
    assert torch.equal(scales, e.squeeze(-1).to(torch.uint8))
    packed = (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8)
    assert torch.equal(codes.view(torch.uint8), packed)
    assert _same(bt.mx_dequantize(codes, scales), x)
    cb, sb = bt.mx_quantize(x.reshape(2, 32, K), F4)
    assert torch.equal(cb.view(torch.uint8).reshape(rows, K // 2), packed) and torch.equal(sb.reshape(rows, K // 32), scales)


def test_mx_quantize_never_makes_a_finite_value_non_finite(bt):
    gen = torch.Generator().manual_seed(9)
    m = torch.rand(256, 96, generator=gen) + 1.0
    e = torch.randint(-149, 128, (256, 96), generator=gen)
    s = torch.randint(0, 2, (256, 96), generator=gen) * 2.0 - 1.0
    x = (s.double() * m.double() * torch.exp2(e.double())).float()           # the whole fp32 range, subnormals included
    x[0, :32] = torch.finfo(torch.float32).max
    x[1, :32] = -torch.finfo(torch.float32).max
    assert torch.isfinite(x).all()
    codes, scales = bt.mx_quantize(x, F4)
    dq = bt.mx_dequantize(codes, scales)
    assert torch.isfinite(dq).all() and (scales <= 252).all()
    # amax = f 2^p with f in [1, 2) is scaled to f 4: the grid there has steps of 2 (half a step: amax / 4 at most, the
    # saturation from up to 8 down to 6 included); where the scale code clamps at 0 half the smallest step, 0.25 2^-127
    amax = x.abs().reshape(256, 3, 32).amax(dim=-1, keepdim=True).expand(256, 3, 32).reshape(256, 96).double()
    assert ((dq.double() - x.double()).abs() <= amax / 4 + 0.25 * 2.0 ** -127).all()
    assert torch.equal(torch.signbit(dq), torch.signbit(x))
