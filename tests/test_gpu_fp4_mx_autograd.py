"""bsmr_torch.SparseOperator with MXFP4 operands (torch.float4_e2m1fn_x2 with B_scale, X_scale, Kt_scale, V_scale): sddmm, spmm,
softmax_spmm and attention, composed and fused, with Kt only, V only and both in fp4, and with an fp8 Kt beside an fp4 V.

With dq = mx_dequantize(codes, scales) (pinned on every byte and scale code in tests/test_fp4_mx_host.py) the checks are
those of tests/test_gpu_fp8_mx_autograd.py with their numbers and no others:
  * every call gives the bits of the raw _x4_mx / _b4_mx calls it is documented to be, forward and backward;
  * every call gives the bits of the same SparseOperator call on the e4m3 re-encoding of the codes with the same scales;
  * 16-bit results and gradients are oracle.round_array(format, gather twin) on dq, bit for bit;
  * products of integers under power-of-two block scales are the exact fp64 dot products;
  * the forward of attention stays within 2 u16 max_row |V| of dense fp64 attention, and the gradient into `values` of
    softmax_spmm inside the bound of DESIGN.md 13 (_fp64_rows), both taken on the dequantised tensors.
Then: every ValueError of the interface on a live operator, and a blocked=True operator against the unblocked one."""
import numpy as np
import pytest

import blocked_twin as bt
from gather_twin import assert_twin
from test_gpu_attention_fused_autograd import _fp64_rows, op16  # noqa: F401  (op16: that module's fixture)
from test_gpu_fp8_autograd import _ints, _same
from test_gpu_fp8_mx_autograd import _narrow, _scales
from test_gpu_io16_autograd import DT, U16, _bits, _np, _operands, _rounded, _t, _t16, _wide

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 64
F4 = torch.float4_e2m1fn_x2
E4M3 = torch.float8_e4m3fn
INTS4 = np.array([0, 1, 2, 3, 4, 6, -1, -2, -3, -4, -6], np.float32)         # the integers of e2m1
MAG4 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], np.float32)        # magnitude codes 0 .. 7


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _quantized(x):
    """(codes, scales) of an fp32 array through mx_quantize, on the device"""
    import bsmr_torch
    c, s = bsmr_torch.mx_quantize(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), F4)
    return c.to(_dev()), s.to(_dev())


def _t4(values):
    """an array of e2m1 values -> the packed device tensor: the nibble is the value's place in the table, bit 3 its sign,
    element 2i in the low nibble of byte i"""
    a = np.ascontiguousarray(values, dtype=np.float32)
    nib = np.searchsorted(MAG4, np.abs(a)).astype(np.uint8)
    assert (MAG4[nib] == np.abs(a)).all()
    nib |= np.signbit(a).astype(np.uint8) << 3
    return torch.from_numpy(nib[..., 0::2] | (nib[..., 1::2] << 4)).view(F4).to(_dev())


def _dq(t4, ts):
    import bsmr_torch
    return bsmr_torch.mx_dequantize(t4.cpu(), ts.cpu()).numpy()


def _as_e4m3(t4):
    """the same values, one e4m3 code each"""
    import bsmr_torch
    plain = bsmr_torch.mx_dequantize(t4.cpu(), torch.full(tuple(t4.shape[:-1]) + (t4.shape[-1] // 16,), 127, dtype=torch.uint8))
    c = plain.to(E4M3)
    assert torch.equal(c.float(), plain) and torch.equal(torch.signbit(c.float()), torch.signbit(plain))
    return c.to(_dev())


@pytest.mark.parametrize("batch", (None, 2))
@pytest.mark.parametrize("mode", (0, 1))
def test_sddmm_is_exact_and_da_equals_the_rounded_twin(engine, oracle, op16, mode, batch):
    o = op16
    rng = np.random.default_rng(420 + 2 * mode + bool(batch))
    lead = () if batch is None else (batch,)
    tA, A = _t16(mode, _ints(rng, *lead, o.M, K), grad=True)
    tB = _t4(INTS4[rng.integers(0, INTS4.size, lead + (o.N, K))])
    tE = _scales(lead + (o.N, K // 32), 125, 130, e8m0=bool(batch))           # 2^-2 .. 2^3: exact everywhere
    B = _dq(tB, tE)
    G = _wide(rng, lead + (o.nnz,), -3, 3)
    P = o.sddmm(tA, tB, B_scale=tE)
    assert P.dtype == torch.float32 and P.shape == lead + (o.nnz,)
    row_of = np.repeat(np.arange(o.M), np.diff(o.ro))
    exact = np.einsum("...tk,...tk->...t", A[..., row_of, :].astype(np.float64), B[..., o.ci, :].astype(np.float64))
    assert np.array_equal(_np(P).astype(np.float64), exact)
    P.backward(_t(G))
    assert tA.grad.dtype == DT[mode] and tB.grad is None
    assert_twin(_np(tA.grad), _rounded(oracle, mode, o.rl, G, B), f"dA mode={mode}")
    # the raw calls
    nb, e8 = batch or 1, tE.view(torch.uint8)
    rawP = torch.full_like(P, float("nan"))
    rawdA = torch.full_like(tA.grad, float("nan"))
    engine.sddmm_b4_mx(o._plan, K, tA.data_ptr(), tB.data_ptr(), e8.data_ptr(), rawP.data_ptr(), nb, mode, _stream())
    tG = _t(G)
    engine.spmm_x4_mx(o._bw, K, False, tG.data_ptr(), tB.data_ptr(), e8.data_ptr(), rawdA.data_ptr(), nb, _stream(), mode=mode)
    torch.cuda.synchronize()
    assert _same(P, rawP) and _bits(tA.grad) == _bits(rawdA)
    assert _same(P, o.sddmm(tA.detach(), _narrow(mode, B)[0]))               # the 16-bit call on narrow(dq)
    # the e4m3 re-encoding under the same scales
    a8 = tA.detach().clone().requires_grad_(True)
    P8 = o.sddmm(a8, _as_e4m3(tB), B_scale=tE)
    P8.backward(_t(G))
    assert _same(P, P8) and _bits(tA.grad) == _bits(a8.grad)


@pytest.mark.parametrize("batch", (None, 2))
@pytest.mark.parametrize("mode", (0, 1))
def test_spmm_equals_the_rounded_twin_and_dvalues_is_exact(engine, oracle, op16, mode, batch):
    o = op16
    rng = np.random.default_rng(440 + 2 * mode + bool(batch))
    lead = () if batch is None else (batch,)
    v = _wide(rng, lead + (o.nnz,), -3, 3)
    tv = _t(v, grad=True)
    tX = _t4(INTS4[rng.integers(0, INTS4.size, lead + (o.N, K))])
    tE = _scales(lead + (o.N, K // 32), 125, 130, salt=1, e8m0=not batch)
    X = _dq(tX, tE)
    tH, H = _t16(mode, _ints(rng, *lead, o.M, K))
    Y = o.spmm(tv, tX, out_dtype=DT[mode], X_scale=tE)
    assert Y.dtype == DT[mode] and Y.shape == lead + (o.M, K)
    assert_twin(_np(Y), _rounded(oracle, mode, o.rl, v, X), f"spmm mode={mode}")
    assert _bits(Y) == _bits(o.spmm(tv.detach(), _narrow(mode, X)[0]))       # exact copy: the 16-bit call, the same bits
    Y.backward(tH)
    row_of = np.repeat(np.arange(o.M), np.diff(o.ro))
    exact = np.einsum("...tk,...tk->...t", H[..., row_of, :].astype(np.float64), X[..., o.ci, :].astype(np.float64))
    assert tv.grad.dtype == torch.float32 and np.array_equal(_np(tv.grad).astype(np.float64), exact)
    nb, e8 = batch or 1, tE.view(torch.uint8)
    rawY, rawdv = torch.full_like(Y, float("nan")), torch.full_like(tv.grad, float("nan"))
    engine.spmm_x4_mx(o._bw, K, False, tv.data_ptr(), tX.data_ptr(), e8.data_ptr(), rawY.data_ptr(), nb, _stream(), mode=mode)
    engine.sddmm_b4_mx(o._plan, K, tH.data_ptr(), tX.data_ptr(), e8.data_ptr(), rawdv.data_ptr(), nb, mode, _stream())
    torch.cuda.synchronize()
    assert _bits(Y) == _bits(rawY) and _same(tv.grad, rawdv)
    v8 = _t(v, grad=True)
    Y8 = o.spmm(v8, _as_e4m3(tX), out_dtype=DT[mode], X_scale=tE)
    Y8.backward(tH)
    assert _bits(Y) == _bits(Y8) and _same(tv.grad, v8.grad)


@pytest.mark.parametrize("mode", (0, 1))
def test_softmax_spmm_trains_values_on_a_quantized_v(engine, op16, mode):
    """V goes through mx_quantize; the bounds are taken on dq(V)"""
    o = op16
    rng = np.random.default_rng(460 + mode)
    _, _, V, H = _operands(mode, rng, o)
    scale = K ** -0.5
    scores = rng.uniform(-8, 8, o.nnz).astype(np.float32)
    tV, tE = _quantized(V)
    wV = _dq(tV, tE)
    amax = np.abs(V).reshape(o.N, K // 32, 32).max(axis=-1).repeat(32, axis=-1)
    assert (np.abs(wV - V) <= amax / 4).all() and np.abs(wV).max() > 0                     # the round trip is a quantisation
    tH, wH = _t16(mode, H)
    P = _t(scores, grad=True)
    O = o.softmax_spmm(P, tV, scale, out_dtype=DT[mode], X_scale=tE)
    O.backward(tH)
    assert O.dtype == DT[mode] and P.grad.dtype == torch.float32
    # the raw calls, forward and backward
    Or, m, s = o._attention_x4(P.detach(), tV, scale, DT[mode], tE)
    rO, rm, rs = (torch.full_like(t, float("nan")) for t in (Or, m, s))
    engine.sparse_attention_x4_mx(o._bw, K, scale, P.data_ptr(), tV.data_ptr(), tE.data_ptr(), rO.data_ptr(), rm.data_ptr(),
                                  rs.data_ptr(), 1, _stream(), mode=mode)
    dWr = torch.full((o.nnz,), float("nan"), device=_dev())
    engine.sddmm_b4_mx(o._plan, K, tH.data_ptr(), tV.data_ptr(), tE.data_ptr(), dWr.data_ptr(), 1, mode, _stream())
    torch.cuda.synchronize()
    assert _bits(O) == _bits(rO) and _same(m, rm) and _same(s, rs)
    dPr, _ = o._attention_backward(P.detach(), rm, rs, dWr.clone(), rO, tH, scale)     # (it writes dP over its dW)
    assert _same(P.grad, dPr)
    # the fp32 call on dq: O rounded once, m and s in bits
    O32, m32, s32 = o._attention(P.detach(), _t(wV), scale)
    assert _bits(O) == _bits(O32.to(DT[mode])) and _same(m, m32) and _same(s, s32)
    # the e4m3 re-encoding under the same scales
    P8 = _t(scores, grad=True)
    O8 = o.softmax_spmm(P8, _as_e4m3(tV), scale, out_dtype=DT[mode], X_scale=tE)
    O8.backward(tH)
    assert _bits(O) == _bits(O8) and _same(P.grad, P8.grad)
    # fp64 on dq(V): the forward within one output rounding, dP inside its bound (dW as the device made it)
    O64, dP64, b16, b32 = _fp64_rows(o, scores, scale, wV, wH, _np(dWr).astype(np.float64))
    vmax = np.maximum.reduceat(np.abs(wV.astype(np.float64))[o.ci], o.ro[:-1], axis=0)
    err = np.abs(_np(O).astype(np.float64) - O64)
    print(f"mode={mode}: worst |O - O64| / bound = {(err / (2 * U16[mode] * vmax)).max():.3f}")
    assert (err <= 2 * U16[mode] * vmax).all()
    err = np.abs(_np(P.grad).astype(np.float64) - dP64)
    bound = U16[mode] * b16 + b32
    print(f"mode={mode}: worst |dP - dP64| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("which", ("kt", "v", "both", "kt8-v4"))
@pytest.mark.parametrize("mode", (0, 1))
def test_attention_composed_and_fused(engine, oracle, op16, mode, which):
    """Kt and V through mx_quantize; the one left out stays a 16-bit tensor; kt8-v4: an MXFP8 (e4m3) Kt beside an fp4 V"""
    import bsmr_torch
    o = op16
    rng = np.random.default_rng(480 + mode)
    Q, Kt, V, H = _operands(mode, rng, o)
    scale = K ** -0.5
    tH, wH = _t16(mode, H)
    kkw, vkw, okw = {}, {}, {}
    tK8 = tV8 = None                                                         # the e4m3 re-encodings of the fp4 tensors
    if which in ("kt", "both"):
        tK, tKs = _quantized(Kt)
        dqK, tK8, kkw = _dq(tK, tKs), _as_e4m3(tK), dict(Kt_scale=tKs)
        wK = _narrow(mode, dqK)[1]                                           # what the SDDMM runs on
    elif which == "kt8-v4":
        c, s = bsmr_torch.mx_quantize(torch.from_numpy(Kt), E4M3)
        tK, tKs = c.to(_dev()), s.to(_dev())
        dqK, tK8, kkw = bsmr_torch.mx_dequantize(c, s).numpy(), tK, dict(Kt_scale=tKs)
        wK = _narrow(mode, dqK)[1]
    else:
        tK, wK = _t16(mode, Kt)
        dqK, tK8 = wK, tK
    if which in ("v", "both", "kt8-v4"):
        tV, tVs = _quantized(V)
        wV, tV8, vkw, okw = _dq(tV, tVs), _as_e4m3(tV), dict(V_scale=tVs), dict(out_dtype=DT[mode])
    else:
        tV, wV = _t16(mode, V)
        tV8 = tV

    def run(how):
        tQ, wQ = _t16(mode, Q, grad=True)
        out = how(tQ)
        O = out[0] if isinstance(out, tuple) else out
        O.backward(tH)
        return (O, tQ.grad, wQ) + (out[1:] if isinstance(out, tuple) else ())

    def by_hand(tQ):
        P = o.sddmm(tQ, tK, B_scale=kkw.get("Kt_scale"))
        W = o.softmax(P, scale)
        P.retain_grad()
        return o.spmm(W, tV, X_scale=vkw.get("V_scale"), **okw), P, W
    O, dQ, wQ, P, W = run(by_hand)
    assert O.dtype == DT[mode] and dQ.dtype == DT[mode] and P.dtype == torch.float32
    assert_twin(_np(O), _rounded(oracle, mode, o.rl, _np(W), wV), f"O mode={mode} {which}")
    assert_twin(_np(dQ), _rounded(oracle, mode, o.rl, _np(P.grad), dqK), f"Q.grad mode={mode} {which}")
    # dense fp64 attention on the dequantised tensors
    mask = np.zeros((o.M, o.N), dtype=bool)
    mask[np.repeat(np.arange(o.M), np.diff(o.ro)), o.ci] = True
    Z = np.where(mask, (wQ.astype(np.float64) @ wK.astype(np.float64).T) * scale, -np.inf)
    E = np.exp(Z - Z.max(axis=1, keepdims=True))
    O64 = (E / E.sum(axis=1, keepdims=True)) @ wV.astype(np.float64)
    bound = 2 * U16[mode] * np.maximum.reduceat(np.abs(wV.astype(np.float64))[o.ci], o.ro[:-1], axis=0)
    assert (np.abs(_np(O).astype(np.float64) - O64) <= bound).all()
    # op.attention is that composition; the fused path is softmax_spmm written out
    a = run(lambda tQ: o.attention(tQ, tK, tV, **kkw, **vkw))
    assert _bits(a[0]) == _bits(O) and _bits(a[1]) == _bits(dQ)
    f = run(lambda tQ: o.attention(tQ, tK, tV, fused=True, **kkw, **vkw))
    g = run(lambda tQ: o.softmax_spmm(o.sddmm(tQ, tK, B_scale=kkw.get("Kt_scale")), tV, scale, X_scale=vkw.get("V_scale"), **okw))
    assert f[0].dtype == DT[mode] and _bits(f[0]) == _bits(g[0]) and _bits(f[1]) == _bits(g[1])
    assert (np.abs(_np(f[0]).astype(np.float64) - O64) <= bound).all()
    assert np.isfinite(_np(f[1])).all() and np.abs(_np(f[1])).max() > 0
    # the same calls on the e4m3 re-encodings under the same scales
    for fused in (False, True):
        w4 = run(lambda tQ: o.attention(tQ, tK, tV, fused=fused, **kkw, **vkw))
        w8 = run(lambda tQ: o.attention(tQ, tK8, tV8, fused=fused, **kkw, **vkw))
        assert _bits(w4[0]) == _bits(w8[0]) and _bits(w4[1]) == _bits(w8[1]), (which, fused)


def _z4(*shape):
    return torch.zeros(*shape, dtype=torch.uint8).view(F4).to(_dev())


def test_every_value_error(engine, op16):
    o = op16
    A, B = torch.zeros(o.M, K, device=_dev()), torch.zeros(o.N, K, device=_dev())
    v = torch.zeros(o.nnz, device=_dev())
    E = torch.full((o.N, K // 32), 127, dtype=torch.uint8, device=_dev())
    half = dict(out_dtype=torch.float16)
    B4, B4b = _z4(o.N, K // 2), _z4(2, o.N, K // 2)
    # missing, dtype, shape, batch, device, layout, grad, type
    bad = (None, E.float(), E.to(torch.int8), E.half(), E[:, :1].contiguous(), E[:-1].contiguous(), E.reshape(-1),
           E.repeat(1, 2), E.unsqueeze(0), E.repeat(2, 1, 1), E.cpu(), E.repeat(1, 2)[:, ::2], E.t().contiguous().t(),
           E.float().requires_grad_(True), E.cpu().numpy(), 127, E.view(torch.float8_e8m0fnu).requires_grad_(True))
    for sc in bad:
        for call in (lambda: o.sddmm(A.half(), B4, B_scale=sc), lambda: o.spmm(v, B4, X_scale=sc, **half),
                     lambda: o.softmax_spmm(v, B4, 1.0, X_scale=sc, **half),
                     lambda: o.attention(A.half(), B4, B.half(), Kt_scale=sc),
                     lambda: o.attention(A.half(), B.half(), B4, V_scale=sc),
                     lambda: o.attention(A.half(), B4, B4, Kt_scale=E, V_scale=sc, fused=True)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        o.spmm(torch.zeros(2, o.nnz, device=_dev()), B4b, X_scale=E, **half)               # an unbatched scale, a batched X
    with pytest.raises(ValueError):
        o.sddmm(A.half(), B4, B_scale=E.repeat(2, 1, 1))                                   # and the other way round
    # out_dtype, transpose, the dtype of A, K, the batch, a gradient into the codes
    EM = torch.full((o.M, K // 32), 127, dtype=torch.uint8, device=_dev())
    for call in (lambda: o.spmm(v, B4, X_scale=E), lambda: o.spmm(v, B4, X_scale=E, out_dtype=torch.float32),
                 lambda: o.spmm(v, _z4(o.M, K // 2), X_scale=EM, out_dtype=torch.float16, transpose=True),
                 lambda: o.softmax_spmm(v, B4, 1.0, X_scale=E), lambda: o.softmax_spmm(v, B4, 1.0, X_scale=E, out_dtype=F4),
                 lambda: o.sddmm(A, B4, B_scale=E),
                 lambda: o.sddmm(torch.zeros(o.M, 32, device=_dev()).half(), B4, B_scale=E),
                 lambda: o.sddmm(torch.zeros(o.M, 48, device=_dev()).half(), _z4(o.N, 24), B_scale=E[:, :1].contiguous()),
                 lambda: o.spmm(v, _z4(o.N, 24), X_scale=E[:, :1].contiguous(), **half),
                 lambda: o.spmm(v, _z4(o.N + 1, K // 2), X_scale=torch.cat([E, E[:1]]), **half),
                 lambda: o.spmm(v, B4b, X_scale=E.repeat(2, 1, 1), **half),
                 lambda: o.sddmm(A.half(), B4.clone().requires_grad_(True), B_scale=E),
                 lambda: o.spmm(v, B4.clone().requires_grad_(True), X_scale=E, **half),
                 lambda: o.attention(A.half(), B.half(), B4.clone().requires_grad_(True), V_scale=E)):
        with pytest.raises(ValueError):
            call()
    # and the good ones pass, in both scale dtypes and batched, beside fp8 and 16-bit partners
    e8 = E.view(torch.float8_e8m0fnu)
    assert o.sddmm(A.half(), B4, B_scale=e8).dtype == torch.float32
    assert o.spmm(v, B4, X_scale=e8, **half).dtype == torch.float16
    assert o.spmm(torch.zeros(2, o.nnz, device=_dev()), B4b, X_scale=E.repeat(2, 1, 1), **half).shape == (2, o.M, K)
    assert o.attention(A.bfloat16(), B4, B4, Kt_scale=E, V_scale=e8, fused=True).dtype == torch.bfloat16
    B8 = torch.zeros(o.N, K).to(E4M3).to(_dev())
    assert o.attention(A.bfloat16(), B8, B4, V_scale=E).dtype == torch.bfloat16            # an unscaled fp8 Kt, an fp4 V
    assert o.attention(A.half(), B4, B8, Kt_scale=E, V_scale=E, out_dtype=torch.float16).dtype == torch.float16
    assert o.attention(A.half(), B4, B.half(), Kt_scale=E).dtype == torch.float16
    torch.cuda.synchronize()


def test_a_blocked_operator_takes_the_gather_for_fp4(engine):
    """blocked=True and blocked=False agree bit for bit on an fp4 X / V: the blocked SpMM has no fp4 form"""
    import bsmr_torch
    M, N, ro, ci = bt.blocked_pattern()
    csr = engine.CSR.from_arrays(M, N, ro, ci)
    blocked = bsmr_torch.SparseOperator(csr, device=0, blocked=True)
    plain = bsmr_torch.SparseOperator(csr, device=0)
    assert engine.backward_blocked_stats(blocked._bw)["blocks"] > 0
    rng = np.random.default_rng(560)
    mode, Kv = 0, 96
    v = _t(rng.uniform(-1, 1, plain.nnz))
    tQ, _ = _t16(mode, rng.uniform(-1, 1, (M, K)))
    tK, tKs = _quantized(rng.uniform(-1, 1, (N, K)))
    tV, tVs = _quantized(rng.uniform(-1, 1, (N, Kv)))
    for call in (lambda op: op.spmm(v, tV, out_dtype=DT[mode], X_scale=tVs),
                 lambda op: op.softmax_spmm(v, tV, 0.5, out_dtype=DT[mode], X_scale=tVs),
                 lambda op: op.attention(tQ, tK, tV, Kt_scale=tKs, V_scale=tVs),
                 lambda op: op.attention(tQ, tK, tV, fused=True, Kt_scale=tKs, V_scale=tVs)):
        assert _bits(call(blocked)) == _bits(call(plain))
    q1, q2 = (tQ.detach().clone().requires_grad_(True) for _ in range(2))    # dA of an fp4-B sddmm: the gather too
    blocked.sddmm(q1, tK, B_scale=tKs).backward(v)
    plain.sddmm(q2, tK, B_scale=tKs).backward(v)
    assert _bits(q1.grad) == _bits(q2.grad)
    # not vacuous: the scales reach the result
    ones = torch.full_like(tVs, 127)
    assert _bits(plain.spmm(v, tV, out_dtype=DT[mode], X_scale=tVs)) != _bits(plain.spmm(v, tV, out_dtype=DT[mode], X_scale=ones))
