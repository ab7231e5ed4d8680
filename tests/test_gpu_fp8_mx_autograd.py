"""bsmr_torch.SparseOperator with MX block scales on its fp8 operands (B_scale, X_scale, Kt_scale, V_scale): sddmm, spmm,
softmax_spmm and attention, composed and fused, with Kt_scale only, V_scale only and both.

With dq = mx_dequantize(codes, scales) - one fp32 multiplication per element - the checks are those of
tests/test_gpu_fp8_autograd.py with dq in the place of the widened tensor, with their numbers and no others:
  * every scaled call gives the bits of the raw _mx calls it is documented to be, forward and backward;
  * with every scale code 127 it gives the bits of the same SparseOperator call without scales;
  * 16-bit results and gradients are oracle.round_array(format, gather twin) on dq, bit for bit;
  * products of integers under power-of-two block scales are the exact fp64 dot products;
  * the forward of attention stays within 2 u16 max_row |V| of dense fp64 attention, and the gradient into `values` of
    softmax_spmm inside the bound of DESIGN.md 13 (_fp64_rows), both taken on the dequantised tensors: V is dq itself, Kt is
    narrow(dq), the 16-bit copy the SDDMM is documented to run on (dq itself in bf16).
Then: every ValueError of the interface, a blocked=True operator against the unblocked one, and tensors made by mx_quantize
all the way through."""
import numpy as np
import pytest

import blocked_twin as bt
from gather_twin import assert_twin
from test_gpu_attention_fused_autograd import _fp64_rows, op16  # noqa: F401  (op16: that module's fixture)
from test_gpu_fp8_autograd import COMBOS, F8, _ints, _same, _t8, _z8
from test_gpu_io16_autograd import DT, U16, _bits, _np, _operands, _rounded, _t, _t16, _wide

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 64


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _scales(shape, lo, hi, salt=0, e8m0=False):
    """scale codes in [lo, hi] that differ between neighbouring batches, rows and blocks -> device tensor (uint8 or
    float8_e8m0fnu: the two dtypes the interface takes)"""
    idx = np.indices(shape)
    steps = (3, 7, 5)[:len(shape)][::-1]
    t = torch.from_numpy((lo + (sum(int(k) * i for k, i in zip(steps, idx)) + salt) % (hi - lo + 1)).astype(np.uint8))
    return (t.view(torch.float8_e8m0fnu) if e8m0 else t).to(_dev())


def _dq(t8, ts):
    """the dequantised tensor as fp32 numpy: torch on the CPU, codes.float() * e8m0.float()"""
    s = ts.cpu().view(torch.float8_e8m0fnu).float().repeat_interleave(32, dim=-1)
    return (t8.cpu().float() * s).numpy()


def _narrow(mode, x32):
    """narrow(dq) as (device 16-bit tensor, its widening as numpy)"""
    c = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(DT[mode])
    return c.to(_dev()), c.float().numpy()


def _ones(ts):
    return torch.full(ts.shape, 127, dtype=torch.uint8, device=_dev())


def _quantized(fmt, x):
    """(codes, scales) of an fp32 array through mx_quantize, on the device"""
    import bsmr_torch
    c, s = bsmr_torch.mx_quantize(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), F8[fmt])
    return c.to(_dev()), s.to(_dev())


@pytest.mark.parametrize("batch", (None, 2))
@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_sddmm_is_exact_and_da_equals_the_rounded_twin(engine, oracle, op16, mode, fmt, batch):
    o = op16
    rng = np.random.default_rng(220 + 4 * mode + 2 * fmt + bool(batch))
    lead = () if batch is None else (batch,)
    tA, A = _t16(mode, _ints(rng, *lead, o.M, K), grad=True)
    tB, _ = _t8(fmt, _ints(rng, *lead, o.N, K))
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
    assert_twin(_np(tA.grad), _rounded(oracle, mode, o.rl, G, B), f"dA mode={mode} fmt={fmt}")
    # the raw calls
    nb, e8 = batch or 1, tE.view(torch.uint8)
    rawP = torch.full_like(P, float("nan"))
    rawdA = torch.full_like(tA.grad, float("nan"))
    engine.sddmm_b8_mx(o._plan, K, tA.data_ptr(), tB.data_ptr(), e8.data_ptr(), rawP.data_ptr(), nb, mode, fmt, _stream())
    tG = _t(G)
    engine.spmm_x8_mx(o._bw, K, False, tG.data_ptr(), tB.data_ptr(), e8.data_ptr(), rawdA.data_ptr(), nb, _stream(),
                      mode=mode, fmt=fmt)
    torch.cuda.synchronize()
    assert _same(P, rawP) and _bits(tA.grad) == _bits(rawdA)
    assert _same(P, o.sddmm(tA.detach(), _narrow(mode, B)[0]))               # the 16-bit call on narrow(dq)
    # scale code 127 everywhere: the call without scales
    a1, a2 = (tA.detach().clone().requires_grad_(True) for _ in range(2))
    P1, P2 = o.sddmm(a1, tB, B_scale=_ones(tE)), o.sddmm(a2, tB)
    P1.backward(_t(G))
    P2.backward(_t(G))
    assert _same(P1, P2) and _bits(a1.grad) == _bits(a2.grad)


@pytest.mark.parametrize("batch", (None, 2))
@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_spmm_equals_the_rounded_twin_and_dvalues_is_exact(engine, oracle, op16, mode, fmt, batch):
    o = op16
    rng = np.random.default_rng(240 + 4 * mode + 2 * fmt + bool(batch))
    lead = () if batch is None else (batch,)
    v = _wide(rng, lead + (o.nnz,), -3, 3)
    tv = _t(v, grad=True)
    tX, _ = _t8(fmt, _ints(rng, *lead, o.N, K))
    tE = _scales(lead + (o.N, K // 32), 125, 130, salt=1, e8m0=not batch)
    X = _dq(tX, tE)
    tH, H = _t16(mode, _ints(rng, *lead, o.M, K))
    Y = o.spmm(tv, tX, out_dtype=DT[mode], X_scale=tE)
    assert Y.dtype == DT[mode] and Y.shape == lead + (o.M, K)
    assert_twin(_np(Y), _rounded(oracle, mode, o.rl, v, X), f"spmm mode={mode} fmt={fmt}")
    assert _bits(Y) == _bits(o.spmm(tv.detach(), _narrow(mode, X)[0]))       # exact copy: the 16-bit call, the same bits
    Y.backward(tH)
    row_of = np.repeat(np.arange(o.M), np.diff(o.ro))
    exact = np.einsum("...tk,...tk->...t", H[..., row_of, :].astype(np.float64), X[..., o.ci, :].astype(np.float64))
    assert tv.grad.dtype == torch.float32 and np.array_equal(_np(tv.grad).astype(np.float64), exact)
    nb, e8 = batch or 1, tE.view(torch.uint8)
    rawY, rawdv = torch.full_like(Y, float("nan")), torch.full_like(tv.grad, float("nan"))
    engine.spmm_x8_mx(o._bw, K, False, tv.data_ptr(), tX.data_ptr(), e8.data_ptr(), rawY.data_ptr(), nb, _stream(),
                      mode=mode, fmt=fmt)
    engine.sddmm_b8_mx(o._plan, K, tH.data_ptr(), tX.data_ptr(), e8.data_ptr(), rawdv.data_ptr(), nb, mode, fmt, _stream())
    torch.cuda.synchronize()
    assert _bits(Y) == _bits(rawY) and _same(tv.grad, rawdv)
    v1, v2 = _t(v, grad=True), _t(v, grad=True)
    Y1, Y2 = o.spmm(v1, tX, out_dtype=DT[mode], X_scale=_ones(tE)), o.spmm(v2, tX, out_dtype=DT[mode])
    Y1.backward(tH)
    Y2.backward(tH)
    assert _bits(Y1) == _bits(Y2) and _same(v1.grad, v2.grad)


@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_softmax_spmm_trains_values_on_a_quantized_v(engine, op16, mode, fmt):
    """V goes through mx_quantize; the bounds are taken on dq(V)"""
    o = op16
    rng = np.random.default_rng(260 + 2 * mode + fmt)
    _, _, V, H = _operands(mode, rng, o)
    scale = K ** -0.5
    scores = rng.uniform(-8, 8, o.nnz).astype(np.float32)
    tV, tE = _quantized(fmt, V)
    wV = _dq(tV, tE)
    assert np.abs(wV - V).max() <= 2.0 ** -(2 if fmt else 3) * np.abs(V).max()            # the round trip is a quantisation
    tH, wH = _t16(mode, H)
    P = _t(scores, grad=True)
    O = o.softmax_spmm(P, tV, scale, out_dtype=DT[mode], X_scale=tE)
    O.backward(tH)
    assert O.dtype == DT[mode] and P.grad.dtype == torch.float32
    # the raw calls, forward and backward
    Or, m, s = o._attention_x8(P.detach(), tV, scale, DT[mode], tE)
    rO, rm, rs = (torch.full_like(t, float("nan")) for t in (Or, m, s))
    engine.sparse_attention_x8_mx(o._bw, K, scale, P.data_ptr(), tV.data_ptr(), tE.data_ptr(), rO.data_ptr(), rm.data_ptr(),
                                  rs.data_ptr(), 1, _stream(), mode=mode, fmt=fmt)
    dWr = torch.full((o.nnz,), float("nan"), device=_dev())
    engine.sddmm_b8_mx(o._plan, K, tH.data_ptr(), tV.data_ptr(), tE.data_ptr(), dWr.data_ptr(), 1, mode, fmt, _stream())
    torch.cuda.synchronize()
    assert _bits(O) == _bits(rO) and _same(m, rm) and _same(s, rs)
    dPr, _ = o._attention_backward(P.detach(), rm, rs, dWr.clone(), rO, tH, scale)     # (it writes dP over its dW)
    assert _same(P.grad, dPr)
    # the fp32 call on dq: O rounded once, m and s in bits
    O32, m32, s32 = o._attention(P.detach(), _t(wV), scale)
    assert _bits(O) == _bits(O32.to(DT[mode])) and _same(m, m32) and _same(s, s32)
    # scale code 127 everywhere: the call without scales
    P1, P2 = _t(scores, grad=True), _t(scores, grad=True)
    O1 = o.softmax_spmm(P1, tV, scale, out_dtype=DT[mode], X_scale=_ones(tE))
    O2 = o.softmax_spmm(P2, tV, scale, out_dtype=DT[mode])
    O1.backward(tH)
    O2.backward(tH)
    assert _bits(O1) == _bits(O2) and _same(P1.grad, P2.grad)
    # fp64 on dq(V): the forward within one output rounding, dP inside its bound (dW as the device made it)
    O64, dP64, b16, b32 = _fp64_rows(o, scores, scale, wV, wH, _np(dWr).astype(np.float64))
    vmax = np.maximum.reduceat(np.abs(wV.astype(np.float64))[o.ci], o.ro[:-1], axis=0)
    err = np.abs(_np(O).astype(np.float64) - O64)
    print(f"mode={mode} fmt={fmt}: worst |O - O64| / bound = {(err / (2 * U16[mode] * vmax)).max():.3f}")
    assert (err <= 2 * U16[mode] * vmax).all()
    err = np.abs(_np(P.grad).astype(np.float64) - dP64)
    bound = U16[mode] * b16 + b32
    print(f"mode={mode} fmt={fmt}: worst |dP - dP64| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("which", ("kt", "v", "both"))
@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_attention_composed_and_fused(engine, oracle, op16, mode, fmt, which):
    """Kt and V through mx_quantize; the one left without a scale stays a 16-bit tensor"""
    o = op16
    rng = np.random.default_rng(280 + 2 * mode + fmt)
    Q, Kt, V, H = _operands(mode, rng, o)
    scale = K ** -0.5
    tH, wH = _t16(mode, H)
    kkw, vkw = {}, {}
    if which in ("kt", "both"):
        tK, tKs = _quantized(fmt, Kt)
        dqK = _dq(tK, tKs)
        wK = _narrow(mode, dqK)[1]                                           # what the SDDMM runs on
        kkw = dict(Kt_scale=tKs)
    else:
        tK, wK = _t16(mode, Kt)
        dqK = wK
    if which in ("v", "both"):
        tV, tVs = _quantized(fmt, V)
        wV = _dq(tV, tVs)
        vkw = dict(V_scale=tVs)
        okw = dict(out_dtype=DT[mode])
    else:
        (tV, wV), okw = _t16(mode, V), {}

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
    assert_twin(_np(O), _rounded(oracle, mode, o.rl, _np(W), wV), f"O mode={mode} fmt={fmt} {which}")
    assert_twin(_np(dQ), _rounded(oracle, mode, o.rl, _np(P.grad), dqK), f"Q.grad mode={mode} fmt={fmt} {which}")
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
    # scale code 127 everywhere: the calls without scales
    ones = {k: _ones(t) for k, t in {**kkw, **vkw}.items()}
    for fused in (False, True):
        w1 = run(lambda tQ: o.attention(tQ, tK, tV, fused=fused, **ones))
        w2 = run(lambda tQ: o.attention(tQ, tK, tV, fused=fused))
        assert _bits(w1[0]) == _bits(w2[0]) and _bits(w1[1]) == _bits(w2[1]), (which, fused)


def test_every_value_error(engine, op16):
    o = op16
    A, B = torch.zeros(o.M, K, device=_dev()), torch.zeros(o.N, K, device=_dev())
    v = torch.zeros(o.nnz, device=_dev())
    E = torch.full((o.N, K // 32), 127, dtype=torch.uint8, device=_dev())
    half = dict(out_dtype=torch.float16)
    for f8 in F8.values():
        B8 = _z8(f8, o.N, K)
        B8b = _z8(f8, 2, o.N, K)
        # a scale without an fp8 operand
        for X in (B, B.half(), B.bfloat16()):
            for call in (lambda: o.sddmm(A.to(X.dtype), X, B_scale=E), lambda: o.spmm(v, X, X_scale=E),
                         lambda: o.softmax_spmm(v, X, 1.0, X_scale=E), lambda: o.attention(A.to(X.dtype), X, X, Kt_scale=E),
                         lambda: o.attention(A.to(X.dtype), X, X, V_scale=E),
                         lambda: o.attention(A.half(), B8, X.half(), Kt_scale=E, V_scale=E),
                         lambda: o.attention(A.half(), X.half(), B8, Kt_scale=E, V_scale=E)):
                with pytest.raises(ValueError):
                    call()
        with pytest.raises(ValueError):
            o.spmm(v, A.half(), transpose=True, X_scale=torch.full((o.M, K // 32), 127, dtype=torch.uint8, device=_dev()))
        # dtype, shape, batch, device, layout, grad, type
        bad = (E.float(), E.to(torch.int8), E.half(), E[:, :1].contiguous(), E[:-1].contiguous(), E.reshape(-1),
               E.unsqueeze(0), E.repeat(2, 1, 1), E.cpu(), E.repeat(1, 2)[:, ::2], E.t().contiguous().t(),
               E.float().requires_grad_(True), E.cpu().numpy(), 127)
        try:                                                                 # a scale that asks for a gradient, where torch
            bad += (E.view(torch.float8_e8m0fnu).requires_grad_(True),)      # lets an e8m0 tensor ask for one
        except RuntimeError:
            pass
        for sc in bad:
            for call in (lambda: o.sddmm(A.half(), B8, B_scale=sc), lambda: o.spmm(v, B8, X_scale=sc, **half),
                         lambda: o.softmax_spmm(v, B8, 1.0, X_scale=sc, **half),
                         lambda: o.attention(A.half(), B8, B.half(), Kt_scale=sc),
                         lambda: o.attention(A.half(), B.half(), B8, V_scale=sc),
                         lambda: o.attention(A.half(), B8, B8, Kt_scale=E, V_scale=sc, fused=True)):
                with pytest.raises(ValueError):
                    call()
        with pytest.raises(ValueError):
            o.spmm(torch.zeros(2, o.nnz, device=_dev()), B8b, X_scale=E, **half)           # an unbatched scale, a batched X
        with pytest.raises(ValueError):
            o.sddmm(A.half(), B8, B_scale=E.repeat(2, 1, 1))                               # and the other way round
        # the rules of the unscaled call still hold beside a good scale
        for kw in (dict(), dict(out_dtype=torch.float32), dict(out_dtype=torch.float16, transpose=True)):
            with pytest.raises(ValueError):
                o.spmm(v, B8, X_scale=E, **kw)
        with pytest.raises(ValueError):
            o.sddmm(A, B8, B_scale=E)                                                      # an fp32 A beside an fp8 B
        g8 = _z8(f8, o.N, K).requires_grad_(True)
        with pytest.raises(ValueError):
            o.sddmm(A.half(), g8, B_scale=E)
        # and the good ones pass, in both scale dtypes and batched
        e8 = E.view(torch.float8_e8m0fnu)
        assert o.sddmm(A.half(), B8, B_scale=e8).dtype == torch.float32
        assert o.spmm(v, B8, X_scale=e8, **half).dtype == torch.float16
        assert o.spmm(torch.zeros(2, o.nnz, device=_dev()), B8b, X_scale=E.repeat(2, 1, 1), **half).shape == (2, o.M, K)
        assert o.attention(A.bfloat16(), B8, B8, Kt_scale=E, V_scale=e8, fused=True).dtype == torch.bfloat16
    torch.cuda.synchronize()


def test_a_blocked_operator_takes_the_gather_for_scaled_fp8(engine):
    """blocked=True and blocked=False agree bit for bit on a scaled fp8 X / V, as they do on an unscaled one"""
    import bsmr_torch
    M, N, ro, ci = bt.blocked_pattern()
    csr = engine.CSR.from_arrays(M, N, ro, ci)
    blocked = bsmr_torch.SparseOperator(csr, device=0, blocked=True)
    plain = bsmr_torch.SparseOperator(csr, device=0)
    assert engine.backward_blocked_stats(blocked._bw)["blocks"] > 0
    rng = np.random.default_rng(360)
    mode, fmt, Kv = 0, 0, 96
    v = _t(rng.uniform(-1, 1, plain.nnz))
    tQ, _ = _t16(mode, rng.uniform(-1, 1, (M, K)))
    tK, tKs = _quantized(fmt, rng.uniform(-1, 1, (N, K)))
    tV, tVs = _quantized(fmt, rng.uniform(-1, 1, (N, Kv)))
    for call in (lambda op: op.spmm(v, tV, out_dtype=DT[mode], X_scale=tVs),
                 lambda op: op.softmax_spmm(v, tV, 0.5, out_dtype=DT[mode], X_scale=tVs),
                 lambda op: op.attention(tQ, tK, tV, Kt_scale=tKs, V_scale=tVs),
                 lambda op: op.attention(tQ, tK, tV, fused=True, Kt_scale=tKs, V_scale=tVs)):
        assert _bits(call(blocked)) == _bits(call(plain))
    q1, q2 = (tQ.detach().clone().requires_grad_(True) for _ in range(2))    # dA of a scaled fp8-B sddmm: the gather too
    blocked.sddmm(q1, tK, B_scale=tKs).backward(v)
    plain.sddmm(q2, tK, B_scale=tKs).backward(v)
    assert _bits(q1.grad) == _bits(q2.grad)
    # not vacuous: the scales reach the result
    assert _bits(plain.spmm(v, tV, out_dtype=DT[mode], X_scale=tVs)) != _bits(plain.spmm(v, tV, out_dtype=DT[mode]))


@pytest.mark.parametrize("fmt", (0, 1))
def test_a_wide_range_tensor_survives_the_round_trip(engine, oracle, op16, fmt):
    """rows of V at very different magnitudes (2^-20 .. 2^20 between blocks): unscaled fp8 cannot hold them (e4m3 saturates
    or flushes), mx_quantize keeps three / two mantissa bits per block, and spmm on (codes, scales) is the rounded twin of
    the dequantised tensor - within one quantisation step of spmm on the original"""
    import bsmr_torch
    o, mode = op16, 1
    rng = np.random.default_rng(380 + fmt)
    mag = np.exp2(rng.integers(-20, 21, (o.N, K // 32))).repeat(32, axis=1)
    V = (rng.uniform(-1, 1, (o.N, K)) * mag).astype(np.float32)
    tV, tVs = _quantized(fmt, V)
    wV = _dq(tV, tVs)
    assert np.array_equal(wV, bsmr_torch.mx_dequantize(tV.cpu(), tVs.cpu()).numpy())
    step = 2.0 ** -(2 if fmt else 3)
    assert (np.abs(wV - V) <= step * mag).all() and len(np.unique(tVs.cpu().numpy())) > 20
    v = rng.uniform(0, 1, o.nnz).astype(np.float32)
    Y = o.spmm(_t(v), tV, out_dtype=DT[mode], X_scale=tVs)
    assert_twin(_np(Y), _rounded(oracle, mode, o.rl, v, wV), f"fmt={fmt}")
    assert _bits(Y) == _bits(o.spmm(_t(v), _t(wV)).to(DT[mode]))             # the fp32 call on dq, rounded once
