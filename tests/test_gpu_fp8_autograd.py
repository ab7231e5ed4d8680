"""bsmr_torch.SparseOperator with fp8 keys and values (torch.float8_e4m3fn / torch.float8_e5m2 on the column side):
sddmm, spmm, softmax_spmm and attention, composed and fused, with Kt fp8 only, V fp8 only and both.

The arithmetic is that of the 16-bit tensors of tests/test_gpu_io16_autograd.py and test_gpu_attention_fused_autograd.py
on the exactly widened operand, so the checks are theirs, with their numbers and no others:
  * 16-bit results and gradients are oracle.round_array(format, gather twin) on the widened fp8 tensor, bit for bit;
  * products of integers are the exact fp64 dot products;
  * the forward of attention stays within 2 u16 max_row |V| of dense fp64 attention on the widened tensors;
  * the gradient into `values` of softmax_spmm stays inside the bound of DESIGN.md 13 (_fp64_rows);
  * every fp8 call gives the bits of the same call on the widened 16-bit tensor.
Then: every ValueError of the interface, one spot check that calls without fp8 tensors run what they ran before, and a
blocked=True operator against the unblocked one."""
import numpy as np
import pytest

import blocked_twin as bt
from gather_twin import assert_twin
from test_gpu_attention_fused_autograd import _fp64_rows, op16  # noqa: F401  (op16: that module's fixture)
from test_gpu_io16_autograd import DT, U16, _bits, _np, _operands, _rounded, _t, _t16, _wide

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 64
F8 = {0: torch.float8_e4m3fn, 1: torch.float8_e5m2}
COMBOS = [(mode, fmt) for mode in (0, 1) for fmt in (0, 1)]


def _dev():
    return torch.device("cuda:0")


def _t8(fmt, a):
    """fp32 array -> (device tensor of the fp8 dtype, cast on the CPU; its exact widening as numpy)"""
    c = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(F8[fmt])
    return c.to(_dev()), c.to(torch.float32).numpy()


def _as16(mode, t8):
    """the exactly widened 16-bit copy of an fp8 device tensor"""
    return t8.cpu().to(torch.float32).to(DT[mode]).to(_dev())


def _z8(f8, *shape):
    return torch.zeros(*shape).to(f8).to(_dev())                             # (cast on the CPU)


def _ints(rng, *shape):
    return rng.integers(-8, 9, size=shape).astype(np.float32)                # exact in e4m3, e5m2, fp16 and bf16


def _same(a, b):
    return a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("batch", (None, 2))
@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_sddmm_is_exact_and_da_equals_the_rounded_twin(engine, oracle, op16, mode, fmt, batch):
    o = op16
    rng = np.random.default_rng(20 + 4 * mode + 2 * fmt + bool(batch))
    lead = () if batch is None else (batch,)
    tA, A = _t16(mode, _ints(rng, *lead, o.M, K), grad=True)
    tB, B = _t8(fmt, _ints(rng, *lead, o.N, K))
    G = _wide(rng, lead + (o.nnz,), -3, 3)
    P = o.sddmm(tA, tB)
    assert P.dtype == torch.float32 and P.shape == lead + (o.nnz,)
    row_of = np.repeat(np.arange(o.M), np.diff(o.ro))
    exact = np.einsum("...tk,...tk->...t", A[..., row_of, :].astype(np.float64), B[..., o.ci, :].astype(np.float64))
    assert np.array_equal(_np(P).astype(np.float64), exact)
    P.backward(_t(G))
    assert tA.grad.dtype == DT[mode] and tB.grad is None
    assert_twin(_np(tA.grad), _rounded(oracle, mode, o.rl, G, B), f"dA mode={mode} fmt={fmt}")
    assert _same(P, o.sddmm(tA.detach(), _as16(mode, tB)))                   # the 16-bit call on the widened B


@pytest.mark.parametrize("batch", (None, 2))
@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_spmm_equals_the_rounded_twin_and_dvalues_is_exact(engine, oracle, op16, mode, fmt, batch):
    o = op16
    rng = np.random.default_rng(40 + 4 * mode + 2 * fmt + bool(batch))
    lead = () if batch is None else (batch,)
    v = _wide(rng, lead + (o.nnz,), -3, 3)
    tv = _t(v, grad=True)
    tX, X = _t8(fmt, _ints(rng, *lead, o.N, K))
    tH, H = _t16(mode, _ints(rng, *lead, o.M, K))
    Y = o.spmm(tv, tX, out_dtype=DT[mode])
    assert Y.dtype == DT[mode] and Y.shape == lead + (o.M, K)
    assert_twin(_np(Y), _rounded(oracle, mode, o.rl, v, X), f"spmm mode={mode} fmt={fmt}")
    assert _bits(Y) == _bits(o.spmm(tv.detach(), _as16(mode, tX)))
    Y.backward(tH)
    row_of = np.repeat(np.arange(o.M), np.diff(o.ro))
    exact = np.einsum("...tk,...tk->...t", H[..., row_of, :].astype(np.float64), X[..., o.ci, :].astype(np.float64))
    assert tv.grad.dtype == torch.float32 and np.array_equal(_np(tv.grad).astype(np.float64), exact)


@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_softmax_spmm_trains_values(engine, op16, mode, fmt):
    o = op16
    rng = np.random.default_rng(60 + 2 * mode + fmt)
    _, _, V, H = _operands(mode, rng, o)
    scale = K ** -0.5
    scores = rng.uniform(-8, 8, o.nnz).astype(np.float32)
    tV, wV = _t8(fmt, V)
    tH, wH = _t16(mode, H)
    P = _t(scores, grad=True)
    O = o.softmax_spmm(P, tV, scale, out_dtype=DT[mode])
    O.backward(tH)
    assert O.dtype == DT[mode] and P.grad.dtype == torch.float32
    # the 16-bit call on the widened V: the same bits, forward and backward
    P16 = _t(scores, grad=True)
    O16 = o.softmax_spmm(P16, _as16(mode, tV), scale)
    O16.backward(tH)
    assert _bits(O) == _bits(O16) and _same(P.grad, P16.grad)
    # fp64 on the widened V: the forward within one output rounding, dP inside its bound
    dW = _np(o._sddmm(tH, _as16(mode, tV))).astype(np.float64)
    O64, dP64, b16, b32 = _fp64_rows(o, scores, scale, wV, wH, dW)
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
    o = op16
    rng = np.random.default_rng(80 + 2 * mode + fmt)
    Q, Kt, V, H = _operands(mode, rng, o)
    scale = K ** -0.5
    tH, wH = _t16(mode, H)
    tK, wK = _t8(fmt, Kt) if which in ("kt", "both") else _t16(mode, Kt)
    tV, wV = _t8(fmt, V) if which in ("v", "both") else _t16(mode, V)
    kw = dict(out_dtype=DT[mode]) if which in ("v", "both") else {}

    def run(how):
        tQ, wQ = _t16(mode, Q, grad=True)
        out = how(tQ)
        O = out[0] if isinstance(out, tuple) else out
        O.backward(tH)
        return (O, tQ.grad, wQ) + (out[1:] if isinstance(out, tuple) else ())

    # composed, written out with P and W kept: the twins of tests/test_gpu_io16_autograd.py on the widened tensors
    def by_hand(tQ):
        P = o.sddmm(tQ, tK)
        W = o.softmax(P, scale)
        P.retain_grad()
        return o.spmm(W, tV, **kw), P, W
    O, dQ, wQ, P, W = run(by_hand)
    assert O.dtype == DT[mode] and dQ.dtype == DT[mode] and P.dtype == torch.float32
    assert_twin(_np(O), _rounded(oracle, mode, o.rl, _np(W), wV), f"O mode={mode} fmt={fmt} {which}")
    assert_twin(_np(dQ), _rounded(oracle, mode, o.rl, _np(P.grad), wK), f"Q.grad mode={mode} fmt={fmt} {which}")
    # dense fp64 attention on the widened tensors
    mask = np.zeros((o.M, o.N), dtype=bool)
    mask[np.repeat(np.arange(o.M), np.diff(o.ro)), o.ci] = True
    Z = np.where(mask, (wQ.astype(np.float64) @ wK.astype(np.float64).T) * scale, -np.inf)
    E = np.exp(Z - Z.max(axis=1, keepdims=True))
    O64 = (E / E.sum(axis=1, keepdims=True)) @ wV.astype(np.float64)
    bound = 2 * U16[mode] * np.maximum.reduceat(np.abs(wV.astype(np.float64))[o.ci], o.ro[:-1], axis=0)
    assert (np.abs(_np(O).astype(np.float64) - O64) <= bound).all()
    # op.attention is that composition; the fused path is softmax_spmm written out; both repeat on the widened tensors
    a = run(lambda tQ: o.attention(tQ, tK, tV))
    assert _bits(a[0]) == _bits(O) and _bits(a[1]) == _bits(dQ)
    f = run(lambda tQ: o.attention(tQ, tK, tV, fused=True))
    g = run(lambda tQ: o.softmax_spmm(o.sddmm(tQ, tK), tV, scale, **kw))
    assert f[0].dtype == DT[mode] and _bits(f[0]) == _bits(g[0]) and _bits(f[1]) == _bits(g[1])
    assert (np.abs(_np(f[0]).astype(np.float64) - O64) <= bound).all()
    assert np.isfinite(_np(f[1])).all() and np.abs(_np(f[1])).max() > 0
    k16 = _as16(mode, tK) if tK.dtype in F8.values() else tK
    v16 = _as16(mode, tV) if tV.dtype in F8.values() else tV
    for fused, want in ((False, a), (True, f)):
        w = run(lambda tQ: o.attention(tQ, k16, v16, fused=fused))
        assert _bits(w[0]) == _bits(want[0]) and _bits(w[1]) == _bits(want[1]), (which, fused)


def test_out_dtype_of_attention_defaults_to_q(engine, op16):
    o = op16
    Q = torch.zeros(o.M, K, device=_dev(), dtype=torch.bfloat16)
    Kt = torch.zeros(o.N, K, device=_dev(), dtype=torch.bfloat16)
    V8 = _z8(torch.float8_e5m2, o.N, K)
    assert o.attention(Q, Kt, V8).dtype == torch.bfloat16 and o.attention(Q, Kt, V8, fused=True).dtype == torch.bfloat16
    assert o.attention(Q, Kt, V8, out_dtype=torch.float16).dtype == torch.float16
    assert o.attention(Q, Kt, Kt, out_dtype=torch.float16).dtype == torch.bfloat16       # unused without an fp8 V


def test_every_value_error(engine, op16):
    o = op16
    A, B = torch.zeros(o.M, K, device=_dev()), torch.zeros(o.N, K, device=_dev())
    v = torch.zeros(o.nnz, device=_dev())
    for f8 in F8.values():
        A8, B8 = _z8(f8, o.M, K), _z8(f8, o.N, K)
        for a, b in ((A8, B.half()), (A8, B8), (A8, B), (A, B8), (A.double(), B8)):
            with pytest.raises(ValueError):
                o.sddmm(a, b)                                                # fp8 A; fp32 (or fp64) A beside an fp8 B
        for kw in (dict(), dict(out_dtype=torch.float32), dict(out_dtype=f8), dict(out_dtype="half"),
                   dict(out_dtype=torch.float16, transpose=True)):
            with pytest.raises(ValueError):
                o.spmm(v, B8, **kw)                                          # a missing or impossible out_dtype; transpose
        with pytest.raises(ValueError):
            o.spmm(v, A8, transpose=True)
        for kw in (dict(), dict(out_dtype=torch.float32)):
            with pytest.raises(ValueError):
                o.softmax_spmm(v, B8, 1.0, **kw)
        with pytest.raises(ValueError):
            o.attention(A, B, B8)                                            # out_dtype defaults to Q's float32
        g8 = _z8(f8, o.N, K).requires_grad_(True)                            # no gradient into an fp8 tensor
        for call in (lambda: o.sddmm(A.half(), g8), lambda: o.spmm(v, g8, out_dtype=torch.float16),
                     lambda: o.softmax_spmm(v, g8, 1.0, out_dtype=torch.float16),
                     lambda: o.attention(A.half(), g8, B.half()), lambda: o.attention(A.half(), B.half(), g8)):
            with pytest.raises(ValueError):
                call()
        for x in (_z8(f8, o.N, 48), A8, B8.cpu(), _z8(f8, o.N, 2 * K)[:, :K]):
            with pytest.raises(ValueError):
                o.spmm(v, x, out_dtype=torch.float16)                        # K, rows, device, layout
        with pytest.raises(ValueError):
            o.spmm(v.half(), B8, out_dtype=torch.float16)                    # values stay fp32
    for X in (B, B.half(), B.bfloat16()):                                    # a superfluous out_dtype
        with pytest.raises(ValueError):
            o.spmm(v, X, out_dtype=torch.float16)
        with pytest.raises(ValueError):
            o.softmax_spmm(v, X, 1.0, out_dtype=X.dtype)
    assert o.spmm(v, _z8(torch.float8_e4m3fn, o.N, K), out_dtype=torch.float16).dtype == torch.float16
    assert o.sddmm(A.bfloat16(), _z8(torch.float8_e5m2, o.N, K)).dtype == torch.float32


def test_calls_without_fp8_tensors_run_what_they_ran(engine, op16):
    """one spot check in 16 bits: the operator's spmm, sddmm and both gradients are the raw 16-bit calls, bit for bit"""
    o, mode = op16, 1
    rng = np.random.default_rng(140)
    s = torch.cuda.current_stream(_dev()).cuda_stream
    tv = _t(_wide(rng, o.nnz, -3, 3), grad=True)
    tX, _ = _t16(mode, _wide(rng, (o.N, K)), grad=True)
    tA, _ = _t16(mode, _wide(rng, (o.M, K)), grad=True)
    tH, _ = _t16(mode, _wide(rng, (o.M, K)))
    raw = {k: torch.full((r, K), float("nan"), device=_dev(), dtype=DT[mode]) for k, r in (("Y", o.M), ("dX", o.N), ("dA", o.M), ("dB", o.N))}
    rawP = torch.full((o.nnz,), float("nan"), device=_dev())
    engine.spmm_16(o._bw, K, False, tv.data_ptr(), tX.data_ptr(), raw["Y"].data_ptr(), 1, s, mode=mode)
    engine.spmm_16(o._bw, K, True, tv.data_ptr(), tH.data_ptr(), raw["dX"].data_ptr(), 1, s, mode=mode)
    engine.sddmm_backward_16(o._bw, K, tv.data_ptr(), tA.data_ptr(), tX.data_ptr(), raw["dA"].data_ptr(), raw["dB"].data_ptr(), 1, s,
                             mode=mode)
    engine.sddmm_16(o._plan, K, tA.data_ptr(), tX.data_ptr(), rawP.data_ptr(), 1, mode, s)
    torch.cuda.synchronize()
    Y = o.spmm(tv, tX)
    Y.backward(tH)
    assert _bits(Y) == _bits(raw["Y"]) and _bits(tX.grad) == _bits(raw["dX"])
    tB = tX.detach().clone().requires_grad_(True)
    P = o.sddmm(tA, tB)
    P.backward(tv.detach())
    assert _same(P, rawP) and _bits(tA.grad) == _bits(raw["dA"]) and _bits(tB.grad) == _bits(raw["dB"])


def test_a_blocked_operator_takes_the_gather_for_fp8(engine):
    """blocked=True and blocked=False agree bit for bit on fp8 X / V (the blocked SpMM has no fp8 form), while the
    widened fp32 X on the same operators does take the blocks"""
    import bsmr_torch
    M, N, ro, ci = bt.blocked_pattern()
    csr = engine.CSR.from_arrays(M, N, ro, ci)
    blocked = bsmr_torch.SparseOperator(csr, device=0, blocked=True)
    plain = bsmr_torch.SparseOperator(csr, device=0)
    assert engine.backward_blocked_stats(blocked._bw)["blocks"] > 0
    rng = np.random.default_rng(160)
    mode, fmt, Kv = 0, 0, 96
    v = _t(rng.uniform(-1, 1, plain.nnz))
    tQ, _ = _t16(mode, rng.uniform(-1, 1, (M, K)))
    tK, _ = _t8(fmt, rng.uniform(-1, 1, (N, K)))
    tV, _ = _t8(fmt, rng.uniform(-1, 1, (N, Kv)))
    for call in (lambda op: op.spmm(v, tV, out_dtype=DT[mode]),
                 lambda op: op.softmax_spmm(v, tV, 0.5, out_dtype=DT[mode]),
                 lambda op: op.attention(tQ, tK, tV),
                 lambda op: op.attention(tQ, tK, tV, fused=True)):
        assert _bits(call(blocked)) == _bits(call(plain))
    q1, q2 = (tQ.detach().clone().requires_grad_(True) for _ in range(2))    # dA of an fp8-B sddmm: the gather too
    blocked.sddmm(q1, tK).backward(v)
    plain.sddmm(q2, tK).backward(v)
    assert _bits(q1.grad) == _bits(q2.grad)
    v32 = tV.cpu().to(torch.float32).to(_dev())
    assert not _same(blocked.spmm(v, v32), plain.spmm(v, v32))               # (not vacuous: the blocks do change fp32 bits)
