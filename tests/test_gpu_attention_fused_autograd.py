"""bsmr_torch.SparseOperator.softmax_spmm and attention(fused=True) as autograd functions on the engine:
  * the two-layer step of tests/test_gpu_softmax_autograd.py through the fused path, against dense masked fp64 torch with
    that file's tolerances, b = None and b = 2; a second run gives the same gradient bits;
  * softmax_spmm written out is attention(fused=True), bit for bit; the default path is unchanged: attention(Q, Kt, V),
    attention(..., fused=False) and the hand composition are bit-equal;
  * rows of S without entries give zero rows;
  * fp16 / bf16 operands: dtypes follow the operands, the forward stays within 2 u16 max_row |V| of fp64, dV / dQ / dK
    are the rounded gather twins of (W, dO) and (dP, Kt / Q) with W and dP from the raw calls and from P.retain_grad(),
    and dP stays inside the bound DESIGN.md 13 derives;
  * bad inputs raise ValueError."""
import numpy as np
import pytest

import synth
from gather_twin import assert_twin, col_lists, row_lists
from softmax_twin import U
from test_gpu_io16_autograd import DT, U16, _bits, _np, _operands, _rounded, _t16
from test_gpu_softmax_autograd import _leaves, _masked_softmax, _rand, op  # noqa: F401  (op: that module's fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 64


def _dev():
    return torch.device("cuda:0")


def _same(a, b):
    return a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes()


def _step(op, leaves, H, **kw):  # noqa: F811
    Q, Kk, V = leaves[0], leaves[1:3], leaves[3:5]
    x = Q
    for i in range(2):
        x = op.attention(x, Kk[i], V[i], **kw)
    (x * H).sum().backward()
    grads = [t.grad.detach().clone() for t in leaves]
    for t in leaves:
        t.grad = None
    return x.detach(), grads


@pytest.mark.parametrize("batch", [None, 2])
def test_two_layer_fused_attention_step(op, batch):  # noqa: F811
    leaves = _leaves(op, batch)
    lead = () if batch is None else (batch,)
    H = _rand(*lead, op.M, 96, seed=26, requires_grad=False)
    out, grads = _step(op, leaves, H, fused=True)

    ref = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    x = ref[0]
    for i in range(2):
        s = (x @ ref[1 + i].transpose(-1, -2)) * x.shape[-1] ** -0.5
        x = _masked_softmax(op, s) @ ref[3 + i]
    (x * H.double().cpu()).sum().backward()
    o, x = out.double().cpu(), x.detach()
    assert torch.allclose(o, x, rtol=1e-4, atol=1e-5 * float(x.abs().max())), float((o - x).abs().max())
    for got, want in zip(grads, ref):
        g, w = got.double().cpu(), want.grad
        assert torch.allclose(g, w, rtol=1e-4, atol=1e-5 * float(w.abs().max())), float((g - w).abs().max())

    out2, again = _step(op, leaves, H, fused=True)
    assert _same(out, out2)
    for a, b in zip(grads, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _one_layer(op, how, batch=None):  # noqa: F811
    lead = () if batch is None else (batch,)
    Q, Kt, V = _rand(*lead, op.M, 64, seed=41), _rand(*lead, op.N, 64, seed=42), _rand(*lead, op.N, 96, seed=43)
    H = _rand(*lead, op.M, 96, seed=44, requires_grad=False)
    O = how(Q, Kt, V)
    (O * H).sum().backward()
    return [O, Q.grad, Kt.grad, V.grad]


@pytest.mark.parametrize("batch", [None, 2])
def test_softmax_spmm_written_out_is_fused_attention(op, batch):  # noqa: F811
    a = _one_layer(op, lambda Q, Kt, V: op.attention(Q, Kt, V, fused=True), batch)
    b = _one_layer(op, lambda Q, Kt, V: op.softmax_spmm(op.sddmm(Q, Kt), V, 64 ** -0.5), batch)
    c = _one_layer(op, lambda Q, Kt, V: op.attention(Q, Kt, V, scale=0.125, fused=True), batch)
    for x, y, z in zip(a, b, c):
        assert _same(x, y) and _same(x, z)


def test_the_default_path_is_unchanged(op):  # noqa: F811
    a = _one_layer(op, lambda Q, Kt, V: op.attention(Q, Kt, V))
    b = _one_layer(op, lambda Q, Kt, V: op.attention(Q, Kt, V, fused=False))
    c = _one_layer(op, lambda Q, Kt, V: op.spmm(op.softmax(op.sddmm(Q, Kt), 64 ** -0.5), V))
    fused = _one_layer(op, lambda Q, Kt, V: op.attention(Q, Kt, V, fused=True))
    for x, y, z, f in zip(a, b, c, fused):
        assert _same(x, y) and _same(x, z)
        x, f = x.detach(), f.detach()
        assert torch.allclose(x, f, rtol=1e-4, atol=1e-5 * float(x.abs().max()))     # the same function, another order


def test_empty_rows_give_zero_rows(op):  # noqa: F811
    Q = _rand(op.M, 32, seed=31, requires_grad=False)
    Kt = _rand(op.N, 32, seed=32, requires_grad=False)
    V = _rand(op.N, 64, seed=33)
    O = op.attention(Q, Kt, V, scale=2.0, fused=True)
    Oc = O.detach().cpu()
    assert (Oc[~op.has_row].view(torch.int32) == 0).all() and (Oc[op.has_row].abs().sum(-1) > 0).all()
    O.sum().backward()
    assert torch.isfinite(V.grad).all()


# ---- 16-bit operands -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def op16(engine):
    """one operator with the defaults (mode F16, gather_mode F32) on a pattern whose rows all have entries"""
    import bsmr_torch
    rows, cols, ro, ci = synth.random_pattern(256, 384, 12000, seed=5)
    assert (np.diff(ro) > 0).all() and np.diff(ro.astype(np.int64)).max() <= 400
    o = bsmr_torch.SparseOperator(engine.CSR.from_arrays(rows, cols, ro, ci), device=0)
    o.rl, o.cl = row_lists(ro, ci), col_lists(rows, cols, ro, ci)
    o.ro, o.ci = ro.astype(np.int64), ci.astype(np.int64)
    return o


def _fp64_rows(o, P, scale, wV, wH, dW):
    """per row, in fp64 over z = fl32(scale P): O64, and dP's reference and bound
         dP64_t = scale w64_t (dW_t - D64),  D64 = dO_r . O64_r
         bound_t = |scale| w64_t [ u16 sum_k |dO_k| |O64_k| ]                                      (the 16-bit term)
                 + |scale| w64_t [ (3 n + 4 Z_r + Kv + 32) u (|dW_t| + A_r) + 2^-25 sum_k |dO_k| ]  (the fp32 terms)
       with A_r = sum_k |dO_k| sum_t w64_t |V[c_t,k]| >= |D64|; the last term covers fp16's subnormal spacing."""
    z = (np.float32(scale) * P.astype(np.float32)).astype(np.float64)
    Kv = wV.shape[1]
    O64 = np.zeros((o.M, Kv))
    dP64, b16, b32 = (np.zeros(o.nnz) for _ in range(3))
    for r in range(o.M):
        a, b = o.ro[r], o.ro[r + 1]
        d = z[a:b] - z[a:b].max()
        w = np.exp(d)
        w /= w.sum()
        x = wV[o.ci[a:b]].astype(np.float64)
        O64[r] = w @ x
        h = np.abs(wH[r].astype(np.float64))
        D64 = wH[r].astype(np.float64) @ O64[r]
        A = h @ (w @ np.abs(x))
        dP64[a:b] = scale * w * (dW[a:b] - D64)
        b16[a:b] = abs(scale) * w * (h @ np.abs(O64[r]))
        b32[a:b] = abs(scale) * w * ((3 * (b - a) + 4 * np.abs(d).max() + Kv + 32) * U * (np.abs(dW[a:b]) + A)
                                     + 2.0 ** -25 * h.sum())
    return O64, dP64, b16, b32


@pytest.mark.parametrize("mode", (0, 1))
def test_16_bit_operands_train_through_the_fused_path(engine, oracle, op16, mode):
    o = op16
    rng = np.random.default_rng(60 + mode)
    Q, Kt, V, H = _operands(mode, rng, o)
    scale = K ** -0.5
    (tQ, wQ), (tK, wK), (tV, wV) = (_t16(mode, x, grad=True) for x in (Q, Kt, V))
    tH, wH = _t16(mode, H)
    P = o.sddmm(tQ, tK)
    P.retain_grad()
    O = o.softmax_spmm(P, tV, scale)
    O.backward(tH)
    assert O.dtype == DT[mode] and P.dtype == torch.float32 and P.grad.dtype == torch.float32
    for g in (tQ.grad, tK.grad, tV.grad):
        assert g.dtype == DT[mode] and np.isfinite(_np(g)).all() and np.abs(_np(g)).max() > 0
    # the raw calls: the same bits, and W
    Pd = P.detach()
    O_raw, m, s = o._attention(Pd, tV.detach(), scale)
    dW = o._sddmm(tH, tV.detach())
    dW_np = _np(dW)
    dP_raw, W = o._attention_backward(Pd, m, s, dW, O_raw, tH, scale)
    assert _bits(O_raw) == _bits(O) and _same(dP_raw, P.grad) and W.dtype == torch.float32
    dP, Wn = _np(P.grad), _np(W)
    assert_twin(_np(tV.grad), _rounded(oracle, mode, o.cl, Wn, wH), "V.grad")
    assert_twin(_np(tQ.grad), _rounded(oracle, mode, o.rl, dP, wK), "Q.grad")
    assert_twin(_np(tK.grad), _rounded(oracle, mode, o.cl, dP, wQ), "Kt.grad")
    # the forward within one output rounding of fp64, dP inside its bound
    O64, dP64, b16, b32 = _fp64_rows(o, _np(Pd), scale, wV, wH, dW_np.astype(np.float64))
    vmax = np.maximum.reduceat(np.abs(wV.astype(np.float64))[o.ci], o.ro[:-1], axis=0)
    err = np.abs(_np(O).astype(np.float64) - O64)
    print(f"mode={mode}: worst |O - O64| / bound = {(err / (2 * U16[mode] * vmax)).max():.3f}")
    assert (err <= 2 * U16[mode] * vmax).all()
    err = np.abs(dP.astype(np.float64) - dP64)
    bound = U16[mode] * b16 + b32
    print(f"mode={mode}: worst |dP - dP64| / bound = {(err / bound).max():.3f}; 16-bit share of the bound "
          f"{(U16[mode] * b16 / bound).min():.3f} .. {(U16[mode] * b16 / bound).max():.3f}")
    assert (err <= bound).all()
    # attention(fused=True) is this composition, and repeats
    for _ in range(2):
        (aQ, _), (aK, _), (aV, _) = (_t16(mode, x, grad=True) for x in (Q, Kt, V))
        A = o.attention(aQ, aK, aV, fused=True)
        A.backward(tH)
        assert _bits(A) == _bits(O)
        for g, h in ((aQ.grad, tQ.grad), (aK.grad, tK.grad), (aV.grad, tV.grad)):
            assert _bits(g) == _bits(h)


def test_bad_inputs_raise_value_error(op):  # noqa: F811
    Q, Kt = torch.zeros(op.M, 64, device=_dev()), torch.zeros(op.N, 64, device=_dev())
    V = torch.zeros(op.N, 64, device=_dev())
    v = torch.zeros(op.nnz, device=_dev())
    for q, k, x in ((Q.half(), Kt, V), (Q, Kt.bfloat16(), V), (Q.half(), Kt.bfloat16(), V), (Q, Kt, V.double())):
        with pytest.raises(ValueError):
            op.attention(q, k, x, fused=True)                                  # mixed or unsupported dtypes
    for x in (torch.zeros(op.N, 48, device=_dev()), torch.zeros(op.M, 64, device=_dev()),
              torch.zeros(2, op.N, 64, device=_dev()), V.cpu(), V.T.contiguous().T):
        with pytest.raises(ValueError):
            op.attention(Q, Kt, x, fused=True)                                 # Kv, rows, batch, device, layout
        with pytest.raises(ValueError):
            op.softmax_spmm(v, x)
    for vals in (v.half(), v.bfloat16(), v[:-1], v.cpu(), v.view(1, -1).expand(2, -1)):
        with pytest.raises(ValueError):
            op.softmax_spmm(vals, V)                                           # 16-bit or misshapen values
    with pytest.raises(ValueError):
        op.softmax_spmm(v.half(), V.half())
    for scale in (float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            op.softmax_spmm(v, V, scale)
    assert op.softmax_spmm(v, V.half()).dtype == torch.float16                 # fp32 values with 16-bit rows are served
    assert op.attention(Q.bfloat16(), Kt.bfloat16(), V, fused=True).dtype == torch.float32
