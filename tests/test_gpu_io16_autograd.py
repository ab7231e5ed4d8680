"""bsmr_torch.SparseOperator on torch.float16 / torch.bfloat16 tensors: the format follows the dtype, nothing is widened
or copied on the way in or out.  Every 16-bit result is oracle.round_array(format, fp32 twin on the widened operand)
(tests/gather_twin.py), bit for bit; P and the softmax weights stay fp32; attention composes, trains and repeats
bitwise; fp32 tensors on the same operator still give the bits of the raw fp32 calls."""
import numpy as np
import pytest

import synth
from gather_twin import assert_twin, col_lists, gather, row_lists

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U16 = {0: 2.0 ** -11, 1: 2.0 ** -8}
ROUND = {0: 2, 1: 3}                 # engine mode -> oracle.round_array id (tests/test_oracle.py: 2 = fp16, 3 = bf16)
DT = {0: torch.float16, 1: torch.bfloat16}
K = 64


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def op(engine):
    """one operator, built with the defaults (mode F16, gather_mode F32): 16-bit tensors do not consult either"""
    import bsmr_torch
    rows, cols, ro, ci = synth.random_pattern(256, 384, 12000, seed=5)
    assert (np.diff(ro) > 0).all()
    o = bsmr_torch.SparseOperator(engine.CSR.from_arrays(rows, cols, ro, ci), device=0)
    o.rl, o.cl = row_lists(ro, ci), col_lists(rows, cols, ro, ci)
    return o


def _wide(rng, shape, lo=-6, hi=3):
    m = rng.integers(1 << 23, 1 << 24, size=shape).astype(np.float64)
    s = rng.choice([-1.0, 1.0], size=shape)
    return (s * np.ldexp(m, rng.integers(lo, hi + 1, size=shape) - 23)).astype(np.float32)


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev()).requires_grad_(grad)


def _t16(mode, a, grad=False):
    """fp32 array -> (device tensor of the mode's dtype, cast on the CPU; its exact widening as numpy)"""
    c = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[mode])
    return c.to(_dev()).requires_grad_(grad), c.float().numpy()


def _np(t):
    return t.detach().float().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().tobytes()


def _rounded(oracle, mode, lists, v, X):
    """round(twin): v (nnz,) or (b, nnz), X (rows, K) or (b, rows, K)"""
    if X.ndim == 2:
        return oracle.round_array(ROUND[mode], gather(oracle, lists, v, X))
    return np.stack([oracle.round_array(ROUND[mode], gather(oracle, lists, v[b], X[b])) for b in range(X.shape[0])])


@pytest.mark.parametrize("batch", (None, 2))
@pytest.mark.parametrize("transpose", (False, True))
@pytest.mark.parametrize("mode", (0, 1))
def test_spmm_forward_and_dx_equal_the_rounded_twin(engine, oracle, op, mode, transpose, batch):
    rng = np.random.default_rng(10 + mode + 2 * transpose + 4 * bool(batch))
    lead = () if batch is None else (batch,)
    rows_x, rows_y = (op.M, op.N) if transpose else (op.N, op.M)
    v = _wide(rng, lead + (op.nnz,), -3, 3)
    tX, X = _t16(mode, _wide(rng, lead + (rows_x, K)), grad=True)
    tH, H = _t16(mode, _wide(rng, lead + (rows_y, K)))
    tv = _t(v, grad=True)
    Y = op.spmm(tv, tX, transpose=transpose)
    assert Y.dtype == DT[mode] and Y.shape == lead + (rows_y, K)
    fwd, bwd = (op.cl, op.rl) if transpose else (op.rl, op.cl)
    assert_twin(_np(Y), _rounded(oracle, mode, fwd, v, X), f"spmm forward mode={mode}")
    Y.backward(tH)
    assert tX.grad.dtype == DT[mode] and tv.grad.dtype == torch.float32 and tv.grad.shape == tv.shape
    assert_twin(_np(tX.grad), _rounded(oracle, mode, bwd, v, H), f"spmm dX mode={mode}")
    assert np.isfinite(_np(tv.grad)).all() and np.abs(_np(tv.grad)).max() > 0


@pytest.mark.parametrize("batch", (None, 2))
@pytest.mark.parametrize("mode", (0, 1))
def test_sddmm_is_exact_and_its_gradients_equal_the_rounded_twin(engine, oracle, op, mode, batch):
    rng = np.random.default_rng(20 + mode + 2 * bool(batch))
    lead = () if batch is None else (batch,)
    ints = lambda rows: rng.integers(-127, 128, size=lead + (rows, K)).astype(np.float32)
    tA, A = _t16(mode, ints(op.M), grad=True)
    tB, B = _t16(mode, ints(op.N), grad=True)
    G = _wide(rng, lead + (op.nnz,), -3, 3)
    P = op.sddmm(tA, tB)
    assert P.dtype == torch.float32 and P.shape == lead + (op.nnz,)
    ro, ci = op.csr.row_offsets.astype(np.int64), op.csr.col_indices.astype(np.int64)
    row_of = np.repeat(np.arange(op.M), np.diff(ro))
    exact = np.einsum("...tk,...tk->...t", A[..., row_of, :].astype(np.float64), B[..., ci, :].astype(np.float64))
    assert np.abs(exact).max() < 2 ** 24 and np.array_equal(_np(P).astype(np.float64), exact)
    P.backward(_t(G))
    assert tA.grad.dtype == DT[mode] and tB.grad.dtype == DT[mode]
    assert_twin(_np(tA.grad), _rounded(oracle, mode, op.rl, G, B), f"dA mode={mode}")
    assert_twin(_np(tB.grad), _rounded(oracle, mode, op.cl, G, A), f"dB mode={mode}")


def _operands(mode, rng, op):
    Q, Kt = rng.uniform(-1, 1, (op.M, K)).astype(np.float32), rng.uniform(-1, 1, (op.N, K)).astype(np.float32)
    V = (rng.choice([-1.0, 1.0], (op.N, K)) * rng.uniform(2.0 ** -6, 2, (op.N, K))).astype(np.float32)
    H = rng.uniform(-1, 1, (op.M, K)).astype(np.float32)
    return Q, Kt, V, H


@pytest.mark.parametrize("mode", (0, 1))
def test_attention_written_out_equals_the_twins_and_op_attention(engine, oracle, op, mode):
    rng = np.random.default_rng(30 + mode)
    Q, Kt, V, H = _operands(mode, rng, op)
    scale = K ** -0.5

    def step(composed):
        (tQ, wQ), (tK, wK), (tV, wV) = (_t16(mode, x, grad=True) for x in (Q, Kt, V))
        tH, wH = _t16(mode, H)
        if composed:
            O = op.attention(tQ, tK, tV)
            P = W = None
        else:
            P = op.sddmm(tQ, tK)
            W = op.softmax(P, scale)
            O = op.spmm(W, tV)
            P.retain_grad()
            W.retain_grad()
        O.backward(tH)
        torch.cuda.synchronize()
        return dict(O=O, dQ=tQ.grad, dK=tK.grad, dV=tV.grad, P=P, W=W, wQ=wQ, wK=wK, wV=wV, wH=wH)

    a = step(False)
    assert a["P"].dtype == torch.float32 and a["W"].dtype == torch.float32
    for k in ("O", "dQ", "dK", "dV"):
        assert a[k].dtype == DT[mode] and np.isfinite(_np(a[k])).all() and np.abs(_np(a[k])).max() > 0, k
    W, dP = _np(a["W"]), _np(a["P"].grad)
    assert_twin(_np(a["O"]), _rounded(oracle, mode, op.rl, W, a["wV"]), "O")
    assert_twin(_np(a["dV"]), _rounded(oracle, mode, op.cl, W, a["wH"]), "V.grad")
    assert_twin(_np(a["dQ"]), _rounded(oracle, mode, op.rl, dP, a["wK"]), "Q.grad")
    assert_twin(_np(a["dK"]), _rounded(oracle, mode, op.cl, dP, a["wQ"]), "Kt.grad")
    for other, name in ((step(True), "op.attention"), (step(False), "a second step")):
        for k in ("O", "dQ", "dK", "dV"):
            assert _bits(other[k]) == _bits(a[k]), (name, k)


@pytest.mark.parametrize("mode", (0, 1))
def test_attention_forward_within_one_output_rounding_of_fp64(engine, op, mode):
    """|O - O64| <= 2 u16 max_{t in row} |V|: the one output rounding gives u16 |O| <= u16 max|V| (O is a convex
    combination of V's rows); the fp32 terms - (n + K) u from the products, the softmax and the chain - stay below u16
    for rows of at most a few hundred entries.  O64: fp64 dense attention on the widened 16-bit operands."""
    rng = np.random.default_rng(50 + mode)
    Q, Kt, V, _ = _operands(mode, rng, op)
    (tQ, wQ), (tK, wK), (tV, wV) = (_t16(mode, x) for x in (Q, Kt, V))
    O = _np(op.attention(tQ, tK, tV)).astype(np.float64)
    ro, ci = op.csr.row_offsets.astype(np.int64), op.csr.col_indices.astype(np.int64)
    assert np.diff(ro).max() <= 400
    mask = np.zeros((op.M, op.N), dtype=bool)
    mask[np.repeat(np.arange(op.M), np.diff(ro)), ci] = True
    Z = np.where(mask, (wQ.astype(np.float64) @ wK.astype(np.float64).T) * K ** -0.5, -np.inf)
    E = np.exp(Z - Z.max(axis=1, keepdims=True))
    O64 = (E / E.sum(axis=1, keepdims=True)) @ wV.astype(np.float64)
    vmax = np.maximum.reduceat(np.abs(wV.astype(np.float64))[ci], ro[:-1], axis=0)      # (M, K): every row has entries
    bound = 2 * U16[mode] * vmax
    err = np.abs(O - O64)
    print(f"mode={mode}: worst |O - O64| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


def test_fp32_tensors_still_give_the_raw_fp32_bits(engine, op):
    rng = np.random.default_rng(40)
    v, X, H, A = _wide(rng, op.nnz, -3, 3), _wide(rng, (op.N, K)), _wide(rng, (op.M, K)), _wide(rng, (op.M, K))
    s = torch.cuda.current_stream(_dev()).cuda_stream
    tv, tX, tH, tA = _t(v), _t(X, grad=True), _t(H), _t(A, grad=True)
    raw = {k: torch.full((r, K), float("nan"), device=_dev()) for k, r in (("Y", op.M), ("dX", op.N), ("dA", op.M), ("dB", op.N))}
    rawP = torch.full((op.nnz,), float("nan"), device=_dev())
    hip = engine.hip()
    assert hip.bsmr_spmm(op._bw, K, 0, tv.data_ptr(), tX.data_ptr(), raw["Y"].data_ptr(), 1, s) == engine.OK
    assert hip.bsmr_spmm(op._bw, K, 1, tv.data_ptr(), tH.data_ptr(), raw["dX"].data_ptr(), 1, s) == engine.OK
    assert hip.bsmr_sddmm_backward(op._bw, K, tv.data_ptr(), tA.data_ptr(), tX.data_ptr(), raw["dA"].data_ptr(),
                                   raw["dB"].data_ptr(), 1, s) == engine.OK
    assert hip.bsmr_sddmm(op._plan, K, tA.data_ptr(), tX.data_ptr(), rawP.data_ptr(), op.mode, s) == engine.OK
    torch.cuda.synchronize()
    same = lambda a, b: a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes()
    Y = op.spmm(tv, tX)
    Y.backward(tH)
    assert Y.dtype == torch.float32 and same(Y, raw["Y"]) and same(tX.grad, raw["dX"])
    tB = _t(X, grad=True)
    P = op.sddmm(tA, tB)
    P.backward(tv)
    assert same(P, rawP) and same(tA.grad, raw["dA"]) and same(tB.grad, raw["dB"])


def test_mixed_dtypes_and_16_bit_values_raise(engine, op):
    A, B = torch.zeros(op.M, K, device=_dev()), torch.zeros(op.N, K, device=_dev())
    v = torch.zeros(op.nnz, device=_dev())
    for a, b in ((A.half(), B), (A, B.bfloat16()), (A.half(), B.bfloat16()), (A.double(), B.double())):
        with pytest.raises(ValueError):
            op.sddmm(a, b)
    for vals, X in ((v.half(), B), (v.bfloat16(), B.bfloat16()), (v.half(), B.half())):
        with pytest.raises(ValueError):
            op.spmm(vals, X)
    with pytest.raises(ValueError):
        op.softmax(v.half())
    with pytest.raises(ValueError):
        op.softmax(v.bfloat16(), 0.5)
    assert op.sddmm(A.half(), B.half()).dtype == torch.float32            # a shared 16-bit dtype is served
    assert op.spmm(v, B.bfloat16()).dtype == torch.bfloat16
