"""bsmr_torch.SparseOperator(csr, gather_mode=...): with COMPUTE_F16 / COMPUTE_BF16 the gathers of spmm (forward and dX)
and of sddmm's backward (dA, dB) read 16-bit rows, and every result is the fp32 twin (tests/gather_twin.py) on the
oracle-rounded operand, bit for bit; attention trains and is bitwise reproducible, within the header's bound of the
fp32 operator; the default operator equals the raw fp32 calls."""
import numpy as np
import pytest

import synth
from gather_twin import assert_twin, col_lists, gather, row_lists

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -24
U16 = {0: 2.0 ** -11, 1: 2.0 ** -8}
ROUND = {0: 2, 1: 3}                 # engine mode -> oracle.round_array id (tests/test_oracle.py: 2 = fp16, 3 = bf16)
K = 64


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(engine):
    """operator(gather_mode) over one pattern (every row has entries); None = built without the argument"""
    import bsmr_torch
    rows, cols, ro, ci = synth.random_pattern(256, 384, 12000, seed=5)
    assert (np.diff(ro) > 0).all()
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    made = {}

    def get(gather_mode):
        if gather_mode not in made:
            kw = {} if gather_mode is None else {"gather_mode": gather_mode}
            o = bsmr_torch.SparseOperator(csr, mode=engine.COMPUTE_F16, device=0, **kw)
            o.rl, o.cl = row_lists(ro, ci), col_lists(rows, cols, ro, ci)
            made[gather_mode] = o
        return made[gather_mode]

    return get


def _wide(rng, shape, lo=-10, hi=10):
    m = rng.integers(1 << 23, 1 << 24, size=shape).astype(np.float64)
    s = rng.choice([-1.0, 1.0], size=shape)
    return (s * np.ldexp(m, rng.integers(lo, hi + 1, size=shape) - 23)).astype(np.float32)


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev()).requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("transpose", (False, True))
@pytest.mark.parametrize("mode", (0, 1))
def test_spmm_forward_and_dx_equal_the_twin_on_rounded_rows(engine, oracle, ops, mode, transpose):
    op = ops(mode)
    rng = np.random.default_rng(10 + mode + 2 * transpose)
    rows_x, rows_y = (op.M, op.N) if transpose else (op.N, op.M)
    v, X, H = _wide(rng, op.nnz, -4, 4), _wide(rng, (rows_x, K)), _wide(rng, (rows_y, K))
    tv, tX = _t(v), _t(X, grad=True)
    Y = op.spmm(tv, tX, transpose=transpose)
    fwd, bwd = (op.cl, op.rl) if transpose else (op.rl, op.cl)
    assert_twin(_np(Y), gather(oracle, fwd, v, oracle.round_array(ROUND[mode], X)), f"spmm forward mode={mode}")
    Y.backward(_t(H))
    assert_twin(_np(tX.grad), gather(oracle, bwd, v, oracle.round_array(ROUND[mode], H)), f"spmm dX mode={mode}")


@pytest.mark.parametrize("mode", (0, 1))
def test_sddmm_gradients_equal_the_twin_on_rounded_rows(engine, oracle, ops, mode):
    op = ops(mode)
    rng = np.random.default_rng(20 + mode)
    A, B, G = _wide(rng, (op.M, K)), _wide(rng, (op.N, K)), _wide(rng, op.nnz, -4, 4)
    tA, tB = _t(A, grad=True), _t(B, grad=True)
    op.sddmm(tA, tB).backward(_t(G))
    assert_twin(_np(tA.grad), gather(oracle, op.rl, G, oracle.round_array(ROUND[mode], B)), f"dA mode={mode}")
    assert_twin(_np(tB.grad), gather(oracle, op.cl, G, oracle.round_array(ROUND[mode], A)), f"dB mode={mode}")


def _attention_step(op, Q, Kt, V, H):
    tQ, tK, tV = _t(Q, grad=True), _t(Kt, grad=True), _t(V, grad=True)
    O = op.attention(tQ, tK, tV)
    O.backward(_t(H))
    torch.cuda.synchronize()
    return [_np(x) for x in (O, tQ.grad, tK.grad, tV.grad)]


@pytest.mark.parametrize("mode", (0, 1))
def test_attention_trains_reproducibly_within_the_bound(engine, ops, mode):
    """O = S_W V with W the row softmax (W >= 0, sum_t W_t <= 1 + (n + 6) u, include/bsmr_hip.h): both operators compute
    the same W, so |O16 - O32| <= |O16 - S_W V| + |O32 - S_W V|
                               <= ((n + 2) u (1 + u16) + u16 + (n + 2) u) (1 + (n + 6) u) max_{t in row} |V[c_t, k]|,
    a bound from V and the pattern alone (V inside the 16-bit formats' normal range)."""
    op, ref = ops(mode), ops(engine.COMPUTE_F32)
    rng = np.random.default_rng(30 + mode)
    Q, Kt = rng.uniform(-1, 1, (op.M, K)).astype(np.float32), rng.uniform(-1, 1, (op.N, K)).astype(np.float32)
    V = (rng.choice([-1.0, 1.0], (op.N, K)) * rng.uniform(2.0 ** -6, 2, (op.N, K))).astype(np.float32)
    H = rng.uniform(-1, 1, (op.M, K)).astype(np.float32)
    first, again = _attention_step(op, Q, Kt, V, H), _attention_step(op, Q, Kt, V, H)
    for a, b, name in zip(first, again, ("O", "dQ", "dKt", "dV")):
        assert a.tobytes() == b.tobytes(), name
        assert np.isfinite(a).all() and np.abs(a).max() > 0, name
    O32 = _attention_step(ref, Q, Kt, V, H)[0]
    ro, ci = op.csr.row_offsets.astype(np.int64), op.csr.col_indices.astype(np.int64)
    n = np.diff(ro).astype(np.float64)[:, None]
    vmax = np.maximum.reduceat(np.abs(V.astype(np.float64))[ci], ro[:-1], axis=0)          # (M, K): every row has entries
    bound = ((n + 2) * U * (1 + U16[mode]) + U16[mode] + (n + 2) * U) * (1 + (n + 6) * U) * vmax
    err = np.abs(first[0].astype(np.float64) - O32)
    print(f"mode={mode}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert (first[0] != O32).any()                       # the mode does change what is gathered


def test_default_operator_equals_the_raw_fp32_calls(engine, ops):
    """built without gather_mode, and with gather_mode=COMPUTE_F32: spmm, its dX and sddmm's dA / dB carry the bits of
    bsmr_spmm / bsmr_sddmm_backward on the same handle"""
    rng = np.random.default_rng(40)
    for op in (ops(None), ops(engine.COMPUTE_F32)):
        assert op.gather_mode == engine.COMPUTE_F32
        v, X, H = _wide(rng, op.nnz, -4, 4), _wide(rng, (op.N, K)), _wide(rng, (op.M, K))
        A = _wide(rng, (op.M, K))
        s = torch.cuda.current_stream(_dev()).cuda_stream
        tv, tX, tH, tA = _t(v), _t(X, grad=True), _t(H), _t(A, grad=True)
        raw = {k: torch.full((r, K), float("nan"), device=_dev()) for k, r in (("Y", op.M), ("dX", op.N), ("dA", op.M),
                                                                              ("dB", op.N))}
        hip = engine.hip()
        assert hip.bsmr_spmm(op._bw, K, 0, tv.data_ptr(), tX.data_ptr(), raw["Y"].data_ptr(), 1, s) == engine.OK
        assert hip.bsmr_spmm(op._bw, K, 1, tv.data_ptr(), tH.data_ptr(), raw["dX"].data_ptr(), 1, s) == engine.OK
        assert hip.bsmr_sddmm_backward(op._bw, K, tv.data_ptr(), tA.data_ptr(), tX.data_ptr(), raw["dA"].data_ptr(),
                                       raw["dB"].data_ptr(), 1, s) == engine.OK
        torch.cuda.synchronize()
        Y = op.spmm(tv, tX)
        Y.backward(tH)
        assert _np(Y).tobytes() == _np(raw["Y"]).tobytes() and _np(tX.grad).tobytes() == _np(raw["dX"]).tobytes()
        tB = _t(X, grad=True)
        op.sddmm(tA, tB).backward(tv)
        assert _np(tA.grad).tobytes() == _np(raw["dA"]).tobytes() and _np(tB.grad).tobytes() == _np(raw["dB"]).tobytes()


def test_gather_mode_is_validated(engine):
    import bsmr_torch
    rows, cols, ro, ci = synth.random_pattern(20, 30, 100, seed=5)
    with pytest.raises(ValueError):
        bsmr_torch.SparseOperator(engine.CSR.from_arrays(rows, cols, ro, ci), gather_mode=5)
