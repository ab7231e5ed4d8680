"""bsmr_torch.SparseOperator: SDDMM and SpMM as torch autograd functions on the engine, against dense fp64 torch.

Gradients are the engine's fp32 gather-and-accumulate (bsmr_sddmm_backward / bsmr_spmm, error bound
(n + 2) u sum|g||x| per element) or the plan's SDDMM in the operator's mode (COMPUTE_F32 here: fp32 products, fp32
sums in some order, bound (K + 2) u sum|a||b|)."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -24


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def op(engine):
    import bsmr_torch
    rows, cols, ro, ci = synth.random_pattern(256, 384, 12000, seed=5)
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    o = bsmr_torch.SparseOperator(csr, mode=engine.COMPUTE_F32, device=0)
    o.rows_t = torch.from_numpy(np.repeat(np.arange(rows), np.diff(ro.astype(np.int64)))).to(_dev())
    o.cols_t = torch.from_numpy(ci.astype(np.int64)).to(_dev())
    assert (np.diff(ro) > 0).all()   # every row has entries (the softmax below needs it)
    return o


def _dense(op, v):
    """(..., nnz) values -> (..., M, N) fp64 dense matrix on the CPU"""
    v = v.detach().double().cpu()
    lead = v.shape[:-1]
    D = torch.zeros(lead + (op.M, op.N), dtype=torch.float64)
    D[..., op.rows_t.cpu(), op.cols_t.cpu()] = v
    return D


def _within(got, want, mag, n):
    got = got.detach().double().cpu()
    assert torch.all((got - want).abs() <= (n + 2) * U * mag + 1e-30), float(((got - want).abs() - (n + 2) * U * mag).max())


def _rand(*shape, seed, requires_grad=True):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1).to(_dev()).requires_grad_(requires_grad)


@pytest.mark.parametrize("batch", [None, 3])
def test_sddmm_gradients(op, batch):
    K = 64
    lead = () if batch is None else (batch,)
    A = _rand(*lead, op.M, K, seed=1)
    B = _rand(*lead, op.N, K, seed=2)
    G = _rand(*lead, op.nnz, seed=3, requires_grad=False)
    P = op.sddmm(A, B)
    assert P.shape == lead + (op.nnz,)
    Gd = _dense(op, G)
    Ad, Bd = A.detach().double().cpu(), B.detach().double().cpu()
    Pd = (Ad @ Bd.transpose(-1, -2))[..., op.rows_t.cpu(), op.cols_t.cpu()]
    mag = (Ad.abs() @ Bd.abs().transpose(-1, -2))[..., op.rows_t.cpu(), op.cols_t.cpu()]
    _within(P, Pd, mag, K)
    (P * G).sum().backward()
    row_n = Gd.ne(0).sum(-1, keepdim=True).double()
    col_n = Gd.ne(0).sum(-2).unsqueeze(-1).double()
    _within(A.grad, Gd @ Bd, Gd.abs() @ Bd.abs(), row_n)
    _within(B.grad, Gd.transpose(-1, -2) @ Ad, Gd.abs().transpose(-1, -2) @ Ad.abs(), col_n)
    # only the inputs that need a gradient get one
    A2 = A.detach().clone().requires_grad_(True)
    B2 = B.detach().clone()
    (op.sddmm(A2, B2) * G).sum().backward()
    assert B2.grad is None and A2.grad.detach().cpu().numpy().tobytes() == A.grad.cpu().numpy().tobytes()


@pytest.mark.parametrize("transpose", [False, True])
def test_spmm_forward_and_gradients(op, transpose):
    K = 96
    rows_x, rows_y = (op.M, op.N) if transpose else (op.N, op.M)
    v = _rand(op.nnz, seed=11)
    X = _rand(rows_x, K, seed=12)
    H = _rand(rows_y, K, seed=13, requires_grad=False)
    Y = op.spmm(v, X, transpose=transpose)
    S = _dense(op, v)
    S = S.T if transpose else S
    Xd, Hd = X.detach().double().cpu(), H.double().cpu()
    n_y = S.ne(0).sum(-1, keepdim=True).double()
    _within(Y, S @ Xd, S.abs() @ Xd.abs(), n_y)
    (Y * H).sum().backward()
    # d values[t] = H[dest(t)] . X[src(t)]
    r, c = op.rows_t.cpu(), op.cols_t.cpu()
    dst, src = (c, r) if transpose else (r, c)
    _within(v.grad, (Hd[dst] * Xd[src]).sum(-1), (Hd[dst].abs() * Xd[src].abs()).sum(-1), K)
    n_x = S.ne(0).sum(-2).unsqueeze(-1).double()
    _within(X.grad, S.T @ Hd, S.abs().T @ Hd.abs(), n_x)


def _softmax_rows(op, P):
    m = torch.full((op.M,), float("-inf"), device=P.device).scatter_reduce(0, op.rows_t, P.detach(), "amax")
    e = torch.exp(P - m[op.rows_t])
    s = torch.zeros(op.M, device=P.device, dtype=P.dtype).index_add(0, op.rows_t, e)
    return e / s[op.rows_t]


def test_two_layer_sparse_attention_step(op):
    """SDDMM -> row softmax in torch -> SpMM, twice (the first layer's output is the second's query), against the same
    computation on dense masked fp64 torch."""
    K = 64
    Q = _rand(op.M, K, seed=21)
    Kk = [_rand(op.N, K, seed=22 + i) for i in range(2)]
    V = [_rand(op.N, K, seed=24 + i) for i in range(2)]
    H = _rand(op.M, K, seed=26, requires_grad=False)
    x = Q
    for i in range(2):
        P = op.sddmm(x, Kk[i]) * K ** -0.5
        x = op.spmm(_softmax_rows(op, P), V[i])
    (x * H).sum().backward()

    mask = torch.zeros(op.M, op.N, dtype=torch.bool)
    mask[op.rows_t.cpu(), op.cols_t.cpu()] = True
    leaves = [Q] + Kk + V
    ref = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    x = ref[0]
    for i in range(2):
        s = (x @ ref[1 + i].T) * K ** -0.5
        x = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1) @ ref[3 + i]
    (x * H.double().cpu()).sum().backward()
    for got, want in zip(leaves, ref):
        g, w = got.grad.double().cpu(), want.grad
        assert torch.allclose(g, w, rtol=1e-4, atol=1e-5 * float(w.abs().max())), float((g - w).abs().max())


def test_bad_inputs_raise_value_error(op):
    K = 64
    A = torch.zeros(op.M, K, device=_dev())
    B = torch.zeros(op.N, K, device=_dev())
    v = torch.zeros(op.nnz, device=_dev())
    bad_pairs = [
        (A.half(), B),                                    # fp16
        (A.cpu(), B),                                     # CPU tensor
        (A[:-1], B),                                      # wrong shape
        (torch.zeros(K, op.M, device=_dev()).T, B),       # non-contiguous
        (torch.zeros(op.M, 48, device=_dev()), torch.zeros(op.N, 48, device=_dev())),   # K not a multiple of 32
        (A, torch.zeros(2, op.N, K, device=_dev())),      # batch mismatch
    ]
    for a, b in bad_pairs:
        with pytest.raises(ValueError):
            op.sddmm(a, b)
    with pytest.raises(ValueError):
        op.spmm(v.half(), B)
    with pytest.raises(ValueError):
        op.spmm(v[:-1], B)
    with pytest.raises(ValueError):
        op.spmm(v, B.cpu())
    with pytest.raises(ValueError):
        op.spmm(v, A)                                     # transpose=False wants N rows
    with pytest.raises(ValueError):
        op.spmm(v, torch.zeros(K, op.N, device=_dev()).T)


# --------------------------------------------------------------------------------------------------------------------
# The shipped modes.  SparseOperator's default is COMPUTE_F16; the mode decides the forward SDDMM and so the gradient
# d values of spmm, but never the fp32 gather of dA / dB / dX, which must equal the backward's twin bit for bit
# (oracle/spmm_oracle.c; lists from numpy, tests/gather_twin.py).
# --------------------------------------------------------------------------------------------------------------------
import ctypes as C  # noqa: E402

from gather_twin import assert_twin, col_lists, gather, row_lists  # noqa: E402

MODES = ("COMPUTE_F16", "COMPUTE_BF16", "COMPUTE_F32")
ROUND = {"COMPUTE_F16": 2, "COMPUTE_BF16": 3}            # oracle.round_array: fp16 / bf16 RNE


@pytest.fixture(scope="module")
def mode_ops(engine):
    import bsmr_torch
    rows, cols, ro, ci = synth.random_pattern(256, 384, 12000, seed=5)
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    made = {}

    def get(mode):
        if mode not in made:
            o = bsmr_torch.SparseOperator(csr, mode=getattr(engine, mode), device=0)
            o.ro, o.ci = ro.astype(np.uint32), ci.astype(np.uint32)
            o.row_of = np.repeat(np.arange(rows), np.diff(ro.astype(np.int64)))
            o.rl, o.cl = row_lists(o.ro, o.ci), col_lists(rows, cols, o.ro, o.ci)
            made[mode] = o
        return made[mode]

    yield get
    made.clear()


def _wide(rng, shape, lo, hi):
    """+-m 2^e, full 24-bit m, e in [lo, hi]"""
    m = rng.integers(1 << 23, 1 << 24, size=shape).astype(np.float64)
    e = rng.integers(lo, hi + 1, size=shape) - 23
    return (rng.choice([-1.0, 1.0], size=shape) * np.ldexp(m, e)).astype(np.float32)


def _leaf(a, requires_grad=True):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev()).requires_grad_(requires_grad)


@pytest.mark.parametrize("batch", [None, 2])
@pytest.mark.parametrize("mode", MODES)
def test_sddmm_gradients_equal_the_twin_in_every_mode(mode_ops, oracle, mode, batch):
    """'exact fp32 products of the given operands in every mode': A.grad and B.grad are the twin's bits"""
    op = mode_ops(mode)
    K = 96
    rng = np.random.default_rng(len(mode) + (batch or 0))
    lead = () if batch is None else (batch,)
    A, B = _wide(rng, lead + (op.M, K), -12, 12), _wide(rng, lead + (op.N, K), -12, 12)
    G = _wide(rng, lead + (op.nnz,), -12, 12)
    tA, tB = _leaf(A), _leaf(B)
    (op.sddmm(tA, tB) * _leaf(G, False)).sum().backward()
    gA, gB = tA.grad.cpu().numpy(), tB.grad.cpu().numpy()
    for b in range(batch or 1):
        sel = (lambda x: x) if batch is None else (lambda x, b=b: x[b])
        assert_twin(sel(gA), gather(oracle, op.rl, sel(G), sel(B)), f"{mode} A.grad batch {b}")
        assert_twin(sel(gB), gather(oracle, op.cl, sel(G), sel(A)), f"{mode} B.grad batch {b}")


def _entry_paths(engine, op, K):
    """per CSR entry: True where this mode's forward SDDMM reads rounded operands (dense path, or a low-precision
    residue)"""
    mode = op.mode
    if mode == engine.COMPUTE_F32:
        return np.zeros(op.nnz, dtype=bool)
    flags = np.zeros(op.nnz, dtype=np.uint8)
    assert engine.hip().bsmr_plan_dense_flags(op._plan, flags.ctypes.data_as(C.c_void_p)) == engine.OK
    lanes, lowp = C.c_uint32(0), C.c_uint32(0)
    assert engine.hip().bsmr_plan_sparse_choice(op._plan, K, mode, C.byref(lanes), C.byref(lowp)) == engine.OK
    return flags.astype(bool) | bool(lowp.value)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -20], ids=["unit", "grad-2^-20"])
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_spmm_gradients_in_every_mode(engine, mode_ops, oracle, mode, transpose, scale):
    """X.grad = spmm(values, dY) is the twin's bits.  d values = the plan's SDDMM of (dY, X) in the operator's mode: an
    entry that the mode rounds is within the forward bound (K/16 + 8) 2^-23 sum|a~||b~| of the fp64 product of the
    rounded operands a~, b~ (oracle.round_array); an fp32 entry within (K + 2) u sum|a||b| of the fp64 product.  With
    dY scaled by 2^-20 most of dY is an fp16 subnormal or zero: this pins what that model gives there."""
    op = mode_ops(mode)
    K = 64
    rng = np.random.default_rng(7 + transpose)
    rows_x, rows_y = (op.M, op.N) if transpose else (op.N, op.M)
    v = rng.uniform(-1, 1, op.nnz).astype(np.float32)
    X = rng.uniform(-1, 1, (rows_x, K)).astype(np.float32)
    H = (rng.uniform(-1, 1, (rows_y, K)) * scale).astype(np.float32)
    tv, tX = _leaf(v), _leaf(X)
    (op.spmm(tv, tX, transpose=transpose) * _leaf(H, False)).sum().backward()
    # X.grad = S_v^T H (transpose False) or S_v H (True)
    assert_twin(tX.grad.cpu().numpy(), gather(oracle, op.rl if transpose else op.cl, v, H), f"{mode} X.grad")
    # d values[t] = a[row(t)] . b[col(t)] with (a, b) = (H, X), transposed (X, H)
    a, b = (X, H) if transpose else (H, X)
    r, c = op.row_of, op.ci.astype(np.int64)
    got = tv.grad.cpu().numpy().astype(np.float64)
    rounded = _entry_paths(engine, op, K)
    exact = (a[r].astype(np.float64) * b[c]).sum(1)
    mag = (np.abs(a[r].astype(np.float64)) * np.abs(b[c])).sum(1)
    s = ~rounded
    assert (np.abs(got[s] - exact[s]) <= (K + 2) * U * mag[s] + 1e-45).all(), (mode, "fp32 entries")
    if mode in ROUND:
        assert rounded.any()
        ar, br = oracle.round_array(ROUND[mode], a), oracle.round_array(ROUND[mode], b)
        model = (ar[r].astype(np.float64) * br[c]).sum(1)
        mag_r = (np.abs(ar[r].astype(np.float64)) * np.abs(br[c])).sum(1)
        err = np.abs(got[rounded] - model[rounded])
        assert (err <= (K / 16 + 8) * 2.0 ** -23 * mag_r[rounded] + 1e-45).all(), (mode, "rounded entries", err.max())
    else:
        assert not rounded.any()


def test_empty_pattern(engine):
    """a pattern without stored entries: spmm gives zeros, and the gradients of spmm and sddmm are zeros (values of
    zero elements come with a NULL data pointer)"""
    import bsmr_torch
    M, N, K = 6, 9, 64
    csr = engine.CSR.from_arrays(M, N, np.zeros(M + 1, np.uint32), np.zeros(0, np.uint32))
    op = bsmr_torch.SparseOperator(csr, device=0)
    for transpose in (False, True):
        rows_x, rows_y = (M, N) if transpose else (N, M)
        v = torch.zeros(0, device=_dev(), requires_grad=True)
        X = torch.rand(rows_x, K, device=_dev(), requires_grad=True)
        Y = op.spmm(v, X, transpose=transpose)
        assert Y.shape == (rows_y, K) and (Y == 0).all()
        (Y * torch.rand(rows_y, K, device=_dev())).sum().backward()
        assert v.grad.shape == (0,) and (X.grad == 0).all()
    A = torch.rand(M, K, device=_dev(), requires_grad=True)
    B = torch.rand(N, K, device=_dev(), requires_grad=True)
    P = op.sddmm(A, B)
    assert P.shape == (0,)
    P.sum().backward()
    assert (A.grad == 0).all() and (B.grad == 0).all()
