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
