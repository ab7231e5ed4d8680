"""bsmr_torch.SparseOperator.softmax and .attention as torch autograd functions on the engine, against dense masked fp64
torch, on a pattern with empty rows (their attention rows are 0); two runs of the attention step give the same gradient
bits, which a softmax built on index_add does not promise."""
import math

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def op(engine):
    import bsmr_torch
    rows, cols, ro, ci = synth.random_pattern(256, 384, 12000, seed=5, empty_rows=19)
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    o = bsmr_torch.SparseOperator(csr, mode=engine.COMPUTE_F32, device=0)
    o.rows_t = torch.from_numpy(np.repeat(np.arange(rows), np.diff(ro.astype(np.int64)))).cpu()
    o.cols_t = torch.from_numpy(ci.astype(np.int64)).cpu()
    o.has_row = torch.from_numpy(np.diff(ro.astype(np.int64)) > 0)
    assert (~o.has_row).sum() == 19
    o.mask = torch.zeros(rows, cols, dtype=torch.bool)
    o.mask[o.rows_t, o.cols_t] = True
    return o


def _rand(*shape, seed, requires_grad=True, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).to(_dev()).requires_grad_(requires_grad)


def _masked_softmax(op, S):
    """row softmax of dense (..., M, N) fp64 scores over S's pattern; rows without entries are 0"""
    fill = torch.where(op.has_row[:, None], float("-inf"), 0.0).to(S.dtype)
    W = torch.softmax(torch.where(op.mask, S, fill), dim=-1)
    return W * op.has_row[:, None].to(S.dtype)


@pytest.mark.parametrize("batch", [None, 3])
def test_softmax_gradients(op, batch):
    lead = () if batch is None else (batch,)
    scale = 0.6
    v = _rand(*lead, op.nnz, seed=1, scale=8.0)
    G = _rand(*lead, op.nnz, seed=2, requires_grad=False)
    W = op.softmax(v, scale)
    (W * G).sum().backward()

    v64 = v.detach().double().cpu().requires_grad_(True)
    dense = lambda t: torch.zeros(op.M, op.N, dtype=torch.float64).index_put((op.rows_t, op.cols_t), t)
    D = dense(v64) if batch is None else torch.stack([dense(v64[b]) for b in range(batch)])
    Wr = _masked_softmax(op, D * scale)[..., op.rows_t, op.cols_t]
    (Wr * G.double().cpu()).sum().backward()
    got = W.detach().double().cpu()
    assert torch.allclose(got, Wr.detach(), rtol=2e-5, atol=1e-7), float((got - Wr).abs().max())
    g, w = v.grad.double().cpu(), v64.grad
    assert torch.allclose(g, w, rtol=1e-4, atol=1e-5 * float(w.abs().max())), float((g - w).abs().max())


def _attention_step(op, leaves, H, batch):
    Q, Kk, V = leaves[0], leaves[1:3], leaves[3:5]
    x = Q
    for i in range(2):
        x = op.attention(x, Kk[i], V[i])   # V is 96 wide, K 64: the second layer's query is 96 wide too
    (x * H).sum().backward()
    return [t.grad.detach().clone() for t in leaves]


def _leaves(op, batch):
    lead = () if batch is None else (batch,)
    return ([_rand(*lead, op.M, 64, seed=21)] + [_rand(*lead, op.N, 64 if i == 0 else 96, seed=22 + i) for i in range(2)]
            + [_rand(*lead, op.N, 96, seed=24 + i) for i in range(2)])


@pytest.mark.parametrize("batch", [None, 2])
def test_two_layer_attention_step(op, batch):
    """attention twice (the first layer's output is the second's query), against dense masked fp64 torch with the rows
    of empty rows set to 0; then a second run gives bitwise-equal gradients"""
    leaves = _leaves(op, batch)
    lead = () if batch is None else (batch,)
    H = _rand(*lead, op.M, 96, seed=26, requires_grad=False)
    grads = _attention_step(op, leaves, H, batch)

    ref = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    x = ref[0]
    for i in range(2):
        K = x.shape[-1]
        s = (x @ ref[1 + i].transpose(-1, -2)) * K ** -0.5
        x = _masked_softmax(op, s) @ ref[3 + i]
    (x * H.double().cpu()).sum().backward()
    for got, want in zip(grads, ref):
        g, w = got.double().cpu(), want.grad
        assert torch.allclose(g, w, rtol=1e-4, atol=1e-5 * float(w.abs().max())), float((g - w).abs().max())

    for t in leaves:
        t.grad = None
    again = _attention_step(op, leaves, H, batch)
    for a, b in zip(grads, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_empty_rows_give_zero_attention(op):
    Q = _rand(op.M, 32, seed=31, requires_grad=False)
    Kt = _rand(op.N, 32, seed=32, requires_grad=False)
    V = _rand(op.N, 64, seed=33, requires_grad=False)
    O = op.attention(Q, Kt, V, scale=2.0).cpu()
    assert (O[~op.has_row] == 0).all() and (O[op.has_row].abs().sum(-1) > 0).all()


def test_bad_inputs_raise_value_error(op):
    v = torch.zeros(op.nnz, device=_dev())
    for bad in (v.half(), v.cpu(), v[:-1], torch.zeros(op.nnz, 2, device=_dev()).T, torch.zeros(0, op.nnz, device=_dev()),
                v.view(1, 1, -1), v.tolist()):
        with pytest.raises(ValueError):
            op.softmax(bad)
    for scale in (float("nan"), math.inf, "x"):
        with pytest.raises(ValueError):
            op.softmax(v, scale)
    Q = torch.zeros(op.M, 64, device=_dev())
    Kt = torch.zeros(op.N, 64, device=_dev())
    with pytest.raises(ValueError):
        op.attention(Q, Kt, torch.zeros(op.N, 48, device=_dev()))          # V width not a multiple of 32
    with pytest.raises(ValueError):
        op.attention(Q, Kt, torch.zeros(2, op.N, 64, device=_dev()))       # batch mismatch
    with pytest.raises(ValueError):
        op.attention(Q, torch.zeros(op.N, 32, device=_dev()), torch.zeros(op.N, 64, device=_dev()))   # K mismatch
    with pytest.raises(ValueError):
        op.attention(Q, Kt, torch.zeros(op.M, 64, device=_dev()))          # V wants N rows
