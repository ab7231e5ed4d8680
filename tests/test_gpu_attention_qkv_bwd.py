"""One-pass backward of sparse attention (include/bsmr_hip.h "One-pass backward of sparse attention") on the
device, with the helpers of tests/test_gpu_attention_qkv.py:
  1. SparseOperator.attention(one_pass=True, one_pass_backward=True): the forward's bits, the same gradient bits step to step,
     and each gradient against fp64 torch autograd of the dense masked attention on the same 16-bit values - the worst error
     at most 2x that of one_pass=True's default backward (the factor test_operator_forward_and_gradients allows);
  2. the C call: every row written, +0 for empty rows and columns, each batch its single call, NULL outputs, the reserve, a NaN;
  3. refusals, and the default path's bits.
Pattern: 1536 x 1536, a ladder in both directions - rows 0-15 hold 0, 1, 15, 16, 17, 33 (the tile edges), 511, 512, 513 (one
chunk, two chunks), 1025 (three chunks) ... entries in columns >= 16, columns 0-15 the same counts in rows >= 16.
Measured on an MI355X: the ratio new / default of test 1 is 1.000 for dQ, dKt and dV in all twelve cases."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_attention_qkv import DEV, LADDER, _bits, _grads, _r16   # noqa: E402

M = N = 1536
SLOTS = 5   # chunk slots of either direction: 513 -> 2, 1025 -> 3


@pytest.fixture(scope="module")
def pat(engine):
    import bsmr_torch
    rng = np.random.default_rng(21)
    r = np.concatenate([np.full(n, i) for i, n in enumerate(LADDER)] + [16 + rng.choice(N - 16, n, replace=False) for n in LADDER])
    c = np.concatenate([16 + rng.choice(N - 16, n, replace=False) for n in LADDER] + [np.full(n, j) for j, n in enumerate(LADDER)])
    order = np.lexsort((c, r))
    ro = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=M))]).astype(np.uint32)
    ci = c[order].astype(np.uint32)
    bw = engine.backward_create(M, N, ro, ci, device=0)
    st = engine.backward_stats(bw)
    assert st["chunk"] == 512 and st["split_rows"] == 2 and st["split_cols"] == 2
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[r, c] = True
    op = bsmr_torch.SparseOperator(engine.CSR.from_arrays(M, N, ro, ci), device=0)
    yield engine, bw, op, mask, (ro, ci)
    engine.backward_destroy(bw)


def _operands(mode, K, Kv, nb):
    rng = np.random.default_rng([K, Kv, mode])
    shapes = ((M, K), (N, K), (N, Kv), (M, Kv))   # Q, Kt, V and the cotangent H
    return [_r16(mode, rng.standard_normal((nb,) + s if nb else s)) for s in shapes]


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("K,Kv", ((32, 32), (64, 256), (96, 160), (128, 128), (256, 256), (160, 224)))
def test_gradients_through_the_operator(pat, K, Kv, mode):
    engine, bw, op, mask, _ = pat
    Q, Kt, V, H = _operands(mode, K, Kv, 2 if (K, Kv) == (128, 128) else None)
    leaves = [t.to(DEV).requires_grad_(True) for t in (Q, Kt, V)]
    new = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True, one_pass_backward=True), leaves, H.to(DEV))
    again = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True, one_pass_backward=True), leaves, H.to(DEV))
    old = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True), leaves, H.to(DEV))
    assert np.array_equal(_bits(new[0]), _bits(old[0]))                       # the forward is one_pass=True's
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(new, again))
    # fp64 autograd of the dense masked attention from the same 16-bit tensors
    ref = [t.double().requires_grad_(True) for t in (Q, Kt, V)]
    z = (ref[0] @ ref[1].transpose(-1, -2)) * K ** -0.5
    top = z.detach().masked_fill(~mask, -np.inf).amax(-1, keepdim=True)
    e = torch.exp((z - torch.where(torch.isfinite(top), top, torch.zeros_like(top))).masked_fill(~mask, -np.inf))
    ((e / e.sum(-1, keepdim=True).clamp_min(1e-300)) @ ref[2] * H.double()).sum().backward()
    for name, g1, g0, want in zip(("dQ", "dKt", "dV"), new[1:], old[1:], ref):
        e1, e0 = float((g1.double() - want.grad).abs().max()), float((g0.double() - want.grad).abs().max())
        print(f"K={K} Kv={Kv} mode={mode} {name}: worst error one_pass_backward {e1:.3e}, default {e0:.3e}, ratio {e1 / e0:.3f}")
        assert e1 <= 2 * e0, (name, e1, e0)


def _forward(engine, bw, mode, Q, Kt, V, scale):
    """(O, m, s) on the device of device tensors Q [b, M, K], Kt, V"""
    O = torch.empty((Q.shape[0], M, V.shape[2]), dtype=Q.dtype, device=DEV)
    m = torch.empty((Q.shape[0], M), device=DEV)
    s = torch.empty_like(m)
    engine.sparse_attention_qkv_16(bw, Q.shape[2], V.shape[2], scale, Q.data_ptr(), Kt.data_ptr(), V.data_ptr(), O.data_ptr(),
                                   m.data_ptr(), s.data_ptr(), Q.shape[0], 0, mode=mode)
    return O, m, s


def _backward(engine, bw, mode, Q, Kt, V, H, scale, want=(True, True, True)):
    """[dQ, dKt, dV] as CPU tensors (None where not wanted) of CPU 16-bit tensors; the outputs start as NaN"""
    q, k, v, h = (t.to(DEV) for t in (Q, Kt, V, H))
    O, m, s = _forward(engine, bw, mode, q, k, v, scale)
    out = [torch.full_like(t, float("nan")) if w else None for t, w in zip((q, k, v), want)]
    engine.sparse_attention_qkv_backward_16(bw, Q.shape[2], V.shape[2], scale, q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                            O.data_ptr(), h.data_ptr(), m.data_ptr(), s.data_ptr(),
                                            *(0 if t is None else t.data_ptr() for t in out), Q.shape[0], 0, mode=mode)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu() for t in out]


@pytest.mark.parametrize("mode", (0, 1))
def test_the_c_call(pat, mode):
    engine, _, op, mask, csr = pat
    K = Kv = 128
    Q, Kt, V, H = _operands(mode, K, Kv, 2)
    bw = engine.backward_create(M, N, *csr, device=0)   # a fresh workspace
    engine.sparse_attention_qkv_backward_reserve(bw, K, Kv, 2)
    reserved = engine.backward_stats(bw)["workspace_bytes"]
    assert reserved == 4 * 2 * (M + SLOTS * K + SLOTS * (K + Kv))
    both = _backward(engine, bw, mode, Q, Kt, V, H, 0.1)
    assert engine.backward_stats(bw)["workspace_bytes"] == reserved
    rows, cols = mask.any(1), mask.any(0)
    assert not rows.all() and not cols.all()
    for g, live in zip(both, (rows, cols, cols)):
        assert not torch.isnan(g).any() and (_bits(g[:, ~live]) == 0).all()           # every row written, +0 without entries
    for b in range(2):                                                                # each batch is its single call
        one = _backward(engine, bw, mode, *(t[b:b + 1] for t in (Q, Kt, V, H)), 0.1)
        assert all(np.array_equal(_bits(a[0]), _bits(g[b])) for a, g in zip(one, both))
    dQ, _, _ = _backward(engine, bw, mode, Q, Kt, V, H, 0.1, want=(True, False, False))
    _, dKt, dV = _backward(engine, bw, mode, Q, Kt, V, H, 0.1, want=(False, True, True))
    assert all(np.array_equal(_bits(a), _bits(g)) for a, g in zip((dQ, dKt, dV), both))
    Qn = Q.clone()
    Qn[0, 8, 77] = float("nan")                                                       # the two-chunk row
    hit = (torch.arange(M) == 8, mask[8], mask[8])
    for g, clean, h in zip(_backward(engine, bw, mode, Qn, Kt, V, H, 0.1), both, hit):
        assert h.any() and torch.isnan(g[0][h]).all()
        assert np.array_equal(_bits(g[0][~h]), _bits(clean[0][~h])) and np.array_equal(_bits(g[1]), _bits(clean[1]))
    engine.backward_destroy(bw)


def test_refusals_and_the_default_path(pat):
    engine, bw, op, _, _ = pat
    f = engine.hip().bsmr_sparse_attention_qkv_backward_16
    buf = torch.zeros(1 << 20, dtype=torch.float16, device=DEV)
    p = buf.data_ptr()
    assert f(bw, 48, 64, 1.0, *[p] * 10, 1, 0, None) == engine.ERR_UNSUPPORTED_K
    assert f(bw, 64, 288, 1.0, *[p] * 10, 1, 0, None) == engine.ERR_UNSUPPORTED_K
    assert engine.hip().bsmr_sparse_attention_qkv_backward_reserve(bw, 64, 288, 1) == engine.ERR_UNSUPPORTED_K
    assert f(bw, 64, 64, float("nan"), *[p] * 10, 1, 0, None) == engine.ERR_INVALID_ARG
    for i in (7, 8, 9):                                                               # a misaligned output
        assert f(bw, 64, 64, 1.0, *[p + 2 * (j == i) for j in range(10)], 1, 0, None) == engine.ERR_INVALID_ARG
    Q, Kt, V, H = (t.to(DEV) for t in _operands(0, 64, 64, None))
    wide = torch.zeros(M, 288, dtype=torch.float16, device=DEV)
    for kw in (dict(one_pass=False), dict(Kt=Kt.to(torch.float8_e4m3fn), V=V.to(torch.float8_e4m3fn)), dict(blocks=True),
               dict(Q=wide, Kt=wide)):
        with pytest.raises(ValueError, match="one_pass_backward=True"):
            op.attention(**{**dict(Q=Q, Kt=Kt, V=V, one_pass=True, one_pass_backward=True), **kw})
    leaves = [t.requires_grad_(True) for t in (Q, Kt, V)]
    a = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True), leaves, H)
    b = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True, one_pass_backward=False), leaves, H)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
