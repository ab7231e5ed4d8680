"""One-pass sparse attention (include/bsmr_hip.h "One-pass sparse attention") on the device, through the C ABI
and SparseOperator.attention(one_pass=True), against plain numpy / torch fp64 on the same 16-bit inputs:
  1. the header's bound on O, m and s for random, ascending and descending scores; each batch is its single call;
  2. exact inputs: O = round16(fl(sum V) / n), s = n, m = fl(scale q.k0) bit for bit; empty and one-entry rows;
  3. a NaN in Q or Kt poisons exactly the rows that read it;  4. reproducibility and the reserve;  5. argument checks;
  6. the operator: forward bits, gradients against fp64 autograd with attention(fused=True) as the yardstick.
Pattern: 16 rows over 1536 columns; rows of 0, 1, 15, 16, 17, 33 (the tile edges), 511, 512, 513 (one chunk, two chunks),
1025 (three chunks) and a few more."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -24
DT = {0: torch.float16, 1: torch.bfloat16}
U16 = {0: 2.0 ** -11, 1: 2.0 ** -8}
LADDER = (0, 1, 15, 16, 17, 33, 511, 512, 513, 1025, 7, 100, 64, 300, 2, 0)
M, N, DEV = len(LADDER), 1536, "cuda:0"


@pytest.fixture(scope="module")
def pat(engine):
    rng = np.random.default_rng(18)
    ci = np.concatenate([np.sort(rng.choice(N, n, replace=False)) for n in LADDER]).astype(np.uint32)
    ro = np.concatenate([[0], np.cumsum(LADDER)]).astype(np.uint32)
    bw = engine.backward_create(M, N, ro, ci, device=0)
    st = engine.backward_stats(bw)
    assert st["chunk"] == 512 and st["split_rows"] == 2 and st["row_items"] == 14 + 2 + 3   # 513: 2 chunks, 1025: 3
    yield engine, bw, ro.astype(np.int64), ci.astype(np.int64)
    engine.backward_destroy(bw)


def _call(engine, bw, mode, Q, Kt, V, scale, stream=0):
    """(O [b, M, Kv] as a CPU 16-bit tensor, m, s [b, M] as numpy) of CPU 16-bit tensors Q [b, M, K], Kt, V"""
    q, k, v = (t.to(DEV) for t in (Q, Kt, V))
    O = torch.full((Q.shape[0], M, V.shape[2]), float("nan"), dtype=Q.dtype, device=DEV)   # poisoned: all is written
    m = torch.full((Q.shape[0], M), float("nan"), device=DEV)
    s = m.clone()
    torch.cuda.synchronize()
    engine.sparse_attention_qkv_16(bw, Q.shape[2], V.shape[2], scale, q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(),
                                   m.data_ptr(), s.data_ptr(), Q.shape[0], stream, mode=mode)
    torch.cuda.synchronize()
    return O.cpu(), m.cpu().numpy(), s.cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int16).numpy()


def _r16(mode, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[mode])


def _ref(ro, ci, Q, Kt, V, scale, mode):
    """fp64 attention of one batch on the 16-bit values and the header's bounds: O64, bound(O), m64, d, s64, bound(s)"""
    q, k, v = (t.double().numpy() for t in (Q, Kt, V))
    K = q.shape[1]
    O64, m64, s64 = np.zeros((M, v.shape[1])), np.full(M, -np.inf), np.zeros(M)
    bO, d, bs = np.zeros_like(O64), np.zeros(M), np.zeros(M)
    for r in range(M):
        c = ci[ro[r]:ro[r + 1]]
        n = len(c)
        if n == 0:
            continue
        z = scale * (k[c] @ q[r])
        d[r] = abs(scale) * (K + 1) * U * (np.abs(k[c]) @ np.abs(q[r])).max()
        m64[r] = z.max()
        e = np.exp(z - m64[r])
        s64[r] = e.sum()
        O64[r] = (e / s64[r]) @ v[c]
        Zr, T, g = m64[r] - z.min() + 2 * d[r], min(-(-n // 16), 32), np.exp(2 * d[r])
        bO[r] = (((g - 1) + g * (2 * n + 6 * T + 2 * Zr + 13) * U) * ((e / s64[r]) @ np.abs(v[c]))
                 + (n + 2 * T + 2) * 2.0 ** -126 * np.abs(v[c]).max(0))
        bs[r] = ((g - 1) + g * (n + 3 * T + Zr + 7) * U) * s64[r]
    bO = bO + U16[mode] * (np.abs(O64) + bO) + (2.0 ** -25 if mode == 0 else 0.0)   # the one rounding of O
    return O64, bO, m64, d, s64, bs


def _operands(mode, K, Kv, order, nb=2):
    rng = np.random.default_rng([K, Kv, mode, len(order)])
    V = _r16(mode, rng.standard_normal((nb, N, Kv)))
    if order == "random":
        return _r16(mode, rng.standard_normal((nb, M, K))), _r16(mode, rng.standard_normal((nb, N, K))), V
    # monotone along every row: Kt[c] = g(c) k0 with g rising or falling in c, Q[r] = a_r k0 with a_r > 0
    k0 = rng.standard_normal((nb, 1, K))
    g = np.linspace(0.5, 1.5, N) if order == "ascending" else np.linspace(1.5, 0.5, N)
    return _r16(mode, rng.uniform(0.3, 0.6, (nb, M, 1)) * k0), _r16(mode, g[None, :, None] * k0), V


@pytest.mark.parametrize("order", ("random", "ascending", "descending"))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("K,Kv", ((32, 32), (64, 256), (96, 160), (128, 128), (512, 512), (160, 384)))
def test_forward_stays_inside_the_bound(pat, K, Kv, mode, order):
    engine, bw, ro, ci = pat
    Q, Kt, V = _operands(mode, K, Kv, order)
    scale = K ** -0.5
    O, m, s = _call(engine, bw, mode, Q, Kt, V, scale)
    worst = 0.0
    for b in range(2):
        O64, bO, m64, d, s64, bs = _ref(ro, ci, Q[b], Kt[b], V[b], scale, mode)
        err = np.abs(O[b].double().numpy() - O64)
        worst = max(worst, float(np.divide(err, bO, out=np.zeros_like(err), where=bO > 0).max()))   # (empty rows: 0 / 0)
        assert (err <= bO).all(), (b, worst)
        live = np.isfinite(m64)
        assert (np.abs(m[b][live] - m64[live]) <= d[live]).all() and (m[b][~live] == -np.inf).all()
        assert (np.abs(s[b] - s64) <= bs).all(), float((np.abs(s[b] - s64)[live] / bs[live]).max())
        O1, m1, s1 = _call(engine, bw, mode, Q[b:b + 1], Kt[b:b + 1], V[b:b + 1], scale)       # the batch is its single call
        assert np.array_equal(_bits(O1[0]), _bits(O[b]))
        assert m1[0].tobytes() == m[b].tobytes() and s1[0].tobytes() == s[b].tobytes()
    print(f"K={K} Kv={Kv} mode={mode} {order}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("K,Kv", ((128, 128), (32, 512)))
def test_equal_scores_are_exact(pat, K, Kv, mode):
    engine, bw, ro, ci = pat
    rng = np.random.default_rng([K, Kv])
    q, k0 = rng.integers(-2, 3, (M, K)), rng.integers(-1, 2, K)
    v = rng.integers(-4, 5, (N, Kv))
    Q, Kt, V = _r16(mode, q[None]), _r16(mode, np.broadcast_to(k0, (1, N, K))), _r16(mode, v[None])
    O, m, s = _call(engine, bw, mode, Q, Kt, V, 2.0 ** -3)
    lens = np.diff(ro)
    sums = np.stack([v[ci[ro[r]:ro[r + 1]]].sum(0) for r in range(M)]).astype(np.float32)
    want = _r16(mode, sums / np.maximum(lens, 1).astype(np.float32)[:, None])
    assert np.array_equal(_bits(O[0]), _bits(want))                       # (empty rows: +0, every bit)
    assert np.array_equal(s[0], lens.astype(np.float32))
    want_m = np.where(lens > 0, np.float32(2.0 ** -3) * (q @ k0).astype(np.float32), -np.inf).astype(np.float32)
    assert m[0].tobytes() == want_m.tobytes()
    assert np.array_equal(_bits(O[0][1]), _bits(V[0][ci[ro[1]]]))         # the one-entry row is its row of V


@pytest.mark.parametrize("mode", (0, 1))
def test_a_nan_poisons_exactly_the_rows_that_read_it(pat, mode):
    engine, bw, ro, ci = pat
    Q, Kt, V = _operands(mode, 128, 128, "random", nb=1)
    clean = _call(engine, bw, mode, Q, Kt, V, 0.1)[0][0]
    col = int(ci[ro[9] + 1020])                                           # read by the third chunk of the 1025-entry row
    Qn, Ktn = Q.clone(), Kt.clone()
    Qn[0, 8, 77] = float("nan")                                           # the two-chunk row
    Ktn[0, col, 5] = float("nan")
    for got, hit in ((_call(engine, bw, mode, Qn, Kt, V, 0.1)[0][0], np.arange(M) == 8),
                     (_call(engine, bw, mode, Q, Ktn, V, 0.1)[0][0],
                      np.array([col in ci[ro[r]:ro[r + 1]] for r in range(M)]))):
        assert hit.any() and torch.isnan(got[hit]).all()
        assert np.array_equal(_bits(got[~hit]), _bits(clean[~hit]))


def test_same_bits_call_to_call_and_no_allocation_after_reserve(pat):
    engine, bw, ro, ci = pat
    Q, Kt, V = _operands(1, 96, 160, "random")
    engine.sparse_attention_qkv_reserve(bw, 96, 160, 2)
    before = engine.backward_stats(bw)["workspace_bytes"]
    assert before >= 2 * 5 * (160 + 2) * 4
    a = _call(engine, bw, 1, Q, Kt, V, 0.3)
    b = _call(engine, bw, 1, Q, Kt, V, 0.3, stream=torch.cuda.Stream(DEV).cuda_stream)
    assert engine.backward_stats(bw)["workspace_bytes"] == before
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_argument_checks(pat):
    engine, bw, ro, ci = pat
    f = engine.hip().bsmr_sparse_attention_qkv_16
    buf = torch.zeros(1 << 20, dtype=torch.float16, device=DEV)
    p = buf.data_ptr()
    for bad in (0, 48, 544):
        assert f(bw, bad, 64, 1.0, p, p, p, p, p, p, 1, 0, None) == engine.ERR_UNSUPPORTED_K
        assert f(bw, 64, bad, 1.0, p, p, p, p, p, p, 1, 0, None) == engine.ERR_UNSUPPORTED_K
        assert engine.hip().bsmr_sparse_attention_qkv_reserve(bw, bad, 64, 1) == engine.ERR_UNSUPPORTED_K
    assert f(bw, 64, 64, 1.0, p, p, p, p, p, p, 1, engine.COMPUTE_F32, None) == engine.ERR_INVALID_ARG
    assert f(bw, 64, 64, float("inf"), p, p, p, p, p, p, 1, 0, None) == engine.ERR_INVALID_ARG
    assert f(None, 64, 64, 1.0, p, p, p, p, p, p, 1, 0, None) == engine.ERR_INVALID_ARG
    for i in range(6):                                                    # each pointer 2 bytes off, then NULL
        for q in (p + 2, None):
            args = [p] * 6
            args[i] = q
            assert f(bw, 64, 64, 1.0, *args, 1, 0, None) == engine.ERR_INVALID_ARG, (i, q)
    O = torch.full((4, 64), float("nan"), dtype=torch.float16, device=DEV)
    m = torch.full((4,), float("nan"), device=DEV)
    s = m.clone()
    assert f(bw, 64, 64, 1.0, p, p, p, O.data_ptr(), m.data_ptr(), s.data_ptr(), 0, 0, None) == engine.OK   # no batch: no-op
    torch.cuda.synchronize()
    assert torch.isnan(O).all() and torch.isnan(m).all()
    empty = engine.backward_create(4, 8, np.zeros(5, np.uint32), np.zeros(0, np.uint32), device=0)
    assert f(empty, 64, 64, 1.0, None, None, None, O.data_ptr(), m.data_ptr(), s.data_ptr(), 1, 0, None) == engine.OK
    torch.cuda.synchronize()
    assert (O.view(torch.int16) == 0).all() and (m == -np.inf).all() and (s == 0).all()
    engine.backward_destroy(empty)


@pytest.fixture(scope="module")
def op(pat):
    import bsmr_torch
    engine, bw, ro, ci = pat
    return bsmr_torch.SparseOperator(engine.CSR.from_arrays(M, N, ro.astype(np.uint32), ci.astype(np.uint32)), device=0)


def _grads(how, leaves, H):
    out = how(*leaves)
    (out * H).sum().backward()
    got = [out.detach().cpu()] + [t.grad.detach().cpu() for t in leaves]
    for t in leaves:
        t.grad = None
    return got


@pytest.mark.parametrize("batch", (None, 2))
@pytest.mark.parametrize("mode", (0, 1))
def test_operator_forward_and_gradients(pat, op, mode, batch):
    engine, bw, ro, ci = pat
    Q, Kt, V = (t if batch else t[0] for t in _operands(mode, 128, 128, "random"))
    H = _r16(mode, np.random.default_rng(7).standard_normal(Q.shape[:-2] + (M, 128)))
    leaves = [t.to(DEV).requires_grad_(True) for t in (Q, Kt, V)]
    one = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True), leaves, H.to(DEV))
    raw = _call(engine, bw, mode, *(t.reshape((-1,) + t.shape[-2:]) for t in (Q, Kt, V)), 128 ** -0.5)[0]
    assert np.array_equal(_bits(one[0]), _bits(raw.reshape(one[0].shape)))
    again = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True), leaves, H.to(DEV))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(one, again))
    fused = _grads(lambda q, k, v: op.attention(q, k, v, fused=True), leaves, H.to(DEV))
    # fp64 autograd of the dense masked attention from the same 16-bit tensors
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[np.repeat(np.arange(M), np.diff(ro)), ci] = True
    ref = [t.double().requires_grad_(True) for t in (Q, Kt, V)]
    z = (ref[0] @ ref[1].transpose(-1, -2)) * 128 ** -0.5
    top = z.detach().masked_fill(~mask, -np.inf).amax(-1, keepdim=True)
    e = torch.exp((z - torch.where(torch.isfinite(top), top, torch.zeros_like(top))).masked_fill(~mask, -np.inf))
    ((e / e.sum(-1, keepdim=True).clamp_min(1e-300)) @ ref[2] * H.double()).sum().backward()
    for name, g1, gf, want in zip(("dQ", "dKt", "dV"), one[1:], fused[1:], ref):
        e1, ef = float((g1.double() - want.grad).abs().max()), float((gf.double() - want.grad).abs().max())
        print(f"mode={mode} batch={batch} {name}: worst error one_pass {e1:.3e}, fused {ef:.3e}, ratio {e1 / ef:.3f}")
        assert e1 <= 2 * ef, (name, e1, ef)


def test_operator_limits_and_the_default_path(op):
    Q, Kt, V = (t[0].to(DEV) for t in _operands(0, 64, 64, "random"))
    for kw in (dict(Q=Q.float()), dict(Kt=Kt.to(torch.float8_e4m3fn)), dict(V=V.bfloat16()), dict(out_dtype=torch.float16), dict(fused=True),
               dict(Kt_scale=torch.zeros(N, 2, dtype=torch.uint8, device=DEV)),
               dict(V_scale=torch.zeros(N, 2, dtype=torch.uint8, device=DEV)),
               dict(Q=torch.zeros(M, 544, dtype=torch.float16, device=DEV), Kt=torch.zeros(N, 544, dtype=torch.float16, device=DEV))):
        with pytest.raises(ValueError):
            op.attention(**{**dict(Q=Q, Kt=Kt, V=V, one_pass=True), **kw})
    a, b = op.attention(Q, Kt, V), op.attention(Q, Kt, V, one_pass=False)
    c = op.spmm(op.softmax(op.sddmm(Q, Kt), 64 ** -0.5), V)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(a.view(torch.int16), c.view(torch.int16))
