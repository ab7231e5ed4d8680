"""One-pass sparse attention over the RPHM's blocks on the device (include/bsmr_hip.h "One-pass sparse attention over
blocks"), through the C ABI and SparseOperator.attention(one_pass=True, blocks=True), against numpy / torch
fp64 on the same 16-bit inputs.  Pattern: tests/blocked_twin.py's (panels of 0 - 5 blocks, empty cells, a ragged panel, a
residue row of three chunks, empty rows), attached whole (segment_blocks 0) and in segments of 2 blocks."""
import numpy as np
import pytest

import blocked_twin as bt

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -24
DT = {0: torch.float16, 1: torch.bfloat16}
U16 = {0: 2.0 ** -11, 1: 2.0 ** -8}
DEV = "cuda:0"
M, N, RO, CI = bt.blocked_pattern()
RO64, CI64 = RO.astype(np.int64), CI.astype(np.int64)


class Handle:
    def __init__(self, engine, S, delta=0.3):
        csr = engine.CSR.from_arrays(M, N, RO, CI)
        self.arrays = a = engine.Pipeline(csr, alpha=0.3, delta=delta, device=-1).arrays()
        self.bw = engine.backward_create(M, N, RO, CI, row_order=a["reorderedRows"], device=0)
        engine.backward_attach_blocks(self.bw, M, N, CI.size, a, S)
        # per row: blocks of its panel, units it is cut into, residue entries
        rr, bo = a["reorderedRows"].astype(np.int64), a["blockOffsets"].astype(np.int64)
        self.blocks, self.units = np.zeros(M, np.int64), np.zeros(M, np.int64)
        for p in range(bo.size - 1):
            nb = bo[p + 1] - bo[p]
            self.blocks[rr[16 * p:16 * p + 16]] = nb
            self.units[rr[16 * p:16 * p + 16]] = (-(-nb // S) if S else 1) if nb else 0
        self.residue = np.diff(bt.residue_lists(M, RO, CI, a)[0].astype(np.int64))


@pytest.fixture(scope="module")
def handles(engine):
    hs = {0: Handle(engine, 0), 2: Handle(engine, 2), "none": Handle(engine, 0, delta=1.0)}
    st = engine.backward_blocked_stats(hs[2].bw)
    assert st["split_panels"] >= 5 and st["padding_columns"] > 0 and hs[0].residue.max() > 2 * bt.CHUNK
    assert engine.backward_blocked_stats(hs["none"].bw)["blocks"] == 0
    yield hs
    for h in hs.values():
        engine.backward_destroy(h.bw)


def _call(engine, bw, mode, Q, Kt, V, scale, blocked=True):
    """(O [b, M, Kv] as a CPU 16-bit tensor, m, s [b, M] as numpy) of CPU 16-bit tensors Q [b, M, K], Kt, V"""
    q, k, v = (t.to(DEV) for t in (Q, Kt, V))
    O = torch.full((Q.shape[0], M, V.shape[2]), float("nan"), dtype=Q.dtype, device=DEV)   # poisoned: all is written
    m = torch.full((Q.shape[0], M), float("nan"), device=DEV)
    s = m.clone()
    f = engine.sparse_attention_qkv_blocked_16 if blocked else engine.sparse_attention_qkv_16
    f(bw, Q.shape[2], V.shape[2], scale, q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(), m.data_ptr(), s.data_ptr(),
      Q.shape[0], 0, mode=mode)
    torch.cuda.synchronize()
    return O.cpu(), m.cpu().numpy(), s.cpu().numpy()


def _same(a, b):
    return (np.array_equal(a[0].view(torch.int16).numpy(), b[0].view(torch.int16).numpy())
            and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes())


def _r16(mode, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[mode])


def _operands(mode, K, Kv, nb=2):
    rng = np.random.default_rng([K, Kv, mode])
    return tuple(_r16(mode, rng.standard_normal(shape)) for shape in ((nb, M, K), (nb, N, K), (nb, N, Kv)))


def _ref(h, Q, Kt, V, scale, mode):
    """fp64 attention of one batch on the 16-bit values and the header's bounds: O64, bound(O), m64, d, s64, bound(s)"""
    q, k, v = (t.double().numpy() for t in (Q, Kt, V))
    K = q.shape[1]
    O64, m64, s64 = np.zeros((M, v.shape[1])), np.full(M, -np.inf), np.zeros(M)
    bO, d, bs = np.zeros_like(O64), np.zeros(M), np.zeros(M)
    for r in range(M):
        c = CI64[RO64[r]:RO64[r + 1]]
        if len(c) == 0:
            continue
        z = scale * (k[c] @ q[r])
        d[r] = abs(scale) * (K + 1) * U * (np.abs(k[c]) @ np.abs(q[r])).max()
        m64[r] = z.max()
        e = np.exp(z - m64[r])
        s64[r] = e.sum()
        O64[r] = (e / s64[r]) @ v[c]
        res = h.residue[r]
        n, T = 16 * h.blocks[r] + res, h.blocks[r] + -(-res // 16)
        P = max(-(-res // bt.CHUNK) + h.units[r], 1)
        Zr, g = m64[r] - z.min() + 2 * d[r], np.exp(2 * d[r])
        bO[r] = (((g - 1) + g * (2 * n + 2 * P + 6 * T + 2 * Zr + 13) * U) * ((e / s64[r]) @ np.abs(v[c]))
                 + (n + P + 2 * T + 2) * 2.0 ** -126 * np.abs(v[c]).max(0))
        bs[r] = ((g - 1) + g * (n + P + 3 * T + Zr + 7) * U) * s64[r]
    bO = bO + U16[mode] * (np.abs(O64) + bO) + (2.0 ** -25 if mode == 0 else 0.0)   # the one rounding of O
    return O64, bO, m64, d, s64, bs


@pytest.mark.parametrize("S", (0, 2))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("K,Kv", ((32, 32), (96, 160), (160, 384), (512, 512)))
def test_forward_stays_inside_the_bound(engine, handles, K, Kv, mode, S):
    h = handles[S]
    Q, Kt, V = _operands(mode, K, Kv)
    scale = K ** -0.5
    got = _call(engine, h.bw, mode, Q, Kt, V, scale)
    assert _same(got, _call(engine, h.bw, mode, Q, Kt, V, scale))                      # call to call
    worst = [0.0, 0.0, 0.0]
    fails = []
    for b in range(2):
        O64, bO, m64, d, s64, bs = _ref(h, Q[b], Kt[b], V[b], scale, mode)
        live = np.isfinite(m64)
        eO, em, es = np.abs(got[0][b].double().numpy() - O64), np.abs(got[1][b][live] - m64[live]), np.abs(got[2][b] - s64)
        for i, (err, bound) in enumerate(((eO, bO), (em, d[live]), (es[live], bs[live]))):
            worst[i] = max(worst[i], float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max()))
            fails.append(bool((err > bound).any()))
        assert (got[1][b][~live] == -np.inf).all() and (got[2][b][~live] == 0).all()
        one = _call(engine, h.bw, mode, Q[b:b + 1], Kt[b:b + 1], V[b:b + 1], scale)        # the batch is its single call
        assert _same(tuple(x[0] for x in one), tuple(x[b] for x in got))
    print(f"K={K} Kv={Kv} mode={mode} S={S}: worst error / bound  O {worst[0]:.3f}  m {worst[1]:.3f}  s {worst[2]:.3f}")
    assert not any(fails), worst


@pytest.mark.parametrize("S", (0, 2))
@pytest.mark.parametrize("mode", (0, 1))
def test_equal_scores_are_exact(engine, handles, mode, S):
    h = handles[S]
    K, Kv = 96, 160
    v = np.random.default_rng(Kv).integers(-4, 5, (N, Kv))
    Q, Kt, V = torch.zeros(1, M, K, dtype=DT[mode]), _operands(mode, K, Kv, nb=1)[1], _r16(mode, v[None])
    got = _call(engine, h.bw, mode, Q, Kt, V, 0.25)
    assert _same(got, _call(engine, h.bw, mode, Q, Kt, V, 0.25, blocked=False))
    lens = np.diff(RO64)
    assert got[2][0].tobytes() == lens.astype(np.float32).tobytes()
    assert np.array_equal(got[1][0], np.where(lens > 0, 0.0, -np.inf).astype(np.float32))
    assert not got[0][0][torch.from_numpy(lens == 0)].view(torch.int16).any()                             # +0, every bit


@pytest.mark.parametrize("mode", (0, 1))
def test_handle_without_blocks_gives_the_one_pass_bits(engine, handles, mode):
    h = handles["none"]
    Q, Kt, V = _operands(mode, 160, 96)
    assert _same(_call(engine, h.bw, mode, Q, Kt, V, 0.1), _call(engine, h.bw, mode, Q, Kt, V, 0.1, blocked=False))


@pytest.mark.parametrize("S", (0, 2))
def test_mask_by_select_and_the_empty_cell_rule(engine, handles, S):
    h = handles[S]
    a = h.arrays
    dc, bv = a["denseCols"].reshape(-1, 16), a["blockValues"].reshape(-1, 16, 16)
    bo, rr = a["blockOffsets"].astype(np.int64), a["reorderedRows"].astype(np.int64)
    # a block column with an empty and a stored cell among the rows that exist
    p, blk, j = next((p, b, j) for p in range(bo.size - 1) for b in range(bo[p], bo[p + 1]) for j in range(16)
                     if dc[b, j] != N and 0 < (bv[b, :min(16, rr.size - 16 * p), j] == bt.NULL).sum() < min(16, rr.size - 16 * p))
    c, kf = int(dc[blk, j]), 37
    row_of = np.repeat(np.arange(M), np.diff(RO64))
    storing = np.zeros(M, bool)
    storing[row_of[CI64 == c]] = True
    # rows with an empty cell at c in a unit in which they store another cell: the empty-cell rule reaches them
    ruled = np.zeros(M, bool)
    for q in range(bo.size - 1):
        step = S or max(int(bo[q + 1] - bo[q]), 1)
        for u0 in range(bo[q], bo[q + 1], step):
            u1 = min(u0 + step, bo[q + 1])
            if (dc[u0:u1] == c).any():
                rows = rr[16 * q:16 * q + 16]
                ruled[rows[(bv[u0:u1, :rows.size] != bt.NULL).any(axis=(0, 2))]] = True
    ruled &= ~storing
    assert storing.any() and ruled.any() and (~storing & ~ruled).any()
    storing, ruled = torch.from_numpy(storing), torch.from_numpy(ruled)
    Q, Kt, V = _operands(0, 64, 64, nb=1)
    clean = _call(engine, h.bw, 0, Q, Kt, V, 0.125)[0][0]
    Ktn, Vn = Kt.clone(), V.clone()
    Ktn[0, c, 9] = float("nan")
    got = _call(engine, h.bw, 0, Q, Ktn, V, 0.125)[0][0]
    assert torch.isnan(got[storing]).all() and torch.equal(got[~storing].view(torch.int16), clean[~storing].view(torch.int16))
    Vn[0, c, kf] = float("inf")
    got = _call(engine, h.bw, 0, Q, Kt, Vn, 0.125)[0][0]
    assert torch.isinf(got[storing, kf]).all() and torch.isnan(got[ruled, kf]).all()
    rest = ~storing & ~ruled
    assert torch.equal(got[rest].view(torch.int16), clean[rest].view(torch.int16))
    got[:, kf] = clean[:, kf]
    assert torch.equal(got.view(torch.int16), clean.view(torch.int16))                  # no other feature moved


def test_reserve_then_no_allocation_and_the_argument_checks(engine, handles):
    h, hip = handles[2], engine.hip()
    engine.sparse_attention_qkv_blocked_reserve(h.bw, 512, 512, 2)
    before = engine.backward_stats(h.bw)["workspace_bytes"]
    _call(engine, h.bw, 1, *_operands(1, 512, 512), 0.1)
    assert engine.backward_stats(h.bw)["workspace_bytes"] == before
    buf = torch.zeros(1 << 21, dtype=torch.float16, device=DEV)
    p = buf.data_ptr()
    f = hip.bsmr_sparse_attention_qkv_blocked_16
    assert f(h.bw, 48, 64, 1.0, p, p, p, p, p, p, 1, 0, None) == engine.ERR_UNSUPPORTED_K
    assert f(h.bw, 64, 544, 1.0, p, p, p, p, p, p, 1, 0, None) == engine.ERR_UNSUPPORTED_K
    assert f(h.bw, 64, 64, 1.0, p, p, p, p, p, p, 1, engine.COMPUTE_F32, None) == engine.ERR_INVALID_ARG
    assert f(h.bw, 64, 64, float("inf"), p, p, p, p, p, p, 1, 0, None) == engine.ERR_INVALID_ARG
    assert f(h.bw, 64, 64, 1.0, p, p + 2, p, p, p, p, 1, 0, None) == engine.ERR_INVALID_ARG
    assert f(h.bw, 64, 64, 1.0, p, p, p, None, p, p, 1, 0, None) == engine.ERR_INVALID_ARG
    plain = engine.backward_create(M, N, RO, CI, device=0)
    assert f(plain, 64, 64, 1.0, p, p, p, p, p, p, 1, 0, None) == engine.ERR_BAD_PLAN
    assert hip.bsmr_sparse_attention_qkv_blocked_reserve(plain, 64, 64, 1) == engine.ERR_BAD_PLAN
    engine.backward_destroy(plain)


# ---- torch: SparseOperator(blocked=True).attention(one_pass=True, blocks=True) ----------------------------------------
@pytest.fixture(scope="module")
def op(engine):
    import bsmr_torch
    return bsmr_torch.SparseOperator(engine.CSR.from_arrays(M, N, RO, CI), device=0, blocked=True, segment_blocks=2)


def _grads(how, leaves, H):
    out = how(*leaves)
    (out * H).sum().backward()
    got = [out.detach().cpu()] + [t.grad.detach().cpu() for t in leaves]
    for t in leaves:
        t.grad = None
    return got


@pytest.mark.parametrize("batch", (None, 2))
@pytest.mark.parametrize("mode", (0, 1))
def test_operator_forward_and_gradients(engine, op, mode, batch):
    Q, Kt, V = (t if batch else t[0] for t in _operands(mode, 128, 128))
    H = _r16(mode, np.random.default_rng(7).standard_normal(Q.shape[:-2] + (M, 128))).to(DEV)
    leaves = [t.to(DEV).requires_grad_(True) for t in (Q, Kt, V)]
    blk = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True, blocks=True), leaves, H)
    raw = _call(engine, op._bw, mode, *(t.reshape((-1,) + t.shape[-2:]) for t in (Q, Kt, V)), 128 ** -0.5)[0]
    assert torch.equal(blk[0].view(torch.int16), raw.reshape(blk[0].shape).view(torch.int16))
    one = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True), leaves, H)
    off = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True, blocks=False), leaves, H)
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(one, off))   # blocks=False: today's bits
    # fp64 autograd of the dense masked attention from the same 16-bit tensors
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[np.repeat(np.arange(M), np.diff(RO64)), CI64] = True
    ref = [t.double().requires_grad_(True) for t in (Q, Kt, V)]
    z = (ref[0] @ ref[1].transpose(-1, -2)) * 128 ** -0.5
    top = z.detach().masked_fill(~mask, -np.inf).amax(-1, keepdim=True)
    e = torch.exp((z - torch.where(torch.isfinite(top), top, torch.zeros_like(top))).masked_fill(~mask, -np.inf))
    ((e / e.sum(-1, keepdim=True).clamp_min(1e-300)) @ ref[2] * H.cpu().double()).sum().backward()
    for name, gb, g1, want in zip(("dQ", "dKt", "dV"), blk[1:], one[1:], ref):
        eb, e1 = float((gb.double() - want.grad).abs().max()), float((g1.double() - want.grad).abs().max())
        print(f"mode={mode} batch={batch} {name}: worst error blocks {eb:.3e}, one_pass {e1:.3e}, ratio {eb / e1:.3f}")
        assert eb <= 2 * e1, (name, eb, e1)


def test_operator_limits(engine, op):
    import bsmr_torch
    Q, Kt, V = (t[0].to(DEV) for t in _operands(0, 64, 64))
    sc = torch.zeros(N, 2, dtype=torch.uint8, device=DEV)
    for kw in (dict(one_pass=False), dict(fused=True), dict(out_dtype=torch.float16), dict(Kt_scale=sc), dict(V_scale=sc),
               dict(Kt=Kt.to(torch.float8_e4m3fn), V=V.to(torch.float8_e4m3fn)), dict(V=V.bfloat16()), dict(Q=Q.float())):
        with pytest.raises(ValueError):
            op.attention(**{**dict(Q=Q, Kt=Kt, V=V, one_pass=True, blocks=True), **kw})
    plain = bsmr_torch.SparseOperator(engine.CSR.from_arrays(M, N, RO, CI), device=0)
    with pytest.raises(ValueError):
        plain.attention(Q, Kt, V, one_pass=True, blocks=True)
