"""One-pass grouped-head sparse attention on the MFMA (include/bsmr_hip.h "One-pass grouped-head sparse attention on the
MFMA") on the device, on the ladder pattern of test_gpu_attention_qkv.py (rows of 0, 1, 15, 16, 17, 33 entries:
both halves of the 32-entry tile and a second tile of one entry; 511 ... 1025: split rows), against plain fp64 numpy on the
same 16-bit inputs:
  1. the header's bound on O, m, s of every head;  2. the exact cases bit for bit;  3. the same bits call to call, each head
     its single call;  4. non-finite operands reach what the contract names and nothing else;  5. argument checks;
  6. the operator: forward bits, gradients against fp64 autograd with mfma=False as the yardstick, the refused combinations."""
import numpy as np
import pytest

from test_gpu_attention_qkv import DEV, LADDER, M, N, U, U16, _bits, _grads, _operands, _r16, _ref, op, pat  # noqa: F401
from test_gpu_attention_qkv_gqa import _call_gqa, _dense_grads, _same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _call_mfma(engine, bw, mode, Q, Kt, V, scale, g):
    """(O, m, s) of the MFMA entry: Q [b, M, K], Kt [b / g, N, K], V [b / g, N, Kv] as CPU 16-bit tensors"""
    q, k, v = (t.to(DEV) for t in (Q, Kt, V))
    O = torch.full((Q.shape[0], M, V.shape[2]), float("nan"), dtype=Q.dtype, device=DEV)   # poisoned: all is written
    m = torch.full((Q.shape[0], M), float("nan"), device=DEV)
    s = m.clone()
    engine.sparse_attention_qkv_gqa_mfma_16(bw, Q.shape[2], V.shape[2], scale, q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                            O.data_ptr(), m.data_ptr(), s.data_ptr(), Q.shape[0], g, 0, mode=mode)
    torch.cuda.synchronize()
    return O.cpu(), m.cpu().numpy(), s.cpu().numpy()


def _grouped(mode, K, Kv, g, nb=None):
    """random Q with 2 g heads (or nb), Kt and V with 2 KV heads"""
    Q, Kt, V = _operands(mode, K, Kv, "random", nb=max(nb or 2 * g, 2))
    return Q[:nb or 2 * g].clone(), Kt[:2].clone(), V[:2].clone()


def _mfma_terms(ro, ci, Q, Kt, V, scale, mode, d):
    """what the header's bound adds to _ref's before the rounding of O, per row and feature: exp(2d) (31 u + u16) sum_t
    w64_t |V[c_t]| for the value MFMA's chain and the 16-bit weights, n 2^-25 max_t |V| for fp16 weights below the normal range"""
    q, k, v = (t.double().numpy() for t in (Q, Kt, V))
    out = np.zeros((M, v.shape[1]))
    for r in range(M):
        c = ci[ro[r]:ro[r + 1]]
        if len(c):
            e = np.exp(scale * (k[c] @ q[r]) - (scale * (k[c] @ q[r])).max())
            out[r] = np.exp(2 * d[r]) * (31 * U + U16[mode]) * ((e / e.sum()) @ np.abs(v[c]))
            out[r] += len(c) * 2.0 ** -25 * np.abs(v[c]).max(0) if mode == 0 else 0.0
    return out * (1 + U16[mode])


@pytest.mark.parametrize("g", (1, 3, 8, 16, 17))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("K,Kv", ((32, 32), (96, 160), (128, 128), (256, 256)))
def test_every_head_stays_inside_the_bound(pat, K, Kv, mode, g):
    engine, bw, ro, ci = pat
    Q, Kt, V = _grouped(mode, K, Kv, g)
    scale = K ** -0.5
    O, m, s = _call_mfma(engine, bw, mode, Q, Kt, V, scale, g)
    worst = 0.0
    for h in range(2 * g):
        O64, bO, m64, d, s64, bs = _ref(ro, ci, Q[h], Kt[h // g], V[h // g], scale, mode)
        bO = bO + _mfma_terms(ro, ci, Q[h], Kt[h // g], V[h // g], scale, mode, d)
        err = np.abs(O[h].double().numpy() - O64)                          # (a missing store is NaN: not <= bO)
        worst = max(worst, float(np.divide(err, bO, out=np.zeros_like(err), where=bO > 0).max()))
        assert (err <= bO).all(), (h, worst)
        live = np.isfinite(m64)
        assert (np.abs(m[h][live] - m64[live]) <= d[live]).all() and (m[h][~live] == -np.inf).all()
        assert (np.abs(s[h] - s64) <= bs).all(), h
    print(f"K={K} Kv={Kv} mode={mode} g={g}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("K,Kv,g", ((128, 128, 3), (32, 96, 17)))
def test_exact_cases_bit_for_bit(pat, K, Kv, mode, g):
    engine, bw, ro, ci = pat
    rng = np.random.default_rng([K, Kv, g])
    Q = _r16(mode, np.zeros((2 * g, M, K)))
    Kt, V = _r16(mode, rng.integers(-2, 3, (2, N, K))), _r16(mode, rng.integers(-4, 5, (2, N, Kv)))
    O, m, s = _call_mfma(engine, bw, mode, Q, Kt, V, 0.125, g)
    lens = np.diff(ro).astype(np.float32)
    assert np.array_equal(_bits(O), _bits(_call_gqa(engine, bw, mode, Q, Kt, V, 0.125, g)[0]))   # round16(sum V / n)
    for h in range(2 * g):
        assert s[h].tobytes() == lens.tobytes() and m[h].tobytes() == np.where(lens > 0, 0, -np.inf).astype(np.float32).tobytes()
        assert not _bits(O[h][[0, 15]]).any()                             # the empty rows: +0, every bit
        assert np.array_equal(_bits(O[h][1]), _bits(V[h // g][ci[ro[1]]]))   # the one-entry row is its row of V


def test_same_bits_call_to_call_and_each_head_is_its_single_call(pat):
    engine, bw, ro, ci = pat
    Q, Kt, V = _grouped(1, 96, 160, 3)
    a, b = (_call_mfma(engine, bw, 1, Q, Kt, V, 0.3, 3) for _ in range(2))
    assert _same(a, b)
    for h in range(6):
        one = _call_mfma(engine, bw, 1, Q[h:h + 1], Kt[h // 3:h // 3 + 1], V[h // 3:h // 3 + 1], 0.3, 1)
        assert _same([x[h:h + 1] for x in a], one), h


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("poison,row", ((float("nan"), 8), (float("-inf"), 9), (float("-inf"), 3)))
def test_a_poisoned_row_of_q_stays_in_its_head(pat, mode, poison, row):
    """NaN in Q[h][row] makes that row NaN; -inf there against positive Kt makes every score of the row -inf: a dead row
    (+0, -inf, 0) beside the live rows of its group neighbours.  Everything else keeps its bits."""
    engine, bw, ro, ci = pat
    Q, Kt, V = _grouped(mode, 128, 128, 3)
    Kt[:, :, 5] = Kt[:, :, 5].abs().clamp_min(0.25)
    clean = _call_mfma(engine, bw, mode, Q, Kt, V, 0.1, 3)
    Q[4, row, 5] = poison
    O, m, s = _call_mfma(engine, bw, mode, Q, Kt, V, 0.1, 3)
    if poison != poison:
        assert torch.isnan(O[4, row]).all() and np.isnan(m[4, row]) and np.isnan(s[4, row])
    else:
        assert not _bits(O[4, row]).any() and m[4, row] == -np.inf and s[4, row] == 0
    for x, y in zip((O, m, s), clean):
        x[4, row] = y[4, row]
    assert _same((O, m, s), clean)


def test_row_0_of_kt_and_v_reaches_only_the_rows_that_store_column_0(pat):
    engine, bw, ro, ci = pat
    Q, Kt, V = _grouped(0, 96, 96, 3)
    clean = _call_mfma(engine, bw, 0, Q, Kt, V, 0.1, 3)
    Kt[:, 0], V[:, 0] = float("nan"), float("nan")
    O, m, s = _call_mfma(engine, bw, 0, Q, Kt, V, 0.1, 3)
    hit = np.array([0 in ci[ro[r]:ro[r + 1]] for r in range(M)])
    assert not hit[:6].any()                                              # the short rows pad their tile with row 0
    assert torch.isnan(O[:, hit]).all() and np.isnan(m[:, hit]).all()
    assert _same([x[:, ~hit] for x in (O, m, s)], [x[:, ~hit] for x in clean])


def test_argument_checks(pat):
    engine, bw, ro, ci = pat
    f = engine.hip().bsmr_sparse_attention_qkv_gqa_mfma_16
    p = torch.zeros(1 << 20, dtype=torch.float16, device=DEV).data_ptr()
    for g in (1, 2):                                                      # no hand-off at kv_group = 1
        assert f(bw, 288, 64, 1.0, p, p, p, p, p, p, 2, g, 0, None) == engine.ERR_UNSUPPORTED_K
        assert f(bw, 64, 288, 1.0, p, p, p, p, p, p, 2, g, 0, None) == engine.ERR_UNSUPPORTED_K
    assert f(bw, 64, 64, 1.0, p, p, p, p, p, p, 8, 0, 0, None) == engine.ERR_INVALID_ARG
    assert f(bw, 64, 64, 1.0, p, p, p, p, p, p, 8, 3, 0, None) == engine.ERR_INVALID_ARG
    assert f(bw, 64, 64, 1.0, p, p, p, p + 2, p, p, 8, 4, 0, None) == engine.ERR_INVALID_ARG


@pytest.mark.parametrize("mode,one_pass_backward", ((0, False), (1, False), (1, True)))
def test_operator_forward_and_gradients(pat, op, mode, one_pass_backward):
    engine, bw, ro, ci = pat
    g, scale = 4, 128 ** -0.5
    Q, Kt, V = _grouped(mode, 128, 128, g)
    H = _r16(mode, np.random.default_rng(7).standard_normal((8, M, 128)))
    leaves = [t.to(DEV).requires_grad_(True) for t in (Q, Kt, V)]
    how = lambda mfma: lambda q, k, v: op.attention(q, k, v, one_pass=True, one_pass_backward=one_pass_backward, mfma=mfma)
    got, yard = _grads(how(True), leaves, H.to(DEV)), _grads(how(False), leaves, H.to(DEV))
    assert np.array_equal(_bits(got[0]), _bits(_call_mfma(engine, bw, mode, Q, Kt, V, scale, g)[0]))
    for name, a, b, want in zip(("dQ", "dKt", "dV"), got[1:], yard[1:], _dense_grads(Q, Kt, V, H, ro, ci, g, scale)):
        e1, e0 = float((a.double() - want).abs().max()), float((b.double() - want).abs().max())
        print(f"mode={mode} one_pass_backward={one_pass_backward} {name}: worst error mfma {e1:.3e}, mfma=False {e0:.3e}, "
              f"ratio {e1 / e0:.3f}")
        assert e1 <= 2 * e0, (name, e1, e0)


def test_operator_refuses_what_the_mfma_form_does_not_take(op):
    Q, Kt, V = (t.to(DEV) for t in _operands(0, 64, 64, "random", nb=8))
    wide = torch.zeros(2, N, 288, dtype=torch.float16, device=DEV)
    scales = torch.zeros(2, N, 2, dtype=torch.uint8, device=DEV)
    for kw in (dict(one_pass=False), dict(blocks=True), dict(Kt=Kt[:2].to(torch.float8_e4m3fn), V=V[:2].to(torch.float8_e4m3fn)),
               dict(Kt_scale=scales, V_scale=scales), dict(V=wide), dict(Q=torch.zeros(8, M, 288, dtype=torch.float16, device=DEV), Kt=wide),
               dict(Kt=Kt, V=V), dict(Q=Q[0], Kt=Kt[0], V=V[0])):
        with pytest.raises(ValueError, match="mfma=True"):
            op.attention(**{**dict(Q=Q, Kt=Kt[:2], V=V[:2], one_pass=True, mfma=True), **kw})
