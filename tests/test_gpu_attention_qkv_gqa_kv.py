"""One-pass grouped-head sparse attention on fp8, MXFP8 and MXFP4 keys and values (include/bsmr_hip.h) on the
device, on the ladder pattern of test_gpu_attention_qkv.py (tile edges, split rows):
  1. the contract: O, m, s are the bits of the ungrouped _kv8 / _kv8_mx / _kv4_mx call on repeat_interleaved codes and scales;
  2. non-finite operands with dead, NaN and live heads of one group side by side; a NaN scale code stays in its group;
  3. every head inside DESIGN.md 19's bound against fp64 on the dequantised operands;  4. argument checks;
  5. the operator: forward bits, dQ against fp64 autograd with one_pass=True on repeated codes and scales as the yardstick,
     and the refused combinations."""
import numpy as np
import pytest

from test_gpu_attention_qkv import DEV, M, N, _bits, _grads, _r16, _ref, op, pat  # noqa: F401
from test_gpu_attention_qkv_gqa import _dense_grads, _same
from test_gpu_attention_qkv_kv import E4M3, E5M2, F4, _call, bt  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FORMS = ((E4M3, False), (E5M2, False), (E4M3, True), (E5M2, True), (F4, True))


def _call_gqa(engine, bw, mode, Q, Kt, V, scale, g, Kts=None, Vs=None):
    """_call through the grouped entries: Q [b, M, K] 16-bit, codes and scales with b / g heads, CPU tensors"""
    kt, kts, v, vs = (None if t is None else t.contiguous().view(torch.uint8).to(DEV) for t in (Kt, Kts, V, Vs))
    q, nb, K, Kv = Q.to(DEV), Q.shape[0], Q.shape[2], Vs.shape[2] * 32 if Vs is not None else V.shape[2]
    O = torch.full((nb, M, Kv), float("nan"), dtype=Q.dtype, device=DEV)   # poisoned: all is written
    m = torch.full((nb, M), float("nan"), device=DEV)
    s = m.clone()
    out = (O.data_ptr(), m.data_ptr(), s.data_ptr(), nb, g, 0)
    if Kt.dtype == F4:
        engine.sparse_attention_qkv_gqa_kv4_mx(bw, K, Kv, scale, q.data_ptr(), kt.data_ptr(), kts.data_ptr(), v.data_ptr(),
                                               vs.data_ptr(), *out, mode=mode)
    elif Kts is not None:
        engine.sparse_attention_qkv_gqa_kv8_mx(bw, K, Kv, scale, q.data_ptr(), kt.data_ptr(), kts.data_ptr(), v.data_ptr(),
                                               vs.data_ptr(), *out, mode=mode, fmt=int(Kt.dtype == E5M2))
    else:
        engine.sparse_attention_qkv_gqa_kv8(bw, K, Kv, scale, q.data_ptr(), kt.data_ptr(), v.data_ptr(), *out, mode=mode,
                                            fmt=int(Kt.dtype == E5M2))
    torch.cuda.synchronize()
    return O.cpu(), m.cpu().numpy(), s.cpu().numpy()


def _rep(t, g):
    """repeat_interleave along the head axis; codes move as bytes"""
    return None if t is None else t.view(torch.uint8).repeat_interleave(g, 0).view(t.dtype)


def _cache(bt, rng, heads, k, fmt, mx):
    """(codes, scales or None) of `heads` random KV heads of k features"""
    x = torch.from_numpy(rng.standard_normal((heads, N, k)).astype(np.float32))
    return bt.mx_quantize(x, fmt) if mx else (x.to(fmt), None)


@pytest.mark.parametrize("g", (2, 3, 8, 16))
@pytest.mark.parametrize("K,Kv", ((32, 32), (96, 160), (256, 256)))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("fmt,mx", FORMS)
def test_bits_of_the_ungrouped_call_on_repeated_codes_and_scales(pat, bt, fmt, mx, mode, K, Kv, g):
    engine, bw, ro, ci = pat
    rng = np.random.default_rng([K, Kv, mode, g])
    Q = _r16(mode, rng.standard_normal((2 * g, M, K)))
    (Kt, Kts), (V, Vs) = _cache(bt, rng, 2, K, fmt, mx), _cache(bt, rng, 2, Kv, fmt, mx)
    got = _call_gqa(engine, bw, mode, Q, Kt, V, K ** -0.5, g, Kts, Vs)
    want = _call(engine, bw, mode, Q, _rep(Kt, g), _rep(V, g), K ** -0.5, _rep(Kts, g), _rep(Vs, g))
    assert not torch.isnan(want[0]).any() and _same(got, want)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("case", ("inf", "scale"))
def test_non_finite_operands_heads_side_by_side(pat, bt, case, mode):
    engine, bw, ro, ci = pat
    g, rng = 4, np.random.default_rng(24)
    q = rng.standard_normal((8, M, 128))
    if case == "inf":
        # Unscaled e5m2: feature 5 of Kt is +inf on every column of the 15- and the 16-entry row and of the first tile of the
        # 511-entry row, and Q's sign there alternates from head to head: an even head sees +inf (NaN rows), its odd neighbour
        # -inf - dead rows, and a first tile met while m = -inf whose rows of V hold inf.
        first = ci[ro[6]:ro[6] + 16]
        hot = np.unique(np.concatenate([ci[ro[2]:ro[3]], ci[ro[3]:ro[4]], first]))
        q[:, :, 5] = np.maximum(np.abs(q[:, :, 5]), 0.25) * np.tile([1.0, -1.0], 4)[:, None]
        k, v = rng.standard_normal((2, N, 128)), rng.standard_normal((2, N, 128))
        k[:, hot, 5] = np.inf
        v[:, first[::3], 1] = np.inf
        v[1, first[1::3], 7] = -np.inf
        (Kt, V), Kts, Vs = (torch.from_numpy(x.astype(np.float32)).to(E5M2) for x in (k, v)), None, None
    else:
        (Kt, Kts), (V, Vs) = _cache(bt, rng, 2, 128, E4M3, True), _cache(bt, rng, 2, 128, E4M3, True)
        col = int(ci[ro[9] + 1020])                                       # read by the third chunk of the 1025-entry row
        Kts[1, col, 2] = 255
    Q = _r16(mode, q)
    got = _call_gqa(engine, bw, mode, Q, Kt, V, 0.1, g, Kts, Vs)
    want = _call(engine, bw, mode, Q, _rep(Kt, g), _rep(V, g), 0.1, _rep(Kts, g), _rep(Vs, g))
    if case == "inf":
        assert torch.isnan(want[0][0::2, 3]).all() and (want[1][1::2, 3] == -np.inf).all()   # NaN and dead heads side by side
        assert np.isfinite(want[1][1::2, 6]).all() and not torch.isnan(want[0][1::2, 6]).any()   # the per-head skip
    else:
        hit = np.array([col in ci[ro[r]:ro[r + 1]] for r in range(M)])
        nan = torch.isnan(want[0]).any(-1).numpy()
        assert hit.any() and not hit.all() and (nan[4:] == hit).all() and not nan[:4].any()
    assert _same(got, want)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("fmt", (E4M3, F4))
def test_every_head_stays_inside_the_bound(pat, bt, fmt, mode):
    engine, bw, ro, ci = pat
    g, scale, rng = 4, 128 ** -0.5, np.random.default_rng([mode, 24])
    Q = _r16(mode, rng.standard_normal((8, M, 128)))
    (Kt, Kts), (V, Vs) = _cache(bt, rng, 2, 128, fmt, True), _cache(bt, rng, 2, 128, fmt, True)
    O, m, s = _call_gqa(engine, bw, mode, Q, Kt, V, scale, g, Kts, Vs)
    k64, v64 = bt.mx_dequantize(Kt, Kts, torch.float64), bt.mx_dequantize(V, Vs, torch.float64)
    for h in range(8):   # DESIGN.md 18's bound, evaluated on the dequantised operands
        O64, bO, m64, d, s64, bs = _ref(ro, ci, Q[h], k64[h // g], v64[h // g], scale, mode)
        err = np.abs(O[h].double().numpy() - O64)
        assert (err <= bO).all(), (h, float(np.divide(err, bO, out=np.zeros_like(err), where=bO > 0).max()))
        live = np.isfinite(m64)
        assert (np.abs(m[h][live] - m64[live]) <= d[live]).all() and (m[h][~live] == -np.inf).all()
        assert (np.abs(s[h] - s64) <= bs).all(), float((np.abs(s[h] - s64)[live] / bs[live]).max())


@pytest.mark.parametrize("name,pointers,tail", (("bsmr_sparse_attention_qkv_gqa_kv8", 6, (0, 0, None)),
                                               ("bsmr_sparse_attention_qkv_gqa_kv8_mx", 8, (0, 0, None)),
                                               ("bsmr_sparse_attention_qkv_gqa_kv4_mx", 8, (0, None))))
def test_argument_checks(pat, name, pointers, tail):
    engine, bw, ro, ci = pat
    f = getattr(engine.hip(), name)
    p = torch.zeros(1 << 20, dtype=torch.float16, device=DEV).data_ptr()
    ins = [p] * (pointers - 3)
    assert f(bw, 64, 64, 1.0, *ins, p, p, p, 8, 0, *tail) == engine.ERR_INVALID_ARG
    assert f(bw, 64, 64, 1.0, *ins, p, p, p, 8, 3, *tail) == engine.ERR_INVALID_ARG
    for bad in (288, 512):
        assert f(bw, bad, 64, 1.0, *ins, p, p, p, 2, 2, *tail) == engine.ERR_UNSUPPORTED_K
        assert f(bw, 64, bad, 1.0, *ins, p, p, p, 2, 2, *tail) == engine.ERR_UNSUPPORTED_K
    O = torch.full((4, 64), float("nan"), dtype=torch.float16, device=DEV)
    assert f(bw, 64, 64, 1.0, *ins, O.data_ptr(), p, p, 0, 2, *tail) == engine.OK   # no batch: no-op
    torch.cuda.synchronize()
    assert torch.isnan(O).all()


def test_a_group_of_one_is_the_ungrouped_call(pat, bt):
    engine, bw, ro, ci = pat
    rng = np.random.default_rng(1)
    Q = _r16(1, rng.standard_normal((2, M, 512)))                         # kv_group = 1: K up to 512
    (Kt, Kts), (V, Vs) = _cache(bt, rng, 2, 512, E4M3, True), _cache(bt, rng, 2, 64, E4M3, True)
    assert _same(_call_gqa(engine, bw, 1, Q, Kt, V, 0.05, 1, Kts, Vs), _call(engine, bw, 1, Q, Kt, V, 0.05, Kts, Vs))


@pytest.mark.parametrize("fmt", (E4M3, F4))
def test_operator_forward_and_dq(pat, op, bt, fmt):
    engine, bw, ro, ci = pat
    g, scale, rng = 4, 128 ** -0.5, np.random.default_rng(11)
    Q, H = (_r16(0, rng.standard_normal((8, M, 128))) for _ in "qh")
    (Kt, Kts), (V, Vs) = _cache(bt, rng, 2, 128, fmt, True), _cache(bt, rng, 2, 128, fmt, True)
    leaf = [Q.to(DEV).requires_grad_(True)]
    run = lambda kt, v, kts, vs: _grads(lambda q: op.attention(q, kt.to(DEV), v.to(DEV), one_pass=True, Kt_scale=kts.to(DEV),
                                                               V_scale=vs.to(DEV)), leaf, H.to(DEV))
    grouped, repeated = run(Kt, V, Kts, Vs), run(*(_rep(t, g) for t in (Kt, V, Kts, Vs)))
    assert np.array_equal(_bits(grouped[0]), _bits(_call_gqa(engine, bw, 0, Q, Kt, V, scale, g, Kts, Vs)[0]))
    want = _dense_grads(Q, bt.mx_dequantize(Kt, Kts, torch.float64), bt.mx_dequantize(V, Vs, torch.float64), H, ro, ci, g, scale)[0]
    e1, e0 = (float((t[1].double() - want).abs().max()) for t in (grouped, repeated))
    print(f"{fmt} dQ: worst error grouped {e1:.3e}, repeated {e0:.3e}")
    assert e1 <= e0, (e1, e0)   # the same backward on the same values


def test_operator_refusals(op, bt):
    Q = torch.zeros(8, M, 64, dtype=torch.float16, device=DEV)
    x = torch.zeros(2, N, 64)
    k8, (k4, s4) = x.to(E4M3).to(DEV), (t.to(DEV) for t in bt.mx_quantize(x, F4))
    s8 = torch.full((2, N, 2), 127, dtype=torch.uint8, device=DEV)
    wide, swide = torch.zeros(2, N, 288, device=DEV).to(E4M3), torch.full((2, N, 9), 127, dtype=torch.uint8, device=DEV)
    ok = dict(Q=Q, Kt=k8, V=k8, Kt_scale=s8, V_scale=s8, one_pass=True)
    assert op.attention(**ok).shape == (8, M, 64)
    for kw in (dict(Kt_scale=None, V_scale=None),                         # unscaled fp8: the C call's, not the operator's
               dict(one_pass_backward=True), dict(blocks=True), dict(V=wide, V_scale=swide),
               dict(Q=torch.zeros(8, M, 288, dtype=torch.float16, device=DEV), Kt=wide, Kt_scale=swide),
               dict(Kt_scale=None), dict(V_scale=None), dict(Kt=k4, V=k4, Kt_scale=s4, V_scale=None),
               dict(Kt=k8.clone().requires_grad_(True)),
               dict(Kt=k4, V=k4.view(torch.uint8).clone().view(F4).requires_grad_(True), Kt_scale=s4, V_scale=s4)):
        with pytest.raises(ValueError):
            op.attention(**{**ok, **kw})
