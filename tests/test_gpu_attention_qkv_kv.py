"""One-pass sparse attention on fp8, MXFP8 and MXFP4 keys and values (include/bsmr_hip.h) on the device, through
the C ABI and SparseOperator.attention(one_pass=True), on the row ladder and with the helpers of tests/test_gpu_attention_qkv.py:
  1. plain fp8: bit for bit bsmr_sparse_attention_qkv_16 on the widened operands; a batch is its single calls;
  2. MX forms on operands whose every sum is exact: m, and O and s of the one-entry row, pinned in every bit; MXFP4 equals
     MXFP8 on the e4m3 re-encoding;
  3. MX forms on random operands: DESIGN.md 19's bound against fp64 on the dequantised operands;
  4. scale code 255, an fp8 NaN code, and an inf row of V behind an all -inf leading tile;
  5. the operator: forward bits, the refusals, dQ against fp64 autograd with attention(fused=True) as the yardstick.
Measured figures: DESIGN.md 19."""
import numpy as np
import pytest

from test_gpu_attention_qkv import DEV, DT, M, N, _bits, _call as _call16, _grads, _r16, _ref, op, pat  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

E4M3, E5M2, F4 = torch.float8_e4m3fn, torch.float8_e5m2, torch.float4_e2m1fn_x2
SHAPES = ((32, 32), (96, 160), (160, 384), (512, 512))


@pytest.fixture(scope="module")
def bt(engine):
    import bsmr_torch
    return bsmr_torch


def _call(engine, bw, mode, Q, Kt, V, scale, Kts=None, Vs=None):
    """(O as a CPU 16-bit tensor, m, s as numpy) of CPU tensors: Q [b, M, K] 16-bit, Kt / V fp8 or fp4 codes, Kts / Vs uint8"""
    kt, kts, v, vs = (None if t is None else t.contiguous().view(torch.uint8).to(DEV) for t in (Kt, Kts, V, Vs))
    q, nb, K, Kv = Q.to(DEV), Q.shape[0], Q.shape[2], vs.shape[2] * 32 if Vs is not None else V.shape[2]
    O = torch.full((nb, M, Kv), float("nan"), dtype=Q.dtype, device=DEV)   # poisoned: all is written
    m = torch.full((nb, M), float("nan"), device=DEV)
    s = m.clone()
    out = (O.data_ptr(), m.data_ptr(), s.data_ptr(), nb, 0)
    torch.cuda.synchronize()
    if Kt.dtype == F4:
        engine.sparse_attention_qkv_kv4_mx(bw, K, Kv, scale, q.data_ptr(), kt.data_ptr(), kts.data_ptr(), v.data_ptr(),
                                           vs.data_ptr(), *out, mode=mode)
    elif Kts is not None:
        engine.sparse_attention_qkv_kv8_mx(bw, K, Kv, scale, q.data_ptr(), kt.data_ptr(), kts.data_ptr(), v.data_ptr(),
                                           vs.data_ptr(), *out, mode=mode, fmt=int(Kt.dtype == E5M2))
    else:
        engine.sparse_attention_qkv_kv8(bw, K, Kv, scale, q.data_ptr(), kt.data_ptr(), v.data_ptr(), *out, mode=mode,
                                        fmt=int(Kt.dtype == E5M2))
    torch.cuda.synchronize()
    return O.cpu(), m.cpu().numpy(), s.cpu().numpy()


def _same(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def _batch_is_its_single_calls(engine, bw, mode, got, Q, Kt, V, scale, Kts=None, Vs=None):
    for b in range(Q.shape[0]):
        one = _call(engine, bw, mode, *(None if t is None else t[b:b + 1] for t in (Q, Kt, V)), scale,
                    *(None if t is None else t[b:b + 1] for t in (Kts, Vs)))
        assert _same(one, tuple(x[b:b + 1] for x in got)), b


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("fmt", (E4M3, E5M2))
@pytest.mark.parametrize("K,Kv", SHAPES)
def test_plain_fp8_is_the_16_bit_call_on_the_widened_operands(pat, K, Kv, fmt, mode):
    engine, bw, ro, ci = pat
    rng = np.random.default_rng([K, Kv, mode])
    Q = _r16(mode, rng.standard_normal((2, M, K)))
    Kt, V = (torch.from_numpy(rng.standard_normal((2, N, k)).astype(np.float32)).to(fmt) for k in (K, Kv))
    got = _call(engine, bw, mode, Q, Kt, V, K ** -0.5)
    assert _same(got, _call16(engine, bw, mode, Q, Kt.to(DT[mode]), V.to(DT[mode]), K ** -0.5))
    _batch_is_its_single_calls(engine, bw, mode, got, Q, Kt, V, K ** -0.5)


def _e2m1_pack(vals):
    """integer values out of 0, +-1, 2, 3, 4, 6 as e2m1 codes, element 2i in the low nibble of byte i"""
    code = np.array([0, 2, 4, 5, 6, 0, 7])[np.abs(vals)] | np.where(vals < 0, 8, 0)
    return torch.from_numpy((code[..., 0::2] | (code[..., 1::2] << 4)).astype(np.uint8)).view(F4)


def _exact_operand(rng, k, fmt):
    """(codes, scale codes, fp64 dq) of integer-valued codes under scale codes 125 ... 129, one per block and row"""
    vals = rng.choice(np.array([-6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6]), (1, N, k))
    sc = rng.integers(125, 130, (1, N, k // 32))
    dq = vals * np.repeat(2.0 ** (sc - 127), 32, axis=2)
    codes = _e2m1_pack(vals) if fmt == F4 else torch.from_numpy(vals.astype(np.float32)).to(fmt)
    return codes, torch.from_numpy(sc.astype(np.uint8)), dq, vals


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("fmt", (E4M3, E5M2, F4))
@pytest.mark.parametrize("K,Kv", SHAPES)
def test_mx_forms_on_exact_operands(pat, K, Kv, fmt, mode):
    engine, bw, ro, ci = pat
    rng = np.random.default_rng([K, Kv])
    q = rng.integers(-4, 5, (1, M, K))
    (Kt, Kts, dk, kvals), (V, Vs, dv, vvals) = _exact_operand(rng, K, fmt), _exact_operand(rng, Kv, fmt)
    got = _call(engine, bw, mode, _r16(mode, q), Kt, V, 2.0 ** -3, Kts, Vs)
    z = 2.0 ** -3 * (q[0].astype(np.float64) @ dk[0].T)                    # every term and sum exact in fp32
    want_m = np.array([z[r, ci[ro[r]:ro[r + 1]]].max(initial=-np.inf) for r in range(M)], np.float32)
    assert got[1][0].tobytes() == want_m.tobytes()
    assert got[2][0, 1] == 1.0 and np.array_equal(_bits(got[0][0, 1]), _bits(_r16(mode, dv[0, ci[ro[1]]])))   # the one-entry row
    if fmt == F4:   # every e2m1 value is an e4m3 value: the same call on the re-encoded codes
        k8, v8 = (torch.from_numpy(x.astype(np.float32)).to(E4M3) for x in (kvals, vvals))
        assert _same(got, _call(engine, bw, mode, _r16(mode, q), k8, v8, 2.0 ** -3, Kts, Vs))


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("fmt", (E4M3, E5M2, F4))
@pytest.mark.parametrize("K,Kv", SHAPES)
def test_mx_forms_stay_inside_the_bound(pat, bt, K, Kv, fmt, mode):
    engine, bw, ro, ci = pat
    rng = np.random.default_rng([K, Kv, mode, 19])
    Q = _r16(mode, rng.standard_normal((2, M, K)))
    (Kt, Kts), (V, Vs) = (bt.mx_quantize(torch.from_numpy(rng.standard_normal((2, N, k)).astype(np.float32)), fmt) for k in (K, Kv))
    scale = K ** -0.5
    got = _call(engine, bw, mode, Q, Kt, V, scale, Kts, Vs)
    (O, m, s), worst = got, 0.0
    for b in range(2):   # DESIGN.md 18's bound, evaluated on the dequantised operands
        O64, bO, m64, d, s64, bs = _ref(ro, ci, Q[b], bt.mx_dequantize(Kt[b], Kts[b], torch.float64),
                                        bt.mx_dequantize(V[b], Vs[b], torch.float64), scale, mode)
        err = np.abs(O[b].double().numpy() - O64)
        worst = max(worst, float(np.divide(err, bO, out=np.zeros_like(err), where=bO > 0).max()))   # (empty rows: 0 / 0)
        print(f"K={K} Kv={Kv} mode={mode} {fmt} b={b}: worst error / bound = {worst:.3f}")
        assert (err <= bO).all(), (b, worst)
        live = np.isfinite(m64)
        assert (np.abs(m[b][live] - m64[live]) <= d[live]).all() and (m[b][~live] == -np.inf).all()
        assert (np.abs(s[b] - s64) <= bs).all(), float((np.abs(s[b] - s64)[live] / bs[live]).max())
    _batch_is_its_single_calls(engine, bw, mode, got, Q, Kt, V, scale, Kts, Vs)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("fmt,what", ((E4M3, "scale"), (F4, "scale"), (E4M3, "code"), (E4M3, "plain code")))
def test_a_nan_scale_or_code_poisons_exactly_the_rows_that_read_it(pat, bt, fmt, what, mode):
    engine, bw, ro, ci = pat
    rng = np.random.default_rng(4)
    Q = _r16(mode, rng.standard_normal((1, M, 128)))
    (Kt, Kts), (V, Vs) = (bt.mx_quantize(torch.from_numpy(rng.standard_normal((1, N, 128)).astype(np.float32)), fmt) for _ in "kv")
    if what == "plain code":
        Kts = Vs = None
    clean = _call(engine, bw, mode, Q, Kt, V, 0.1, Kts, Vs)
    col = int(ci[ro[9] + 1020])                                           # read by the third chunk of the 1025-entry row
    if what == "scale":
        Kts = Kts.clone()
        Kts[0, col, 2] = 255
    else:
        Kt = Kt.clone()
        Kt.view(torch.uint8)[0, col, 77] = 0x7F                           # an e4m3 NaN code
    O, m, s = _call(engine, bw, mode, Q, Kt, V, 0.1, Kts, Vs)
    hit = np.array([col in ci[ro[r]:ro[r + 1]] for r in range(M)])
    assert hit.any() and not hit.all() and torch.isnan(O[0][hit]).all() and np.isnan(m[0][hit]).all()   # the softmax flag
    assert np.array_equal(_bits(O[0][~hit]), _bits(clean[0][0][~hit])) and m[0][~hit].tobytes() == clean[1][0][~hit].tobytes()


@pytest.mark.parametrize("mx", (False, True))
def test_an_inf_row_of_v_behind_a_leading_tile_of_minus_inf_does_not_reach_o(pat, mx):
    engine, bw, ro, ci = pat
    rng = np.random.default_rng(5)
    q = rng.standard_normal((1, M, 64))
    q[0, :, 0] = -1.0
    k, v = rng.standard_normal((1, N, 64)), rng.standard_normal((1, N, 64))
    lead, last = ci[ro[4]:ro[4] + 16], int(ci[ro[4] + 16])                # the 17-entry row: one full tile, then one entry
    k[0, lead] = 0.0
    k[0, lead, 0] = np.inf                                                # e5m2 has infinities: these scores are -inf
    v[0, lead] = np.inf
    Kt, V = (torch.from_numpy(x.astype(np.float32)).to(E5M2) for x in (k, v))
    Kts = Vs = torch.full((1, N, 2), 127, dtype=torch.uint8) if mx else None
    O, m, s = _call(engine, bw, 1, _r16(1, q), Kt, V, 0.5, Kts, Vs)
    assert np.isfinite(m[0, 4]) and s[0, 4] == 1.0 and np.array_equal(_bits(O[0, 4]), _bits(V[0, last].to(torch.bfloat16)))


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("fmt,mx", ((E5M2, False), (E4M3, True), (F4, True)))
def test_operator_forward_and_dq(pat, op, bt, fmt, mx, mode):
    engine, bw, ro, ci = pat
    rng = np.random.default_rng(11)
    Q, H = (_r16(mode, rng.standard_normal((2, M, 128))) for _ in "qh")
    quant = lambda x: bt.mx_quantize(x, fmt) if mx else (x.to(fmt), None)
    (Kt, Kts), (V, Vs) = (quant(torch.from_numpy(rng.standard_normal((2, N, 128)).astype(np.float32))) for _ in "kv")
    dev = lambda t: None if t is None else t.to(DEV)
    leaf = [Q.to(DEV).requires_grad_(True)]
    kw = dict(Kt_scale=dev(Kts), V_scale=dev(Vs))
    one = _grads(lambda q: op.attention(q, dev(Kt), dev(V), one_pass=True, **kw), leaf, H.to(DEV))
    raw = _call(engine, bw, mode, Q, Kt, V, 128 ** -0.5, Kts, Vs)[0]
    assert np.array_equal(_bits(one[0]), _bits(raw))
    fused = _grads(lambda q: op.attention(q, dev(Kt), dev(V), fused=True, **kw), leaf, H.to(DEV))
    # fp64 autograd of the dense masked attention on the dequantised operands
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[np.repeat(np.arange(M), np.diff(ro)), ci] = True
    q64 = Q.double().requires_grad_(True)
    k64, v64 = ((bt.mx_dequantize(c, sc, torch.float64) if mx else c.double()) for c, sc in ((Kt, Kts), (V, Vs)))
    z = (q64 @ k64.transpose(-1, -2)) * 128 ** -0.5
    top = z.detach().masked_fill(~mask, -np.inf).amax(-1, keepdim=True)
    e = torch.exp((z - torch.where(torch.isfinite(top), top, torch.zeros_like(top))).masked_fill(~mask, -np.inf))
    ((e / e.sum(-1, keepdim=True).clamp_min(1e-300)) @ v64 * H.double()).sum().backward()
    e1, ef = (float((g[1].double() - q64.grad).abs().max()) for g in (one, fused))
    print(f"mode={mode} {fmt} mx={mx} dQ: worst error one_pass {e1:.3e}, fused {ef:.3e}, ratio {e1 / ef:.3f}")
    assert e1 <= 2 * ef, (e1, ef)


def test_operator_refusals(op, bt):
    x = torch.zeros(N, 64, device=DEV)
    Q, K16 = torch.zeros(M, 64, dtype=torch.float16, device=DEV), x.half()
    k8, k5, (k4, s4) = x.to(E4M3), x.to(E5M2), (t.to(DEV) for t in bt.mx_quantize(x.cpu(), F4))
    s8 = torch.full((N, 2), 127, dtype=torch.uint8, device=DEV)
    for kw in (dict(Kt=k8, V=K16), dict(Kt=K16, V=k8), dict(Kt=k8, V=k5), dict(Kt=k4, V=k8, Kt_scale=s4),   # mixed formats
               dict(Kt=k8, V=k8, Kt_scale=s8), dict(Kt=k8, V=k8, V_scale=s8),                               # one fp8 scale
               dict(Kt=k4, V=k4), dict(Kt=k4, V=k4, Kt_scale=s4),                                           # fp4 without its scales
               dict(Kt=k8, V=k8, out_dtype=torch.float16), dict(Kt=k8, V=k8, fused=True), dict(Q=Q.float(), Kt=k8, V=k8),
               dict(Kt=k8.clone().requires_grad_(True), V=k8), dict(Kt=k8, V=k8.clone().requires_grad_(True)),
               dict(Kt=k4.view(torch.uint8).clone().view(F4).requires_grad_(True), V=k4, Kt_scale=s4, V_scale=s4),
               dict(Kt=torch.zeros(N, 544, device=DEV).to(E4M3), V=k8, Q=torch.zeros(M, 544, dtype=torch.float16, device=DEV))):
        with pytest.raises(ValueError):
            op.attention(**{**dict(Q=Q, Kt=k8, V=k8, one_pass=True), **kw})
    with pytest.raises(ValueError, match="one_pass=False"):
        op.attention(Q, k8, K16, one_pass=True)
