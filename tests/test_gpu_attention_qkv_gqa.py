"""One-pass sparse attention with grouped key/value heads (include/bsmr_hip.h "One-pass sparse attention with grouped
key/value heads") on the device, on the ladder pattern of test_gpu_attention_qkv.py (tile edges, split rows):
  1. the contract: O, m, s are the bits of bsmr_sparse_attention_qkv_16 on repeat_interleaved Kt and V, for random operands
     and for operands whose heads of one group are dead (-inf), NaN and live side by side;
  2. every head inside DESIGN.md 18's bound against fp64;  3. argument checks;  4. the operator: forward bits, gradients
     against fp64 autograd with one_pass=True on repeat_interleaved leaves as the yardstick, and the refused combinations."""
import numpy as np
import pytest

from test_gpu_attention_qkv import DEV, DT, LADDER, M, N, _bits, _call, _grads, _operands, _r16, _ref, op, pat  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _call_gqa(engine, bw, mode, Q, Kt, V, scale, g):
    """_call through the grouped entry: Q [b, M, K], Kt [b / g, N, K], V [b / g, N, Kv] as CPU 16-bit tensors"""
    q, k, v = (t.to(DEV) for t in (Q, Kt, V))
    O = torch.full((Q.shape[0], M, V.shape[2]), float("nan"), dtype=Q.dtype, device=DEV)   # poisoned: all is written
    m = torch.full((Q.shape[0], M), float("nan"), device=DEV)
    s = m.clone()
    engine.sparse_attention_qkv_gqa_16(bw, Q.shape[2], V.shape[2], scale, q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(),
                                       m.data_ptr(), s.data_ptr(), Q.shape[0], g, 0, mode=mode)
    torch.cuda.synchronize()
    return O.cpu(), m.cpu().numpy(), s.cpu().numpy()


def _same(got, want):
    """NaN exactly where `want` has NaN, every other element bit for bit; (O, m, s) triples"""
    for a, b in zip(got, want):
        a, b = (torch.from_numpy(x) if isinstance(x, np.ndarray) else x for x in (a, b))
        nan = torch.isnan(b)
        if not torch.equal(torch.isnan(a), nan):
            return False
        raw = torch.int16 if a.element_size() == 2 else torch.int32
        if not torch.equal(a.contiguous().view(raw)[~nan], b.contiguous().view(raw)[~nan]):
            return False
    return True


@pytest.mark.parametrize("g", (2, 3, 4, 7, 8, 16))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("K,Kv", ((32, 32), (128, 128), (96, 160), (256, 256)))
def test_bits_of_the_plain_call_on_repeated_keys_and_values(pat, K, Kv, mode, g):
    engine, bw, ro, ci = pat
    b = 2 * g
    Q, Kt, V = _operands(mode, K, Kv, "random", nb=b)
    Kt, V = Kt[:2].clone(), V[:2].clone()
    scale = K ** -0.5
    got = _call_gqa(engine, bw, mode, Q, Kt, V, scale, g)
    want = _call(engine, bw, mode, Q, Kt.repeat_interleave(g, 0), V.repeat_interleave(g, 0), scale)
    assert not torch.isnan(want[0]).any() and _same(got, want)
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    # Non-finite operands: feature 5 of Kt is +inf on every column of the 15- and the 16-entry row and of the first tile
    # of the 511-entry row, and Q's sign there alternates from head to head: an even head of a group sees +inf (NaN rows),
    # its odd neighbour -inf - dead rows, and a first tile met while m = -inf.  That tile's rows of V hold inf: the 511-entry
    # row of an odd head stays free of NaN only if the head skips the tile while its even neighbour does not.
    first = ci[ro[6]:ro[6] + 16]
    hot = np.unique(np.concatenate([ci[ro[2]:ro[3]], ci[ro[3]:ro[4]], first]))
    Q, Kt = Q.clone(), Kt.clone()
    Q[:, :, 5] = Q[:, :, 5].abs().clamp_min(0.25) * torch.tensor([1.0, -1.0]).repeat(g)[:, None].to(Q.dtype)
    Kt[:, hot, 5] = float("inf")
    V[:, first[::3], 1] = float("inf")
    V[1, first[1::3], 7] = float("-inf")
    got = _call_gqa(engine, bw, mode, Q, Kt, V, scale, g)
    want = _call(engine, bw, mode, Q, Kt.repeat_interleave(g, 0), V.repeat_interleave(g, 0), scale)
    assert torch.isnan(want[0][0::2, 3]).all() and (want[1][1::2, 3] == -np.inf).all()   # NaN and dead heads side by side
    assert np.isfinite(want[1][1::2, 6]).all() and not torch.isnan(want[0][1::2, 6]).any()
    assert _same(got, want)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("K,Kv", ((128, 128), (256, 256)))
def test_every_head_stays_inside_the_bound(pat, K, Kv, mode):
    engine, bw, ro, ci = pat
    g, scale = 4, K ** -0.5
    Q, Kt, V = _operands(mode, K, Kv, "random", nb=8)
    Kt, V = Kt[:2], V[:2]
    O, m, s = _call_gqa(engine, bw, mode, Q, Kt, V, scale, g)
    for h in range(8):
        O64, bO, m64, d, s64, bs = _ref(ro, ci, Q[h], Kt[h // g], V[h // g], scale, mode)
        assert (np.abs(O[h].double().numpy() - O64) <= bO).all(), h
        live = np.isfinite(m64)
        assert (np.abs(m[h][live] - m64[live]) <= d[live]).all() and (m[h][~live] == -np.inf).all()
        assert (np.abs(s[h] - s64) <= bs).all(), h


def test_argument_checks(pat):
    engine, bw, ro, ci = pat
    f = engine.hip().bsmr_sparse_attention_qkv_gqa_16
    buf = torch.zeros(1 << 20, dtype=torch.float16, device=DEV)
    p = buf.data_ptr()
    assert f(bw, 64, 64, 1.0, p, p, p, p, p, p, 8, 0, 0, None) == engine.ERR_INVALID_ARG
    assert f(bw, 64, 64, 1.0, p, p, p, p, p, p, 8, 3, 0, None) == engine.ERR_INVALID_ARG
    for bad in (288, 512):
        assert f(bw, bad, 64, 1.0, p, p, p, p, p, p, 2, 2, 0, None) == engine.ERR_UNSUPPORTED_K
        assert f(bw, 64, bad, 1.0, p, p, p, p, p, p, 2, 2, 0, None) == engine.ERR_UNSUPPORTED_K
    O = torch.full((4, 64), float("nan"), dtype=torch.float16, device=DEV)
    assert f(bw, 64, 64, 1.0, p, p, p, O.data_ptr(), p, p, 0, 2, 0, None) == engine.OK   # no batch: no-op
    torch.cuda.synchronize()
    assert torch.isnan(O).all()
    Q, Kt, V = _operands(1, 512, 64, "random")                            # kv_group = 1: the plain call, K up to 512
    assert _same(_call_gqa(engine, bw, 1, Q, Kt, V, 0.05, 1), _call(engine, bw, 1, Q, Kt, V, 0.05))


def _dense_grads(Q, Kt, V, H, ro, ci, g, scale):
    """fp64 autograd of the dense masked grouped attention from the 16-bit tensors: dQ, dKt, dV"""
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[np.repeat(np.arange(M), np.diff(ro)), ci] = True
    ref = [t.double().requires_grad_(True) for t in (Q, Kt, V)]
    z = (ref[0] @ ref[1].repeat_interleave(g, 0).transpose(-1, -2)) * scale
    top = z.detach().masked_fill(~mask, -np.inf).amax(-1, keepdim=True)
    e = torch.exp((z - torch.where(torch.isfinite(top), top, torch.zeros_like(top))).masked_fill(~mask, -np.inf))
    ((e / e.sum(-1, keepdim=True).clamp_min(1e-300)) @ ref[2].repeat_interleave(g, 0) * H.double()).sum().backward()
    return [t.grad for t in ref]


@pytest.mark.parametrize("mode,one_pass_backward", ((0, False), (1, False), (1, True)))
def test_operator_forward_and_gradients(pat, op, mode, one_pass_backward):
    engine, bw, ro, ci = pat
    g, scale = 4, 128 ** -0.5
    Q, Kt, V = _operands(mode, 128, 128, "random", nb=8)
    Kt, V = Kt[:2].clone(), V[:2].clone()
    H = _r16(mode, np.random.default_rng(7).standard_normal((8, M, 128)))
    leaves = [t.to(DEV).requires_grad_(True) for t in (Q, Kt, V)]
    grouped = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True, one_pass_backward=one_pass_backward), leaves, H.to(DEV))
    assert np.array_equal(_bits(grouped[0]), _bits(_call_gqa(engine, bw, mode, Q, Kt, V, scale, g)[0]))
    rep = [t.to(DEV).requires_grad_(True) for t in (Q, Kt.repeat_interleave(g, 0), V.repeat_interleave(g, 0))]
    plain = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True, one_pass_backward=one_pass_backward), rep, H.to(DEV))
    assert np.array_equal(_bits(grouped[0]), _bits(plain[0]))
    fold = lambda t: t.double().view(2, g, N, -1).sum(1)                  # the yardstick's dKt / dV: its heads summed in fp64
    plain = [plain[1].double(), fold(plain[2]), fold(plain[3])]
    for name, got, yard, want in zip(("dQ", "dKt", "dV"), grouped[1:], plain, _dense_grads(Q, Kt, V, H, ro, ci, g, scale)):
        e1, e0 = float((got.double() - want).abs().max()), float((yard - want).abs().max())
        print(f"mode={mode} one_pass_backward={one_pass_backward} {name}: worst error grouped {e1:.3e}, repeated {e0:.3e}, "
              f"ratio {e1 / e0:.3f}")
        assert e1 <= 2 * e0, (name, e1, e0)


def test_operator_refuses_what_the_grouped_form_does_not_take(op):
    Q, Kt, V = (t.to(DEV) for t in _operands(0, 64, 64, "random", nb=8))
    wide = torch.zeros(2, N, 288, dtype=torch.float16, device=DEV)
    for kw in (dict(blocks=True), dict(Kt=Kt[:2].to(torch.float8_e4m3fn), V=V[:2].to(torch.float8_e4m3fn)), dict(Kt=Kt[:3], V=V[:3]),
               dict(V=V[:4]), dict(V=wide), dict(Q=torch.zeros(8, M, 288, dtype=torch.float16, device=DEV), Kt=wide)):
        with pytest.raises(ValueError):
            op.attention(**{**dict(Q=Q, Kt=Kt[:2], V=V[:2], one_pass=True), **kw})
