"""One-pass backward of sparse attention with grouped key/value heads (include/bsmr_hip.h "One-pass backward of sparse
attention with grouped key/value heads") on the device, on the two-sided ladder of
test_gpu_attention_qkv_bwd.py (empty row and column, lists of 15, 16 and 17 entries, two split rows and two split columns):
  1. dQ has the bits of bsmr_sparse_attention_qkv_backward_16 on repeat_interleaved Kt and V, every output row is written;
     dKt and dV against fp64 autograd of the dense masked grouped attention, the ungrouped call with its heads summed in
     fp64 as the yardstick: the worst error at most 2x the yardstick's;
  2. a NaN stays in its own row and its KV head's columns, a dead row of a neighbouring head adds nothing;
  3. NULL gradients;  4. argument checks;  5. the operator: bits and the memory of the backward.
Measured on an MI355X: the ratios of test 1 are listed in DESIGN.md 23."""
import numpy as np
import pytest

from test_gpu_attention_qkv import DEV, _bits, _grads
from test_gpu_attention_qkv_bwd import M, N, _backward, _forward, _operands, pat  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _grouped(engine, bw, mode, Q, Kt, V, H, scale, g, want=(True, True, True), fix=None):
    """[dQ, dKt, dV] of the grouped call as CPU tensors (None where not wanted) of CPU 16-bit tensors Q, H [b, ...] and
    Kt, V [b / g, ...]; the outputs start as NaN.  fix(m, s): edits the forward's m and s in place"""
    q, k, v, h = (t.to(DEV) for t in (Q, Kt, V, H))
    O, m, s = _forward(engine, bw, mode, q, k.repeat_interleave(g, 0), v.repeat_interleave(g, 0), scale)
    if fix:
        fix(m, s)
    out = [torch.full_like(t, float("nan")) if w else None for t, w in zip((q, k, v), want)]
    engine.sparse_attention_qkv_gqa_backward_16(bw, Q.shape[2], V.shape[2], scale, q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                                O.data_ptr(), h.data_ptr(), m.data_ptr(), s.data_ptr(),
                                                *(0 if t is None else t.data_ptr() for t in out), Q.shape[0], g, 0, mode=mode)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu() for t in out]


def _dense_grads(Q, Kt, V, H, mask, g, scale):
    """fp64 autograd of the dense masked grouped attention from the 16-bit tensors, on the device: dKt, dV"""
    mask = mask.to(DEV)
    q, k, v = (t.to(DEV).double().requires_grad_(True) for t in (Q, Kt, V))
    z = (q @ k.repeat_interleave(g, 0).transpose(-1, -2)) * scale
    top = z.detach().masked_fill(~mask, -np.inf).amax(-1, keepdim=True)
    e = torch.exp((z - torch.where(torch.isfinite(top), top, torch.zeros_like(top))).masked_fill(~mask, -np.inf))
    ((e / e.sum(-1, keepdim=True).clamp_min(1e-300)) @ v.repeat_interleave(g, 0) * H.to(DEV).double()).sum().backward()
    return k.grad.cpu(), v.grad.cpu()


@pytest.mark.parametrize("g", (2, 3, 4, 8))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("K,Kv", ((32, 32), (96, 160), (128, 128), (256, 256)))
def test_dq_bits_and_the_error_of_dkt_and_dv(pat, K, Kv, mode, g):
    engine, bw, _, mask, _ = pat
    st = engine.backward_stats(bw)
    assert st["split_rows"] == 2 and st["split_cols"] == 2
    Q, Kt, V, H = _operands(mode, K, Kv, 2 * g)
    Kt, V, scale = Kt[:2].clone(), V[:2].clone(), K ** -0.5
    dQ, dKt, dV = _grouped(engine, bw, mode, Q, Kt, V, H, scale, g)
    rQ, rKt, rV = _backward(engine, bw, mode, Q, Kt.repeat_interleave(g, 0), V.repeat_interleave(g, 0), H, scale)
    assert not torch.isnan(rQ).any() and np.array_equal(_bits(dQ), _bits(rQ))
    rows, cols = mask.any(1), mask.any(0)
    for t, live in ((dQ, rows), (dKt, cols), (dV, cols)):
        assert not torch.isnan(t).any() and (_bits(t[:, ~live]) == 0).all()           # every row written, +0 without entries
    fold = lambda t: t.double().view(2, g, N, -1).sum(1)                              # the yardstick: its heads summed in fp64
    for name, got, yard, want in zip(("dKt", "dV"), (dKt, dV), (fold(rKt), fold(rV)), _dense_grads(Q, Kt, V, H, mask, g, scale)):
        e1, e0 = float((got.double() - want).abs().max()), float((yard - want).abs().max())
        print(f"K={K} Kv={Kv} mode={mode} g={g} {name}: worst error grouped {e1:.3e}, repeated {e0:.3e}, ratio {e1 / e0:.3f}")
        assert e1 <= 2 * e0, (name, e1, e0)


@pytest.mark.parametrize("mode", (0, 1))
def test_a_nan_stays_in_its_row_and_a_dead_row_adds_nothing(pat, mode):
    engine, bw, _, mask, (ro, ci) = pat
    K, Kv, g = 128, 128, 4
    Q, Kt, V, H = _operands(mode, K, Kv, 2 * g)
    Kt, V = Kt[:2].clone(), V[:2].clone()
    r = int(np.flatnonzero(mask[:, 8].numpy())[1])      # the second entry of the two-chunk column: heads 2 and 3 of KV head 0 meet
                                                        # in one wave of the row side and in one tile slot of the column side

    def dead(m, s):                                     # head 3's row r as the forward leaves a row whose scores are all -inf
        m[3, r], s[3, r] = float("-inf"), 0.0

    clean = _grouped(engine, bw, mode, Q, Kt, V, H, 0.1, g, fix=dead)
    Qn = Q.clone()
    Qn[2, r, 77], Qn[3, r, 5] = float("nan"), float("inf")
    hit = (torch.arange(M) == r, mask[r], mask[r])
    for i, (got, was, h) in enumerate(zip(_grouped(engine, bw, mode, Qn, Kt, V, H, 0.1, g, fix=dead), clean, hit)):
        head = 2 if i == 0 else 0                       # dQ: query head 2; dKt, dV: its KV head
        assert h.any() and torch.isnan(got[head][h]).all()
        keep = torch.ones(got.shape[:2], dtype=torch.bool)
        keep[head, h] = False
        assert np.array_equal(_bits(got[keep]), _bits(was[keep]))
    assert (_bits(clean[0][3, r]) == 0).all()


@pytest.mark.parametrize("mode", (0, 1))
def test_null_gradients(pat, mode):
    engine, bw, _, _, _ = pat
    Q, Kt, V, H = _operands(mode, 96, 160, 6)
    Kt, V = Kt[:2].clone(), V[:2].clone()
    both = _grouped(engine, bw, mode, Q, Kt, V, H, 0.1, 3)
    for i in range(3):
        one = _grouped(engine, bw, mode, Q, Kt, V, H, 0.1, 3, want=tuple(j == i for j in range(3)))
        assert np.array_equal(_bits(one[i]), _bits(both[i]))


def test_argument_checks(pat):
    engine, bw, _, _, _ = pat
    f = engine.hip().bsmr_sparse_attention_qkv_gqa_backward_16
    buf = torch.zeros(1 << 20, dtype=torch.float16, device=DEV)
    p = buf.data_ptr()
    assert f(bw, 64, 64, 1.0, *[p] * 10, 8, 0, 0, None) == engine.ERR_INVALID_ARG
    assert f(bw, 64, 64, 1.0, *[p] * 10, 8, 3, 0, None) == engine.ERR_INVALID_ARG
    assert f(bw, 288, 64, 1.0, *[p] * 10, 2, 2, 0, None) == engine.ERR_UNSUPPORTED_K
    assert f(bw, 64, 288, 1.0, *[p] * 10, 2, 2, 0, None) == engine.ERR_UNSUPPORTED_K
    out = torch.full((3, 4, 64), float("nan"), dtype=torch.float16, device=DEV)
    assert f(bw, 64, 64, 1.0, *[p] * 7, *(t.data_ptr() for t in out), 0, 2, 0, None) == engine.OK   # no batch: no-op
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    Q, Kt, V, H = _operands(1, 64, 64, 2)                                             # kv_group = 1: the existing backward
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(_grouped(engine, bw, 1, Q, Kt, V, H, 0.1, 1),
                                                                  _backward(engine, bw, 1, Q, Kt, V, H, 0.1)))


@pytest.mark.parametrize("mode", (0, 1))
def test_the_operator(pat, mode):
    engine, bw, op, _, _ = pat
    K, Kv, g = 128, 128, 4
    Q, Kt, V, H = _operands(mode, K, Kv, 2 * g)
    Kt, V, scale = Kt[:2].clone(), V[:2].clone(), K ** -0.5
    leaves = [t.to(DEV).requires_grad_(True) for t in (Q, Kt, V)]
    got = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True, one_pass_backward=True), leaves, H.to(DEV))
    old = _grads(lambda q, k, v: op.attention(q, k, v, one_pass=True), leaves, H.to(DEV))
    assert np.array_equal(_bits(got[0]), _bits(old[0]))                               # the forward keeps its bits
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[1:], _grouped(engine, bw, mode, Q, Kt, V, H, scale, g)))
    # the memory of the backward: below the operands of the path it replaces - Kt and V repeated, dKt and dV on b heads
    h = H.to(DEV)
    O = op.attention(*leaves, one_pass=True, one_pass_backward=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    O.backward(h)
    torch.cuda.synchronize()
    repeated = 2 * g * (Kt.numel() + V.numel()) * Kt.element_size()                   # Kr, Vr, dKr, dVr
    assert torch.cuda.max_memory_allocated() - before < repeated
