"""The fused sparse attention without a GPU: the declaration and binding of its five calls, their argument checks (made
before any device call), and the twins of tests/attention_twin.py against hand-derived bits."""
import numpy as np

import synth
from attention_twin import butterfly, check_forward, exact_forward, forward_f64, row_dot, values_backward

NAMES = ("bsmr_sparse_attention_reserve", "bsmr_sparse_attention", "bsmr_sparse_attention_16",
         "bsmr_sparse_attention_backward", "bsmr_sparse_attention_backward_16")
A12 = np.float32(1 + 2.0 ** -12)


def test_symbols_are_declared_and_bound(engine):
    from test_capi import INCLUDE, LIB, declared_functions, exported

    decl = declared_functions(INCLUDE / "bsmr_hip.h")
    for name in NAMES:
        assert name in decl and name in engine.HIP_SYMBOLS and name in exported(LIB / "libbsmr_hip.so")
    assert engine.hip().bsmr_abi_revision() == 5   # five functions added, no layout changed


def test_null_handle_is_refused(engine):
    hip = engine.hip()
    bad = engine.ERR_INVALID_ARG
    assert hip.bsmr_sparse_attention_reserve(None, 32, 1) == bad
    for nb in (1, 0):                                                            # num_batches 0 is no excuse
        assert hip.bsmr_sparse_attention(None, 32, 1.0, 16, 16, 16, 16, 16, nb, None) == bad
        assert hip.bsmr_sparse_attention_16(None, 32, 1.0, 16, 16, 16, 16, 16, nb, engine.COMPUTE_F16, None) == bad
        assert hip.bsmr_sparse_attention_backward(None, 32, 1.0, 16, 16, 16, 16, 16, 16, 16, 16, nb, None) == bad
        assert hip.bsmr_sparse_attention_backward_16(None, 32, 1.0, 16, 16, 16, 16, 16, 16, 16, 16, nb,
                                                     engine.COMPUTE_BF16, None) == bad
    # the handle comes first: a bad Kv, scale or mode beside it does not change the answer
    assert hip.bsmr_sparse_attention(None, 33, float("nan"), None, None, None, None, None, 1, None) == bad
    assert hip.bsmr_sparse_attention_16(None, 0, 1.0, 16, 16, 16, 16, 16, 1, engine.COMPUTE_F32, None) == bad
    with np.testing.assert_raises(engine.BsmrError):
        engine.sparse_attention(None, 32, 1.0, 16, 16, 16, 16, 16)
    with np.testing.assert_raises(engine.BsmrError):
        engine.sparse_attention_backward(None, 32, 1.0, 16, 16, 16, 16, 16, 16, 16, 16, mode=engine.COMPUTE_F16)
    with np.testing.assert_raises(engine.BsmrError):
        engine.sparse_attention_reserve(None, 32)


def test_arguments_on_a_handle(engine):
    """with a handle (only where a device exists: creating one uploads S): scale, Kv, compute_mode, the batch count and
    the pointers, in the header's order; no call here reaches a kernel"""
    rows, cols, ro, ci = synth.random_pattern(20, 30, 100, seed=5)
    st, h = engine.backward_create_status(rows, cols, ro, ci)
    if st == engine.ERR_NO_DEVICE:
        assert engine.backward_create_status(4, 4, np.zeros(5, np.uint32), np.zeros(0, np.uint32))[0] == st
        return
    assert st == engine.OK
    hip = engine.hip()
    bad, bad_k = engine.ERR_INVALID_ARG, engine.ERR_UNSUPPORTED_K
    F16, F32 = engine.COMPUTE_F16, engine.COMPUTE_F32
    fwd = lambda Kv, scale, *p, nb=1: hip.bsmr_sparse_attention(h, Kv, scale, *p, nb, None)
    fwd16 = lambda Kv, scale, mode, *p, nb=1: hip.bsmr_sparse_attention_16(h, Kv, scale, *p, nb, mode, None)
    bwd = lambda Kv, scale, *p, nb=1: hip.bsmr_sparse_attention_backward(h, Kv, scale, *p, nb, None)
    bwd16 = lambda Kv, scale, mode, *p, nb=1: hip.bsmr_sparse_attention_backward_16(h, Kv, scale, *p, nb, mode, None)
    ok5, ok8 = (16,) * 5, (16,) * 8
    try:
        for s in (float("nan"), float("inf"), float("-inf")):
            assert fwd(32, s, *ok5) == bad and fwd16(32, s, F16, *ok5) == bad
            assert bwd(32, s, *ok8) == bad and bwd16(32, s, F16, *ok8) == bad
            assert fwd(33, s, *ok5) == bad                       # scale is checked before Kv
        for Kv in (0, 16, 33, 100):
            assert fwd(Kv, 1.0, *ok5) == bad_k and fwd16(Kv, 1.0, F32, *ok5) == bad_k   # Kv before compute_mode
            assert bwd(Kv, 1.0, *ok8) == bad_k and bwd16(Kv, 1.0, 7, *ok8) == bad_k
            assert hip.bsmr_sparse_attention_reserve(h, Kv, 1) == bad_k
        for mode in (F32, -1, 3):
            assert fwd16(32, 1.0, mode, *ok5) == bad and bwd16(32, 1.0, mode, *ok8) == bad
        assert fwd(32, 1.0, *ok5, nb=65536) == bad and bwd(32, 1.0, *ok8, nb=65536) == bad
        assert hip.bsmr_sparse_attention_reserve(h, 32, 65536) == bad
        for i in range(5):                                       # a NULL array with nnz > 0
            assert fwd(32, 1.0, *[None if j == i else 16 for j in range(5)]) == bad
        for i in range(8):
            assert bwd(32, 1.0, *[None if j == i else 16 for j in range(8)]) == bad
        # P, V, O, m, s: 4, 16, 16, 4, 4 bytes
        for i, off in enumerate((2, 4, 8, 2, 2)):
            assert fwd(32, 1.0, *[16 + off if j == i else 16 for j in range(5)]) == bad
            assert fwd16(32, 1.0, F16, *[16 + off if j == i else 16 for j in range(5)]) == bad
        # P, m, s, dW, O, dO, dP, W: 4, 4, 4, 4, 16, 16, 4, 4 bytes
        for i, off in enumerate((2, 2, 2, 2, 4, 8, 2, 2)):
            assert bwd(32, 1.0, *[16 + off if j == i else 16 for j in range(8)]) == bad
            assert bwd16(32, 1.0, F16, *[16 + off if j == i else 16 for j in range(8)]) == bad
        assert fwd(32, 1.0, *ok5, nb=0) == engine.OK and bwd16(32, 1.0, F16, *ok8, nb=0) == engine.OK   # no-ops
    finally:
        engine.backward_destroy(h)


# ---- the twins -------------------------------------------------------------------------------------------------------
def test_exact_twin_on_three_rows(oracle):
    """row 0: two entries; row 1: (c, -inf, c, c) whose chain 1 + 2^-24 rounds back to 1 before the last 1 arrives, so
    acc = 2 where the exact sum is 2 + 2^-24, and O = fl(2 / 3); row 2: empty"""
    ro = np.array([0, 2, 6, 6], np.uint32)
    ci = np.array([0, 1, 0, 1, 2, 3], np.uint32)
    e = np.array([1, 1, 1, 0, 1, 1], np.float32)
    V = np.array([[1, 5], [3, 6], [2.0 ** -24, 0.25], [1, -1]], np.float32)
    O, s = exact_forward(oracle, ro, ci, e, V)
    assert s.tolist() == [2.0, 3.0, 0.0]
    assert O[0].tolist() == [2.0, 5.5]
    assert O[1, 0] == np.float32(2) / np.float32(3) and O[1].view(np.uint32)[0] == 0x3F2AAAAB
    assert O[1, 1] == np.float32(np.float32(5 + 0.25 - 1) / np.float32(3))
    assert (O[2].view(np.uint32) == 0).all()                     # exact +0
    # the fp64 reference sees 2 + 2^-24 there, inside the bound
    p = np.where(e > 0, np.float32(1.5), -np.inf).astype(np.float32)
    O64, bound, m, s64 = forward_f64(ro, ci, p, 2.0, V)
    assert m.tolist() == [3.0, 3.0, -np.inf] and s64.tolist() == [2.0, 3.0, 0.0]
    assert abs(O64[1, 0] - (2 + 2.0 ** -24) / 3) < 1e-15
    check_forward(ro, ci, p, 2.0, V, O, "three rows")


def test_fp64_reference_special_values():
    inf, nan = np.inf, np.nan
    rows = [[-inf, -inf], [1.0, -inf, 1.0], [nan, -inf], [inf, 0.0], [3.0], []]
    ro = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    ci = np.concatenate([np.arange(len(r)) for r in rows]).astype(np.uint32)
    p = np.array([v for r in rows for v in r], np.float32)
    V = np.array([[1, 2], [3, 4], [5, 8]], np.float32)
    O, _, m, s = forward_f64(ro, ci, p, 1.0, V)
    assert O[0].tolist() == [0, 0] and O[1].tolist() == [3.0, 5.0]
    assert np.isnan(O[2]).all() and np.isnan(O[3]).all() and np.isnan(m[2])
    assert O[4].tolist() == [1.0, 2.0] and O[5].tolist() == [0, 0]
    assert m[0] == -inf and m[5] == -inf and s[0] == 0 and s[4] == 1


def test_row_dot_order(oracle):
    """K = 64: lane 0 owns k = 0 and k = 32, in that order: fmaf(A12, A12, 0) rounds to 1 + 2^-11 (a tie, to even) and the
    second term cancels it to 0; the other order gives 2^-24.  The butterfly: 2^24 in lane 0 meets the 1 of lane 16 first
    (a tie back to 2^24) and the 1 of lane 17 last (again), where any sum that adds the two ones first gives 2^24 + 2."""
    O = np.zeros((2, 64), np.float32)
    dO = np.ones((2, 64), np.float32)
    O[0, 0], dO[0, 0] = A12, A12
    O[0, 32] = -(1 + 2.0 ** -11)
    O[1, 0], O[1, 16], O[1, 17] = 2.0 ** 24, 1, 1
    D = row_dot(oracle, dO, O)
    assert D[0] == 0.0 and D[1] == np.float32(2.0 ** 24)
    assert row_dot(oracle, dO[:, ::-1], O[:, ::-1])[0] == np.float32(2.0 ** -24)      # the chain's order matters
    parts = np.zeros(32, np.float32)
    parts[[0, 16, 17]] = 2.0 ** 24, 1, 1
    assert butterfly(parts) == np.float32(2.0 ** 24)
    parts[[16, 17]] = 0
    parts[[1, 3]] = 1                                            # lanes 1 and 3 meet at offset 2, before lane 0
    assert butterfly(parts) == np.float32(2.0 ** 24 + 2)


def test_row_dot_against_fp64(oracle):
    rng = np.random.default_rng(2)
    for K in (32, 96, 512):
        O = rng.standard_normal((37, K)).astype(np.float32)
        dO = rng.standard_normal((37, K)).astype(np.float32)
        D = row_dot(oracle, dO, O)
        want = (O.astype(np.float64) * dO).sum(axis=1)
        mag = np.abs(O.astype(np.float64) * dO).sum(axis=1)
        assert (np.abs(D - want) <= (K // 32 + 5) * 2.0 ** -24 * mag).all()


def test_values_backward_rounds_each_step():
    a = np.float32(3.0e7)
    ro = np.array([0, 3, 3, 4], np.uint32)
    W = np.array([0.5, 0.5, 0.25, 1.0], np.float32)
    dW = np.array([a, -a, 3.0, 7.0], np.float32)
    D = np.array([0.75, 123.0, 7.0], np.float32)
    f = np.float32
    dP = values_backward(ro, W, dW, D, 2.0)
    assert dP.tolist() == [f(f(f(0.5) * f(a - f(0.75))) * f(2)), f(f(f(0.5) * f(-a - f(0.75))) * f(2)), f(1.125), 0.0]
