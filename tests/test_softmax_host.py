"""The sparse row softmax without a GPU: the declaration and binding of both calls, their argument checks (made before any
device call), and the backward's fp32 twin (tests/softmax_twin.py) against fp64 and against hand-derived bits."""
import numpy as np

import synth
from gather_twin import CHUNK
from softmax_twin import backward_twin, forward_f64, row_sums

A12 = np.float32(1 + 2.0 ** -12)


def test_symbols_are_declared_and_bound(engine):
    from test_capi import INCLUDE, LIB, declared_functions, exported

    decl = declared_functions(INCLUDE / "bsmr_hip.h")
    for name in ("bsmr_sparse_softmax", "bsmr_sparse_softmax_backward"):
        assert name in decl and name in engine.HIP_SYMBOLS and name in exported(LIB / "libbsmr_hip.so")
    assert engine.hip().bsmr_abi_revision() == 5   # two functions added, no layout changed


def test_null_handle_and_arguments_are_refused(engine):
    hip = engine.hip()
    bad = engine.ERR_INVALID_ARG
    assert hip.bsmr_sparse_softmax(None, 1.0, None, None, 1, None) == bad
    assert hip.bsmr_sparse_softmax(None, 1.0, 16, 16, 1, None) == bad
    assert hip.bsmr_sparse_softmax(None, 1.0, 16, 16, 0, None) == bad            # num_batches 0 is no excuse
    assert hip.bsmr_sparse_softmax_backward(None, 1.0, None, None, None, 1, None) == bad
    assert hip.bsmr_sparse_softmax_backward(None, 0.5, 16, 16, 16, 1, None) == bad
    with np.testing.assert_raises(engine.BsmrError):
        engine.sparse_softmax(None, 1.0, 16, 16)
    with np.testing.assert_raises(engine.BsmrError):
        engine.sparse_softmax_backward(None, 1.0, 16, 16, 16)


def test_arguments_on_a_handle(engine):
    """with a handle (only where a device exists: creating one uploads S): a non-finite scale and NULL arrays with nnz > 0
    are refused, NULL arrays with nnz = 0 and num_batches = 0 are no-ops"""
    rows, cols, ro, ci = synth.random_pattern(20, 30, 100, seed=5)
    st, h = engine.backward_create_status(rows, cols, ro, ci)
    if st == engine.ERR_NO_DEVICE:
        assert engine.backward_create_status(4, 4, np.zeros(5, np.uint32), np.zeros(0, np.uint32))[0] == st
        return
    assert st == engine.OK
    hip = engine.hip()
    bad = engine.ERR_INVALID_ARG
    try:
        for s in (float("nan"), float("inf"), float("-inf")):
            assert hip.bsmr_sparse_softmax(h, s, 16, 16, 1, None) == bad
            assert hip.bsmr_sparse_softmax_backward(h, s, 16, 16, 16, 1, None) == bad
        assert hip.bsmr_sparse_softmax(h, 1.0, None, 16, 1, None) == bad
        assert hip.bsmr_sparse_softmax(h, 1.0, 16, None, 1, None) == bad
        assert hip.bsmr_sparse_softmax_backward(h, 1.0, None, 16, 16, 1, None) == bad
        assert hip.bsmr_sparse_softmax_backward(h, 1.0, 16, None, 16, 1, None) == bad
        assert hip.bsmr_sparse_softmax_backward(h, 1.0, 16, 16, None, 1, None) == bad
        assert hip.bsmr_sparse_softmax(h, 1.0, 16, 16, 65536, None) == bad
    finally:
        engine.backward_destroy(h)
    h = engine.backward_create(4, 4, np.zeros(5, np.uint32), np.zeros(0, np.uint32))
    try:
        assert hip.bsmr_sparse_softmax(h, 1.0, None, None, 3, None) == engine.OK
        assert hip.bsmr_sparse_softmax_backward(h, 1.0, None, None, None, 3, None) == engine.OK
        assert hip.bsmr_sparse_softmax(h, float("nan"), None, None, 1, None) == bad
    finally:
        engine.backward_destroy(h)


# ---- the twin ----------------------------------------------------------------------------------------------------------
def _one_row(values):
    return np.array([0, len(values)], np.uint32)


def test_twin_against_fp64(oracle):
    rows, cols, ro, ci = synth.random_pattern(200, 3000, 40000, seed=7, empty_rows=20)
    rng = np.random.default_rng(1)
    y = rng.random(ci.size).astype(np.float32)
    dY = rng.standard_normal(ci.size).astype(np.float32)
    g = row_sums(oracle, ro, y, dY)
    r = np.repeat(np.arange(rows), np.diff(ro.astype(np.int64)))
    g64 = np.bincount(r, weights=y.astype(np.float64) * dY, minlength=rows)
    mag = np.bincount(r, weights=np.abs(y.astype(np.float64) * dY), minlength=rows)
    n = np.diff(ro.astype(np.int64))
    assert (np.abs(g - g64) <= (n + 2) * 2.0 ** -24 * mag).all()
    assert (g[n == 0] == 0).all()
    dX = backward_twin(oracle, ro, y, dY, 0.25)
    want = y.astype(np.float64) * (dY - g64[r]) * 0.25
    assert np.allclose(dX, want, rtol=1e-4, atol=1e-5 * np.abs(want).max())


def test_twin_chunk_boundaries(oracle):
    """y = 1, dY = [2^24, 1, 1, ...]: a single chain absorbs every 1; chunks of 512 restart at 0, so the second chunk's
    ones survive when there are at least two of them (a lone 1 ties back to 2^24, to even)"""
    # 1100 = 512 + 512 + 76: the partials 2^24, 512 and 76 add exactly
    for L, want in ((511, 2.0 ** 24), (512, 2.0 ** 24), (513, 2.0 ** 24), (514, 2.0 ** 24 + 2), (1100, 2.0 ** 24 + 588)):
        dY = np.ones(L, np.float32)
        dY[0] = 2.0 ** 24
        g = row_sums(oracle, _one_row(dY), np.ones(L, np.float32), dY)
        assert g[0] == np.float32(want), (L, g[0])
    assert CHUNK == 512


def test_twin_cancellation_in_g(oracle):
    """g = 0.5 a + 0.5 (-a) = 0 exactly, so dX_t = y_t dY_t scale with no trace of a"""
    a = np.float32(3.0e7)
    y = np.array([0.5, 0.5, 0.25], np.float32)
    dY = np.array([a, -a, 3.0], np.float32)
    ro = _one_row(y)
    g = row_sums(oracle, ro, y, dY)
    assert g[0] == np.float32(0.75)
    dX = backward_twin(oracle, ro, y, dY, 2.0)
    f = np.float32
    assert dX.tolist() == [f(f(f(0.5) * f(a - f(0.75))) * f(2)), f(f(f(0.5) * f(-a - f(0.75))) * f(2)), f(1.125)]


def test_twin_uses_fma(oracle):
    """acc = -(1 + 2^-11), then fmaf(A12, A12, acc) = 2^-24 exactly; a multiply then add rounds A12^2 to 1 + 2^-11
    (a tie, to even) and gives 0"""
    y = np.array([1.0, A12], np.float32)
    dY = np.array([-(1 + 2.0 ** -11), A12], np.float32)
    g = row_sums(oracle, _one_row(y), y, dY)
    assert g[0] == np.float32(2.0 ** -24)
    assert np.float32(np.float32(A12 * A12) + dY[0]) == 0.0   # what the contract's order avoids
    dX = backward_twin(oracle, _one_row(y), y, dY, 1.0)
    assert dX[1] == np.float32(A12 * np.float32(A12 - np.float32(2.0 ** -24)))


def test_fp64_reference_special_values():
    inf, nan = np.inf, np.nan
    rows = [[-inf, -inf], [1.0, -inf, 1.0], [nan, -inf], [inf, 0.0], [3.0], [], [2.0, 2.0, 2.0, 2.0]]
    ro = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    x = np.array([v for r in rows for v in r], np.float32)
    y = forward_f64(ro, x, 1.0)[0]
    assert y[:2].tolist() == [0.0, 0.0]
    assert y[2:5].tolist() == [0.5, 0.0, 0.5]
    assert np.isnan(y[5:9]).all()
    assert y[9] == 1.0 and y[10:].tolist() == [0.25] * 4
