"""The host side of the SDDMM backward without a GPU: bsmr_csr_transpose against a stable argsort transpose, and the
argument checks of bsmr_backward_create / bsmr_spmm / bsmr_sddmm_backward, which reject bad input before any device
call (include/bsmr_hip.h "SDDMM backward")."""
import ctypes as C

import numpy as np
import pytest

import synth


def reference_transpose(rows, cols, ro, ci):
    ro = np.asarray(ro, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    row_of = np.repeat(np.arange(rows), np.diff(ro))
    order = np.argsort(ci, kind="stable")
    co = np.zeros(cols + 1, dtype=np.int64)
    np.add.at(co, ci + 1, 1)
    return np.cumsum(co), row_of[order], order


def empty_columns_pattern():
    rows, cols, ro, ci = synth.random_pattern(60, 90, 700, seed=11)
    ci = np.where(ci % 3 == 0, ci, ci - ci % 3)       # only every third column is used
    per_row = [np.unique(ci[ro[r]:ro[r + 1]]) for r in range(rows)]
    ro2 = np.zeros(rows + 1, dtype=np.uint32)
    ro2[1:] = np.cumsum([len(p) for p in per_row])
    return rows, cols, ro2, np.concatenate(per_row).astype(np.uint32)


PATTERNS = {
    "random_empty_rows": lambda: synth.random_pattern(120, 80, 1500, seed=3, empty_rows=17),
    "empty_columns": empty_columns_pattern,
    "nnz0": lambda: (5, 7, np.zeros(6, np.uint32), np.zeros(0, np.uint32)),
    "one_by_one": lambda: (1, 1, np.array([0, 1], np.uint32), np.array([0], np.uint32)),
}


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_csr_transpose_matches_stable_argsort(engine, name):
    rows, cols, ro, ci = PATTERNS[name]()
    co, csc_rows, csc_to_csr = engine.csr_transpose(rows, cols, ro, ci)
    want_co, want_rows, want_map = reference_transpose(rows, cols, ro, ci)
    assert np.array_equal(co, want_co)
    assert np.array_equal(csc_rows, want_rows)
    assert np.array_equal(csc_to_csr, want_map)
    if name == "empty_columns":
        assert (np.diff(co) == 0).sum() >= cols // 2
    # ascending row within each column (= ascending CSR index)
    for c in range(cols):
        seg = csc_to_csr[co[c]:co[c + 1]]
        assert np.all(np.diff(seg.astype(np.int64)) > 0)


def test_csr_transpose_rejects_bad_input(engine):
    hip = engine.hip()
    rows, cols, ro, ci = synth.random_pattern(20, 30, 100, seed=5)
    out = [np.zeros(cols + 1, np.uint32), np.zeros(ci.size, np.uint32), np.zeros(ci.size, np.uint32)]
    p = engine._ptr

    def call(ro_, ci_, nnz=ci.size, n=cols):
        return hip.bsmr_csr_transpose(rows, n, nnz, p(ro_), p(ci_), p(out[0]), p(out[1]), p(out[2]))

    assert call(ro, ci) == engine.OK
    assert hip.bsmr_csr_transpose(rows, cols, ci.size, None, p(ci), p(out[0]), p(out[1]), p(out[2])) == engine.ERR_INVALID_ARG
    assert hip.bsmr_csr_transpose(rows, cols, ci.size, p(ro), p(ci), None, p(out[1]), p(out[2])) == engine.ERR_INVALID_ARG
    assert call(ro, ci, n=int(ci.max())) == engine.ERR_INVALID_ARG           # a column id >= N
    assert call(ro, ci, nnz=ci.size - 1) == engine.ERR_INVALID_ARG          # row_offsets[M] != nnz
    bad = ro.copy()
    bad[5] = bad[6] + 1                                                      # non-monotone
    assert call(bad, ci) == engine.ERR_INVALID_ARG


def _no_gpu_or_ok(engine, st, handle):
    assert st in (engine.OK, engine.ERR_NO_DEVICE), engine.hip().bsmr_strerror(st)
    if st == engine.OK:
        engine.backward_destroy(handle)


def test_backward_create_rejects_bad_input_before_the_device(engine):
    rows, cols, ro, ci = synth.random_pattern(50, 40, 400, seed=9, empty_rows=4)
    create = engine.backward_create_status
    # valid input reaches the device step: OK with a GPU, NO_DEVICE without one
    _no_gpu_or_ok(engine, *create(rows, cols, ro, ci))
    _no_gpu_or_ok(engine, *create(rows, cols, ro, ci, row_order=np.arange(rows)[::-1]))
    _no_gpu_or_ok(engine, *create(rows, cols, ro, ci, row_order=np.array([7, 3, 11])))     # a subset
    # row_order: duplicate, out of range
    assert create(rows, cols, ro, ci, row_order=np.array([1, 2, 1]))[0] == engine.ERR_INVALID_ARG
    assert create(rows, cols, ro, ci, row_order=np.array([0, rows]))[0] == engine.ERR_INVALID_ARG
    # a column id >= N, row_offsets[M] != nnz, non-monotone row_offsets
    assert create(rows, int(ci.max()), ro, ci)[0] == engine.ERR_INVALID_ARG
    short = ro.copy()
    short[-1] -= 1
    assert create(rows, cols, short, ci)[0] == engine.ERR_INVALID_ARG
    bumpy = ro.copy()
    bumpy[10] = bumpy[11] + 1
    assert create(rows, cols, bumpy, ci)[0] == engine.ERR_INVALID_ARG
    # NULL arguments
    hip = engine.hip()
    p = engine._ptr
    h = C.c_void_p()
    assert hip.bsmr_backward_create(None, 0, rows, cols, ci.size, p(ro), p(ci), None, 0) == engine.ERR_INVALID_ARG
    assert hip.bsmr_backward_create(C.byref(h), 0, rows, cols, ci.size, None, p(ci), None, 0) == engine.ERR_INVALID_ARG
    assert hip.bsmr_backward_create(C.byref(h), 0, rows, cols, ci.size, p(ro), None, None, 0) == engine.ERR_INVALID_ARG
    assert hip.bsmr_backward_create(C.byref(h), 0, rows, cols, ci.size, p(ro), p(ci), None, 3) == engine.ERR_INVALID_ARG
    assert not h.value


def test_backward_calls_on_null_handle(engine):
    hip = engine.hip()
    assert hip.bsmr_spmm(None, 32, 0, None, None, None, 1, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_spmm(None, 32, 1, None, None, None, 1, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_sddmm_backward(None, 32, None, None, None, None, None, 1, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_backward_reserve(None, 32, 1) == engine.ERR_INVALID_ARG
    assert hip.bsmr_backward_get_stats(None, None, 0) == engine.ERR_INVALID_ARG
    assert hip.bsmr_backward_destroy(None) == engine.OK


def test_abi_revision_is_5(engine):
    assert engine.hip().bsmr_abi_revision() == 5


# --------------------------------------------------------------------------------------------------------------------
# The backward's fp32 twin (oracle/spmm_oracle.c) on lists built here: exact against scipy on integers, and the bits of
# hand-derived vectors that only the contract's order, fma and chunk sum produce.
# --------------------------------------------------------------------------------------------------------------------
import gather_twin  # noqa: E402

A12 = np.float32(1 + 2.0 ** -12)


def _twin_one(oracle, v, x, K=3):
    """one destination whose list reads (v[t], x[t]) in order; x[t] is broadcast over K columns"""
    n = len(v)
    lists = (np.array([0, n], np.uint32), np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32))
    X = np.repeat(np.asarray(x, np.float32)[:, None], K, axis=1)
    Y = gather_twin.gather(oracle, lists, np.asarray(v, np.float32), X)
    assert (Y.view(np.uint32) == Y[0, 0].view(np.uint32)).all()
    return Y[0, 0]


def _bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.mark.parametrize("name", ["random_empty_rows", "empty_columns", "nnz0", "one_by_one", "long_lists"])
def test_gather_twin_exact_on_integers(oracle, name):
    import scipy.sparse as sp
    if name == "long_lists":        # a row of 1 300 and a column of 1 100 entries: three chunks each
        rows, cols = 1200, 1400
        rng = np.random.default_rng(2)
        per_row = [set(rng.choice(cols, 3, replace=False).tolist()) for _ in range(rows)]
        per_row[5] |= set(range(1300))
        for r in range(1100):
            per_row[r].add(1399)
        per_row = [np.array(sorted(p), np.uint32) for p in per_row]
        ro = np.zeros(rows + 1, np.uint32)
        ro[1:] = np.cumsum([p.size for p in per_row])
        ci = np.concatenate(per_row)
    else:
        rows, cols, ro, ci = PATTERNS[name]()
    rng = np.random.default_rng(7)
    K = 5
    v = rng.integers(-8, 9, ci.size).astype(np.float32)
    Xn = rng.integers(-8, 9, (cols, K)).astype(np.float32)
    Xm = rng.integers(-8, 9, (rows, K)).astype(np.float32)
    S = sp.csr_matrix((v.astype(np.float64), np.asarray(ci, np.int64), np.asarray(ro, np.int64)), shape=(rows, cols))
    Y = gather_twin.gather(oracle, gather_twin.row_lists(ro, ci), v, Xn)
    assert np.array_equal(Y, S @ Xn.astype(np.float64))
    Y = gather_twin.gather(oracle, gather_twin.col_lists(rows, cols, ro, ci), v, Xm)
    assert np.array_equal(Y, S.T @ Xm.astype(np.float64))


def test_gather_twin_list_order(oracle):
    # 2^24 + 1 rounds back to 2^24 (tie to even), then -2^24 leaves 0; the reverse order keeps the 1
    assert _bits(_twin_one(oracle, [1, 1, 1], [2.0 ** 24, 1, -2.0 ** 24])) == 0
    assert _bits(_twin_one(oracle, [1, 1, 1], [-2.0 ** 24, 1, 2.0 ** 24])) == _bits(1.0)


def test_gather_twin_fma_not_mul_add(oracle):
    # -1 + a*a = 2^-11 + 2^-24 exactly in one fma; a*a rounded first (or the reverse order) loses the 2^-24
    want = np.float32(2.0 ** -11 + 2.0 ** -24)
    assert _bits(_twin_one(oracle, [-1, A12], [1, A12])) == _bits(want) == 0x3A000400
    assert _bits(_twin_one(oracle, [A12, -1], [A12, 1])) == _bits(2.0 ** -11)


def test_gather_twin_chunk_order(oracle):
    # 1 025 entries = chunks [0, 512), [512, 1024), [1024, 1025) with partials 2^24, 1, -2^24: (2^24 + 1) - 2^24 = 0,
    # where the reverse chunk order gives 1
    v = np.zeros(1025, np.float32)
    x = np.ones(1025, np.float32)
    v[[0, 512, 1024]] = 1
    x[[0, 512, 1024]] = [2.0 ** 24, 1, -2.0 ** 24]
    assert _bits(_twin_one(oracle, v, x)) == 0
    x[[0, 1024]] = x[[1024, 0]]
    assert _bits(_twin_one(oracle, v, x)) == _bits(1.0)
    # each chunk is its own chain from +0: 2^24, +1, +1 in chunk 0 stays 2^24, chunk 1's 1 + 1 = 2 survives the chunk
    # sum (2^24 + 2 is exact); one chain over all 1 025 entries would give 2^24
    v[:] = 0
    x[:] = 1
    v[[0, 1, 2, 512, 513]] = 1
    x[0] = 2.0 ** 24
    assert _bits(_twin_one(oracle, v, x)) == _bits(2.0 ** 24 + 2)
    assert _bits(_twin_one(oracle, v, x, K=1)) == _bits(2.0 ** 24 + 2)
    assert gather_twin.CHUNK == 512


def test_gather_twin_starts_at_plus_zero(oracle):
    # every product is -0; +0 + -0 = +0, so the chain stays +0
    assert _bits(_twin_one(oracle, [-1, 1, -0.0, -3], [0, -0.0, 5, 0])) == 0
    # an empty list is +0 too
    assert _bits(_twin_one(oracle, [], [])) == 0
    # but fma(2^-100, -2^-100, +0) rounds the exact -2^-200 to -0: the sign of a result that underflows to zero
    assert _bits(_twin_one(oracle, [2.0 ** -100], [-2.0 ** -100])) == 0x80000000
