"""Host side of the blocked SpMM with split panels (include/bsmr_hip.h "Blocked SpMM", segment_blocks), no device needed:
  * tests/blocked_split_twin.py against bits derived by hand, against BlockedTwin where nothing is split, against the
    gather twin on exact integers, and the share of elements in which splitting changes the bits - what makes the bit
    tests of tests/test_gpu_spmm_blocked_split.py tests of the split;
  * the four statistics bsmr_blocked_check_split adds, against numpy counts;
  * the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import blocked_split_twin as st
import blocked_twin as bt
from gather_twin import gather, row_lists

NULL = bt.NULL
SPLITS = (0, 1, 2, 4, 5, 2 ** 32 - 1)


@pytest.fixture(scope="module")
def case(engine):
    M, N, ro, ci = bt.blocked_pattern()
    csr = engine.CSR.from_arrays(M, N, ro, ci)
    arrays = engine.Pipeline(csr, alpha=0.3, delta=0.3, device=-1).arrays()
    return M, N, ro, ci, arrays


@pytest.fixture(scope="module")
def twin(case, oracle):
    M, N, ro, ci, arrays = case
    return st.SplitTwin(oracle, M, N, ro, ci, arrays)


def _normal(seed, nnz, N, K):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(nnz).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)


def test_twin_against_hand_derived_bits(engine, oracle):
    """One ragged panel of one row with two blocks, no residue, K = 1, x = 1.  e = 2^-24 = half an ulp of 1.
      block 0  cell j = 0 with v = 1:     contributes 1
      block 1  cells j = 0, 1 with v = e:  contribute e + e
    Unsplit, one chain: fmaf(e, 1, 1) is a tie between 1 and 1 + 2e and rounds to even, 1 - twice.  Y = 1.
    S = 1, two segments: p0 = 1; p1 = e, then 2e = 2^-23, exact; p0 + p1 = 1 + 2^-23, exact."""
    M, N = 1, 40
    ro = np.array([0, 3], dtype=np.uint32)
    ci = np.array([0, 16, 17], dtype=np.uint32)
    bv = np.full((2, 16, 16), NULL, dtype=np.uint32)
    bv[0, 0, 0], bv[1, 0, 0], bv[1, 0, 1] = 0, 1, 2
    empty = np.zeros(0, dtype=np.uint32)
    arrays = {"reorderedRows": np.zeros(1, dtype=np.uint32), "denseCols": np.arange(32, dtype=np.uint32),
              "blockOffsets": np.array([0, 2], dtype=np.uint32), "blockValues": bv.reshape(-1),
              "sparseValueOffsets": np.zeros(2, dtype=np.uint32), "sparseValues": empty, "sparseRelativeRows": empty,
              "sparseColIndices": empty}
    for S, want in ((0, (0, 0, 1, 2)), (1, (1, 1, 2, 1)), (2, (2, 0, 1, 2))):
        status, s = engine.blocked_check_status(M, N, ro, ci, arrays, segment_blocks=S)
        assert status == engine.OK
        assert (s["segment_blocks"], s["split_panels"], s["segments"], s["max_blocks_per_segment"]) == want
        assert (s["panels"], s["blocks"], s["block_entries"], s["residue_entries"]) == (1, 2, 3, 0)
    e = np.float32(2.0 ** -24)
    v = np.array([1, e, e], dtype=np.float32)
    X = np.ones((N, 1), dtype=np.float32)
    tw = st.SplitTwin(oracle, M, N, ro, ci, arrays)
    bits = lambda a: a[:, 0].view(np.uint32).tolist()
    one, next_up = np.array([1.0], dtype=np.float32), np.array([1 + 2.0 ** -23], dtype=np.float32)
    assert bits(tw.twin(v, X, 0)) == one.view(np.uint32).tolist()
    assert bits(tw.twin(v, X, 1)) == next_up.view(np.uint32).tolist()
    assert bits(tw.twin(v, X, 2)) == one.view(np.uint32).tolist()          # nb <= S: one segment, the unsplit bits
    assert bits(bt.BlockedTwin.twin(tw, v, X)) == one.view(np.uint32).tolist()


def test_pattern_has_split_and_unsplit_panels(case, twin):
    """panels of 0, 2, 5, 5, 5, 5, 5, 3 blocks: S = 1 splits all seven, S = 2 six, S = 4 five, S >= 5 none"""
    arrays = case[4]
    assert np.diff(arrays["blockOffsets"].astype(np.int64)).tolist() == [0, 2, 5, 5, 5, 5, 5, 3]
    assert [st.split_stats(arrays, S)["split_panels"] for S in SPLITS] == [0, 7, 6, 5, 0, 0]
    assert [int(twin.split_rows(S).sum()) for S in (1, 2, 3, 4, 5, 8)] == [107, 91, 80, 80, 0, 0]


@pytest.mark.parametrize("S", (0, 5, 8, 2 ** 32 - 1))
def test_twin_without_a_split_panel_equals_the_blocked_twin(twin, S):
    v, X = _normal(3, twin.nnz, twin.N, 64)
    assert twin.twin(v, X, S).tobytes() == bt.BlockedTwin.twin(twin, v, X).tobytes()


@pytest.mark.parametrize("S", SPLITS)
def test_twin_on_exact_integers_equals_the_gather_twin(case, twin, oracle, S):
    M, N, ro, ci, _ = case
    rng = np.random.default_rng(7)
    v = rng.integers(-7, 8, ci.size).astype(np.float32)
    X = rng.integers(-15, 16, (N, 32)).astype(np.float32)
    assert twin.twin(v, X, S).tobytes() == gather(oracle, row_lists(ro, ci), v, X).tobytes()


@pytest.mark.parametrize("S", (1, 2, 4))
def test_splitting_changes_the_bits_of_split_panels_only(twin, S):
    """on normal data a device that ignores S fails the bit tests: more than a fifth of the elements in rows of split
    panels differ from the unsplit twin; rows of unsplit panels never do"""
    v, X = _normal(1, twin.nnz, twin.N, 64)
    a, b = twin.twin(v, X, S).view(np.uint32), twin.twin(v, X, 0).view(np.uint32)
    rows = twin.split_rows(S)
    share = float((a[rows] != b[rows]).mean())
    print(f"S = {S}: {int(rows.sum())} rows in split panels, {share:.2f} of their elements differ from the unsplit twin")
    assert share > 0.2
    assert a[~rows].tobytes() == b[~rows].tobytes()


@pytest.mark.parametrize("S", (1, 2, 4))
def test_twin_within_the_fp64_bound(twin, S):
    v, X = _normal(11, twin.nnz, twin.N, 64)
    Y64, bound = twin.fp64(v, X, S)
    assert (np.abs(twin.twin(v, X, S).astype(np.float64) - Y64) <= bound).all()
    assert (bound <= twin.fp64(v, X, 0)[1]).all()          # shorter chains: never a wider bound than the unsplit form


@pytest.mark.parametrize("S", SPLITS)
def test_statistics_equal_numpy_counts(engine, case, S):
    M, N, ro, ci, arrays = case
    status, s = engine.blocked_check_status(M, N, ro, ci, arrays, segment_blocks=S)
    assert status == engine.OK
    want = dict(bt.numpy_stats(M, N, ro, ci, arrays), **st.split_stats(arrays, S))
    assert {k: s[k] for k in want} == want
    assert s["device_index_bytes"] == 0


def test_check_is_the_split_check_at_zero(engine, case):
    M, N, ro, ci, arrays = case
    hip = engine.hip()
    d, keep = engine.rphm_desc(M, N, int(ci.size), arrays)
    a, b = engine.BlockedStats(), engine.BlockedStats()
    assert hip.bsmr_blocked_check(M, N, ci.size, ro.ctypes.data, ci.ctypes.data, C.byref(d), C.byref(a), C.sizeof(a)) == engine.OK
    assert hip.bsmr_blocked_check_split(M, N, ci.size, ro.ctypes.data, ci.ctypes.data, C.byref(d), 0, C.byref(b),
                                        C.sizeof(b)) == engine.OK
    assert bytes(a) == bytes(b)
    assert (a.segment_blocks, a.split_panels, a.segments, a.max_blocks_per_segment) == \
        (0, 0, a.panels_with_blocks, a.max_blocks_per_panel)
    # a plan without blocks has no segments, whatever S
    arrays1 = engine.Pipeline(engine.CSR.from_arrays(M, N, ro, ci), alpha=0.3, delta=1.0, device=-1).arrays()
    for S in (0, 3):
        status, s = engine.blocked_check_status(M, N, ro, ci, arrays1, segment_blocks=S)
        assert status == engine.OK
        assert (s["segment_blocks"], s["split_panels"], s["segments"], s["max_blocks_per_segment"]) == (S, 0, 0, 0)


def test_invalid_arguments(engine, case):
    M, N, ro, ci, arrays = case
    hip = engine.hip()
    s = engine.BlockedStats()
    nnz = int(ci.size)
    d, keep = engine.rphm_desc(M, N, nnz, arrays)
    rop, cip = ro.ctypes.data, ci.ctypes.data
    size = C.sizeof(s)
    check = hip.bsmr_blocked_check_split
    for S in (1, 2 ** 32 - 1):
        assert check(M, N, nnz, rop, cip, C.byref(d), S, C.byref(s), size) == engine.OK
        assert check(M, N, nnz, rop, cip, None, S, C.byref(s), size) == engine.ERR_INVALID_ARG
        assert check(M, N, nnz, rop, cip, C.byref(d), S, None, size) == engine.ERR_INVALID_ARG
        assert check(M, N, nnz, None, cip, C.byref(d), S, C.byref(s), size) == engine.ERR_INVALID_ARG
        assert check(M - 1, N, nnz, rop, cip, C.byref(d), S, C.byref(s), size) == engine.ERR_INVALID_ARG
    bad = bt.copy_arrays(arrays)
    bad["sparseColIndices"][0] = (bad["sparseColIndices"][0] + 1) % N
    assert engine.blocked_check_status(M, N, ro, ci, bad, segment_blocks=2)[0] == engine.ERR_BAD_PLAN
    # out_size bounds what is written: a caller built against the shorter struct keeps its bytes
    old = C.sizeof(s) - 16
    raw = (C.c_uint8 * size)(*([0xAB] * size))
    assert check(M, N, nnz, rop, cip, C.byref(d), 2, C.cast(raw, C.POINTER(engine.BlockedStats)), old) == engine.OK
    assert bytes(raw[old:]) == b"\xab" * 16 and bytes(raw[:old]) != b"\xab" * old
    # the handle is checked first
    assert hip.bsmr_backward_attach_blocks_split(None, C.byref(d), 2) == engine.ERR_INVALID_ARG
    assert hip.bsmr_backward_attach_blocks_split(None, None, 0) == engine.ERR_INVALID_ARG
    assert hip.bsmr_abi_revision() == 5
