"""Host side of the blocked SpMM (include/bsmr_hip.h "Blocked SpMM"), no device needed:
  * bsmr_blocked_check accepts what the host pipeline builds, refuses every way in which an RPHM can fail to be a
    partition of the CSR (one corruption at a time: BSMR_ERR_BAD_PLAN) and every inconsistent argument
    (BSMR_ERR_INVALID_ARG), and its statistics equal counts taken in numpy;
  * the test pattern (tests/blocked_twin.py) has the properties the GPU tests rely on - asserted from those statistics,
    so that a change to the pipeline cannot empty the tests unnoticed;
  * the argument checks of attach and of the two device calls that need no handle;
  * the twin itself against bits derived by hand."""
import ctypes as C

import numpy as np
import pytest

import blocked_twin as bt
import synth

NULL = bt.NULL


@pytest.fixture(scope="module")
def case(engine):
    M, N, ro, ci = bt.blocked_pattern()
    csr = engine.CSR.from_arrays(M, N, ro, ci)
    arrays = engine.Pipeline(csr, alpha=0.3, delta=0.3, device=-1).arrays()
    return M, N, ro, ci, arrays


def _check(engine, case, arrays=None):
    M, N, ro, ci, own = case
    return engine.blocked_check_status(M, N, ro, ci, own if arrays is None else arrays)


def test_pattern_has_the_properties_the_gpu_tests_rely_on(engine, case):
    M, N, ro, ci, arrays = case
    st, s = _check(engine, case)
    assert st == engine.OK
    per_panel = np.diff(arrays["blockOffsets"].astype(np.int64))
    assert s["panels"] == per_panel.size and s["panels_with_blocks"] < s["panels"]     # a panel without blocks
    assert s["max_blocks_per_panel"] >= 4
    assert s["padding_columns"] > 0
    assert s["split_residue_rows"] >= 1 and s["max_residue_row"] > 2 * 512            # a residue row of three chunks
    rows_in = arrays["reorderedRows"].size
    assert rows_in < M                                                                  # empty rows
    assert rows_in % 16 != 0 and per_panel[-1] > 0                                      # a ragged last panel with blocks
    assert 0 < s["block_entries"] < 256 * s["blocks"]                                   # empty cells
    assert s["block_entries"] + s["residue_entries"] == ci.size


def test_statistics_equal_numpy_counts(engine, case):
    M, N, ro, ci, arrays = case
    st, s = _check(engine, case)
    assert st == engine.OK
    want = bt.numpy_stats(M, N, ro, ci, arrays)
    assert {k: s[k] for k in want} == want
    assert s["device_index_bytes"] == 0


@pytest.mark.parametrize("which", ["delta_one", "random"])
def test_plans_without_blocks_are_accepted(engine, which):
    if which == "delta_one":
        M, N, ro, ci = bt.blocked_pattern()
        delta = 1.0
    else:
        M, N, ro, ci = synth.random_pattern(100, 3000, 900, seed=3)
        delta = 0.3
    csr = engine.CSR.from_arrays(M, N, ro, ci)
    arrays = engine.Pipeline(csr, alpha=0.3, delta=delta, device=-1).arrays()
    st, s = engine.blocked_check_status(M, N, ro, ci, arrays)
    assert st == engine.OK
    assert s["blocks"] == 0 and s["panels_with_blocks"] == 0 and s["residue_entries"] == ci.size
    assert {k: s[k] for k in bt.numpy_stats(M, N, ro, ci, arrays)} == bt.numpy_stats(M, N, ro, ci, arrays)


def _first_full_cell_pair(arrays, same):
    """(block, i1, j1, i2, j2) of two non-empty cells of one block in one column (same = "col") or one row ("row")"""
    bv = arrays["blockValues"].reshape(-1, 16, 16)
    for b in range(bv.shape[0]):
        full = bv[b] != NULL
        for a in range(16):
            line = full[:, a] if same == "col" else full[a, :]
            idx = np.flatnonzero(line)
            if idx.size >= 2:
                return (b, idx[0], a, idx[1], a) if same == "col" else (b, a, idx[0], a, idx[1])
    raise AssertionError("no such pair")


def _corrupt(name, case):
    M, N, ro, ci, arrays = case
    a = bt.copy_arrays(arrays)
    bv = a["blockValues"].reshape(-1, 16, 16)      # a view: writes land in a["blockValues"]
    if name == "index_missing":
        b, i, j, _, _ = _first_full_cell_pair(a, "row")
        bv[b, i, j] = NULL
    elif name == "index_twice_in_cells":
        b, i, j1, _, j2 = _first_full_cell_pair(a, "row")
        bv[b, i, j2] = bv[b, i, j1]
    elif name == "index_twice_in_residue":
        a["sparseValues"][1] = a["sparseValues"][0]
        a["sparseRelativeRows"][1] = a["sparseRelativeRows"][0]
        a["sparseColIndices"][1] = a["sparseColIndices"][0]
    elif name == "index_in_cell_and_residue":
        b, i, j, _, _ = _first_full_cell_pair(a, "row")
        a["sparseValues"][0] = bv[b, i, j]
    elif name == "index_out_of_range":
        a["sparseValues"][0] = ci.size
    elif name == "cell_in_wrong_row":
        b, i1, j, i2, _ = _first_full_cell_pair(a, "col")
        bv[b, i1, j], bv[b, i2, j] = bv[b, i2, j], bv[b, i1, j]
    elif name == "cell_in_wrong_column":
        b, i, j1, _, j2 = _first_full_cell_pair(a, "row")
        bv[b, i, j1], bv[b, i, j2] = bv[b, i, j2], bv[b, i, j1]
    elif name == "cell_in_padding_column":
        b, i, j, _, _ = _first_full_cell_pair(a, "row")
        a["denseCols"][16 * b + j] = N
    elif name == "column_id_above_N":
        pad = np.flatnonzero(a["denseCols"] == N)
        a["denseCols"][pad[0]] = N + 1
    elif name == "residue_relative_row":
        a["sparseRelativeRows"][0] = (a["sparseRelativeRows"][0] + 1) % 16
    elif name == "residue_relative_row_range":
        a["sparseRelativeRows"][0] = 16
    elif name == "residue_column":
        a["sparseColIndices"][0] = (a["sparseColIndices"][0] + 1) % N
    elif name == "block_offsets_not_monotone":
        a["blockOffsets"][2] = a["blockOffsets"][3] + 1
    elif name == "sparse_offsets_not_monotone":
        a["sparseValueOffsets"][1] = a["sparseValueOffsets"][2] + 1
    elif name == "offsets_start":
        a["sparseValueOffsets"][0] = 1
    elif name == "row_twice":
        a["reorderedRows"][1] = a["reorderedRows"][0]
    elif name == "row_out_of_range":
        a["reorderedRows"][0] = M
    else:
        raise KeyError(name)
    return a


CORRUPTIONS = ["index_missing", "index_twice_in_cells", "index_twice_in_residue", "index_in_cell_and_residue",
               "index_out_of_range", "cell_in_wrong_row", "cell_in_wrong_column", "cell_in_padding_column",
               "column_id_above_N", "residue_relative_row", "residue_relative_row_range", "residue_column",
               "block_offsets_not_monotone", "sparse_offsets_not_monotone", "offsets_start", "row_twice", "row_out_of_range"]


@pytest.mark.parametrize("name", CORRUPTIONS)
def test_each_corruption_is_a_bad_plan(engine, case, name):
    assert _check(engine, case)[0] == engine.OK
    st, _ = _check(engine, case, _corrupt(name, case))
    assert st == engine.ERR_BAD_PLAN


def test_panel_count_must_match_the_rows(engine, case):
    M, N, ro, ci, arrays = case
    d, keep = engine.rphm_desc(M, N, ci.size, arrays)
    s = engine.BlockedStats()
    call = lambda: engine.hip().bsmr_blocked_check(M, N, ci.size, ro.ctypes.data, ci.ctypes.data, C.byref(d), C.byref(s),
                                                   C.sizeof(s))
    assert call() == engine.OK
    d.num_nonzero_rows -= 16
    assert call() == engine.ERR_BAD_PLAN


def test_invalid_arguments(engine, case):
    M, N, ro, ci, arrays = case
    hip = engine.hip()
    s = engine.BlockedStats()
    nnz = int(ci.size)
    d, keep = engine.rphm_desc(M, N, nnz, arrays)
    rop, cip = ro.ctypes.data, ci.ctypes.data
    size = C.sizeof(s)
    assert hip.bsmr_blocked_check(M, N, nnz, rop, cip, C.byref(d), C.byref(s), size) == engine.OK
    assert hip.bsmr_blocked_check(M, N, nnz, rop, cip, None, C.byref(s), size) == engine.ERR_INVALID_ARG
    assert hip.bsmr_blocked_check(M, N, nnz, rop, cip, C.byref(d), None, size) == engine.ERR_INVALID_ARG
    assert hip.bsmr_blocked_check(M, N, nnz, None, cip, C.byref(d), C.byref(s), size) == engine.ERR_INVALID_ARG
    assert hip.bsmr_blocked_check(M, N, nnz, rop, None, C.byref(d), C.byref(s), size) == engine.ERR_INVALID_ARG
    # sizes that disagree with the CSR: in the call (row_offsets[M] != nnz, a column id >= N) and in the desc
    assert hip.bsmr_blocked_check(M - 1, N, nnz, rop, cip, C.byref(d), C.byref(s), size) == engine.ERR_INVALID_ARG
    assert hip.bsmr_blocked_check(M, N, nnz - 1, rop, cip, C.byref(d), C.byref(s), size) == engine.ERR_INVALID_ARG
    assert hip.bsmr_blocked_check(M, int(ci.max()), nnz, rop, cip, C.byref(d), C.byref(s), size) == engine.ERR_INVALID_ARG
    for field in ("M", "N", "nnz"):
        d2, keep2 = engine.rphm_desc(M, N, nnz, arrays)
        setattr(d2, field, getattr(d2, field) + 1)
        assert hip.bsmr_blocked_check(M, N, nnz, rop, cip, C.byref(d2), C.byref(s), size) == engine.ERR_INVALID_ARG
    for field in ("block_offsets", "sparse_value_offsets", "reordered_rows", "block_values", "dense_cols", "sparse_values"):
        d2, keep2 = engine.rphm_desc(M, N, nnz, arrays)
        setattr(d2, field, None)
        assert hip.bsmr_blocked_check(M, N, nnz, rop, cip, C.byref(d2), C.byref(s), size) == engine.ERR_INVALID_ARG
    # out_size bounds what is written
    raw = (C.c_uint8 * size)(*([0xAB] * size))
    assert hip.bsmr_blocked_check(M, N, nnz, rop, cip, C.byref(d), C.cast(raw, C.POINTER(engine.BlockedStats)), 8) == engine.OK
    assert bytes(raw[8:]) == b"\xab" * (size - 8) and bytes(raw[:8]) != b"\xab" * 8


def test_calls_on_a_null_handle(engine):
    hip = engine.hip()
    d = engine.RphmDesc()
    s = engine.BlockedStats()
    assert hip.bsmr_backward_attach_blocks(None, C.byref(d)) == engine.ERR_INVALID_ARG
    assert hip.bsmr_backward_attach_blocks(None, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_backward_get_blocked_stats(None, C.byref(s), C.sizeof(s)) == engine.ERR_INVALID_ARG
    for K in (32, 48, 0):   # the handle is checked first, as in bsmr_spmm
        assert hip.bsmr_spmm_blocked(None, K, None, None, None, 1, None) == engine.ERR_INVALID_ARG
        assert hip.bsmr_spmm_blocked_16(None, K, None, None, None, 1, engine.COMPUTE_F16, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_abi_revision() == 5


def test_twin_against_hand_derived_bits(engine, oracle):
    """One ragged panel of three rows, one block whose last column is padding, three residue entries, K = 1.
    Block columns 0 .. 14 (+ padding); x = 1 except x[1] = a = 1 + 2^-12 and x[4] = 5.  e = 2^-24 = half an ulp of 1.
      row 0  cells j = 0, 2, 3 with v = 1, e, e (j = 1 is an EMPTY cell over x[1] = a); residue: columns 15, 16, 17, v = e.
             B: fmaf(1, 1, +0) = 1; the empty cell leaves 1; 1 + e is a tie and rounds to even: 1, twice.  B = 1.
             R: e, 2e, 3e - exact.  Y = fl(1 + 3e): a tie between 1 + 2e (odd) and 1 + 4e (even) -> 1 + 2^-22.
             (One chain in CSR order, as the plain gather runs it, gives 1: five ties in a row.)
      row 1  cells j = 0, 1 with v = -1, a.  fmaf(-1, 1, +0) = -1; fmaf(a, a, -1) = 2^-11 + 2^-24 exactly - one rounding
             per product (a multiply rounded on its own gives a a = 1 + 2^-11 and the sum 2^-11).
      row 2  cell j = 4 with v = -0: fmaf(-0, 5, +0) = +0, and +0 + R (+0) = +0."""
    M, N = 3, 20
    per_row = [[0, 2, 3, 15, 16, 17], [0, 1], [4]]
    ro = np.cumsum([0] + [len(r) for r in per_row]).astype(np.uint32)
    ci = np.concatenate(per_row).astype(np.uint32)
    bv = np.full((1, 16, 16), NULL, dtype=np.uint32)
    bv[0, 0, 0], bv[0, 0, 2], bv[0, 0, 3] = 0, 1, 2
    bv[0, 1, 0], bv[0, 1, 1] = 6, 7
    bv[0, 2, 4] = 8
    arrays = {"reorderedRows": np.arange(3, dtype=np.uint32),
              "denseCols": np.array(list(range(15)) + [N], dtype=np.uint32),
              "blockOffsets": np.array([0, 1], dtype=np.uint32), "blockValues": bv.reshape(-1),
              "sparseValueOffsets": np.array([0, 3], dtype=np.uint32),
              "sparseValues": np.array([3, 4, 5], dtype=np.uint32),
              "sparseRelativeRows": np.zeros(3, dtype=np.uint32),
              "sparseColIndices": np.array([15, 16, 17], dtype=np.uint32)}
    st, s = engine.blocked_check_status(M, N, ro, ci, arrays)
    assert st == engine.OK
    assert (s["panels"], s["blocks"], s["block_entries"], s["padding_columns"], s["residue_entries"]) == (1, 1, 6, 1, 3)
    e, a = np.float32(2.0 ** -24), np.float32(1 + 2.0 ** -12)
    v = np.array([1, e, e, e, e, e, -1, a, -0.0], dtype=np.float32)
    X = np.ones((N, 1), dtype=np.float32)
    X[1, 0], X[4, 0] = a, 5
    tw = bt.BlockedTwin(oracle, M, N, ro, ci, arrays)
    B, R = tw.parts(v, X)
    assert B[:, 0].tolist() == [1.0, 2.0 ** -11 + 2.0 ** -24, 0.0]
    assert R[:, 0].tolist() == [3 * 2.0 ** -24, 0.0, 0.0]
    Y = tw.twin(v, X)
    want = np.array([1 + 2.0 ** -22, 2.0 ** -11 + 2.0 ** -24, 0.0], dtype=np.float32)
    assert Y[:, 0].view(np.uint32).tolist() == want.view(np.uint32).tolist()      # row 2: +0, not -0
    # the same entries as one chain per row (the plain gather's contract) give other bits in row 0
    from gather_twin import gather, row_lists
    assert gather(oracle, row_lists(ro, ci), v, X)[:, 0].tolist() == [1.0, 2.0 ** -11 + 2.0 ** -24, 0.0]
