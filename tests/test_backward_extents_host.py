"""The builders and position helpers of tests/test_gpu_backward_extents.py at a wrap threshold of 2^12 elements and K = 4,
where everything fits on the host: the patterns really hold far, alias and sign-window positions, a far row and its alias
hold different data and give different twins (so a wrapped index could not pass), the empty far rows exist, and the
crossing arithmetic of cases S and V selects what the GPU cases say it selects."""
import numpy as np
import pytest

from attention_twin import exact_forward, exact_scores
from gather_twin import CHUNK, col_lists, gather, row_lists
from test_gpu_backward_extents import (FAR, attention_far_pattern, batches_to_check, checked_rows, far_pattern,
                                       full_pattern_with_long_row, row_of_slot, slot_crossing, slot_table, split_rows_pattern,
                                       sub_rows)
from test_gpu_backward_twin import _fill_on_device, _sub_lists, narrow

torch = pytest.importorskip("torch")

T, K, M = 1 << 12, 4, 64


def _filled(rows, batch=0):
    t = torch.empty((rows, K), dtype=torch.float32)
    _fill_on_device(t, batch)
    return t.numpy()


@pytest.fixture(scope="module")
def case_r():
    N, ro, ci = far_pattern(M, T, K, seed=1)
    return N, ro, ci, checked_rows(T, K)


def test_case_r_holds_far_alias_and_sign_columns(case_r):
    N, ro, ci, rows = case_r
    wrap = T // K
    assert N == wrap + FAR and N * K > T and int(ci.max()) * K >= T
    assert (rows["far"] * K >= T).all() and (rows["far"] < N).all()
    assert np.array_equal(rows["alias"], rows["far"] - wrap) and (rows["alias"] * K < T // 2).all()
    lower, upper = rows["sign"][:FAR // 2], rows["sign"][FAR // 2:]
    assert (lower * K < T // 2).all() and (upper * K >= T // 2).all() and (upper * K < T).all()
    for name, part in (("far", rows["far"]), ("alias", rows["alias"]), ("sign, lower", lower), ("sign, upper", upper)):
        assert np.isin(part, ci).any(), name
    # columns: far ones with entries, far ones with none over an alias that has some
    n = np.diff(col_lists(M, N, ro, ci)[0].astype(np.int64))
    far_len, alias_len = n[rows["far"]], n[rows["alias"]]
    assert (far_len > 0).any() and (far_len == 0).any() and (alias_len[far_len == 0] > 0).any()
    # rows stay sorted and free of duplicates
    for r in range(M):
        assert (np.diff(ci[ro[r]:ro[r + 1]].astype(np.int64)) > 0).all()


def test_far_rows_and_their_aliases_differ_under_the_fill(case_r):
    N, _, _, rows = case_r
    X = _filled(N)
    for a, b in zip(rows["far"], rows["alias"]):
        assert (X[a] != X[b]).any()
    assert (X != _filled(N, batch=1)).any(axis=1).all()                       # ... and every batch differs in every row


def test_case_r_twins_of_far_and_alias_positions_differ(oracle, case_r):
    N, ro, ci, rows = case_r
    rng = np.random.default_rng(2)
    v = narrow(rng, ci.size)
    # rows: the twin over X against the twin over an X whose far rows are the alias rows (what a wrapped s K reads)
    X = _filled(N)
    wrapped = X.copy()
    wrapped[rows["far"]] = X[rows["alias"]]
    rl = row_lists(ro, ci)
    good, bad = gather(oracle, rl, v, X), gather(oracle, rl, v, wrapped)
    reads_far = np.array([np.isin(ci[ro[r]:ro[r + 1]], rows["far"]).any() for r in range(M)])
    assert reads_far.sum() >= 8 and (good[reads_far] != bad[reads_far]).any(axis=1).all()
    # columns: a far destination and its alias have different lists, so different rows (what a wrapped dest K overwrites)
    cl = col_lists(M, N, ro, ci)
    A = narrow(rng, (M, K))
    far = gather(oracle, _sub_lists(cl, rows["far"]), v, A)
    alias = gather(oracle, _sub_lists(cl, rows["alias"]), v, A)
    n = np.diff(cl[0].astype(np.int64))
    assert (far != alias).any(axis=1)[(n[rows["far"]] > 0) | (n[rows["alias"]] > 0)].all()
    assert (far.view(np.uint32)[n[rows["far"]] == 0] == 0).all()             # an empty list is +0


def test_case_o_pattern_and_twins(oracle):
    N = 640
    Mo, ro, ci, empty = attention_far_pattern(T, K, N, seed=3)
    wrap = T // K
    rows = checked_rows(T, K)
    lens = np.diff(ro.astype(np.int64))
    assert Mo == wrap + FAR and (Mo - 1) * K >= T
    assert (lens[empty] == 0).all() and lens.max() == CHUNK + 1 and set(lens.tolist()) == {0, 1, 2, 3, CHUNK + 1}
    far_empty = empty[np.isin(empty, rows["far"])]
    assert far_empty.size >= 3 and (lens[far_empty - wrap] > 0).all()         # empty far rows over non-empty aliases
    assert np.isin(empty, rows["alias"]).any() and np.isin(empty, rows["sign"]).any()
    assert lens[Mo - 1] == CHUNK + 1 == lens[Mo - 1 - wrap]
    first, slots = slot_table(ro)
    assert slots == 4 and first[Mo - 1] == 2 and first[Mo - 1 - wrap] == 0     # both are split rows: attnReduce writes them
    for r in range(Mo):
        assert np.unique(ci[ro[r]:ro[r + 1]]).size == lens[r]                   # distinct columns in every row
    # the twins of the far rows and of their aliases differ wherever either has entries
    rng = np.random.default_rng(4)
    p, e = exact_scores(ro, rng)
    V = rng.standard_normal((N, K)).astype(np.float32)
    out = {}
    for name in ("far", "alias"):
        sub_ro, sub_ci, idx = sub_rows(ro, ci, rows[name])
        assert np.array_equal(sub_ci, ci[idx]) and np.array_equal(np.diff(sub_ro.astype(np.int64)), lens[rows[name]])
        out[name] = exact_forward(oracle, sub_ro, sub_ci, e[idx], V)[0]
    either = (lens[rows["far"]] > 0) | (lens[rows["alias"]] > 0)
    assert (out["far"] != out["alias"]).any(axis=1)[either].all()
    assert (out["far"].view(np.uint32)[lens[rows["far"]] == 0] == 0).all()


def test_case_s_crossing_selects_a_split_row():
    Ms, N, nb = 40, 640, 13
    ro, ci = split_rows_pattern(Ms, N, CHUNK + 1, seed=13)
    for r in range(Ms):
        assert np.unique(ci[ro[r]:ro[r + 1]]).size == CHUNK + 1
    first, slots = slot_table(ro)
    assert slots == 2 * Ms and np.array_equal(first, 2 * np.arange(Ms))
    b, slot = slot_crossing(T, slots, K)
    assert (b, slot) == (12, 64) and b == nb - 1
    assert (b * slots + slot) * K >= T > (b * slots + slot - 1) * K and nb * slots * K > T
    d, k = row_of_slot(ro, slot)
    assert (d, k) == (32, 0) and ro[d + 1] - ro[d] > CHUNK
    assert row_of_slot(ro, slot + 1) == (32, 1) and row_of_slot(ro, slots - 1) == (Ms - 1, 1)
    # a table with unsplit rows in between
    mixed = np.array([0, 3, 3 + 1025, 3 + 1025 + 512, 3 + 1025 + 512 + 513], np.uint32)
    first, slots = slot_table(mixed)
    assert first.tolist() == [-1, 0, -1, 3] and slots == 5
    assert [row_of_slot(mixed, s) for s in range(5)] == [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1)]
    # the figures the GPU case asserts
    assert slot_crossing(1 << 32, 65568, 1024) == (63, 63520) and slot_crossing(1 << 31, 65568, 1024) == (31, 64544)


def test_case_v_batches_and_pattern():
    assert batches_to_check(T, 100, 45) == [0, 19, 20, 21, 39, 40, 41, 44]
    nnz = (1 << 17) + 300
    got = batches_to_check(1 << 32, nnz, 32800)
    c = (1 << 32) // nnz
    assert c * nnz <= 1 << 32 < (c + 1) * nnz and {0, c - 1, c, c + 1, 32799} <= set(got) and got[-1] * nnz > 1 << 32
    with pytest.raises(AssertionError):
        batches_to_check(T, 100, 41)                                           # no whole batch past the threshold
    N, ro, ci = full_pattern_with_long_row(512, 256, 300, 7)
    assert N == 556 and ci.size == nnz and int(ci.max()) == N - 1
    lens = np.diff(ro.astype(np.int64))
    assert lens[7] == 556 > CHUNK and (np.delete(lens, 7) == 256).all()
    first, slots = slot_table(ro)
    assert slots == 2 and first[7] == 0                                        # one long row: the block kernels run
    assert np.diff(col_lists(512, N, ro, ci)[0].astype(np.int64)).max() == CHUNK   # no split column
