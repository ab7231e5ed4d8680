"""Row patterns that sit where the row clustering takes its shortcuts, and a census of what a sequential run meets on them,
for tests/test_clustering_exact.py (host pipeline) and tests/test_gpu_cluster.py (bsmr_cluster_rows).  Imports no product
code: the patterns are numpy, the census runs over oracle/bsmr_oracle.py (`encodings`, `similarity`).

What the shortcuts are (csrc/cluster_kernels.hpp, src/rowReordering.cpp): a similarity is only compared with alpha, so both
implementations decide it from the row's sparse (bin, count) list in double arithmetic and re-evaluate only pairs within 1e-4
of alpha in the reference's fp32 order (per-thread bin sums, 32-lane butterflies, a fold that skips warps); the comparison
is strict (reference src/rowReordering.cu:388); the representative's sum of squares is a 32-bit accumulator that wraps.

  uniform_rows   every bin count is 1, so two rows of n bins that share i of them have similarity i / (2n - i) in exact
                 arithmetic - with alpha at (or one ulp beside) such a value, whether fp32 lands on, above or below it depends
                 on the block's order of additions, and many pairs sit exactly on alpha
  wrap_pattern   every row fills bin 0; with a bin width of 256 the representative's count there reaches 65 536 after 256
                 rows and its square is 0 modulo 2^32
  census         the sequential clustering restated once more, counting the comparisons of each kind; the same walk with
                 another verdict in place of the reference's (`sequential_clustering`) shows that a case can fail"""
import functools

import numpy as np

import bsmr_oracle as bo

BAND = 1e-4   # pairs this close to alpha are re-evaluated in the reference's order of operations

F32 = np.float32
THIRD_BELOW = float(np.nextafter(F32(1) / F32(3), F32(0)))   # the fp32 neighbour below f32(1/3)
SIX_TENTHS = float(F32(0.6))

U20 = tuple(range(9))                              # 20 bins: one warp
U300 = (0, 1, 2, 3, 5, 8, 13, 21, 40)              # 300 bins: 96 threads, warp 2 of 3 is skipped (none of these bins lies there)
U1250 = (0, 1, 33, 70, 100, 130, 161, 200, 260)    # 1 250 bins: 320 threads, bin 130 lies in a skipped warp (4 of 10)


def _csr(per_row, cols):
    ro = np.zeros(len(per_row) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([c.size for c in per_row])
    return len(per_row), cols, ro, np.concatenate(per_row).astype(np.uint32)


def uniform_rows(rows, universe, sizes, bw, bins, seed):
    """rows of n (drawn from `sizes`) distinct bins of `universe`, one column in each: every bin count is 1"""
    rng = np.random.default_rng(seed)
    universe = np.asarray(universe, dtype=np.int64)
    assert universe.max() < bins
    per = []
    for _ in range(rows):
        n = int(rng.choice(sizes))
        b = np.sort(rng.choice(universe, size=n, replace=False))
        per.append(b * bw + rng.integers(0, bw, n))
    return _csr(per, bins * bw)


def wrap_pattern(rows, bw, bins, seed):
    """every row holds all bw columns of bin 0 and one column in one of bins 1 to 5"""
    rng = np.random.default_rng(seed)
    assert bins > 5
    per = []
    for _ in range(rows):
        b = int(rng.integers(1, 6))
        per.append(np.concatenate([np.arange(bw), [b * bw + int(rng.integers(0, bw))]]).astype(np.int64))
    return _csr(per, bins * bw)


def live_bins(num_bins):
    """which bins enter the reference's block-wide sums (include/cudaUtil.cuh:37-43: the fold of the per-warp values reads
    only some warps when their number is not a power of two), found by running bsmr_oracle.block_sum on unit vectors"""
    threads = bo.cluster_threads(num_bins)
    warp_live = [bo.block_sum(np.repeat(np.eye(threads // 32, dtype=np.float64)[w], 32)) != 0 for w in range(threads // 32)]
    return np.asarray([warp_live[(b % threads) // 32] for b in range(num_bins)], dtype=bool)


def quotient_f64(rep, row, live):
    """The similarity's quotient the way both implementations first form it: the norms as executed (sqrtf of the wrapped
    32-bit sums of squares over the bins that count), the min-sum and the max-sum in float64."""
    x, y = rep[live].astype(np.int64), row[live].astype(np.int64)
    sx, sy = int(np.sum(x * x)) & 0xFFFFFFFF, int(np.sum(y * y)) & 0xFFFFFFFF
    if sx == 0 and sy == 0:
        return 1.0
    if sx == 0 or sy == 0:
        return 0.0
    a = x / float(np.sqrt(F32(sx)))
    c = y / float(np.sqrt(F32(sy)))
    return float(np.minimum(a, c).sum() / np.maximum(a, c).sum())


def similarity_norm64(rep, row):
    """bsmr_oracle.similarity with sums of squares that do NOT wrap (a 64-bit norm): what the reference does not compute"""
    threads = bo.cluster_threads(rep.size)
    sx = int(bo.block_sum(bo.per_thread((rep * rep).astype(np.uint64), threads)))
    sy = int(bo.block_sum(bo.per_thread((row * row).astype(np.uint64), threads)))
    if sx == 0 and sy == 0:
        return F32(1.0)
    if sx == 0 or sy == 0:
        return F32(0.0)
    a = rep.astype(F32) / np.sqrt(F32(sx))
    c = row.astype(F32) / np.sqrt(F32(sy))
    mn = bo.block_sum(bo.per_thread(np.minimum(a, c), threads))
    mx = bo.block_sum(bo.per_thread(np.maximum(a, c), threads))
    return F32(mn / mx)


VERDICTS = ("reference", "float64", "greater_equal", "norm64")


def sequential_clustering(rows, cols, ro, ci, alpha, bw, verdict="reference", similarity=None):
    """bsmr_oracle.row_reordering's walk (reference src/rowReordering.cu:325-432, :939-995, :1082-1090) with a verdict of choice
    and a census.  Returns (reorderedRows, numClusters, census).

    verdict  "reference"      fp32 block-order similarity > alpha: what the reference computes
             "float64"        the float64 quotient > alpha: an implementation that never re-evaluates near alpha
             "greater_equal"  fp32 block-order similarity >= alpha
             "norm64"         fp32 block order, sums of squares that do not wrap
    census   comparisons; near = float64 quotient within BAND of alpha; equal = fp32 similarity == alpha; flips = the fp32
             verdict differs from the float64 one; wrapped = the representative's true sum of squares over the bins that
             count is >= 2^32; cluster_sizes in cluster order (the census describes the walk actually taken, so it is
             the reference's only under verdict "reference")
    similarity: the fp32 block-order evaluation, bsmr_oracle.similarity unless given (oracle/clustering_oracle.c's is the
    same function, tests/test_clustering_exact.py, and faster)."""
    assert verdict in VERDICTS
    similarity = similarity or bo.similarity
    alpha32 = F32(alpha)
    alpha64 = float(alpha32)
    enc, disp = bo.encodings(rows, cols, ro, ci, bw)
    live = live_bins(enc.shape[1])
    order = np.argsort(disp, kind="stable")
    cluster = np.full(rows, -1, dtype=np.int64)
    z = 0
    while z < rows and disp[order[z]] == 0:
        cluster[z] = 0
        z += 1
    census = dict(comparisons=0, near=0, equal=0, flips=0, wrapped=0, cluster_sizes=[])
    cid, start = 1, z
    while start < rows:
        cluster[start] = cid
        rep = enc[order[start]].copy()
        size, nxt = 1, -1
        for p in range(start + 1, rows):
            if cluster[p] != -1:
                continue
            row = enc[order[p]]
            s32 = F32(similarity(rep, row))
            s64 = quotient_f64(rep, row, live)
            census["comparisons"] += 1
            census["near"] += abs(s64 - alpha64) <= BAND
            census["equal"] += bool(s32 == alpha32)
            census["flips"] += bool(s32 > alpha32) != (s64 > alpha64)
            census["wrapped"] += int(np.sum(rep[live] * rep[live])) >= 1 << 32
            if verdict == "reference":
                joins = s32 > alpha32
            elif verdict == "float64":
                joins = s64 > alpha64
            elif verdict == "greater_equal":
                joins = s32 >= alpha32
            else:
                joins = similarity_norm64(rep, row) > alpha32
            if joins:
                cluster[p] = cid
                rep += row
                size += 1
            elif nxt < 0:
                nxt = p
        census["cluster_sizes"].append(size)
        if nxt < 0:
            break
        start = nxt
        cid += 1
    pos = np.argsort(cluster, kind="stable")
    perm = order[pos]
    num_clusters = int(cluster[pos][pos[-1]]) + (1 if z != 0 else 0) if rows else 0
    k = 0
    while k < rows and ro[perm[k] + 1] - ro[perm[k]] == 0:
        k += 1
    census = {k_: (int(v) if not isinstance(v, list) else v) for k_, v in census.items()}
    return perm[k:].astype(np.uint32), num_clusters, census


def census(rows, cols, ro, ci, alpha, bw, similarity=None):
    """what the reference's sequential run meets on the pattern (see sequential_clustering)"""
    return sequential_clustering(rows, cols, ro, ci, alpha, bw, "reference", similarity)[2]


# --------------------------------------------------------------------------------------------------------------------------
# The cases.  name -> (generator, arguments, bin width, alpha).  All tie cases: 200 rows, bin width 16, seed 5 but for one.
# --------------------------------------------------------------------------------------------------------------------------
ROWS, BW, SEED = 200, 16, 5
TIE_CASES = {
    # flips: pairs whose fp32 block-order verdict differs from the float64 one
    "b20-s4-third": (uniform_rows, (ROWS, U20, (4,), BW, 20, SEED), BW, THIRD_BELOW),
    "b20-s46-half": (uniform_rows, (ROWS, U20, (4, 6), BW, 20, SEED), BW, 0.5),
    "b300-s4-third": (uniform_rows, (ROWS, U300, (4,), BW, 300, SEED), BW, THIRD_BELOW),
    "b300-s46-third": (uniform_rows, (ROWS, U300, (4, 6), BW, 300, SEED), BW, THIRD_BELOW),
    # (seed 2: 3 flips; seed 5 has 1, seed 7 has 2, and of the fp32 neighbours of 1/3, 1/2, 3/5 only 1/2 itself has any)
    "b1250-s4-half": (uniform_rows, (ROWS, U1250, (4,), BW, 1250, 2), BW, 0.5),
    # pairs exactly on alpha: 4-bin rows that share 3 bins, 3 / 5 = f32(0.6) in either bin count
    "b20-s4-sixtenths": (uniform_rows, (ROWS, U20, (4,), BW, 20, SEED), BW, SIX_TENTHS),
    "b300-s4-sixtenths": (uniform_rows, (ROWS, U300, (4,), BW, 300, SEED), BW, SIX_TENTHS),
}
FLIP_CASES = [n for n in TIE_CASES if not n.endswith("sixtenths")]
EQUAL_CASES = [n for n in TIE_CASES if n.endswith("sixtenths")]
WRAP_CASES = {
    "wrap-0.3": (wrap_pattern, (700, 256, 20, 3), 256, 0.3),
    "wrap-0.9": (wrap_pattern, (700, 256, 20, 3), 256, 0.9),
}
ALL_CASES = {**TIE_CASES, **WRAP_CASES}
MIN_FLIPS = {n: 5 for n in FLIP_CASES}
MIN_FLIPS["b1250-s4-half"] = 2
MIN_EQUAL = 1000
MIN_WRAPPED = 500


@functools.lru_cache(maxsize=None)
def case_pattern(name):
    """(rows, cols, rowOffsets, colIndices, bin width, alpha) of a case; shared by the tests, never modified"""
    gen, args, bw, alpha = ALL_CASES[name]
    rows, cols, ro, ci = gen(*args)
    ro.setflags(write=False)
    ci.setflags(write=False)
    return rows, cols, ro, ci, bw, alpha


_census_cache = {}


def case_census(name, similarity=None):
    """census of a case, computed once per process and per source of the fp32 similarity (numpy when none is given)"""
    key = (name, similarity is None)
    if key not in _census_cache:
        rows, cols, ro, ci, bw, alpha = case_pattern(name)
        _census_cache[key] = census(rows, cols, ro, ci, alpha, bw, similarity)
    return _census_cache[key]


def assert_case_is_loaded(name, c):
    """the conditions a case has to meet on its own input, so that a changed generator cannot empty it"""
    if name in MIN_FLIPS:
        assert c["flips"] >= MIN_FLIPS[name], (name, c)
        assert c["near"] >= c["flips"], (name, c)
    if name in EQUAL_CASES:
        assert c["equal"] >= MIN_EQUAL, (name, c)
    if name in WRAP_CASES:
        assert c["wrapped"] >= MIN_WRAPPED and c["cluster_sizes"][0] == 256, (name, c)
