"""Row clustering: the product's sparse / incremental evaluation against the plain dense
restatement (oracle/clustering_oracle.c), bit for bit.

The reference's block-wide sum (include/cudaUtil.cuh:14-45) skips some warps when the
thread count of the clustering block (src/rowReordering.cu:912-922) is not a power-of-two
number of warps; the cases below walk through 1, 3, 5, 6, 7, 10 and 32 warps, rows that
live entirely in skipped bins, and alphas outside (0, 1)."""
import numpy as np
import pytest

import synth

import bsmr_oracle as bo
import cluster_patterns as cp


def clustered_pattern(rows, cols, groups, per_row, seed, noise=0.3):
    """rows drawn around `groups` column prototypes so that clusters actually form"""
    rng = np.random.default_rng(seed)
    protos = [rng.choice(cols, size=min(cols, 3 * per_row), replace=False) for _ in range(groups)]
    per = []
    for r in range(rows):
        g = rng.integers(groups)
        k = max(1, int(rng.integers(per_row // 2, per_row + 1)))
        own = rng.choice(protos[g], size=min(k, protos[g].size), replace=False)
        extra = rng.choice(cols, size=max(0, int(noise * k)), replace=False)
        per.append(np.unique(np.concatenate([own, extra])))
    ro = np.zeros(rows + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([c.size for c in per])
    return rows, cols, ro, np.concatenate(per).astype(np.uint32)


def test_thread_count_and_skipped_warps(oracle):
    # (bins, threads) from src/rowReordering.cu:912-922
    for nb, threads in ((1, 32), (31, 32), (32, 32), (160, 64), (300, 96), (520, 160), (768, 192),
                        (800, 224), (1250, 320), (4500, 1024), (100000, 1024)):
        assert oracle.lib.oracle_cluster_threads(nb) == threads == bo.cluster_threads(nb)
    live = {nb: sorted(set((np.nonzero(oracle.cluster_bin_mask(nb))[0] % t) // 32))
            for nb, t in ((300, 96), (520, 160), (768, 192), (800, 224), (1250, 320), (4500, 1024))}
    assert live[300] == [0, 1]                      # 3 warps: stride 1 only, warp 2 never read
    assert live[520] == [0, 1, 2, 3]                # 5 warps: strides 2, 1
    assert live[768] == [0, 1, 3, 4]                # 6 warps: strides 3, 1
    assert live[800] == [0, 1, 3, 4]                # 7 warps: strides 3, 1
    assert live[1250] == [0, 1, 2, 3, 5, 6, 7, 8]   # 10 warps: strides 5, 2, 1
    assert live[4500] == list(range(32))


def test_similarity_restatements_agree(oracle):
    rng = np.random.default_rng(5)
    for nb in (20, 300, 768, 1250):
        for _ in range(20):
            rep = (rng.random(nb) < 0.2) * rng.integers(1, 40, nb)
            row = (rng.random(nb) < 0.1) * rng.integers(1, 17, nb)
            a = oracle.cluster_similarity(rep, row)
            b = float(bo.similarity(rep.astype(np.int64), row.astype(np.int64)))
            assert a == b, (nb, a, b)
    # all-zero and one-sided cases (src/rowReordering.cu:263-268)
    z = np.zeros(40, np.uint32)
    one = z.copy()
    one[3] = 2
    assert oracle.cluster_similarity(z, z) == 1.0
    assert oracle.cluster_similarity(z, one) == 0.0 == oracle.cluster_similarity(one, z)
    # a row that only touches bins of a skipped warp looks empty to the block
    hidden = np.zeros(300, np.uint32)
    hidden[70] = 5                                   # thread 70 -> warp 2 of 3
    seen = np.zeros(300, np.uint32)
    seen[10] = 5
    assert oracle.cluster_similarity(hidden, hidden) == 1.0
    assert oracle.cluster_similarity(seen, hidden) == 0.0


CASES = [
    # rows, cols, bin width, groups, nnz per row, seed
    (300, 320, 16, 6, 12, 1),        # 20 bins, one warp
    (400, 4800, 16, 8, 20, 2),       # 300 bins, 3 warps
    (400, 8320, 16, 8, 24, 3),       # 520 bins, 5 warps
    (500, 12288, 16, 10, 30, 4),     # 768 bins, 6 warps
    (300, 16000, 20, 6, 40, 5),      # 800 bins, 7 warps
    (600, 20000, 16, 12, 16, 6),     # 1250 bins, 10 warps
    (200, 72000, 16, 4, 60, 7),      # 4500 bins, 1024 threads
]


@pytest.mark.parametrize("case", CASES, ids=[f"bins{-(-c[1] // c[2])}" for c in CASES])
@pytest.mark.parametrize("alpha", [0.1, 0.3, 0.6, 0.9])
def test_product_order_equals_dense_restatement(engine, oracle, case, alpha):
    rows, cols, bw, groups, per_row, seed = case
    rows, cols, ro, ci = clustered_pattern(rows, cols, groups, per_row, seed)
    perm, clusters = oracle.bsa_row_reordering(rows, cols, ro, ci, bw, alpha)
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    pipe = engine.Pipeline(csr, alpha=alpha, delta=0.3, block_size=bw, device=-1)
    assert np.array_equal(pipe.array("reorderedRows"), perm)
    assert pipe.num_clusters == clusters
    if alpha == 0.1:
        assert clusters < rows        # the pattern does cluster


@pytest.mark.parametrize("alpha", [-0.5, 0.0, 0.3, 1.0, 1.5])
def test_rows_hidden_in_skipped_bins_and_extreme_alphas(engine, oracle, alpha):
    """300 bins / 3 warps: bins whose thread sits in warp 2 never enter a sum, so rows made
    only of them have 'zero' norm - similarity 1 among themselves, 0 with everything else."""
    rng = np.random.default_rng(11)
    cols, bw = 4800, 16
    hidden_bins = [b for b in range(300) if (b % 96) >= 64]
    per = []
    for r in range(120):
        if r % 3 == 0:                # hidden rows
            bins = rng.choice(hidden_bins, size=4, replace=False)
        elif r % 3 == 1:              # mixed
            bins = np.concatenate([rng.choice(hidden_bins, size=2, replace=False), rng.integers(0, 64, 3)])
        else:
            bins = rng.integers(0, 64, 5)
        per.append(np.unique(bins * bw + rng.integers(0, bw, bins.size)))
    per[7] = np.zeros(0, np.int64)   # an empty row -> cluster 0, dropped from the order
    ro = np.zeros(len(per) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([c.size for c in per])
    ci = np.concatenate(per).astype(np.uint32)
    perm, clusters = oracle.bsa_row_reordering(len(per), cols, ro, ci, bw, alpha)
    csr = engine.CSR.from_arrays(len(per), cols, ro, ci)
    pipe = engine.Pipeline(csr, alpha=alpha, delta=0.3, block_size=bw, device=-1)
    assert np.array_equal(pipe.array("reorderedRows"), perm)
    assert pipe.num_clusters == clusters
    assert 7 not in perm and perm.size == len(per) - 1
    if alpha == 0.3:
        # all hidden rows end up in one cluster: contiguous in the order
        pos = sorted(int(np.nonzero(perm == r)[0][0]) for r in range(0, 120, 3))
        assert pos[-1] - pos[0] == len(pos) - 1


def test_numpy_restatement_on_small_input(engine, oracle):
    rows, cols, ro, ci = clustered_pattern(60, 4800, 4, 10, 21)
    for alpha in (0.2, 0.5):
        perm, clusters = oracle.bsa_row_reordering(rows, cols, ro, ci, 16, alpha)
        rr, nc = bo.row_reordering(rows, cols, ro, ci, alpha, 16)
        assert np.array_equal(rr, perm) and nc == clusters


# ------------------------------------------------------------------------------------------------------------------------
# Ties with alpha, pairs exactly on alpha, a representative whose squared norm wraps (tests/cluster_patterns.py)
# ------------------------------------------------------------------------------------------------------------------------
def oracle_result(oracle, name):
    rows, cols, ro, ci, bw, alpha = cp.case_pattern(name)
    return oracle.bsa_row_reordering(rows, cols, ro, ci, bw, alpha)


def test_bins_that_count_restated(oracle):
    for nb in (20, 300, 520, 768, 800, 1250, 4500):
        assert np.array_equal(cp.live_bins(nb), oracle.cluster_bin_mask(nb)), nb


@pytest.mark.parametrize("name", list(cp.ALL_CASES))
def test_host_pipeline_on_ties_and_wrapped_norms(engine, oracle, name):
    """The case meets its own conditions (>= 5 flips, >= 2 at 1 250 bins; >= 1 000 pairs on alpha; >= 500 comparisons with
    a wrapped norm and a first cluster of exactly 256 rows), and the host pipeline gives the C oracle's row order and
    cluster count on it.

    Census of the reference's sequential run per case (numpy restatement; `near` = float64 quotient within 1e-4 of alpha,
    `equal` = fp32 similarity == alpha, `flips` = fp32 block-order verdict differs from the float64 one, `wrapped` = the
    representative's true sum of squares is >= 2^32; clusters = number of clusters formed):
      case                 alpha                  comparisons  near   equal  flips  wrapped  clusters
      b20-s4-third         nextafter(f32(1/3),0)          394    18      13     13        0         6
      b20-s46-half         0.5                           1096    18      14      8        0        22
      b300-s4-third        nextafter(f32(1/3),0)          385    16       6      6        0         6
      b300-s46-third       nextafter(f32(1/3),0)          271    17       5      5        0         5
      b1250-s4-half        0.5 (seed 2)                  1822    77      77      3        0        28
      b20-s4-sixtenths     f32(0.6)                      8984  1460    1460      0        0       100
      b300-s4-sixtenths    f32(0.6)                      8984  1460    1460      0        0       100
      wrap-0.3, wrap-0.9   0.3, 0.9                      1329     0       0      0      632         3 (256, 256, 188 rows)
    """
    rows, cols, ro, ci, bw, alpha = cp.case_pattern(name)
    cp.assert_case_is_loaded(name, cp.case_census(name))
    want, want_clusters = oracle_result(oracle, name)
    pipe = engine.Pipeline(engine.CSR.from_arrays(rows, cols, ro, ci), alpha=alpha, delta=0.3, block_size=bw, device=-1)
    assert np.array_equal(pipe.array("reorderedRows"), want)
    assert pipe.num_clusters == want_clusters


@pytest.mark.parametrize("name", [n for n in cp.ALL_CASES if n.startswith(("b20-", "wrap-"))])
def test_numpy_restatement_on_ties_and_wrapped_norms(oracle, name):
    """bsmr_oracle.row_reordering and the census' own walk equal the C oracle; the census is the same whether the fp32
    similarity comes from numpy or from C"""
    rows, cols, ro, ci, bw, alpha = cp.case_pattern(name)
    want, want_clusters = oracle_result(oracle, name)
    rr, nc = bo.row_reordering(rows, cols, ro, ci, alpha, bw)
    assert np.array_equal(rr, want) and nc == want_clusters
    perm, clusters, census = cp.sequential_clustering(rows, cols, ro, ci, alpha, bw, "reference", oracle.cluster_similarity)
    assert np.array_equal(perm, want) and clusters == want_clusters
    assert census == cp.case_census(name)


def defect_differs(oracle, name, verdict):
    rows, cols, ro, ci, bw, alpha = cp.case_pattern(name)
    want, want_clusters = oracle_result(oracle, name)
    # the walk itself is the oracle's: only the verdict can make the difference below
    perm, clusters, _ = cp.sequential_clustering(rows, cols, ro, ci, alpha, bw, "reference", oracle.cluster_similarity)
    assert np.array_equal(perm, want) and clusters == want_clusters
    perm, clusters, _ = cp.sequential_clustering(rows, cols, ro, ci, alpha, bw, verdict, oracle.cluster_similarity)
    return not np.array_equal(perm, want) or clusters != want_clusters


@pytest.mark.parametrize("name", cp.FLIP_CASES)
def test_a_float64_verdict_fails_the_flip_cases(oracle, name):
    """an implementation that never re-evaluated pairs near alpha in the reference's fp32 order would not pass"""
    assert defect_differs(oracle, name, "float64")


@pytest.mark.parametrize("name", cp.EQUAL_CASES)
def test_greater_equal_fails_the_cases_on_alpha(oracle, name):
    assert defect_differs(oracle, name, "greater_equal")


@pytest.mark.parametrize("name", list(cp.WRAP_CASES))
def test_a_64_bit_norm_fails_the_wrap_cases(oracle, name):
    """with a squared norm that does not wrap all 700 rows form one cluster"""
    rows, cols, ro, ci, bw, alpha = cp.case_pattern(name)
    perm, clusters, census = cp.sequential_clustering(rows, cols, ro, ci, alpha, bw, "norm64", oracle.cluster_similarity)
    assert census["cluster_sizes"] == [700]
    assert defect_differs(oracle, name, "norm64")


def limit_pattern(bins, bw=16, rows=48, seed=9):
    """48 rows around 3 column prototypes over bins * bw columns; every third row also holds the last column"""
    cols = bins * bw
    _, _, ro, ci = clustered_pattern(rows, cols, 3, 12, seed)
    per = [ci[ro[r]:ro[r + 1]] for r in range(rows)]
    for r in range(0, rows, 3):
        per[r] = np.union1d(per[r], [cols - 1]).astype(np.uint32)
    ro = np.zeros(rows + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([c.size for c in per])
    return rows, cols, ro, np.concatenate(per).astype(np.uint32)


@pytest.mark.parametrize("bins", [40944, 40945])
def test_host_pipeline_around_the_device_histogram_limit(engine, oracle, bins):
    """40 944 bins is the largest row histogram bsmr_cluster_rows takes (numBins * 4 <= 160 KiB - 64); from 40 945 on the
    pipeline clusters on the host.  The host implementation equals the oracle on both sides (tests/test_gpu_cluster.py
    runs the device on them)."""
    rows, cols, ro, ci = limit_pattern(bins)
    assert int(ci.max()) // 16 == bins - 1
    for alpha in (0.1, 0.3):
        want, want_clusters = oracle.bsa_row_reordering(rows, cols, ro, ci, 16, alpha)
        pipe = engine.Pipeline(engine.CSR.from_arrays(rows, cols, ro, ci), alpha=alpha, delta=0.3, block_size=16, device=-1)
        assert np.array_equal(pipe.array("reorderedRows"), want) and pipe.num_clusters == want_clusters
