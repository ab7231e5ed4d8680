"""Row clustering on the device (bsmr_cluster_rows) against the host implementation, the
plain dense restatement and the reference's published logs - identical row order and cluster
count everywhere; then on inputs that sit on its shortcuts (ties with alpha, wrapped norms, the
one-wave-per-item form and the long-row branch on small inputs, every scheduling knob, the LDS limit)."""
import ctypes as C
import json
import time
from pathlib import Path

import numpy as np
import pytest

import cluster_patterns as cp
import synth
from test_clustering_exact import CASES, clustered_pattern, limit_pattern

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).parent / "golden" / "reference_logs.json").read_text())["matrices"]


def logged_clusters(name, alpha):
    return next(r["bsmr_numClusters"] for r in GOLDEN[name]["runs"] if abs(r["alpha"] - alpha) < 1e-6)


@pytest.mark.parametrize("case", CASES, ids=[f"bins{-(-c[1] // c[2])}" for c in CASES])
@pytest.mark.parametrize("alpha", [0.1, 0.3, 0.6, 0.9])
def test_device_order_equals_host_and_oracle(engine, oracle, case, alpha):
    rows, cols, bw, groups, per_row, seed = case
    rows, cols, ro, ci = clustered_pattern(rows, cols, groups, per_row, seed)
    st, perm, clusters, stats = engine.cluster_rows_device(rows, cols, ro, ci, bw, alpha)
    assert st == engine.OK
    want, want_clusters = oracle.bsa_row_reordering(rows, cols, ro, ci, bw, alpha)
    assert np.array_equal(perm, want) and clusters == want_clusters
    pipe = engine.Pipeline(engine.CSR.from_arrays(rows, cols, ro, ci), alpha=alpha, delta=0.3, block_size=bw,
                           device=-1)
    assert np.array_equal(pipe.array("reorderedRows"), perm)
    assert stats["threads_per_pair"] == oracle.lib.oracle_cluster_threads(-(-cols // bw))


@pytest.mark.parametrize("alpha", [-0.5, 0.0, 0.3, 1.0, 1.5])
def test_device_edge_cases(engine, oracle, alpha):
    """empty rows, rows hidden in skipped bins, alphas outside (0, 1), a single row, no rows"""
    rng = np.random.default_rng(11)
    cols, bw = 4800, 16
    hidden_bins = [b for b in range(300) if (b % 96) >= 64]
    per = []
    for r in range(90):
        if r % 3 == 0:
            bins = rng.choice(hidden_bins, size=4, replace=False)
        elif r % 3 == 1:
            bins = np.concatenate([rng.choice(hidden_bins, size=2, replace=False), rng.integers(0, 64, 3)])
        else:
            bins = rng.integers(0, 64, 5)
        per.append(np.unique(bins * bw + rng.integers(0, bw, bins.size)))
    per[7] = np.zeros(0, np.int64)
    per[8] = np.zeros(0, np.int64)
    ro = np.zeros(len(per) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([c.size for c in per])
    ci = np.concatenate(per).astype(np.uint32)
    st, perm, clusters, _ = engine.cluster_rows_device(len(per), cols, ro, ci, bw, alpha)
    want, want_clusters = oracle.bsa_row_reordering(len(per), cols, ro, ci, bw, alpha)
    assert st == engine.OK and np.array_equal(perm, want) and clusters == want_clusters
    # one row / all rows empty
    st, perm, clusters, _ = engine.cluster_rows_device(1, 40, np.array([0, 2], np.uint32), np.array([3, 9], np.uint32), 16, alpha)
    assert st == engine.OK and perm.tolist() == [0] and clusters == 1
    st, perm, clusters, _ = engine.cluster_rows_device(3, 40, np.zeros(4, np.uint32), np.zeros(0, np.uint32), 16, alpha)
    assert st == engine.OK and perm.size == 0


@pytest.mark.parametrize("name,pattern,alphas", [
    ("mycielskian14", lambda: synth.mycielskian_pattern(14), (0.1, 0.3, 0.5, 0.7, 0.9)),
    ("Trefethen_20000", lambda: synth.trefethen_pattern(20000), (0.1, 0.3, 0.5, 0.7, 0.9)),
    ("wathen100", lambda: synth.wathen_pattern(100, 100), (0.3, 0.9)),
    ("mycielskian15", lambda: synth.mycielskian_pattern(15), (0.3,)),
])
def test_device_clustering_reproduces_reference_logs(engine, name, pattern, alphas):
    rows, cols, ro, ci = pattern()
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    for alpha in alphas:
        t0 = time.perf_counter()
        st, perm, clusters, stats = engine.cluster_rows_device(rows, cols, ro, ci, 16, alpha)
        wall = time.perf_counter() - t0
        assert st == engine.OK
        assert clusters == logged_clusters(name, alpha), (name, alpha)
        print(f"{name} alpha={alpha}: {clusters} clusters, device {stats['elapsed_ms']:.1f} ms (wall {wall * 1e3:.0f} ms), "
              f"{stats['passes']} passes, {stats['similarities']} similarities")
        if alpha == 0.3:
            pipe = engine.Pipeline(csr, alpha=alpha, delta=0.3, block_size=16, device=-1)
            assert np.array_equal(pipe.array("reorderedRows"), perm)


def test_clusters_running_ahead_give_the_host_order(engine):
    """A reddit-like row range (power-law degrees, most rows end in clusters of their own): the passes run ahead of the older
    clusters' decisions - tentative seeds, parked hits, drops - and the row order and cluster count are the host
    implementation's all the same."""
    rows, cols, ro, ci = synth.reddit_shard_like(rows=6000, seed=5)
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    bw = csr.calculate_block_size(200 << 30)
    for alpha in (0.3, 0.6):
        st, perm, clusters, stats = engine.cluster_rows_device(rows, cols, ro, ci, bw, alpha)
        assert st == engine.OK
        pipe = engine.Pipeline(csr, alpha=alpha, delta=0.3, block_size=bw, device=-1)
        assert np.array_equal(pipe.array("reorderedRows"), perm) and pipe.num_clusters == clusters
        assert stats["passes_ahead"] > 0, stats
        print(f"reddit-like 6000 rows alpha={alpha}: {clusters} clusters, {stats['passes']} passes ({stats['passes_ahead']} ahead), "
              f"{stats['dropped_seeds']} dropped seeds, device {stats['elapsed_ms']:.1f} ms")


def test_a_grid_larger_than_the_pass_keeps_the_host_order(engine, monkeypatch):
    """with many more workgroups than a pass has items (BSMR_CLUSTER_GRID = 65535), workgroups without an
    item are still being scheduled when the closing workgroup has written the next pass's state.  The state is kept in
    two copies used in turn (a launch reads one, its closing workgroup writes the other), so such a workgroup sees its
    own pass's state and leaves: row order and cluster count stay the host implementation's."""
    monkeypatch.setenv("BSMR_CLUSTER_GRID", "65535")
    rows, cols, ro, ci = synth.reddit_shard_like(rows=6000, seed=5)
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    bw = csr.calculate_block_size(200 << 30)
    for alpha in (0.3, 0.6):
        pipe = engine.Pipeline(csr, alpha=alpha, delta=0.3, block_size=bw, device=-1)
        for _ in range(3):
            st, perm, clusters, stats = engine.cluster_rows_device(rows, cols, ro, ci, bw, alpha)
            assert st == engine.OK
            assert np.array_equal(pipe.array("reorderedRows"), perm) and pipe.num_clusters == clusters, stats
    rows, cols, ro, ci = synth.mycielskian_pattern(12)
    for alpha in (0.3,):
        st, perm, clusters, stats = engine.cluster_rows_device(rows, cols, ro, ci, 16, alpha)
        pipe = engine.Pipeline(engine.CSR.from_arrays(rows, cols, ro, ci), alpha=alpha, delta=0.3, block_size=16, device=-1)
        assert st == engine.OK and np.array_equal(pipe.array("reorderedRows"), perm) and pipe.num_clusters == clusters


@pytest.mark.parametrize("rule", [1, 2])
def test_either_scheduling_rule_gives_the_host_order(engine, monkeypatch, rule):
    """BSMR_CLUSTER_RULE: 1 = clusters only judge what every older one has decided (round 2's rule, the kernel's cap on
    clusters that may run unconfirmed), 2 = the host switches between the two rules by the measured rows per millisecond,
    batch by batch.  What a pass may judge early changes, what the clusters are does not: row order and cluster count stay
    the host implementation's."""
    monkeypatch.setenv("BSMR_CLUSTER_RULE", str(rule))
    cases = [(synth.reddit_shard_like(rows=6000, seed=5), None), (synth.wathen_pattern(nx=30, ny=30), 16), (synth.nips_like(), None)]
    for (rows, cols, ro, ci), block in cases:
        csr = engine.CSR.from_arrays(rows, cols, ro, ci)
        bw = block or csr.calculate_block_size(200 << 30)
        for alpha in (0.3, 0.6):
            st, perm, clusters, stats = engine.cluster_rows_device(rows, cols, ro, ci, bw, alpha)
            assert st == engine.OK
            pipe = engine.Pipeline(csr, alpha=alpha, delta=0.3, block_size=bw, device=-1)
            assert np.array_equal(pipe.array("reorderedRows"), perm) and pipe.num_clusters == clusters, (rule, rows, alpha, stats)
            if rule == 1:
                assert stats["passes_ahead"] <= 1, stats


# ------------------------------------------------------------------------------------------------------------------------
# Inputs that sit where the passes take their shortcuts (tests/cluster_patterns.py; the census of every case is tabulated
# in tests/test_clustering_exact.py and asserted here on the test's own input).  Expected row order and cluster count come
# from oracle/clustering_oracle.c.
# ------------------------------------------------------------------------------------------------------------------------
def device_equals_oracle(engine, oracle, rows, cols, ro, ci, bw, alpha):
    st, perm, clusters, stats = engine.cluster_rows_device(rows, cols, ro, ci, bw, alpha)
    assert st == engine.OK
    want, want_clusters = oracle.bsa_row_reordering(rows, cols, ro, ci, bw, alpha)
    print(f"{rows} rows, {-(-cols // bw)} bins, alpha={alpha}: {clusters} clusters (oracle {want_clusters}), {stats['passes']} passes "
          f"({stats['passes_ahead']} ahead), {stats['similarities']} similarities, {stats['exact_similarities']} exact, "
          f"{stats['dropped_seeds']} dropped seeds, device {stats['elapsed_ms']:.1f} ms")
    assert np.array_equal(perm, want) and clusters == want_clusters, (clusters, want_clusters, stats)
    return stats


@pytest.mark.parametrize("name", list(cp.ALL_CASES))
def test_ties_with_alpha_and_wrapped_norms(engine, oracle, name):
    """Pairs whose fp32 block-order verdict differs from an accurate evaluation (>= 5 per case, >= 2 at 1 250 bins), >= 1 000
    pairs exactly on alpha (the comparison is strict), a representative whose squared norm wraps after 256 rows (>= 500
    comparisons behind the wrap).  Default grid: every pass is of the whole-workgroup form, which evaluates each pair in
    the reference's order of operations and counts it as an exact similarity.

    Census of the sequential run (comparisons / within 1e-4 of alpha / equal to alpha / flips / clusters formed):
      b20-s4-third 394 / 18 / 13 / 13 / 6      b20-s46-half 1096 / 18 / 14 / 8 / 22     b300-s4-third 385 / 16 / 6 / 6 / 6
      b300-s46-third 271 / 17 / 5 / 5 / 5      b1250-s4-half 1822 / 77 / 77 / 3 / 28    b20-, b300-s4-sixtenths 8984 / 1460 / 1460 / 0 / 100
      wrap-0.3, wrap-0.9: 1329 comparisons, 632 of them with a wrapped norm, clusters of 256, 256 and 188 rows"""
    rows, cols, ro, ci, bw, alpha = cp.case_pattern(name)
    cp.assert_case_is_loaded(name, cp.case_census(name, oracle.cluster_similarity))
    stats = device_equals_oracle(engine, oracle, rows, cols, ro, ci, bw, alpha)
    assert stats["exact_similarities"] > 0, stats


@pytest.mark.parametrize("name", list(cp.ALL_CASES))
def test_one_wave_per_item_form_on_small_inputs(engine, oracle, monkeypatch, name):
    """BSMR_CLUSTER_GRID=32, the smallest grid: the host switches to the one-wave-per-item form as soon as a batch judged
    more than 32 items per pass, which the 200-row cases (and the 700-row wrap case) do after the first batch of four
    passes - 200 rows were enough, no larger input was needed (MI355X: 2 807 to 9 007 similarities per tie case, 314 to 2 197
    of them re-evaluated exactly; 11 691 on the wrap case).  Only that form counts `similarities`: the double evaluation
    from the sparse list and the list of near pairs ran.  The workgroups also take several rounds each in the
    whole-workgroup passes before the switch.  Census per case: test_ties_with_alpha_and_wrapped_norms."""
    monkeypatch.setenv("BSMR_CLUSTER_GRID", "32")
    rows, cols, ro, ci, bw, alpha = cp.case_pattern(name)
    cp.assert_case_is_loaded(name, cp.case_census(name, oracle.cluster_similarity))
    stats = device_equals_oracle(engine, oracle, rows, cols, ro, ci, bw, alpha)
    assert stats["similarities"] > 0, stats
    if name in cp.TIE_CASES:
        # most pairs were decided by the double evaluation alone: the exact count holds the whole-workgroup passes before the
        # switch and the pairs near alpha (at most 1 460 of 8 984 comparisons in the census), not every pair
        assert 0 < stats["exact_similarities"] < stats["similarities"], stats


@pytest.mark.parametrize("alpha", [0.1, 0.15])
def test_long_rows_go_to_the_whole_workgroup(engine, oracle, monkeypatch, alpha):
    """BSMR_CLUSTER_LONG_ROW=64 (its minimum) against the default (2 048), both with grid 32: rows with more than 64
    (bin, count) entries leave the one-wave-per-item evaluation for the whole workgroup's.  400 rows over 4 500 bins: 362 of
    them have more than 64 entries (the longest 117), 38 have fewer (the shortest 55), so both evaluations run side by
    side.  The sequential run forms 23 clusters in 1 976 comparisons at alpha 0.1 and 178 clusters in 27 040 comparisons
    at 0.15."""
    monkeypatch.setenv("BSMR_CLUSTER_GRID", "32")
    rows, cols, ro, ci = clustered_pattern(400, 72000, 4, 90, 7)
    entries = np.array([np.unique(ci[ro[r]:ro[r + 1]] // 16).size for r in range(rows)])
    assert (entries > 64).sum() >= 100 and (entries <= 64).sum() >= 10, (entries.min(), entries.max())
    assert entries.max() <= 2048   # no row is long under the default
    short = device_equals_oracle(engine, oracle, rows, cols, ro, ci, 16, alpha)
    monkeypatch.setenv("BSMR_CLUSTER_LONG_ROW", "64")
    stats = device_equals_oracle(engine, oracle, rows, cols, ro, ci, 16, alpha)
    assert stats["similarities"] > 0 and short["similarities"] > 0, (stats, short)
    # every pair whose row is long is counted as an exact similarity, and 9 rows of 10 are long: more than half of what the
    # one-wave-per-item passes judged, and more than with the default threshold, under which only the pairs near alpha and
    # the whole-workgroup passes count (MI355X: 6 016 of 6 405 against 568 of 6 405 at alpha 0.1, 44 819 of 48 628 against
    # 5 653 of 48 476 at 0.15)
    assert 2 * stats["exact_similarities"] > stats["similarities"], stats
    assert stats["exact_similarities"] > short["exact_similarities"], (stats, short)


KNOBS = [("BSMR_CLUSTER_ACTIVE", 1), ("BSMR_CLUSTER_ACTIVE", 2), ("BSMR_CLUSTER_ACTIVE", 32),
         ("BSMR_CLUSTER_TENTATIVE", 0), ("BSMR_CLUSTER_TENTATIVE", 32), ("BSMR_CLUSTER_CHUNK", 32)]


def knob_inputs():
    """a tie case (6 clusters, the first of 105 rows), the case with 1 460 pairs on alpha (100 clusters) and a clustered
    pattern over 3 warps (332 clusters of 400 rows)"""
    rows, cols, bw, groups, per_row, seed = CASES[1]
    return {"b20-s4-third": cp.case_pattern("b20-s4-third"), "b300-s4-sixtenths": cp.case_pattern("b300-s4-sixtenths"),
            "clustered": clustered_pattern(rows, cols, groups, per_row, seed) + (bw, 0.3)}


def check_no_pass_ahead(stats, active):
    # clusters judge ahead of the older ones' decisions only while kClusterSpeculateFrom = 8 or more may run unconfirmed,
    # and that number never exceeds the clusters in flight (clusterPass: `tentative < maxActive`)
    if active < 8:
        assert stats["passes_ahead"] == 0, stats


@pytest.mark.parametrize("knob,value", KNOBS, ids=[f"{k[13:].lower()}{v}" for k, v in KNOBS])
def test_every_knob_keeps_the_result(engine, oracle, monkeypatch, knob, value):
    """One knob at a time on the default grid, where inputs of this size stay in the whole-workgroup form of a pass: the
    knobs shape the schedule - clusters in flight, clusters that may run unconfirmed, positions per pass - not the result."""
    monkeypatch.setenv(knob, str(value))
    for rows, cols, ro, ci, bw, alpha in knob_inputs().values():
        stats = device_equals_oracle(engine, oracle, rows, cols, ro, ci, bw, alpha)
        if knob == "BSMR_CLUSTER_ACTIVE":
            check_no_pass_ahead(stats, value)


@pytest.mark.parametrize("tentative", [0, 32])
@pytest.mark.parametrize("active", [1, 2, 32])
def test_knobs_together_in_the_one_wave_per_item_form(engine, oracle, monkeypatch, active, tentative):
    """BSMR_CLUSTER_ACTIVE x BSMR_CLUSTER_TENTATIVE, all at BSMR_CLUSTER_CHUNK=32 and BSMR_CLUSTER_GRID=32: the
    one-wave-per-item form runs under every combination (`similarities` > 0) and the result stays the oracle's.  The host
    switches to that form when a batch judged MORE items than 32 workgroups x passes.  With one cluster in flight and 32
    positions per pass only a cluster's first window (64 positions) is larger than that, so the tie case, whose few clusters
    take a row in nearly every pass, stays in the whole-workgroup form at ACTIVE=1 (measured: 0 similarities there, 2 591
    to 3 148 otherwise); the two inputs of many small clusters switch under every combination (6 596 to 10 299 and 26 969
    to 65 647 similarities)."""
    monkeypatch.setenv("BSMR_CLUSTER_GRID", "32")
    monkeypatch.setenv("BSMR_CLUSTER_CHUNK", "32")
    monkeypatch.setenv("BSMR_CLUSTER_ACTIVE", str(active))
    monkeypatch.setenv("BSMR_CLUSTER_TENTATIVE", str(tentative))
    for name, (rows, cols, ro, ci, bw, alpha) in knob_inputs().items():
        stats = device_equals_oracle(engine, oracle, rows, cols, ro, ci, bw, alpha)
        check_no_pass_ahead(stats, active)
        if active > 1 or name != "b20-s4-third":
            assert stats["similarities"] > 0, (name, stats)


def test_largest_histogram_that_fits_the_lds(engine, oracle):
    """40 944 bins: numBins * 4 = 160 KiB - 64, the largest row histogram bsmr_cluster_rows takes; 1 024 threads per pair"""
    rows, cols, ro, ci = limit_pattern(40944)
    for alpha in (0.1, 0.3):
        stats = device_equals_oracle(engine, oracle, rows, cols, ro, ci, 16, alpha)
        assert stats["threads_per_pair"] == 1024
    assert oracle.bsa_row_reordering(rows, cols, ro, ci, 16, 0.1)[1] < rows   # the pattern does cluster


def test_one_bin_more_is_declined_and_the_pipeline_falls_back(engine, oracle, monkeypatch):
    """40 945 bins: BSMR_ERR_OOM, the caller's arrays untouched; a pipeline asked to cluster on the device (explicit bin
    width 16: the automatic width, 107 columns here, never gets near the limit) falls back to the host implementation."""
    rows, cols, ro, ci = limit_pattern(40945)
    out = np.full(rows, 0xDEADBEEF, dtype=np.uint32)
    n, clusters, stats = C.c_uint32(0), C.c_int32(0), engine.ClusterStats()
    st = engine.hip().bsmr_cluster_rows(0, rows, cols, ro.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), 16, 0.3,
                                        out.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(clusters), C.byref(stats))
    assert st == engine.ERR_OOM
    assert (out == 0xDEADBEEF).all() and n.value == 0 and clusters.value == 0 and stats.passes == 0
    monkeypatch.setenv("BSMR_CLUSTER", "device")
    want, want_clusters = oracle.bsa_row_reordering(rows, cols, ro, ci, 16, 0.3)
    pipe = engine.Pipeline(engine.CSR.from_arrays(rows, cols, ro, ci), alpha=0.3, delta=0.3, block_size=16, device=0)
    assert np.array_equal(pipe.array("reorderedRows"), want) and pipe.num_clusters == want_clusters
