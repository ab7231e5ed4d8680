"""Every reachable instantiation of the residue kernels (sparseEntries, sparseEntriesLowp) on exact operands.

The residue kernels are templates over lanes per entry, chunks per lane (a tuned shape, or 0: the run-time K loop), the
form (panel rows staged in LDS, panel rows from global memory, free) and, in 16 bits, whether A arrives as fp32 and is
rounded while it is staged.  Which instantiation a call runs follows from K, the mode and the plan options; each case
below asserts through plan_stats() and sparse_choice() that it ran the form, lanes and precision it is named after.

Operands are signed integers, |v| <= 127 up to K = 1024 (K * 127^2 < 2^24) and |v| <= 63 at K = 2048: exact in fp16 and
bf16, and every product and partial sum is exact in fp32, so every kernel returns the integer dot product whatever its
summation order.  Expected values are numpy int64 dot products, compared with ==.

Pattern R: all residue (delta = 1.1), 64 x 80, natural row order, four row panels of 1280, 150, 70 and 1 entries.  With
256 entries per item the items hold 256 (five of them), 150, 70 and 1 entries: 64, 32 or 16 entries per round at 4, 8
or 16 lanes give 1, 2, 3 and >= 4 rounds, both parities of the round count in the two-buffer loop, and last rounds that
are only partly live.
Pattern H: the random generator of rand-hybrid (tests/test_gpu_numerics.py) at 32 x 160 with 409 entries - the smallest
of the sizes tried (rows 32 ... 112, columns 64 ... 220, density 0.08 ... 0.15) that has a dense part and a residue panel
of more than 64 entries (70 and 62), so that the 16-bit kernel makes a second round at 4 lanes per entry.

Reached, of the 73 instantiations: all 19 of sparseEntries and all 54 of sparseEntriesLowp."""
import numpy as np
import pytest

import rphm_desc
import synth
from test_gpu_numerics import Plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TUNED_KS = (32, 64, 128, 256, 512)
B_ONLY = dict(b_only=1, b_only_work_m=1)      # all-sparse plans: modes 0 / 1 convert B alone, the kernel rounds A (A_FP32)
HYBRID = dict(fold_dense_below=0, promote_average=0, convert_in_kernel=0)


class Pat:
    def __init__(self, engine, name, rows, cols, ro, ci, delta, arrays=None):
        self.name, self.rows, self.cols, self.delta = name, rows, cols, delta
        self.ro = np.ascontiguousarray(ro, dtype=np.uint32)
        self.ci = np.ascontiguousarray(ci, dtype=np.uint32)
        self.nnz = int(self.ci.size)
        self.csr = engine.CSR.from_arrays(rows, cols, self.ro, self.ci)
        if arrays is None:
            arrays = engine.Pipeline(self.csr, alpha=0.3, delta=delta, device=-1).arrays()
        self.arrays = arrays
        self.row_of = np.repeat(np.arange(rows), np.diff(self.ro.astype(np.int64)))


def _pattern_r(engine):
    rows, cols = 64, 80
    m = np.zeros((rows, cols), dtype=bool)
    m[0:16, :] = True                                   # 1280
    for i in range(16):                                 # 150 = 16 * 9 + 6
        m[16 + i, (np.arange(9 + (i < 6)) * 7 + i) % cols] = True
    for i in range(16):                                 # 70 = 16 * 4 + 6
        m[32 + i, (np.arange(4 + (i < 6)) * 11 + 3 * i) % cols] = True
    m[48, 41] = True                                    # 1
    ro = np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.uint32)
    ci = np.nonzero(m)[1].astype(np.uint32)
    arrays = rphm_desc.oracle_arrays(rows, cols, ro, ci, None, 1.1)     # natural row order: the panels as laid out above
    per_panel = np.diff(np.asarray(arrays["sparseValueOffsets"]).astype(np.int64)).tolist()
    assert per_panel == [1280, 150, 70, 1], per_panel
    return Pat(engine, "R", rows, cols, ro, ci, 1.1, arrays)


class Bench:
    """patterns, plans (one per pattern and option set) and operands (one pair per pattern and K) of the module"""

    def __init__(self, engine):
        self.engine = engine
        self.pats = {"R": _pattern_r(engine), "H": Pat(engine, "H", *synth.random_pattern(32, 160, 409, seed=11), 0.1)}
        self.plans, self.data = {}, {}

    def plan(self, pname, **opts):
        key = (pname, tuple(sorted(opts.items())))
        if key not in self.plans:
            self.plans[key] = Plan(self.engine, self.pats[pname], opts)
        return self.plans[key]

    def operands(self, pname, K, problem=0):
        """(A, B, the exact results as int64), computed once"""
        key = (pname, K, problem)
        if key not in self.data:
            pat = self.pats[pname]
            rng = np.random.default_rng([K, problem, len(pname), pat.nnz])
            hi = 127 if K <= 1024 else 63
            A = rng.integers(-hi, hi + 1, size=(pat.rows, K))
            B = rng.integers(-hi, hi + 1, size=(pat.cols, K))
            want = np.einsum("ek,ek->e", A[pat.row_of], B[pat.ci.astype(np.int64)])
            A32, B32 = A.astype(np.float32), B.astype(np.float32)
            want.setflags(write=False)
            self.data[key] = (A32, B32, want)
        return self.data[key]

    def close(self):
        for p in self.plans.values():
            p.close()


@pytest.fixture(scope="module")
def bench(engine):
    b = Bench(engine)
    yield b
    b.close()


def lanes_of(K, lowp, sparse_lpe=0):
    """lanes per entry of the residue kernel: the tuned shapes at K = 32 ... 512, else 8, or what the plan was told"""
    chunks = K // (8 if lowp else 4)
    if sparse_lpe:
        lpe = sparse_lpe
        while lpe > 1 and lpe > chunks:
            lpe //= 2
        return lpe
    if K in TUNED_KS:
        return (4 if K <= 128 else 8) if lowp else (4 if K <= 64 else 8 if K <= 256 else 16)
    return 8


def check(bench, pname, K, mode, lowp, opts, free=False):
    plan = bench.plan(pname, **opts)
    pat = bench.pats[pname]
    where = f"{pname} K={K} mode={mode} {opts}"
    st = plan.plan_stats()
    if pname == "R":
        assert st["num_dense_entries"] == 0 and st["num_sparse_entries"] == pat.nnz, where
    else:
        assert st["num_dense_entries"] > 0 and st["num_sparse_entries"] > 0 and st["folded_dense_entries"] == 0, where
    assert st["free_residue"] == (1 if free else 0), where
    A, B, want = bench.operands(pname, K)
    got = plan.run(K, A, B, mode)
    choice = plan.sparse_choice(K, mode)
    assert choice["low_precision"] == lowp, (where, choice)
    assert choice["lanes_per_entry"] == lanes_of(K, lowp, opts.get("sparse_lpe", 0)), (where, choice)
    bad = np.flatnonzero(got.astype(np.float64) != want.astype(np.float64))
    assert bad.size == 0, f"{where}: {bad.size} entries differ; first {bad[:5].tolist()}: got {got[bad[:5]].tolist()} " \
                          f"want {want[bad[:5]].tolist()}"
    return got


@pytest.mark.parametrize("K", TUNED_KS)
def test_tuned_shapes_over_a_staged_panel(bench, K):
    """R: the pipelined loops.  Mode 2: sparseEntries<LPE, true, CPL>; modes 0 / 1 on a plan that converts B alone:
    sparseEntriesLowp<LPE, MODE, true, CPL, false, true>."""
    for mode in (0, 1, 2):
        check(bench, "R", K, mode, mode != 2, B_ONLY)


@pytest.mark.parametrize("lpe", (0, 4, 8, 16))
def test_run_time_loop_over_a_staged_panel(bench, lpe):
    """R, K = 96 (no tuned shape), default and forced lanes: sparseEntries<LPE, true, 0> and, with fp32 A,
    sparseEntriesLowp<LPE, MODE, true, 0, false, true> (16 lanes: K = 256, since 96 / 8 chunks admit 8 lanes)."""
    opts = dict(B_ONLY, sparse_lpe=lpe) if lpe else B_ONLY
    for mode in (0, 1, 2):
        check(bench, "R", 96, mode, mode != 2, opts)
    if lpe == 16:
        for mode in (0, 1):
            check(bench, "R", 256, mode, True, opts)


@pytest.mark.parametrize("lpe", (0, 4, 16))
def test_fp32_panel_too_large_for_lds(bench, lpe):
    """R, mode 2, K = 1024: 16 x (1024 + 4) floats exceed 64 KiB, the A rows come from global memory:
    sparseEntries<LPE, false, 0>."""
    check(bench, "R", 1024, 2, False, dict(B_ONLY, sparse_lpe=lpe) if lpe else B_ONLY)


@pytest.mark.parametrize("K", TUNED_KS + (96,))
def test_free_form(bench, K):
    """R with free_residue = 1: sparseEntries<LPE, false, CPL, true> in mode 2, sparseEntriesLowp<LPE, MODE, false, CPL,
    true> in modes 0 / 1 (the residue is large enough for the plan to convert both operands); at K = 96 also with 4
    and 16 lanes."""
    for lpe in ((0, 4, 16) if K == 96 else (0,)):
        opts = dict(B_ONLY, free_residue=1, **(dict(sparse_lpe=lpe) if lpe else {}))
        for mode in (0, 1, 2):
            check(bench, "R", K, mode, mode != 2, opts, free=True)
    if K == 96:     # 16 lanes in 16 bits need 16 chunks of 8
        for mode in (0, 1):
            check(bench, "R", 256, mode, True, dict(B_ONLY, free_residue=1, sparse_lpe=16), free=True)


@pytest.mark.parametrize("K", TUNED_KS + (96,))
def test_hybrid_residue_from_the_converted_copies(bench, K):
    """H, modes 0 / 1: the conversion pass runs for the dense part and the residue reads the 16-bit copies, staged:
    sparseEntriesLowp<LPE, MODE, true, CPL>; at K = 96 also with 4 lanes, at K = 256 with the run-time loop on 16."""
    for mode in (0, 1):
        check(bench, "H", K, mode, True, HYBRID)
        if K == 96:
            check(bench, "H", K, mode, True, dict(HYBRID, sparse_lpe=4))
        if K == 256:
            check(bench, "H", K, mode, True, dict(HYBRID, sparse_lpe=16))


@pytest.mark.parametrize("lpe", (0, 4, 16))
def test_hybrid_residue_panel_too_large_for_lds(bench, lpe):
    """H, K = 2048: 16 x (4096 + 16) bytes exceed 64 KiB: sparseEntriesLowp<LPE, MODE, false, 0>."""
    for mode in (0, 1):
        check(bench, "H", 2048, mode, True, dict(HYBRID, sparse_lpe=lpe) if lpe else HYBRID)


@pytest.mark.parametrize("K", (64, 96))
def test_hybrid_residue_free_form(bench, K):
    """H with free_residue = 1: sparseEntriesLowp<LPE, MODE, false, CPL, true>."""
    for mode in (0, 1):
        check(bench, "H", K, mode, True, dict(HYBRID, free_residue=1), free=True)


@pytest.mark.parametrize("pname,mode,opts", [("R", 2, B_ONLY), ("H", 0, HYBRID)], ids=["R-fp32", "H-fp16"])
def test_batch_equals_single_calls(bench, pname, mode, opts):
    """one two-problem bsmr_sddmm_batch call at K = 64: each problem equals its single call (and the exact result)"""
    K = 64
    plan = bench.plan(pname, **opts)
    problems = [bench.operands(pname, K, problem=b) for b in (0, 1)]
    singles = [plan.run(K, A, B, mode) for A, B, _ in problems]
    both = plan.run_batch(K, [(A, B) for A, B, _ in problems], mode)
    for b, (_, _, want) in enumerate(problems):
        assert np.array_equal(both[b], singles[b]), (pname, b)
        assert np.array_equal(both[b].astype(np.float64), want.astype(np.float64)), (pname, b)
