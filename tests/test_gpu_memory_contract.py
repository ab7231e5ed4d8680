"""Where every device entry point reads and writes: each call runs on guarded, minimally aligned buffers (tests/guarded.py)
and must leave the guards and its inputs bit for bit as they were, overwrite every element of its outputs, return the
reference result, and return the very bits of the same call on ordinary torch tensors (address independence).

The other GPU modules hand the library fresh torch tensors: 512-byte aligned, rounded up and carved out of shared blocks
by the caching allocator.  A store a few floats outside P, dA, Y or the 16-bit copies lands in a neighbour or in padding
there, a read past the last row of A, the last column of B or the last value of v finds zeros or an old tensor, and an
assumption of more than the documented alignment (16 bytes for operand matrices, 4 for value arrays, include/bsmr_hip.h
"Alignment") is always met.  Here the memory on both sides of every buffer holds a NaN pattern and every pointer is only
as aligned as the header asks for.

Operands are the exact families of tests/test_gpu_numerics.py (signed integers, dyadic fractions, power-of-two scales):
every product and partial sum is exact, so every path and mode must equal the fp64 oracle exactly and a single NaN from a
guard cannot hide in a tolerance.  bsmr_spmm, bsmr_sddmm_backward and the softmax backward are compared with their fp32
twins bit for bit, the softmax forward with its existing bound.  No tolerance is introduced here.

What this cannot see: a read beyond an operand that only feeds lanes whose results are masked out (padding rows of a
macro-tile, columns of a ragged 16-column block that no entry uses) changes no stored bit and is not detected; neither
is an overrun inside the plan's or the handle's own workspace.  The first is harmless numerically; where the GEMM engine
relies on a buffer descriptor's byte count to return zeros for such rows, these cases still prove that the count is not
too large for any row that reaches a result.  Guards are mapped memory of the buffer's own allocation: nothing here
relies on, or provokes, a fault.

Misaligned pointers are refused before any device work (BSMR_ERR_INVALID_ARG), so the last test may pass them: it asserts
the status and that no bit of any buffer changed."""
import ctypes as C
import zlib

import numpy as np
import pytest

import synth
from gather_twin import assert_twin, col_lists, gather, row_lists
from guarded import OPERAND, VALUES, Guarded, check_all
from softmax_twin import backward_twin, check_forward
from test_gpu_numerics import (BATCHED, PATHS, Pattern, Plan, _build, _pats, _through_copies, assert_exact, assert_path,
                               exact_ints, families, model, patterns)  # noqa: F401  (patterns: the module's fixture)
from test_gpu_softmax import lengths_pattern

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _in(name, a, offset, K):
    return Guarded.input(name, a, offset, K, _dev())


def _out(name, count, offset, K, dtype=np.float32):
    return Guarded.output(name, count, offset, K, _dev(), dtype=dtype)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float32, device=_dev())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_bits(got, plain, where):
    assert np.array_equal(_bits(got), _bits(plain)), f"{where}: guarded and plain buffers give different bits"


# ------------------------------------------------------------------------------------------------------------------
# patterns with the edges a kernel can trip over
# ------------------------------------------------------------------------------------------------------------------
def edge_pattern(empty_ends):
    """330 x 1500 nips-like (M % 16 = 10, N % 16 = 12) with columns 0 and N - 1 stored - in the first and the last row, or,
    with `empty_ends`, in their neighbours while the first and the last row are empty - and an odd number of entries"""
    rows, cols, ro, ci = synth.nips_like(rows=330, cols=1500, nnz=42000, seed=3)
    per_row = [set(ci[ro[r]:ro[r + 1]].tolist()) for r in range(rows)]
    a, b = (1, rows - 2) if empty_ends else (0, rows - 1)
    if empty_ends:
        per_row[0], per_row[rows - 1] = set(), set()
    per_row[a] |= {0, cols - 1}
    per_row[b] |= {0, cols - 1}
    if sum(len(s) for s in per_row) % 2 == 0:
        mid = rows // 2
        per_row[mid].discard(max(c for c in per_row[mid] if c != cols - 1))
    ro = np.concatenate([[0], np.cumsum([len(s) for s in per_row])]).astype(np.uint32)
    ci = np.concatenate([np.array(sorted(s), dtype=np.uint32) for s in per_row])
    return rows, cols, ro, ci


def assert_edges(pat, empty_ends):
    """the edges this module is about are in the pattern (a later change of synth cannot silently remove them)"""
    lens = np.diff(pat.ro.astype(np.int64))
    if empty_ends:
        assert lens[0] == 0 and lens[-1] == 0, pat.name
    else:
        assert lens[0] > 0 and lens[-1] > 0, pat.name
        assert pat.ci[0] == 0 and pat.ci[-1] == pat.cols - 1, pat.name     # (first row, column 0), (last row, column N - 1)
    assert (pat.ci == 0).any() and (pat.ci == pat.cols - 1).any(), pat.name   # the last row of B / X really is read
    assert pat.cols % 16 != 0 and pat.rows % 16 != 0, pat.name
    assert pat.nnz % 2 == 1, pat.name                                      # batch 1 of a value array starts on an odd float


EDGES = {"edge-dense": (False, 0.0), "edge-hybrid": (False, 0.1), "edge-sparse": (False, 1.1),
         "edgeE-hybrid": (True, 0.1), "edgeE-sparse": (True, 1.1)}


@pytest.fixture(scope="module")
def edges(engine):
    made = {}
    for name, (empty_ends, delta) in EDGES.items():
        made[name] = Pattern(engine, name, *edge_pattern(empty_ends), delta)
        assert_edges(made[name], empty_ends)
    return made


def _edge_pats(name):
    if name == "residue-b-only":
        return ("edge-sparse", "edgeE-sparse")
    if "pats" in PATHS[name]:                       # hybrid plans only
        return ("edge-hybrid", "edgeE-hybrid")
    return ("edge-dense", "edge-hybrid", "edgeE-hybrid")


# ------------------------------------------------------------------------------------------------------------------
# the forward calls on guarded buffers
# ------------------------------------------------------------------------------------------------------------------
def guarded_forward(engine, plan, K, problems, mode, entry="sddmm"):
    """bsmr_sddmm / _batch / _timed / bsmr_plan_tune on guarded buffers; problems: [(A, B), ...] (more than one: the batch
    entry).  Returns P as [batches, nnz]."""
    nb, nnz = len(problems), plan.pat.nnz
    gA = _in("A", np.concatenate([np.ravel(a) for a, _ in problems]), OPERAND, K)
    gB = _in("B", np.concatenate([np.ravel(b) for _, b in problems]), OPERAND, K)
    gP = _out("P", nb * nnz, VALUES, K)
    s = _stream()
    if entry == "batch":
        engine.sddmm_batch(plan.plan, K, gA.ptr, gB.ptr, gP.ptr, nb, mode, s)
    else:
        assert nb == 1
        if entry == "sddmm":
            engine.sddmm(plan.plan, K, gA.ptr, gB.ptr, gP.ptr, mode, s)
        elif entry == "timed":
            engine.sddmm_timed(plan.plan, K, gA.ptr, gB.ptr, gP.ptr, mode, s, warmup=0, iters=1)
        elif entry == "tune":
            engine.plan_tune(plan.plan, K, gA.ptr, gB.ptr, gP.ptr, mode, s)
        else:
            raise KeyError(entry)
    torch.cuda.synchronize()
    check_all(gA, gB, gP)
    return gP.numpy().reshape(nb, nnz)


def check_forward_case(engine, oracle, plan, K, A, B, mode, where, name=None, entry="sddmm"):
    """guards, the exact reference, the bits of the same call on plain tensors"""
    got = guarded_forward(engine, plan, K, [(A, B)], mode, entry)[0]
    if name is not None:
        assert_path(plan, name, K, mode)
    assert_exact(got, model(oracle, plan.pat, K, A, B, mode, plan.rounded(K, mode)), where)
    assert_same_bits(got, plan.run(K, A, B, mode), where)


def check_batch_case(engine, oracle, plan, K, problems, mode, where):
    got = guarded_forward(engine, plan, K, problems, mode, "batch")
    rounded = plan.rounded(K, mode)
    for b, (a, bb) in enumerate(problems):
        assert_exact(got[b], model(oracle, plan.pat, K, a, bb, mode, rounded), f"{where} batch {b}")
    assert_same_bits(got, plan.run_batch(K, problems, mode), where)


# ------------------------------------------------------------------------------------------------------------------
# 1. bsmr_sddmm and bsmr_sddmm_batch over the whole path matrix
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PATHS))
def test_every_path_stays_inside_the_buffers(engine, oracle, patterns, edges, name):
    """Every engine, macro-tile shape and operand variant of test_gpu_numerics.PATHS at each of its K, modes 0 / 1 / 2, on
    the five patterns of that module (all families) and on the edge patterns (integers, the smallest and the largest K);
    three batches on the BATCHED paths."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    ks = PATHS[name]["ks"]
    cases = [(patterns[p], ks, True) for p in _pats(name)] + [(edges[p], (ks[0], ks[-1]), False) for p in _edge_pats(name)]
    for pat, pat_ks, all_families in cases:
        plan = _build(engine, pat, name)
        try:
            for K in pat_ks:
                for fam, A, B in families(rng, pat, K):
                    if fam != "int" and not all_families:
                        continue
                    for mode in (0, 1, 2):
                        check_forward_case(engine, oracle, plan, K, A, B, mode, f"{name} {pat.name} K={K} {fam} mode={mode}",
                                           name=name if fam == "int" else None)
                if name in BATCHED and K in (64, 128, 512):
                    problems = [(exact_ints(rng, pat.rows, K, lo, hi), exact_ints(rng, pat.cols, K, -hi, -lo))
                                for lo, hi in ((-127, 127), (-50, 90), (-90, 50))]
                    for mode in (0, 1):
                        check_batch_case(engine, oracle, plan, K, problems, mode, f"{name} {pat.name} K={K} mode={mode}")
        finally:
            plan.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. the placement knobs that change how P is addressed
# ------------------------------------------------------------------------------------------------------------------
_STREAM = dict(convert_in_kernel=0, dense_group=1)
KNOBS = {
    "output-mode-0": dict(_STREAM, output_mode=0),
    "output-mode-1": dict(_STREAM, output_mode=1),
    "output-mode-2": dict(_STREAM, output_mode=2),
    "mask-tiles-0": dict(_STREAM, mask_tiles=0),
    "mask-tiles-1": dict(_STREAM, mask_tiles=1),
    "force-tile32": dict(convert_in_kernel=0, dense_group=2, force_tile32=1),
    "free-residue": dict(_STREAM, free_residue=1),
    "sparse-lpe-4": dict(_STREAM, sparse_lpe=4),
    "sparse-lpe-8": dict(_STREAM, sparse_lpe=8),
    "sparse-lpe-16": dict(_STREAM, sparse_lpe=16),
    "stream-waves-4": dict(_STREAM, stream_waves=4),
    "sweep-waves-8": dict(dense_engine=4, sweep_fp32=0, sweep_waves=8),
    "gemm-blocks-12": dict(dense_engine=5, gemm_fp32=0, gemm_panels=16, gemm_blocks=12),
    "gemm-natural-columns": dict(dense_engine=5, gemm_fp32=0, gemm_balance_columns=0),
}
KNOB_KS = (64, 512)      # (the path matrix above walks every K; the knobs change the addressing of P, not the K loop)


@pytest.mark.parametrize("knob", list(KNOBS))
def test_placement_knobs_stay_inside_the_buffers(engine, oracle, patterns, edges, knob):
    rng = np.random.default_rng(zlib.crc32(knob.encode()))
    for pat in (edges["edge-hybrid"], edges["edgeE-hybrid"], patterns["rand-hybrid"]):
        plan = Plan(engine, pat, dict(fold_dense_below=0, promote_average=0, **KNOBS[knob]))
        try:
            st = plan.plan_stats()
            assert st["num_dense_entries"] > 0 and st["num_sparse_entries"] > 0 and st["folded_dense_entries"] == 0, (knob, pat.name)
            assert st["free_residue"] == (1 if knob == "free-residue" else 0), (knob, pat.name)
            for K in KNOB_KS:
                A, B = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
                for mode in (0, 1, 2):
                    check_forward_case(engine, oracle, plan, K, A, B, mode, f"{knob} {pat.name} K={K} mode={mode}")
                    if mode != 2 and (knob.startswith("sweep") or knob.startswith("gemm")):
                        g = plan.dense_group(K)     # (of the call prepared last; mode 2 runs the exact-fp32 kernel)
                        assert g == 16 if knob == "gemm-blocks-12" else g >= 4, (knob, pat.name, K, mode, g)
                if knob.startswith("sparse-lpe"):       # the fp32 residue of mode 2 runs with the lanes asked for
                    assert plan.sparse_choice(K, 2)["lanes_per_entry"] == min(KNOBS[knob]["sparse_lpe"], K // 4)
        finally:
            plan.close()


def test_promoted_plan_stays_inside_the_buffers(engine, oracle):
    """promote_average at its default: residue entries of full panels run as extra dense blocks of the plan"""
    rows, cols, ro, ci = synth.community_graph(n=600, avg_degree=60, communities=5, seed=11)
    pat = Pattern(engine, "community-promoted", rows, cols, ro, ci, 0.3)
    plan = Plan(engine, pat, dict(fold_dense_below=0, **_STREAM))
    rng = np.random.default_rng(5)
    try:
        st = plan.plan_stats()
        rphm_dense = int((pat.arrays["blockValues"] != 0xFFFFFFFF).sum())
        assert 0 < rphm_dense < pat.nnz and st["promoted_sparse_entries"] > 0, st
        assert st["num_dense_entries"] == rphm_dense + st["promoted_sparse_entries"], st
        for K in KNOB_KS:
            A, B = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
            for mode in (0, 1, 2):
                check_forward_case(engine, oracle, plan, K, A, B, mode, f"promoted K={K} mode={mode}")
    finally:
        plan.close()


@pytest.mark.parametrize("shape", [(1, 40, 30), (5, 5, 2), (17, 33, 200), (300, 20, 1500)])
def test_tiny_shapes_stay_inside_the_buffers(engine, oracle, shape):
    """the shapes of test_gpu_parity.test_edge_shapes, all-dense, hybrid and all-sparse splits; plans with the small dense
    part on the dense kernels (fold_dense_below = 0) and with the shipping rules (folded into the residue)"""
    rows, cols, nnz = shape
    rows, cols, ro, ci = synth.random_pattern(rows, cols, nnz, seed=sum(shape))
    rng = np.random.default_rng(sum(shape))
    K = 64
    A, B = exact_ints(rng, rows, K), exact_ints(rng, cols, K)
    for delta in (0.0, 0.3, 1.1):
        pat = Pattern(engine, f"{shape} delta={delta}", rows, cols, ro, ci, delta)
        for opts in (dict(fold_dense_below=0, promote_average=0), dict()):
            plan = Plan(engine, pat, opts)
            try:
                for mode in (0, 1, 2):
                    check_forward_case(engine, oracle, plan, K, A, B, mode, f"{pat.name} {opts} mode={mode}")
            finally:
                plan.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. bsmr_sddmm_timed, bsmr_plan_tune
# ------------------------------------------------------------------------------------------------------------------
def test_timed_call_stays_inside_the_buffers(engine, oracle, edges):
    pat = edges["edge-hybrid"]
    rng = np.random.default_rng(41)
    for name in ("stream-pass", "gemm-16bit-16x20"):
        plan = _build(engine, pat, name)
        try:
            for K in (64, 128):
                A, B = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
                for mode in (0, 1, 2):
                    check_forward_case(engine, oracle, plan, K, A, B, mode, f"timed {name} K={K} mode={mode}", entry="timed")
        finally:
            plan.close()


def test_tuner_stays_inside_the_buffers(engine, oracle, edges):
    """bsmr_plan_tune runs every engine on the caller's buffers; P holds the correct result afterwards, and so does a
    call of the tuned plan"""
    pat = edges["edge-hybrid"]
    plan = Plan(engine, pat, dict(fold_dense_below=0, promote_average=0, dense_engine=engine.ENGINE_TUNED))
    rng = np.random.default_rng(43)
    try:
        assert plan.plan_stats()["num_dense_entries"] > 0 and plan.plan_stats()["num_sparse_entries"] > 0
        for K, mode in ((128, 0), (64, 1)):
            A, B = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
            where = f"tune K={K} mode={mode}"
            got = guarded_forward(engine, plan, K, [(A, B)], mode, "tune")[0]
            want = model(oracle, pat, K, A, B, mode, plan.rounded(K, mode))
            assert_exact(got, want, where)
            tA, tB, tP = _t(A.ravel()), _t(B.ravel()), _nan(pat.nnz)
            engine.plan_tune(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), mode, _stream())
            torch.cuda.synchronize()
            # (the second measurement may choose another engine: on these operands every engine is exact, so the
            # bits are the same whichever won)
            assert_exact(tP.cpu().numpy(), model(oracle, pat, K, A, B, mode, plan.rounded(K, mode)), where + " plain")
            assert_same_bits(got, tP.cpu().numpy(), where)
            check_forward_case(engine, oracle, plan, K, A, B, mode, where + " tuned call")
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. bsmr_convert_operands, bsmr_sddmm_lowp
# ------------------------------------------------------------------------------------------------------------------
def _bits16(oracle, mode, a):
    """the 16-bit patterns of oracle_round_fp16 / oracle_round_bf16 (values exactly representable after rounding)"""
    r = oracle.round_array(2 if mode == 0 else 3, np.ascontiguousarray(a, dtype=np.float32).ravel())
    if mode == 0:
        return r.astype(np.float16).view(np.uint16)
    return (r.view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.parametrize("name", ("stream-pass", "stream-fp32-residue", "gemm-16bit-8x20"))
def test_converted_copies_stay_inside_the_buffers(engine, oracle, edges, name):
    """bsmr_convert_operands writes exactly the M K and N K 16-bit elements of guarded A16 / B16 (bits of the oracle's
    rounding); bsmr_sddmm_lowp reads them - with the fp32 operands and, where the residue reads the copies, without."""
    rng = np.random.default_rng(47)
    for pname in ("edge-hybrid", "edgeE-hybrid"):
        pat = edges[pname]
        plan = _build(engine, pat, name)
        try:
            for K in (64, 512):
                A, B = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
                if K == 64:     # dyadic values: other 16-bit patterns than small integers
                    A, B = A * np.float32(2.0 ** -7), B * np.float32(2.0 ** -7)
                for mode in (0, 1):
                    where = f"{name} {pname} K={K} mode={mode}"
                    s = _stream()
                    gA, gB = _in("A", A, OPERAND, K), _in("B", B, OPERAND, K)
                    gA16 = _out("A16", pat.rows * K, OPERAND, K, dtype=np.uint16)
                    gB16 = _out("B16", pat.cols * K, OPERAND, K, dtype=np.uint16)
                    engine.convert_operands(plan.plan, K, gA.ptr, gB.ptr, gA16.ptr, gB16.ptr, mode, s)
                    torch.cuda.synchronize()
                    check_all(gA, gB, gA16, gB16)
                    assert np.array_equal(gA16.numpy(), _bits16(oracle, mode, A)), where + " A16"
                    assert np.array_equal(gB16.numpy(), _bits16(oracle, mode, B)), where + " B16"
                    gA16.freeze()
                    gB16.freeze()
                    plain, a16, b16 = _through_copies(engine, plan, K, A, B, mode)
                    assert np.array_equal(gA16.numpy(), a16) and np.array_equal(gB16.numpy(), b16), where
                    want = model(oracle, pat, K, A, B, mode, plan.rounded(K, mode))
                    residue_lowp = plan.sparse_choice(K, mode)["low_precision"]
                    assert residue_lowp == PATHS[name]["lowp"], where
                    for with_fp32 in (True, False):
                        if not with_fp32 and not residue_lowp:
                            continue            # (the fp32 residue needs A and B)
                        gP = _out("P", pat.nnz, VALUES, K)
                        engine.sddmm_lowp(plan.plan, K, gA16.ptr, gB16.ptr, gA.ptr if with_fp32 else None,
                                          gB.ptr if with_fp32 else None, gP.ptr, mode, s)
                        torch.cuda.synchronize()
                        check_all(gA, gB, gA16, gB16, gP)
                        assert_exact(gP.numpy(), want, f"{where} fp32 operands {with_fp32}")
                        assert_same_bits(gP.numpy(), plain, where)
        finally:
            plan.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. bsmr_batched_transpose
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (32, 32, 2), (33, 65, 3), (100, 7, 4), (5, 300, 1)])
def test_batched_transpose_stays_inside_the_buffers(engine, shape):
    width, height, nb = shape
    x = np.arange(nb * width * height, dtype=np.float32).reshape(nb, height, width) - 3
    gin, gout = _in("in", x, VALUES, 32), _out("out", x.size, VALUES, 32)
    engine.batched_transpose(width, height, nb, gin.ptr, gout.ptr, _stream())
    tx, ty = _t(x), _nan(x.size)
    engine.batched_transpose(width, height, nb, tx.data_ptr(), ty.data_ptr(), _stream())
    torch.cuda.synchronize()
    check_all(gin, gout)
    want = np.ascontiguousarray(x.transpose(0, 2, 1)).ravel()
    assert np.array_equal(_bits(gout.numpy()), _bits(want))
    assert_same_bits(gout.numpy(), ty.cpu().numpy(), f"transpose {shape}")


# ------------------------------------------------------------------------------------------------------------------
# 6. the handle's calls: bsmr_spmm, bsmr_sddmm_backward, bsmr_sparse_softmax and its backward
# ------------------------------------------------------------------------------------------------------------------
def lengths_transposed():
    """the transpose of test_gpu_softmax.lengths_pattern: columns of 1 ... 60 000 entries around the wave and chunk
    boundaries, interleaved with empty and short ones"""
    rows, cols, ro, ci = lengths_pattern()
    r = np.repeat(np.arange(rows), np.diff(ro.astype(np.int64)))
    order = np.lexsort((r, ci))                          # by new row (old column), then new column (old row)
    new_ro = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=cols))]).astype(np.uint32)
    return cols, rows, new_ro, r[order].astype(np.uint32)


class Handle:
    def __init__(self, engine, name, rows, cols, ro, ci):
        self.engine, self.name, self.rows, self.cols = engine, name, rows, cols
        self.ro = np.ascontiguousarray(ro, dtype=np.uint32)
        self.ci = np.ascontiguousarray(ci, dtype=np.uint32)
        self.nnz = int(self.ci.size)
        self.rl, self.cl = row_lists(self.ro, self.ci), col_lists(rows, cols, self.ro, self.ci)
        self.bw = engine.backward_create(rows, cols, self.ro, self.ci, device=0)


HANDLES = {"lengths": lengths_pattern, "lengths-transposed": lengths_transposed,
           "edge": lambda: edge_pattern(False), "edge-empty-ends": lambda: edge_pattern(True)}


@pytest.fixture(scope="module")
def handles(engine):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Handle(engine, name, *HANDLES[name]())
        return made[name]

    yield get
    for h in made.values():
        engine.backward_destroy(h.bw)


def test_handle_patterns_have_their_edges(engine, handles):
    h = handles("lengths")
    assert np.diff(h.ro.astype(np.int64)).max() == 60000 and (np.diff(h.ro.astype(np.int64)) == 0).any()
    t = handles("lengths-transposed")
    assert t.nnz == h.nnz and (t.rows, t.cols) == (h.cols, h.rows)
    col_lens = np.bincount(t.ci, minlength=t.cols)
    assert col_lens.max() == 60000 and (col_lens > 512).sum() >= 3          # columns cut into chunks
    st = engine.backward_stats(t.bw)
    assert st["split_cols"] >= 3 and st["max_col_length"] == 60000
    assert engine.backward_stats(h.bw)["split_rows"] >= 3
    for name, empty_ends in (("edge", False), ("edge-empty-ends", True)):
        assert_edges(handles(name), empty_ends)


def _f32(rng, *shape):
    return rng.standard_normal(shape, dtype=np.float32)


@pytest.mark.parametrize("nb", (1, 3))
@pytest.mark.parametrize("K", (32, 64, 128, 256))
@pytest.mark.parametrize("name", list(HANDLES))
def test_spmm_and_backward_stay_inside_the_buffers(engine, oracle, handles, name, K, nb):
    """bsmr_spmm with both values of `transpose`; bsmr_sddmm_backward with both outputs, dA alone and dB alone: guards and
    inputs intact, every output element written, the twin's bits, the bits of the same calls on plain tensors"""
    h = handles(name)
    rng = np.random.default_rng(zlib.crc32(f"{name} {K} {nb}".encode()))
    v, Xn, Xm = _f32(rng, nb, h.nnz), _f32(rng, nb, h.cols, K), _f32(rng, nb, h.rows, K)
    twin_rows = np.stack([gather(oracle, h.rl, v[b], Xn[b]) for b in range(nb)])      # S_v Xn   = dA with B = Xn
    twin_cols = np.stack([gather(oracle, h.cl, v[b], Xm[b]) for b in range(nb)])      # S_v^T Xm = dB with A = Xm
    s = _stream()
    where = f"{name} K={K} nb={nb}"
    tv, tXn, tXm = _t(v), _t(Xn), _t(Xm)

    def plain(call, rows):
        out = _nan(nb * rows * K)
        call(out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(nb, rows, K)

    gv, gXn, gXm = _in("v", v, VALUES, K), _in("Xn", Xn, OPERAND, K), _in("Xm", Xm, OPERAND, K)
    for transpose, gX, tX, rows, twin in ((False, gXn, tXn, h.rows, twin_rows), (True, gXm, tXm, h.cols, twin_cols)):
        gY = _out("Y", nb * rows * K, OPERAND, K)
        engine.spmm(h.bw, K, transpose, gv.ptr, gX.ptr, gY.ptr, nb, s)
        torch.cuda.synchronize()
        check_all(gv, gX, gY)
        got = gY.numpy().reshape(nb, rows, K)
        assert_twin(got, twin, f"{where} spmm transpose={transpose}")
        assert_same_bits(got, plain(lambda y: engine.spmm(h.bw, K, transpose, tv.data_ptr(), tX.data_ptr(), y, nb, s), rows),
                         f"{where} spmm transpose={transpose}")
    for want_dA, want_dB in ((True, True), (True, False), (False, True)):
        gdA = _out("dA", nb * h.rows * K, OPERAND, K) if want_dA else None
        gdB = _out("dB", nb * h.cols * K, OPERAND, K) if want_dB else None
        engine.sddmm_backward(h.bw, K, gv.ptr, gXm.ptr, gXn.ptr, gdA.ptr if gdA else None, gdB.ptr if gdB else None, nb, s)
        torch.cuda.synchronize()
        check_all(gv, gXm, gXn, gdA, gdB)
        tag = f"{where} backward dA={want_dA} dB={want_dB}"
        if gdA:
            got = gdA.numpy().reshape(nb, h.rows, K)
            assert_twin(got, twin_rows, tag + ": dA")
            assert_same_bits(got, plain(lambda y: engine.sddmm_backward(h.bw, K, tv.data_ptr(), tXm.data_ptr(), tXn.data_ptr(),
                                                                        y, None, nb, s), h.rows), tag + ": dA")
        if gdB:
            got = gdB.numpy().reshape(nb, h.cols, K)
            assert_twin(got, twin_cols, tag + ": dB")
            assert_same_bits(got, plain(lambda y: engine.sddmm_backward(h.bw, K, tv.data_ptr(), tXm.data_ptr(), tXn.data_ptr(),
                                                                        None, y, nb, s), h.cols), tag + ": dB")


@pytest.mark.parametrize("nb", (1, 3))
@pytest.mark.parametrize("name", list(HANDLES))
def test_softmax_stays_inside_the_buffers(engine, oracle, handles, name, nb):
    """bsmr_sparse_softmax and its backward, out of place and in place (Y = X, dX = dY)"""
    h = handles(name)
    rng = np.random.default_rng(zlib.crc32(f"softmax {name} {nb}".encode()))
    x, dY = _f32(rng, nb, h.nnz) * np.float32(5), _f32(rng, nb, h.nnz)
    scale = 0.7
    s = _stream()
    where = f"softmax {name} nb={nb}"
    K = 32                                               # (no inner dimension: the guards take their 2 MiB)
    # forward, out of place
    gX, gY = _in("X", x, VALUES, K), _out("Y", nb * h.nnz, VALUES, K)
    engine.sparse_softmax(h.bw, scale, gX.ptr, gY.ptr, nb, s)
    torch.cuda.synchronize()
    check_all(gX, gY)
    y = gY.numpy().reshape(nb, h.nnz)
    for b in range(nb):
        check_forward(h.ro, x[b], scale, y[b], f"{where} batch {b}")
    tx, ty = _t(x), _nan(nb * h.nnz)
    engine.sparse_softmax(h.bw, scale, tx.data_ptr(), ty.data_ptr(), nb, s)
    torch.cuda.synchronize()
    assert_same_bits(y, ty.cpu().numpy().reshape(nb, h.nnz), where)
    # forward, in place
    gXY = Guarded.inplace("X=Y", x, VALUES, K, _dev())
    engine.sparse_softmax(h.bw, scale, gXY.ptr, gXY.ptr, nb, s)
    torch.cuda.synchronize()
    gXY.check()
    assert_same_bits(gXY.numpy().reshape(nb, h.nnz), y, where + " in place")
    # backward, out of place
    gYin, gdY, gdX = _in("Y", y, VALUES, K), _in("dY", dY, VALUES, K), _out("dX", nb * h.nnz, VALUES, K)
    engine.sparse_softmax_backward(h.bw, scale, gYin.ptr, gdY.ptr, gdX.ptr, nb, s)
    torch.cuda.synchronize()
    check_all(gYin, gdY, gdX)
    dx = gdX.numpy().reshape(nb, h.nnz)
    for b in range(nb):
        assert_twin(dx[b], backward_twin(oracle, h.ro, y[b], dY[b], scale), f"{where} backward batch {b}")
    tY, td, tdx = _t(y), _t(dY), _nan(nb * h.nnz)
    engine.sparse_softmax_backward(h.bw, scale, tY.data_ptr(), td.data_ptr(), tdx.data_ptr(), nb, s)
    torch.cuda.synchronize()
    assert_same_bits(dx, tdx.cpu().numpy().reshape(nb, h.nnz), where + " backward")
    # backward, in place
    gD = Guarded.inplace("dY=dX", dY, VALUES, K, _dev())
    engine.sparse_softmax_backward(h.bw, scale, gYin.ptr, gD.ptr, gD.ptr, nb, s)
    torch.cuda.synchronize()
    check_all(gYin, gD)
    assert_same_bits(gD.numpy().reshape(nb, h.nnz), dx, where + " backward in place")


# ------------------------------------------------------------------------------------------------------------------
# 7. pointers below the documented alignment are refused before any device work
# ------------------------------------------------------------------------------------------------------------------
def test_misaligned_pointers_are_refused_before_any_device_work(engine, edges, handles):
    """base + 4 for an operand matrix or a 16-bit copy (16 bytes needed), base + 2 for a value array (4 bytes needed):
    BSMR_ERR_INVALID_ARG from every entry point, and no bit of any buffer changed.  (The check precedes every launch,
    which is what makes passing such a pointer safe; the guards own the bytes behind base + 4.)"""
    hip, bad = engine.hip(), engine.ERR_INVALID_ARG
    pat = edges["edge-hybrid"]
    K, mode, s = 64, 0, _stream()
    rng = np.random.default_rng(53)
    # every buffer is an "input" here: nothing may change, the outputs' present bits included
    gA, gB = _in("A", exact_ints(rng, pat.rows, K), OPERAND, K), _in("B", exact_ints(rng, pat.cols, K), OPERAND, K)
    gP = _in("P", _f32(rng, 3 * pat.nnz), VALUES, K)
    gA16 = Guarded.input("A16", rng.integers(0, 1 << 15, pat.rows * K), OPERAND, K, _dev(), dtype=np.uint16)
    gB16 = Guarded.input("B16", rng.integers(0, 1 << 15, pat.cols * K), OPERAND, K, _dev(), dtype=np.uint16)
    A, B, P, A16, B16 = gA.ptr, gB.ptr, gP.ptr, gA16.ptr, gB16.ptr
    plan = _build(engine, pat, "stream-pass")
    tuned = Plan(engine, pat, dict(fold_dense_below=0, promote_average=0, dense_engine=engine.ENGINE_TUNED))
    timing = engine.Timing()
    try:
        for a, b, p in ((A + 4, B, P), (A, B + 4, P), (A, B, P + 2), (A + 8, B, P), (A, B + 12, P), (A, B, P + 1)):
            assert hip.bsmr_sddmm(plan.plan, K, a, b, p, mode, s) == bad
            assert hip.bsmr_sddmm_batch(plan.plan, K, a, b, p, 3, mode, s) == bad
            assert hip.bsmr_sddmm_timed(plan.plan, K, a, b, p, mode, s, 0, 1, C.byref(timing)) == bad
            assert hip.bsmr_plan_tune(tuned.plan, K, a, b, p, mode, s, None) == bad
            assert hip.bsmr_sddmm_lowp(plan.plan, K, A16, B16, a, b, p, mode, s) == bad
        for a, b, a16, b16 in ((A + 4, B, A16, B16), (A, B + 4, A16, B16), (A, B, A16 + 4, B16), (A, B, A16, B16 + 4),
                               (A, B, A16 + 2, B16), (A, B, A16, B16 + 8)):
            assert hip.bsmr_convert_operands(plan.plan, K, a, b, a16, b16, mode, s) == bad
            if (a, b) == (A, B):
                assert hip.bsmr_sddmm_lowp(plan.plan, K, a16, b16, A, B, P, mode, s) == bad
                assert hip.bsmr_sddmm_lowp(plan.plan, K, a16, b16, None, None, P, mode, s) == bad
        assert hip.bsmr_batched_transpose(8, 8, 2, P + 2, P + 4096, s) == bad
        assert hip.bsmr_batched_transpose(8, 8, 2, P, P + 4098, s) == bad
        # the handle's calls: v / dP and the softmax arrays are value arrays, X / Y / A / B / dA / dB operand matrices
        h = handles("edge")
        assert (h.rows, h.cols) == (pat.rows, pat.cols) and h.nnz <= 3 * pat.nnz
        X, Y = B, A                                      # N x K and M x K
        for v, x, y in ((P + 2, X, Y), (P, X + 4, Y), (P, X, Y + 4)):
            assert hip.bsmr_spmm(h.bw, K, 0, v, x, y, 1, s) == bad
        for dp, a, b, da, db in ((P + 2, A, B, A, B), (P, A + 4, B, A, B), (P, A, B + 4, A, B), (P, A, B, A + 4, B),
                                 (P, A, B, A, B + 4)):
            assert hip.bsmr_sddmm_backward(h.bw, K, dp, a, b, da, db, 1, s) == bad
        Q = P + 4 * h.nnz
        for x, y in ((P + 2, Q), (P, Q + 2)):
            assert hip.bsmr_sparse_softmax(h.bw, 1.0, x, y, 1, s) == bad
        for y, dy, dx in ((P + 2, Q, Q), (P, Q + 2, Q), (P, Q, Q + 2)):
            assert hip.bsmr_sparse_softmax_backward(h.bw, 1.0, y, dy, dx, 1, s) == bad
        torch.cuda.synchronize()
        check_all(gA, gB, gP, gA16, gB16)
        # ... and the same pointers, aligned, are served
        assert hip.bsmr_sddmm(plan.plan, K, A, B, P, mode, s) == engine.OK
        torch.cuda.synchronize()
    finally:
        plan.close()
        tuned.close()
