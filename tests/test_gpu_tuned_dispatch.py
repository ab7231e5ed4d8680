"""The tuned-plan dispatch, choice by choice, on exact operands.

bench.py, smoke() and every production caller run SDDMM through a tunable plan (dense_engine = BSMR_ENGINE_TUNED): after
bsmr_plan_tune or bsmr_plan_set_tuned, prepareDense (csrc/bsmr_capi.hip) copies the Tuned record of (K, mode) into per-call
plan state on every call, and runPieces picks a dense road, a residue road, a conversion and one stream or two from it.  The
other modules build their plans with a fixed dense_engine, or let the timer pick; here every choice is installed by hand
(bsmr_plan_set_tuned, never a BSMR_* variable) on plans of

    plan_options(dense_engine=ENGINE_TUNED, fold_dense_below=0, promote_average=0)

  1. the choice matrix (MATRIX, one literal table: choice, K, patterns, expected status per pattern): an accepted choice is
     read back as installed, takes its road (dense_choice, conversion pass, residue precision), returns the exact result on
     exact operands and the bits of the fixed-engine plan on signed random operands; a refused one leaves the plan as it was;
  2. one plan, many (K, mode): no state carried from call to call;
  3. bsmr_sddmm_batch, bsmr_convert_operands + bsmr_sddmm_lowp, bsmr_sddmm_16 and bsmr_sddmm_timed on tuned plans;
  4. the fork and the join of overlap = 1 under load on the caller's stream;
  5. bsmr_plan_tune at small shapes: exact whatever it picks, and replayable.

No tolerance is introduced: every comparison is exact (test_gpu_numerics.assert_exact), bit for bit, or - for a 16-bit residue
that has no fixed-engine plan with the same kernel to be compared with - the bound of test_gpu_parity.check_case."""
import ctypes as C
import zlib

import numpy as np
import pytest

import synth
from test_gpu_numerics import (PATHS, Pattern, Plan, _rand_pattern, _through_copies, assert_exact, exact_ints, families,
                               model)
from test_gpu_parity import _dev, dense_flags, expected_twin, run_hip

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STREAM, TILES, SHARED, SWEEP, GEMM = 0, 1, 2, 4, 5               # BSMR_ENGINE_*
OK, INVALID_ARG, UNSUPPORTED_K, BAD_PLAN = 0, 1, 4, 6             # BSMR_OK, BSMR_ERR_*
BASE = dict(fold_dense_below=0, promote_average=0)
TUNABLE = dict(dense_engine=3, **BASE)


def choice(engine, group=0, blocks=0, fmt=-1, b_only=-1, overlap=-1, cvt=-1, waves=0):
    return dict(engine=engine, group=group, blocks_per_item=blocks, format=fmt, b_only=b_only, overlap=overlap,
                cvt_in_kernel=cvt, waves=waves)


# ------------------------------------------------------------------------------------------------------------------
# the choice matrix
# ------------------------------------------------------------------------------------------------------------------
# One row: a bsmr_tuned_choice, the K it is installed for, the status bsmr_plan_set_tuned must answer per pattern, the
# options of the fixed-engine plan an accepted call is compared with (a name of test_gpu_numerics.PATHS or the options
# test_gpu_gemm / test_gpu_sweep use), and what bsmr_plan_dense_choice must report (an int, a dict by K, or None: the
# engine's own rule - then only the fixed-engine plan's answer is asked for).  Rows with `pins` state a rule of refusal:
# they are refused on every pattern; every other row is accepted on at least one (asserted below, at collection).
DENSE = {"nips-dense": OK, "nips-hybrid": OK, "rand-hybrid": OK}
NIPS = {"nips-dense": OK, "nips-hybrid": OK}
HYBRID = {"nips-hybrid": OK, "rand-hybrid": OK}
NO_DENSE_PART = {"rand-sparse": BAD_PLAN}      # (an engine other than the streaming one needs dense entries)
SWEEP_GROUP = {(4, 0): {32: 16, 64: 16, 128: 16, 512: 8}, (8, 0): {32: 32, 128: 32, 512: 16},     # consumer waves x panels per
               (4, 2): {32: 8, 128: 8, 512: 8}, (8, 2): {32: 16, 64: 16, 128: 16, 512: 16}}        # wave (4, or 2 at K = 512)


def _row(name, ch, ks, on, fixed, group, pins=None):
    return dict(name=name, ch=ch, ks=ks, on=on, fixed=fixed, group=group, pins=pins)


def _sweep(waves, group, cvt):
    return dict(dense_engine=SWEEP, sweep_fp32=cvt, sweep_waves=waves, sweep_panels=group)


def _gemm(panels, blocks, cvt):
    return dict(dense_engine=GEMM, gemm_fp32=cvt, gemm_panels=panels, gemm_blocks=blocks)


MATRIX = [
    # the streaming engine
    _row("stream-f0-pass", choice(STREAM, fmt=0, cvt=0), (32, 64, 128, 256, 512), dict(DENSE, **{"bern-grouped": OK}),
         "stream-pass", 1),
    _row("stream-f0-in-kernel", choice(STREAM, fmt=0, cvt=1), (32, 64, 128), DENSE, "stream-cvt-in-kernel", 1),
    _row("stream-grouped", choice(STREAM, fmt=1, cvt=0), (128, 512), {"bern-grouped": OK, "rand-sparse": BAD_PLAN},
         "stream-pass-g4", 4),
    # tiles and shared-B
    _row("tiles-g0", choice(TILES, group=0, cvt=0), (32, 128, 512), dict(DENSE, **NO_DENSE_PART),
         dict(dense_engine=TILES, convert_in_kernel=0, tile_group=0), None),
    _row("tiles-g2", choice(TILES, group=2, cvt=0), (32, 128, 512), DENSE, "tiles", 2),
    _row("shared-g0", choice(SHARED, group=0, cvt=0), (32, 128, 512), DENSE,
         dict(dense_engine=SHARED, convert_in_kernel=0, tile_group=0), None),
    _row("shared-g8", choice(SHARED, group=8, cvt=0), (32, 128, 512), dict(DENSE, **NO_DENSE_PART), "shared", 8),
    # the sweep engine: consumer waves x panels per wave, 16-bit copies and fp32 operands
    _row("sweep-w4-g0", choice(SWEEP, group=0, cvt=0, waves=4), (32, 128, 512), dict(DENSE, **NO_DENSE_PART), _sweep(4, 0, 0),
         SWEEP_GROUP[4, 0]),
    _row("sweep-w4-g2", choice(SWEEP, group=2, cvt=0, waves=4), (32, 128, 512), DENSE, _sweep(4, 2, 0), SWEEP_GROUP[4, 2]),
    _row("sweep-w8-g0", choice(SWEEP, group=0, cvt=0, waves=8), (32, 128, 512), DENSE, _sweep(8, 0, 0), SWEEP_GROUP[8, 0]),
    _row("sweep-w8-g2", choice(SWEEP, group=2, cvt=0, waves=8), (32, 128, 512), DENSE, _sweep(8, 2, 0), SWEEP_GROUP[8, 2]),
    _row("sweep-w4-g0-in-kernel", choice(SWEEP, group=0, cvt=1, waves=4), (64, 128), DENSE, _sweep(4, 0, 1), SWEEP_GROUP[4, 0]),
    _row("sweep-w8-g2-in-kernel", choice(SWEEP, group=2, cvt=1, waves=8), (64, 128), DENSE, _sweep(8, 2, 1), SWEEP_GROUP[8, 2]),
    # the GEMM engine: the shapes of test_gpu_gemm.SHAPES and the model's own
    _row("gemm-16x16", choice(GEMM, 16, 16, cvt=0), (64, 128, 256, 512), dict(DENSE, **NO_DENSE_PART), "gemm-16bit-16x16", 16),
    _row("gemm-16x20", choice(GEMM, 16, 20, cvt=0), (64, 128, 256, 512), HYBRID, "gemm-16bit-16x20", 16),
    _row("gemm-16x12", choice(GEMM, 16, 12, cvt=0), (64, 128, 256, 512), NIPS, _gemm(16, 12, 0), 16),
    _row("gemm-8x16", choice(GEMM, 8, 16, cvt=0), (64, 128, 256, 512), NIPS, _gemm(8, 16, 0), 8),
    _row("gemm-8x20", choice(GEMM, 8, 20, cvt=0), (64, 128, 256, 512), HYBRID, "gemm-16bit-8x20", 8),
    _row("gemm-model", choice(GEMM, 0, 0, cvt=0), (64, 128, 256, 512), DENSE, _gemm(0, 0, 0), None),
    _row("gemm-16x16-in-kernel", choice(GEMM, 16, 16, cvt=1), (64, 128), DENSE, "gemm-fp32-16x16", 16),
    _row("gemm-8x20-in-kernel", choice(GEMM, 8, 20, cvt=1), (64, 128), HYBRID, "gemm-fp32-8x20", 8),
    _row("gemm-model-in-kernel", choice(GEMM, 0, 0, cvt=1), (64, 128), NIPS, _gemm(0, 0, 1), None),
    # hybrid plans: one stream or two
    _row("stream-one-stream", choice(STREAM, fmt=0, cvt=0, overlap=0), (128,), HYBRID,
         dict(convert_in_kernel=0, dense_group=1, overlap_streams=0), 1),
    _row("stream-two-streams", choice(STREAM, fmt=0, cvt=0, overlap=1), (128,), HYBRID,
         dict(convert_in_kernel=0, dense_group=1, overlap_streams=1), 1),
    _row("sweep-one-stream", choice(SWEEP, group=0, cvt=1, waves=4, overlap=0), (64,), HYBRID,
         dict(_sweep(4, 0, 1), overlap_streams=0), SWEEP_GROUP[4, 0]),
    _row("sweep-two-streams", choice(SWEEP, group=0, cvt=1, waves=4, overlap=1), (64,), HYBRID,
         dict(_sweep(4, 0, 1), overlap_streams=1), SWEEP_GROUP[4, 0]),
    _row("gemm-one-stream", choice(GEMM, 16, 16, cvt=0, overlap=0), (512,), HYBRID, dict(_gemm(16, 16, 0), overlap_streams=0), 16),
    _row("gemm-two-streams", choice(GEMM, 16, 16, cvt=0, overlap=1), (512,), HYBRID, dict(_gemm(16, 16, 0), overlap_streams=1), 16),
    # plans without a dense part: B converted alone, or the fp32 residue
    _row("residue-b-only", choice(STREAM, b_only=1), (64, 128, 512), {"rand-sparse": OK}, "residue-b-only", None),
    _row("residue-fp32", choice(STREAM, b_only=0), (64, 128, 512), {"rand-sparse": OK}, dict(b_only=0, sparse_lowp=0), None),
    # rules of refusal
    _row("tiles-in-kernel", choice(TILES, group=2, cvt=1), (32, 128), {"nips-dense": INVALID_ARG, "nips-hybrid": INVALID_ARG,
                                                                     "rand-sparse": INVALID_ARG}, None, None,
         pins="the tiles kernels read the 16-bit copies only"),
    _row("shared-in-kernel", choice(SHARED, group=8, cvt=1), (64,), {"nips-hybrid": INVALID_ARG}, None, None,
         pins="the shared-B kernels read the 16-bit copies only"),
    _row("no-such-engine", choice(3), (128,), {"nips-hybrid": INVALID_ARG}, None, None, pins="BSMR_ENGINE_TUNED is no engine"),
    _row("no-such-format", choice(STREAM, fmt=2), (128,), {"nips-dense": INVALID_ARG}, None, None, pins="format is -1, 0 or 1"),
    _row("k-48", choice(STREAM, fmt=0, cvt=0), (48,), {"nips-hybrid": UNSUPPORTED_K, "rand-sparse": UNSUPPORTED_K}, None, None,
         pins="K is a multiple of 32"),
    _row("tiles-k96", choice(TILES, cvt=0), (96,), {"nips-dense": BAD_PLAN}, None, None, pins="tiles serve K = 32 ... 512, powers of two"),
    _row("gemm-k32", choice(GEMM, 16, 16, cvt=0), (32, 96), {"nips-hybrid": BAD_PLAN}, None, None, pins="the GEMM engine serves K = 64 ... 512"),
    _row("gemm-no-such-shape", choice(GEMM, 4, 4, cvt=0), (128,), {"nips-dense": BAD_PLAN}, None, None, pins="no kernel of that macro-tile"),
    _row("gemm-16x12-in-kernel", choice(GEMM, 16, 12, cvt=1), (128,), {"nips-dense": BAD_PLAN}, None, None,
         pins="the fp32-operand GEMM kernels are built for four shapes"),
    _row("gemm-in-kernel-k256", choice(GEMM, 16, 16, cvt=1), (256,), {"nips-hybrid": BAD_PLAN}, None, None, pins="fp32 operands: K = 64, 128"),
    _row("sweep-in-kernel-k256", choice(SWEEP, cvt=1, waves=4), (256,), {"nips-hybrid": BAD_PLAN}, None, None, pins="fp32 operands: K <= 128"),
    _row("stream-in-kernel-k256", choice(STREAM, fmt=0, cvt=1), (256,), {"nips-dense": BAD_PLAN}, None, None, pins="fp32 operands: K = 32, 64, 128"),
]
ROWS = {r["name"]: r for r in MATRIX}

# (collection time) the matrix cannot hide a failure: names are unique, every choice row is accepted somewhere, every rule
# of refusal is refused everywhere, and an accepted row names the plan it is compared with
assert len(ROWS) == len(MATRIX)
for _r in MATRIX:
    _codes = set(_r["on"].values())
    assert _codes <= {OK, INVALID_ARG, UNSUPPORTED_K, BAD_PLAN} and _r["on"] and _r["ks"], _r["name"]
    if _r["pins"] is None:
        assert OK in _codes and _r["fixed"] is not None, f"{_r['name']}: refused on every pattern"
    else:
        assert OK not in _codes, f"{_r['name']}: a rule of refusal that is accepted"


def _fixed_options(row):
    opts = PATHS[row["fixed"]]["opts"] if isinstance(row["fixed"], str) else row["fixed"]
    return dict(BASE, **opts)


# ------------------------------------------------------------------------------------------------------------------
# patterns, operands, plans
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pats(engine):
    nips = synth.nips_like(rows=330, cols=1500, nnz=42000, seed=3)
    rand = _rand_pattern()
    bern = synth.bernoulli(rows=256, cols=512, density=0.1, seed=4)
    return {"nips-dense": Pattern(engine, "nips-dense", *nips, 0.0),
            "nips-hybrid": Pattern(engine, "nips-hybrid", *nips, 0.1),
            "rand-hybrid": Pattern(engine, "rand-hybrid", *rand, 0.1),
            "rand-sparse": Pattern(engine, "rand-sparse", *rand, 1.1),
            "bern-grouped": Pattern(engine, "bern-grouped", *bern, 0.0)}


class Operands:
    """exact families per (pattern, K) and their exact results, computed once for the module"""

    def __init__(self):
        self.fams, self.wants, self.normal = {}, {}, {}

    def families(self, pat, K):
        key = (pat.name, K)
        if key not in self.fams:
            rng = np.random.default_rng(zlib.crc32(f"{pat.name} {K}".encode()))
            self.fams[key] = list(families(rng, pat, K))
        return self.fams[key]

    def ints(self, pat, K):
        return self.families(pat, K)[0][1:]

    def want(self, oracle, pat, K, fam, A, B, mode, rounded):
        key = (pat.name, K, fam, mode, int(rounded.sum()))
        if key not in self.wants:
            self.wants[key] = model(oracle, pat, K, A, B, mode, rounded)
        return self.wants[key]

    def signed(self, pat, K, seed=0):
        key = (pat.name, K, seed)
        if key not in self.normal:
            rng = np.random.default_rng(zlib.crc32(f"{pat.name} {K} {seed}".encode()))
            self.normal[key] = (rng.standard_normal((pat.rows, K)).astype(np.float32),
                                rng.standard_normal((pat.cols, K)).astype(np.float32))
        return self.normal[key]


@pytest.fixture(scope="module")
def ops():
    return Operands()


def set_tuned(engine, plan, K, mode, ch):
    """status of bsmr_plan_set_tuned (engine.plan_set_tuned raises on a refusal)"""
    c = engine.TunedChoice()
    c.struct_size = C.sizeof(engine.TunedChoice)
    for n, v in ch.items():
        setattr(c, n, int(v))
    return engine.hip().bsmr_plan_set_tuned(plan.plan, K, mode, C.byref(c))


def get_tuned(engine, plan, K, mode):
    """the installed choice, None when (K, mode) was never tuned"""
    c = engine.TunedChoice()
    st = engine.hip().bsmr_plan_get_tuned(plan.plan, K, mode, C.byref(c))
    if st != OK:
        assert st == INVALID_ARG
        return None
    return {n: getattr(c, n) for n, _ in engine.TunedChoice._fields_ if n != "struct_size"}


def dense_choice(plan, K):
    """(panels per group, tiles, columns gathered) of the call prepared last"""
    g, t, u = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    assert plan.engine.hip().bsmr_plan_dense_choice(plan.plan, K, C.byref(g), C.byref(t), C.byref(u)) == OK
    return g.value, t.value, u.value


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def differing(a, b):
    return int((bits(a) != bits(b)).sum())


def parts(plan):
    st = plan.plan_stats()
    has_dense, has_sparse = st["num_dense_entries"] > 0, st["num_sparse_entries"] > 0
    assert st["folded_dense_entries"] == 0 and st["promoted_sparse_entries"] == 0
    assert has_dense == (plan.pat.delta < 1) and has_sparse == (plan.pat.delta > 0), plan.pat.name
    return has_dense, has_sparse


def implied(ch, has_dense, has_sparse):
    """(conversion pass, 16-bit residue) a choice implies: a pass with cvt_in_kernel = 0 and a dense part, or with
    b_only = 1; the residue reads the 16-bit copies whenever a pass ran (the plans here keep sparse_lowp = 1)"""
    converts = (ch["cvt_in_kernel"] == 0 and has_dense) or ch["b_only"] == 1
    return converts, converts and has_sparse


def check_residue(oracle, plan, K, A, B, mode, got, where):
    """a residue against what the project already uses: the fp32 kernel bit for bit against oracle.sparse_twin, the
    16-bit kernel inside check_case's bound against dense_lowp_model"""
    pat = plan.pat
    A, B = np.ascontiguousarray(A.ravel()), np.ascontiguousarray(B.ravel())
    twin, flags, lowp_model = expected_twin(oracle, plan, K, pat.ro, pat.ci, A, B, mode)
    s = ~flags
    if plan.sparse_choice(K, mode)["low_precision"]:
        absdot = oracle.sddmm_f64(pat.rows, K, pat.ro, pat.ci, np.abs(A), np.abs(B))
        err = np.abs(got[s].astype(np.float64) - lowp_model[s])
        assert (err <= (K / 16 + 8) * 2.0 ** -23 * absdot[s] + 1e-30).all(), (where, "16-bit residue", err.max())
    else:
        assert np.array_equal(bits(got[s]), bits(twin[s])), (where, "fp32 residue", differing(got[s], twin[s]))


def accepted(engine, oracle, ops, row, plan, fixed, K, mode):
    ch, pat = row["ch"], plan.pat
    where = f"{row['name']} {pat.name} K={K} mode={mode}"
    has_dense, has_sparse = parts(plan)
    assert set_tuned(engine, plan, K, mode, ch) == OK, where
    assert get_tuned(engine, plan, K, mode) == ch, where
    if ch["format"] == 1:
        assert plan.plan_stats()["grouped_group_size"] == 4, where
    converts, lowp = implied(ch, has_dense, has_sparse)
    # (b) exact operands, and (a) right after the first call
    tuned_dense = None
    for fam, A, B in ops.families(pat, K):
        got = plan.run(K, A, B, mode)
        if fam == "int":
            tuned_dense = dense_choice(plan, K)
            assert plan.converts(K, mode) == converts, (where, "conversion pass")
            assert plan.sparse_choice(K, mode)["low_precision"] == lowp, (where, "residue precision")
        assert_exact(got, ops.want(oracle, pat, K, fam, A, B, mode, plan.rounded(K, mode)), f"{where} {fam}")
    # (c) the bits of the fixed-engine plan
    rng = np.random.default_rng(zlib.crc32(where.encode()))
    A = rng.standard_normal((pat.rows, K)).astype(np.float32)
    B = rng.standard_normal((pat.cols, K)).astype(np.float32)
    got = plan.run(K, A, B, mode)
    assert dense_choice(plan, K) == tuned_dense, where
    mine = plan.sparse_choice(K, mode)
    ref = run_hip(engine, fixed, K, A.ravel(), B.ravel(), mode)
    fixed_dense, theirs = dense_choice(fixed, K), fixed.sparse_choice(K, mode)
    if has_dense:
        group = row["group"][K] if isinstance(row["group"], dict) else row["group"]
        assert group is None or tuned_dense[0] == group, (where, "dense_choice", tuned_dense, group)
        assert tuned_dense[0] == fixed_dense[0], (where, "dense_choice", tuned_dense, fixed_dense)
        if ch["engine"] != STREAM:      # (same engine, same shape, same dense entries: the same tiles and columns)
            assert tuned_dense == fixed_dense, (where, "dense_choice", tuned_dense, fixed_dense)
    flags = dense_flags(plan).astype(bool)
    assert np.array_equal(flags, dense_flags(fixed).astype(bool)), where
    assert not np.isnan(got).any() and not np.isnan(ref).any(), where
    assert np.array_equal(bits(got[flags]), bits(ref[flags])), (where, "dense entries", differing(got[flags], ref[flags]))
    if mine == theirs:
        assert np.array_equal(bits(got[~flags]), bits(ref[~flags])), (where, "residue", differing(got[~flags], ref[~flags]))
    if has_sparse and (mine != theirs or K == row["ks"][0]):
        check_residue(oracle, plan, K, A, B, mode, got, where + " tuned")
        if mine != theirs:
            check_residue(oracle, fixed, K, A, B, mode, ref, where + " fixed")


def refused(engine, ops, row, plan, K, mode, status):
    ch, pat = row["ch"], plan.pat
    where = f"{row['name']} {pat.name} K={K} mode={mode}"
    call_k = K if K % 32 == 0 else 64       # (a K no call takes: the plan is watched through a neighbour)
    A, B = ops.signed(pat, call_k)
    for base in (None, choice(STREAM, fmt=0, cvt=0)):       # never tuned, then tuned
        if base is not None:
            assert set_tuned(engine, plan, call_k, mode, base) == OK, where
        before = get_tuned(engine, plan, K, mode)
        assert before == (base if call_k == K else None), where
        index_bytes = plan.plan_stats()["device_index_bytes"]
        p0 = plan.run(call_k, A, B, mode)
        assert not np.isnan(p0).any(), where
        assert set_tuned(engine, plan, K, mode, ch) == status, where
        assert get_tuned(engine, plan, K, mode) == before, where
        assert plan.plan_stats()["device_index_bytes"] == index_bytes, where
        p1 = plan.run(call_k, A, B, mode)
        assert np.array_equal(bits(p0), bits(p1)), (where, "the call after the refusal", differing(p0, p1))


@pytest.mark.parametrize("name", list(ROWS))
def test_choice_matrix(engine, oracle, pats, ops, name):
    """One row of MATRIX on each of its patterns, every K, modes 0 and 1.  Accepted: (a) the choice is read back as
    installed and the call takes its road, (b) exact operands give the exact result, (c) signed random operands give the
    bits of the fixed-engine plan.  Refused: (d) the status is the table's, the plan is as before the attempt."""
    row, problems, ran = ROWS[name], [], 0
    for pname, status in row["on"].items():
        plan = Plan(engine, pats[pname], TUNABLE)
        fixed = Plan(engine, pats[pname], _fixed_options(row)) if status == OK else None
        try:
            for K in row["ks"]:
                for mode in (0, 1):
                    try:
                        if status == OK:
                            accepted(engine, oracle, ops, row, plan, fixed, K, mode)
                        else:
                            refused(engine, ops, row, plan, K, mode, status)
                        ran += 1
                    except AssertionError as e:         # (every case of the row is reported, not the first alone)
                        problems.append(f"{name} {pname} K={K} mode={mode}: {str(e)[:600]}")
        finally:
            plan.close()
            if fixed is not None:
                fixed.close()
    print(f"{name}: {ran} cases")
    assert not problems, f"{len(problems)} cases:\n" + "\n".join(problems)
    assert ran == 2 * len(row["ks"]) * len(row["on"])


def test_matrix_names_the_library_constants(engine):
    assert (STREAM, TILES, SHARED, SWEEP, GEMM) == (engine.ENGINE_STREAM, engine.ENGINE_TILES, engine.ENGINE_SHARED,
                                                    engine.ENGINE_SWEEP, engine.ENGINE_GEMM)
    assert (OK, INVALID_ARG, UNSUPPORTED_K, BAD_PLAN) == (engine.OK, engine.ERR_INVALID_ARG, engine.ERR_UNSUPPORTED_K,
                                                         engine.ERR_BAD_PLAN)
    assert TUNABLE["dense_engine"] == engine.ENGINE_TUNED


# ------------------------------------------------------------------------------------------------------------------
# 2. one plan, many (K, mode)
# ------------------------------------------------------------------------------------------------------------------
MANY = {
    "nips-hybrid": {
        (64, 0): choice(STREAM, fmt=0, cvt=1, overlap=0),
        (128, 0): choice(GEMM, 16, 16, cvt=0, overlap=1),
        (128, 1): choice(SWEEP, group=2, cvt=1, waves=8, overlap=0),
        (256, 0): choice(TILES, group=2, cvt=0, overlap=1),
        (512, 1): choice(SHARED, group=8, cvt=0, overlap=0),
        (512, 0): choice(STREAM, fmt=0, cvt=0, overlap=1),
        (32, 1): choice(SWEEP, group=0, cvt=0, waves=4, overlap=1),
        (64, 1): choice(GEMM, 8, 20, cvt=1, overlap=0),
    },
    "rand-sparse": {
        (64, 0): choice(STREAM, b_only=1),
        (128, 0): choice(STREAM, fmt=0, b_only=0),
        (128, 1): choice(STREAM, b_only=1, cvt=0),
        (256, 1): choice(STREAM, b_only=0, cvt=0),
        (512, 0): choice(STREAM, fmt=0, b_only=0, cvt=0),
        (512, 1): choice(STREAM, b_only=1),
    },
}
# A fixed shuffled order: the tuned pairs, mode 2 at the same K, an untuned K (96; 1024 makes the 16-bit workspace grow
# behind the K = 512 the installs reserved), an untuned mode of a tuned K ((256, 1) / (64, 1)); K goes up and down.
ORDER = {
    "nips-hybrid": [(32, 1), (512, 0), (64, 0), (128, 2), (128, 0), (96, 0), (512, 1), (64, 1), (256, 0), (256, 1), (32, 1),
                    (1024, 0), (128, 1), (64, 2), (512, 0), (128, 0), (96, 1), (256, 0), (64, 0), (512, 2), (512, 1), (128, 1),
                    (32, 0), (64, 1), (1024, 1), (256, 2), (128, 0), (64, 0), (512, 1), (32, 1)],
    "rand-sparse": [(64, 0), (512, 1), (128, 0), (128, 2), (96, 0), (512, 0), (64, 1), (128, 1), (256, 1), (1024, 0), (64, 0),
                    (256, 0), (512, 2), (128, 0), (512, 1), (96, 1), (128, 1), (64, 2), (512, 0), (256, 1), (64, 0), (1024, 1),
                    (128, 0), (512, 1), (256, 2), (128, 1)],
}
REINSTALL = {
    "nips-hybrid": {(128, 0): choice(SWEEP, group=0, cvt=0, waves=4, overlap=0),       # another engine
                    (256, 0): choice(TILES, group=4, cvt=0, overlap=1)},                # tiles: 2 -> 4 panels per group
    "rand-sparse": {(64, 0): choice(STREAM, b_only=0)},
}


class Fresh:
    """What a call of (K, mode) returns on a fresh plan that carries only that one choice (or none): result bits,
    dense_choice, sparse_choice.  Each plan is built once and kept for the module."""

    def __init__(self, engine, pats, ops):
        self.engine, self.pats, self.ops, self.plans, self.results = engine, pats, ops, {}, {}

    def expect(self, pname, K, mode, ch):
        key = (pname, K, mode, None if ch is None else tuple(sorted(ch.items())))
        if key not in self.results:
            pkey = key if ch is not None else (pname, "untuned")
            if pkey not in self.plans:
                self.plans[pkey] = Plan(self.engine, self.pats[pname], TUNABLE)
                if ch is not None:
                    assert set_tuned(self.engine, self.plans[pkey], K, mode, ch) == OK, key
            plan = self.plans[pkey]
            A, B = self.ops.signed(self.pats[pname], K)
            got = plan.run(K, A, B, mode)
            assert not np.isnan(got).any(), key
            self.results[key] = (got, dense_choice(plan, K), plan.sparse_choice(K, mode))
        return self.results[key]

    def close(self):
        for plan in self.plans.values():
            plan.close()


@pytest.fixture(scope="module")
def fresh(engine, pats, ops):
    f = Fresh(engine, pats, ops)
    yield f
    f.close()


def _covers(pname):
    chs = list(MANY[pname].values())
    got = {f: {c[f] for c in chs} for f in ("engine", "format", "cvt_in_kernel", "overlap", "b_only")}
    if pname == "nips-hybrid":
        return got["engine"] == {STREAM, TILES, SHARED, SWEEP, GEMM} and {0, 1} <= got["cvt_in_kernel"] and {0, 1} <= got["overlap"]
    return {0, 1} <= got["b_only"] and {-1, 0} <= got["format"] and {-1, 0} <= got["cvt_in_kernel"]


assert all(_covers(p) and len(MANY[p]) >= 6 and len(ORDER[p]) >= 24 for p in MANY)


@pytest.mark.parametrize("pname", list(MANY))
def test_one_plan_serves_many_k_and_modes_without_carrying_state(engine, pats, ops, fresh, pname):
    """Different choices for six and more (K, mode) pairs on ONE plan, then calls in a fixed shuffled order (tuned pairs,
    mode 2, untuned K, an untuned mode of a tuned K; K up and down, the workspace growing on the way): every call returns
    the bits, the dense_choice and the sparse_choice of a fresh plan that carries that one choice alone - no ...Now field
    left from the call before, no format of another K, no workspace of a smaller one.  Then two pairs are installed
    anew (another engine; tiles 2 -> 4 panels per group): they follow, the others stay."""
    pat, installed, problems = pats[pname], dict(MANY[pname]), []
    plan = Plan(engine, pat, TUNABLE)

    def call(step, K, mode):
        ch = installed.get((K, mode)) if mode != 2 else None
        A, B = ops.signed(pat, K)
        got = plan.run(K, A, B, mode)
        seen = (dense_choice(plan, K), plan.sparse_choice(K, mode))
        want, dense, sparse = fresh.expect(pname, K, mode, ch)
        if seen != (dense, sparse):
            problems.append(f"{step} K={K} mode={mode}: took {seen}, a fresh plan takes {(dense, sparse)}")
        if not np.array_equal(bits(got), bits(want)):
            problems.append(f"{step} K={K} mode={mode}: {differing(got, want)} of {got.size} entries differ from a fresh plan's")

    try:
        for (K, mode), ch in installed.items():
            assert set_tuned(engine, plan, K, mode, ch) == OK, (K, mode)
        for (K, mode), ch in installed.items():
            assert get_tuned(engine, plan, K, mode) == ch, (K, mode)
        for i, (K, mode) in enumerate(ORDER[pname]):
            call(f"call {i}", K, mode)
        for (K, mode), ch in REINSTALL[pname].items():
            assert installed[K, mode] != ch and set_tuned(engine, plan, K, mode, ch) == OK, (K, mode)
            installed[K, mode] = ch
        for (K, mode), ch in installed.items():
            assert get_tuned(engine, plan, K, mode) == ch, (K, mode)
        for K, mode in reversed(list(installed)):
            call("after the re-install", K, mode)
        for K, mode in installed:
            call("after the re-install, again", K, mode)
    finally:
        plan.close()
    assert not problems, f"{len(problems)}:\n" + "\n".join(problems)


# ------------------------------------------------------------------------------------------------------------------
# 3. the other entry points on a tuned plan
# ------------------------------------------------------------------------------------------------------------------
ENTRY_CHOICES = {
    "stream": choice(STREAM, fmt=0, cvt=0),
    "tiles": choice(TILES, group=2, cvt=0),
    "shared": choice(SHARED, group=8, cvt=0),
    "sweep": choice(SWEEP, group=0, cvt=0, waves=4),
    "gemm": choice(GEMM, 16, 16, cvt=0),
    "sweep-in-kernel": choice(SWEEP, group=0, cvt=1, waves=4),
    "gemm-in-kernel": choice(GEMM, 16, 16, cvt=1),
}


@pytest.mark.parametrize("name", list(ENTRY_CHOICES))
def test_batched_calls_on_a_tuned_plan(engine, oracle, pats, ops, name):
    """bsmr_sddmm_batch, two problems with different exact operands, on a tuned plan between single calls of a smaller and
    a larger K: the batch repeats prepareDense / needsWorkspace / the fork in its own words and converts both problems
    in one pass (a workspace of K x 2 behind a reserve of K).  Each batch is exact and the bits of its single call."""
    pat, K, ch = pats["nips-hybrid"], 128, ENTRY_CHOICES[name]
    plan = Plan(engine, pat, TUNABLE)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    try:
        A0, B0 = ops.ints(pat, K)
        A1, B1 = exact_ints(rng, pat.rows, K, -50, 90), exact_ints(rng, pat.cols, K, -90, 50)
        small, large = ops.ints(pat, 32), ops.ints(pat, 512)
        for mode in (0, 1):
            where = f"{name} mode={mode}"
            assert set_tuned(engine, plan, K, mode, ch) == OK, where
            converts, lowp = implied(ch, True, True)

            def batch():
                both = plan.run_batch(K, [(A0, B0), (A1, B1)], mode)
                assert dense_choice(plan, K)[0] == {"stream": 1, "tiles": 2, "shared": 8}.get(name, 16), where
                assert plan.sparse_choice(K, mode)["low_precision"] == lowp, where
                return both

            def single(k, a, b):
                got = plan.run(k, a, b, mode)
                assert_exact(got, ops.want(oracle, pat, k, "int", a, b, mode, plan.rounded(k, mode)), f"{where} single K={k}")

            single(32, *small)
            first = batch()
            single(512, *large)
            second = batch()
            single(32, *small)
            assert np.array_equal(bits(first), bits(second)), where
            rounded = plan.rounded(K, mode)
            for b, (a, bb) in enumerate(((A0, B0), (A1, B1))):
                one = plan.run(K, a, bb, mode)
                assert_exact(first[b], model(oracle, pat, K, a, bb, mode, rounded), f"{where} batch {b}")
                assert np.array_equal(bits(first[b]), bits(one)), (where, b, differing(first[b], one))
    finally:
        plan.close()


def _sddmm_16(engine, plan, K, problems, mode, stream=None):
    """bsmr_sddmm_16 on the library's own roundings of `problems` (bsmr_convert_operands, one problem at a time)"""
    dev, pat = _dev(), plan.pat
    s = torch.cuda.current_stream(dev).cuda_stream
    dt = torch.float16 if mode == 0 else torch.bfloat16
    a16 = torch.empty(len(problems) * pat.rows * K, dtype=dt, device=dev)
    b16 = torch.empty(len(problems) * pat.cols * K, dtype=dt, device=dev)
    for i, (a, b) in enumerate(problems):
        tA = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).ravel()).to(dev)
        tB = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32).ravel()).to(dev)
        engine.convert_operands(plan.plan, K, tA.data_ptr(), tB.data_ptr(), a16[i * pat.rows * K:].data_ptr(),
                                b16[i * pat.cols * K:].data_ptr(), mode, s)
    tP = torch.full((len(problems) * pat.nnz,), float("nan"), dtype=torch.float32, device=dev)
    engine.sddmm_16(plan.plan, K, a16.data_ptr(), b16.data_ptr(), tP.data_ptr(), len(problems), mode, s)
    torch.cuda.synchronize()
    return tP.cpu().numpy().reshape(len(problems), pat.nnz)


@pytest.mark.parametrize("name", ["gemm-in-kernel", "sweep-in-kernel", "gemm", "sweep", "stream"])
def test_16_bit_entry_points_on_a_tuned_plan(engine, oracle, pats, ops, name):
    """bsmr_convert_operands + bsmr_sddmm_lowp, and bsmr_sddmm_16 with one and two batches, on plans whose installed
    choice rounds in the kernel (GEMM, sweep) or behind a pass: the caller's 16-bit operands reach the engine's 16-bit
    kernel whatever road the plan's fp32 operands take.  Exact on exact operands; on signed random operands the dense
    entries are the bits of bsmr_sddmm under the choice with cvt_in_kernel = 0."""
    pat, K, ch = pats["nips-hybrid"], 128, ENTRY_CHOICES[name]
    plan, passing = Plan(engine, pat, TUNABLE), Plan(engine, pat, TUNABLE)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    try:
        A0, B0 = ops.ints(pat, K)
        A1, B1 = exact_ints(rng, pat.rows, K, -50, 90), exact_ints(rng, pat.cols, K, -90, 50)
        S0, S1 = ops.signed(pat, K), ops.signed(pat, K, seed=1)
        flags = dense_flags(plan).astype(bool)
        group = {"stream": 1}.get(name, 16)
        for mode in (0, 1):
            where = f"{name} mode={mode}"
            assert set_tuned(engine, plan, K, mode, ch) == OK, where
            assert set_tuned(engine, passing, K, mode, dict(ch, cvt_in_kernel=0)) == OK, where
            every = np.ones(pat.nnz, dtype=bool)       # (16-bit operands in: every entry is computed from rounded operands)
            want0, want1 = (model(oracle, pat, K, a, b, mode, every) for a, b in ((A0, B0), (A1, B1)))
            got, _, _ = _through_copies(engine, plan, K, A0, B0, mode)
            assert dense_choice(plan, K)[0] == group, where
            assert_exact(got, want0, where + " bsmr_sddmm_lowp")
            one = _sddmm_16(engine, plan, K, [(A0, B0)], mode)
            assert dense_choice(plan, K)[0] == group, where
            assert_exact(one[0], want0, where + " bsmr_sddmm_16")
            two = _sddmm_16(engine, plan, K, [(A1, B1), (A0, B0)], mode)
            assert_exact(two[0], want1, where + " bsmr_sddmm_16 batch 0 of 2")
            assert_exact(two[1], want0, where + " bsmr_sddmm_16 batch 1 of 2")
            # signed random operands: the dense entries of bsmr_sddmm behind the conversion pass
            refs = [passing.run(K, a, b, mode) for a, b in (S0, S1)]
            assert implied(dict(ch, cvt_in_kernel=0), True, True) == (passing.converts(K, mode), passing.sparse_choice(K, mode)["low_precision"])
            lowp, _, _ = _through_copies(engine, plan, K, *S0, mode)
            assert np.array_equal(bits(lowp[flags]), bits(refs[0][flags])), (where, "bsmr_sddmm_lowp", differing(lowp[flags], refs[0][flags]))
            # (both read the 16-bit copies with the 16-bit residue kernel: the residue agrees too)
            assert np.array_equal(bits(lowp), bits(refs[0])), (where, "bsmr_sddmm_lowp residue", differing(lowp, refs[0]))
            for problems, want in (([S0], refs[:1]), ([S0, S1], refs)):
                got16 = _sddmm_16(engine, plan, K, problems, mode)
                for b in range(len(problems)):
                    assert np.array_equal(bits(got16[b]), bits(want[b])), (where, "bsmr_sddmm_16", len(problems), b, differing(got16[b], want[b]))
    finally:
        plan.close()
        passing.close()


@pytest.mark.parametrize("pname,name", [("nips-hybrid", n) for n in ENTRY_CHOICES] + [("rand-sparse", "residue-b-only"), ("rand-sparse", "residue-fp32")])
def test_timed_calls_on_a_tuned_plan(engine, pats, ops, pname, name):
    """bsmr_sddmm_timed, one iteration: P afterwards is bsmr_sddmm's, bit for bit, and a convert time is reported exactly
    when the choice implies a conversion pass."""
    pat, K = pats[pname], 128
    ch = ENTRY_CHOICES[name] if name in ENTRY_CHOICES else ROWS[name]["ch"]
    plan = Plan(engine, pat, TUNABLE)
    dev = _dev()
    try:
        A, B = ops.signed(pat, K)
        tA, tB = torch.from_numpy(A.ravel()).to(dev), torch.from_numpy(B.ravel()).to(dev)
        for mode in (0, 1):
            assert set_tuned(engine, plan, K, mode, ch) == OK, (name, mode)
            want = plan.run(K, A, B, mode)
            tP = torch.full((pat.nnz,), float("nan"), dtype=torch.float32, device=dev)
            t = engine.sddmm_timed(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), mode,
                                   torch.cuda.current_stream(dev).cuda_stream, warmup=0, iters=1)
            torch.cuda.synchronize()
            got = tP.cpu().numpy()
            assert np.array_equal(bits(got), bits(want)), (name, mode, differing(got, want))
            assert (t["convert_ms"] > 0) == implied(ch, *parts(plan))[0], (name, mode, t)
            assert t["total_ms"] > 0
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. the fork and the join of overlap = 1
# ------------------------------------------------------------------------------------------------------------------
FILLS = 8          # fills of a 1 GiB buffer in front of the call: about 2.5 ms of work on the caller's stream
ROUNDS = 10


@pytest.mark.parametrize("name", ["stream", "gemm"])
def test_the_forked_residue_waits_for_the_callers_stream_and_is_waited_for(engine, pats, ops, name):
    """overlap = 1 on a non-default stream s, no host synchronisation in between: milliseconds of fills on s, the operands
    copied into place on s, P filled with NaN on s, the call on s, P copied out on s, ONE synchronisation.  The copy
    holds no NaN and is the overlap = 0 result bit for bit: the residue kernel on the side stream waited for the work
    queued on s before the call (it would otherwise read operands that are still zero and be overwritten by the NaN
    fill), and the copy waited for the residue.  The same through bsmr_sddmm_batch (two batches) and bsmr_sddmm_16."""
    pat, K, mode = pats["nips-hybrid"], 128, 0
    base = ENTRY_CHOICES[name]
    forked, serial = Plan(engine, pat, TUNABLE), Plan(engine, pat, TUNABLE)
    dev = _dev()
    problems = []
    try:
        assert set_tuned(engine, forked, K, mode, dict(base, overlap=1)) == OK
        assert set_tuned(engine, serial, K, mode, dict(base, overlap=0)) == OK
        flags = dense_flags(forked).astype(bool)
        S = [ops.signed(pat, K), ops.signed(pat, K, seed=1)]
        srcA = torch.from_numpy(np.concatenate([a.ravel() for a, _ in S])).to(dev)
        srcB = torch.from_numpy(np.concatenate([b.ravel() for _, b in S])).to(dev)
        big = torch.empty(1 << 28, dtype=torch.float32, device=dev)       # 1 GiB
        s = torch.cuda.Stream(dev)
        for case, nb in (("bsmr_sddmm", 1), ("bsmr_sddmm_batch", 2), ("bsmr_sddmm_16", 1)):
            nA, nB = nb * pat.rows * K, nb * pat.cols * K
            if case == "bsmr_sddmm_16":
                srcA_, srcB_ = srcA[:nA].to(torch.float16), srcB[:nB].to(torch.float16)
            else:
                srcA_, srcB_ = srcA[:nA], srcB[:nB]
            tA, tB = torch.zeros_like(srcA_), torch.zeros_like(srcB_)
            tP = torch.zeros(nb * pat.nnz, dtype=torch.float32, device=dev)
            out = torch.zeros_like(tP)

            def call(plan, stream):
                if case == "bsmr_sddmm":
                    engine.sddmm(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), mode, stream)
                elif case == "bsmr_sddmm_batch":
                    engine.sddmm_batch(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), nb, mode, stream)
                else:
                    engine.sddmm_16(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), nb, mode, stream)

            # the overlap = 0 result, and one quiet call of the forked plan (formats and workspace exist from here on)
            tA.copy_(srcA_)
            tB.copy_(srcB_)
            want = None
            for plan in (forked, serial):
                tP.fill_(float("nan"))
                call(plan, torch.cuda.current_stream(dev).cuda_stream)
                torch.cuda.synchronize()
                want = tP.cpu().numpy()
            assert not np.isnan(want).any(), case
            for r in range(ROUNDS):
                tA.zero_()
                tB.zero_()
                out.zero_()
                torch.cuda.synchronize()
                with torch.cuda.stream(s):
                    for _ in range(FILLS):
                        big.fill_(float(r))
                    tA.copy_(srcA_)
                    tB.copy_(srcB_)
                    tP.fill_(float("nan"))
                    call(forked, s.cuda_stream)
                    out.copy_(tP)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                nans, diff = int(np.isnan(got).sum()), differing(got, want)
                if nans or diff:
                    res = ~np.tile(flags, nb)
                    problems.append(f"{name} {case} round {r}: {nans} NaN, {diff} of {got.size} entries differ from the "
                                    f"overlap = 0 result ({differing(got[res], want[res])} of them in the residue)")
    finally:
        forked.close()
        serial.close()
        big = None
        torch.cuda.empty_cache()        # (the GiB goes back to the device, not into torch's cache)
    assert not problems, f"{len(problems)}:\n" + "\n".join(problems)


# ------------------------------------------------------------------------------------------------------------------
# 5. bsmr_plan_tune at small shapes, whatever it picks
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["nips-dense", "nips-hybrid", "rand-sparse"])
def test_the_tuner_leaves_exact_results_and_a_choice_that_replays(engine, oracle, pats, ops, pname):
    """bsmr_plan_tune on exact integer operands: P as the tuner leaves it and P of the tuned call are EXACT, whichever
    engine the timer preferred; bsmr_plan_get_tuned agrees with the report; the choice installed on a second plan gives
    the first plan's bits (also on signed random operands) and takes its road."""
    pat = pats[pname]
    dev = _dev()
    for K, mode in ((64, 0), (128, 0), (512, 1)):
        where = f"{pname} K={K} mode={mode}"
        first, second = Plan(engine, pat, TUNABLE), Plan(engine, pat, TUNABLE)
        try:
            A, B = ops.ints(pat, K)
            tA, tB = torch.from_numpy(A.ravel()).to(dev), torch.from_numpy(B.ravel()).to(dev)
            tP = torch.full((pat.nnz,), float("nan"), dtype=torch.float32, device=dev)
            assert get_tuned(engine, first, K, mode) is None
            report = engine.plan_tune(first.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), mode,
                                      torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize()
            left = tP.cpu().numpy()
            ch = get_tuned(engine, first, K, mode)
            print(where, report["chosen"], ch)
            assert ch is not None, where
            assert engine.ENGINE_NAMES[ch["engine"]] == report["chosen"], (where, report, ch)
            assert (ch["b_only"], ch["overlap"], ch["cvt_in_kernel"]) == (report["b_only"], report["overlap"], report["cvt_in_kernel"]), (where, report, ch)
            if report["sweep_fp32"] or report["gemm_fp32"]:
                assert ch["cvt_in_kernel"] == 1 and ch["engine"] == (SWEEP if report["sweep_fp32"] else GEMM), (where, report, ch)
            has_dense, has_sparse = parts(first)
            assert (ch["overlap"] in (0, 1)) == (has_dense and has_sparse) and (ch["b_only"] in (0, 1)) == (not has_dense), (where, ch)
            tuned = first.run(K, A, B, mode)
            road = (dense_choice(first, K), first.sparse_choice(K, mode), first.converts(K, mode))
            want = ops.want(oracle, pat, K, "int", A, B, mode, first.rounded(K, mode))
            assert_exact(left, want, where + " left by bsmr_plan_tune")
            assert_exact(tuned, want, where + " tuned call")
            assert set_tuned(engine, second, K, mode, ch) == OK, where
            assert get_tuned(engine, second, K, mode) == ch, where
            replay = second.run(K, A, B, mode)
            assert (dense_choice(second, K), second.sparse_choice(K, mode), second.converts(K, mode)) == road, where
            assert np.array_equal(bits(replay), bits(tuned)), (where, differing(replay, tuned))
            SA, SB = ops.signed(pat, K)
            a, b = first.run(K, SA, SB, mode), second.run(K, SA, SB, mode)
            assert np.array_equal(bits(a), bits(b)), (where, "signed operands", differing(a, b))
        finally:
            first.close()
            second.close()
