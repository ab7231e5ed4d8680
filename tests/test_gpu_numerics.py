"""Numerics of every operand-rounding site and dense engine, on operands the U[0, 2) tests never produce.

The other GPU tests feed make_data (positive, of order 1): strong on placement and on engine-vs-engine identity, blind
to sign, range, rounding ties, subnormals and non-finite values.  Here every assertion follows from IEEE arithmetic:

  1. exact signed operands (integers in [-127, 127], dyadic fractions, power-of-two scales): every product and partial
     sum is exact in fp32, so EVERY path and mode returns the exact dot product, whatever its summation order;
  2. a rounding-site probe: one operand a unit vector, the other an adversarial list (ties, fp16 overflow, fp16 and
     fp32 subnormals, bf16 near FLT_MAX, +-0, +-inf, NaN) - each entry is one rounded operand, compared exactly;
  3. signed random operands against the existing twins and error bounds;
  4. NaN / inf operands stay in the entries that read them;
  5. fp16 overflow through a whole call.

Expected values come from the oracle (oracle/sddmm_oracle.c): fp64 sums over operands rounded by oracle_round_fp16 /
oracle_round_bf16 (RNE, subnormals kept, overflow to inf) where the path rounds, over the fp32 operands where it does
not.  Values are compared with == (so -0 == +0) and NaN by class: hardware quiets NaN payloads.

Each case asserts the path it meant to take (dense_choice / sparse_choice / plan stats, and whether a call runs the
conversion pass, from bsmr_sddmm_timed's convert time)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import synth
from test_gpu_parity import _dev, dense_flags, expected_twin, run_hip

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = (32, 64, 128, 512, 1024)


# ------------------------------------------------------------------------------------------------------------------
# patterns and plans
# ------------------------------------------------------------------------------------------------------------------
class Pattern:
    def __init__(self, engine, name, rows, cols, ro, ci, delta):
        self.name, self.rows, self.cols, self.delta = name, rows, cols, delta
        self.ro = np.ascontiguousarray(ro, dtype=np.uint32)
        self.ci = np.ascontiguousarray(ci, dtype=np.uint32)
        self.nnz = int(self.ci.size)
        self.csr = engine.CSR.from_arrays(rows, cols, self.ro, self.ci)
        self.host = engine.Pipeline(self.csr, alpha=0.3, delta=delta, device=-1)
        self.arrays = self.host.arrays()
        self.row_of = np.repeat(np.arange(rows), np.diff(self.ro.astype(np.int64)))


def _rand_pattern():
    """150 x 220: 9 empty rows, a ragged last column block (220 = 13 * 16 + 12), and column 5 read by no entry."""
    rows, cols, ro, ci = synth.random_pattern(150, 220, 5000, seed=11, empty_rows=9)
    r = np.repeat(np.arange(rows), np.diff(ro.astype(np.int64)))
    keep = ci != 5
    ro = np.concatenate([[0], np.cumsum(np.bincount(r[keep], minlength=rows))]).astype(np.uint32)
    return rows, cols, ro, ci[keep]


@pytest.fixture(scope="module")
def patterns(engine):
    nips = synth.nips_like(rows=330, cols=1500, nnz=42000, seed=3)        # 330 rows: 20.6 panels, 1500 = 93 * 16 + 12
    rand = _rand_pattern()
    return {"nips-dense": Pattern(engine, "nips-dense", *nips, 0.0),
            "nips-hybrid": Pattern(engine, "nips-hybrid", *nips, 0.1),
            "rand-hybrid": Pattern(engine, "rand-hybrid", *rand, 0.1),
            "rand-sparse": Pattern(engine, "rand-sparse", *rand, 1.1),
            "nips-sparse": Pattern(engine, "nips-sparse", *nips, 1.1)}


class Plan:
    """A plan built by bsmr_plan_create_ex from a pattern's RPHM arrays and explicit options.  Quacks like a
    Pipeline where the helpers of test_gpu_parity need it (run_hip, dense_flags, expected_twin)."""

    def __init__(self, engine, pat, opts):
        self.engine, self.pat, self.csr, self.delta = engine, pat, pat.csr, pat.delta
        st, self.plan = engine.plan_from_arrays(pat.rows, pat.cols, pat.nnz, pat.arrays, device=0,
                                                options=engine.plan_options(**opts))
        assert st == engine.OK, (pat.name, opts, st)

    def close(self):
        self.engine.plan_destroy(self.plan)

    def array(self, name):
        return self.pat.host.array(name)

    def plan_stats(self):
        s = self.engine.PlanStats()
        assert self.engine.hip().bsmr_plan_get_stats(self.plan, C.byref(s)) == self.engine.OK
        return {k: getattr(s, k) for k, _ in self.engine.PlanStats._fields_}

    def dense_flags(self):
        flags = np.zeros(self.pat.nnz, dtype=np.uint8)
        assert self.engine.hip().bsmr_plan_dense_flags(self.plan, flags.ctypes.data_as(C.c_void_p)) == self.engine.OK
        return flags

    def sparse_choice(self, K, mode):
        lanes, lowp = C.c_uint32(0), C.c_uint32(0)
        assert self.engine.hip().bsmr_plan_sparse_choice(self.plan, K, mode, C.byref(lanes), C.byref(lowp)) == self.engine.OK
        return {"lanes_per_entry": lanes.value, "low_precision": bool(lowp.value)}

    def dense_group(self, K):
        """panels per group / macro-tile of the call prepared last (bsmr_plan_dense_choice, as test_gpu_gemm._run)"""
        g, t, u = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        assert self.engine.hip().bsmr_plan_dense_choice(self.plan, K, C.byref(g), C.byref(t), C.byref(u)) == self.engine.OK
        return g.value

    def converts(self, K, mode):
        """True when a call of (K, mode) starts with a conversion pass (full or B alone): bsmr_sddmm_timed reports a
        convert time exactly then.  One timed iteration; the operands are zeros, the output scratch."""
        dev = _dev()
        tA = torch.zeros(self.pat.rows * K, dtype=torch.float32, device=dev)
        tB = torch.zeros(self.pat.cols * K, dtype=torch.float32, device=dev)
        tP = torch.zeros(max(self.pat.nnz, 1), dtype=torch.float32, device=dev)
        t = self.engine.sddmm_timed(self.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), mode,
                                    torch.cuda.current_stream(dev).cuda_stream, warmup=0, iters=1)
        return t["convert_ms"] > 0

    def run(self, K, A, B, mode):
        return run_hip(self.engine, self, K, A.ravel(), B.ravel(), mode)

    def run_batch(self, K, problems, mode):
        dev = _dev()
        tA = torch.from_numpy(np.concatenate([a.ravel() for a, _ in problems])).to(dev)
        tB = torch.from_numpy(np.concatenate([b.ravel() for _, b in problems])).to(dev)
        tP = torch.full((len(problems) * self.pat.nnz,), float("nan"), dtype=torch.float32, device=dev)
        self.engine.sddmm_batch(self.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), len(problems), mode,
                                torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        return tP.cpu().numpy().reshape(len(problems), self.pat.nnz)

    def rounded(self, K, mode):
        """per entry: True where the call computes from 16-bit operands (every dense entry in modes 0 / 1, the residue
        when its low-precision kernel runs)"""
        if mode == 2:
            return np.zeros(self.pat.nnz, dtype=bool)
        flags = dense_flags(self).astype(bool)
        return flags | self.sparse_choice(K, mode)["low_precision"]


# The path matrix.  opts: plan options on top of fold_dense_below=0; ks: the K each path serves; pats: the patterns
# it runs on; group: what bsmr_plan_dense_choice must report (None: not checked); converts: whether a mode-0/1 call
# runs the conversion pass; lowp: whether the residue of a hybrid plan reads the converted copies.
PATHS = {
    "stream-pass": dict(opts=dict(convert_in_kernel=0, dense_group=1), ks=KS, group=1, converts=True, lowp=True),
    "stream-pass-g4": dict(opts=dict(convert_in_kernel=0, dense_group=4), ks=(32, 128, 512), group=4, converts=True, lowp=True),
    "stream-fp32-residue": dict(opts=dict(convert_in_kernel=0, dense_group=1, sparse_lowp=0), ks=(64, 512), group=1,
                                converts=True, lowp=False, pats=("nips-hybrid", "rand-hybrid")),
    "stream-cvt-in-kernel": dict(opts=dict(convert_in_kernel=1, dense_group=1), ks=(32, 64, 128), group=1, converts=False, lowp=False),
    "tiles": dict(opts=dict(dense_engine=1, convert_in_kernel=0, tile_group=2), ks=(32, 64, 128, 512), group=2, converts=True, lowp=True),
    "shared": dict(opts=dict(dense_engine=2, convert_in_kernel=0, tile_group=8), ks=(32, 64, 128, 512), group=8, converts=True, lowp=True),
    "sweep-16bit": dict(opts=dict(dense_engine=4, sweep_fp32=0), ks=(32, 64, 128, 512), group="sweep", converts=True, lowp=True),
    "sweep-fp32": dict(opts=dict(dense_engine=4, sweep_fp32=1), ks=(32, 64, 128), group="sweep", converts=False, lowp=False),
    "gemm-16bit-16x16": dict(opts=dict(dense_engine=5, gemm_fp32=0, gemm_panels=16, gemm_blocks=16), ks=(64, 128, 256, 512),
                             group=16, converts=True, lowp=True),
    "gemm-16bit-16x20": dict(opts=dict(dense_engine=5, gemm_fp32=0, gemm_panels=16, gemm_blocks=20), ks=(64, 128, 256, 512),
                             group=16, converts=True, lowp=True),
    "gemm-16bit-8x20": dict(opts=dict(dense_engine=5, gemm_fp32=0, gemm_panels=8, gemm_blocks=20), ks=(64, 128, 256, 512),
                            group=8, converts=True, lowp=True),
    "gemm-fp32-16x16": dict(opts=dict(dense_engine=5, gemm_fp32=1, gemm_panels=16, gemm_blocks=16), ks=(64, 128), group=16,
                            converts=False, lowp=False),
    "gemm-fp32-8x20": dict(opts=dict(dense_engine=5, gemm_fp32=1, gemm_panels=8, gemm_blocks=20), ks=(64, 128), group=8,
                           converts=False, lowp=False),
    # all-sparse plans: B alone converted, the residue kernel rounds A while it stages it (test_all_sparse_plans_convert_b_alone)
    "residue-b-only": dict(opts=dict(b_only=1, b_only_work_m=1), ks=(64, 128, 512, 1024), group=None, converts=True,
                           lowp=True, pats=("nips-sparse", "rand-sparse")),
}
DENSE_PATS = ("nips-dense", "nips-hybrid", "rand-hybrid")
BATCHED = ("stream-pass", "stream-cvt-in-kernel", "gemm-16bit-16x16", "gemm-fp32-16x16", "residue-b-only")


def _pats(name):
    return PATHS[name].get("pats", DENSE_PATS)


def _build(engine, pat, name):
    # (no promotion: the residue of a hybrid RPHM stays a residue)
    return Plan(engine, pat, dict(fold_dense_below=0, promote_average=0, **PATHS[name]["opts"]))


def assert_path(plan, name, K, mode):
    """the case ran the path it is named after (call after a call of (K, mode) on the plan)"""
    p = PATHS[name]
    st = plan.plan_stats()
    where = f"{name} {plan.pat.name} K={K} mode={mode}"
    if name == "residue-b-only":
        assert st["num_dense_entries"] == 0 and st["num_sparse_entries"] == plan.pat.nnz, where
    else:
        assert st["num_dense_entries"] > 0 and st["folded_dense_entries"] == 0, where
        assert (st["num_sparse_entries"] > 0) == (plan.pat.delta > 0), where
    if mode == 2:       # (every engine's mode-2 call runs the exact-fp32 dense kernel and the fp32 residue)
        assert not plan.sparse_choice(K, mode)["low_precision"], where
        return
    if name != "residue-b-only":
        g = plan.dense_group(K)
        if p["group"] == "sweep":
            assert g >= 4 and g % 4 == 0, (where, g)       # consumer waves x panels per wave
        else:
            assert g == p["group"], (where, g)
    converts = plan.converts(K, mode)
    if name.startswith("stream-pass") and st["num_sparse_entries"] == 0 and K <= 64:
        # (untuned, an all-dense plan with a small gather rounds in the streaming kernel at K <= 64 whatever
        # convert_in_kernel says: bsmr_capi.hip cvtInKernel - the in-kernel row covers that kernel)
        pass
    else:
        assert converts == p["converts"], (where, "conversion pass")
    if st["num_sparse_entries"]:
        assert plan.sparse_choice(K, mode)["low_precision"] == p["lowp"], (where, "residue kernel")
        if p["lowp"]:
            assert st["sparse_lowp"], where


# ------------------------------------------------------------------------------------------------------------------
# expectations
# ------------------------------------------------------------------------------------------------------------------
def model(oracle, pat, K, A, B, mode, rounded):
    """fp64 dot products; over the operands rounded to fp16 (mode 0) / bf16 (mode 1) where `rounded`, else over the
    fp32 operands.  Class-aware: inf * 0 = NaN, inf - inf = NaN, as IEEE."""
    A = np.ascontiguousarray(A, dtype=np.float32).ravel()
    B = np.ascontiguousarray(B, dtype=np.float32).ravel()
    raw = oracle.sddmm_f64(pat.rows, K, pat.ro, pat.ci, A, B)
    if mode == 2 or not rounded.any():
        return raw
    low = oracle.dense_lowp_model(2 if mode == 0 else 3, pat.rows, K, pat.ro, pat.ci, A, B)
    return np.where(rounded, low, raw)


def assert_exact(got, want64, where):
    """got equals the exact result: NaN where the model is NaN, == elsewhere (-0 == +0, inf == inf)"""
    want = want64.astype(np.float32)
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | (~nan & (got != want))
    if bad.any():
        i = np.flatnonzero(bad)
        raise AssertionError(f"{where}: {i.size} entries differ from the exact result; first {i[:5].tolist()}: "
                             f"got {got[i[:5]].tolist()} want {want[i[:5]].tolist()}")


def exact_ints(rng, rows, K, lo=-127, hi=127):
    return rng.integers(lo, hi + 1, size=(rows, K)).astype(np.float32)


def families(rng, pat, K):
    """three operand families whose products and partial sums are exact in fp32 (and inside the fp16 normal range)"""
    A, B = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
    yield "int", A, B
    if K in (64, 512):
        yield "dyadic", exact_ints(rng, pat.rows, K) * np.float32(2.0 ** -7), exact_ints(rng, pat.cols, K) * np.float32(2.0 ** -7)
        ra = np.ldexp(np.float32(1), rng.integers(-8, 9, size=(pat.rows, 1))).astype(np.float32)
        cb = np.ldexp(np.float32(1), rng.integers(-8, 9, size=(pat.cols, 1))).astype(np.float32)
        yield "pow2-scaled", A * ra, B * cb


# ------------------------------------------------------------------------------------------------------------------
# 1. exact signed operands
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PATHS))
def test_exact_signed_operands(engine, oracle, patterns, name):
    """Every path, every mode: P equals the exact dot product of signed integer / dyadic / power-of-two-scaled operands."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    for pname in _pats(name):
        pat = patterns[pname]
        plan = _build(engine, pat, name)
        try:
            for K in PATHS[name]["ks"]:
                for fam, A, B in families(rng, pat, K):
                    for mode in (0, 1, 2):
                        got = plan.run(K, A, B, mode)
                        if fam == "int":
                            assert_path(plan, name, K, mode)
                        assert_exact(got, model(oracle, pat, K, A, B, mode, plan.rounded(K, mode)),
                                     f"{name} {pname} K={K} {fam} mode={mode}")
                if name in BATCHED and K in (64, 128, 512):
                    # bsmr_sddmm_batch: problem 1 carries other operands
                    A0, B0 = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
                    A1, B1 = exact_ints(rng, pat.rows, K, -50, 90), exact_ints(rng, pat.cols, K, -90, 50)
                    for mode in (0, 1):
                        both = plan.run_batch(K, [(A0, B0), (A1, B1)], mode)
                        for b, (a, bb) in enumerate(((A0, B0), (A1, B1))):
                            assert_exact(both[b], model(oracle, pat, K, a, bb, mode, plan.rounded(K, mode)),
                                         f"{name} {pname} K={K} batch {b} mode={mode}")
        finally:
            plan.close()


def test_exact_signed_operands_through_converted_copies(engine, oracle, patterns):
    """bsmr_convert_operands + bsmr_sddmm_lowp on a hybrid plan: the caller's own 16-bit operands, exact results."""
    pat = patterns["nips-hybrid"]
    plan = _build(engine, pat, "stream-pass")
    rng = np.random.default_rng(17)
    try:
        for K in (64, 512):
            A, B = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
            for mode in (0, 1):
                got, _, _ = _through_copies(engine, plan, K, A, B, mode)
                assert plan.sparse_choice(K, mode)["low_precision"]
                assert_exact(got, model(oracle, pat, K, A, B, mode, plan.rounded(K, mode)), f"lowp entry K={K} mode={mode}")
    finally:
        plan.close()


def _through_copies(engine, plan, K, A, B, mode):
    dev = _dev()
    s = torch.cuda.current_stream(dev).cuda_stream
    tA = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32).ravel()).to(dev)
    tB = torch.from_numpy(np.ascontiguousarray(B, dtype=np.float32).ravel()).to(dev)
    dt = torch.float16 if mode == 0 else torch.bfloat16
    a16 = torch.empty(tA.numel(), dtype=dt, device=dev)
    b16 = torch.empty(tB.numel(), dtype=dt, device=dev)
    tP = torch.full((plan.pat.nnz,), float("nan"), dtype=torch.float32, device=dev)
    engine.convert_operands(plan.plan, K, tA.data_ptr(), tB.data_ptr(), a16.data_ptr(), b16.data_ptr(), mode, s)
    engine.sddmm_lowp(plan.plan, K, a16.data_ptr(), b16.data_ptr(), tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), mode, s)
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)
    return tP.cpu().numpy(), bits(a16), bits(b16)


# ------------------------------------------------------------------------------------------------------------------
# 2. rounding-site probe
# ------------------------------------------------------------------------------------------------------------------
def _f(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def _probe_values():
    """(values finite after rounding in every mode, values that overflow in some mode, non-finite values); both signs"""
    one = np.float32(1)
    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    dn = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))
    finite = []
    for tie in (1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1000.25, 1000.75, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 301.0, 303.0):
        finite += [np.float32(tie), up(tie), dn(tie)]                       # fp16 / bf16 ties (even and odd kept bit) +- 1 ulp
    finite += [np.float32(65504), dn(65520), np.float32(2.0 ** -24), np.float32(2.0 ** -25), np.float32(3 * 2.0 ** -26),
               np.float32(2.0 ** -14 - 2.0 ** -25), np.float32(2.0 ** -14), np.float32(2.0 ** -20 + 2.0 ** -25), up(2.0 ** -25),
               np.float32(5 * 2.0 ** -26),                                   # fp16 subnormals and the values rounding into / out of them
               _f(0x00400000), _f(0x00000001), _f(0x00008001), _f(0x00018000), # fp32 subnormals (bf16 keeps or rounds them)
               one, np.float32(0.0)]
    overflow = [np.float32(65520), np.float32(65535), _f(0x7F7F0000), _f(0x7F7F7FFF), _f(0x7F7F8000), _f(0x7F7FFFFF)]
    nonfinite = [np.float32(np.inf), np.float32(np.nan)]
    sign = lambda vs: np.array([v for x in vs for v in (x, -x)], dtype=np.float32)
    return sign(finite), sign(overflow), sign(nonfinite)


def _probe_operands(rows, K, seed):
    """rows x K adversarial matrix: every row holds the finite list in its own rotation; every third row carries one
    value that is non-finite after rounding in some mode (each such value in a row of its own), at a position that
    varies by row.  Returns the matrix."""
    finite, overflow, nonfinite = _probe_values()
    assert finite.size <= K
    rng = np.random.default_rng(seed)
    M = np.zeros((rows, K), dtype=np.float32)
    special = np.concatenate([overflow, nonfinite])
    for i in range(rows):
        row = np.resize(finite, K)
        M[i] = np.roll(row, rng.integers(K))
        if i % 3 == 1:
            M[i, rng.integers(K)] = special[(i // 3) % special.size]
    return M


def _unit(n, K):
    U = np.zeros((n, K), dtype=np.float32)
    U[np.arange(n), np.arange(n) % K] = 1.0
    return U


PROBE_PATHS = ("stream-pass", "stream-fp32-residue", "stream-cvt-in-kernel", "tiles", "shared", "sweep-16bit", "sweep-fp32",
               "gemm-16bit-16x16", "gemm-16bit-8x20", "gemm-fp32-16x16", "residue-b-only")


@pytest.mark.parametrize("name", PROBE_PATHS)
def test_rounding_site_probe(engine, oracle, patterns, name):
    """B unit columns, A adversarial (then the roles swapped): every entry is one rounded operand, compared exactly with
    oracle_round_fp16 / bf16 (modes 0, 1) or the operand itself (mode 2); non-finite operands spread NaN through
    inf * 0 exactly as the model predicts."""
    K = 128                 # (the finite list holds 68 values)
    for pname in _pats(name)[1:] if name != "residue-b-only" else _pats(name):
        pat = patterns[pname]
        plan = _build(engine, pat, name)
        try:
            for side in ("A", "B"):
                if side == "A":
                    A, B = _probe_operands(pat.rows, K, 1), _unit(pat.cols, K)
                else:
                    A, B = _unit(pat.rows, K), _probe_operands(pat.cols, K, 2)
                for mode in (0, 1, 2):
                    got = plan.run(K, A, B, mode)
                    assert_path(plan, name, K, mode)
                    rounded = plan.rounded(K, mode)
                    want = model(oracle, pat, K, A, B, mode, rounded)
                    # the placement rule: entries whose operand row / column holds no overflowing value are single
                    # rounded operands - the model must agree with the per-element rounding itself
                    adv = A if side == "A" else B
                    idx = pat.row_of if side == "A" else pat.ci
                    k = (pat.ci if side == "A" else pat.row_of) % K
                    op = adv[idx, k]
                    direct = op if mode == 2 else np.where(rounded, oracle.round_array(2 if mode == 0 else 3, op), op)
                    clean = np.isfinite(want)
                    assert clean.sum() > pat.nnz // 2 and np.array_equal(want[clean].astype(np.float32), direct[clean])
                    assert_exact(got, want, f"{name} {pname} probe {side} mode={mode}")
        finally:
            plan.close()


def test_convert_operands_rounds_like_ieee(engine, patterns):
    """bsmr_convert_operands: fp16 bits = np.float16 (RNE, subnormals, overflow to inf); bf16 bits = RNE on the fp32
    bits; NaN stays NaN (payloads not compared)."""
    pat = patterns["nips-hybrid"]
    plan = _build(engine, pat, "stream-pass")
    try:
        K = 128
        A, B = _probe_operands(pat.rows, K, 3), _probe_operands(pat.cols, K, 4)
        for mode in (0, 1):
            _, a16, b16 = _through_copies(engine, plan, K, A, B, mode)
            for x, got in ((A.ravel(), a16), (B.ravel(), b16)):
                nan = np.isnan(x)
                if mode == 0:
                    with np.errstate(over="ignore"):                 # (65520 and up: inf, as wanted)
                        want = x.astype(np.float16).view(np.uint16)
                    got_nan = (got & 0x7C00) == 0x7C00
                    got_nan &= (got & 0x03FF) != 0
                else:
                    u = x.view(np.uint32).astype(np.uint64)
                    want = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)
                    got_nan = ((got & 0x7F80) == 0x7F80) & ((got & 0x007F) != 0)
                assert np.array_equal(got_nan, nan), f"mode {mode}: NaN class"
                bad = np.flatnonzero(got[~nan] != want[~nan])
                assert bad.size == 0, f"mode {mode}: {bad.size} values, first inputs {x[~nan][bad[:5]].tolist()}"
    finally:
        plan.close()


def test_rounding_probe_through_converted_copies(engine, oracle, patterns):
    """bsmr_convert_operands + bsmr_sddmm_lowp: the probe on the caller's 16-bit copies, dense part and residue"""
    pat = patterns["nips-hybrid"]
    plan = _build(engine, pat, "stream-pass")
    try:
        K = 128
        for A, B in ((_probe_operands(pat.rows, K, 5), _unit(pat.cols, K)), (_unit(pat.rows, K), _probe_operands(pat.cols, K, 6))):
            for mode in (0, 1):
                got, _, _ = _through_copies(engine, plan, K, A, B, mode)
                assert_exact(got, model(oracle, pat, K, A, B, mode, plan.rounded(K, mode)), f"lowp entry probe mode={mode}")
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. signed random operands against the existing models
# ------------------------------------------------------------------------------------------------------------------
SIGNED_PATHS = ("stream-pass", "stream-fp32-residue", "stream-cvt-in-kernel", "tiles", "shared", "sweep-16bit", "sweep-fp32",
                "gemm-16bit-16x20", "gemm-fp32-8x20", "residue-b-only")


@pytest.mark.parametrize("name", SIGNED_PATHS)
def test_signed_random_operands(engine, oracle, patterns, name):
    """U[-1, 1) operands, with and without per-row scales 2^[-12, 12]: mode 2 bit-identical to the fp32 twins, modes
    0 / 1 within the dense and low-precision-residue error bounds of the rounded-operand model."""
    pname = "rand-sparse" if name == "residue-b-only" else "nips-hybrid"
    pat = patterns[pname]
    plan = _build(engine, pat, name)
    K = 128 if 128 in PATHS[name]["ks"] else 64
    try:
        for scaled in (False, True):
            A = engine.make_data(pat.rows * K, 5489).reshape(pat.rows, K) - np.float32(1)
            B = engine.make_data(pat.cols * K, 5490).reshape(pat.cols, K) - np.float32(1)
            if scaled:
                rng = np.random.default_rng(8)
                A = A * np.ldexp(np.float32(1), rng.integers(-12, 13, size=(pat.rows, 1))).astype(np.float32)
                B = B * np.ldexp(np.float32(1), rng.integers(-12, 13, size=(pat.cols, 1))).astype(np.float32)
            A, B = np.ascontiguousarray(A.ravel()), np.ascontiguousarray(B.ravel())
            absdot = oracle.sddmm_f64(pat.rows, K, pat.ro, pat.ci, np.abs(A), np.abs(B))
            for mode in (0, 1, 2):
                got = plan.run(K, A, B, mode)
                assert_path(plan, name, K, mode)
                where = f"{name} K={K} scaled={scaled} mode={mode}"
                twin, flags, lowp_model = expected_twin(oracle, plan, K, pat.ro, pat.ci, A, B, mode)
                s = ~flags
                if mode == 2:
                    assert np.array_equal(got.view(np.uint32), twin.view(np.uint32)), where
                    continue
                if plan.sparse_choice(K, mode)["low_precision"]:
                    err = np.abs(got[s].astype(np.float64) - lowp_model[s])
                    assert (err <= (K / 16 + 8) * 2.0 ** -23 * absdot[s]).all(), (where, "lowp residue", err.max())
                else:
                    assert np.array_equal(got[s].view(np.uint32), twin[s].view(np.uint32)), (where, "fp32 residue")
                err = np.abs(got[flags].astype(np.float64) - lowp_model[flags])
                assert (err <= (K / 32 + 4) * 2.0 ** -23 * absdot[flags]).all(), (where, "dense", err.max() if err.size else 0)
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. non-finite operands stay where they are read
# ------------------------------------------------------------------------------------------------------------------
NONFINITE_PATHS = ("stream-pass", "stream-fp32-residue", "stream-cvt-in-kernel", "tiles", "shared", "sweep-16bit", "sweep-fp32",
                   "gemm-16bit-16x16", "gemm-16bit-8x20", "gemm-fp32-16x16", "residue-b-only")


def _two_columns(pat):
    """two columns read together by as many rows as possible"""
    counts = np.bincount(pat.ci, minlength=pat.cols)
    top = np.argsort(-counts)[:24]
    rows_of = {int(c): set(pat.row_of[pat.ci == c].tolist()) for c in top}
    c1, c2 = max(((a, b) for a in rows_of for b in rows_of if a < b), key=lambda ab: len(rows_of[ab[0]] & rows_of[ab[1]]))
    assert rows_of[c1] & rows_of[c2]
    return c1, c2, rows_of[c1]


@pytest.mark.parametrize("name", NONFINITE_PATHS)
def test_nonfinite_operands_stay_where_they_are_read(engine, oracle, patterns, name):
    """NaN in a few elements of A, +inf in one column of B and -inf in another (rows that read both, entries that hit
    inf * 0): every entry reading none of them equals the finite baseline; every other entry has the model's class and,
    when finite, its exact value.  NaN in an empty row of A and in a column of B no entry reads changes nothing."""
    K = 64
    for pname in (_pats(name)[1:] if name != "residue-b-only" else _pats(name)):
        pat = patterns[pname]
        plan = _build(engine, pat, name)
        rng = np.random.default_rng(23)
        try:
            A, B = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
            c1, c2, readers = _two_columns(pat)
            live = np.flatnonzero(np.diff(pat.ro.astype(np.int64)) > 0)
            nan_rows = rng.choice(live, size=3, replace=False)
            readers = np.array(sorted(readers))
            A[readers[::2], 7] = 0.0                     # inf * 0 in half of c1's readers
            A2, B2 = A.copy(), B.copy()
            A2[nan_rows, rng.integers(K, size=3)] = np.nan
            B2[c1, 7], B2[c2, 40] = np.inf, -np.inf
            touched = np.isin(pat.row_of, nan_rows) | np.isin(pat.ci, [c1, c2])
            # the unread elements: an empty row of A, the column of B no entry reads
            empty = np.flatnonzero(np.diff(pat.ro.astype(np.int64)) == 0)
            dead = np.setdiff1d(np.arange(pat.cols), pat.ci)
            assert (empty.size and dead.size) or not pname.startswith("rand")
            A3, B3 = A.copy(), B.copy()
            A3[empty, :] = np.nan
            B3[dead, :] = np.nan
            for mode in (0, 1, 2):
                base = plan.run(K, A, B, mode)
                where = f"{name} {pname} mode={mode}"
                assert_path(plan, name, K, mode)
                rounded = plan.rounded(K, mode)
                assert_exact(base, model(oracle, pat, K, A, B, mode, rounded), where + " baseline")
                got = plan.run(K, A2, B2, mode)
                want = model(oracle, pat, K, A2, B2, mode, rounded)
                assert np.isnan(want[touched]).any() and np.isinf(want[touched]).any()
                assert np.array_equal(got[~touched], base[~touched]), where + " untouched entries changed"
                assert_exact(got, want, where + " non-finite")
                if empty.size or dead.size:
                    got = plan.run(K, A3, B3, mode)
                    assert_exact(got, base.astype(np.float64), where + " unread NaN")
        finally:
            plan.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. fp16 overflow through a whole call
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("stream-pass", "stream-cvt-in-kernel", "sweep-16bit", "sweep-fp32", "gemm-16bit-16x16",
                                  "gemm-fp32-16x16", "residue-b-only"))
def test_fp16_overflow_through_a_call(engine, oracle, patterns, name):
    """At most one element per row of A in [65504, 65535]: in mode 0 exactly the entries reading an element >= 65520
    (rounds to inf) leave the finite range, as the model predicts; every other entry - and every entry of modes 1 and 2
    (bf16 rounds these to 65536) - is the exact dot product (65536 * 127 + 511 * 127^2 < 2^24)."""
    K = 128 if 128 in PATHS[name]["ks"] else 64
    pat = patterns["rand-sparse" if name == "residue-b-only" else "nips-hybrid"]
    plan = _build(engine, pat, name)
    rng = np.random.default_rng(31)
    try:
        A, B = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
        big = rng.choice(pat.rows, size=pat.rows // 3, replace=False)
        hot = big[: big.size // 2]
        A[hot, rng.integers(K, size=hot.size)] = rng.integers(65520, 65536, size=hot.size)
        warm = big[big.size // 2:]
        A[warm, rng.integers(K, size=warm.size)] = rng.integers(65504, 65520, size=warm.size)
        A[big[::2]] *= -1
        for mode in (0, 1, 2):
            got = plan.run(K, A, B, mode)
            assert_path(plan, name, K, mode)
            rounded = plan.rounded(K, mode)
            want = model(oracle, pat, K, A, B, mode, rounded)
            assert_exact(got, want, f"{name} mode={mode}")
            reads_hot = np.isin(pat.row_of, hot) & rounded
            if mode == 0:
                assert not np.isfinite(want[reads_hot]).any() and np.isfinite(want[~reads_hot]).all()
                assert reads_hot.any()
            else:
                assert np.isfinite(want).all()
    finally:
        plan.close()
