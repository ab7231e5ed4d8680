"""fp16 / bf16 tensors end to end on the device: bsmr_sddmm_16, bsmr_spmm_16, bsmr_sddmm_backward_16 (include/bsmr_hip.h
"fp16 / bf16 tensors end to end").

The gathers: Y16 = round_mode(Y), Y the fp32 fma-chain twin (tests/gather_twin.py) on (v, widen(X16)) - so the expected
result is always oracle.round_array(2 if fp16 else 3, twin), compared bit for bit after widening the device's words
(NaN by class).  16-bit inputs are made with torch's CPU cast, which equals the oracle's rounding.  One pattern, built
here in numpy, puts both directions on every boundary of the kernels: an empty row and an empty column, lists of 1, 3,
4, 5, 63, 64, 65 and 511 entries, one row and one column of 1300 entries (three chunks each: the fp32 partials and the
rounding reduce), an odd nnz.  K covers every slice width (32, 64, 128, 256) and several slices per row (96, 512); both
lane layouts, both formats, both directions, one problem and a batch of three.

The forward: every path of tests/test_gpu_numerics.py PATHS on integer operands that are exact in both formats, so P is
the exact dot product with no tolerance - in particular on the plans whose fp32 road never makes 16-bit copies
(stream-fp32-residue, stream-cvt-in-kernel, sweep-fp32, gemm-fp32-*, residue-b-only), where bsmr_sddmm_lowp would refuse
or read fp32 operands."""
import numpy as np
import pytest

from gather_twin import CHUNK, assert_twin, col_lists, gather, row_lists
from guarded import OPERAND, VALUES, Guarded, check_all
from test_gpu_numerics import BATCHED, PATHS, _build, assert_exact, exact_ints, model, patterns  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = (32, 64, 96, 128, 256, 512)
SIZE = 1400
ROW_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 511, 1300)
LONG_COL, EMPTY_COL, LONG = 7, 9, 1300
NB = 3
ROUND = {0: 2, 1: 3}                             # engine mode -> oracle.round_array id (fp16 RNE, bf16 RNE)
DT = {0: torch.float16, 1: torch.bfloat16}
DENSE_PATS = ("nips-dense", "nips-hybrid", "rand-hybrid")


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_dev())


def _nan16(mode, *shape):
    return torch.full(shape, float("nan"), dtype=DT[mode], device=_dev())    # poisoned: every element is written


def _wide(rng, shape, lo, hi):
    """+-m 2^e with a full 24-bit m and e in [lo, hi]"""
    m = rng.integers(1 << 23, 1 << 24, size=shape).astype(np.float64)
    s = rng.choice([-1.0, 1.0], size=shape)
    return (s * np.ldexp(m, rng.integers(lo, hi + 1, size=shape) - 23)).astype(np.float32)


def to16(mode, a):
    """fp32 array -> CPU tensor of the mode's 16-bit dtype (torch's cast = the oracle's rounding)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[mode])


def words(t16):
    return t16.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def widen_words(mode, w):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int16)).view(DT[mode]).float().numpy()


def build_pattern(seed=23):
    rng = np.random.default_rng(seed)
    special_rows = {40 + 120 * i: n for i, n in enumerate(ROW_LENGTHS)}
    plain_cols = np.array([c for c in range(SIZE) if c not in (LONG_COL, EMPTY_COL)])
    per_row = []
    for r in range(SIZE):
        n = special_rows.get(r, int(rng.integers(2, 5)))
        per_row.append(set(rng.choice(plain_cols, n, replace=False).tolist()))
    plain_rows = np.array([r for r in range(SIZE) if r not in special_rows])
    for r in rng.choice(plain_rows, LONG, replace=False):
        per_row[r].add(LONG_COL)
    if sum(len(s) for s in per_row) % 2 == 0:
        r = int(plain_rows[0])
        per_row[r].add(int(next(c for c in plain_cols if c not in per_row[r])))
    out = []
    for r, s in enumerate(per_row):
        a = np.array(sorted(s), dtype=np.uint32)
        out.append(rng.permutation(a) if r % 2 else a)
    ro = np.zeros(SIZE + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([a.size for a in out])
    return ro, np.concatenate(out).astype(np.uint32), {n: r for r, n in special_rows.items()}


class Pattern:
    def __init__(self, engine):
        self.engine = engine
        self.rows = self.cols = SIZE
        self.ro, self.ci, self.row_with = build_pattern()
        self.nnz = int(self.ci.size)
        self.rl = row_lists(self.ro, self.ci)
        self.cl = col_lists(self.rows, self.cols, self.ro, self.ci)
        self.bw = {}
        with pytest.MonkeyPatch.context() as mp:                       # the layout is read at create
            for lanes in (4, 8):
                mp.setenv("BSMR_GATHER16_LANES", str(lanes))
                self.bw[lanes] = engine.backward_create(self.rows, self.cols, self.ro, self.ci, device=0)
        # the planted entries (batch 0): a one-entry row, a 5-entry row, an entry of the 3-entry row
        self.e_sub = int(self.ro[self.row_with[1]])
        r5 = self.row_with[5]
        self.e_big = np.arange(int(self.ro[r5]), int(self.ro[r5 + 1]))
        self.e_nan = int(self.ro[self.row_with[3]]) + 1
        self._data = {}

    def lists(self, transpose):
        return self.cl if transpose else self.rl

    def data(self, mode, K):
        """(v (NB, nnz) fp32, Xn16 (NB, N, K), Xm16 (NB, M, K)) as CPU tensors, made once per (mode, K): v over 2^+-3, X
        over 2^[-8, 4] so that sums stay inside the fp16 range, with the special cases planted in batch 0"""
        if (mode, K) not in self._data:
            rng = np.random.default_rng(4000 + K)
            v = _wide(rng, (NB, self.nnz), -3, 3)
            Xn, Xm = _wide(rng, (NB, self.cols, K), -8, 4), _wide(rng, (NB, self.rows, K), -8, 4)
            v[0, self.e_sub] = 2.0 ** -20              # products of 2^[-28, -16]: fp16 subnormals (and zeros)
            v[0, self.e_big] = 3000.0                  # 5 x 3000 x 30 = 450 000: beyond fp16, finite in fp32 and bf16
            Xn[0, self.ci[self.e_big], 0], Xn[0, self.ci[self.e_big], 1] = 30.0, -30.0
            v[0, self.e_nan] = np.nan
            self._data[(mode, K)] = (v, to16(mode, Xn), to16(mode, Xm))
        return self._data[(mode, K)]


@pytest.fixture(scope="module")
def pat(engine):
    p = Pattern(engine)
    yield p
    for bw in p.bw.values():
        engine.backward_destroy(bw)


@pytest.fixture(scope="module")
def twins(oracle, pat):
    """get(mode, transpose, K) -> (fp32 twin on (v, widen(X16)), its rounding to the mode's format), (NB, rows, K) each;
    computed once and read-only"""
    made = {}

    def get(mode, transpose, K):
        key = (mode, bool(transpose), K)
        if key not in made:
            v, Xn16, Xm16 = pat.data(mode, K)
            X = (Xm16 if transpose else Xn16).float().numpy()
            twin = np.stack([gather(oracle, pat.lists(transpose), v[b], X[b]) for b in range(NB)])
            want = oracle.round_array(ROUND[mode], twin)
            twin.setflags(write=False)
            want.setflags(write=False)
            made[key] = (twin, want)
        return made[key]

    return get


# ---- device calls --------------------------------------------------------------------------------------------------
def dev_spmm16(engine, bw, p, K, transpose, v, X16, mode, nb):
    """v (nb, nnz) numpy, X16 (nb, rows, K) CPU tensor -> Y widened to fp32 (nb, rows_y, K), and its raw words"""
    tv, tX = _t(v[:nb]), X16[:nb].contiguous().to(_dev())
    tY = _nan16(mode, nb, p.cols if transpose else p.rows, K)
    engine.spmm_16(bw, K, transpose, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), nb, _stream(), mode=mode)
    torch.cuda.synchronize()
    return tY.float().cpu().numpy(), words(tY)


def dev_backward16(engine, bw, p, K, dP, A16, B16, mode, nb, want_a=True, want_b=True):
    tdP, tA, tB = _t(dP[:nb]), A16[:nb].contiguous().to(_dev()), B16[:nb].contiguous().to(_dev())
    tdA = _nan16(mode, nb, p.rows, K) if want_a else None
    tdB = _nan16(mode, nb, p.cols, K) if want_b else None
    engine.sddmm_backward_16(bw, K, tdP.data_ptr(), tA.data_ptr(), tB.data_ptr(), tdA.data_ptr() if want_a else None,
                             tdB.data_ptr() if want_b else None, nb, _stream(), mode=mode)
    torch.cuda.synchronize()
    out = lambda t: None if t is None else (t.float().cpu().numpy(), words(t))
    return out(tdA), out(tdB)


# ---- 0. the pattern and the planted cases --------------------------------------------------------------------------
def test_pattern_has_its_lists(engine, pat):
    rl, cl = np.diff(pat.ro.astype(np.int64)), np.bincount(pat.ci, minlength=pat.cols)
    assert set(ROW_LENGTHS) <= set(rl.tolist()) and (rl == 0).sum() == 1
    assert cl[LONG_COL] == LONG and cl[EMPTY_COL] == 0 and (cl == 0).sum() == 1
    assert pat.nnz % 2 == 1
    for r in range(pat.rows):
        assert np.unique(pat.ci[pat.ro[r]:pat.ro[r + 1]]).size == rl[r]
    assert -(-LONG // CHUNK) == 3 and rl.max() == LONG and cl.max() == LONG
    for bw in pat.bw.values():
        st = engine.backward_stats(bw)
        assert (st["split_rows"], st["split_cols"]) == (1, 1)


def _check_planted(p, mode, transpose, twin, want):
    """the twin itself shows every planted case (batch 0), so none is vacuous"""
    nan_dest = int(p.ci[p.e_nan]) if transpose else p.row_with[3]
    assert np.isnan(want[0, nan_dest]).all()                                 # a NaN in v reaches its destination ...
    rest = np.ones(want.shape[1], bool)
    rest[nan_dest] = False
    assert not np.isnan(want[:, rest]).any() and not np.isnan(want[1:]).any()   # ... and no other
    if transpose or mode != 0:
        return
    r1, r5 = p.row_with[1], p.row_with[5]
    sub = (np.abs(want[0, r1]) > 0) & (np.abs(want[0, r1]) < 2.0 ** -14)
    assert sub.sum() >= 4 and (twin[0, r1][sub] != want[0, r1][sub]).any()   # fp16 subnormals, and rounding into them
    assert twin[0, r5, 0] == 450000.0 and twin[0, r5, 1] == -450000.0        # finite fp32 sums beyond 65504 ...
    assert want[0, r5, 0] == np.inf and want[0, r5, 1] == -np.inf            # ... become +-inf


def _check_empty(p, transpose, w16):
    """destinations without entries are +0: all sixteen bits"""
    d = EMPTY_COL if transpose else p.row_with[0]
    assert not w16[:, d].any()


# ---- 1. the gathers equal the rounded twin, in both lane layouts ---------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mode", (0, 1))
def test_spmm_16_equals_the_rounded_twin(engine, pat, twins, mode, K):
    v, Xn16, Xm16 = pat.data(mode, K)
    for transpose, X16 in ((0, Xn16), (1, Xm16)):
        twin, want = twins(mode, transpose, K)
        _check_planted(pat, mode, transpose, twin, want)
        bits = {}
        for lanes, bw in pat.bw.items():
            for nb in (1, NB):
                where = f"spmm_16 mode={mode} transpose={transpose} K={K} lanes={lanes} batches={nb}"
                Y, w16 = dev_spmm16(engine, bw, pat, K, transpose, v, X16, mode, nb)
                assert_twin(Y, want[:nb], where)
                _check_empty(pat, transpose, w16)
                bits[(lanes, nb)] = w16.tobytes()
        for nb in (1, NB):
            assert bits[(4, nb)] == bits[(8, nb)], f"mode={mode} transpose={transpose} K={K}: the two layouts differ"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mode", (0, 1))
def test_backward_16_equals_the_rounded_twin(engine, pat, twins, mode, K):
    """dA16 = round(S_dP widen(B16)), dB16 = round(S_dP^T widen(A16)): both together in both layouts and batch sizes,
    each alone once"""
    dP, B16, A16 = pat.data(mode, K)
    wantA, wantB = twins(mode, 0, K)[1], twins(mode, 1, K)[1]
    bits = {}
    for lanes, bw in pat.bw.items():
        for nb in (1, NB):
            where = f"backward_16 mode={mode} K={K} lanes={lanes} batches={nb}"
            (dA, wA), (dB, wB) = dev_backward16(engine, bw, pat, K, dP, A16, B16, mode, nb)
            assert_twin(dA, wantA[:nb], where + ": dA")
            assert_twin(dB, wantB[:nb], where + ": dB")
            _check_empty(pat, 0, wA)
            _check_empty(pat, 1, wB)
            bits[(lanes, nb)] = (wA.tobytes(), wB.tobytes())
    for nb in (1, NB):
        assert bits[(4, nb)] == bits[(8, nb)], f"mode={mode} K={K}: the two layouts differ"
    bw = pat.bw[8]
    only_a, none_b = dev_backward16(engine, bw, pat, K, dP, A16, B16, mode, 1, want_b=False)
    none_a, only_b = dev_backward16(engine, bw, pat, K, dP, A16, B16, mode, 1, want_a=False)
    assert none_a is None and none_b is None
    assert (only_a[1].tobytes(), only_b[1].tobytes()) == bits[(8, 1)]


def test_rounding_happens_once_after_the_fp32_reduce(engine, pat, twins):
    """the three-chunk lists: the device equals round(fp32 sum of the fp32 partials); rounding each partial first would
    give other bits on this data, so the check is not vacuous"""
    K, mode = 128, 0
    v, Xn16, _ = pat.data(mode, K)
    twin, want = twins(mode, 0, K)
    r = pat.row_with[LONG]
    lo, hi = int(pat.ro[r]), int(pat.ro[r + 1])
    X = Xn16[0].float().numpy()
    part = [np.zeros(K, np.float32) for _ in range(3)]
    for k in range(3):
        for t in range(lo + k * CHUNK, min(hi, lo + (k + 1) * CHUNK)):
            part[k] = (v[0, t].astype(np.float64) * X[pat.ci[t]].astype(np.float64) + part[k]).astype(np.float32)
    h = lambda a: a.astype(np.float16).astype(np.float32)
    early = h(h(h(part[0]) + h(part[1])) + h(part[2]))
    assert (early != want[0, r]).any()
    Y, _ = dev_spmm16(engine, pat.bw[8], pat, K, 0, v, Xn16, mode, 1)
    assert_twin(Y[0, r], want[0, r], "the 1300-entry row")


# ---- 2. nnz = 0, the workspace -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", (1, 2))
def test_empty_pattern_with_null_inputs(engine, nb):
    M, N, K = 5, 7, 64
    bw = engine.backward_create(M, N, np.zeros(M + 1, np.uint32), np.zeros(0, np.uint32), device=0)
    hip, s = engine.hip(), _stream()
    try:
        for mode in (0, 1):
            for transpose, rows_y in ((0, M), (1, N)):
                Y = _nan16(mode, nb, rows_y, K)
                assert hip.bsmr_spmm_16(bw, K, transpose, None, None, Y.data_ptr(), nb, mode, s) == engine.OK
                torch.cuda.synchronize()
                assert not words(Y).any()
            dA, dB = _nan16(mode, nb, M, K), _nan16(mode, nb, N, K)
            assert hip.bsmr_sddmm_backward_16(bw, K, None, None, None, dA.data_ptr(), dB.data_ptr(), nb, mode, s) == engine.OK
            torch.cuda.synchronize()
            assert not words(dA).any() and not words(dB).any()
            assert hip.bsmr_spmm_16(bw, K, 0, None, None, None, nb, mode, s) == engine.ERR_INVALID_ARG
    finally:
        engine.backward_destroy(bw)


def test_calls_after_reserve_allocate_nothing(engine, pat, twins):
    """bsmr_backward_reserve(K, num_batches) - the fp32 reserve, no room for 16-bit copies - covers the new calls"""
    K, nb, mode = 128, 2, 1
    v, Xn16, Xm16 = pat.data(mode, K)
    bw = engine.backward_create(pat.rows, pat.cols, pat.ro, pat.ci, device=0)
    try:
        engine.backward_reserve(bw, K, nb)
        reserved = engine.backward_stats(bw)["workspace_bytes"]
        assert reserved == (3 * K + pat.nnz) * nb * 4                        # three chunk partials + the permuted values
        for _ in range(2):
            for transpose, X16 in ((0, Xn16), (1, Xm16)):
                Y, _ = dev_spmm16(engine, bw, pat, K, transpose, v, X16, mode, nb)
                assert_twin(Y, twins(mode, transpose, K)[1][:nb], f"after reserve, transpose={transpose}")
            (dA, _), (dB, _) = dev_backward16(engine, bw, pat, K, v, Xm16, Xn16, mode, nb)
            assert_twin(dA, twins(mode, 0, K)[1][:nb], "after reserve: dA")
            assert_twin(dB, twins(mode, 1, K)[1][:nb], "after reserve: dB")
            assert engine.backward_stats(bw)["workspace_bytes"] == reserved
    finally:
        engine.backward_destroy(bw)


# ---- 3. bsmr_sddmm_16 on every path --------------------------------------------------------------------------------
def _ks(name):
    return tuple(sorted({min(K, 512) for K in PATHS[name]["ks"]}))           # 1024 x 127^2 passes 2^24: capped at 512


def dev_sddmm16(engine, plan, K, A16, B16, mode, nb=1):
    """A16 / B16: CPU tensors (nb, rows, K) or (rows, K) -> P (nb, nnz)"""
    tA, tB = A16.contiguous().to(_dev()), B16.contiguous().to(_dev())
    tP = torch.full((nb, plan.pat.nnz), float("nan"), dtype=torch.float32, device=_dev())
    engine.sddmm_16(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), nb, mode, _stream())
    torch.cuda.synchronize()
    return tP.cpu().numpy()


def _assert_engine(plan, name, K, mode):
    """the call that ran last used the engine and format the path is named after (test_gpu_numerics.assert_path's
    check of bsmr_plan_dense_choice): an fp32-road plan keeps its engine here, on that engine's 16-bit kernel"""
    group = PATHS[name]["group"]
    if group is None:
        assert plan.plan_stats()["num_dense_entries"] == 0, name
        return
    g = plan.dense_group(K)
    if group == "sweep":
        assert g >= 4 and g % 4 == 0, (name, K, mode, g)
    else:
        assert g == group, (name, K, mode, g)


@pytest.mark.parametrize("name", list(PATHS))
def test_sddmm_16_is_exact_on_every_path(engine, oracle, patterns, name):
    """signed integers |x| <= 127 are exact in fp16 and bf16 and their sums exact in fp32 up to K = 512: P equals the
    exact dot product on every engine and residue form, without fp32 operands"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    for pname in PATHS[name].get("pats", DENSE_PATS):
        pat = patterns[pname]
        plan = _build(engine, pat, name)
        every = np.ones(pat.nnz, dtype=bool)
        try:
            for K in _ks(name):
                nb = NB if name in BATCHED else 1
                A = np.stack([exact_ints(rng, pat.rows, K) for _ in range(nb)])
                B = np.stack([exact_ints(rng, pat.cols, K) for _ in range(nb)])
                for mode in (0, 1):
                    A16, B16 = to16(mode, A), to16(mode, B)
                    assert np.array_equal(A16.float().numpy(), A) and np.array_equal(B16.float().numpy(), B)
                    P1 = dev_sddmm16(engine, plan, K, A16[0], B16[0], mode)
                    _assert_engine(plan, name, K, mode)
                    assert_exact(P1[0], model(oracle, pat, K, A[0], B[0], mode, every), f"{name} {pname} K={K} mode={mode}")
                    if nb > 1:
                        Pb = dev_sddmm16(engine, plan, K, A16, B16, mode, nb)
                        for b in range(nb):
                            assert_exact(Pb[b], model(oracle, pat, K, A[b], B[b], mode, every),
                                         f"{name} {pname} K={K} mode={mode} batch {b}")
        finally:
            plan.close()


@pytest.mark.parametrize("mode", (0, 1))
def test_sddmm_16_is_sddmm_lowp_where_that_serves(engine, patterns, mode):
    """stream-pass on a hybrid plan, random operands: the same kernels on the same copies, the same bits"""
    pat = patterns["nips-hybrid"]
    plan = _build(engine, pat, "stream-pass")
    rng = np.random.default_rng(91 + mode)
    try:
        for K in (64, 512):
            A16 = to16(mode, rng.uniform(-1, 1, (pat.rows, K)))
            B16 = to16(mode, rng.uniform(-1, 1, (pat.cols, K)))
            assert plan.sparse_choice(K, mode)["low_precision"] and plan.plan_stats()["num_sparse_entries"] > 0
            tA, tB = A16.to(_dev()), B16.to(_dev())
            tP = torch.full((pat.nnz,), float("nan"), dtype=torch.float32, device=_dev())
            engine.sddmm_lowp(plan.plan, K, tA.data_ptr(), tB.data_ptr(), None, None, tP.data_ptr(), mode, _stream())
            torch.cuda.synchronize()
            got = dev_sddmm16(engine, plan, K, A16, B16, mode)[0]
            assert np.isfinite(got).all() and got.tobytes() == tP.cpu().numpy().tobytes(), f"K={K}"
    finally:
        plan.close()


# ---- 4. the rules --------------------------------------------------------------------------------------------------
def test_misaligned_pointers_are_refused_before_any_work(engine, pat, patterns):
    hip, bad, s = engine.hip(), engine.ERR_INVALID_ARG, _stream()
    K = 64
    npat = patterns["nips-hybrid"]
    plan = _build(engine, npat, "stream-pass")
    t = torch.zeros(1500 * K + 50000, dtype=torch.float32, device=_dev())
    p = t.data_ptr()
    assert p % 16 == 0
    try:
        for mode in (0, 1):
            for a, b, P in ((p + 8, p, p), (p, p + 8, p), (p, p, p + 2), (None, p, p), (p, None, p), (p, p, None)):
                assert hip.bsmr_sddmm_16(plan.plan, K, a, b, P, 1, mode, s) == bad
            assert hip.bsmr_sddmm_16(plan.plan, K, p, p, p, 65536, mode, s) == bad
            assert hip.bsmr_sddmm_16(plan.plan, K, p, p, p, 0, mode, s) == engine.OK            # no-op
            bw = pat.bw[8]
            for v, x, y in ((p + 2, p, p), (p, p + 8, p), (p, p, p + 8), (None, p, p), (p, None, p), (p, p, None)):
                assert hip.bsmr_spmm_16(bw, K, 0, v, x, y, 1, mode, s) == bad
            assert hip.bsmr_spmm_16(bw, K, 2, p, p, p, 1, mode, s) == bad                       # transpose is 0 or 1
            assert hip.bsmr_spmm_16(bw, K, 0, p, p, p, 65536, mode, s) == bad
            assert hip.bsmr_spmm_16(bw, K, 0, p, p, p, 0, mode, s) == engine.OK
            for dp, a, b, da, db in ((p + 2, p, p, p, p), (p, p + 8, p, p, p), (p, p, p + 8, p, p), (p, p, p, p + 8, p),
                                     (p, p, p, p, p + 8), (None, p, p, p, p), (p, None, p, None, p), (p, p, None, p, None)):
                assert hip.bsmr_sddmm_backward_16(bw, K, dp, a, b, da, db, 1, mode, s) == bad
            assert hip.bsmr_sddmm_backward_16(bw, K, p, p, p, p, p, 0, mode, s) == engine.OK
            assert hip.bsmr_sddmm_backward_16(bw, K, p, p, p, None, None, 1, mode, s) == engine.OK   # nothing asked for
        for call in (lambda m, k: hip.bsmr_sddmm_16(plan.plan, k, p, p, p, 1, m, s),
                     lambda m, k: hip.bsmr_spmm_16(pat.bw[8], k, 0, p, p, p, 1, m, s),
                     lambda m, k: hip.bsmr_sddmm_backward_16(pat.bw[8], k, p, p, p, p, p, 1, m, s)):
            assert call(engine.COMPUTE_F32, K) == bad
            assert call(0, 48) == engine.ERR_UNSUPPORTED_K and call(1, 0) == engine.ERR_UNSUPPORTED_K
        torch.cuda.synchronize()
        assert not t.any()                                                                       # nothing ran
    finally:
        plan.close()


# ---- 5. extents ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (32, 256))
@pytest.mark.parametrize("mode", (0, 1))
def test_calls_stay_inside_the_buffers(engine, oracle, pat, patterns, mode, K):
    """all three calls, 16-bit arrays 16 bytes and value arrays 4 bytes past a 512-byte boundary, two batches: guards
    and inputs intact, every output word written, the expected bits"""
    nb = 2
    dev, s = _dev(), _stream()
    rng = np.random.default_rng(57 * K + mode)
    v = _wide(rng, (nb, pat.nnz), -3, 3)
    Xn16, Xm16 = to16(mode, _wide(rng, (nb, pat.cols, K), -8, 4)), to16(mode, _wide(rng, (nb, pat.rows, K), -8, 4))
    want = {t: oracle.round_array(ROUND[mode], np.stack([gather(oracle, pat.lists(t), v[b], X[b].float().numpy())
                                                          for b in range(nb)]))
            for t, X in ((0, Xn16), (1, Xm16))}
    gv = Guarded.input("v", v, VALUES, K, dev)
    g16 = {0: Guarded.input("Xn16", words(Xn16), OPERAND, K, dev, dtype=np.uint16),
           1: Guarded.input("Xm16", words(Xm16), OPERAND, K, dev, dtype=np.uint16)}
    assert g16[0].nbytes == pat.cols * K * 2 * nb
    for lanes, bw in pat.bw.items():
        for transpose, rows in ((0, pat.rows), (1, pat.cols)):
            gY = Guarded.output("Y16", nb * rows * K, OPERAND, K, dev, dtype=np.uint16)
            engine.spmm_16(bw, K, transpose, gv.ptr, g16[transpose].ptr, gY.ptr, nb, s, mode=mode)
            torch.cuda.synchronize()
            check_all(gv, g16[transpose], gY)
            assert_twin(widen_words(mode, gY.numpy()).reshape(nb, rows, K), want[transpose],
                        f"mode={mode} K={K} lanes={lanes} transpose={transpose}: spmm_16")
        for want_a, want_b in ((True, True), (True, False), (False, True)):
            gdA = Guarded.output("dA16", nb * pat.rows * K, OPERAND, K, dev, dtype=np.uint16) if want_a else None
            gdB = Guarded.output("dB16", nb * pat.cols * K, OPERAND, K, dev, dtype=np.uint16) if want_b else None
            engine.sddmm_backward_16(bw, K, gv.ptr, g16[1].ptr, g16[0].ptr, gdA.ptr if gdA else None,
                                     gdB.ptr if gdB else None, nb, s, mode=mode)
            torch.cuda.synchronize()
            check_all(gv, g16[0], g16[1], gdA, gdB)
            if gdA:
                assert_twin(widen_words(mode, gdA.numpy()).reshape(nb, pat.rows, K), want[0], f"lanes={lanes}: dA16")
            if gdB:
                assert_twin(widen_words(mode, gdB.numpy()).reshape(nb, pat.cols, K), want[1], f"lanes={lanes}: dB16")
    # the forward: a hybrid plan (dense kernel + residue) and an all-sparse one
    for pname, name in (("nips-hybrid", "stream-pass"), ("rand-sparse", "residue-b-only")):
        npat = patterns[pname]
        plan = _build(engine, npat, name)
        try:
            A = np.stack([exact_ints(rng, npat.rows, K) for _ in range(nb)])
            B = np.stack([exact_ints(rng, npat.cols, K) for _ in range(nb)])
            gA = Guarded.input("A16", words(to16(mode, A)), OPERAND, K, dev, dtype=np.uint16)
            gB = Guarded.input("B16", words(to16(mode, B)), OPERAND, K, dev, dtype=np.uint16)
            gP = Guarded.output("P", nb * npat.nnz, VALUES, K, dev)
            engine.sddmm_16(plan.plan, K, gA.ptr, gB.ptr, gP.ptr, nb, mode, s)
            torch.cuda.synchronize()
            check_all(gA, gB, gP)
            P = gP.numpy().reshape(nb, npat.nnz)
            for b in range(nb):
                assert_exact(P[b], model(oracle, npat, K, A[b], B[b], mode, np.ones(npat.nnz, bool)),
                             f"{name} {pname} K={K} mode={mode} batch {b}")
        finally:
            plan.close()
