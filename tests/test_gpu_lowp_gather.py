"""The fp16 / bf16 gather modes on the device (bsmr_spmm_mode, bsmr_sddmm_backward_mode, bsmr_spmm_lowp,
bsmr_backward_reserve_mode; include/bsmr_hip.h "fp16 / bf16 gather modes").

Widening a 16-bit element to fp32 is exact, so the contract needs no oracle of its own: every output element equals the
fp32 fma-chain twin (oracle_gather_twin through tests/gather_twin.py) applied to (v, round(X)), round = the oracle's
fp16 / bf16 round-to-nearest-even (oracle.round_array, ids 2 / 3 as tests/test_oracle.py pins them).  One small pattern,
built here, puts both directions on every boundary of the kernel: lists of 0, 1, 3, 4, 5, 63, 64, 65 entries, whole,
two-chunk and three-chunk lists, and an odd nnz so that the second batch starts on an odd float.  K covers every slice
width (32, 64, 128, 256) and several slices per row (96, 512).  The lists of the twin come from numpy, never from the
library."""
import numpy as np
import pytest

from gather_twin import CHUNK, assert_twin, col_lists, gather, row_lists
from guarded import OPERAND, VALUES, Guarded, check_all

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = (32, 64, 96, 128, 256, 512)
ROW_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 512, 513, 1025)
LONG_COLS = {3: 1030, 600: 513}                  # column id: rows that store it
SIZE = 1100
NAN_SRC, BIG_SRC = 20, (21, 22)                  # source rows of X that hold NaN / values beyond the fp16 range
U = 2.0 ** -24
U16 = {0: 2.0 ** -11, 1: 2.0 ** -8}              # unit roundoff of fp16 / bf16
ROUND = {0: 2, 1: 3}                             # engine mode -> oracle.round_array id (fp16 RNE, bf16 RNE)


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_dev())


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=_dev())   # poisoned: every element is written


def build_pattern(seed=11):
    """1100 x 1100, about 7 000 entries, duplicate-free, an odd nnz; the column ids of every other row are shuffled"""
    rng = np.random.default_rng(seed)
    special_rows = {50 + 90 * i: n for i, n in enumerate(ROW_LENGTHS)}
    plain_cols = np.array([c for c in range(SIZE) if c not in LONG_COLS])
    per_row = []
    for r in range(SIZE):
        n = special_rows.get(r, int(rng.integers(2, 5)))
        per_row.append(set(rng.choice(plain_cols, n, replace=False).tolist()))
    plain_rows = np.array([r for r in range(SIZE) if r not in special_rows])
    for c, n in LONG_COLS.items():
        for r in rng.choice(plain_rows, n, replace=False):
            per_row[r].add(c)
    for s in (NAN_SRC,) + BIG_SRC:               # every special source is listed by rows, and has entries as a row
        for r in rng.choice(plain_rows, 3, replace=False):
            per_row[r].add(s)
    if sum(len(s) for s in per_row) % 2 == 0:
        per_row[plain_rows[0]].add(int(next(c for c in plain_cols if c not in per_row[plain_rows[0]])))
    out = []
    for r, s in enumerate(per_row):
        a = np.array(sorted(s), dtype=np.uint32)
        out.append(rng.permutation(a) if r % 2 else a)
    ro = np.zeros(SIZE + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([a.size for a in out])
    return SIZE, SIZE, ro, np.concatenate(out)


class Pattern:
    def __init__(self, engine):
        self.engine = engine
        self.rows, self.cols, self.ro, self.ci = build_pattern()
        self.nnz = int(self.ci.size)
        self.rl = row_lists(self.ro, self.ci)
        self.cl = col_lists(self.rows, self.cols, self.ro, self.ci)
        self.bw = engine.backward_create(self.rows, self.cols, self.ro, self.ci, device=0)   # natural row order
        self._data = {}

    def lists(self, transpose):
        return self.cl if transpose else self.rl

    def data(self, K):
        """(v, Xn, Xm) of this K, made once: v narrow and signed, X signed over 2^+-12 with the special values planted"""
        if K not in self._data:
            rng = np.random.default_rng(1000 + K)
            self._data[K] = (_wide(rng, self.nnz, -4, 4), special_x(rng, self.cols, K), special_x(rng, self.rows, K))
        return self._data[K]


@pytest.fixture(scope="module")
def pat(engine):
    p = Pattern(engine)
    yield p
    engine.backward_destroy(p.bw)


@pytest.fixture(scope="module")
def twins(oracle, pat):
    """twin(mode, transpose, K) -> the fp32 twin on (v, round_mode(X)); mode 2 = on X itself.  Computed once each."""
    made = {}

    def get(mode, transpose, K):
        key = (mode, bool(transpose), K)
        if key not in made:
            v, Xn, Xm = pat.data(K)
            X = Xm if transpose else Xn
            Xr = X if mode == 2 else oracle.round_array(ROUND[mode], X)
            made[key] = gather(oracle, pat.lists(transpose), v, Xr)
            made[key].setflags(write=False)
        return made[key]

    return get


# ---- operands ------------------------------------------------------------------------------------------------------
def _wide(rng, shape, lo, hi):
    """+-m 2^e with a full 24-bit m and e in [lo, hi]"""
    m = rng.integers(1 << 23, 1 << 24, size=shape).astype(np.float64)
    s = rng.choice([-1.0, 1.0], size=shape)
    return (s * np.ldexp(m, rng.integers(lo, hi + 1, size=shape) - 23)).astype(np.float32)


def special_x(rng, rows, K):
    X = _wide(rng, (rows, K), -12, 12)
    flat = X.reshape(-1)
    idx = rng.permutation(flat.size)
    n = flat.size // 16
    sub, tie16, tie_bf = idx[:n], idx[n:2 * n], idx[2 * n:3 * n]
    flat[sub] = _wide(rng, n, -20, -16)                                      # fp16 subnormals: below 2^-14
    sign = rng.choice([-1.0, 1.0], size=n)
    e = rng.integers(-6, 7, size=n)
    flat[tie16] = sign * np.ldexp(1 + (2 * rng.integers(0, 1024, n) + 1) * 2.0 ** -11, e)   # half way between two fp16
    flat[tie_bf] = sign * np.ldexp(1 + (2 * rng.integers(0, 128, n) + 1) * 2.0 ** -8, e)    # ... between two bf16
    X[BIG_SRC[0], 0::2], X[BIG_SRC[0], 1::2] = 70000.0, -1.0e5               # +-inf as fp16, finite as bf16
    X[BIG_SRC[1]] = 65520.0                                                   # the tie that rounds up to fp16's inf
    X[NAN_SRC] = np.nan
    return X


def bits16(oracle, mode, a):
    """the 16-bit words of round_mode(a), from the oracle's rounding"""
    r = oracle.round_array(ROUND[mode], np.ascontiguousarray(a, dtype=np.float32).ravel())
    if mode == 0:
        with np.errstate(over="ignore"):
            return r.astype(np.float16).view(np.uint16)
    return (r.view(np.uint32) >> 16).astype(np.uint16)


def same_bits(a, b, where):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), where


# ---- device calls --------------------------------------------------------------------------------------------------
def dev_spmm(engine, bw, p, K, transpose, v, X, mode, nb=1):
    tv, tX = _t(v), _t(X)
    tY = _nan(nb, p.cols if transpose else p.rows, K)
    engine.spmm(bw, K, transpose, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), nb, _stream(), mode=mode)
    torch.cuda.synchronize()
    return tY.cpu().numpy()[0] if nb == 1 else tY.cpu().numpy()


def dev_lowp(engine, bw, p, K, transpose, v, words, mode, nb=1):
    tv, tX = _t(v), words if isinstance(words, torch.Tensor) else _t(words.view(np.int16), np.int16)
    tY = _nan(nb, p.cols if transpose else p.rows, K)
    engine.spmm_lowp(bw, K, transpose, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), nb, _stream(), mode=mode)
    torch.cuda.synchronize()
    return tY.cpu().numpy()[0] if nb == 1 else tY.cpu().numpy()


def dev_backward(engine, bw, p, K, dP, A, B, mode, want_a=True, want_b=True, nb=1):
    tdP, tA, tB = _t(dP), _t(A), _t(B)
    tdA = _nan(nb, p.rows, K) if want_a else None
    tdB = _nan(nb, p.cols, K) if want_b else None
    engine.sddmm_backward(bw, K, tdP.data_ptr(), tA.data_ptr(), tB.data_ptr(), tdA.data_ptr() if want_a else None,
                          tdB.data_ptr() if want_b else None, nb, _stream(), mode=mode)
    torch.cuda.synchronize()
    sel = (lambda t: t.cpu().numpy()[0]) if nb == 1 else (lambda t: t.cpu().numpy())
    return (sel(tdA) if want_a else None), (sel(tdB) if want_b else None)


# ---- 0. the pattern ------------------------------------------------------------------------------------------------
def test_pattern_has_its_lists(engine, pat):
    rl, cl = np.diff(pat.ro.astype(np.int64)), np.bincount(pat.ci, minlength=pat.cols)
    assert set(ROW_LENGTHS) <= set(rl.tolist())
    assert all(cl[c] == n for c, n in LONG_COLS.items())
    assert 6500 <= pat.nnz <= 7500 and pat.nnz % 2 == 1
    for r in range(pat.rows):                                            # duplicate-free; some rows unsorted
        assert np.unique(pat.ci[pat.ro[r]:pat.ro[r + 1]]).size == rl[r]
    assert any((np.diff(pat.ci[pat.ro[r]:pat.ro[r + 1]].astype(np.int64)) < 0).any() for r in range(pat.rows))
    chunks = lambda n: {int(x) for x in -(-n[n > 0] // CHUNK)}
    assert {1, 2, 3} <= chunks(rl) and {1, 2, 3} <= chunks(cl)           # whole, two-chunk and three-chunk lists
    st = engine.backward_stats(pat.bw)
    assert (st["split_rows"], st["split_cols"]) == (2, 2)
    for s in (NAN_SRC,) + BIG_SRC:
        assert cl[s] > 0 and rl[s] > 0


# ---- 1. the twin, bit for bit --------------------------------------------------------------------------------------
def _listing(lists, sources):
    offsets, src, _ = lists
    hit = np.flatnonzero(np.isin(src, sources))
    return np.unique(np.searchsorted(offsets, hit, side="right") - 1)


def _check_special_rows(p, transpose, mode, Y, where):
    """NaN reaches exactly the destinations that list the NaN row; what is beyond the fp16 range becomes inf in fp16 only,
    and only in the destinations that list those rows"""
    lists = p.lists(transpose)
    nan_dest, big_dest = _listing(lists, [NAN_SRC]), _listing(lists, list(BIG_SRC))
    assert nan_dest.size and big_dest.size
    assert np.isnan(Y[nan_dest]).all(), where
    rest = np.ones(Y.shape[0], bool)
    rest[nan_dest] = False
    if mode == 0:
        assert not np.isfinite(Y[big_dest]).any(), where                   # +-inf, or NaN where the signs meet
        rest[big_dest] = False
    assert np.isfinite(Y[rest]).all(), where


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("transpose", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
def test_spmm_mode_equals_the_twin_on_rounded_rows(engine, pat, twins, mode, transpose, K):
    v, Xn, Xm = pat.data(K)
    where = f"spmm_mode mode={mode} transpose={transpose} K={K}"
    Y = dev_spmm(engine, pat.bw, pat, K, transpose, v, Xm if transpose else Xn, mode)
    assert_twin(Y, twins(mode, transpose, K), where)
    _check_special_rows(pat, transpose, mode, Y, where)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mode", (0, 1))
def test_backward_mode_equals_the_twin_on_rounded_rows(engine, pat, twins, mode, K):
    """dA = S_dP round(B), dB = S_dP^T round(A): each alone and both together"""
    dP, B, A = pat.data(K)
    for want_a, want_b in ((True, True), (True, False), (False, True)):
        dA, dB = dev_backward(engine, pat.bw, pat, K, dP, A, B, mode, want_a, want_b)
        where = f"backward_mode mode={mode} K={K} dA={want_a} dB={want_b}"
        assert (dA is None) == (not want_a) and (dB is None) == (not want_b)
        if want_a:
            assert_twin(dA, twins(mode, 0, K), where + ": dA")
        if want_b:
            assert_twin(dB, twins(mode, 1, K), where + ": dB")


@pytest.mark.parametrize("lanes", ("4", "8"))
def test_both_lane_layouts_equal_the_twin(engine, pat, twins, monkeypatch, lanes):
    """BSMR_GATHER16_LANES at create forces 4 or 8 elements per lane for every slice width: the same bits"""
    monkeypatch.setenv("BSMR_GATHER16_LANES", lanes)
    bw = engine.backward_create(pat.rows, pat.cols, pat.ro, pat.ci, device=0)
    try:
        for K in (32, 64, 128, 256):
            v, Xn, Xm = pat.data(K)
            for mode in (0, 1):
                dA, dB = dev_backward(engine, bw, pat, K, v, Xm, Xn, mode)
                assert_twin(dA, twins(mode, 0, K), f"lanes={lanes} mode={mode} K={K}: dA")
                assert_twin(dB, twins(mode, 1, K), f"lanes={lanes} mode={mode} K={K}: dB")
    finally:
        engine.backward_destroy(bw)


# ---- 2. equivalences on the device, bitwise ------------------------------------------------------------------------
EQ_KS = (96, 256)


@pytest.mark.parametrize("K", EQ_KS)
def test_f32_mode_is_the_fp32_call(engine, pat, twins, K):
    v, Xn, Xm = pat.data(K)
    F32 = engine.COMPUTE_F32
    for transpose, X in ((0, Xn), (1, Xm)):
        tv, tX, tY = _t(v), _t(X), _nan(pat.cols if transpose else pat.rows, K)
        assert engine.hip().bsmr_spmm_mode(pat.bw, K, transpose, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), 1, F32,
                                           _stream()) == engine.OK
        torch.cuda.synchronize()
        same_bits(tY.cpu().numpy(), dev_spmm(engine, pat.bw, pat, K, transpose, v, X, F32), f"spmm_mode(F32) K={K}")
        assert_twin(tY.cpu().numpy(), twins(2, transpose, K), f"spmm_mode(F32) K={K}")
    tdP, tA, tB = _t(v), _t(Xm), _t(Xn)
    tdA, tdB = _nan(pat.rows, K), _nan(pat.cols, K)
    assert engine.hip().bsmr_sddmm_backward_mode(pat.bw, K, tdP.data_ptr(), tA.data_ptr(), tB.data_ptr(), tdA.data_ptr(),
                                                 tdB.data_ptr(), 1, F32, _stream()) == engine.OK
    torch.cuda.synchronize()
    dA, dB = dev_backward(engine, pat.bw, pat, K, v, Xm, Xn, F32)
    same_bits(tdA.cpu().numpy(), dA, "backward_mode(F32): dA")
    same_bits(tdB.cpu().numpy(), dB, "backward_mode(F32): dB")


@pytest.mark.parametrize("K", EQ_KS)
@pytest.mark.parametrize("mode", (0, 1))
def test_mode_equals_fp32_on_rounded_rows_and_lowp(engine, oracle, pat, mode, K):
    """_mode(m) on X = bsmr_spmm on round(X) = bsmr_spmm_lowp on bsmr_convert_operands' copies = bsmr_spmm_lowp on the
    oracle's 16-bit words"""
    v, Xn, Xm = pat.data(K)
    csr = engine.CSR.from_arrays(pat.rows, pat.cols, pat.ro, pat.ci)
    pipe = engine.Pipeline(csr, alpha=0.3, delta=0.3, device=-1)
    st, plan = engine.plan_from_arrays(pat.rows, pat.cols, pat.nnz, pipe.arrays(), device=0)
    assert st == engine.OK
    try:
        tA, tB = _t(Xm), _t(Xn)
        tA16 = torch.zeros(pat.rows * K, dtype=torch.int16, device=_dev())
        tB16 = torch.zeros(pat.cols * K, dtype=torch.int16, device=_dev())
        engine.convert_operands(plan, K, tA.data_ptr(), tB.data_ptr(), tA16.data_ptr(), tB16.data_ptr(), mode, _stream())
        torch.cuda.synchronize()
        for transpose, X, t16 in ((0, Xn, tB16), (1, Xm, tA16)):
            where = f"mode={mode} transpose={transpose} K={K}"
            ref = dev_spmm(engine, pat.bw, pat, K, transpose, v, X, mode)
            rounded = dev_spmm(engine, pat.bw, pat, K, transpose, v, oracle.round_array(ROUND[mode], X), engine.COMPUTE_F32)
            assert_twin(ref, rounded, where + ": fp32 call on rounded rows")      # (NaN payloads may differ)
            same_bits(dev_lowp(engine, pat.bw, pat, K, transpose, v, t16, mode), ref, where + ": lowp on converted copies")
            words = bits16(oracle, mode, X)
            assert np.array_equal(t16.cpu().numpy().view(np.uint16)[~np.isnan(X.ravel())], words[~np.isnan(X.ravel())])
            assert_twin(dev_lowp(engine, pat.bw, pat, K, transpose, v, words, mode), ref, where + ": lowp on numpy words")
    finally:
        engine.plan_destroy(plan)


@pytest.mark.parametrize("mode", (0, 1))
def test_permute_row_order_and_batches(engine, pat, monkeypatch, mode):
    """BSMR_BACKWARD_PERMUTE=0, a shuffled row_order and a batch of 3 (odd nnz: batch 1 starts on an odd float) give
    the bits of the default handle's single calls"""
    K, nb = 64, 3
    assert pat.nnz % 2 == 1
    rng = np.random.default_rng(5 + mode)
    v = np.stack([_wide(rng, pat.nnz, -4, 4) for _ in range(nb)])
    Xn = np.stack([special_x(rng, pat.cols, K) for _ in range(nb)])
    Xm = np.stack([special_x(rng, pat.rows, K) for _ in range(nb)])
    single = [dev_backward(engine, pat.bw, pat, K, v[b], Xm[b], Xn[b], mode) for b in range(nb)]
    dA, dB = dev_backward(engine, pat.bw, pat, K, v, Xm, Xn, mode, nb=nb)
    Yr = dev_spmm(engine, pat.bw, pat, K, 0, v, Xn, mode, nb=nb)
    Yc = dev_spmm(engine, pat.bw, pat, K, 1, v, Xm, mode, nb=nb)
    for b in range(nb):
        same_bits(dA[b], single[b][0], f"batch {b}: dA")
        same_bits(dB[b], single[b][1], f"batch {b}: dB")
        same_bits(Yr[b], single[b][0], f"batch {b}: spmm rows")
        same_bits(Yc[b], single[b][1], f"batch {b}: spmm columns")
    monkeypatch.setenv("BSMR_BACKWARD_PERMUTE", "0")
    in_place = engine.backward_create(pat.rows, pat.cols, pat.ro, pat.ci, device=0)
    monkeypatch.delenv("BSMR_BACKWARD_PERMUTE")
    shuffled = engine.backward_create(pat.rows, pat.cols, pat.ro, pat.ci,
                                      row_order=np.random.default_rng(3).permutation(pat.rows), device=0)
    try:
        assert engine.backward_stats(in_place)["permute_values"] == 0 and engine.backward_stats(pat.bw)["permute_values"] == 1
        for name, bw in (("BSMR_BACKWARD_PERMUTE=0", in_place), ("shuffled row_order", shuffled)):
            gA, gB = dev_backward(engine, bw, pat, K, v[0], Xm[0], Xn[0], mode)
            same_bits(gA, single[0][0], name + ": dA")
            same_bits(gB, single[0][1], name + ": dB")
            same_bits(dev_spmm(engine, bw, pat, K, 1, v[0], Xm[0], mode), single[0][1], name + ": spmm columns")
    finally:
        engine.backward_destroy(in_place)
        engine.backward_destroy(shuffled)


# ---- 3. the error bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 1))
def test_error_bound_against_fp64(engine, oracle, pat, mode):
    """|Y - S_v X| <= (n + 2) u sum|v||x~| + u16 sum|v||x| against the fp64 product of the UNROUNDED operands, X inside
    the normal range of both formats"""
    import scipy.sparse as sp
    K = 128
    rng = np.random.default_rng(77 + mode)
    v = rng.uniform(-1, 1, pat.nnz).astype(np.float32)
    S = sp.csr_matrix((v.astype(np.float64), pat.ci.astype(np.int64), pat.ro.astype(np.int64)), shape=(pat.rows, pat.cols))
    for transpose, rows_x in ((0, pat.cols), (1, pat.rows)):
        X = (rng.choice([-1.0, 1.0], (rows_x, K)) * rng.uniform(2.0 ** -10, 4, (rows_x, K))).astype(np.float32)
        Y = dev_spmm(engine, pat.bw, pat, K, transpose, v, X, mode).astype(np.float64)
        T = S.T if transpose else S
        Xr = oracle.round_array(ROUND[mode], X).astype(np.float64)
        want = T @ X.astype(np.float64)
        n = np.diff(pat.lists(transpose)[0].astype(np.int64)).astype(np.float64)[:, None]
        bound = (n + 2) * U * (abs(T) @ np.abs(Xr)) + U16[mode] * (abs(T) @ np.abs(X.astype(np.float64)))
        err = np.abs(Y - want)
        print(f"mode={mode} transpose={transpose}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all()
        assert (Y[n[:, 0] == 0] == 0).all()


# ---- 4. exact placement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (32, 96, 256))
@pytest.mark.parametrize("mode", (0, 1))
def test_exact_placement(engine, pat, mode, K):
    """a one-hot v moves exactly one source row to exactly one destination.  X holds integers m 2^e <= 2040 with m <= 255:
    exact in fp16 (11 significant bits) and in bf16 (8), so the result is the integer product with ==."""
    rng = np.random.default_rng(K + mode)
    mk = lambda rows: (rng.integers(1, 256, (rows, K)) << rng.integers(0, 4, (rows, K))).astype(np.float32)
    Xn, Xm = mk(pat.cols), mk(pat.rows)
    assert Xn.max() <= 2048 and np.array_equal(Xn, Xn.astype(np.float16).astype(np.float32))
    row_of = np.repeat(np.arange(pat.rows), np.diff(pat.ro.astype(np.int64)))
    long_row = int(np.flatnonzero(np.diff(pat.ro.astype(np.int64)) == 1025)[0])
    picks = list(rng.choice(pat.nnz, 2, replace=False)) + [int(pat.ro[long_row]) + 600,          # inside a second chunk
                                                           int(np.flatnonzero(pat.ci == 3)[700])]  # ... of a column
    for e in picks:
        v = np.zeros(pat.nnz, np.float32)
        v[e] = 1.0
        r, c = row_of[e], pat.ci[e]
        Y = dev_spmm(engine, pat.bw, pat, K, 0, v, Xn, mode)
        assert np.array_equal(Y[r], Xn[c])
        Y[r] = 0
        assert np.all(Y == 0)
        Y = dev_spmm(engine, pat.bw, pat, K, 1, v, Xm, mode)
        assert np.array_equal(Y[c], Xm[r])
        Y[c] = 0
        assert np.all(Y == 0)


# ---- 5. graph capture after bsmr_backward_reserve_mode ---------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 1))
def test_graph_capture_after_reserve_mode(engine, pat, mode):
    K = 128
    dev = _dev()
    v, Xn, Xm = pat.data(K)
    tv, tA, tB = _t(v), _t(Xm), _t(Xn)
    tdA = torch.empty((pat.rows, K), dtype=torch.float32, device=dev)
    tdB = torch.empty((pat.cols, K), dtype=torch.float32, device=dev)
    bw = engine.backward_create(pat.rows, pat.cols, pat.ro, pat.ci, device=0)
    try:
        engine.backward_reserve(bw, K, 1)
        fp32_bytes = engine.backward_stats(bw)["workspace_bytes"]
        engine.backward_reserve(bw, K, 1, mode=mode)
        reserved = engine.backward_stats(bw)["workspace_bytes"]
        assert reserved >= fp32_bytes + (pat.rows + pat.cols) * K * 2             # room for both 16-bit copies
        side = torch.cuda.Stream(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            engine.sddmm_backward(bw, K, tv.data_ptr(), tA.data_ptr(), tB.data_ptr(), tdA.data_ptr(), tdB.data_ptr(), 1,
                                  side.cuda_stream, mode=mode)
            side.synchronize()
            want = (tdA.cpu().numpy().tobytes(), tdB.cpu().numpy().tobytes())
            with torch.cuda.graph(graph, stream=side):
                engine.sddmm_backward(bw, K, tv.data_ptr(), tA.data_ptr(), tB.data_ptr(), tdA.data_ptr(), tdB.data_ptr(),
                                      1, torch.cuda.current_stream(dev).cuda_stream, mode=mode)
        for _ in range(2):
            tdA.fill_(float("nan"))
            tdB.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert tdA.cpu().numpy().tobytes() == want[0] and tdB.cpu().numpy().tobytes() == want[1]
        assert engine.backward_stats(bw)["workspace_bytes"] == reserved
        del graph
    finally:
        torch.cuda.synchronize()
        engine.backward_destroy(bw)


# ---- 6. the rules --------------------------------------------------------------------------------------------------
def test_argument_rules(engine, pat):
    hip, bad = engine.hip(), engine.ERR_INVALID_ARG
    K, s = 64, _stream()
    t = torch.zeros(SIZE * K + pat.nnz + 64, dtype=torch.float32, device=_dev())
    p = t.data_ptr()
    assert p % 16 == 0
    for mode in (-1, 3, 7):
        assert hip.bsmr_spmm_mode(pat.bw, K, 0, p, p, p, 1, mode, s) == bad
        assert hip.bsmr_sddmm_backward_mode(pat.bw, K, p, p, p, p, p, 1, mode, s) == bad
        assert hip.bsmr_spmm_lowp(pat.bw, K, 0, p, p, p, 1, mode, s) == bad
        assert hip.bsmr_backward_reserve_mode(pat.bw, K, 1, mode) == bad
    assert hip.bsmr_spmm_lowp(pat.bw, K, 0, p, p, p, 1, engine.COMPUTE_F32, s) == bad
    for mode in (0, 1, 2):
        assert hip.bsmr_spmm_mode(pat.bw, 48, 0, p, p, p, 1, mode, s) == engine.ERR_UNSUPPORTED_K
        assert hip.bsmr_spmm_mode(pat.bw, 0, 0, p, p, p, 1, mode, s) == engine.ERR_UNSUPPORTED_K
        assert hip.bsmr_sddmm_backward_mode(pat.bw, 48, p, p, p, p, None, 1, mode, s) == engine.ERR_UNSUPPORTED_K
        assert hip.bsmr_backward_reserve_mode(pat.bw, 48, 1, mode) == engine.ERR_UNSUPPORTED_K
        assert hip.bsmr_spmm_mode(pat.bw, K, 2, p, p, p, 1, mode, s) == bad                      # transpose is 0 or 1
        assert hip.bsmr_spmm_mode(pat.bw, K, 0, p, p, p, 65536, mode, s) == bad
        assert hip.bsmr_spmm_mode(pat.bw, K, 0, p, p, p, 0, mode, s) == engine.OK                # no-op
        assert hip.bsmr_sddmm_backward_mode(pat.bw, K, p, p, p, p, p, 0, mode, s) == engine.OK
        for v, x, y in ((p + 2, p, p), (p, p + 4, p), (p, p, p + 8), (None, p, p), (p, None, p), (p, p, None)):
            assert hip.bsmr_spmm_mode(pat.bw, K, 0, v, x, y, 1, mode, s) == bad
        for dp, a, b, da, db in ((p + 2, p, p, p, p), (p, p + 4, p, p, p), (p, p, p + 4, p, p), (p, p, p, p + 4, p),
                                 (p, p, p, p, p + 4), (None, p, p, p, p), (p, None, p, None, p), (p, p, None, p, None)):
            assert hip.bsmr_sddmm_backward_mode(pat.bw, K, dp, a, b, da, db, 1, mode, s) == bad
    assert hip.bsmr_spmm_lowp(pat.bw, 48, 0, p, p, p, 1, 0, s) == engine.ERR_UNSUPPORTED_K
    for x16 in (p + 2, p + 4, p + 8, None):                                                     # X16_dev: 16 bytes
        assert hip.bsmr_spmm_lowp(pat.bw, K, 0, p, x16, p, 1, 1, s) == bad
    assert hip.bsmr_spmm_lowp(pat.bw, K, 0, p + 2, p, p, 1, 0, s) == bad
    assert hip.bsmr_spmm_lowp(pat.bw, K, 0, p, p, p + 4, 1, 0, s) == bad
    assert hip.bsmr_spmm_lowp(pat.bw, K, 0, p, p, p, 0, 0, s) == engine.OK
    torch.cuda.synchronize()
    assert not t.any()                                                                           # nothing ran


@pytest.mark.parametrize("nb", (1, 2))
def test_empty_pattern_with_null_operands(engine, nb):
    """nnz = 0: v / dP and the operands may be NULL, every output element is still written with +0"""
    M, N, K = 5, 7, 64
    bw = engine.backward_create(M, N, np.zeros(M + 1, np.uint32), np.zeros(0, np.uint32), device=0)
    hip, s = engine.hip(), _stream()
    try:
        for mode in (0, 1):
            for transpose, rows_y in ((0, M), (1, N)):
                for call in (hip.bsmr_spmm_mode, hip.bsmr_spmm_lowp):
                    Y = _nan(nb, rows_y, K)
                    assert call(bw, K, transpose, None, None, Y.data_ptr(), nb, mode, s) == engine.OK
                    torch.cuda.synchronize()
                    assert (Y.cpu().numpy().view(np.uint32) == 0).all()
            dA, dB = _nan(nb, M, K), _nan(nb, N, K)
            assert hip.bsmr_sddmm_backward_mode(bw, K, None, None, None, dA.data_ptr(), dB.data_ptr(), nb, mode, s) == engine.OK
            torch.cuda.synchronize()
            assert (dA.cpu().numpy().view(np.uint32) == 0).all() and (dB.cpu().numpy().view(np.uint32) == 0).all()
            assert hip.bsmr_spmm_mode(bw, K, 0, None, None, None, nb, mode, s) == engine.ERR_INVALID_ARG
            assert hip.bsmr_backward_reserve_mode(bw, K, nb, mode) == engine.OK
    finally:
        engine.backward_destroy(bw)


# ---- 7. extents ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (32, 256))
@pytest.mark.parametrize("mode", (0, 1))
def test_calls_stay_inside_the_buffers(engine, oracle, pat, mode, K):
    """the three compute entries, both directions, operands at the weakest accepted alignment (16 bytes for matrices and
    16-bit rows, 4 for values), two batches: guards and inputs intact, every output element written, the twin's bits -
    a read past the rows K 2 b bytes of X16 (or of X) would show in them"""
    nb = 2
    dev, s = _dev(), _stream()
    rng = np.random.default_rng(31 * K + mode)
    v = np.stack([_wide(rng, pat.nnz, -4, 4) for _ in range(nb)])
    Xn = np.stack([_wide(rng, (pat.cols, K), -8, 8) for _ in range(nb)])
    Xm = np.stack([_wide(rng, (pat.rows, K), -8, 8) for _ in range(nb)])
    twin = {t: np.stack([gather(oracle, pat.lists(t), v[b], oracle.round_array(ROUND[mode], X[b])) for b in range(nb)])
            for t, X in ((0, Xn), (1, Xm))}
    gv = Guarded.input("v", v, VALUES, K, dev)
    gXn, gXm = Guarded.input("Xn", Xn, OPERAND, K, dev), Guarded.input("Xm", Xm, OPERAND, K, dev)
    g16 = {0: Guarded.input("Xn16", bits16(oracle, mode, Xn), OPERAND, K, dev, dtype=np.uint16),
           1: Guarded.input("Xm16", bits16(oracle, mode, Xm), OPERAND, K, dev, dtype=np.uint16)}
    assert g16[0].nbytes == pat.cols * K * 2 * nb and g16[1].nbytes == pat.rows * K * 2 * nb
    for transpose, gX, rows in ((0, gXn, pat.rows), (1, gXm, pat.cols)):
        where = f"mode={mode} K={K} transpose={transpose}"
        gY = Guarded.output("Y", nb * rows * K, OPERAND, K, dev)
        engine.spmm(pat.bw, K, transpose, gv.ptr, gX.ptr, gY.ptr, nb, s, mode=mode)
        torch.cuda.synchronize()
        check_all(gv, gX, gY)
        assert_twin(gY.numpy().reshape(nb, rows, K), twin[transpose], where + ": spmm_mode")
        gY = Guarded.output("Y", nb * rows * K, OPERAND, K, dev)
        engine.spmm_lowp(pat.bw, K, transpose, gv.ptr, g16[transpose].ptr, gY.ptr, nb, s, mode=mode)
        torch.cuda.synchronize()
        check_all(gv, g16[transpose], gY)
        assert_twin(gY.numpy().reshape(nb, rows, K), twin[transpose], where + ": spmm_lowp")
    for want_a, want_b in ((True, True), (True, False), (False, True)):
        gdA = Guarded.output("dA", nb * pat.rows * K, OPERAND, K, dev) if want_a else None
        gdB = Guarded.output("dB", nb * pat.cols * K, OPERAND, K, dev) if want_b else None
        engine.sddmm_backward(pat.bw, K, gv.ptr, gXm.ptr, gXn.ptr, gdA.ptr if gdA else None, gdB.ptr if gdB else None, nb, s,
                              mode=mode)
        torch.cuda.synchronize()
        check_all(gv, gXm, gXn, gdA, gdB)
        if gdA:
            assert_twin(gdA.numpy().reshape(nb, pat.rows, K), twin[0], f"mode={mode} K={K} backward_mode: dA")
        if gdB:
            assert_twin(gdB.numpy().reshape(nb, pat.cols, K), twin[1], f"mode={mode} K={K} backward_mode: dB")
