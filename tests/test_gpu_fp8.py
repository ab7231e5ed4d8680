"""fp8 keys and values on the device: bsmr_widen_fp8, bsmr_sddmm_b8, bsmr_spmm_x8, bsmr_sparse_attention_x8
(include/bsmr_hip.h "fp8 keys and values").

The contract is one sentence - an fp8 call is, bit for bit, the 16-bit call on the exactly widened operand - so every
expectation here is one the project already has, applied to widen(X8), the widening being torch's CPU cast
uint8.view(fp8).to(float32):
  1. the code table: all 256 codes of both formats through bsmr_widen_fp8 in both modes, bits against torch (NaN by class);
  2. bsmr_spmm_x8 = oracle.round_array(mode, gather twin(v, widen(X8))) on the boundary pattern of tests/test_gpu_io16.py,
     and = bsmr_spmm_16 on the widened copy;
  3. bsmr_sparse_attention_x8 = bsmr_sparse_attention_16 on the widened V (O, m, s), which is the fp32 call rounded once,
     which stays inside attention_twin.check_forward's bound;
  4. bsmr_sddmm_b8 on integers in [-8, 8] (exact in e4m3, e5m2, fp16 and bf16): P is the exact dot product and equals
     bsmr_sddmm_16 on the widened B, also on plans whose fp32 road never allocates the 16-bit workspace;
  5. every array of every call inside a guarded buffer;  6. the argument rules on live handles."""
import numpy as np
import pytest

from attention_twin import check_forward
from gather_twin import assert_twin, gather
from guarded import OPERAND, VALUES, Guarded, check_all
from test_gpu_io16 import DT, EMPTY_COL, KS, NB, ROUND, Pattern, _wide, to16, widen_words, words
from test_gpu_numerics import DENSE_PATS, _build, assert_exact, model, patterns  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F8 = {0: torch.float8_e4m3fn, 1: torch.float8_e5m2}
COMBOS = [(mode, fmt) for mode in (0, 1) for fmt in (0, 1)]


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(_dev())             # (a copy: shared references are read-only)


def widen(fmt, codes):
    """uint8 array -> its exact fp32 values (torch's CPU cast: the OCP table)"""
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(F8[fmt]).to(torch.float32).numpy()


def widen16(mode, fmt, codes):
    """uint8 array -> CPU tensor of the mode's 16-bit dtype (exact)"""
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(F8[fmt]).to(torch.float32).to(DT[mode])


def finite_codes(rng, fmt, shape):
    """random bytes without the NaN and infinity codes: e4m3fn S.1111.111, e5m2 S.11111.xx"""
    c = rng.integers(0, 256, size=shape, dtype=np.uint8)
    special = (c & 0x7F) == 0x7F if fmt == 0 else (c & 0x7C) == 0x7C
    c[special] &= 0xBF                                                       # clears an exponent bit: a finite code
    assert np.isfinite(widen(fmt, c)).all()
    return c


def int_codes(fmt, ints):
    """integers in [-8, 8] as fp8 codes (exact in both formats)"""
    t = torch.from_numpy(np.ascontiguousarray(ints, dtype=np.float32)).to(F8[fmt])
    assert np.array_equal(t.to(torch.float32).numpy(), ints)
    return t.view(torch.uint8).numpy()


def small_ints(rng, *shape):
    return rng.integers(-8, 9, size=shape).astype(np.float32)


# ---- 1. the code table -------------------------------------------------------------------------------------------------
def _assert_widened(got_words, mode, fmt, codes, where):
    want = widen16(mode, fmt, codes)
    want_words = words(want)
    nan = torch.isnan(want).numpy()
    got_nan = np.isnan(widen_words(mode, got_words))
    assert np.array_equal(got_nan, nan), (where, "NaN codes", np.flatnonzero(got_nan != nan)[:8])
    bad = ~nan & (got_words != want_words)                                   # bits: the sign of zero is compared
    assert not bad.any(), (where, [(int(c), hex(int(g)), hex(int(w))) for c, g, w in
                                   zip(codes[bad][:8], got_words[bad][:8], want_words[bad][:8])])


def test_the_table_itself():
    """what the issue states about the formats, on the CPU reference used below"""
    c = np.arange(256, dtype=np.uint8)
    for fmt, nans, infs in ((0, 2, 0), (1, 6, 2)):
        f = widen(fmt, c)
        assert np.isnan(f).sum() == nans and np.isinf(f).sum() == infs
        assert np.signbit(f[0x80]) and f[0x80] == 0 and not np.signbit(f[0])
        for mode in (0, 1):                                                  # both 16-bit formats hold every code exactly
            back = widen16(mode, fmt, c).float().numpy()
            assert np.array_equal(back[~np.isnan(f)], f[~np.isnan(f)])


@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_widen_matches_the_code_table(engine, mode, fmt):
    """count 256; 256 * 5 + 16; a count that is no multiple of 16 (the last elements go one per thread)"""
    for count in (256, 256 * 5 + 16, 256 * 5 + 16 + 7, 5):
        codes = (np.arange(count) % 256).astype(np.uint8) if count >= 256 else np.array([0x80, 0x7F, 0x01, 0xFC, 0x7B], np.uint8)
        pad = -count % 4                                                     # (guarded payloads are whole words)
        g_in = Guarded.input("in8", np.concatenate([codes, np.zeros(pad, np.uint8)]), OPERAND, 32, _dev(), dtype=np.uint8)
        out = torch.full((count + 8,), -1, dtype=torch.int16, device=_dev())
        engine.widen_fp8(g_in.ptr, out.data_ptr(), count, mode, fmt, _stream())
        torch.cuda.synchronize()
        g_in.check()
        got = out.cpu().numpy().view(np.uint16)
        assert (got[count:] == 0xFFFF).all(), "written past count"
        _assert_widened(got[:count], mode, fmt, codes, f"mode={mode} fmt={fmt} count={count}")


def test_widen_strides_over_a_large_array(engine):
    """more groups of 16 than the grid has threads (4096 blocks x 256): the grid-stride loop takes a second step"""
    mode, fmt = 1, 0
    count = 4096 * 256 * 16 + 3 * 16 + 5
    rng = np.random.default_rng(8)
    codes = rng.integers(0, 256, size=count, dtype=np.uint8)
    src = torch.from_numpy(codes).to(_dev())
    out = torch.full((count + 8,), -1, dtype=torch.int16, device=_dev())
    engine.widen_fp8(src.data_ptr(), out.data_ptr(), count, mode, fmt, _stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert (got[count:] == 0xFFFF).all()
    _assert_widened(got[:count], mode, fmt, codes, "large")


# ---- 2. the SpMM twin --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pat(engine):
    p = Pattern(engine)
    yield p
    for bw in p.bw.values():
        engine.backward_destroy(bw)


@pytest.fixture(scope="module")
def values(pat):
    v = _wide(np.random.default_rng(77), (NB, pat.nnz), -3, 3)
    v.setflags(write=False)
    return v


def dev_spmm8(engine, bw, p, K, transpose, v, X8, mode, fmt, nb):
    """v (nb, nnz) fp32, X8 (nb, rows, K) uint8 -> the words of Y (nb, rows_y, K)"""
    tv, tX = _t(v[:nb]), _t(X8[:nb], np.uint8)
    tY = torch.full((nb, p.cols if transpose else p.rows, K), float("nan"), dtype=DT[mode], device=_dev())
    engine.spmm_x8(bw, K, transpose, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), nb, _stream(), mode=mode, fmt=fmt)
    torch.cuda.synchronize()
    return words(tY)


def dev_spmm16(engine, bw, p, K, transpose, v, X16, mode, nb):
    tv, tX = _t(v[:nb]), X16[:nb].contiguous().to(_dev())
    tY = torch.full((nb, p.cols if transpose else p.rows, K), float("nan"), dtype=DT[mode], device=_dev())
    engine.spmm_16(bw, K, transpose, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), nb, _stream(), mode=mode)
    torch.cuda.synchronize()
    return words(tY)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("fmt", (0, 1))
def test_spmm_x8_equals_the_rounded_twin(engine, oracle, pat, values, fmt, K):
    rng = np.random.default_rng(100 * K + fmt)
    bw = pat.bw[8]
    for transpose, rows in ((0, pat.cols), (1, pat.rows)):
        X8 = finite_codes(rng, fmt, (NB, rows, K))
        X = widen(fmt, X8)
        twin = np.stack([gather(oracle, pat.lists(transpose), values[b], X[b]) for b in range(NB)])
        empty = EMPTY_COL if transpose else pat.row_with[0]
        for mode in (0, 1):
            want = oracle.round_array(ROUND[mode], twin)
            for nb in (1, NB):
                where = f"spmm_x8 fmt={fmt} mode={mode} transpose={transpose} K={K} batches={nb}"
                w = dev_spmm8(engine, bw, pat, K, transpose, values, X8, mode, fmt, nb)
                assert_twin(widen_words(mode, w), want[:nb], where)
                assert not w[:, empty].any(), where + ": a destination without entries is +0"
                w16 = dev_spmm16(engine, bw, pat, K, transpose, values, widen16(mode, fmt, X8), mode, nb)
                assert w.tobytes() == w16.tobytes(), where + ": differs from bsmr_spmm_16 on the widened copy"


@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_spmm_x8_with_nan_and_infinity_rows(engine, oracle, pat, values, mode, fmt):
    """a source row of NaN codes (every NaN code of the format) and, for e5m2, rows of +inf and of -inf: each reaches
    the destinations that list it and no other, as in the twin"""
    K, bw = 128, pat.bw[8]
    rng = np.random.default_rng(300 + 2 * mode + fmt)
    X8 = finite_codes(rng, fmt, (1, pat.cols, K))
    nan_codes = np.array([0x7F, 0xFF] if fmt == 0 else [0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF], np.uint8)
    src = pat.ci[pat.ro[pat.row_with[5]]:pat.ro[pat.row_with[5] + 1]]        # the columns of the 5-entry row
    X8[0, src[0]] = np.resize(nan_codes, K)
    if fmt == 1:
        X8[0, src[1]], X8[0, src[2]] = 0x7C, 0xFC
    X = widen(fmt, X8)
    assert np.isnan(X[0, src[0]]).all() and (fmt == 0 or (X[0, src[1]] == np.inf).all() and (X[0, src[2]] == -np.inf).all())
    twin = gather(oracle, pat.lists(0), values[0], X[0])
    assert np.isnan(twin[pat.row_with[5]]).all() and np.isfinite(twin).any(axis=1).sum() > pat.rows // 2
    w = dev_spmm8(engine, bw, pat, K, 0, values, X8, mode, fmt, 1)
    assert_twin(widen_words(mode, w)[0], oracle.round_array(ROUND[mode], twin), f"mode={mode} fmt={fmt}")


class InPlacePattern:
    """M = N = 96 on two handles: one created under BSMR_BACKWARD_PERMUTE=0, whose transposed gather reads v through
    csc_to_csr (the MAP = true kernels; the C ABI takes transpose = 1 there, the torch operator does not), and one as by
    default.  Row 40 has 600 entries, 520 of them in column 7 - a CSR may name a column twice, every entry has its own
    value - so one list of either direction is cut into two chunks and the reduce runs; the other rows have 1 - 3."""

    def __init__(self, engine):
        rng = np.random.default_rng(5)
        self.engine, self.rows, self.cols = engine, 96, 96
        per_row = [np.sort(rng.choice(96, int(rng.integers(1, 4)), replace=False)) for _ in range(96)]
        per_row[40] = rng.permutation(np.concatenate([np.full(520, 7), rng.integers(0, 96, 80)]))
        self.ro = np.zeros(97, dtype=np.uint32)
        self.ro[1:] = np.cumsum([a.size for a in per_row])
        self.ci = np.concatenate(per_row).astype(np.uint32)
        self.nnz = int(self.ci.size)
        self.permuted = engine.backward_create(96, 96, self.ro, self.ci, device=0)
        with pytest.MonkeyPatch.context() as mp:                             # read at create
            mp.setenv("BSMR_BACKWARD_PERMUTE", "0")
            self.bw = engine.backward_create(96, 96, self.ro, self.ci, device=0)
        for bw, permute in ((self.bw, 0), (self.permuted, 1)):
            st = engine.backward_stats(bw)
            assert (st["permute_values"], st["split_rows"], st["split_cols"]) == (permute, 1, 1)
            assert st["max_row_length"] == 600 and st["chunk"] < st["max_col_length"] < 2 * st["chunk"]

    def close(self):
        self.engine.backward_destroy(self.bw)
        self.engine.backward_destroy(self.permuted)


@pytest.fixture(scope="module")
def in_place(engine):
    p = InPlacePattern(engine)
    yield p
    p.close()


@pytest.mark.parametrize("K", (32, 96, 256))
def test_spmm_x8_in_place_is_spmm_16_on_the_widened_rows(engine, in_place, K):
    """BSMR_BACKWARD_PERMUTE=0 with transpose = 1 is spmmGather8<.., MAP = true>: bit for bit bsmr_spmm_16 on the widened
    copy and the call on the permuting handle, over direct and split lists, one slice, three slices and the widest slice"""
    p, nb = in_place, 2
    rng = np.random.default_rng(900 + K)
    v = _wide(rng, (nb, p.nnz), -3, 3)
    for mode, fmt in COMBOS:
        X8 = finite_codes(rng, fmt, (nb, 96, K))
        for transpose in (1, 0):
            where = f"in place: fmt={fmt} mode={mode} transpose={transpose} K={K}"
            w = dev_spmm8(engine, p.bw, p, K, transpose, v, X8, mode, fmt, nb)
            w16 = dev_spmm16(engine, p.bw, p, K, transpose, v, widen16(mode, fmt, X8), mode, nb)
            assert w.any() and w.tobytes() == w16.tobytes(), where + ": differs from bsmr_spmm_16 on the widened copy"
            wp = dev_spmm8(engine, p.permuted, p, K, transpose, v, X8, mode, fmt, nb)
            assert w.tobytes() == wp.tobytes(), where + ": differs from the handle that permutes v"


# ---- 3. the fused attention --------------------------------------------------------------------------------------------
def dev_attention(engine, bw, p, Kv, scale, scores, V, nb, mode, fmt=None):
    """V: uint8 codes (fmt given), a 16-bit CPU tensor, or fp32 numpy (mode None) -> (O words or fp32, m, s) as numpy"""
    tp = _t(scores)
    out_dtype = torch.float32 if mode is None else DT[mode]
    tO = torch.full((nb, p.rows, Kv), float("nan"), dtype=out_dtype, device=_dev())
    tm = torch.full((nb, p.rows), float("nan"), device=_dev())
    ts = torch.full((nb, p.rows), float("nan"), device=_dev())
    if fmt is not None:
        tV = _t(V, np.uint8)
        engine.sparse_attention_x8(bw, Kv, scale, tp.data_ptr(), tV.data_ptr(), tO.data_ptr(), tm.data_ptr(), ts.data_ptr(),
                                   nb, _stream(), mode=mode, fmt=fmt)
    else:
        tV = _t(V) if mode is None else V.contiguous().to(_dev())
        engine.sparse_attention(bw, Kv, scale, tp.data_ptr(), tV.data_ptr(), tO.data_ptr(), tm.data_ptr(), ts.data_ptr(), nb,
                                _stream(), mode=engine.COMPUTE_F32 if mode is None else mode)
    torch.cuda.synchronize()
    return (tO.cpu().numpy() if mode is None else words(tO)), tm.cpu().numpy(), ts.cpu().numpy()


@pytest.mark.parametrize("Kv", (32, 128, 256))
@pytest.mark.parametrize("fmt", (0, 1))
def test_attention_x8_is_attention_16_on_the_widened_v(engine, pat, fmt, Kv):
    rng = np.random.default_rng(500 + 10 * Kv + fmt)
    bw, nb, scale = pat.bw[8], 2, 0.37
    scores = (rng.uniform(-8, 8, (nb, pat.nnz)) / scale).astype(np.float32)
    dead = pat.row_with[63]
    scores[0, pat.ro[dead]:pat.ro[dead + 1]] = -np.inf                       # a dead row; row_with[0] is the empty one
    V8 = finite_codes(rng, fmt, (nb, pat.cols, Kv))
    V = widen(fmt, V8)
    O32, m32, s32 = dev_attention(engine, bw, pat, Kv, scale, scores, V, nb, None)
    for b in range(nb):
        check_forward(pat.ro, pat.ci, scores[b], scale, V[b], O32[b], f"fmt={fmt} Kv={Kv} batch {b}")
    for mode in (0, 1):
        where = f"attention_x8 fmt={fmt} mode={mode} Kv={Kv}"
        O8, m8, s8 = dev_attention(engine, bw, pat, Kv, scale, scores, V8, nb, mode, fmt)
        O16, m16, s16 = dev_attention(engine, bw, pat, Kv, scale, scores, widen16(mode, fmt, V8), nb, mode)
        assert O8.tobytes() == O16.tobytes() and m8.tobytes() == m16.tobytes() and s8.tobytes() == s16.tobytes(), where
        assert np.array_equal(O8, words(to16(mode, O32))), where + ": not the fp32 call rounded once"
        assert m8.tobytes() == m32.tobytes() and s8.tobytes() == s32.tobytes(), where
        for r in (dead, pat.row_with[0]):
            assert not O8[0, r].any() and m8[0, r] == -np.inf and s8[0, r] == 0, (where, r)
        assert s8[1, dead] > 0 and np.isfinite(widen_words(mode, O8)).all()


# ---- 4. the forward is exact -------------------------------------------------------------------------------------------
def dev_sddmm(engine, plan, K, A16, B, nb, mode, fmt=None):
    """A16 (nb, M, K) 16-bit CPU tensor; B: uint8 codes (fmt given) or a 16-bit CPU tensor -> P (nb, nnz)"""
    tA = A16.contiguous().to(_dev())
    tP = torch.full((nb, plan.pat.nnz), float("nan"), dtype=torch.float32, device=_dev())
    if fmt is not None:
        tB = _t(B, np.uint8)
        engine.sddmm_b8(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), nb, mode, fmt, _stream())
    else:
        tB = B.contiguous().to(_dev())
        engine.sddmm_16(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), nb, mode, _stream())
    torch.cuda.synchronize()
    return tP.cpu().numpy()


# (path of test_gpu_numerics.PATHS, pattern, K): the dense, hybrid and residue-only patterns on the conversion-pass road,
# and two roads that never make 16-bit copies, so that bsmr_sddmm_b8 reserves the workspace from cold
FORWARD_CASES = [("stream-pass", p, (32, 128, 512)) for p in DENSE_PATS] + [
    ("residue-b-only", "rand-sparse", (32, 128, 512)),
    ("stream-cvt-in-kernel", "nips-hybrid", (32, 128)),
    ("gemm-fp32-16x16", "nips-dense", (128,))]


@pytest.mark.parametrize("name,pname,ks", FORWARD_CASES)
def test_sddmm_b8_is_exact_on_small_integers(engine, oracle, patterns, name, pname, ks):
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"{name} {pname}".encode()))
    pat = patterns[pname]
    every = np.ones(pat.nnz, dtype=bool)
    plan = _build(engine, pat, name)            # a fresh plan: the first call reserves from cold, later ones grow it
    try:
        for K in ks:
            A, B = small_ints(rng, NB, pat.rows, K), small_ints(rng, NB, pat.cols, K)
            want = [model(oracle, pat, K, A[b], B[b], 0, every) for b in range(NB)]
            assert max(np.abs(w).max() for w in want) <= 64 * K
            for mode, fmt in COMBOS:
                A16, B8 = to16(mode, A), int_codes(fmt, B)
                for nb in (1, NB):
                    where = f"{name} {pname} K={K} mode={mode} fmt={fmt} batches={nb}"
                    P = dev_sddmm(engine, plan, K, A16[:nb], B8[:nb], nb, mode, fmt)
                    for b in range(nb):
                        assert_exact(P[b], want[b], f"{where} batch {b}")
                    P16 = dev_sddmm(engine, plan, K, A16[:nb], widen16(mode, fmt, B8[:nb]), nb, mode)
                    assert P.tobytes() == P16.tobytes(), where + ": differs from bsmr_sddmm_16 on the widened B"
    finally:
        plan.close()


# ---- 5. the memory contract --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (32, 256))
@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_calls_stay_inside_the_buffers(engine, oracle, pat, patterns, mode, fmt, K):
    """fp8 and 16-bit arrays 16 bytes, value arrays 4 bytes past a 512-byte boundary, two batches: guards and inputs
    intact, every output word written, the expected bits"""
    nb, dev, s, bw = 2, _dev(), _stream(), pat.bw[8]
    rng = np.random.default_rng(57 * K + 2 * mode + fmt)
    v = _wide(rng, (nb, pat.nnz), -3, 3)
    gv = Guarded.input("v", v, VALUES, K, dev)
    X8 = {0: finite_codes(rng, fmt, (nb, pat.cols, K)), 1: finite_codes(rng, fmt, (nb, pat.rows, K))}
    g8 = {t: Guarded.input(f"X8[{t}]", X8[t], OPERAND, K, dev, dtype=np.uint8) for t in (0, 1)}
    assert g8[0].nbytes == pat.cols * K * nb
    # the widening pass
    gW = Guarded.output("widened", X8[0].size, OPERAND, K, dev, dtype=np.uint16)
    engine.widen_fp8(g8[0].ptr, gW.ptr, X8[0].size, mode, fmt, s)
    torch.cuda.synchronize()
    check_all(g8[0], gW)
    assert np.array_equal(gW.numpy(), words(widen16(mode, fmt, X8[0])).ravel())
    # the gather, both directions
    for transpose, rows in ((0, pat.rows), (1, pat.cols)):
        X = widen(fmt, X8[transpose])
        want = oracle.round_array(ROUND[mode], np.stack([gather(oracle, pat.lists(transpose), v[b], X[b]) for b in range(nb)]))
        gY = Guarded.output("Y16", nb * rows * K, OPERAND, K, dev, dtype=np.uint16)
        engine.spmm_x8(bw, K, transpose, gv.ptr, g8[transpose].ptr, gY.ptr, nb, s, mode=mode, fmt=fmt)
        torch.cuda.synchronize()
        check_all(gv, g8[transpose], gY)
        assert_twin(widen_words(mode, gY.numpy()).reshape(nb, rows, K), want, f"K={K} transpose={transpose}: spmm_x8")
    # the fused attention
    scale = 0.5
    scores = rng.uniform(-6, 6, (nb, pat.nnz)).astype(np.float32)
    gP = Guarded.input("P", scores, VALUES, K, dev)
    gO = Guarded.output("O16", nb * pat.rows * K, OPERAND, K, dev, dtype=np.uint16)
    gm, gs = Guarded.output("m", nb * pat.rows, VALUES, K, dev), Guarded.output("s", nb * pat.rows, VALUES, K, dev)
    engine.sparse_attention_x8(bw, K, scale, gP.ptr, g8[0].ptr, gO.ptr, gm.ptr, gs.ptr, nb, s, mode=mode, fmt=fmt)
    torch.cuda.synchronize()
    check_all(gP, g8[0], gO, gm, gs)
    O16, m16, s16 = dev_attention(engine, bw, pat, K, scale, scores, widen16(mode, fmt, X8[0]), nb, mode)
    assert gO.numpy().tobytes() == O16.tobytes() and gm.numpy().tobytes() == m16.tobytes() and gs.numpy().tobytes() == s16.tobytes()
    # the forward: a hybrid plan (dense kernel + residue) and an all-sparse one
    for pname, name in (("nips-hybrid", "stream-pass"), ("rand-sparse", "residue-b-only")):
        npat = patterns[pname]
        plan = _build(engine, npat, name)
        try:
            A, B = small_ints(rng, nb, npat.rows, K), small_ints(rng, nb, npat.cols, K)
            gA = Guarded.input("A16", words(to16(mode, A)), OPERAND, K, dev, dtype=np.uint16)
            gB = Guarded.input("B8", int_codes(fmt, B), OPERAND, K, dev, dtype=np.uint8)
            gOut = Guarded.output("P", nb * npat.nnz, VALUES, K, dev)
            engine.sddmm_b8(plan.plan, K, gA.ptr, gB.ptr, gOut.ptr, nb, mode, fmt, s)
            torch.cuda.synchronize()
            check_all(gA, gB, gOut)
            P = gOut.numpy().reshape(nb, npat.nnz)
            for b in range(nb):
                assert_exact(P[b], model(oracle, npat, K, A[b], B[b], mode, np.ones(npat.nnz, bool)),
                             f"{name} {pname} K={K} mode={mode} fmt={fmt} batch {b}")
        finally:
            plan.close()


# ---- 6. the rules ------------------------------------------------------------------------------------------------------
def test_argument_rules_on_live_handles(engine, pat, patterns):
    """handle, K, the two modes, the pointers, num_batches - and afterwards the scratch tensor every pointer aimed at is
    still zero: nothing ran"""
    hip, bad, ok, s = engine.hip(), engine.ERR_INVALID_ARG, engine.OK, _stream()
    K = 64
    plan = _build(engine, patterns["nips-hybrid"], "stream-pass")
    t = torch.zeros(1500 * K + 50000, dtype=torch.float32, device=_dev())
    p = t.data_ptr()
    assert p % 16 == 0
    bw = pat.bw[8]
    sddmm = lambda a=p, b=p, P=p, nb=1, mode=0, fmt=0, k=K: hip.bsmr_sddmm_b8(plan.plan, k, a, b, P, nb, mode, fmt, s)
    spmm = lambda v=p, x=p, y=p, nb=1, mode=0, fmt=0, k=K, tr=0: hip.bsmr_spmm_x8(bw, k, tr, v, x, y, nb, mode, fmt, s)
    attn = lambda P=p, v=p, o=p, m=p, ss=p, nb=1, mode=0, fmt=0, k=K, scale=1.0: hip.bsmr_sparse_attention_x8(
        bw, k, scale, P, v, o, m, ss, nb, mode, fmt, s)
    try:
        for call in (sddmm, spmm, attn):
            for k in (0, 48, 16):
                assert call(k=k) == engine.ERR_UNSUPPORTED_K
                assert call(k=k, mode=2, fmt=5) == engine.ERR_UNSUPPORTED_K                      # K before the modes
            for mode, fmt in ((2, 0), (3, 0), (-1, 1), (0, 2), (1, -1), (2, 2)):
                assert call(mode=mode, fmt=fmt) == bad
            for mode, fmt in COMBOS:
                assert call(nb=65536, mode=mode, fmt=fmt) == bad
                assert call(nb=0, mode=mode, fmt=fmt) == ok                                      # a no-op
        for mode, fmt in COMBOS:
            m = dict(mode=mode, fmt=fmt)
            for kw in (dict(a=p + 8), dict(b=p + 8), dict(P=p + 2), dict(a=None), dict(b=None), dict(P=None)):
                assert sddmm(**kw, **m) == bad, kw
            for kw in (dict(v=p + 2), dict(x=p + 8), dict(y=p + 8), dict(v=None), dict(x=None), dict(y=None), dict(tr=2)):
                assert spmm(**kw, **m) == bad, kw
            for kw in (dict(P=p + 2), dict(v=p + 8), dict(o=p + 8), dict(m=p + 2), dict(ss=p + 2), dict(P=None), dict(v=None),
                       dict(o=None), dict(m=None), dict(ss=None), dict(scale=float("nan")), dict(scale=float("inf"))):
                assert attn(**kw, **m) == bad, kw
            for src, dst in ((p + 8, p), (p, p + 8), (None, p), (p, None)):
                assert hip.bsmr_widen_fp8(src, dst, 256, mode, fmt, s) == bad
            assert hip.bsmr_widen_fp8(p + 8, None, 0, mode, fmt, s) == ok
        for mode, fmt in ((2, 0), (0, 2), (3, 1)):
            assert hip.bsmr_widen_fp8(p, p, 256, mode, fmt, s) == bad
        # the existing entry points keep refusing mode 3
        assert hip.bsmr_spmm_mode(bw, K, 0, p, p, p, 1, 3, s) == bad and hip.bsmr_spmm_16(bw, K, 0, p, p, p, 1, 3, s) == bad
        torch.cuda.synchronize()
        assert not t.any()                                                                       # nothing ran
    finally:
        plan.close()


def test_empty_pattern_reads_nothing(engine):
    """nnz = 0: the inputs may be NULL; the gather and the attention still write their zero outputs"""
    M, N, K, nb = 5, 7, 64, 2
    bw = engine.backward_create(M, N, np.zeros(M + 1, np.uint32), np.zeros(0, np.uint32), device=0)
    hip, s = engine.hip(), _stream()
    try:
        for mode, fmt in COMBOS:
            for transpose, rows_y in ((0, M), (1, N)):
                Y = torch.full((nb, rows_y, K), float("nan"), dtype=DT[mode], device=_dev())
                assert hip.bsmr_spmm_x8(bw, K, transpose, None, None, Y.data_ptr(), nb, mode, fmt, s) == engine.OK
                torch.cuda.synchronize()
                assert not words(Y).any()
            O = torch.full((nb, M, K), float("nan"), dtype=DT[mode], device=_dev())
            m, ss = torch.zeros(nb, M, device=_dev()), torch.ones(nb, M, device=_dev())
            assert hip.bsmr_sparse_attention_x8(bw, K, 1.0, None, None, O.data_ptr(), m.data_ptr(), ss.data_ptr(), nb, mode,
                                                fmt, s) == engine.OK
            torch.cuda.synchronize()
            assert not words(O).any() and (m == -np.inf).all() and not ss.any()
            assert hip.bsmr_spmm_x8(bw, K, 0, None, None, None, nb, mode, fmt, s) == engine.ERR_INVALID_ARG
    finally:
        engine.backward_destroy(bw)
