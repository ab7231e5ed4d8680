"""MX block scales on the fp8 operand, on the device: bsmr_widen_fp8_mx, bsmr_sddmm_b8_mx, bsmr_spmm_x8_mx,
bsmr_sparse_attention_x8_mx (include/bsmr_hip.h "MX block scales").

The contract: dq = widen(code) * 2^(E - 127) is one fp32 multiplication, made before anything else, and an _mx call is, bit
for bit, the fp32 call on dq with each output rounded once (the SDDMM: the 16-bit call on narrow(dq)).  The reference for dq
is torch on the CPU, codes.float() * scales.view(float8_e8m0fnu).float(); every other expectation is one the project already
has, applied to dq:
  1. the table: all 256 codes x 13 scale codes through bsmr_widen_fp8_mx, bits against narrow(dq) (NaN by class, zero by
     its sign), and a count past the grid;
  2. bsmr_spmm_x8_mx = oracle.round_array(mode, gather twin(v, dq)) on the boundary pattern of tests/test_gpu_io16.py, =
     bsmr_spmm on dq narrowed, = bsmr_spmm_16 on the 16-bit copy of dq where that copy is exact, = bsmr_spmm_x8 when every
     scale code is 127;  3. rows of NaN, overflow, subnormal and infinite elements;
  4. bsmr_sparse_attention_x8_mx = bsmr_sparse_attention on dq, O rounded once, m and s in bits;
  5. bsmr_sddmm_b8_mx on exact products;  6. guarded buffers, the scales at an odd address;  7. the rules; nnz = 0.
Every scale array holds different codes in neighbouring rows, blocks and batches, so a wrong block index changes bits."""
import numpy as np
import pytest

from attention_twin import check_forward
from gather_twin import assert_twin, gather
from guarded import OPERAND, VALUES, Guarded, check_all
from test_gpu_fp8 import (COMBOS, F8, dev_attention, dev_sddmm, dev_spmm8, dev_spmm16, finite_codes, in_place, int_codes,  # noqa: F401
                          small_ints)
from test_gpu_io16 import DT, EMPTY_COL, NB, ROUND, Pattern, _wide, to16, widen_words, words
from test_gpu_numerics import DENSE_PATS, _build, assert_exact, model, patterns  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = (32, 64, 96, 128, 384)      # one block per row; two blocks per slice; slice = block; two lanes per block; three slices
TABLE_SCALES = (0, 1, 2, 3, 10, 112, 126, 127, 128, 134, 253, 254, 255)


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(_dev())


def dq32(fmt, codes, scales):
    """the contract on the CPU: (..., K) uint8 codes, (..., K / 32) uint8 scale codes -> fp32, one multiplication"""
    c = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(F8[fmt]).to(torch.float32)
    s = torch.from_numpy(np.ascontiguousarray(scales, dtype=np.uint8)).view(torch.float8_e8m0fnu).to(torch.float32)
    return (c * s.repeat_interleave(32, dim=-1)).numpy()


def scale_codes(shape, lo=112, hi=134, salt=0):
    """codes in [lo, hi] that differ between neighbouring batches, rows and blocks (steps 5, 7, 3 modulo the range)"""
    idx = np.indices(shape)
    steps = (3, 7, 5)[:len(shape)][::-1]                                     # last axis (blocks) 3, rows 7, batches 5
    return (lo + (sum(int(k) * i for k, i in zip(steps, idx)) + salt) % (hi - lo + 1)).astype(np.uint8)


SUB = np.array([1.0, 1.25, 1.5, 1.75], np.float32)   # values of both formats below 2: times 2^-127 they are fp32 subnormals


def sub_codes(fmt):
    """a block of 32 codes with the values of SUB, eight times over"""
    t = torch.from_numpy(np.tile(SUB, 8)).to(F8[fmt])
    assert np.array_equal(t.float().numpy(), np.tile(SUB, 8))
    return t.view(torch.uint8).numpy()


def copy_is_exact(mode, x32):
    """whether the 16-bit copy of x32 holds every element exactly (NaN by class)"""
    back = to16(mode, x32).float().numpy()
    return bool(((back == x32) | (np.isnan(back) & np.isnan(x32))).all())


def _assert_words(got_words, mode, want32, where):
    """got equals narrow(want32): NaN by class, everything else in bits (so zero by its sign)"""
    want = to16(mode, want32)
    want_words = words(want)
    nan = torch.isnan(want).numpy()
    got_nan = np.isnan(widen_words(mode, got_words))
    assert np.array_equal(got_nan, nan), (where, "NaN", np.flatnonzero(got_nan != nan)[:8])
    bad = ~nan & (got_words != want_words)
    assert not bad.any(), (where, int(bad.sum()), [(int(i), hex(int(g)), hex(int(w))) for i, g, w in
                                                    zip(np.flatnonzero(bad)[:8], got_words[bad][:8], want_words[bad][:8])])


# ---- 1. the table ------------------------------------------------------------------------------------------------------
def test_the_reference_itself():
    """what the contract states about the scale codes and the multiplication, on the CPU reference used below"""
    one = {fmt: int_codes(fmt, np.ones(32, np.float32)) for fmt in (0, 1)}
    for fmt, top in ((0, 448.0), (1, 57344.0)):
        big = torch.full((32,), top).to(F8[fmt]).view(torch.uint8).numpy()
        assert (dq32(fmt, one[fmt], [0]) == np.float32(2.0 ** -127)).all()                 # a subnormal, kept
        assert (dq32(fmt, one[fmt], [254]) == np.float32(2.0 ** 127)).all()
        assert np.isnan(dq32(fmt, one[fmt], [255])).all()
        assert (dq32(fmt, big, [254]) == np.inf).all() and (dq32(fmt, big | 0x80, [254]) == -np.inf).all()
        z = dq32(fmt, np.full(32, 0x80, np.uint8), [3])
        assert (z == 0).all() and np.signbit(z).all()


@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_widen_mx_matches_the_table(engine, mode, fmt):
    """row i, block j: the codes 32 j .. 32 j + 31 under TABLE_SCALES[(i + j) % 13] - every code meets every scale code, and
    neighbouring blocks differ; the codes 16 bytes and the scales 1 byte past a word of a guarded buffer"""
    n = len(TABLE_SCALES)
    codes = np.tile(np.arange(256, dtype=np.uint8), (n, 1))
    scales = np.array([[TABLE_SCALES[(i + j) % n] for j in range(8)] for i in range(n)], np.uint8)
    want = dq32(fmt, codes, scales).ravel()
    count = codes.size
    g_in = Guarded.input("in8", codes, OPERAND, 32, _dev(), dtype=np.uint8)
    junk = np.concatenate([[0xAB], scales.ravel(), np.zeros(-(scales.size + 1) % 4, np.uint8)]).astype(np.uint8)
    g_sc = Guarded.input("scales", junk, VALUES, 32, _dev(), dtype=np.uint8)
    out = torch.full((count + 8,), -1, dtype=torch.int16, device=_dev())
    engine.widen_fp8_mx(g_in.ptr, g_sc.ptr + 1, out.data_ptr(), count, mode, fmt, _stream())
    torch.cuda.synchronize()
    check_all(g_in, g_sc)
    got = out.cpu().numpy().view(np.uint16)
    assert (got[count:] == 0xFFFF).all(), "written past count"
    _assert_words(got[:count], mode, want, f"mode={mode} fmt={fmt}")
    # scale code 127 everywhere: bsmr_widen_fp8
    ones = torch.full((n * 8,), 127, dtype=torch.uint8, device=_dev())
    plain = torch.full((count,), -1, dtype=torch.int16, device=_dev())
    engine.widen_fp8(g_in.ptr, plain.data_ptr(), count, mode, fmt, _stream())
    engine.widen_fp8_mx(g_in.ptr, ones.data_ptr(), out.data_ptr(), count, mode, fmt, _stream())
    torch.cuda.synchronize()
    assert torch.equal(out[:count], plain)


def test_widen_mx_strides_over_a_large_array(engine):
    """more groups of 16 than the grid has threads (4096 blocks x 256): the grid-stride loop takes a second step"""
    mode, fmt = 1, 0
    count = 4096 * 256 * 16 + 32
    rng = np.random.default_rng(8)
    codes = rng.integers(0, 256, size=count, dtype=np.uint8)
    scales = scale_codes((count // 32,), 100, 150)
    src, sc = torch.from_numpy(codes).to(_dev()), torch.from_numpy(scales).to(_dev())
    out = torch.full((count + 8,), -1, dtype=torch.int16, device=_dev())
    engine.widen_fp8_mx(src.data_ptr(), sc.data_ptr(), out.data_ptr(), count, mode, fmt, _stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert (got[count:] == 0xFFFF).all()
    _assert_words(got[:count], mode, dq32(fmt, codes, scales), "large")


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


def dev_spmm8_mx(engine, bw, p, K, transpose, v, X8, E8, mode, fmt, nb):
    """v (nb, nnz) fp32, X8 (nb, rows, K) uint8, E8 (nb, rows, K / 32) uint8 -> the words of Y (nb, rows_y, K)"""
    tv, tX, tE = _t(v[:nb]), _t(X8[:nb], np.uint8), _t(E8[:nb], np.uint8)
    tY = torch.full((nb, p.cols if transpose else p.rows, K), float("nan"), dtype=DT[mode], device=_dev())
    engine.spmm_x8_mx(bw, K, transpose, tv.data_ptr(), tX.data_ptr(), tE.data_ptr(), tY.data_ptr(), nb, _stream(),
                      mode=mode, fmt=fmt)
    torch.cuda.synchronize()
    return words(tY)


def dev_spmm32(engine, bw, p, K, transpose, v, X, nb):
    tv, tX = _t(v[:nb]), _t(X[:nb])
    tY = torch.full((nb, p.cols if transpose else p.rows, K), float("nan"), device=_dev())
    engine.spmm(bw, K, transpose, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), nb, _stream())
    torch.cuda.synchronize()
    return tY.cpu().numpy()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("fmt", (0, 1))
def test_spmm_x8_mx_equals_the_rounded_twin(engine, oracle, pat, values, fmt, K):
    rng = np.random.default_rng(100 * K + fmt)
    bw = pat.bw[8]
    for transpose, rows in ((0, pat.cols), (1, pat.rows)):
        X8 = finite_codes(rng, fmt, (NB, rows, K))
        E8 = scale_codes((NB, rows, K // 32), salt=K + transpose)
        X = dq32(fmt, X8, E8)
        assert np.isfinite(X).all()
        twin = np.stack([gather(oracle, pat.lists(transpose), values[b], X[b]) for b in range(NB)])
        Y32 = dev_spmm32(engine, bw, pat, K, transpose, values, X, NB)
        empty = EMPTY_COL if transpose else pat.row_with[0]
        ones = np.full_like(E8, 127)
        for mode in (0, 1):
            want = oracle.round_array(ROUND[mode], twin)
            # the ranges of include/bsmr_hip.h: codes 112 .. 134 are exact in bf16, in fp16 for e4m3 alone
            exact = copy_is_exact(mode, X)
            assert exact == (mode == 1 or fmt == 0)
            for nb in (1, NB):
                where = f"spmm_x8_mx fmt={fmt} mode={mode} transpose={transpose} K={K} batches={nb}"
                w = dev_spmm8_mx(engine, bw, pat, K, transpose, values, X8, E8, mode, fmt, nb)
                assert_twin(widen_words(mode, w), want[:nb], where)
                assert not w[:, empty].any(), where + ": a destination without entries is +0"
                assert w.tobytes() == words(to16(mode, Y32[:nb])).tobytes(), where + ": not bsmr_spmm on dq narrowed"
                if exact:
                    w16 = dev_spmm16(engine, bw, pat, K, transpose, values, to16(mode, X), mode, nb)
                    assert w.tobytes() == w16.tobytes(), where + ": differs from bsmr_spmm_16 on the dequantised copy"
                w1 = dev_spmm8_mx(engine, bw, pat, K, transpose, values, X8, ones, mode, fmt, nb)
                w8 = dev_spmm8(engine, bw, pat, K, transpose, values, X8, mode, fmt, nb)
                assert w1.tobytes() == w8.tobytes(), where + ": scale code 127 is not bsmr_spmm_x8"


@pytest.mark.parametrize("K", (32, 96, 256))
def test_spmm_x8_mx_in_place_is_spmm_on_dq(engine, in_place, K):
    """BSMR_BACKWARD_PERMUTE=0 with transpose = 1 is spmmGather8<.., MAP = true, .., MX = true>: bit for bit bsmr_spmm on dq
    narrowed, bsmr_spmm_16 on the 16-bit copy of dq where that copy is exact, and the call on the permuting handle"""
    p, nb = in_place, 2
    rng = np.random.default_rng(950 + K)
    v = _wide(rng, (nb, p.nnz), -3, 3)
    for mode, fmt in COMBOS:
        X8 = finite_codes(rng, fmt, (nb, 96, K))
        E8 = scale_codes((nb, 96, K // 32), salt=K + fmt)
        X = dq32(fmt, X8, E8)
        for transpose in (1, 0):
            where = f"in place: fmt={fmt} mode={mode} transpose={transpose} K={K}"
            w = dev_spmm8_mx(engine, p.bw, p, K, transpose, v, X8, E8, mode, fmt, nb)
            Y32 = dev_spmm32(engine, p.bw, p, K, transpose, v, X, nb)
            assert w.any() and w.tobytes() == words(to16(mode, Y32)).tobytes(), where + ": not bsmr_spmm on dq narrowed"
            if copy_is_exact(mode, X):
                w16 = dev_spmm16(engine, p.bw, p, K, transpose, v, to16(mode, X), mode, nb)
                assert w.tobytes() == w16.tobytes(), where + ": differs from bsmr_spmm_16 on the dequantised copy"
            wp = dev_spmm8_mx(engine, p.permuted, p, K, transpose, v, X8, E8, mode, fmt, nb)
            assert w.tobytes() == wp.tobytes(), where + ": differs from the handle that permutes v"


@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_spmm_x8_mx_with_non_finite_blocks(engine, oracle, pat, values, mode, fmt):
    """in the sources of the 5-entry row: a block under scale code 255 (NaN), a block of the largest code under 254
    (overflow: +inf), a block under scale code 0 (subnormal elements) and, for e5m2, blocks of +inf and -inf codes.  Each
    reaches the destinations that list it and no other, as in the twin"""
    K, bw = 128, pat.bw[8]
    rng = np.random.default_rng(300 + 2 * mode + fmt)
    X8 = finite_codes(rng, fmt, (1, pat.cols, K))
    E8 = scale_codes((1, pat.cols, K // 32), salt=11)
    src = pat.ci[pat.ro[pat.row_with[5]]:pat.ro[pat.row_with[5] + 1]]        # the columns of the 5-entry row
    top = int(torch.tensor([448.0 if fmt == 0 else 57344.0]).to(F8[fmt]).view(torch.uint8).item())
    E8[0, src[0], 1] = 255
    X8[0, src[1], 64:96], E8[0, src[1], 2] = top, 254
    X8[0, src[2], 96:128], E8[0, src[2], 3] = sub_codes(fmt), 0
    if fmt == 1:
        X8[0, src[3], 0:32], X8[0, src[4], 0:32] = 0x7C, 0xFC
    X = dq32(fmt, X8, E8)
    assert np.isnan(X[0, src[0], 32:64]).all() and (X[0, src[1], 64:96] == np.inf).all()
    sub = X[0, src[2], 96:128]
    assert (sub > 0).all() and (sub < np.float32(2.0 ** -126)).all()                       # subnormal, not flushed
    assert fmt == 0 or ((X[0, src[3], :32] == np.inf).all() and (X[0, src[4], :32] == -np.inf).all())
    twin = gather(oracle, pat.lists(0), values[0], X[0])
    r5 = twin[pat.row_with[5]]
    assert np.isnan(r5[32:64]).all() and np.isinf(r5[64:96]).all() and np.isfinite(r5[96:128]).all()
    assert fmt == 0 or not np.isfinite(r5[:32]).any()                                      # +-inf, or NaN where they meet
    assert np.isfinite(twin).any(axis=1).sum() > pat.rows // 2
    w = dev_spmm8_mx(engine, bw, pat, K, 0, values, X8, E8, mode, fmt, 1)
    assert_twin(widen_words(mode, w)[0], oracle.round_array(ROUND[mode], twin), f"mode={mode} fmt={fmt}")
    Y32 = dev_spmm32(engine, bw, pat, K, 0, values, X, 1)
    assert_twin(Y32[0], twin, f"fp32 gather, fmt={fmt}")


def test_subnormal_elements_are_not_flushed(engine, oracle):
    """one destination, one source, weight 2^20: X = code 2^-127 is subnormal, the product is normal.  A kernel that flushed
    the dequantised element would give 0"""
    M, N, K = 1, 1, 32
    bw = engine.backward_create(M, N, np.array([0, 1], np.uint32), np.zeros(1, np.uint32), device=0)
    try:
        for mode, fmt in COMBOS:
            X8 = sub_codes(fmt).reshape(1, 1, K)
            E8 = np.zeros((1, 1, 1), np.uint8)
            v = np.full((1, 1), 2.0 ** 20, np.float32)
            want = (dq32(fmt, X8, E8) * np.float32(2.0 ** 20))[0]
            assert (want == np.tile(SUB, 8) * np.float32(2.0 ** -107)).all()
            tY = torch.full((1, 1, K), float("nan"), dtype=DT[mode], device=_dev())
            tv, tX, tE = _t(v), _t(X8, np.uint8), _t(E8, np.uint8)
            engine.spmm_x8_mx(bw, K, False, tv.data_ptr(), tX.data_ptr(), tE.data_ptr(), tY.data_ptr(), 1, _stream(),
                              mode=mode, fmt=fmt)
            torch.cuda.synchronize()
            assert words(tY).tobytes() == words(to16(mode, want)).tobytes(), (mode, fmt)
            assert mode == 0 or (widen_words(mode, words(tY)) == want).all()               # bf16 holds them exactly
    finally:
        engine.backward_destroy(bw)


# ---- 4. the fused attention --------------------------------------------------------------------------------------------
def dev_attention_mx(engine, bw, p, Kv, scale, scores, V8, E8, nb, mode, fmt):
    tp, tV, tE = _t(scores), _t(V8, np.uint8), _t(E8, np.uint8)
    tO = torch.full((nb, p.rows, Kv), float("nan"), dtype=DT[mode], device=_dev())
    tm = torch.full((nb, p.rows), float("nan"), device=_dev())
    ts = torch.full((nb, p.rows), float("nan"), device=_dev())
    engine.sparse_attention_x8_mx(bw, Kv, scale, tp.data_ptr(), tV.data_ptr(), tE.data_ptr(), tO.data_ptr(), tm.data_ptr(),
                                  ts.data_ptr(), nb, _stream(), mode=mode, fmt=fmt)
    torch.cuda.synchronize()
    return words(tO), tm.cpu().numpy(), ts.cpu().numpy()


@pytest.mark.parametrize("Kv", (32, 128))
@pytest.mark.parametrize("fmt", (0, 1))
def test_attention_x8_mx_is_the_fp32_attention_on_dq(engine, pat, fmt, Kv):
    rng = np.random.default_rng(500 + 10 * Kv + fmt)
    bw, nb, scale = pat.bw[8], 2, 0.37
    scores = (rng.uniform(-8, 8, (nb, pat.nnz)) / scale).astype(np.float32)
    dead = pat.row_with[63]
    scores[0, pat.ro[dead]:pat.ro[dead + 1]] = -np.inf                       # a dead row; row_with[0] is the empty one
    V8 = finite_codes(rng, fmt, (nb, pat.cols, Kv))
    E8 = scale_codes((nb, pat.cols, Kv // 32), salt=Kv)
    V = dq32(fmt, V8, E8)
    O32, m32, s32 = dev_attention(engine, bw, pat, Kv, scale, scores, V, nb, None)
    for b in range(nb):
        check_forward(pat.ro, pat.ci, scores[b], scale, V[b], O32[b], f"fmt={fmt} Kv={Kv} batch {b}")
    for mode in (0, 1):
        where = f"attention_x8_mx fmt={fmt} mode={mode} Kv={Kv}"
        O8, m8, s8 = dev_attention_mx(engine, bw, pat, Kv, scale, scores, V8, E8, nb, mode, fmt)
        assert np.array_equal(O8, words(to16(mode, O32))), where + ": not the fp32 call rounded once"
        assert m8.tobytes() == m32.tobytes() and s8.tobytes() == s32.tobytes(), where
        for r in (dead, pat.row_with[0]):
            assert not O8[0, r].any() and m8[0, r] == -np.inf and s8[0, r] == 0, (where, r)
        assert s8[1, dead] > 0
        O1, m1, s1 = dev_attention_mx(engine, bw, pat, Kv, scale, scores, V8, np.full_like(E8, 127), nb, mode, fmt)
        Ox, mx, sx = dev_attention(engine, bw, pat, Kv, scale, scores, V8, nb, mode, fmt)
        assert O1.tobytes() == Ox.tobytes() and m1.tobytes() == mx.tobytes() and s1.tobytes() == sx.tobytes(), \
            where + ": scale code 127 is not bsmr_sparse_attention_x8"


# ---- 5. the forward is exact -------------------------------------------------------------------------------------------
def dev_sddmm_mx(engine, plan, K, A16, B8, E8, nb, mode, fmt):
    tA, tB, tE = A16.contiguous().to(_dev()), _t(B8, np.uint8), _t(E8, np.uint8)
    tP = torch.full((nb, plan.pat.nnz), float("nan"), dtype=torch.float32, device=_dev())
    engine.sddmm_b8_mx(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tE.data_ptr(), tP.data_ptr(), nb, mode, fmt, _stream())
    torch.cuda.synchronize()
    return tP.cpu().numpy()


# the dense, hybrid and residue-only patterns on the conversion-pass road, and a road whose fp32 form never allocates the
# 16-bit workspace, so that bsmr_sddmm_b8_mx reserves it from cold
FORWARD_CASES = [("stream-pass", p, (32, 128)) for p in DENSE_PATS] + [
    ("residue-b-only", "rand-sparse", (32, 128)),
    ("stream-cvt-in-kernel", "nips-hybrid", (32, 128))]


@pytest.mark.parametrize("name,pname,ks", FORWARD_CASES)
def test_sddmm_b8_mx_is_exact_on_scaled_integers(engine, oracle, patterns, name, pname, ks):
    """integers in [-8, 8] under block scales 2^s, s in [-2, 3]: multiples of 1/4 up to 64, exact in e4m3, e5m2, fp16 and
    bf16; the products and their sums (below 8 * 64 * K) are exact in fp32"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"mx {name} {pname}".encode()))
    pat = patterns[pname]
    every = np.ones(pat.nnz, dtype=bool)
    plan = _build(engine, pat, name)
    try:
        for K in ks:
            A, B = small_ints(rng, NB, pat.rows, K), small_ints(rng, NB, pat.cols, K)
            E8 = scale_codes((NB, pat.cols, K // 32), 125, 130, salt=K)
            for mode, fmt in COMBOS:
                A16, B8 = to16(mode, A), int_codes(fmt, B)
                Bdq = dq32(fmt, B8, E8)
                assert copy_is_exact(mode, Bdq) and np.abs(Bdq).max() <= 64
                want = [model(oracle, pat, K, A[b], Bdq[b], 0, ~every) for b in range(NB)]
                for nb in (1, NB):
                    where = f"{name} {pname} K={K} mode={mode} fmt={fmt} batches={nb}"
                    P = dev_sddmm_mx(engine, plan, K, A16[:nb], B8[:nb], E8[:nb], nb, mode, fmt)
                    for b in range(nb):
                        assert_exact(P[b], want[b], f"{where} batch {b}")
                    P16 = dev_sddmm(engine, plan, K, A16[:nb], to16(mode, Bdq[:nb]), nb, mode)
                    assert P.tobytes() == P16.tobytes(), where + ": differs from bsmr_sddmm_16 on narrow(dq(B))"
    finally:
        plan.close()


# ---- 6. the memory contract --------------------------------------------------------------------------------------------
def _guarded_scales(name, E8, K, dev):
    """the scale bytes one byte into a guarded payload: an odd address, a byte in front and the padding behind it that
    must stay as they are; returns (buffer, pointer to the scales)"""
    raw = np.concatenate([[0xAB], E8.ravel(), np.full(-(E8.size + 1) % 4, 0xCD, np.uint8)]).astype(np.uint8)
    g = Guarded.input(name, raw, VALUES, K, dev, dtype=np.uint8)
    return g, g.ptr + 1


@pytest.mark.parametrize("K", (32, 256))
@pytest.mark.parametrize("mode,fmt", COMBOS)
def test_mx_calls_stay_inside_the_buffers(engine, oracle, pat, patterns, mode, fmt, K):
    """fp8 and 16-bit arrays 16 bytes, value arrays 4 bytes past a 512-byte boundary, the scales at an odd address, two
    batches: guards and inputs intact, every output word written, the expected bits"""
    nb, dev, s, bw = 2, _dev(), _stream(), pat.bw[8]
    rng = np.random.default_rng(57 * K + 2 * mode + fmt)
    v = _wide(rng, (nb, pat.nnz), -3, 3)
    gv = Guarded.input("v", v, VALUES, K, dev)
    X8 = {0: finite_codes(rng, fmt, (nb, pat.cols, K)), 1: finite_codes(rng, fmt, (nb, pat.rows, K))}
    E8 = {t: scale_codes((nb, X8[t].shape[1], K // 32), salt=t) for t in (0, 1)}
    g8 = {t: Guarded.input(f"X8[{t}]", X8[t], OPERAND, K, dev, dtype=np.uint8) for t in (0, 1)}
    gE = {t: _guarded_scales(f"E8[{t}]", E8[t], K, dev) for t in (0, 1)}
    X = {t: dq32(fmt, X8[t], E8[t]) for t in (0, 1)}
    # the dequantising pass
    gW = Guarded.output("widened", X8[0].size, OPERAND, K, dev, dtype=np.uint16)
    engine.widen_fp8_mx(g8[0].ptr, gE[0][1], gW.ptr, X8[0].size, mode, fmt, s)
    torch.cuda.synchronize()
    check_all(g8[0], gE[0][0], gW)
    _assert_words(gW.numpy(), mode, X[0].ravel(), "widen_fp8_mx")
    # the gather, both directions
    for transpose, rows in ((0, pat.rows), (1, pat.cols)):
        want = oracle.round_array(ROUND[mode], np.stack([gather(oracle, pat.lists(transpose), v[b], X[transpose][b])
                                                         for b in range(nb)]))
        gY = Guarded.output("Y16", nb * rows * K, OPERAND, K, dev, dtype=np.uint16)
        engine.spmm_x8_mx(bw, K, transpose, gv.ptr, g8[transpose].ptr, gE[transpose][1], gY.ptr, nb, s, mode=mode, fmt=fmt)
        torch.cuda.synchronize()
        check_all(gv, g8[transpose], gE[transpose][0], gY)
        assert_twin(widen_words(mode, gY.numpy()).reshape(nb, rows, K), want, f"K={K} transpose={transpose}: spmm_x8_mx")
    # the fused attention
    scale = 0.5
    scores = rng.uniform(-6, 6, (nb, pat.nnz)).astype(np.float32)
    gP = Guarded.input("P", scores, VALUES, K, dev)
    gO = Guarded.output("O16", nb * pat.rows * K, OPERAND, K, dev, dtype=np.uint16)
    gm, gs = Guarded.output("m", nb * pat.rows, VALUES, K, dev), Guarded.output("s", nb * pat.rows, VALUES, K, dev)
    engine.sparse_attention_x8_mx(bw, K, scale, gP.ptr, g8[0].ptr, gE[0][1], gO.ptr, gm.ptr, gs.ptr, nb, s, mode=mode, fmt=fmt)
    torch.cuda.synchronize()
    check_all(gP, g8[0], gE[0][0], gO, gm, gs)
    O32, m32, s32 = dev_attention(engine, bw, pat, K, scale, scores, X[0], nb, None)
    assert gO.numpy().tobytes() == words(to16(mode, O32)).tobytes()
    assert gm.numpy().tobytes() == m32.tobytes() and gs.numpy().tobytes() == s32.tobytes()
    # the forward: a hybrid plan (dense kernel + residue) and an all-sparse one
    for pname, name in (("nips-hybrid", "stream-pass"), ("rand-sparse", "residue-b-only")):
        npat = patterns[pname]
        plan = _build(engine, npat, name)
        try:
            A, B = small_ints(rng, nb, npat.rows, K), small_ints(rng, nb, npat.cols, K)
            Es = scale_codes((nb, npat.cols, K // 32), 125, 130)
            B8 = int_codes(fmt, B)
            gA = Guarded.input("A16", words(to16(mode, A)), OPERAND, K, dev, dtype=np.uint16)
            gB = Guarded.input("B8", B8, OPERAND, K, dev, dtype=np.uint8)
            gBs, pBs = _guarded_scales("Bs", Es, K, dev)
            gOut = Guarded.output("P", nb * npat.nnz, VALUES, K, dev)
            engine.sddmm_b8_mx(plan.plan, K, gA.ptr, gB.ptr, pBs, gOut.ptr, nb, mode, fmt, s)
            torch.cuda.synchronize()
            check_all(gA, gB, gBs, gOut)
            P, Bdq = gOut.numpy().reshape(nb, npat.nnz), dq32(fmt, B8, Es)
            for b in range(nb):
                assert_exact(P[b], model(oracle, npat, K, A[b], Bdq[b], 0, np.zeros(npat.nnz, bool)),
                             f"{name} {pname} K={K} mode={mode} fmt={fmt} batch {b}")
        finally:
            plan.close()


# ---- 7. the rules ------------------------------------------------------------------------------------------------------
def test_argument_rules_on_live_handles(engine, pat, patterns):
    """handle, K, the two modes, the pointers (the scales among them, at any alignment), num_batches - and afterwards the
    scratch tensor every pointer aimed at is still zero: nothing ran"""
    hip, bad, ok, s = engine.hip(), engine.ERR_INVALID_ARG, engine.OK, _stream()
    K = 64
    plan = _build(engine, patterns["nips-hybrid"], "stream-pass")
    t = torch.zeros(1500 * K + 50000, dtype=torch.float32, device=_dev())
    p = t.data_ptr()
    assert p % 16 == 0
    bw = pat.bw[8]
    sddmm = lambda a=p, b=p, e=p + 1, P=p, nb=1, mode=0, fmt=0, k=K: hip.bsmr_sddmm_b8_mx(plan.plan, k, a, b, e, P, nb, mode,
                                                                                           fmt, s)
    spmm = lambda v=p, x=p, e=p + 1, y=p, nb=1, mode=0, fmt=0, k=K, tr=0: hip.bsmr_spmm_x8_mx(bw, k, tr, v, x, e, y, nb, mode,
                                                                                              fmt, s)
    attn = lambda P=p, v=p, e=p + 1, o=p, m=p, ss=p, nb=1, mode=0, fmt=0, k=K, scale=1.0: hip.bsmr_sparse_attention_x8_mx(
        bw, k, scale, P, v, e, o, m, ss, nb, mode, fmt, s)
    try:
        for call in (sddmm, spmm, attn):
            for k in (0, 48, 16):
                assert call(k=k) == engine.ERR_UNSUPPORTED_K
                assert call(k=k, mode=2, fmt=5) == engine.ERR_UNSUPPORTED_K                      # K before the modes
            for mode, fmt in ((2, 0), (3, 0), (-1, 1), (0, 2), (1, -1), (2, 2)):
                assert call(mode=mode, fmt=fmt) == bad
                assert call(mode=mode, fmt=fmt, e=None) == bad
            for mode, fmt in COMBOS:
                assert call(nb=65536, mode=mode, fmt=fmt) == bad
                assert call(nb=0, mode=mode, fmt=fmt) == ok                                      # a no-op
                assert call(e=None, mode=mode, fmt=fmt) == bad                                   # the scales are an input
        for mode, fmt in COMBOS:
            m = dict(mode=mode, fmt=fmt)
            for kw in (dict(a=p + 8), dict(b=p + 8), dict(P=p + 2), dict(a=None), dict(b=None), dict(P=None)):
                assert sddmm(**kw, **m) == bad, kw
            for kw in (dict(v=p + 2), dict(x=p + 8), dict(y=p + 8), dict(v=None), dict(x=None), dict(y=None), dict(tr=2)):
                assert spmm(**kw, **m) == bad, kw
            for kw in (dict(P=p + 2), dict(v=p + 8), dict(o=p + 8), dict(m=p + 2), dict(ss=p + 2), dict(P=None), dict(v=None),
                       dict(o=None), dict(m=None), dict(ss=None), dict(scale=float("nan")), dict(scale=float("inf"))):
                assert attn(**kw, **m) == bad, kw
            for src, sc, dst in ((p + 8, p, p), (p, p, p + 8), (None, p, p), (p, None, p), (p, p, None)):
                assert hip.bsmr_widen_fp8_mx(src, sc, dst, 256, mode, fmt, s) == bad
            assert hip.bsmr_widen_fp8_mx(p, p + 3, p, 48, mode, fmt, s) == bad                    # count % 32
            assert hip.bsmr_widen_fp8_mx(p + 8, None, None, 0, mode, fmt, s) == ok
        for mode, fmt in ((2, 0), (0, 2), (3, 1)):
            assert hip.bsmr_widen_fp8_mx(p, p, p, 256, mode, fmt, s) == bad
        torch.cuda.synchronize()
        assert not t.any()                                                                       # nothing ran
    finally:
        plan.close()


def test_empty_pattern_reads_nothing(engine):
    """nnz = 0: the inputs, the scales among them, may be NULL; the gather and the attention still write their zero
    outputs"""
    M, N, K, nb = 5, 7, 64, 2
    bw = engine.backward_create(M, N, np.zeros(M + 1, np.uint32), np.zeros(0, np.uint32), device=0)
    hip, s = engine.hip(), _stream()
    try:
        for mode, fmt in COMBOS:
            for transpose, rows_y in ((0, M), (1, N)):
                Y = torch.full((nb, rows_y, K), float("nan"), dtype=DT[mode], device=_dev())
                assert hip.bsmr_spmm_x8_mx(bw, K, transpose, None, None, None, Y.data_ptr(), nb, mode, fmt, s) == engine.OK
                torch.cuda.synchronize()
                assert not words(Y).any()
            O = torch.full((nb, M, K), float("nan"), dtype=DT[mode], device=_dev())
            m, ss = torch.zeros(nb, M, device=_dev()), torch.ones(nb, M, device=_dev())
            assert hip.bsmr_sparse_attention_x8_mx(bw, K, 1.0, None, None, None, O.data_ptr(), m.data_ptr(), ss.data_ptr(), nb,
                                                   mode, fmt, s) == engine.OK
            torch.cuda.synchronize()
            assert not words(O).any() and (m == -np.inf).all() and not ss.any()
            assert hip.bsmr_spmm_x8_mx(bw, K, 0, None, None, None, None, nb, mode, fmt, s) == engine.ERR_INVALID_ARG
    finally:
        engine.backward_destroy(bw)
