"""MXFP4 keys and values on the device: bsmr_widen_fp4_mx, bsmr_sddmm_b4_mx, bsmr_spmm_x4_mx, bsmr_sparse_attention_x4_mx
(include/bsmr_hip.h "MXFP4 keys and values").

The contract: dq = widen(code) * 2^(E - 127) is one fp32 multiplication - exact for every e2m1 code and every scale code up
to 254 - made before anything else, and a call is, bit for bit, the fp32 call on dq with each output rounded once (the
SDDMM: the 16-bit call on narrow(dq)).  The reference for dq is built here from the format's definition (the eight
magnitudes, low nibble first, 2^(e-127) by ldexp in fp64, one cast to fp32); every other expectation is one the project
already has, applied to dq.  A second, independent pin: every e2m1 value is an e4m3 value, so each call equals the MXFP8
call on the re-encoded codes with the same scales.
  1. the table: all 256 bytes x all 256 scale codes x both modes through bsmr_widen_fp4_mx, bits against narrow(dq) (NaN by
     class, zero by its sign), the scales at an odd address; and a count past the grid;
  2. bsmr_spmm_x4_mx = oracle.round_array(mode, gather twin(v, dq)) on the boundary pattern of tests/test_gpu_io16.py, =
     bsmr_spmm on dq narrowed, = bsmr_spmm_16 on the 16-bit copy of dq, = bsmr_spmm_x8_mx on the e4m3 re-encoding;
  3. planted blocks: scale code 255, the value 6 under 253 and 254, scale code 0 under a weight of 2^20, -0 codes;
  4. bsmr_sparse_attention_x4_mx = bsmr_sparse_attention on dq, O rounded once, m and s in bits;
  5. bsmr_sddmm_b4_mx on exact products;  6. guarded buffers, the scales at an odd address;  7. the rules; nnz = 0.
Every scale array holds different codes in neighbouring rows, blocks and batches, so a wrong block index changes bits."""
import math

import numpy as np
import pytest

from attention_twin import check_forward
from gather_twin import assert_twin, gather
from guarded import OPERAND, VALUES, Guarded, check_all
from test_gpu_fp8 import dev_attention, dev_sddmm, dev_spmm16, in_place, small_ints  # noqa: F401 (fixture)
from test_gpu_fp8_mx import (_assert_words, _guarded_scales, copy_is_exact, dev_attention_mx, dev_sddmm_mx, dev_spmm8_mx,
                             dev_spmm32, scale_codes)
from test_gpu_io16 import DT, EMPTY_COL, NB, ROUND, Pattern, _wide, to16, widen_words, words
from test_gpu_numerics import DENSE_PATS, _build, assert_exact, model, patterns  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = (32, 64, 96, 128, 384)      # the four lane layouts (W = 32, 64, 32 x 3, 128) and three slices of 128
MAG = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])                     # OCP e2m1, magnitude codes 0 .. 7
VALUE = np.concatenate([MAG, -MAG])                                          # nibble -> value; nibble 8 is -0
SCALE = np.array([math.ldexp(1.0, e - 127) for e in range(255)] + [math.nan])
E4M3 = 0                                                                     # BSMR_FP8_E4M3


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(_dev())


def pack4(nib):
    """(..., K) nibbles -> (..., K / 2) bytes: element 2i the low nibble of byte i"""
    nib = np.asarray(nib, np.uint8)
    return (nib[..., 0::2] | (nib[..., 1::2] << 4)).astype(np.uint8)


def unpack4(packed):
    packed = np.asarray(packed, np.uint8)
    return np.stack([packed & 15, packed >> 4], axis=-1).reshape(packed.shape[:-1] + (2 * packed.shape[-1],))


def dq4(packed, scales):
    """the contract on the CPU: (..., K / 2) bytes, (..., K / 32) scale codes -> fp32.  The product is formed in fp64,
    where it is exact for every pair, and cast once: exact wherever fp32 holds it, +-inf beyond, NaN for scale code 255"""
    v = VALUE[unpack4(packed)]
    s = np.repeat(SCALE[np.asarray(scales, np.uint8)], 32, axis=-1)
    with np.errstate(over="ignore", invalid="ignore"):
        return (v * s).astype(np.float32)


def e4m3_of(packed):
    """the same values as e4m3 codes, one per byte ((..., K)); -0 stays -0"""
    t = torch.from_numpy(VALUE[unpack4(packed)].astype(np.float32)).to(torch.float8_e4m3fn)
    assert np.array_equal(t.float().numpy(), VALUE[unpack4(packed)].astype(np.float32))
    return t.view(torch.uint8).numpy()


def nibbles(rng, shape):
    return rng.integers(0, 16, size=shape, dtype=np.uint8)


# ---- 1. the table ------------------------------------------------------------------------------------------------------
def test_the_reference_itself():
    """what the contract states, on the CPU reference used below"""
    one, six = pack4(np.full(32, 2)), pack4(np.full(32, 7))
    assert (dq4(one, [127]) == 1).all() and (dq4(pack4(np.arange(32) % 16), [127]) == np.tile(VALUE, 2)).all()
    assert (dq4(pack4(np.full(32, 1)), [0]) == np.float32(2.0 ** -128)).all()              # a subnormal, kept
    assert (dq4(one, [254]) == np.float32(2.0 ** 127)).all() and np.isnan(dq4(pack4(np.zeros(32)), [255])).all()
    assert np.isfinite(dq4(six, [252])).all() and (dq4(six, [253]) == np.inf).all()
    assert (dq4(pack4(np.full(32, 15)), [254]) == -np.inf).all()
    z = dq4(pack4(np.full(32, 8)), [3])
    assert (z == 0).all() and np.signbit(z).all()
    assert (dq4(np.array([0x21], np.uint8).repeat(16), [127])[:2] == [0.5, 1.0]).all()     # low nibble first


def _table():
    """row i, block j: the bytes 16 j .. 16 j + 15 under scale code (i + j) % 256 - every byte meets every scale code, and
    neighbouring blocks and rows differ"""
    packed = np.tile(np.arange(256, dtype=np.uint8), (256, 1))
    scales = ((np.arange(256)[:, None] + np.arange(16)[None, :]) % 256).astype(np.uint8)
    return packed, scales


@pytest.mark.parametrize("mode", (0, 1))
def test_widen_matches_the_whole_table(engine, mode):
    """all 256 bytes x all 256 scale codes; the codes 16 bytes and the scales 1 byte past a word of a guarded buffer"""
    packed, scales = _table()
    want = dq4(packed, scales).ravel()
    count = 2 * packed.size
    g_in = Guarded.input("in4", packed, OPERAND, 32, _dev(), dtype=np.uint8)
    g_sc, p_sc = _guarded_scales("scales", scales, 32, _dev())
    assert p_sc % 2 == 1
    out = torch.full((count + 8,), -1, dtype=torch.int16, device=_dev())
    engine.widen_fp4_mx(g_in.ptr, p_sc, out.data_ptr(), count, mode, _stream())
    torch.cuda.synchronize()
    check_all(g_in, g_sc)
    got = out.cpu().numpy().view(np.uint16)
    assert (got[count:] == 0xFFFF).all(), "written past count"
    _assert_words(got[:count], mode, want, f"mode={mode}")
    # the second pin: bsmr_widen_fp8_mx on the e4m3 re-encoding
    t8, ts = _t(e4m3_of(packed), np.uint8), _t(scales, np.uint8)
    out8 = torch.full((count,), -1, dtype=torch.int16, device=_dev())
    engine.widen_fp8_mx(t8.data_ptr(), ts.data_ptr(), out8.data_ptr(), count, mode, E4M3, _stream())
    torch.cuda.synchronize()
    got8 = out8.cpu().numpy().view(np.uint16)
    nan = np.isnan(want)
    assert np.array_equal(got[:count][~nan], got8[~nan]) and np.isnan(widen_words(mode, got8[nan])).all()


def test_widen_strides_over_a_large_array(engine):
    """2^24 + 32 elements: more blocks of 32 than the grid has threads (2048 blocks x 256), so the grid-stride loop takes
    a second step"""
    mode = 1
    count = (1 << 24) + 32
    rng = np.random.default_rng(8)
    packed = rng.integers(0, 256, size=count // 2, dtype=np.uint8)
    scales = scale_codes((count // 32,), 100, 150)
    src, sc = torch.from_numpy(packed).to(_dev()), torch.from_numpy(scales).to(_dev())
    out = torch.full((count + 8,), -1, dtype=torch.int16, device=_dev())
    engine.widen_fp4_mx(src.data_ptr(), sc.data_ptr(), out.data_ptr(), count, mode, _stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert (got[count:] == 0xFFFF).all()
    _assert_words(got[:count], mode, dq4(packed, scales), "large")


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


def dev_spmm4(engine, bw, p, K, transpose, v, X4, E8, mode, nb):
    """v (nb, nnz) fp32, X4 (nb, rows, K / 2) uint8, E8 (nb, rows, K / 32) uint8 -> the words of Y (nb, rows_y, K)"""
    tv, tX, tE = _t(v[:nb]), _t(X4[:nb], np.uint8), _t(E8[:nb], np.uint8)
    tY = torch.full((nb, p.cols if transpose else p.rows, K), float("nan"), dtype=DT[mode], device=_dev())
    engine.spmm_x4_mx(bw, K, transpose, tv.data_ptr(), tX.data_ptr(), tE.data_ptr(), tY.data_ptr(), nb, _stream(), mode=mode)
    torch.cuda.synchronize()
    return words(tY)


@pytest.mark.parametrize("K", KS)
def test_spmm_x4_mx_equals_the_rounded_twin(engine, oracle, pat, values, K):
    rng = np.random.default_rng(100 * K + 4)
    bw = pat.bw[8]
    for transpose, rows in ((0, pat.cols), (1, pat.rows)):
        X4 = pack4(nibbles(rng, (NB, rows, K)))
        E8 = scale_codes((NB, rows, K // 32), salt=K + transpose)            # codes 112 .. 134
        X = dq4(X4, E8)
        assert np.isfinite(X).all()
        twin = np.stack([gather(oracle, pat.lists(transpose), values[b], X[b]) for b in range(NB)])
        Y32 = dev_spmm32(engine, bw, pat, K, transpose, values, X, NB)
        empty = EMPTY_COL if transpose else pat.row_with[0]
        X8 = e4m3_of(X4)
        for mode in (0, 1):
            want = oracle.round_array(ROUND[mode], twin)
            assert copy_is_exact(mode, X)                                    # bf16 always; fp16: shifts -15 .. 7 lie in [-23, 13]
            for nb in (1, NB):
                where = f"spmm_x4_mx mode={mode} transpose={transpose} K={K} batches={nb}"
                w = dev_spmm4(engine, bw, pat, K, transpose, values, X4, E8, mode, nb)
                assert_twin(widen_words(mode, w), want[:nb], where)
                assert not w[:, empty].any(), where + ": a destination without entries is +0"
                assert w.tobytes() == words(to16(mode, Y32[:nb])).tobytes(), where + ": not bsmr_spmm on dq narrowed"
                w16 = dev_spmm16(engine, bw, pat, K, transpose, values, to16(mode, X), mode, nb)
                assert w.tobytes() == w16.tobytes(), where + ": differs from bsmr_spmm_16 on the dequantised copy"
                w8 = dev_spmm8_mx(engine, bw, pat, K, transpose, values, X8, E8, mode, E4M3, nb)
                assert w.tobytes() == w8.tobytes(), where + ": differs from bsmr_spmm_x8_mx on the e4m3 re-encoding"


@pytest.mark.parametrize("K", (32, 64, 256))
def test_spmm_x4_mx_in_place_is_spmm_on_dq(engine, in_place, K):
    """BSMR_BACKWARD_PERMUTE=0 with transpose = 1 is spmmGather4<.., MAP = true, ..>: bit for bit bsmr_spmm on dq narrowed,
    bsmr_spmm_x8_mx on the re-encoding, and the call on the permuting handle; K = 256 is the widest slice"""
    p, nb = in_place, 2
    rng = np.random.default_rng(950 + K)
    v = _wide(rng, (nb, p.nnz), -3, 3)
    X4 = pack4(nibbles(rng, (nb, 96, K)))
    E8 = scale_codes((nb, 96, K // 32), salt=K)
    X, X8 = dq4(X4, E8), e4m3_of(X4)
    for mode in (0, 1):
        for transpose in (1, 0):
            where = f"in place: mode={mode} transpose={transpose} K={K}"
            w = dev_spmm4(engine, p.bw, p, K, transpose, v, X4, E8, mode, nb)
            Y32 = dev_spmm32(engine, p.bw, p, K, transpose, v, X, nb)
            assert w.any() and w.tobytes() == words(to16(mode, Y32)).tobytes(), where + ": not bsmr_spmm on dq narrowed"
            w8 = dev_spmm8_mx(engine, p.bw, p, K, transpose, v, X8, E8, mode, E4M3, nb)
            assert w.tobytes() == w8.tobytes(), where + ": differs from bsmr_spmm_x8_mx on the e4m3 re-encoding"
            wp = dev_spmm4(engine, p.permuted, p, K, transpose, v, X4, E8, mode, nb)
            assert w.tobytes() == wp.tobytes(), where + ": differs from the handle that permutes v"


# ---- 3. planted blocks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 1))
def test_spmm_x4_mx_with_planted_blocks(engine, oracle, pat, values, mode):
    """in the sources of the 5-entry row: a block under scale code 255 (NaN - and only the rows that list it), blocks of
    the value 6 under 253 and of -6 under 254 (+-inf), a block of 0.5 .. 1.5 under scale code 0 (subnormal elements) and a
    block of -0 codes.  Each reaches the destinations that list it and no other, as in the twin"""
    K, bw = 128, pat.bw[8]
    rng = np.random.default_rng(300 + mode)
    N4 = nibbles(rng, (1, pat.cols, K))
    E8 = scale_codes((1, pat.cols, K // 32), salt=11)
    src = pat.ci[pat.ro[pat.row_with[5]]:pat.ro[pat.row_with[5] + 1]]        # the columns of the 5-entry row
    E8[0, src[0], 1] = 255
    N4[0, src[1], 64:96], E8[0, src[1], 2] = 7, 253
    N4[0, src[2], 96:128], E8[0, src[2], 3] = np.tile([1, 2, 3, 9], 8), 0
    N4[0, src[3], 0:32], E8[0, src[3], 0] = 15, 254
    N4[0, src[4], 32:64] = 8
    X4 = pack4(N4)
    X = dq4(X4, E8)
    assert np.isnan(X[0, src[0], 32:64]).all() and (X[0, src[1], 64:96] == np.inf).all() and (X[0, src[3], :32] == -np.inf).all()
    sub = X[0, src[2], 96:128]
    assert (sub != 0).all() and (np.abs(sub) < np.float32(2.0 ** -126)).all()              # subnormal, not flushed
    assert (X[0, src[4], 32:64] == 0).all() and np.signbit(X[0, src[4], 32:64]).all()
    twin = gather(oracle, pat.lists(0), values[0], X[0])
    r5 = twin[pat.row_with[5]]
    assert np.isnan(r5[32:64]).all() and np.isinf(r5[64:96]).all() and np.isinf(r5[:32]).all() and np.isfinite(r5[96:128]).all()
    nan_rows = np.isnan(twin).any(axis=1)
    lists_src0 = np.array([src[0] in pat.ci[pat.ro[r]:pat.ro[r + 1]] for r in range(pat.rows)])
    assert np.array_equal(nan_rows, lists_src0)                                            # that row's readers, no other
    w = dev_spmm4(engine, bw, pat, K, 0, values, X4, E8, mode, 1)
    assert_twin(widen_words(mode, w)[0], oracle.round_array(ROUND[mode], twin), f"mode={mode}")
    w8 = dev_spmm8_mx(engine, bw, pat, K, 0, values, e4m3_of(X4), E8, mode, E4M3, 1)
    got, got8 = widen_words(mode, w), widen_words(mode, w8)
    assert np.array_equal(np.isnan(got), np.isnan(got8)) and np.array_equal(w[~np.isnan(got)], w8[~np.isnan(got8)])


def test_subnormal_elements_are_not_flushed(engine):
    """one destination, one source, weight 2^20: under scale code 0 the elements 0.5 .. 6 times 2^-127 are subnormal or
    barely normal, the products are normal.  A kernel that flushed the dequantised element would give 0 for the small ones"""
    K = 32
    bw = engine.backward_create(1, 1, np.array([0, 1], np.uint32), np.zeros(1, np.uint32), device=0)
    try:
        N4 = (np.arange(K) % 16).astype(np.uint8).reshape(1, 1, K)
        X4, E8 = pack4(N4), np.zeros((1, 1, 1), np.uint8)
        v = np.full((1, 1), 2.0 ** 20, np.float32)
        want = (np.float32(0.0) + dq4(X4, E8) * np.float32(2.0 ** 20))[0]    # the chain starts at +0: 2^20 * -0 ends as +0
        assert (want == (np.tile(VALUE, 2) * 2.0 ** -107).astype(np.float32)).all() and np.count_nonzero(want) == 28
        assert not np.signbit(want[want == 0]).any()
        for mode in (0, 1):
            tY = torch.full((1, 1, K), float("nan"), dtype=DT[mode], device=_dev())
            tv, tX, tE = _t(v), _t(X4, np.uint8), _t(E8, np.uint8)
            engine.spmm_x4_mx(bw, K, False, tv.data_ptr(), tX.data_ptr(), tE.data_ptr(), tY.data_ptr(), 1, _stream(), mode=mode)
            torch.cuda.synchronize()
            assert words(tY).tobytes() == words(to16(mode, want)).tobytes(), mode
            assert mode == 0 or (widen_words(mode, words(tY)) == want).all()               # bf16 holds them exactly
    finally:
        engine.backward_destroy(bw)


# ---- 4. the fused attention --------------------------------------------------------------------------------------------
def dev_attention4(engine, bw, p, Kv, scale, scores, V4, E8, nb, mode):
    tp, tV, tE = _t(scores), _t(V4, np.uint8), _t(E8, np.uint8)
    tO = torch.full((nb, p.rows, Kv), float("nan"), dtype=DT[mode], device=_dev())
    tm = torch.full((nb, p.rows), float("nan"), device=_dev())
    ts = torch.full((nb, p.rows), float("nan"), device=_dev())
    engine.sparse_attention_x4_mx(bw, Kv, scale, tp.data_ptr(), tV.data_ptr(), tE.data_ptr(), tO.data_ptr(), tm.data_ptr(),
                                  ts.data_ptr(), nb, _stream(), mode=mode)
    torch.cuda.synchronize()
    return words(tO), tm.cpu().numpy(), ts.cpu().numpy()


@pytest.mark.parametrize("Kv", (32, 128))
def test_attention_x4_mx_is_the_fp32_attention_on_dq(engine, pat, Kv):
    rng = np.random.default_rng(500 + 10 * Kv + 4)
    bw, nb, scale = pat.bw[8], 2, 0.37
    scores = (rng.uniform(-8, 8, (nb, pat.nnz)) / scale).astype(np.float32)
    dead = pat.row_with[63]
    scores[0, pat.ro[dead]:pat.ro[dead + 1]] = -np.inf                       # a dead row; row_with[0] is the empty one
    V4 = pack4(nibbles(rng, (nb, pat.cols, Kv)))
    E8 = scale_codes((nb, pat.cols, Kv // 32), salt=Kv)
    V = dq4(V4, E8)
    O32, m32, s32 = dev_attention(engine, bw, pat, Kv, scale, scores, V, nb, None)
    for b in range(nb):
        check_forward(pat.ro, pat.ci, scores[b], scale, V[b], O32[b], f"Kv={Kv} batch {b}")
    for mode in (0, 1):
        where = f"attention_x4_mx mode={mode} Kv={Kv}"
        O4, m4, s4 = dev_attention4(engine, bw, pat, Kv, scale, scores, V4, E8, nb, mode)
        assert np.array_equal(O4, words(to16(mode, O32))), where + ": not the fp32 call rounded once"
        assert m4.tobytes() == m32.tobytes() and s4.tobytes() == s32.tobytes(), where
        for r in (dead, pat.row_with[0]):
            assert not O4[0, r].any() and m4[0, r] == -np.inf and s4[0, r] == 0, (where, r)
        assert s4[1, dead] > 0
        O8, m8, s8 = dev_attention_mx(engine, bw, pat, Kv, scale, scores, e4m3_of(V4), E8, nb, mode, E4M3)
        assert O4.tobytes() == O8.tobytes() and m4.tobytes() == m8.tobytes() and s4.tobytes() == s8.tobytes(), \
            where + ": differs from bsmr_sparse_attention_x8_mx on the e4m3 re-encoding"


# ---- 5. the forward is exact -------------------------------------------------------------------------------------------
INT_NIBBLES = np.array([0, 2, 4, 5, 6, 7, 8, 10, 12, 13, 14, 15], np.uint8)  # 0, +-1, +-2, +-3, +-4, +-6 (and -0)


def dev_sddmm4(engine, plan, K, A16, B4, E8, nb, mode):
    tA, tB, tE = A16.contiguous().to(_dev()), _t(B4, np.uint8), _t(E8, np.uint8)
    tP = torch.full((nb, plan.pat.nnz), float("nan"), dtype=torch.float32, device=_dev())
    engine.sddmm_b4_mx(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tE.data_ptr(), tP.data_ptr(), nb, mode, _stream())
    torch.cuda.synchronize()
    return tP.cpu().numpy()


# the dense, hybrid and residue-only patterns on the conversion-pass road, and a road whose fp32 form never allocates the
# 16-bit workspace, so that bsmr_sddmm_b4_mx reserves it from cold
FORWARD_CASES = [("stream-pass", p, (32, 128)) for p in DENSE_PATS] + [
    ("residue-b-only", "rand-sparse", (32, 128)),
    ("stream-cvt-in-kernel", "nips-hybrid", (32, 128))]


@pytest.mark.parametrize("name,pname,ks", FORWARD_CASES)
def test_sddmm_b4_mx_is_exact_on_scaled_integers(engine, oracle, patterns, name, pname, ks):
    """A integers in [-8, 8], B the integers of e2m1 under block scales 2^s, s in [-2, 3]: multiples of 1/4 up to 48, exact
    in fp16 and bf16; the products and their sums (below 8 * 48 * K) are exact in fp32"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"fp4 {name} {pname}".encode()))
    pat = patterns[pname]
    every = np.ones(pat.nnz, dtype=bool)
    plan = _build(engine, pat, name)
    try:
        for K in ks:
            A = small_ints(rng, NB, pat.rows, K)
            B4 = pack4(INT_NIBBLES[rng.integers(0, INT_NIBBLES.size, size=(NB, pat.cols, K))])
            E8 = scale_codes((NB, pat.cols, K // 32), 125, 130, salt=K)
            Bdq = dq4(B4, E8)
            assert np.abs(Bdq).max() <= 48
            want = [model(oracle, pat, K, A[b], Bdq[b], 0, ~every) for b in range(NB)]
            for mode in (0, 1):
                A16 = to16(mode, A)
                assert copy_is_exact(mode, Bdq)
                for nb in (1, NB):
                    where = f"{name} {pname} K={K} mode={mode} batches={nb}"
                    P = dev_sddmm4(engine, plan, K, A16[:nb], B4[:nb], E8[:nb], nb, mode)
                    for b in range(nb):
                        assert_exact(P[b], want[b], f"{where} batch {b}")
                    P16 = dev_sddmm(engine, plan, K, A16[:nb], to16(mode, Bdq[:nb]), nb, mode)
                    assert P.tobytes() == P16.tobytes(), where + ": differs from bsmr_sddmm_16 on narrow(dq(B))"
                    P8 = dev_sddmm_mx(engine, plan, K, A16[:nb], e4m3_of(B4[:nb]), E8[:nb], nb, mode, E4M3)
                    assert P.tobytes() == P8.tobytes(), where + ": differs from bsmr_sddmm_b8_mx on the e4m3 re-encoding"
    finally:
        plan.close()


# ---- 6. the memory contract --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (32, 256))
@pytest.mark.parametrize("mode", (0, 1))
def test_fp4_calls_stay_inside_the_buffers(engine, oracle, pat, patterns, mode, K):
    """fp4 and 16-bit arrays 16 bytes, value arrays 4 bytes past a 512-byte boundary, the scales at an odd address, two
    batches: guards and inputs intact, every output word written, the expected bits.  The fp4 payload is rows * K / 2
    bytes and its guard starts directly behind it: a kernel that strode rows by K bytes would take the second half of
    its rows from the guard, whose bytes decode to finite e2m1 values, not NaN - so it is the comparison of the bits with
    the twin, on every row, that trips"""
    nb, dev, s, bw = 2, _dev(), _stream(), pat.bw[8]
    rng = np.random.default_rng(57 * K + 2 * mode + 4)
    v = _wide(rng, (nb, pat.nnz), -3, 3)
    gv = Guarded.input("v", v, VALUES, K, dev)
    X4 = {0: pack4(nibbles(rng, (nb, pat.cols, K))), 1: pack4(nibbles(rng, (nb, pat.rows, K)))}
    E8 = {t: scale_codes((nb, X4[t].shape[1], K // 32), salt=t) for t in (0, 1)}
    g4 = {t: Guarded.input(f"X4[{t}]", X4[t], OPERAND, K, dev, dtype=np.uint8) for t in (0, 1)}
    assert g4[0].nbytes == nb * pat.cols * K // 2
    gE = {t: _guarded_scales(f"E8[{t}]", E8[t], K, dev) for t in (0, 1)}
    X = {t: dq4(X4[t], E8[t]) for t in (0, 1)}
    # the dequantising pass
    gW = Guarded.output("widened", 2 * X4[0].size, OPERAND, K, dev, dtype=np.uint16)
    engine.widen_fp4_mx(g4[0].ptr, gE[0][1], gW.ptr, 2 * X4[0].size, mode, s)
    torch.cuda.synchronize()
    check_all(g4[0], gE[0][0], gW)
    _assert_words(gW.numpy(), mode, X[0].ravel(), "widen_fp4_mx")
    # the gather, both directions
    for transpose, rows in ((0, pat.rows), (1, pat.cols)):
        want = oracle.round_array(ROUND[mode], np.stack([gather(oracle, pat.lists(transpose), v[b], X[transpose][b])
                                                         for b in range(nb)]))
        gY = Guarded.output("Y16", nb * rows * K, OPERAND, K, dev, dtype=np.uint16)
        engine.spmm_x4_mx(bw, K, transpose, gv.ptr, g4[transpose].ptr, gE[transpose][1], gY.ptr, nb, s, mode=mode)
        torch.cuda.synchronize()
        check_all(gv, g4[transpose], gE[transpose][0], gY)
        assert_twin(widen_words(mode, gY.numpy()).reshape(nb, rows, K), want, f"K={K} transpose={transpose}: spmm_x4_mx")
    # the fused attention
    scale = 0.5
    scores = rng.uniform(-6, 6, (nb, pat.nnz)).astype(np.float32)
    gP = Guarded.input("P", scores, VALUES, K, dev)
    gO = Guarded.output("O16", nb * pat.rows * K, OPERAND, K, dev, dtype=np.uint16)
    gm, gs = Guarded.output("m", nb * pat.rows, VALUES, K, dev), Guarded.output("s", nb * pat.rows, VALUES, K, dev)
    engine.sparse_attention_x4_mx(bw, K, scale, gP.ptr, g4[0].ptr, gE[0][1], gO.ptr, gm.ptr, gs.ptr, nb, s, mode=mode)
    torch.cuda.synchronize()
    check_all(gP, g4[0], gE[0][0], gO, gm, gs)
    O32, m32, s32 = dev_attention(engine, bw, pat, K, scale, scores, X[0], nb, None)
    assert gO.numpy().tobytes() == words(to16(mode, O32)).tobytes()
    assert gm.numpy().tobytes() == m32.tobytes() and gs.numpy().tobytes() == s32.tobytes()
    # the forward: a hybrid plan (dense kernel + residue) and an all-sparse one
    for pname, name in (("nips-hybrid", "stream-pass"), ("rand-sparse", "residue-b-only")):
        npat = patterns[pname]
        plan = _build(engine, npat, name)
        try:
            A = small_ints(rng, nb, npat.rows, K)
            B4 = pack4(INT_NIBBLES[rng.integers(0, INT_NIBBLES.size, size=(nb, npat.cols, K))])
            Es = scale_codes((nb, npat.cols, K // 32), 125, 130)
            gA = Guarded.input("A16", words(to16(mode, A)), OPERAND, K, dev, dtype=np.uint16)
            gB = Guarded.input("B4", B4, OPERAND, K, dev, dtype=np.uint8)
            gBs, pBs = _guarded_scales("Bs", Es, K, dev)
            gOut = Guarded.output("P", nb * npat.nnz, VALUES, K, dev)
            engine.sddmm_b4_mx(plan.plan, K, gA.ptr, gB.ptr, pBs, gOut.ptr, nb, mode, s)
            torch.cuda.synchronize()
            check_all(gA, gB, gBs, gOut)
            P, Bdq = gOut.numpy().reshape(nb, npat.nnz), dq4(B4, Es)
            for b in range(nb):
                assert_exact(P[b], model(oracle, npat, K, A[b], Bdq[b], 0, np.zeros(npat.nnz, bool)),
                             f"{name} {pname} K={K} mode={mode} batch {b}")
        finally:
            plan.close()


# ---- 7. the rules ------------------------------------------------------------------------------------------------------
def test_argument_rules_on_live_handles(engine, pat, patterns):
    """handle, K, the mode, the pointers (the scales among them, at any alignment), num_batches - and afterwards the
    scratch tensor every pointer aimed at is still zero: nothing ran"""
    hip, bad, ok, s = engine.hip(), engine.ERR_INVALID_ARG, engine.OK, _stream()
    K = 64
    plan = _build(engine, patterns["nips-hybrid"], "stream-pass")
    t = torch.zeros(1500 * K + 50000, dtype=torch.float32, device=_dev())
    p = t.data_ptr()
    assert p % 16 == 0
    bw = pat.bw[8]
    sddmm = lambda a=p, b=p, e=p + 1, P=p, nb=1, mode=0, k=K: hip.bsmr_sddmm_b4_mx(plan.plan, k, a, b, e, P, nb, mode, s)
    spmm = lambda v=p, x=p, e=p + 1, y=p, nb=1, mode=0, k=K, tr=0: hip.bsmr_spmm_x4_mx(bw, k, tr, v, x, e, y, nb, mode, s)
    attn = lambda P=p, v=p, e=p + 1, o=p, m=p, ss=p, nb=1, mode=0, k=K, scale=1.0: hip.bsmr_sparse_attention_x4_mx(
        bw, k, scale, P, v, e, o, m, ss, nb, mode, s)
    try:
        for call in (sddmm, spmm, attn):
            for k in (0, 48, 16):
                assert call(k=k) == engine.ERR_UNSUPPORTED_K
                assert call(k=k, mode=2) == engine.ERR_UNSUPPORTED_K                             # K before the mode
            for mode in (2, 3, -1, 7):
                assert call(mode=mode) == bad
                assert call(mode=mode, e=None) == bad
            for mode in (0, 1):
                assert call(nb=65536, mode=mode) == bad
                assert call(nb=0, mode=mode) == ok                                               # a no-op
                assert call(e=None, mode=mode) == bad                                            # the scales are an input
                assert call(e=None, nb=0, mode=mode) == bad                                      # ... also in front of the no-op
        for mode in (0, 1):
            m = dict(mode=mode)
            for kw in (dict(a=p + 8), dict(b=p + 8), dict(P=p + 2), dict(a=None), dict(b=None), dict(P=None)):
                assert sddmm(**kw, **m) == bad, kw
            for kw in (dict(v=p + 2), dict(x=p + 8), dict(y=p + 8), dict(v=None), dict(x=None), dict(y=None), dict(tr=2)):
                assert spmm(**kw, **m) == bad, kw
            for kw in (dict(P=p + 2), dict(v=p + 8), dict(o=p + 8), dict(m=p + 2), dict(ss=p + 2), dict(P=None), dict(v=None),
                       dict(o=None), dict(m=None), dict(ss=None), dict(scale=float("nan")), dict(scale=float("inf"))):
                assert attn(**kw, **m) == bad, kw
            for src, sc, dst in ((p + 8, p, p), (p, p, p + 8), (None, p, p), (p, None, p), (p, p, None)):
                assert hip.bsmr_widen_fp4_mx(src, sc, dst, 256, mode, s) == bad
            assert hip.bsmr_widen_fp4_mx(p, p + 3, p, 48, mode, s) == bad                         # count % 32
            assert hip.bsmr_widen_fp4_mx(p + 8, None, None, 0, mode, s) == ok
        for mode in (2, 3, -1):
            assert hip.bsmr_widen_fp4_mx(p, p, p, 256, mode, s) == bad
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
        for mode in (0, 1):
            for transpose, rows_y in ((0, M), (1, N)):
                Y = torch.full((nb, rows_y, K), float("nan"), dtype=DT[mode], device=_dev())
                assert hip.bsmr_spmm_x4_mx(bw, K, transpose, None, None, None, Y.data_ptr(), nb, mode, s) == engine.OK
                torch.cuda.synchronize()
                assert not words(Y).any()
            O = torch.full((nb, M, K), float("nan"), dtype=DT[mode], device=_dev())
            m, ss = torch.zeros(nb, M, device=_dev()), torch.ones(nb, M, device=_dev())
            assert hip.bsmr_sparse_attention_x4_mx(bw, K, 1.0, None, None, None, O.data_ptr(), m.data_ptr(), ss.data_ptr(), nb,
                                                   mode, s) == engine.OK
            torch.cuda.synchronize()
            assert not words(O).any() and (m == -np.inf).all() and not ss.any()
            assert hip.bsmr_spmm_x4_mx(bw, K, 0, None, None, None, None, nb, mode, s) == engine.ERR_INVALID_ARG
    finally:
        engine.backward_destroy(bw)
