"""Everything on the bsmr_backward handle past 2^32 *elements*: the SpMM gathers of the backward, their fp16 / bf16 forms and
16-bit stores, the sparse row softmax and the fused attention (include/bsmr_hip.h).

tests/test_gpu_backward_twin.py::test_addresses_past_4gib and tests/test_gpu_softmax.py::test_large_batch_past_4gib pass
4 GiB in bytes and stay below 2^31 elements.  These kernels use plain pointer arithmetic, so the compiler scales to bytes
in 64 bits by itself; what one dropped (uint64_t) gives is a 32-bit element index - s * K, (b * M + dest) * K,
b * pBatch + slot * K, blockIdx.y * nnz - which wraps at 2^32 elements (16 GiB of fp32, 8 GiB of 16-bit data) and goes
negative at 2^31.  Each case below takes the smallest shape at which one of these indices passes 2^32, asserts the crossing
in Python before it allocates, and checks positions past 2^32, their aliases 2^32 lower (where a wrapped index would land)
and positions between 2^31 and 2^32:
  R  far source and destination rows: S is 64 x (2^22 + 64) at K = 1024, so s * K and dest * K pass 2^32 (and the host's
     rowsX * K, rowsY * K); bsmr_sddmm_backward, bsmr_spmm through csc_to_csr (MAP), bsmr_spmm_lowp, bsmr_sddmm_backward_mode
     (roundOperands over more than 2^32 elements, the copy of A more than 2^32 elements behind the copy of B),
     bsmr_sddmm_backward_16 under both lane layouts, bsmr_spmm_16;
  O  far rows of O: S is (2^22 + 64) x 640 at Kv = 1024: (b * M + dest) * Kv in attnGather / attnGather16 / attnReduce (the
     last row and its alias are split rows) and r * K in attnRowDot; forward and backward, fp32 and bf16;
  S  workspace rows past 2^32 floats: 2^15 + 16 rows of 513 entries (two chunks each), K = 1024, 64 batches:
     b * pBatch + slot * K and (b * numSlots + slot) * K; bsmr_spmm, bsmr_spmm_16, bsmr_sparse_attention;
  V  value arrays past 2^32 entries: nnz = 2^17 + 300 (a full 512 x 256 pattern and one row of 556 entries), 32 800 batches:
     b * nnz in the four softmax kernels, attnRowMax, attnValuesBackward, attnGather, spmmGather and spmmPermute.
References: the fma-chain twin (tests/gather_twin.py) over the lists of the checked destinations only, on the rows of X
the device really holds (fetched with index_select); for the attention the exact-weights twin (tests/attention_twin.py).
Cases S and V also compare whole batches bit for bit with the same call at num_batches = 1, and hold the last batch
against the numpy twins (the forward softmax and the forward attention on random scores have no bit-exact twin: there the
twin is the header's error bound, and the bits are pinned by the single-batch call).  Outputs start as NaN.  Whole arrays
never come to the host.  A case skips, naming the amounts, when the device lacks the memory; the largest (V's attention
backward) peaks at about 71 GiB, and on a 288 GB MI355X none skips.

The pattern builders and the helpers that pick the positions to check take the wrap threshold as a parameter, 2^32 here;
tests/test_backward_extents_host.py runs them at 2^12 with K = 4 on the CPU."""
import time

import numpy as np
import pytest

from attention_twin import check_forward as attention_bound
from attention_twin import exact_forward, exact_scores, row_dot, values_backward
from gather_twin import CHUNK, assert_twin, col_lists, gather, row_lists
from softmax_twin import backward_twin
from softmax_twin import check_forward as softmax_bound
from softmax_twin import z_of
from test_gpu_backward_twin import _far_pattern, _fill_on_device, _sub_lists, narrow

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GiB = 1 << 30
T32 = 1 << 32
FAR = 64                                       # rows checked past the threshold, and the width of the sign-bit window
ROUND = {0: 2, 1: 3}                           # engine mode -> oracle.round_array id (fp16 RNE, bf16 RNE)
DT = {0: torch.float16, 1: torch.bfloat16}


# ---- builders and position helpers (threshold T in elements; shared with the CPU companion) ------------------------------
def checked_rows(T, K):
    """rows of a [rows, K] matrix to check: `far` (r K >= T), `alias` (far - T / K: where a wrapped index lands) and `sign`
    (around T / 2: the upper half has r K in [T / 2, T), negative as a signed index of that width)"""
    assert T % (2 * K) == 0
    wrap = T // K
    far = np.arange(wrap, wrap + FAR, dtype=np.int64)
    return {"far": far, "alias": far - wrap, "sign": np.arange(wrap // 2 - FAR // 2, wrap // 2 + FAR // 2, dtype=np.int64)}


def far_pattern(M, T, K, seed):
    """Case R: (N, ro, ci) with N = T / K + 64.  _far_pattern's 40 random columns per row, rows 0 - 7 with 12 of the last 64
    columns (c K >= T); rows 8 ... also hold 12 alias columns c - T / K (0 ... 63), rows 4 - 19 12 columns of the sign window;
    four of the far columns are kept empty in every row"""
    wrap = T // K
    N = wrap + FAR
    holes = set((wrap + np.array([1, 22, 45, 62])).tolist())
    ro, ci = _far_pattern(M, N, seed)
    rng = np.random.default_rng(seed + 77)
    per_row = []
    for r in range(M):
        s = set(ci[ro[r]:ro[r + 1]].tolist())
        if r >= 8:
            s |= set(rng.choice(FAR, 12, replace=False).tolist())
        if 4 <= r < 20:
            s |= set((wrap // 2 - FAR // 2 + rng.choice(FAR, 12, replace=False)).tolist())
        per_row.append(np.array(sorted(s - holes), np.uint32))
    ro = np.zeros(M + 1, np.uint32)
    ro[1:] = np.cumsum([x.size for x in per_row])
    return N, ro, np.concatenate(per_row)


def attention_far_pattern(T, Kv, N, seed):
    """Case O: (M, ro, ci, empty) with M = T / Kv + 64 rows over N columns: one to three distinct columns per row, `empty`
    rows with none (among the far 64, among their aliases, in the sign window and elsewhere), and CHUNK + 1 entries in the
    last row and in its alias M - 1 - T / Kv (split rows)"""
    wrap = T // Kv
    M = wrap + FAR
    assert N > CHUNK
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 4, M)
    empty = np.unique(np.concatenate([wrap + np.array([3, 17, 40]), np.array([5, 29]), wrap // 2 + np.array([-7, 9]),
                                      rng.integers(FAR, wrap // 2 - FAR, 8)]))
    lens[empty] = 0
    long_rows = (M - 1 - wrap, M - 1)
    lens[list(long_rows)] = CHUNK + 1
    ro = np.zeros(M + 1, np.int64)
    ro[1:] = np.cumsum(lens)
    row = np.repeat(np.arange(M), lens)
    pos = np.arange(int(ro[-1])) - ro[row]
    c0 = rng.integers(0, N, M)
    c1 = (c0 + rng.integers(1, N // 2, M)) % N
    c2 = (c0 + rng.integers(N // 2, N, M)) % N
    ci = np.where(pos == 0, c0[row], np.where(pos == 1, c1[row], c2[row]))
    for r in long_rows:
        ci[ro[r]:ro[r + 1]] = rng.permutation(N)[:CHUNK + 1]
    return M, ro.astype(np.uint32), ci.astype(np.uint32), empty


def split_rows_pattern(M, N, length, seed):
    """Case S: M rows of `length` distinct columns each (a shifted prefix of one of 64 permutations of the N columns)"""
    assert length <= N
    rng = np.random.default_rng(seed)
    perms = np.stack([rng.permutation(N)[:length] for _ in range(64)])
    r = np.arange(M)
    ci = (perms[r % 64] + (r * 7)[:, None]) % N
    return (np.arange(M + 1, dtype=np.int64) * length).astype(np.uint32), ci.reshape(-1).astype(np.uint32)


def slot_table(offsets):
    """(first_slot per destination or -1, num_slots): the chunk table bsmr_backward_create builds (natural order)"""
    n = np.diff(np.asarray(offsets, np.int64))
    chunks = np.where(n > CHUNK, -(-n // CHUNK), 0)
    first = np.cumsum(chunks) - chunks
    return np.where(chunks > 0, first, -1), int(chunks.sum())


def slot_crossing(T, num_slots, K):
    """(batch, slot) of the first workspace row of [batch][num_slots][K] floats whose element index reaches T"""
    return divmod(-(-T // K), num_slots)


def row_of_slot(offsets, slot):
    """(destination, chunk) that owns workspace row `slot`"""
    first, _ = slot_table(offsets)
    n = np.diff(np.asarray(offsets, np.int64))
    owners = np.flatnonzero((first >= 0) & (first <= slot))
    d = int(owners[-1])
    k = slot - int(first[d])
    assert 0 <= k < -(-int(n[d]) // CHUNK)
    return d, k


def batches_to_check(T, nnz, nb):
    """batch 0, the batches whose [b nnz, (b + 1) nnz) holds entry T / 2 and entry T and their neighbours, the last batch"""
    h, c = (T // 2) // nnz, T // nnz
    assert c + 1 < nb, "the batches do not pass the threshold"
    return sorted({0, h - 1, h, h + 1, c - 1, c, c + 1, nb - 1} & set(range(nb)))


def sub_rows(ro, ci, rows):
    """(sub_ro, sub_ci, idx): the pattern of `rows` only, in that order; idx = their positions in the CSR arrays"""
    ro = np.asarray(ro, np.int64)
    parts = [np.arange(ro[r], ro[r + 1], dtype=np.int64) for r in rows]
    idx = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    sub = np.zeros(len(rows) + 1, np.uint32)
    sub[1:] = np.cumsum([x.size for x in parts])
    return sub, np.asarray(ci)[idx].astype(np.uint32), idx


def row_max(sub_ro, z):
    """m of the contract for NaN-free z: the fp32 maximum per row, -inf for an empty row"""
    sub_ro = np.asarray(sub_ro, np.int64)
    m = np.full(sub_ro.size - 1, -np.inf, np.float32)
    live = np.flatnonzero(np.diff(sub_ro) > 0)
    if live.size:
        m[live] = np.maximum.reduceat(np.asarray(z, np.float32), sub_ro[live])
    return m


def full_pattern_with_long_row(M, N0, extra, long_row):
    """Case V: every row holds columns 0 ... N0 - 1; `long_row` also holds N0 ... N0 + extra - 1"""
    lens = np.full(M, N0, np.int64)
    lens[long_row] += extra
    ro = np.zeros(M + 1, np.int64)
    ro[1:] = np.cumsum(lens)
    ci = np.concatenate([np.arange(n) for n in lens])
    return N0 + extra, ro.astype(np.uint32), ci.astype(np.uint32)


# ---- device helpers ------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_dev())


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=_dev())      # poisoned: every element must be written


def _need(extra_bytes, what):
    """skip unless the device has `extra_bytes` free beyond what the case already holds"""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(_dev())
    if free < extra_bytes + GiB:
        pytest.skip(f"{what}: needs {(extra_bytes + GiB) / GiB:.1f} GiB of free device memory, {free / GiB:.1f} GiB free")
    torch.cuda.reset_peak_memory_stats(_dev())


def _log(engine, what, bw, t0):
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(_dev()) + engine.backward_stats(bw)["workspace_bytes"]
    print(f"[backward-extents] {what}: peak {peak / GiB:.1f} GiB (tensors + workspace), {time.time() - t0:.1f} s", flush=True)


def _fetch(t, rows):
    """rows of a device matrix (or entries of a vector) as fp32 numpy; 16-bit elements widen exactly"""
    got = t.index_select(0, torch.from_numpy(np.asarray(rows, np.int64)).to(t.device))
    return got.float().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                       b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


def _mode(engine, mode):
    return engine.COMPUTE_F32 if mode is None else mode


# ---- Case R: far source rows and far destination rows ----------------------------------------------------------------------
class FarRows:
    T, M, K = T32, 64, 1024

    def __init__(self, engine, oracle):
        self.engine, self.oracle = engine, oracle
        T, M, K = self.T, self.M, self.K
        self.N, self.ro, self.ci = far_pattern(M, T, K, seed=1)
        self.nnz = int(self.ci.size)
        rows = checked_rows(T, K)
        self.dests = np.concatenate([rows["far"], rows["alias"], rows["sign"]])
        # the crossings: a source row read (s K) and a destination row stored (dest K) past T, the host's rowsX K / rowsY K
        assert int(self.ci.max()) * K >= T and int(rows["far"][0]) * K >= T and self.N * K > T
        assert T // 2 < int(rows["sign"][-1]) * K < T                         # ... and positions between T / 2 and T
        assert np.isin(rows["sign"][FAR // 2:], self.ci).any()
        self.rl, self.cl = row_lists(self.ro, self.ci), col_lists(M, self.N, self.ro, self.ci)
        self.col_len = np.diff(self.cl[0].astype(np.int64))[self.dests]
        far_len, alias_len = self.col_len[:FAR], self.col_len[FAR:2 * FAR]
        assert (far_len > 0).any() and (far_len == 0).any() and (alias_len[far_len == 0] > 0).any()
        self.sub = _sub_lists(self.cl, self.dests)
        self.used, remap = np.unique(self.ci, return_inverse=True)
        self.row_sub = (self.rl[0], remap.astype(np.uint32), self.rl[2])
        rng = np.random.default_rng(5)
        self.v, self.A = narrow(rng, self.nnz), narrow(rng, (M, K))
        self.tv, self.tA = _t(self.v), _t(self.A)
        self.handles, self._B = {}, None

    def handle(self, permute="1", lanes=None):
        key = (permute, lanes)
        if key not in self.handles:
            with pytest.MonkeyPatch.context() as mp:                             # both are read at create
                mp.setenv("BSMR_BACKWARD_PERMUTE", permute)
                if lanes:
                    mp.setenv("BSMR_GATHER16_LANES", str(lanes))
                else:
                    mp.delenv("BSMR_GATHER16_LANES", raising=False)
                self.handles[key] = self.engine.backward_create(self.M, self.N, self.ro, self.ci, device=0)
            assert self.engine.backward_stats(self.handles[key])["permute_values"] == int(permute)
        return self.handles[key]

    def B(self):
        """N x K fp32 on the device, a function of (row, k): kept for the whole case"""
        if self._B is None:
            self._B = torch.empty((self.N, self.K), dtype=torch.float32, device=_dev())
            _fill_on_device(self._B, 0)
        return self._B

    def B16(self, mode):
        """B / 2^12 in the mode's format (inside the fp16 range), converted on the device piece by piece"""
        B = self.B()
        out = torch.empty((self.N, self.K), dtype=DT[mode], device=_dev())
        step = 1 << 18
        for r0 in range(0, self.N, step):
            out[r0:r0 + step] = (B[r0:r0 + step] * 2.0 ** -12).to(DT[mode])
        return out

    def A16(self, mode):
        return self.tA.to(DT[mode])

    def check_rows(self, got, X, where, x_round=None, out_mode=None):
        """Y = S_v X / dA, all M rows, against the twin over the rows of X the pattern reads"""
        rows_read = _fetch(X, self.used)
        if x_round is not None:
            rows_read = self.oracle.round_array(ROUND[x_round], rows_read)
        want = gather(self.oracle, self.row_sub, self.v, rows_read)
        if out_mode is not None:
            want = self.oracle.round_array(ROUND[out_mode], want)
        assert_twin(got.float().cpu().numpy(), want, where)

    def check_cols(self, Y, A, where, out_mode=None):
        """Y = S_v^T X / dB on the far rows, their aliases and the sign window against the twin over their lists"""
        got = _fetch(Y, self.dests)
        want = gather(self.oracle, self.sub, self.v, A)
        if out_mode is not None:
            want = self.oracle.round_array(ROUND[out_mode], want)
        assert_twin(got, want, where)
        assert (_bits(got)[self.col_len == 0] == 0).all(), where + ": an empty column is +0"
        assert (np.abs(got[:FAR][self.col_len[:FAR] > 0]) > 0).any()

    def close(self):
        torch.cuda.synchronize()
        for h in self.handles.values():
            self.engine.backward_destroy(h)
        self._B = None
        torch.cuda.empty_cache()


@pytest.fixture(scope="class")
def far(engine, oracle):
    case = FarRows(engine, oracle)
    yield case
    case.close()


class TestFarRows:
    """Case R"""

    def test_sddmm_backward_fp32(self, engine, far):
        N, K, M = far.N, far.K, far.M
        assert N * K > T32                                                       # B read and dB stored past 2^32 elements
        _need(2 * N * K * 4, "B and dB")
        t0 = time.time()
        dA, dB = _nan(M, K), _nan(N, K)
        bw = far.handle()
        engine.sddmm_backward(bw, K, far.tv.data_ptr(), far.tA.data_ptr(), far.B().data_ptr(), dA.data_ptr(), dB.data_ptr(),
                              1, _stream())
        torch.cuda.synchronize()
        far.check_rows(dA, far.B(), "bsmr_sddmm_backward: dA")
        far.check_cols(dB, far.A, "bsmr_sddmm_backward: dB")
        _log(engine, "R bsmr_sddmm_backward fp32", bw, t0)

    def test_spmm_through_the_map(self, engine, far):
        """BSMR_BACKWARD_PERMUTE=0: the transposed direction reads v through csc_to_csr (spmmGather<W, true>)"""
        N, K, M = far.N, far.K, far.M
        assert N * K > T32
        _need(2 * N * K * 4, "X and Y")
        t0 = time.time()
        bw = far.handle(permute="0")
        Y0, Y1 = _nan(M, K), _nan(N, K)
        engine.spmm(bw, K, False, far.tv.data_ptr(), far.B().data_ptr(), Y0.data_ptr(), 1, _stream())
        engine.spmm(bw, K, True, far.tv.data_ptr(), far.tA.data_ptr(), Y1.data_ptr(), 1, _stream())
        torch.cuda.synchronize()
        far.check_rows(Y0, far.B(), "bsmr_spmm: Y = S X")
        far.check_cols(Y1, far.A, "bsmr_spmm: Y = S^T X through the map")
        _log(engine, "R bsmr_spmm, map", bw, t0)

    def test_spmm_lowp_fp16(self, engine, far):
        N, K, M, mode = far.N, far.K, far.M, 0
        assert N * K > T32
        _need(N * K * 4 + N * K * 4 + N * K * 2, "B, its fp16 copy and Y")
        t0 = time.time()
        bw = far.handle()
        X16, A16 = far.B16(mode), far.A16(mode)
        Y0, Y1 = _nan(M, K), _nan(N, K)
        engine.spmm_lowp(bw, K, False, far.tv.data_ptr(), X16.data_ptr(), Y0.data_ptr(), 1, _stream(), mode=mode)
        engine.spmm_lowp(bw, K, True, far.tv.data_ptr(), A16.data_ptr(), Y1.data_ptr(), 1, _stream(), mode=mode)
        torch.cuda.synchronize()
        far.check_rows(Y0, X16, "bsmr_spmm_lowp fp16: Y = S X16")
        far.check_cols(Y1, A16.float().cpu().numpy(), "bsmr_spmm_lowp fp16: Y = S^T X16")
        _log(engine, "R bsmr_spmm_lowp fp16", bw, t0)

    def test_sddmm_backward_mode_bf16(self, engine, far):
        """the library rounds B (more than 2^32 elements) and A itself; A's copy lies nB > 2^32 elements behind B's"""
        N, K, M, mode = far.N, far.K, far.M, 1
        nB = N * K
        assert nB > T32
        _need(2 * nB * 4 + nB * 2, "B, dB and the workspace copy of B")
        t0 = time.time()
        bw = far.handle()
        dA, dB = _nan(M, K), _nan(N, K)
        engine.sddmm_backward(bw, K, far.tv.data_ptr(), far.tA.data_ptr(), far.B().data_ptr(), dA.data_ptr(), dB.data_ptr(),
                              1, _stream(), mode=mode)
        torch.cuda.synchronize()
        assert engine.backward_stats(bw)["workspace_bytes"] >= (nB + M * K) * 2
        far.check_rows(dA, far.B(), "bsmr_sddmm_backward_mode bf16: dA", x_round=mode)
        far.check_cols(dB, far.oracle.round_array(ROUND[mode], far.A), "bsmr_sddmm_backward_mode bf16: dB")
        _log(engine, "R bsmr_sddmm_backward_mode bf16", bw, t0)

    @pytest.mark.parametrize("lanes", (4, 8))
    def test_sddmm_backward_16_fp16(self, engine, far, lanes):
        """16-bit stores at dest K >= 2^32, under both lane layouts of spmmGather16"""
        N, K, M, mode = far.N, far.K, far.M, 0
        assert N * K > T32
        _need(N * K * 4 + 2 * N * K * 2, "B, its fp16 copy and dB16")
        t0 = time.time()
        bw = far.handle(lanes=lanes)
        B16, A16 = far.B16(mode), far.A16(mode)
        dA, dB = _nan(M, K, dtype=DT[mode]), _nan(N, K, dtype=DT[mode])
        engine.sddmm_backward_16(bw, K, far.tv.data_ptr(), A16.data_ptr(), B16.data_ptr(), dA.data_ptr(), dB.data_ptr(), 1,
                                 _stream(), mode=mode)
        torch.cuda.synchronize()
        far.check_rows(dA, B16, f"bsmr_sddmm_backward_16 fp16 lanes {lanes}: dA16", out_mode=mode)
        far.check_cols(dB, A16.float().cpu().numpy(), f"bsmr_sddmm_backward_16 fp16 lanes {lanes}: dB16", out_mode=mode)
        _log(engine, f"R bsmr_sddmm_backward_16 fp16 lanes {lanes}", bw, t0)

    def test_spmm_16_bf16(self, engine, far):
        N, K, M, mode = far.N, far.K, far.M, 1
        assert N * K > T32
        _need(N * K * 4 + 2 * N * K * 2, "B, its bf16 copy and Y16")
        t0 = time.time()
        bw = far.handle()
        X16, A16 = far.B16(mode), far.A16(mode)
        Y0, Y1 = _nan(M, K, dtype=DT[mode]), _nan(N, K, dtype=DT[mode])
        engine.spmm_16(bw, K, False, far.tv.data_ptr(), X16.data_ptr(), Y0.data_ptr(), 1, _stream(), mode=mode)
        engine.spmm_16(bw, K, True, far.tv.data_ptr(), A16.data_ptr(), Y1.data_ptr(), 1, _stream(), mode=mode)
        torch.cuda.synchronize()
        far.check_rows(Y0, X16, "bsmr_spmm_16 bf16: Y16 = S X16", out_mode=mode)
        far.check_cols(Y1, A16.float().cpu().numpy(), "bsmr_spmm_16 bf16: Y16 = S^T X16", out_mode=mode)
        _log(engine, "R bsmr_spmm_16 bf16", bw, t0)


# ---- Case O: far rows of O in the attention calls --------------------------------------------------------------------------
class FarOutputs:
    T, Kv, N, scale = T32, 1024, 640, 0.5

    def __init__(self, engine, oracle):
        self.engine, self.oracle = engine, oracle
        T, Kv = self.T, self.Kv
        self.M, self.ro, self.ci, self.empty = attention_far_pattern(T, Kv, self.N, seed=3)
        self.nnz = int(self.ci.size)
        rows = checked_rows(T, Kv)
        self.rows = np.concatenate([rows["far"], rows["alias"], rows["sign"]])
        self.wrap = T // Kv
        assert (self.M - 1) * Kv >= T and self.M * Kv > T                        # (b M + dest) Kv and r K pass T
        assert T // 2 < int(rows["sign"][-1]) * Kv < T
        lens = np.diff(self.ro.astype(np.int64))
        assert lens[self.M - 1] == CHUNK + 1 == lens[self.M - 1 - self.wrap]     # attnReduce writes a far row
        far_empty = self.empty[np.isin(self.empty, rows["far"])]
        assert far_empty.size >= 3 and (lens[far_empty - self.wrap] > 0).all()    # empty far rows over non-empty aliases
        rng = np.random.default_rng(31)
        self.dead = np.array([self.wrap + 9, 21])                                # all -inf: a far row and an alias row
        assert (lens[self.dead] > 0).all()
        self.p, self.e = exact_scores(self.ro, rng, self.dead)
        self.sub_ro, self.sub_ci, self.idx = sub_rows(self.ro, self.ci, self.rows)
        self.dW = rng.standard_normal(self.nnz).astype(np.float32)
        self.V = rng.standard_normal((self.N, Kv)).astype(np.float32)
        self.bw = engine.backward_create(self.M, self.N, self.ro, self.ci, device=0)

    def close(self):
        torch.cuda.synchronize()
        self.engine.backward_destroy(self.bw)
        torch.cuda.empty_cache()

    def run(self, mode):
        engine, oracle, M, Kv, scale = self.engine, self.oracle, self.M, self.Kv, self.scale
        dt = torch.float32 if mode is None else DT[mode]
        size = 4 if mode is None else 2
        _need(2 * M * Kv * size, "O and dO")
        t0 = time.time()
        where = f"attention {'fp32' if mode is None else dt}"
        tV = _t(self.V).to(dt)
        Vw = tV.float().cpu().numpy()
        tp, tdW = _t(self.p), _t(self.dW)
        O, m, s = _nan(M, Kv, dtype=dt), _nan(M), _nan(M)
        engine.sparse_attention(self.bw, Kv, scale, tp.data_ptr(), tV.data_ptr(), O.data_ptr(), m.data_ptr(), s.data_ptr(), 1,
                                _stream(), mode=_mode(engine, mode))
        torch.cuda.synchronize()
        want_O, want_s = exact_forward(oracle, self.sub_ro, self.sub_ci, self.e[self.idx], Vw)
        if mode is not None:
            want_O = oracle.round_array(ROUND[mode], want_O)
        want_m = row_max(self.sub_ro, z_of(self.p[self.idx], scale))
        got_O, got_m, got_s = _fetch(O, self.rows), _fetch(m, self.rows), _fetch(s, self.rows)
        assert_twin(got_O, want_O, where + ": O")
        assert np.array_equal(_bits(got_m), _bits(want_m)), where + ": m"
        assert np.array_equal(_bits(got_s), _bits(want_s)), where + ": s"
        none = np.isin(self.rows, np.concatenate([self.empty, self.dead]))
        assert none[:FAR].sum() >= 4 and (want_s[~none] > 0).all()
        assert (_bits(got_O)[none] == 0).all() and (got_m[none] == -np.inf).all() and (_bits(got_s)[none] == 0).all()
        far_row, alias_row = M - 1, M - 1 - self.wrap
        assert not np.array_equal(got_O[FAR - 1], got_O[2 * FAR - 1])            # the far split row and its alias differ
        # backward: D = dO . O over every row, then dP and W of every entry
        gen = torch.Generator(device=_dev()).manual_seed(9)
        dO = torch.randn((M, Kv), generator=gen, device=_dev(), dtype=dt)
        dO[far_row] = torch.sign(O[far_row].float()).to(dt) * 4                  # D > 0 there ...
        dO[alias_row] = torch.sign(O[alias_row].float()).to(dt) * -4             # ... and < 0 in the alias
        dP, W = _nan(self.nnz), _nan(self.nnz)
        engine.sparse_attention_backward(self.bw, Kv, scale, tp.data_ptr(), m.data_ptr(), s.data_ptr(), tdW.data_ptr(),
                                         O.data_ptr(), dO.data_ptr(), dP.data_ptr(), W.data_ptr(), 1, _stream(),
                                         mode=_mode(engine, mode))
        torch.cuda.synchronize()
        D = row_dot(oracle, _fetch(dO, self.rows), got_O)                        # on the saved (rounded) O, as the device
        assert D[FAR - 1] > 1 and D[2 * FAR - 1] < -1
        s_e = np.repeat(want_s, np.diff(self.sub_ro.astype(np.int64)))
        with np.errstate(all="ignore"):
            want_W = np.where(s_e > 0, self.e[self.idx] / s_e, np.float32(0)).astype(np.float32)
        assert_twin(_fetch(W, self.idx), want_W, where + ": W")
        assert_twin(_fetch(dP, self.idx), values_backward(self.sub_ro, want_W, self.dW[self.idx], D, scale), where + ": dP")
        _log(engine, f"O {where}", self.bw, t0)


@pytest.fixture(scope="class")
def far_out(engine, oracle):
    case = FarOutputs(engine, oracle)
    yield case
    case.close()


class TestFarOutputs:
    """Case O"""

    def test_attention_fp32(self, far_out):
        far_out.run(None)

    def test_attention_bf16(self, far_out):
        far_out.run(1)


# ---- Case S: workspace rows past 2^32 floats -------------------------------------------------------------------------------
class SplitRows:
    T, K, N, NB, M, scale = T32, 1024, 640, 64, (1 << 15) + 16, 0.5

    def __init__(self, engine, oracle):
        self.engine, self.oracle = engine, oracle
        T, K, N, NB, M = self.T, self.K, self.N, self.NB, self.M
        self.ro, self.ci = split_rows_pattern(M, N, CHUNK + 1, seed=13)
        self.nnz = int(self.ci.size)
        _, self.slots = slot_table(self.ro)
        assert self.slots == 2 * M == 65568
        # b pBatch + slot K = (b numSlots + slot) K: the first workspace row at or past T, and past T / 2
        self.cross, self.half = slot_crossing(T, self.slots, K), slot_crossing(T // 2, self.slots, K)
        assert self.cross == (63, 63520) and self.half == (31, 64544) and self.cross[0] == NB - 1
        assert (NB * self.slots - 1) * K >= T > (self.cross[0] * self.slots + self.cross[1] - 1) * K
        rc, rh = row_of_slot(self.ro, self.cross[1])[0], row_of_slot(self.ro, self.half[1])[0]
        assert (rc, rh) == (31760, 32272)
        self.checked = {0: [0, rc, M - 1], self.half[0]: [0, rh - 1, rh, rh + 1, M - 1],
                        NB - 1: [0, rc - 1, rc, rc + 1, M - 1]}
        rng = np.random.default_rng(41)
        self.base_v = narrow(rng, self.nnz)
        self.base_p, self.e = exact_scores(self.ro, rng)
        self.f = np.linspace(0.5, 1.5, NB).astype(np.float32)
        self.rl = row_lists(self.ro, self.ci)
        self.bw = engine.backward_create(M, N, self.ro, self.ci, device=0)
        self.X = torch.empty((NB, N, K), dtype=torch.float32, device=_dev())
        for b in range(NB):
            _fill_on_device(self.X[b], b)
        self.X *= 2.0 ** -14                                                     # (sums of 513 products inside the fp16 range)
        self.tf = _t(self.f).view(NB, 1)

    def close(self):
        torch.cuda.synchronize()
        self.engine.backward_destroy(self.bw)
        self.X = None
        torch.cuda.empty_cache()

    def spmm(self, mode):
        engine, oracle, K, NB, M = self.engine, self.oracle, self.K, self.NB, self.M
        dt = torch.float32 if mode is None else DT[mode]
        size = 4 if mode is None else 2
        assert NB * self.slots * K > T32
        _need(NB * self.slots * K * 4 + NB * self.nnz * 4 + NB * M * K * size, "the partials, v and Y")
        t0 = time.time()
        where = f"bsmr_spmm{'' if mode is None else '_16 ' + str(dt)}"
        v = _t(self.base_v).view(1, -1) * self.tf                                # batch b: base * f_b, made on the device
        X = self.X.to(dt)
        Y, Y1 = _nan(NB, M, K, dtype=dt), _nan(M, K, dtype=dt)

        def call(vv, xx, yy, nb):
            if mode is None:
                engine.spmm(self.bw, K, False, vv.data_ptr(), xx.data_ptr(), yy.data_ptr(), nb, _stream())
            else:
                engine.spmm_16(self.bw, K, False, vv.data_ptr(), xx.data_ptr(), yy.data_ptr(), nb, _stream(), mode=mode)

        call(v, X, Y, NB)
        torch.cuda.synchronize()
        for b, rows in self.checked.items():
            Y1.fill_(float("nan"))
            call(v[b], X[b], Y1, 1)
            torch.cuda.synchronize()
            assert _same_bits(Y[b], Y1), f"{where}: batch {b} differs from the single-batch call"
            want = gather(oracle, _sub_lists(self.rl, rows), self.base_v * self.f[b], X[b].float().cpu().numpy())
            if mode is not None:
                want = oracle.round_array(ROUND[mode], want)
            assert_twin(_fetch(Y[b], rows), want, f"{where}: batch {b} rows {rows}")
        _log(engine, f"S {where}", self.bw, t0)

    def attention(self):
        engine, oracle, K, NB, M, scale = self.engine, self.oracle, self.K, self.NB, self.M, self.scale
        assert NB * self.slots * K > T32
        _need(NB * self.slots * K * 4 + 2 * NB * self.nnz * 4 + NB * M * K * 4, "the partials, P and O")
        t0 = time.time()
        P = _t(self.base_p).view(1, -1) * self.tf                                # -inf stays -inf, a row stays one constant
        O, m, s = _nan(NB, M, K), _nan(NB, M), _nan(NB, M)
        O1, m1, s1 = _nan(M, K), _nan(M), _nan(M)

        def call(pp, xx, oo, mm, ss, nb):
            engine.sparse_attention(self.bw, K, scale, pp.data_ptr(), xx.data_ptr(), oo.data_ptr(), mm.data_ptr(), ss.data_ptr(),
                                    nb, _stream())

        call(P, self.X, O, m, s, NB)
        torch.cuda.synchronize()
        for b, rows in self.checked.items():
            for t in (O1, m1, s1):
                t.fill_(float("nan"))
            call(P[b], self.X[b], O1, m1, s1, 1)
            torch.cuda.synchronize()
            assert _same_bits(O[b], O1) and _same_bits(m[b], m1) and _same_bits(s[b], s1), f"attention: batch {b}"
            sub_ro, sub_ci, idx = sub_rows(self.ro, self.ci, rows)
            want_O, want_s = exact_forward(oracle, sub_ro, sub_ci, self.e[idx], self.X[b].cpu().numpy())
            assert_twin(_fetch(O[b], rows), want_O, f"attention: batch {b} rows {rows}: O")
            assert np.array_equal(_bits(_fetch(s[b], rows)), _bits(want_s))
            want_m = row_max(sub_ro, z_of((self.base_p * self.f[b])[idx], scale))
            assert np.array_equal(_bits(_fetch(m[b], rows)), _bits(want_m))
        _log(engine, "S bsmr_sparse_attention", self.bw, t0)


@pytest.fixture(scope="class")
def split(engine, oracle):
    torch.cuda.empty_cache()
    case = SplitRows(engine, oracle)
    yield case
    case.close()


class TestWorkspaceRows:
    """Case S"""

    def test_spmm_fp32(self, split):
        split.spmm(None)

    def test_spmm_16_fp16(self, split):
        split.spmm(0)

    def test_attention_fp32(self, split):
        split.attention()


# ---- Case V: value arrays past 2^32 entries --------------------------------------------------------------------------------
class LongValues:
    T, M, N0, EXTRA, LONG_ROW, K, NB, scale = T32, 512, 256, 300, 7, 32, 32800, 0.8

    def __init__(self, engine, oracle):
        self.engine, self.oracle = engine, oracle
        self.N, self.ro, self.ci = full_pattern_with_long_row(self.M, self.N0, self.EXTRA, self.LONG_ROW)
        self.nnz = int(self.ci.size)
        assert self.nnz == (1 << 17) + self.EXTRA and self.NB * self.nnz > self.T and self.NB <= 65535     # b nnz passes T
        self.batches = batches_to_check(self.T, self.nnz, self.NB)
        assert any(self.T // 2 <= b * self.nnz < self.T for b in self.batches) and self.batches[-1] * self.nnz >= self.T
        self.rl, self.cl = row_lists(self.ro, self.ci), col_lists(self.M, self.N, self.ro, self.ci)
        rng = np.random.default_rng(51)
        self.base = (rng.standard_normal(self.nnz) * 3).astype(np.float32)
        self.base[rng.choice(self.nnz, 200, replace=False)] = -np.inf
        self.dbase = rng.standard_normal(self.nnz).astype(np.float32)
        self.f = np.linspace(0.5, 1.5, self.NB).astype(np.float32)
        self.g = np.linspace(1.25, 0.75, self.NB).astype(np.float32)
        self.bw = engine.backward_create(self.M, self.N, self.ro, self.ci, device=0)
        st = engine.backward_stats(self.bw)
        assert st["split_rows"] == 1 and st["permute_values"] == 1               # the long-row kernels run; spmmPermute runs
        self.tbase, self.tdbase = _t(self.base), _t(self.dbase)
        self.tf, self.tg = _t(self.f).view(-1, 1), _t(self.g).view(-1, 1)

    def values(self, base, factors):
        """[NB, nnz] on the device: batch b = base * factors[b]"""
        return base.view(1, -1) * factors

    def close(self):
        torch.cuda.synchronize()
        self.engine.backward_destroy(self.bw)
        torch.cuda.empty_cache()

    def softmax(self):
        engine, oracle, NB, nnz, scale, last = self.engine, self.oracle, self.NB, self.nnz, self.scale, self.NB - 1
        _need(2 * NB * nnz * 4, "X and Y (then Y and dY)")
        t0 = time.time()
        X = self.values(self.tbase, self.tf)
        Y = _nan(NB, nnz)
        engine.sparse_softmax(self.bw, scale, X.data_ptr(), Y.data_ptr(), NB, _stream())
        torch.cuda.synchronize()
        y1 = _nan(nnz)
        for b in self.batches:
            y1.fill_(float("nan"))
            engine.sparse_softmax(self.bw, scale, X[b].data_ptr(), y1.data_ptr(), 1, _stream())
            torch.cuda.synchronize()
            assert _same_bits(Y[b], y1), f"softmax: batch {b} differs from the single-batch call"
        softmax_bound(self.ro, self.base * self.f[last], scale, Y[last].cpu().numpy(), "softmax: last batch")
        del X
        torch.cuda.empty_cache()
        dY = self.values(self.tdbase, self.tg)
        engine.sparse_softmax_backward(self.bw, scale, Y.data_ptr(), dY.data_ptr(), dY.data_ptr(), NB, _stream())   # in place
        torch.cuda.synchronize()
        for b in self.batches:
            dy = self.tdbase * self.tg[b]
            y1.fill_(float("nan"))
            engine.sparse_softmax_backward(self.bw, scale, Y[b].data_ptr(), dy.data_ptr(), y1.data_ptr(), 1, _stream())
            torch.cuda.synchronize()
            assert _same_bits(dY[b], y1), f"softmax backward: batch {b} differs from the single-batch call"
        want = backward_twin(oracle, self.ro, Y[last].cpu().numpy(), self.dbase * self.g[last], scale)
        assert_twin(dY[last].cpu().numpy(), want, "softmax backward: last batch")
        _log(engine, "V softmax forward and backward", self.bw, t0)

    def spmm(self):
        engine, oracle, NB, nnz, K, M, N = self.engine, self.oracle, self.NB, self.nnz, self.K, self.M, self.N
        last = NB - 1
        _need(2 * NB * nnz * 4 + 2 * NB * (M + N) * K * 4, "v, its permuted copy, X and Y")
        t0 = time.time()
        v = self.values(self.tdbase, self.tg)
        gen = torch.Generator(device=_dev()).manual_seed(10)
        for transpose, rows_x, rows_y, lists in ((False, N, M, self.rl), (True, M, N, self.cl)):
            X = torch.randn((NB, rows_x, K), generator=gen, device=_dev())
            Y, Y1 = _nan(NB, rows_y, K), _nan(rows_y, K)
            engine.spmm(self.bw, K, transpose, v.data_ptr(), X.data_ptr(), Y.data_ptr(), NB, _stream())
            torch.cuda.synchronize()
            for b in self.batches:
                Y1.fill_(float("nan"))
                engine.spmm(self.bw, K, transpose, v[b].data_ptr(), X[b].data_ptr(), Y1.data_ptr(), 1, _stream())
                torch.cuda.synchronize()
                assert _same_bits(Y[b], Y1), f"bsmr_spmm transpose {transpose}: batch {b} differs from the single-batch call"
            want = gather(oracle, lists, self.dbase * self.g[last], X[last].cpu().numpy())
            assert_twin(Y[last].cpu().numpy(), want, f"bsmr_spmm transpose {transpose}: last batch")
            del X, Y, Y1
        _log(engine, "V bsmr_spmm both directions", self.bw, t0)

    def attention(self):
        engine, oracle, NB, nnz, K, M, N = self.engine, self.oracle, self.NB, self.nnz, self.K, self.M, self.N
        scale, last = self.scale, NB - 1
        _need(4 * NB * nnz * 4 + NB * (N + 2 * M) * K * 4, "P, dW, W, the workspace, V, O and dO")
        t0 = time.time()
        gen = torch.Generator(device=_dev()).manual_seed(11)
        P = self.values(self.tbase, self.tf)
        V = torch.randn((NB, N, K), generator=gen, device=_dev())
        O, m, s = _nan(NB, M, K), _nan(NB, M), _nan(NB, M)

        def fwd(pp, vv, oo, mm, ss, nb):
            engine.sparse_attention(self.bw, K, scale, pp.data_ptr(), vv.data_ptr(), oo.data_ptr(), mm.data_ptr(), ss.data_ptr(),
                                    nb, _stream())

        fwd(P, V, O, m, s, NB)
        torch.cuda.synchronize()
        O1, m1, s1 = _nan(M, K), _nan(M), _nan(M)
        for b in self.batches:
            for t in (O1, m1, s1):
                t.fill_(float("nan"))
            fwd(P[b], V[b], O1, m1, s1, 1)
            torch.cuda.synchronize()
            assert _same_bits(O[b], O1) and _same_bits(m[b], m1) and _same_bits(s[b], s1), f"attention: batch {b}"
        p_last = self.base * self.f[last]
        O_last = O[last].cpu().numpy()
        attention_bound(self.ro, self.ci, p_last, scale, V[last].cpu().numpy(), O_last, "attention: last batch")
        assert np.array_equal(_bits(m[last].cpu().numpy()), _bits(row_max(self.ro, z_of(p_last, scale))))
        # backward, dP in place of dW
        dO = torch.randn((NB, M, K), generator=gen, device=_dev())
        dW = self.values(self.tdbase, self.tg)
        W = _nan(NB, nnz)

        def bwd(pp, mm, ss, dw, oo, do, dp, ww, nb):
            engine.sparse_attention_backward(self.bw, K, scale, pp.data_ptr(), mm.data_ptr(), ss.data_ptr(), dw.data_ptr(),
                                             oo.data_ptr(), do.data_ptr(), dp.data_ptr(), ww.data_ptr(), nb, _stream())

        bwd(P, m, s, dW, O, dO, dW, W, NB)
        torch.cuda.synchronize()
        dp1, w1 = _nan(nnz), _nan(nnz)
        for b in self.batches:
            dw = self.tdbase * self.tg[b]
            dp1.fill_(float("nan"))
            w1.fill_(float("nan"))
            bwd(P[b], m[b], s[b], dw, O[b], dO[b], dp1, w1, 1)
            torch.cuda.synchronize()
            assert _same_bits(dW[b], dp1) and _same_bits(W[b], w1), f"attention backward: batch {b}"
        W_last = W[last].cpu().numpy()
        softmax_bound(self.ro, p_last, scale, W_last, "attention backward: W of the last batch")
        D = row_dot(oracle, dO[last].cpu().numpy(), O_last)
        assert_twin(dW[last].cpu().numpy(), values_backward(self.ro, W_last, self.dbase * self.g[last], D, scale),
                    "attention backward: dP of the last batch")
        _log(engine, "V attention forward and backward", self.bw, t0)


@pytest.fixture(scope="class")
def long_values(engine, oracle):
    torch.cuda.empty_cache()
    case = LongValues(engine, oracle)
    yield case
    case.close()


class TestValueArrays:
    """Case V"""

    def test_softmax(self, long_values):
        long_values.softmax()

    def test_spmm_both_directions(self, long_values):
        long_values.spmm()

    def test_attention(self, long_values):
        long_values.attention()
