"""The forward SDDMM at addresses past 4 GiB: P, the operands, their 16-bit copies and batch offsets.

Every other forward test runs plans of a few million entries on operands far below 4 GiB, so a 32-bit offset anywhere on
the forward path would pass them.  Here every case runs one BSMR_ENGINE_TUNED plan under each engine in turn
(bsmr_plan_set_tuned: streaming format 0 and 1, tiles, shared, sweep and GEMM on the 16-bit copies and on fp32 operands)
and under the tuner's own choice in modes 0, 1 and 2, and checks P against an exact fp64 reference:
  1. P past 4 GiB in one problem: fully dense patterns of 2^30 - 1, 2^30 and 2^30 + 2^15 entries.  The GEMM engine stores P
     at byte offset 4 x CSR index through a buffer resource of num_records = 0xFFFFFFFC, so it must serve the first plan
     and refuse the other two (gemmFits), whose entries every other engine must still write exactly;
  2. operands past 4 GiB: K = 512 with M = N = 2^22 - 16 (16-bit copies just under 4 GiB: the GEMM engine serves it) and
     2^22 (refused), the fp32 GEMM at K = 128 with 2^23 - 16 (served) and 2^23 (refused), entries in the first and last
     rows and columns, dense blocks and residue;
  3. batch offsets past 4 GiB (bsmr_sddmm_batch): P of the later batches, and A, B and the contiguous converted copies;
  4. bsmr_convert_operands + bsmr_sddmm_lowp on caller-owned 16-bit copies whose far rows lie past 4 GiB.
Operands are integers in [-15, 15] generated on the device from (row, k, salt), so that every product and partial sum is
exact in fp32 and in every mode: P must equal the fp64 dot product (torch on the device over the whole of P, numpy on
the host over a sample that always holds the boundary entries).  P starts as NaN, so an entry never written shows up.
An engine may refuse a choice (BSMR_ERR_BAD_PLAN / _INVALID_ARG); the plan must then be unchanged and the next call exact.
Each case asserts the path it took (bsmr_plan_get_tuned, bsmr_plan_dense_choice).  Cases skip, with the amounts, where the
device or the host lacks the memory; on an MI355X none does."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GiB = 1 << 30
NONE = 0xFFFFFFFF


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _need(device_bytes, host_bytes=0):
    """skip unless the device has `device_bytes` free and the host `host_bytes` available"""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(_dev())
    if free < device_bytes:
        pytest.skip(f"needs {device_bytes / GiB:.1f} GiB of free device memory, {free / GiB:.1f} GiB free")
    avail = os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
    if avail < host_bytes:
        pytest.skip(f"needs {host_bytes / GiB:.1f} GiB of available host memory, {avail / GiB:.1f} GiB available")


def _log(msg):
    print(f"[extents] {msg}", flush=True)


# ---- operands ------------------------------------------------------------------------------------------------------
def fill(t, salt, row0=0):
    """t (rows, K) fp32 on the device: integers in [-15, 15], a hash of (row0 + row, k, salt)"""
    rows, K = t.shape
    k = torch.arange(K, device=t.device, dtype=torch.int64)[None, :]
    step = max(1, (1 << 24) // K)
    for r0 in range(0, rows, step):
        r = torch.arange(row0 + r0, row0 + min(rows, r0 + step), device=t.device, dtype=torch.int64)[:, None]
        h = (r * 1000003 + k * 7919 + salt * 104729 + 12345) % 2147483647
        t[r0:r0 + r.shape[0]] = (h % 31 - 15).to(torch.float32)


def operands(M, N, K, nb=1, salt=0):
    """A (nb, M, K), B (nb, N, K) fp32 on the device; batch b uses salts salt + 2b, salt + 2b + 1"""
    A = torch.empty((nb, M, K), dtype=torch.float32, device=_dev())
    B = torch.empty((nb, N, K), dtype=torch.float32, device=_dev())
    for b in range(nb):
        fill(A[b], salt + 2 * b)
        fill(B[b], salt + 2 * b + 1)
    return A, B


def nan_p(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=_dev())


# ---- references ----------------------------------------------------------------------------------------------------
def ref_entries(A, B, rows, cols, chunk=1 << 20):
    """fp64 dot products of the entries (rows[i], cols[i]) on the device; A (M, K), B (N, K)"""
    out = torch.empty(rows.numel(), dtype=torch.float64, device=_dev())
    for i in range(0, rows.numel(), chunk):
        a = A.index_select(0, rows[i:i + chunk]).double()
        b = B.index_select(0, cols[i:i + chunk]).double()
        out[i:i + chunk] = (a * b).sum(1)
    return out


def host_check(P, A, B, idx, row_of, col_of, where):
    """numpy fp64 on the host over the sampled entries idx (int64 array)"""
    idx = np.unique(np.asarray(idx, dtype=np.int64))
    r, c = row_of(idx), col_of(idx)
    ti = torch.from_numpy(idx).to(_dev())
    got = P.index_select(0, ti).cpu().numpy().astype(np.float64)
    a = A.index_select(0, torch.from_numpy(r).to(_dev())).cpu().numpy().astype(np.float64)
    b = B.index_select(0, torch.from_numpy(c).to(_dev())).cpu().numpy().astype(np.float64)
    want = np.einsum("ij,ij->i", a, b)
    bad = ~(got == want)
    assert not bad.any(), f"{where}: host sample wrong at {idx[bad][:10].tolist()}: got {got[bad][:5]}, want {want[bad][:5]}"


def mismatch(got, want):
    """indices (int64, device) where got != want (NaN included)"""
    return torch.nonzero(~(got.double() == want)).flatten()


# ---- plans ---------------------------------------------------------------------------------------------------------
def rphm_dense(R, N, drop_last=False, panel_chunk=64):
    """RPHM arrays of the fully dense R x N pattern in identity row order: every panel holds all N / 16 blocks, no residue
    (the last panel may be partial; drop_last leaves out entry (R - 1, N - 1)).  Built in uint32 straight from the layout:
    the CSR index of (row, col) is row * N + col."""
    assert N % 16 == 0
    P, NB = -(-R // 16), N // 16
    nnz = R * N - int(drop_last)
    assert nnz <= NONE
    bv = np.empty((P, NB, 16, 16), dtype=np.uint32)
    jj = np.arange(16, dtype=np.uint64)
    for p0 in range(0, P, panel_chunk):
        p1 = min(P, p0 + panel_chunk)
        row = (np.arange(p0 * 16, p1 * 16, dtype=np.uint64)).reshape(p1 - p0, 1, 16, 1)
        col = (np.arange(NB, dtype=np.uint64) * 16).reshape(1, NB, 1, 1) + jj.reshape(1, 1, 1, 16)
        v = row * np.uint64(N) + col
        v[np.broadcast_to(row >= R, v.shape)] = NONE
        bv[p0:p1] = v.astype(np.uint32)
    if drop_last:
        bv[(R - 1) // 16, NB - 1, (R - 1) % 16, 15] = NONE
    arrays = {"reorderedRows": np.arange(R, dtype=np.uint32),
              "denseCols": np.tile(np.arange(N, dtype=np.uint32), P),
              "blockOffsets": (np.arange(P + 1, dtype=np.uint64) * NB).astype(np.uint32),
              "blockValues": bv.reshape(-1),
              "sparseValueOffsets": np.zeros(P + 1, dtype=np.uint32),
              "sparseValues": np.zeros(0, np.uint32), "sparseRelativeRows": np.zeros(0, np.uint32),
              "sparseColIndices": np.zeros(0, np.uint32)}
    return arrays, nnz


def rphm_from_panels(M, N, panels):
    """RPHM arrays from a list of panels (rows [<= 16 row ids], blocks [(16 column ids, 16 x 16 bool mask)], residue
    [(row in panel, column)]); CSR indices follow from the sorted (row, column) entries.  Returns (arrays, rows, cols)
    with rows / cols the entries in CSR order."""
    ent = []
    for rows, blocks, residue in panels:
        for cols16, mask in blocks:
            for i, j in zip(*np.nonzero(mask)):
                ent.append((rows[i], cols16[j]))
        ent.extend((rows[i], c) for i, c in residue)
    key = np.array([r * N + c for r, c in ent], dtype=np.int64)
    assert np.unique(key).size == key.size, "an entry listed twice"
    order = np.sort(key)
    csr = {int(k): i for i, k in enumerate(order)}
    reordered, dense_cols, offsets, values = [], [], [0], []
    soff, sval, srow, scol = [0], [], [], []
    for rows, blocks, residue in panels:
        reordered.extend(rows)
        for cols16, mask in blocks:
            dense_cols.extend(cols16)
            bv = np.full((16, 16), NONE, dtype=np.uint32)
            for i, j in zip(*np.nonzero(mask)):
                bv[i, j] = csr[rows[i] * N + cols16[j]]
            values.append(bv.reshape(-1))
        offsets.append(offsets[-1] + len(blocks))
        for i, c in residue:
            sval.append(csr[rows[i] * N + c])
            srow.append(i)
            scol.append(c)
        soff.append(len(sval))
    u = lambda x: np.asarray(x, dtype=np.uint32)
    arrays = {"reorderedRows": u(reordered), "denseCols": u(dense_cols), "blockOffsets": u(offsets),
              "blockValues": np.concatenate(values).astype(np.uint32) if values else u([]),
              "sparseValueOffsets": u(soff), "sparseValues": u(sval), "sparseRelativeRows": u(srow),
              "sparseColIndices": u(scol)}
    return arrays, order // N, order % N


class Plan:
    def __init__(self, engine, M, N, nnz, arrays, dense_engine=None):
        self.engine, self.M, self.N, self.nnz = engine, M, N, nnz
        t0 = time.perf_counter()
        opts = engine.plan_options(dense_engine=engine.ENGINE_TUNED if dense_engine is None else dense_engine,
                                   fold_dense_below=0, promote_average=0)
        st, self.plan = engine.plan_from_arrays(M, N, nnz, arrays, device=0, options=opts)
        assert st == engine.OK, st
        self.build_s = time.perf_counter() - t0

    def close(self):
        if self.plan:
            self.engine.plan_destroy(self.plan)
            self.plan = None

    def stats(self):
        s = self.engine.PlanStats()
        assert self.engine.hip().bsmr_plan_get_stats(self.plan, C.byref(s)) == self.engine.OK
        return {k: getattr(s, k) for k, _ in self.engine.PlanStats._fields_}

    def dense_choice(self, K):
        g, t, u = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        assert self.engine.hip().bsmr_plan_dense_choice(self.plan, K, C.byref(g), C.byref(t), C.byref(u)) == self.engine.OK
        return g.value, t.value, u.value

    def tuned(self, K, mode):
        c = self.engine.TunedChoice()
        st = self.engine.hip().bsmr_plan_get_tuned(self.plan, K, mode, C.byref(c))
        return None if st != self.engine.OK else {n: getattr(c, n) for n, _ in self.engine.TunedChoice._fields_
                                                   if n != "struct_size"}

    def set_tuned(self, K, mode, choice):
        c = self.engine.TunedChoice()
        c.struct_size = C.sizeof(self.engine.TunedChoice)
        for n, v in choice.items():
            setattr(c, n, v)
        return self.engine.hip().bsmr_plan_set_tuned(self.plan, K, mode, C.byref(c))


def is_gemm(dc):
    """bsmr_plan_dense_choice of a GEMM call: PM panels, tiles = items PM NB, union = items (PM + NB) 16"""
    g, t, u = dc
    return g in (8, 16) and any(t % (g * nb) == 0 and u == t // (g * nb) * (g + nb) * 16 for nb in (8, 12, 16, 20))


def choice(engine_id, **kw):
    c = dict(engine=engine_id, group=0, blocks_per_item=0, format=-1, b_only=-1, overlap=-1, cvt_in_kernel=-1, waves=0)
    c.update(kw)
    return c


def engine_choices(engine, K):
    """(name, choice) of every engine this test installs at K"""
    out = [("stream-f0", choice(engine.ENGINE_STREAM, format=0)), ("stream-f1", choice(engine.ENGINE_STREAM, format=1)),
           ("tiles", choice(engine.ENGINE_TILES)), ("shared", choice(engine.ENGINE_SHARED)),
           ("sweep-16", choice(engine.ENGINE_SWEEP, cvt_in_kernel=0)), ("gemm-16", choice(engine.ENGINE_GEMM, cvt_in_kernel=0))]
    if K <= 128:
        out += [("sweep-fp32", choice(engine.ENGINE_SWEEP, cvt_in_kernel=1)),
                ("gemm-fp32", choice(engine.ENGINE_GEMM, cvt_in_kernel=1))]
    return out


def run_engines(engine, plan, K, modes, call, check, gemm_served, gemm_fp32_served=None):
    """Install every engine in turn, call, check.  gemm_served: whether the GEMM engine on the 16-bit copies must serve
    the plan (gemm_fp32_served: on the fp32 operands; None = as gemm_served).  A refused choice must leave the plan's
    choice as it was and the next call exact.  Returns the names served."""
    if gemm_fp32_served is None:
        gemm_fp32_served = gemm_served
    served = []
    for mode in modes:
        for name, c in engine_choices(engine, K):
            before = plan.tuned(K, mode)
            t0 = time.perf_counter()
            st = plan.set_tuned(K, mode, c)
            set_s = time.perf_counter() - t0
            where = f"{name} mode {mode}"
            if name.startswith("gemm") and st == engine.OK and not (gemm_served if name == "gemm-16" else gemm_fp32_served):
                try:   # served where it must be refused: what it computed goes into the message
                    check(call(mode), where)
                    found = "P exact"
                except AssertionError as e:
                    found = str(e).split("\n")[0]
                raise AssertionError(f"{where}: served, must be refused; {found}")
            if name.startswith("gemm"):
                assert (st == engine.OK) == (gemm_served if name == "gemm-16" else gemm_fp32_served), \
                    f"{where}: set_tuned returned {st}"
            if st != engine.OK:
                assert st in (engine.ERR_BAD_PLAN, engine.ERR_INVALID_ARG), f"{where}: set_tuned returned {st}"
                assert plan.tuned(K, mode) == before, f"{where}: a refused choice changed the plan"
                t0 = time.perf_counter()
                check(call(mode), f"{where} (refused, previous choice {before})")
                _log(f"{where}: refused ({st}), set {set_s:.1f} s, call + check {time.perf_counter() - t0:.1f} s")
                continue
            assert plan.tuned(K, mode) == c, where
            t0 = time.perf_counter()
            P = call(mode)
            dc = plan.dense_choice(K)
            assert is_gemm(dc) == name.startswith("gemm"), f"{where}: dense_choice {dc}"
            if name.startswith("stream"):
                s = plan.stats()
                want = (s["group_size"], s["num_dense_tiles"], s["union_columns"]) if c["format"] == 0 else \
                    (s["grouped_group_size"], s["grouped_dense_tiles"], s["grouped_union_columns"])
                assert dc == want, f"{where}: dense_choice {dc}, format {want}"
            check(P, where)
            served.append(name)
            _log(f"{where}: served, dense_choice {dc}, set {set_s:.1f} s, call + check {time.perf_counter() - t0:.1f} s")
    return served


def run_tuner(engine, plan, K, modes, tune, check, gemm_allowed):
    for mode in modes:
        t0 = time.perf_counter()
        P, report = tune(mode)
        tune_s = time.perf_counter() - t0
        _log(f"tuner mode {mode}: {report['chosen']} ({tune_s:.1f} s)")
        if not gemm_allowed:
            assert report["chosen"] != "gemm", f"mode {mode}: the tuner chose the GEMM engine"
            if mode != engine.COMPUTE_F32:
                assert not is_gemm(plan.dense_choice(K)), f"mode {mode}"
        check(P, f"tuned mode {mode} ({report['chosen']})")


# ---- 1. P past 4 GiB in one problem --------------------------------------------------------------------------------
def test_dense_builder_matches_pipeline(engine):
    """rphm_dense against the host pipeline over the same 48 x 64 pattern: same P bit for bit, and exact"""
    R, N, K = 48, 64, 64
    for drop_last in (False, True):
        ro = (np.arange(R + 1, dtype=np.int64) * N).astype(np.uint32)
        ci = np.tile(np.arange(N, dtype=np.uint32), R)
        if drop_last:
            ro[-1] -= 1
            ci = ci[:-1]
        csr = engine.CSR.from_arrays(R, N, ro, ci)
        pipe = engine.Pipeline(csr, alpha=0.3, delta=0.0, device=-1)
        arrays, nnz = rphm_dense(R, N, drop_last)
        assert nnz == ci.size
        A, B = operands(R, N, K)
        rows = torch.from_numpy(np.repeat(np.arange(R), np.diff(ro.astype(np.int64)))).to(_dev())
        want = ref_entries(A[0], B[0], rows, torch.from_numpy(ci.astype(np.int64)).to(_dev()))
        got = []
        for arr in (arrays, pipe.arrays()):
            plan = Plan(engine, R, N, nnz, arr)
            try:
                for mode in (0, 2):
                    P = nan_p(nnz)
                    engine.sddmm(plan.plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(), mode, _stream())
                    torch.cuda.synchronize()
                    assert mismatch(P, want).numel() == 0, (drop_last, mode)
                    got.append(P.cpu().numpy())
            finally:
                plan.close()
        assert np.array_equal(got[0].view(np.uint32), got[2].view(np.uint32))
        assert np.array_equal(got[1].view(np.uint32), got[3].view(np.uint32))


DENSE_PLANS = {   # rows, drop_last: nnz = rows * 32768 - drop_last
    "nnz-below-limit": (32768, True),
    "nnz-at-limit": (32768, False),
    "nnz-wrapping": (32769, False),
}


@pytest.mark.parametrize("name", list(DENSE_PLANS))
def test_p_past_4gib(engine, name):
    """Fully dense 32768-column plans of 2^30 - 1, 2^30 and 2^30 + 2^15 entries, K = 64: every engine and the tuner.
    The GEMM engine serves the first (its last entry, index 2^30 - 2, at byte offset 0xFFFFFFF8) and is refused for the
    other two; every entry is exact under every engine that serves a plan."""
    R, drop_last = DENSE_PLANS[name]
    N, K = 32768, 64
    nnz = R * N - int(drop_last)
    gemm_ok = nnz < 1 << 30
    p_bytes = nnz * 4
    _need(3 * p_bytes + 24 * GiB, 48 * GiB)
    t0 = time.perf_counter()
    arrays, n = rphm_dense(R, N, drop_last)
    assert n == nnz
    arrays_s = time.perf_counter() - t0
    plan = Plan(engine, R, N, nnz, arrays)
    del arrays
    _log(f"{name}: nnz {nnz}, arrays {arrays_s:.1f} s, plan build {plan.build_s:.1f} s")
    A, B = operands(R, N, K)
    A, B = A[0], B[0]
    Bd = B.double()
    boundary = [0, 1, N - 1, N, (1 << 30) - 2, (1 << 30) - 1, 1 << 30, nnz - 1, nnz - N, (1 << 30) + 1]
    boundary = [i for i in boundary if 0 <= i < nnz]
    sample = np.concatenate([boundary, np.random.default_rng(R).integers(0, nnz, 300)])

    def check(P, where):
        bad_count, bad_idx = 0, []
        step = 1024
        for r0 in range(0, R, step):
            r1 = min(R, r0 + step)
            e0, e1 = r0 * N, min(nnz, r1 * N)
            want = (A[r0:r1].double() @ Bd.T).flatten()[:e1 - e0]
            bad = mismatch(P[e0:e1], want)
            if bad.numel():
                bad_count += bad.numel()
                bad_idx.append(bad[:4].cpu().numpy() + e0)
                bad_idx.append(bad[-1:].cpu().numpy() + e0)
        if bad_count:
            idx = np.unique(np.concatenate(bad_idx))
            last = float(P[(1 << 30) - 1].item()) if nnz > (1 << 30) - 1 else None
            raise AssertionError(f"{name} {where}: {bad_count} wrong entries, e.g. {idx[:12].tolist()} (rows "
                                 f"{sorted(set((idx // N).tolist()))[:8]}); P[2^30 - 1] = {last}")
        host_check(P, A, B, sample, lambda i: i // N, lambda i: i % N, f"{name} {where}")

    P = nan_p(nnz)

    def call(mode):
        P.fill_(float("nan"))
        engine.sddmm(plan.plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(), mode, _stream())
        torch.cuda.synchronize()
        return P

    def tune(mode):
        P.fill_(float("nan"))
        report = engine.plan_tune(plan.plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(), mode, _stream())
        torch.cuda.synchronize()
        return P, report

    try:
        served = run_engines(engine, plan, K, (engine.COMPUTE_F16,), call, check, gemm_ok)
        assert {"stream-f0", "gemm-16" if gemm_ok else "stream-f0"} <= set(served)
        run_tuner(engine, plan, K, (engine.COMPUTE_F16, engine.COMPUTE_BF16, engine.COMPUTE_F32), tune, check, gemm_ok)
        plan.close()
        if not gemm_ok:
            # a plan built for the GEMM engine runs another one
            torch.cuda.empty_cache()
            arrays, _ = rphm_dense(R, N, drop_last)
            plan = Plan(engine, R, N, nnz, arrays, dense_engine=engine.ENGINE_GEMM)
            del arrays
            P2 = call(engine.COMPUTE_F16)
            assert not is_gemm(plan.dense_choice(K))
            check(P2, "plan built with dense_engine = GEMM")
    finally:
        plan.close()
        del P, A, B, Bd
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---- 2. operands past 4 GiB ----------------------------------------------------------------------------------------
def far_panels(M, N, seed):
    """5 panels: rows 0..15 and the last 64 rows; dense blocks on the first and last 16-column blocks and on columns
    N - 64.. N - 49 (masks of ~80 % of the cells), residue entries in the first and last 64 columns"""
    rng = np.random.default_rng(seed)
    row_sets = [list(range(16))] + [list(range(M - 64 + 16 * i, M - 48 + 16 * i)) for i in range(4)]
    col_blocks = [list(range(16)), list(range(N - 64, N - 48)), list(range(N - 16, N))]
    panels = []
    for pi, rows in enumerate(row_sets):
        blocks = [(cb, rng.random((16, 16)) < 0.8) for cb in col_blocks]
        if pi == 0 or pi == len(row_sets) - 1:
            blocks[-1][1][:] = True                 # the last row x last column cell in a dense block
            blocks[0][1][:] = True
        taken = set(c for cb in col_blocks for c in cb)
        cand = [c for c in list(range(64)) + list(range(N - 64, N)) if c not in taken]
        residue = [(i, c) for i in range(16) for c in rng.choice(cand, 6, replace=False).tolist()]
        panels.append((rows, blocks, residue))
    return panels


def _check_entries(A, B, rows, cols, name):
    tr = torch.from_numpy(rows.astype(np.int64)).to(_dev())
    tc = torch.from_numpy(cols.astype(np.int64)).to(_dev())
    want = ref_entries(A, B, tr, tc)
    nnz = rows.size
    far = np.nonzero((rows >= A.shape[0] - 64) | (cols >= B.shape[0] - 64))[0]
    sample = np.concatenate([[0, nnz - 1], far[:: max(1, far.size // 200)], far[-1:]])

    def check(P, where):
        bad = mismatch(P, want)
        assert bad.numel() == 0, (f"{name} {where}: {bad.numel()} wrong entries, e.g. rows "
                                  f"{rows[bad[:8].cpu().numpy()].tolist()} cols {cols[bad[:8].cpu().numpy()].tolist()}")
        host_check(P, A, B, sample, lambda i: rows[i], lambda i: cols[i], f"{name} {where}")
    return check


OPERAND_PLANS = {   # M = N, K, GEMM on the 16-bit copies served, GEMM on fp32 operands served (K <= 128)
    "K512-below": ((1 << 22) - 16, 512, True, None),
    "K512-at": (1 << 22, 512, False, None),
    "K128-fp32-below": ((1 << 23) - 16, 128, True, True),
    "K128-fp32-at": (1 << 23, 128, True, False),
}


@pytest.mark.parametrize("name", list(OPERAND_PLANS))
def test_operands_past_4gib(engine, name):
    """A and B of 4 to 8 GiB, entries in their first and last rows: gemmFits on both sides of its bound, every other
    engine and the residue (fp32 and from the converted copies) reading the far rows exactly"""
    MN, K, gemm16, gemm32 = OPERAND_PLANS[name]
    op_bytes = MN * K * 4
    _need(2 * op_bytes + op_bytes + 8 * GiB, 8 * GiB)
    arrays, rows, cols = rphm_from_panels(MN, MN, far_panels(MN, MN, seed=K))
    nnz = rows.size
    plan = Plan(engine, MN, MN, nnz, arrays)
    _log(f"{name}: nnz {nnz}, plan build {plan.build_s:.1f} s, operands {op_bytes / GiB:.1f} GiB each")
    A, B = operands(MN, MN, K, salt=K)
    A, B = A[0], B[0]
    check = _check_entries(A, B, rows, cols, name)
    P = nan_p(nnz)

    def call(mode):
        P.fill_(float("nan"))
        engine.sddmm(plan.plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(), mode, _stream())
        torch.cuda.synchronize()
        return P

    def tune(mode):
        P.fill_(float("nan"))
        report = engine.plan_tune(plan.plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(), mode, _stream())
        torch.cuda.synchronize()
        return P, report

    try:
        check(call(engine.COMPUTE_F32), "mode 2")
        served = run_engines(engine, plan, K, (engine.COMPUTE_F16, engine.COMPUTE_BF16), call, check, gemm16,
                             gemm32 if gemm32 is not None else False)
        assert "stream-f0" in served
        run_tuner(engine, plan, K, (engine.COMPUTE_F16, engine.COMPUTE_BF16, engine.COMPUTE_F32), tune, check,
                  gemm16)
    finally:
        plan.close()
        del P, A, B
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---- 3. batch offsets past 4 GiB -----------------------------------------------------------------------------------
def _batch_case(engine, name, plan, rows, cols, M, N, K, nb, check_batches):
    A, B = operands(M, N, K, nb=nb, salt=7)
    nnz = rows.size
    tr = torch.from_numpy(rows.astype(np.int64)).to(_dev())
    tc = torch.from_numpy(cols.astype(np.int64)).to(_dev())
    wants = {b: ref_entries(A[b], B[b], tr, tc) for b in check_batches}
    sample = np.concatenate([[0, nnz - 1], np.random.default_rng(nb).integers(0, nnz, 100)])
    P = nan_p(nb * nnz)

    def check(P, where):
        for b in check_batches:
            bad = mismatch(P[b * nnz:(b + 1) * nnz], wants[b])
            assert bad.numel() == 0, (f"{name} {where} batch {b} (P at {b * nnz * 4 / GiB:.2f} GiB, A at "
                                      f"{b * M * K * 4 / GiB:.2f} GiB): {bad.numel()} wrong entries, first "
                                      f"{bad[:6].cpu().numpy().tolist()}")
            host_check(P[b * nnz:(b + 1) * nnz], A[b], B[b], sample, lambda i: rows[i], lambda i: cols[i],
                       f"{name} {where} batch {b}")

    def call(mode):
        P.fill_(float("nan"))
        engine.sddmm_batch(plan.plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(), nb, mode, _stream())
        torch.cuda.synchronize()
        return P

    try:
        check(call(engine.COMPUTE_F32), "mode 2")
        served = run_engines(engine, plan, K, (engine.COMPUTE_F16,), call, check, True)
        assert "gemm-16" in served and "stream-f0" in served
    finally:
        del P, A, B
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def test_batch_p_past_4gib(engine):
    """bsmr_sddmm_batch: a hybrid plan of ~4 M entries, 1100 batches: P of the later batches lies past 4 GiB and past
    2^32 elements (18 GB)"""
    rows_, cols_, ro, ci = synth.bernoulli(rows=2048, cols=4096, density=0.5, seed=3)
    nnz = int(ci.size)
    K = 64
    nb = 1100
    assert (nb - 1) * nnz > 1 << 32
    _need(nb * nnz * 4 * 2 + 4 * GiB, 4 * GiB)
    csr = engine.CSR.from_arrays(rows_, cols_, ro, ci)
    arrays = engine.Pipeline(csr, alpha=0.3, delta=0.5, device=-1).arrays()   # (blocks of density ~0.5: about half dense)
    plan = Plan(engine, rows_, cols_, nnz, arrays)
    assert plan.stats()["num_sparse_entries"] > 0 and plan.stats()["num_dense_entries"] > 0
    rows = np.repeat(np.arange(rows_), np.diff(ro.astype(np.int64)))
    at_4gib, at_2e32 = (4 * GiB) // (nnz * 4), (1 << 32) // nnz   # the batches whose P straddles 4 GiB / 2^32 elements
    try:
        _batch_case(engine, "batch-P", plan, rows, ci.astype(np.int64), rows_, cols_, K, nb,
                    (0, at_4gib, at_4gib + 1, at_2e32, at_2e32 + 1, nb - 1))
    finally:
        plan.close()


def test_batch_operands_past_4gib(engine):
    """bsmr_sddmm_batch: M = N = 16384, K = 512, 260 batches: A and B (8.1 GiB each) and the contiguous 16-bit copies
    (4.1 GiB each) cross 4 GiB; entries in the far rows and columns"""
    M = N = 16384
    K, nb = 512, 260
    op = nb * M * K * 4
    _need(2 * op + op + 4 * GiB, 8 * GiB)
    arrays, rows, cols = rphm_from_panels(M, N, far_panels(M, N, seed=5))
    plan = Plan(engine, M, N, rows.size, arrays)
    per16 = M * K * 2
    check_batches = (0, (4 * GiB) // (M * K * 4) - 1, (4 * GiB) // (M * K * 4), (4 * GiB) // per16 - 1,
                     (4 * GiB) // per16, nb - 1)
    try:
        _batch_case(engine, "batch-operands", plan, rows, cols, M, N, K, nb, check_batches)
    finally:
        plan.close()


def test_batch_limits(engine):
    """num_batches = 65536 and K num_batches > 2^32 - 1 are refused before anything runs"""
    arrays, rows, cols = rphm_from_panels(256, 256, far_panels(256, 256, seed=1))
    plan = Plan(engine, 256, 256, rows.size, arrays)
    t = torch.zeros(1024, dtype=torch.float32, device=_dev())
    hip = engine.hip()
    try:
        assert hip.bsmr_sddmm_batch(plan.plan, 64, t.data_ptr(), t.data_ptr(), t.data_ptr(), 65536, 0, _stream()) == \
            engine.ERR_INVALID_ARG
        assert hip.bsmr_sddmm_batch(plan.plan, 1 << 17, t.data_ptr(), t.data_ptr(), t.data_ptr(), 1 << 15, 0,
                                    _stream()) == engine.ERR_INVALID_ARG
        torch.cuda.synchronize()
    finally:
        plan.close()


# ---- 4. caller-owned 16-bit copies past 4 GiB ----------------------------------------------------------------------
def test_lowp_copies_past_4gib(engine):
    """bsmr_convert_operands into caller-owned copies of 4 GiB + 64 KiB (M = N = 2^22 + 64, K = 512): the far rows of
    the copies lie past 4 GiB; bsmr_sddmm_lowp on them is exact under every engine that serves the plan"""
    MN, K = (1 << 22) + 64, 512
    op = MN * K * 4
    _need(2 * op + op + 8 * GiB, 8 * GiB)
    arrays, rows, cols = rphm_from_panels(MN, MN, far_panels(MN, MN, seed=9))
    plan = Plan(engine, MN, MN, rows.size, arrays)
    A, B = operands(MN, MN, K, salt=9)
    A, B = A[0], B[0]
    check = _check_entries(A, B, rows, cols, "lowp")
    A16 = torch.empty((MN, K), dtype=torch.float16, device=_dev())
    B16 = torch.empty((MN, K), dtype=torch.float16, device=_dev())
    assert (MN - 64) * K * 2 >= 4 * GiB
    P = nan_p(rows.size)

    def call(mode):
        engine.convert_operands(plan.plan, K, A.data_ptr(), B.data_ptr(), A16.data_ptr(), B16.data_ptr(), mode, _stream())
        P.fill_(float("nan"))
        engine.sddmm_lowp(plan.plan, K, A16.data_ptr(), B16.data_ptr(), A.data_ptr(), B.data_ptr(), P.data_ptr(), mode,
                          _stream())
        torch.cuda.synchronize()
        return P

    try:
        call(engine.COMPUTE_F16)
        # the converted far rows are the operands' values (integers: exact in fp16 and bf16)
        far = torch.arange(MN - 64, MN, device=_dev())
        assert torch.equal(A16.index_select(0, far).float(), A.index_select(0, far))
        assert torch.equal(B16.index_select(0, far).float(), B.index_select(0, far))
        served = run_engines(engine, plan, K, (engine.COMPUTE_F16, engine.COMPUTE_BF16), call, check, False, False)
        assert "stream-f0" in served
    finally:
        plan.close()
        del P, A, B, A16, B16
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
