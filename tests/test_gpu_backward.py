"""The SDDMM backward on the device (bsmr_spmm, bsmr_sddmm_backward; include/bsmr_hip.h "SDDMM backward").

What the numerical contract pins:
  * exact values: integer operands small enough that every partial sum is exact in fp32, so the result equals the fp64
    product (scipy.sparse) with ==, whatever the order of the sums;
  * exact placement: a one-hot v moves exactly one source row to exactly one destination, everything else is 0;
  * the error bound |Y - Y64| <= (n + 2) u sum|v||x| on U[0, 2) operands (n = list length, u = 2^-24);
  * bitwise reproducibility: call to call, stream to stream, batch to batch, any row_order, dP permuted or read in place;
  * chunked lists (longer than BSMR_BACKWARD_CHUNK) in both directions;
  * a NaN in v reaches exactly its destination row, in all K columns;
  * batches, graph capture after bsmr_backward_reserve, and the K rules."""
import numpy as np
import pytest
import scipy.sparse as sp

import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = (32, 64, 128, 256, 512)
U = 2.0 ** -24


def _dev():
    return torch.device("cuda:0")


class Pattern:
    def __init__(self, engine, name, rows, cols, ro, ci):
        self.name, self.rows, self.cols = name, rows, cols
        self.ro = np.ascontiguousarray(ro, dtype=np.uint32)
        self.ci = np.ascontiguousarray(ci, dtype=np.uint32)
        self.nnz = int(self.ci.size)
        self.row_of = np.repeat(np.arange(rows), np.diff(self.ro.astype(np.int64)))
        csr = engine.CSR.from_arrays(rows, cols, self.ro, self.ci)
        self.order = engine.Pipeline(csr, alpha=0.3, delta=0.3, device=-1).array("reorderedRows")
        self.bw = engine.backward_create(rows, cols, self.ro, self.ci, row_order=self.order, device=0)
        self.engine = engine

    def matrix(self, v):
        return sp.csr_matrix((np.asarray(v, np.float64), self.ci.astype(np.int64), self.ro.astype(np.int64)),
                             shape=(self.rows, self.cols))

    def row_len(self):
        return np.diff(self.ro.astype(np.int64))

    def col_len(self):
        return np.bincount(self.ci, minlength=self.cols)

    def close(self):
        self.engine.backward_destroy(self.bw)


def _chunk_pattern():
    """2 000 x 3 000 random, plus row 7 with 1 700 entries and column 11 in 1 700 rows (both > 3 x 512)."""
    rows, cols, ro, ci = synth.random_pattern(2000, 3000, 30000, seed=21, empty_rows=40)
    per_row = [set(ci[ro[r]:ro[r + 1]].tolist()) for r in range(rows)]
    rng = np.random.default_rng(5)
    per_row[7] |= set(rng.choice(cols, 1700, replace=False).tolist())
    for r in rng.choice(rows, 1700, replace=False):
        per_row[r].add(11)
    per_row = [np.array(sorted(p), dtype=np.uint32) for p in per_row]
    ro = np.zeros(rows + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([p.size for p in per_row])
    return rows, cols, ro, np.concatenate(per_row)


BUILDERS = {
    "nips": lambda: synth.nips_like(rows=320, cols=1500, nnz=40000, seed=1),
    "random_empty_rows": lambda: synth.random_pattern(300, 400, 9000, seed=3, empty_rows=23),
    "outlier_row": lambda: synth.outlier_row_pattern(groups=10, shared=64, long_row=2000, cols=8000, seed=7),
    "chunked": _chunk_pattern,
}


@pytest.fixture(scope="module")
def patterns(engine):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Pattern(engine, name, *BUILDERS[name]())
        return made[name]

    yield get
    for p in made.values():
        p.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _spmm(engine, p, K, transpose, v, X, nb=1, stream=None, bw=None):
    rows_y = p.cols if transpose else p.rows
    tv, tX = _t(v), _t(X)
    tY = torch.full((nb, rows_y, K), float("nan"), dtype=torch.float32, device=_dev())   # poisoned
    s = stream.cuda_stream if stream is not None else torch.cuda.current_stream(_dev()).cuda_stream
    engine.spmm(bw or p.bw, K, transpose, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), nb, s)
    torch.cuda.synchronize()
    return tY.cpu().numpy()[0] if nb == 1 else tY.cpu().numpy()


def _backward(engine, p, K, dP, A, B, nb=1, bw=None):
    tdP, tA, tB = _t(dP), _t(A), _t(B)
    tdA = torch.full((nb, p.rows, K), float("nan"), dtype=torch.float32, device=_dev())
    tdB = torch.full((nb, p.cols, K), float("nan"), dtype=torch.float32, device=_dev())
    engine.sddmm_backward(bw or p.bw, K, tdP.data_ptr(), tA.data_ptr(), tB.data_ptr(), tdA.data_ptr(), tdB.data_ptr(), nb,
                          torch.cuda.current_stream(_dev()).cuda_stream)
    torch.cuda.synchronize()
    dA, dB = tdA.cpu().numpy(), tdB.cpu().numpy()
    return (dA[0], dB[0]) if nb == 1 else (dA, dB)


def _ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ["nips", "random_empty_rows", "outlier_row"])
def test_exact_integer_operands(engine, patterns, name, K):
    p = patterns(name)
    rng = np.random.default_rng(K)
    v = _ints(rng, p.nnz)
    Xn, Xm = _ints(rng, (p.cols, K)), _ints(rng, (p.rows, K))
    S = p.matrix(v)
    assert np.array_equal(_spmm(engine, p, K, False, v, Xn), S @ Xn.astype(np.float64))
    assert np.array_equal(_spmm(engine, p, K, True, v, Xm), S.T @ Xm.astype(np.float64))
    dA, dB = _backward(engine, p, K, v, Xm, Xn)
    assert np.array_equal(dA, S @ Xn.astype(np.float64))
    assert np.array_equal(dB, S.T @ Xm.astype(np.float64))
    # destinations without entries are exact zeros (+0 or -0 compare equal; the poison is gone)
    assert np.all(dA[p.row_len() == 0] == 0) and np.all(dB[p.col_len() == 0] == 0)


@pytest.mark.parametrize("K", (64, 96, 128))
def test_exact_placement(engine, patterns, K):
    p = patterns("random_empty_rows")
    Xn = (np.arange(p.cols * K, dtype=np.float32) + 1).reshape(p.cols, K)
    Xm = (np.arange(p.rows * K, dtype=np.float32) + 1).reshape(p.rows, K)
    for e in np.random.default_rng(K).choice(p.nnz, 4, replace=False):
        v = np.zeros(p.nnz, np.float32)
        v[e] = 1.0
        r, c = p.row_of[e], p.ci[e]
        Y = _spmm(engine, p, K, False, v, Xn)
        assert np.array_equal(Y[r], Xn[c])
        Y[r] = 0
        assert np.all(Y == 0)
        Y = _spmm(engine, p, K, True, v, Xm)
        assert np.array_equal(Y[c], Xm[r])
        Y[c] = 0
        assert np.all(Y == 0)


def _check_bound(p, v, X, Y, transpose):
    S = p.matrix(v)
    S = S.T if transpose else S
    want = S @ X.astype(np.float64)
    mag = abs(S) @ np.abs(X.astype(np.float64))
    n = (p.col_len() if transpose else p.row_len()).astype(np.float64)[:, None]
    assert np.all(np.abs(Y.astype(np.float64) - want) <= (n + 2) * U * mag)


@pytest.mark.parametrize("name", ["nips", "outlier_row"])
def test_error_bound(engine, patterns, name):
    p = patterns(name)
    K = 128
    v = engine.make_data(p.nnz, 31)
    B = engine.make_data(p.cols * K, 32).reshape(p.cols, K)
    A = engine.make_data(p.rows * K, 33).reshape(p.rows, K)
    dA, dB = _backward(engine, p, K, v, A, B)
    _check_bound(p, v, B, dA, False)
    _check_bound(p, v, A, dB, True)


def test_bitwise_reproducible(engine, patterns, monkeypatch):
    p = patterns("chunked")
    K = 128
    v = engine.make_data(p.nnz, 41) - 1.0
    A = engine.make_data(p.rows * K, 42).reshape(p.rows, K) - 1.0
    B = engine.make_data(p.cols * K, 43).reshape(p.cols, K) - 1.0
    ref = _backward(engine, p, K, v, A, B)
    again = _backward(engine, p, K, v, A, B)
    s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    y1 = _spmm(engine, p, K, False, v, B, stream=s1)
    y2 = _spmm(engine, p, K, False, v, B, stream=s2)
    z1 = _spmm(engine, p, K, True, v, A, stream=s1)
    z2 = _spmm(engine, p, K, True, v, A, stream=s2)
    for x in (again[0], y1, y2):
        assert x.tobytes() == ref[0].tobytes()
    for x in (again[1], z1, z2):
        assert x.tobytes() == ref[1].tobytes()
    orders = {"natural": None, "random": np.random.default_rng(3).permutation(p.rows), "subset": p.order[::2].copy()}
    for name, order in orders.items():
        bw = engine.backward_create(p.rows, p.cols, p.ro, p.ci, row_order=order, device=0)
        try:
            got = _backward(engine, p, K, v, A, B, bw=bw)
        finally:
            engine.backward_destroy(bw)
        assert got[0].tobytes() == ref[0].tobytes(), name
        assert got[1].tobytes() == ref[1].tobytes(), name
    # dP read in place through csc_to_csr instead of permuted into CSC order by a pass of its own: the same bits
    assert engine.backward_stats(p.bw)["permute_values"] == 1
    monkeypatch.setenv("BSMR_BACKWARD_PERMUTE", "0")
    bw = engine.backward_create(p.rows, p.cols, p.ro, p.ci, row_order=p.order, device=0)
    try:
        assert engine.backward_stats(bw)["permute_values"] == 0
        got = _backward(engine, p, K, v, A, B, bw=bw)
    finally:
        engine.backward_destroy(bw)
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()


def test_chunked_lists(engine, patterns):
    p = patterns("chunked")
    st = engine.backward_stats(p.bw)
    chunk = st["chunk"]
    assert chunk == 512
    assert st["max_row_length"] > 3 * chunk and st["max_col_length"] > 3 * chunk
    assert st["split_rows"] >= 1 and st["split_cols"] >= 1
    assert st["row_items"] > p.rows and st["col_items"] > p.cols
    assert st["device_index_bytes"] >= 12 * p.nnz
    for K in (64, 256):
        rng = np.random.default_rng(K)
        v = _ints(rng, p.nnz)
        A, B = _ints(rng, (p.rows, K)), _ints(rng, (p.cols, K))
        S = p.matrix(v)
        dA, dB = _backward(engine, p, K, v, A, B)
        assert np.array_equal(dA, S @ B.astype(np.float64))
        assert np.array_equal(dB, S.T @ A.astype(np.float64))
    assert engine.backward_stats(p.bw)["workspace_bytes"] > 0


def test_reddit_like_shard_within_bound(engine):
    rows, cols, ro, ci = synth.reddit_shard_like(rows=2000, seed=3)
    p = Pattern(engine, "reddit", rows, cols, ro, ci)
    try:
        st = engine.backward_stats(p.bw)
        assert st["split_rows"] >= 1
        K = 64
        v = engine.make_data(p.nnz, 51)
        A = engine.make_data(p.rows * K, 52).reshape(p.rows, K)
        B = engine.make_data(p.cols * K, 53).reshape(p.cols, K)
        dA, dB = _backward(engine, p, K, v, A, B)
        _check_bound(p, v, B, dA, False)
        _check_bound(p, v, A, dB, True)
    finally:
        p.close()


def test_nan_reaches_exactly_its_destinations(engine, patterns):
    p = patterns("nips")
    K = 128
    v = engine.make_data(p.nnz, 61)
    A = engine.make_data(p.rows * K, 62).reshape(p.rows, K)
    B = engine.make_data(p.cols * K, 63).reshape(p.cols, K)
    e = p.nnz // 3
    v[e] = np.nan
    dA, dB = _backward(engine, p, K, v, A, B)
    r, c = p.row_of[e], p.ci[e]
    assert np.all(np.isnan(dA[r])) and np.all(np.isnan(dB[c]))
    assert np.isfinite(np.delete(dA, r, axis=0)).all()
    assert np.isfinite(np.delete(dB, c, axis=0)).all()


def test_batches_equal_single_calls(engine, patterns):
    p = patterns("chunked")
    K, nb = 64, 3
    v = np.stack([engine.make_data(p.nnz, 70 + b) for b in range(nb)])
    A = np.stack([engine.make_data(p.rows * K, 80 + b).reshape(p.rows, K) for b in range(nb)])
    B = np.stack([engine.make_data(p.cols * K, 90 + b).reshape(p.cols, K) for b in range(nb)])
    dA, dB = _backward(engine, p, K, v, A, B, nb=nb)
    Yt = _spmm(engine, p, K, True, v, A, nb=nb)
    for b in range(nb):
        a1, b1 = _backward(engine, p, K, v[b], A[b], B[b])
        assert dA[b].tobytes() == a1.tobytes() and dB[b].tobytes() == b1.tobytes()
        assert Yt[b].tobytes() == b1.tobytes()


def test_graph_capture_after_reserve(engine, patterns):
    p = patterns("chunked")
    K = 128
    dev = _dev()
    tv = _t(engine.make_data(p.nnz, 101))
    tA = _t(engine.make_data(p.rows * K, 102).reshape(p.rows, K))
    tB = _t(engine.make_data(p.cols * K, 103).reshape(p.cols, K))
    tdA = torch.empty((p.rows, K), dtype=torch.float32, device=dev)
    tdB = torch.empty((p.cols, K), dtype=torch.float32, device=dev)
    bw = engine.backward_create(p.rows, p.cols, p.ro, p.ci, row_order=p.order, device=0)
    try:
        engine.backward_reserve(bw, K, 1)
        reserved = engine.backward_stats(bw)["workspace_bytes"]
        side = torch.cuda.Stream(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            engine.sddmm_backward(bw, K, tv.data_ptr(), tA.data_ptr(), tB.data_ptr(), tdA.data_ptr(), tdB.data_ptr(), 1,
                                  side.cuda_stream)
            side.synchronize()
            want = (tdA.cpu().numpy().tobytes(), tdB.cpu().numpy().tobytes())
            with torch.cuda.graph(graph, stream=side):
                engine.sddmm_backward(bw, K, tv.data_ptr(), tA.data_ptr(), tB.data_ptr(), tdA.data_ptr(), tdB.data_ptr(),
                                      1, torch.cuda.current_stream(dev).cuda_stream)
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


def test_k_rules(engine, patterns):
    p = patterns("random_empty_rows")
    hip = engine.hip()
    t = torch.zeros(max(p.rows, p.cols) * 64 + p.nnz, dtype=torch.float32, device=_dev())
    ptr = t.data_ptr()
    assert hip.bsmr_spmm(p.bw, 48, 0, ptr, ptr, ptr, 1, None) == engine.ERR_UNSUPPORTED_K
    assert hip.bsmr_spmm(p.bw, 0, 0, ptr, ptr, ptr, 1, None) == engine.ERR_UNSUPPORTED_K
    assert hip.bsmr_sddmm_backward(p.bw, 48, ptr, ptr, ptr, ptr, None, 1, None) == engine.ERR_UNSUPPORTED_K
    assert hip.bsmr_backward_reserve(p.bw, 48, 1) == engine.ERR_UNSUPPORTED_K
    K = 96
    rng = np.random.default_rng(96)
    v = _ints(rng, p.nnz)
    A, B = _ints(rng, (p.rows, K)), _ints(rng, (p.cols, K))
    S = p.matrix(v)
    dA, dB = _backward(engine, p, K, v, A, B)
    assert np.array_equal(dA, S @ B.astype(np.float64)) and np.array_equal(dB, S.T @ A.astype(np.float64))
