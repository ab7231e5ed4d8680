"""The sparse row softmax on the device (include/bsmr_hip.h "Sparse row softmax"), on handles from
bsmr_backward_create:
  * exact cases: single entries, rows of 2^k equal values, -inf entries, all -inf rows, NaN / +inf rows that leave every
    other row bitwise unchanged, +-1e30 inputs with large and small scale;
  * the forward against fp64 under the header's bound (and each row's sum against 1), on a random pattern with empty rows,
    on rows of 1 .. 60 000 entries around the wave and chunk boundaries, and on the reddit-like shard;
  * the backward bit for bit against its fp32 twin (tests/softmax_twin.py), NaN in dY included;
  * determinism: repeated calls, natural vs clustered row_order, batch vs single calls, two streams, in place vs not;
  * graph capture after bsmr_backward_reserve: nothing allocated, identical bits on replay;
  * nnz = 0 with NULL pointers; a batch whose values pass 2^30 floats (its own test, deselectable)."""
import numpy as np
import pytest

import synth
from gather_twin import assert_twin
from softmax_twin import backward_twin, check_forward, row_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LENGTHS = (1, 63, 64, 65, 511, 512, 513, 1025, 60000)


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def lengths_pattern():
    """rows of LENGTHS entries interleaved with empty rows and short ones, columns 0 .. n-1"""
    lens = []
    for n in LENGTHS:
        lens += [n, 0, 2, 7]
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    ci = np.concatenate([np.arange(n) for n in lens]).astype(np.uint32)
    return len(lens), 60000, ro, ci


PATTERNS = {
    "random_empty_rows": lambda: synth.random_pattern(300, 200, 6000, seed=3, empty_rows=40),
    "lengths": lengths_pattern,
    "reddit_shard": lambda: synth.reddit_shard_like(),
}


class Pat:
    def __init__(self, engine, rows, cols, ro, ci):
        self.engine, self.rows, self.cols = engine, rows, cols
        self.ro = np.ascontiguousarray(ro, dtype=np.uint32)
        self.ci = np.ascontiguousarray(ci, dtype=np.uint32)
        self.nnz = int(self.ci.size)
        self.bw = engine.backward_create(rows, cols, self.ro, self.ci, device=0)

    def forward(self, x, scale, nb=1, bw=None):
        tx = _t(x)
        ty = torch.full_like(tx, float("nan"))
        self.engine.sparse_softmax(bw or self.bw, scale, tx.data_ptr(), ty.data_ptr(), nb, _stream())
        torch.cuda.synchronize()
        return ty.cpu().numpy()

    def backward(self, y, dY, scale, nb=1):
        ty, td = _t(y), _t(dY)
        tdx = torch.full_like(td, float("nan"))
        self.engine.sparse_softmax_backward(self.bw, scale, ty.data_ptr(), td.data_ptr(), tdx.data_ptr(), nb, _stream())
        torch.cuda.synchronize()
        return tdx.cpu().numpy()


@pytest.fixture(scope="module")
def pats(engine):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Pat(engine, *PATTERNS[name]())
        return made[name]

    yield get
    for p in made.values():
        engine.backward_destroy(p.bw)


def _rows(engine, rows_values):
    ro = np.cumsum([0] + [len(r) for r in rows_values]).astype(np.uint32)
    ci = np.concatenate([np.arange(len(r)) for r in rows_values] + [np.zeros(0)]).astype(np.uint32)
    x = np.array([v for r in rows_values for v in r], np.float32)
    return Pat(engine, len(rows_values), max(1, max(len(r) for r in rows_values)), ro, ci), x


# ---- 1. exact cases ------------------------------------------------------------------------------------------------
def test_exact_values(engine):
    inf, nan = np.inf, np.nan
    rows = [[5.0], [-3e30], [7.0] * 2, [-1.5] * 8, [0.25] * 64, [3.0] * 512, [1.0] * 1024, [2.0] * 4096,
            [1.0, -inf, 1.0, -inf], [-inf] * 3, [-inf] * 700, [2.0] + [-inf] * 600, [nan, -inf, -inf], [nan],
            [1.0, inf, 2.0], [inf] * 3, [-inf, 4.0], []]
    p, x = _rows(engine, rows)
    try:
        y = p.forward(x, 1.0)
        r = row_of(p.ro)
        row = lambda i: y[r == i]
        assert row(0).tolist() == [1.0] and row(1).tolist() == [1.0]
        for i, k in ((2, 1), (3, 3), (4, 6), (5, 9), (6, 10), (7, 12)):
            assert (row(i) == np.float32(2.0 ** -k)).all(), (i, row(i)[:4])
        assert row(8).tolist() == [0.5, 0.0, 0.5, 0.0]
        assert (row(9).view(np.uint32) == 0).all() and (row(10).view(np.uint32) == 0).all()   # exact +0
        assert row(11)[0] == 1.0 and (row(11)[1:] == 0).all()
        for i in (12, 13, 14, 15):
            assert np.isnan(row(i)).all(), i
        assert row(16).tolist() == [0.0, 1.0]
        # all -inf rows: zero gradient
        dY = np.random.default_rng(0).standard_normal(x.size).astype(np.float32)
        dx = p.backward(y, dY, 0.5)
        assert (row_of(p.ro) == 9).sum() == 3
        assert (dx[r == 9] == 0).all() and (dx[r == 10] == 0).all()
    finally:
        engine.backward_destroy(p.bw)


def test_nonfinite_rows_touch_no_other_row(engine, pats):
    p = pats("lengths")
    rng = np.random.default_rng(1)
    x = rng.standard_normal(p.nnz).astype(np.float32) * 4
    clean = p.forward(x, 0.7)
    r = row_of(p.ro)
    lens = np.diff(p.ro.astype(np.int64))
    for value in (np.nan, np.inf):
        x2 = x.copy()
        hit = [i for i in range(p.rows) if lens[i] > 0][::3]
        for i in hit:
            x2[p.ro[i] + (lens[i] - 1) // 2] = value
        y = p.forward(x2, 0.7)
        bad = np.isin(r, hit)
        assert np.isnan(y[bad]).all()
        assert (y[~bad].view(np.uint32) == clean[~bad].view(np.uint32)).all()


@pytest.mark.parametrize("scale", [1e8, 1.0, 1e-30])
def test_huge_inputs_do_not_overflow(engine, scale):
    """+-1e30 with scale 1e8 (z = +-1e38, z - m passes the fp32 range), 1 and 1e-30 (z ~ 1): finite, bounded, summing
    to 1"""
    rng = np.random.default_rng(2)
    rows = [list(rng.choice([-1e30, 1e30, 5e29, -7e29], n)) for n in (1, 2, 5, 64, 100, 513, 700)]
    p, x = _rows(engine, rows)
    try:
        y = p.forward(x, scale)
        assert np.isfinite(y).all()
        check_forward(p.ro, x, scale, y, f"scale {scale}")
    finally:
        engine.backward_destroy(p.bw)


# ---- 2. the forward under the bound, the backward bit for bit ------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_forward_bound_and_backward_twin(engine, oracle, pats, name):
    p = pats(name)
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(p.nnz) * 6).astype(np.float32)
    scale = 0.37
    y = p.forward(x, scale)
    r = row_of(p.ro)
    assert (np.diff(p.ro.astype(np.int64)) == 0).any() or name == "reddit_shard"
    check_forward(p.ro, x, scale, y, name)
    dY = rng.standard_normal(p.nnz).astype(np.float32)
    if name != "reddit_shard":
        dY[p.ro[np.nonzero(np.diff(p.ro.astype(np.int64)) > 3)[0][::5]] + 1] = np.nan   # NaN in dY on some rows
    dx = p.backward(y, dY, scale)
    assert_twin(dx, backward_twin(oracle, p.ro, y, dY, scale), f"{name} backward")
    assert r.size == p.nnz


# ---- 3. determinism -----------------------------------------------------------------------------------------------
def test_determinism(engine, pats):
    p = pats("lengths")
    rng = np.random.default_rng(4)
    nb = 3
    x = (rng.standard_normal((nb, p.nnz)) * 5).astype(np.float32)
    dY = rng.standard_normal((nb, p.nnz)).astype(np.float32)
    scale = 1.3
    csr = engine.CSR.from_arrays(p.rows, p.cols, p.ro, p.ci)
    order = engine.Pipeline(csr, alpha=0.3, delta=0.3, device=-1).array("reorderedRows")
    clustered = engine.backward_create(p.rows, p.cols, p.ro, p.ci, row_order=order, device=0)
    try:
        y = p.forward(x, scale, nb)
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
        assert (bits(p.forward(x, scale, nb)) == bits(y)).all()
        assert (bits(p.forward(x, scale, nb, bw=clustered)) == bits(y)).all()
        for b in range(nb):
            assert (bits(p.forward(x[b], scale)) == bits(y[b])).all()
        dx = p.backward(y, dY, scale, nb)
        for b in range(nb):
            assert (bits(p.backward(y[b], dY[b], scale)) == bits(dx[b])).all()
        # in place: Y = X, dX = dY
        tx, td, ty = _t(x), _t(dY), _t(y)
        engine.sparse_softmax(p.bw, scale, tx.data_ptr(), tx.data_ptr(), nb, _stream())
        engine.sparse_softmax_backward(p.bw, scale, ty.data_ptr(), td.data_ptr(), td.data_ptr(), nb, _stream())
        torch.cuda.synchronize()
        assert (bits(tx.cpu().numpy()) == bits(y)).all() and (bits(td.cpu().numpy()) == bits(dx)).all()
        # two streams
        s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
        tx = _t(x)
        o1, o2 = torch.empty_like(tx), torch.empty_like(tx)
        torch.cuda.synchronize()
        engine.sparse_softmax(p.bw, scale, tx.data_ptr(), o1.data_ptr(), nb, s1.cuda_stream)
        engine.sparse_softmax(clustered, scale, tx.data_ptr(), o2.data_ptr(), nb, s2.cuda_stream)
        torch.cuda.synchronize()
        assert (bits(o1.cpu().numpy()) == bits(y)).all() and (bits(o2.cpu().numpy()) == bits(y)).all()
    finally:
        engine.backward_destroy(clustered)


# ---- 4. capture, empty pattern -------------------------------------------------------------------------------------
def test_graph_capture_allocates_nothing(engine, pats):
    p = pats("lengths")
    nb = 2
    engine.backward_reserve(p.bw, 32, nb)
    before = engine.backward_stats(p.bw)["workspace_bytes"]
    rng = np.random.default_rng(5)
    tx = _t(rng.standard_normal((nb, p.nnz)).astype(np.float32))
    td = _t(rng.standard_normal((nb, p.nnz)).astype(np.float32))
    ty, tdx = torch.empty_like(tx), torch.empty_like(tx)
    s = torch.cuda.Stream(_dev())
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        engine.sparse_softmax(p.bw, 0.9, tx.data_ptr(), ty.data_ptr(), nb, s.cuda_stream)
        engine.sparse_softmax_backward(p.bw, 0.9, ty.data_ptr(), td.data_ptr(), tdx.data_ptr(), nb, s.cuda_stream)
    assert engine.backward_stats(p.bw)["workspace_bytes"] == before
    g.replay()
    torch.cuda.synchronize()
    y1, dx1 = ty.cpu().numpy(), tdx.cpu().numpy()
    ty.fill_(float("nan"))
    tdx.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert (ty.cpu().numpy().view(np.uint32) == y1.view(np.uint32)).all()
    assert (tdx.cpu().numpy().view(np.uint32) == dx1.view(np.uint32)).all()
    want = p.forward(tx.cpu().numpy(), 0.9, nb)
    assert (want.view(np.uint32) == y1.view(np.uint32)).all()


def test_empty_pattern_with_null_pointers(engine):
    bw = engine.backward_create(5, 7, np.zeros(6, np.uint32), np.zeros(0, np.uint32), device=0)
    hip = engine.hip()
    try:
        for nb in (1, 2):
            assert hip.bsmr_sparse_softmax(bw, 1.0, None, None, nb, _stream()) == engine.OK
            assert hip.bsmr_sparse_softmax_backward(bw, 1.0, None, None, None, nb, _stream()) == engine.OK
        torch.cuda.synchronize()
    finally:
        engine.backward_destroy(bw)


# ---- 5. a batch past 2^30 floats -----------------------------------------------------------------------------------
def test_large_batch_past_4gib(engine, pats):
    """b * nnz > 2^30: values past 4 GiB (the last batches' offsets need 64 bits) match the per-batch result.  This covers
    byte offsets: b * nnz stays below 2^31 entries; b * nnz past 2^32 entries is case V of
    tests/test_gpu_backward_extents.py."""
    p = pats("lengths")
    nb = (1 << 30) // p.nnz + 2
    assert nb * p.nnz > 1 << 30 and nb <= 65535
    need = 3 * nb * p.nnz * 4 + (1 << 30)
    free, _ = torch.cuda.mem_get_info(_dev())
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")
    rng = np.random.default_rng(6)
    one = _t((rng.standard_normal(p.nnz) * 3).astype(np.float32))
    dY = _t(rng.standard_normal(p.nnz).astype(np.float32))
    scales = torch.linspace(0.5, 1.5, nb, device=_dev()).view(nb, 1)
    X = (one.view(1, -1) * scales).contiguous()           # batch b: x * scale_b, generated on the device
    Y = torch.empty_like(X)
    s = _stream()
    engine.sparse_softmax(p.bw, 0.8, X.data_ptr(), Y.data_ptr(), nb, s)
    dYb = dY.view(1, -1).expand(nb, -1).contiguous()
    dX = torch.empty_like(X)
    engine.sparse_softmax_backward(p.bw, 0.8, Y.data_ptr(), dYb.data_ptr(), dX.data_ptr(), nb, s)
    torch.cuda.synchronize()
    del dYb
    y1, dx1 = torch.empty_like(one), torch.empty_like(one)
    for b in (0, nb // 2, nb - 2, nb - 1):
        engine.sparse_softmax(p.bw, 0.8, X[b].data_ptr(), y1.data_ptr(), 1, s)
        engine.sparse_softmax_backward(p.bw, 0.8, Y[b].data_ptr(), dY.data_ptr(), dx1.data_ptr(), 1, s)
        torch.cuda.synchronize()
        assert torch.equal(Y[b].view(torch.int32), y1.view(torch.int32)), b
        assert torch.equal(dX[b].view(torch.int32), dx1.view(torch.int32)), b
    assert (nb - 1) * p.nnz * 4 >= 4 << 30
    del X, Y, dX
    torch.cuda.empty_cache()
