"""The SDDMM backward on the device, bit for bit against its fp32 twin (oracle/spmm_oracle.c via tests/gather_twin.py).

include/bsmr_hip.h "SDDMM backward" and DESIGN section 9 state the arithmetic: each destination is a sequential fp32 fma
chain over its list in list order from +0 (CSR order for rows, ascending row for columns), and a list longer than
BSMR_BACKWARD_CHUNK is summed chunk by chunk with the partials added left to right.  tests/test_gpu_backward.py checks
exact integers, an error bound and self-consistency, none of which sees the order or the fma.  Here every output
element of bsmr_spmm (both directions) and bsmr_sddmm_backward (dA and dB) must equal the twin's bits (a NaN of the twin
may be any NaN), on operands chosen so that order and rounding show:
  * every slice width W, with one slice and with several (K matrix);
  * a pattern whose row and column lengths sit on the kernel's boundaries (4-entry steps, the G-entry load groups, the
    chunk length and its multiples), interleaved so that narrow-group waves mix long and short items;
  * wide exponent ranges, cancellation, hand-derived vectors planted in real lists, subnormals and underflow, overflow
    inside a chunk and only across chunks, +-inf and NaN in X;
  * row_order, the dP permutation pass on and off, batches;
  * addresses past 4 GiB, in a source, in an output and across a batch offset;
  * an empty pattern called with NULL operands.
The lists of the twin come from numpy (gather_twin.row_lists / col_lists), never from the library."""
import numpy as np
import pytest

import synth
from gather_twin import CHUNK, assert_twin, col_lists, gather, row_lists

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = (32, 64, 96, 128, 160, 192, 256, 384, 480, 640, 768, 1024)
BOUNDARY = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1537)
A12 = np.float32(1 + 2.0 ** -12)


def _dev():
    return torch.device("cuda:0")


def _items(lists):
    n = np.diff(lists[0].astype(np.int64))
    return int(np.maximum(1, -(-n // CHUNK)).sum())


class Pattern:
    def __init__(self, engine, name, rows, cols, ro, ci, row_order="clustered"):
        self.engine, self.name, self.rows, self.cols = engine, name, rows, cols
        self.ro = np.ascontiguousarray(ro, dtype=np.uint32)
        self.ci = np.ascontiguousarray(ci, dtype=np.uint32)
        self.nnz = int(self.ci.size)
        self.rl = row_lists(self.ro, self.ci)
        self.cl = col_lists(rows, cols, self.ro, self.ci)
        self.bw = self.create(row_order)

    def create(self, row_order):
        if row_order == "clustered":
            csr = self.engine.CSR.from_arrays(self.rows, self.cols, self.ro, self.ci)
            order = self.engine.Pipeline(csr, alpha=0.3, delta=0.3, device=-1).array("reorderedRows")
        elif row_order == "reversed":
            order = np.arange(self.rows)[::-1]
        else:
            order = None
        return self.engine.backward_create(self.rows, self.cols, self.ro, self.ci, row_order=order, device=0)

    def close(self):
        self.engine.backward_destroy(self.bw)


def boundary_pattern(seed=0):
    """Rows with every length of BOUNDARY (twice) over one set of columns, columns with every length of BOUNDARY (twice)
    over a disjoint set of rows.  Row and column ids are shuffled, so the long and short lists of either direction sit
    side by side in the schedule; one spare empty row / column makes both item counts odd."""
    rng = np.random.default_rng(seed)
    L = np.array(BOUNDARY * 2)
    pool = 1600                                     # columns of the row block = rows of the column block (> 1537)
    rows, cols = L.size + pool, pool + L.size
    for extra_r in (0, 1):
        for extra_c in (0, 1):
            R, Cn = rows + extra_r, cols + extra_c
            rid, cid = rng.permutation(R), rng.permutation(Cn)
            r_block, r_pool = rid[:L.size], rid[L.size:L.size + pool]
            c_pool, c_block = cid[:pool], cid[pool:pool + L.size]
            per_row = [set() for _ in range(R)]
            for r, n in zip(r_block, L):
                per_row[r].update(c_pool[rng.choice(pool, n, replace=False)].tolist())
            for c, n in zip(c_block, L):
                for r in r_pool[rng.choice(pool, n, replace=False)]:
                    per_row[r].add(int(c))
            per_row = [np.array(sorted(s), dtype=np.uint32) for s in per_row]
            ro = np.zeros(R + 1, dtype=np.uint32)
            ro[1:] = np.cumsum([p.size for p in per_row])
            ci = np.concatenate(per_row)
            if _items(row_lists(ro, ci)) % 2 and _items(col_lists(R, Cn, ro, ci)) % 2:
                return R, Cn, ro, ci
    raise AssertionError("no odd item counts")


def _chunked():
    from test_gpu_backward import BUILDERS
    return BUILDERS["chunked"]()


BUILDERS = {
    "boundary": boundary_pattern,
    "nips": lambda: synth.nips_like(rows=320, cols=1500, nnz=40000, seed=1),
    "outlier_row": lambda: synth.outlier_row_pattern(groups=10, shared=64, long_row=2000, cols=8000, seed=7),
    "chunked": _chunked,
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


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=_dev())   # poisoned: every element is written


def device_all(engine, p, K, v, Xn, Xm, nb=1, bw=None):
    """bsmr_spmm in both directions and bsmr_sddmm_backward (dA, dB) on one set of operands:
    Y_rows = S_v Xn = dA (B = Xn), Y_cols = S_v^T Xm = dB (A = Xm)"""
    bw = bw or p.bw
    lead = (nb,) if nb > 1 else ()
    tv, tXn, tXm = _t(v), _t(Xn), _t(Xm)
    out = {k: _nan(*lead, p.rows if k in ("rows", "dA") else p.cols, K) for k in ("rows", "cols", "dA", "dB")}
    s = torch.cuda.current_stream(_dev()).cuda_stream
    engine.spmm(bw, K, False, tv.data_ptr(), tXn.data_ptr(), out["rows"].data_ptr(), nb, s)
    engine.spmm(bw, K, True, tv.data_ptr(), tXm.data_ptr(), out["cols"].data_ptr(), nb, s)
    engine.sddmm_backward(bw, K, tv.data_ptr(), tXm.data_ptr(), tXn.data_ptr(), out["dA"].data_ptr(),
                          out["dB"].data_ptr(), nb, s)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


def check(engine, oracle, p, K, v, Xn, Xm, where, nb=1, bw=None):
    """every output element of the four products against the twin; returns (twin_rows, twin_cols) of batch 0"""
    got = device_all(engine, p, K, v, Xn, Xm, nb=nb, bw=bw)
    twins = []
    for b in range(nb):
        vb, Xnb, Xmb = (v, Xn, Xm) if nb == 1 else (v[b], Xn[b], Xm[b])
        tr, tc = gather(oracle, p.rl, vb, Xnb), gather(oracle, p.cl, vb, Xmb)
        sel = (lambda a: a) if nb == 1 else (lambda a, b=b: a[b])
        for k, want in (("rows", tr), ("dA", tr), ("cols", tc), ("dB", tc)):
            assert_twin(sel(got[k]), want, f"{p.name} K={K} {where} batch {b}: {k}")
        twins.append((tr, tc))
    return twins[0]


# ---- operands ------------------------------------------------------------------------------------------------------
def wide(rng, shape, lo=-30, hi=30):
    """+-m 2^e with a full 24-bit m and e in [lo, hi] (below 2^-126 the cast to fp32 rounds to a subnormal)"""
    m = rng.integers(1 << 23, 1 << 24, size=shape).astype(np.float64)
    s = rng.choice([-1.0, 1.0], size=shape)
    return (s * np.ldexp(m, rng.integers(lo, hi + 1, size=shape) - 23)).astype(np.float32)


def narrow(rng, shape):
    """+-m 2^e with e in [-4, 4]: the products of a list are of one size, so every order and every rounding shows (with
    e over [-30, 30] the largest product of a list dominates its sum and hides most of them)"""
    return wide(rng, shape, -4, 4)


def _position(lists, nnz):
    """position of every CSR entry within its list of this direction"""
    offsets, _, eidx = lists
    pos = np.empty(nnz, dtype=np.int64)
    n = np.diff(offsets.astype(np.int64))
    pos[eidx] = np.arange(nnz) - np.repeat(offsets[:-1].astype(np.int64), n)
    return pos


def _lengths(lists):
    return np.diff(lists[0].astype(np.int64))


def _subnormal(a):
    return (a != 0) & (np.abs(a) < np.float32(2.0 ** -126))


def _chunk_partials(oracle, lists, v, X):
    """every chunk of every list as a destination of its own: the partials spmmReduce adds"""
    offsets, src, eidx = lists
    bounds, owner = [], []
    for d, (b, e) in enumerate(zip(offsets[:-1].tolist(), offsets[1:].tolist())):
        starts = range(b, e, CHUNK) if e > b else [b]
        bounds.extend(starts)
        owner.extend([d] * len(starts))
    bounds.append(int(offsets[-1]))
    return gather(oracle, (np.array(bounds, np.uint32), src, eidx), v, X, chunk=0), np.array(owner)


# ---- 1. every slice width, one slice and several ------------------------------------------------------------------
def test_boundary_pattern_shape(engine, patterns):
    p = patterns("boundary")
    rl, cl = _lengths(p.rl), _lengths(p.cl)
    assert set(BOUNDARY) <= set(rl.tolist()) and set(BOUNDARY) <= set(cl.tolist())
    st = engine.backward_stats(p.bw)
    assert st["row_items"] == _items(p.rl) and st["col_items"] == _items(p.cl)
    assert st["row_items"] % 2 == 1 and st["col_items"] % 2 == 1    # units per block (4, 16, 32) never divide the units
    assert st["max_row_length"] == st["max_col_length"] == 1537


@pytest.mark.parametrize("K", KS)
def test_k_matrix(engine, oracle, patterns, K):
    p = patterns("boundary")
    rng = np.random.default_rng(K)
    for gen, where in ((narrow, "narrow"), (wide, "wide")):
        check(engine, oracle, p, K, gen(rng, p.nnz), gen(rng, (p.cols, K)), gen(rng, (p.rows, K)), where)


@pytest.mark.parametrize("K", (160, 640))
@pytest.mark.parametrize("name", ["nips", "outlier_row", "chunked"])
def test_existing_builders(engine, oracle, patterns, name, K):
    p = patterns(name)
    rng = np.random.default_rng(K + 1)
    check(engine, oracle, p, K, narrow(rng, p.nnz), narrow(rng, (p.cols, K)), narrow(rng, (p.rows, K)), "narrow")


# ---- 2. operand classes -------------------------------------------------------------------------------------------
CLASS_KS = (32, 192, 768)


@pytest.mark.parametrize("K", CLASS_KS)
def test_cancellation(engine, oracle, patterns, K):
    """X near 2^20 plus a few units, v = +-(1 + small) alternating along the list: the running sum swings by 2^20 at
    every step and the final value is small, so every rounding of the chain is visible"""
    p = patterns("boundary")
    rng = np.random.default_rng(3 * K)
    Xn = (2.0 ** 20 + rng.uniform(-8, 8, (p.cols, K))).astype(np.float32)
    Xm = (2.0 ** 20 + rng.uniform(-8, 8, (p.rows, K))).astype(np.float32)
    mag = 1 + rng.integers(0, 64, p.nnz) * 2.0 ** -23
    for lists, where in ((p.rl, "alternating along rows"), (p.cl, "alternating along columns")):
        v = (np.where(_position(lists, p.nnz) % 2 == 0, 1.0, -1.0) * mag).astype(np.float32)
        tr, tc = check(engine, oracle, p, K, v, Xn, Xm, where)
        Y = tr if lists is p.rl else tc
        n = _lengths(lists)
        even = (n >= 64) & (n % 2 == 0)
        assert even.any() and (np.abs(Y[even]) < 2.0 ** 16).all()     # the sums of even-length lists really cancel


def _components(p):
    """connected component of every row and every column of S (the two blocks of the boundary pattern)"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    S = sp.csr_matrix((np.ones(p.nnz), p.ci.astype(np.int64), p.ro.astype(np.int64)), shape=(p.rows, p.cols))
    G = sp.bmat([[None, S], [S.T, None]])
    _, label = connected_components(G, directed=False)
    return label[:p.rows], label[p.rows:]


def _plant_rows_and_cols(p):
    """Hand-derived vectors (tests/test_backward_host.py) planted in real lists, for each direction: v is 0 except on the
    planted entries and X is 1 except one source row of a = 1 + 2^-12; the lists of the two blocks of the boundary
    pattern read disjoint sources, so no planted value reaches another planted list.  Returns per direction
    (v, X, {destination: expected fp32 value})."""
    out = {}
    comp_rows, comp_cols = _components(p)
    for direction in ("rows", "cols"):
        lists = p.rl if direction == "rows" else p.cl
        offsets, src, eidx = lists
        n = _lengths(lists)
        num_src = p.cols if direction == "rows" else p.rows
        # the block with prescribed lengths of this direction reads sources no list of the other block reads
        comp = comp_rows if direction == "rows" else comp_cols
        block = comp[np.flatnonzero(n == 1537)[0]]
        in_pool = lambda d: comp[d] == block
        v = np.zeros(p.nnz, np.float32)
        X = np.ones((num_src, 1), np.float32)
        want = {}
        taken = set()

        def pick(length):
            d = next(int(d) for d in np.flatnonzero(n == length) if int(d) not in taken and in_pool(d))
            taken.add(d)
            return d, int(offsets[d])

        d, o = pick(65)                      # order: across the 4-step and the 8-, 16-, 64-entry load groups
        v[eidx[o + 62:o + 65]] = [2.0 ** 24, 1, -2.0 ** 24]
        want[d] = 0.0
        d, o = pick(1025)                    # chunk order: partials 2^24, 1, -2^24
        v[eidx[[o, o + 512, o + 1024]]] = [2.0 ** 24, 1, -2.0 ** 24]
        want[d] = 0.0
        d, o = pick(1023)                    # each chunk its own chain: 2^24 + 1 + 1 | 1 + 1
        v[eidx[[o, o + 1, o + 2, o + 512, o + 513]]] = [2.0 ** 24, 1, 1, 1, 1]
        want[d] = 2.0 ** 24 + 2
        d, o = pick(17)                      # all products -0: the chain starts at +0
        v[eidx[o:o + 17]] = -0.0
        want[d] = 0.0
        # fma, not mul + add: -1 * 1 then a * a, in a list of the other block (whose sources no planted list reads)
        d = next(int(d) for d in np.flatnonzero(n >= 2) if comp[d] != block)
        e = int(offsets[d + 1])
        v[eidx[[e - 2, e - 1]]] = [-1, A12]
        X[src[e - 1]] = A12
        want[d] = 2.0 ** -11 + 2.0 ** -24
        out[direction] = (v, X, want)
    return out


@pytest.mark.parametrize("K", CLASS_KS)
def test_hand_vectors_in_real_lists(engine, oracle, patterns, K):
    p = patterns("boundary")
    for direction, (v, X1, want) in _plant_rows_and_cols(p).items():
        X = np.repeat(X1, K, axis=1)
        Xo = np.ones((p.rows if direction == "rows" else p.cols, K), np.float32)
        Xn, Xm = (X, Xo) if direction == "rows" else (Xo, X)
        tr, tc = check(engine, oracle, p, K, v, Xn, Xm, f"hand vectors in {direction}")
        Y = tr if direction == "rows" else tc
        expect = np.zeros_like(Y)
        for d, val in want.items():
            expect[d] = np.float32(val)
        # the twin's own bits, written by hand: every other destination reads only +-0 products
        assert_twin(Y, expect, f"hand bits {direction}")


@pytest.mark.parametrize("K", CLASS_KS)
@pytest.mark.parametrize("case", ["subnormal-v", "subnormal-x", "underflow"])
def test_subnormals(engine, oracle, patterns, case, K):
    """fp32 subnormal v or X, and normal operands whose products fall into (or below) the subnormal range; the twin
    keeps subnormals, so a device flush to zero fails here"""
    p = patterns("boundary")
    rng = np.random.default_rng(K + len(case))
    if case == "subnormal-v":
        v, Xn, Xm = wide(rng, p.nnz, -149, -127), wide(rng, (p.cols, K), -4, 4), wide(rng, (p.rows, K), -4, 4)
    elif case == "subnormal-x":
        v, Xn, Xm = wide(rng, p.nnz, -4, 4), wide(rng, (p.cols, K), -149, -127), wide(rng, (p.rows, K), -149, -127)
    else:
        v, Xn, Xm = wide(rng, p.nnz, -80, -60), wide(rng, (p.cols, K), -80, -60), wide(rng, (p.rows, K), -80, -60)
    if case != "underflow":
        assert _subnormal(v).any() or _subnormal(Xn).any()
    tr, tc = check(engine, oracle, p, K, v, Xn, Xm, case)
    assert _subnormal(tr).mean() > 0.1 and _subnormal(tc).mean() > 0.1


@pytest.mark.parametrize("K", CLASS_KS)
@pytest.mark.parametrize("where", ["inside-a-chunk", "across-chunks"])
def test_overflow(engine, oracle, patterns, where, K):
    """positive v, X of sign (-1)^k, products near 2^123 (a chunk of a few dozen entries overflows) or near 2^117 (a
    512-entry chunk stays finite, two or three chunks overflow in the partial sum)"""
    p = patterns("boundary")
    rng = np.random.default_rng(K + len(where))
    e = 106 if where == "inside-a-chunk" else 100
    v = np.ldexp(rng.uniform(1, 2, p.nnz), e).astype(np.float32)
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    Xn = (np.ldexp(rng.uniform(1, 2, (p.cols, K)), 17) * sign).astype(np.float32)
    Xm = (np.ldexp(rng.uniform(1, 2, (p.rows, K)), 17) * sign).astype(np.float32)
    tr, tc = check(engine, oracle, p, K, v, Xn, Xm, where)
    for lists, X, Y in ((p.rl, Xn, tr), (p.cl, Xm, tc)):
        assert np.isposinf(Y[:, 0]).any() and np.isneginf(Y[:, 1]).any() and np.isfinite(Y).any()
        part, owner = _chunk_partials(oracle, lists, v, X)
        finite_parts = np.ones(Y.shape[0], bool)
        np.logical_and.at(finite_parts, owner, np.isfinite(part).all(axis=1))
        only_across = finite_parts & ~np.isfinite(Y).all(axis=1)
        if where == "across-chunks":
            assert only_across.any()              # every chunk finite, the chunk sum overflows
        else:
            assert (~finite_parts).any()          # a chunk's own chain overflows


def _plant_nonfinite(rng, lists, v, X, K):
    """in one list with >= 3 entries: +inf in the first source, -inf in the second (both read with v > 0: opposite
    infinities), NaN in the third, over different k; another list reading the +inf source reads it with v = 0
    (0 * inf).  Returns the destinations that read a planted source."""
    offsets, src, eidx = lists
    n = np.diff(offsets.astype(np.int64))
    for d in rng.permutation(np.flatnonzero((n >= 3) & (n <= 64))):
        o = int(offsets[d])
        s0 = src[o]
        readers = [int(t) for t in np.flatnonzero(src == s0) if not offsets[d] <= t < offsets[d + 1]]
        if readers:
            break
    else:
        raise AssertionError("no list shares its first source")
    k_inf, k_nan = np.arange(0, K, 3), np.arange(1, K, 3)
    X[src[o], k_inf] = np.inf
    X[src[o + 1], k_inf] = -np.inf
    X[src[o + 2], k_nan] = np.nan
    v[eidx[[o, o + 1]]] = np.abs(v[eidx[[o, o + 1]]])
    v[eidx[readers[0]]] = 0
    touched = {int(np.searchsorted(offsets, t, side="right") - 1)
               for t in np.flatnonzero(np.isin(src, src[o:o + 3]))}
    dest_zero = int(np.searchsorted(offsets, readers[0], side="right") - 1)
    return d, dest_zero, touched, k_inf, k_nan


@pytest.mark.parametrize("K", CLASS_KS)
def test_nonfinite_x_rows(engine, oracle, patterns, K):
    """+-inf and NaN in rows of X (the sources): only the destinations whose lists read them change, with the twin's
    class; opposite infinities and 0 * inf give NaN"""
    p = patterns("boundary")
    for direction in ("rows", "cols"):
        rng = np.random.default_rng(K + (direction == "cols"))
        v = wide(rng, p.nnz, -8, 8)
        Xn, Xm = wide(rng, (p.cols, K), -8, 8), wide(rng, (p.rows, K), -8, 8)
        lists, X = (p.rl, Xn) if direction == "rows" else (p.cl, Xm)
        d, dz, touched, k_inf, k_nan = _plant_nonfinite(rng, lists, v, X, K)
        tr, tc = check(engine, oracle, p, K, v, Xn, Xm, f"non-finite X of {direction}")
        Y = tr if direction == "rows" else tc
        assert np.isnan(Y[d][k_inf]).all() and np.isnan(Y[d][k_nan]).all()        # inf - inf; NaN
        assert np.isnan(Y[dz][k_inf]).all()                                        # 0 * inf
        rest = np.ones(Y.shape[0], bool)
        rest[list(touched)] = False
        assert np.isfinite(Y[rest]).all()


# ---- 3. configurations --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("permute", ["0", "1"])
@pytest.mark.parametrize("row_order", ["natural", "clustered", "reversed"])
def test_row_order_and_permute(engine, oracle, patterns, monkeypatch, row_order, permute):
    p = patterns("boundary")
    monkeypatch.setenv("BSMR_BACKWARD_PERMUTE", permute)
    bw = p.create(row_order)
    try:
        assert engine.backward_stats(bw)["permute_values"] == int(permute)
        for K in (96, 256):
            rng = np.random.default_rng(K + 7)
            v = narrow(rng, p.nnz)
            Xn, Xm = narrow(rng, (p.cols, K)), narrow(rng, (p.rows, K))
            check(engine, oracle, p, K, v, Xn, Xm, f"row_order={row_order} permute={permute}", bw=bw)
    finally:
        engine.backward_destroy(bw)


@pytest.mark.parametrize("nb", [1, 2, 5])
@pytest.mark.parametrize("K", [192, 384])
def test_batches(engine, oracle, patterns, K, nb):
    p = patterns("boundary")
    rng = np.random.default_rng(K * nb)
    v = np.stack([narrow(rng, p.nnz) for _ in range(nb)])
    Xn = np.stack([narrow(rng, (p.cols, K)) for _ in range(nb)])
    Xm = np.stack([narrow(rng, (p.rows, K)) for _ in range(nb)])
    if nb == 1:
        v, Xn, Xm = v[0], Xn[0], Xm[0]
    check(engine, oracle, p, K, v, Xn, Xm, f"nb={nb}", nb=nb)


# ---- 4. addresses past 4 GiB --------------------------------------------------------------------------------------
def _fill_on_device(t, batch):
    """t (rows, K) fp32 on the device: m 2^e, m in [-2048, 2047], e in [-8, 8], an integer function of (row, k, batch)"""
    rows, K = t.shape
    k = torch.arange(K, device=t.device, dtype=torch.int64)[None, :]
    step = 1 << 16
    for r0 in range(0, rows, step):
        r = torch.arange(r0, min(rows, r0 + step), device=t.device, dtype=torch.int64)[:, None]
        h = (r * 1000003 + k * 7919 + batch * 104729) % 2147483647
        t[r0:r0 + r.shape[0]] = torch.ldexp((h % 4096 - 2048).to(torch.float32), ((h // 4096) % 17 - 8).to(torch.float32))


def _sub_lists(lists, dests):
    """the lists of `dests` only, in that order (the twin of a few destinations of a huge output)"""
    offsets, src, eidx = lists
    parts = [np.arange(offsets[d], offsets[d + 1], dtype=np.int64) for d in dests]
    idx = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    sub = np.zeros(len(dests) + 1, np.uint32)
    sub[1:] = np.cumsum([x.size for x in parts])
    return sub, src[idx], eidx[idx]


def _far_pattern(M, N, seed):
    """M rows with 40 random columns each; rows 0..7 also hold entries in the last 64 columns"""
    rng = np.random.default_rng(seed)
    per_row = []
    for r in range(M):
        s = set(rng.choice(N, 40, replace=False).tolist())
        if r < 8:
            s |= set((N - 1 - rng.choice(64, 12, replace=False)).tolist())
        per_row.append(np.array(sorted(s), np.uint32))
    ro = np.zeros(M + 1, np.uint32)
    ro[1:] = np.cumsum([x.size for x in per_row])
    return ro, np.concatenate(per_row)


@pytest.mark.parametrize("nb,N", [(1, 1_100_000), (2, 560_000)], ids=["one-batch-4.5GB", "two-batches-2.3GB"])
def test_addresses_past_4gib(engine, oracle, nb, N):
    """dA = S_dP B reads rows of B past 4 GiB (one batch: B is N x 1024 fp32 = 4.5 GB; two batches of 2.3 GB: batch 1's
    rows start 2.3 GB in); dB = S_dP^T A writes rows past 4 GiB of its N x K output.  B is generated on the device and
    only the rows read come back; dB is checked on the far rows that have entries and on far rows that have none.
    This covers byte offsets: every element index stays below 2^31 (1.13 - 1.15 x 2^30 elements); the cases whose element
    indices pass 2^32 live in tests/test_gpu_backward_extents.py."""
    M, K = 64, 1024
    x_bytes = nb * N * K * 4
    need = 2 * x_bytes + (4 << 30)
    free, _ = torch.cuda.mem_get_info(_dev())
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")
    assert x_bytes > 4 << 30 and N * K * 4 > 2 << 30
    ro, ci = _far_pattern(M, N, seed=nb)
    nnz = int(ci.size)
    assert ((nb - 1) * N + int(ci.max())) * K * 4 >= 4 << 30            # a row of B read past 4 GiB
    assert ((nb - 1) * N + N - 64) * K * 4 >= 4 << 30                     # the dB rows checked lie past 4 GiB
    bw = engine.backward_create(M, N, ro, ci, device=0)
    dev = _dev()
    try:
        rng = np.random.default_rng(17)
        v = np.stack([wide(rng, nnz, -8, 8) for _ in range(nb)])
        A = np.stack([wide(rng, (M, K), -8, 8) for _ in range(nb)])
        tB = torch.empty((nb, N, K), dtype=torch.float32, device=dev)
        for b in range(nb):
            _fill_on_device(tB[b], b)
        tv, tA = _t(v), _t(A)
        tdA = _nan(nb, M, K)
        tdB = _nan(nb, N, K)
        engine.sddmm_backward(bw, K, tv.data_ptr(), tA.data_ptr(), tB.data_ptr(), tdA.data_ptr(), tdB.data_ptr(), nb,
                              torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        rl, cl = row_lists(ro, ci), col_lists(M, N, ro, ci)
        used, remap = np.unique(ci, return_inverse=True)
        col_len = np.diff(cl[0].astype(np.int64))
        far_cols = np.arange(N - 64, N)
        assert (col_len[far_cols] > 0).any() and (col_len[far_cols] == 0).any()
        sub = _sub_lists(cl, far_cols)
        for b in range(nb):
            rows_read = tB[b].index_select(0, torch.from_numpy(used.astype(np.int64)).to(dev)).cpu().numpy()
            want = gather(oracle, (rl[0], remap.astype(np.uint32), rl[2]), v[b], rows_read)
            assert_twin(tdA[b].cpu().numpy(), want, f"dA batch {b}, B rows up to {(b * N + N) * K * 4 / 2**30:.2f} GiB")
            got = tdB[b].index_select(0, torch.from_numpy(far_cols).to(dev)).cpu().numpy()
            assert_twin(got, gather(oracle, sub, v[b], A[b]), f"dB batch {b}, far rows")
            assert (np.abs(got[col_len[far_cols] > 0]) > 0).any()
        del tB, tdB
    finally:
        torch.cuda.synchronize()
        engine.backward_destroy(bw)
        torch.cuda.empty_cache()


# ---- 5. an empty pattern and NULL operands -------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 2])
def test_empty_pattern_with_null_operands(engine, nb):
    """nnz = 0: v / dP, X, A and B may be NULL (nothing is read; torch hands out NULL for a zero-element tensor), and
    every element of Y, dA and dB is still written: +0 over a NaN poison"""
    M, N, K = 5, 7, 64
    bw = engine.backward_create(M, N, np.zeros(M + 1, np.uint32), np.zeros(0, np.uint32), device=0)
    hip = engine.hip()
    s = torch.cuda.current_stream(_dev()).cuda_stream
    try:
        for transpose, rows_y in ((0, M), (1, N)):
            Y = _nan(nb, rows_y, K)
            assert hip.bsmr_spmm(bw, K, transpose, None, None, Y.data_ptr(), nb, s) == engine.OK
            torch.cuda.synchronize()
            assert (Y.cpu().numpy().view(np.uint32) == 0).all()
        dA, dB = _nan(nb, M, K), _nan(nb, N, K)
        assert hip.bsmr_sddmm_backward(bw, K, None, None, None, dA.data_ptr(), dB.data_ptr(), nb, s) == engine.OK
        torch.cuda.synchronize()
        assert (dA.cpu().numpy().view(np.uint32) == 0).all() and (dB.cpu().numpy().view(np.uint32) == 0).all()
        # still refused: a NULL output
        assert hip.bsmr_spmm(bw, K, 0, None, None, None, nb, s) == engine.ERR_INVALID_ARG
    finally:
        engine.backward_destroy(bw)
    # with entries, a NULL operand is still refused
    ro, ci = np.array([0, 1, 1, 1, 1, 1], np.uint32), np.array([3], np.uint32)
    bw = engine.backward_create(M, N, ro, ci, device=0)
    try:
        Y = _nan(M, K)
        assert hip.bsmr_spmm(bw, K, 0, None, Y.data_ptr(), Y.data_ptr(), 1, s) == engine.ERR_INVALID_ARG
        assert hip.bsmr_spmm(bw, K, 0, Y.data_ptr(), None, Y.data_ptr(), 1, s) == engine.ERR_INVALID_ARG
        assert hip.bsmr_sddmm_backward(bw, K, None, Y.data_ptr(), Y.data_ptr(), Y.data_ptr(), None, 1, s) == \
            engine.ERR_INVALID_ARG
        assert hip.bsmr_sddmm_backward(bw, K, Y.data_ptr(), None, None, Y.data_ptr(), None, 1, s) == engine.ERR_INVALID_ARG
    finally:
        engine.backward_destroy(bw)
