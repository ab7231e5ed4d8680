"""References of the sparse row softmax (include/bsmr_hip.h "Sparse row softmax"), built in numpy and never taken from
the library:
  * backward: bit-exact fp32 twin.  g = the chunked fma chain of each row over y * dY, i.e. oracle_gather_twin at K = 1
    with src = eidx = arange(nnz), v = y, X = dY[:, None]; then dX = fl32(fl32(y * fl32(dY - g)) * scale);
  * forward: fp64 softmax over the same z = fl32(scale * x), with the contract's special values, and its error bound.
Shared by tests/test_softmax_host.py (the twin against hand-derived bits) and the GPU modules."""
import numpy as np

from gather_twin import gather

U = 2.0 ** -24
TINY = 2.0 ** -126
C_Y = 6   # the constants of the header's bound


def row_of(ro):
    ro = np.asarray(ro, dtype=np.int64)
    return np.repeat(np.arange(ro.size - 1), np.diff(ro))


def row_sums(oracle, ro, y, dY):
    """g[r] = sum_t y_t dY_t over row r in the contract's order"""
    ro = np.ascontiguousarray(ro, dtype=np.uint32)
    idx = np.arange(int(ro[-1]), dtype=np.uint32)
    return gather(oracle, (ro, idx, idx), np.asarray(y, np.float32), np.asarray(dY, np.float32).reshape(-1, 1))[:, 0]


def backward_twin(oracle, ro, y, dY, scale):
    y = np.asarray(y, np.float32)
    dY = np.asarray(dY, np.float32)
    g = row_sums(oracle, ro, y, dY)
    with np.errstate(all="ignore"):
        return (y * (dY - g[row_of(ro)])) * np.float32(scale)


def z_of(x, scale):
    with np.errstate(all="ignore"):
        return np.float32(scale) * np.asarray(x, np.float32)


def forward_f64(ro, x, scale):
    """(y64, z, m per entry, Z_r per entry, n per entry) in fp64 over z = fl32(scale x)"""
    ro = np.asarray(ro, dtype=np.int64)
    z = z_of(x, scale).astype(np.float64)
    n = np.diff(ro)
    live = np.nonzero(n > 0)[0]
    r = row_of(ro)
    y = np.zeros_like(z)
    m_row = np.full(n.size, np.nan)
    zr_row = np.zeros(n.size)
    if live.size:
        m_row[live] = np.maximum.reduceat(z, ro[live])     # NaN propagates: the contract's m
    m = m_row[r]
    with np.errstate(all="ignore"):
        d = z - m
        e = np.where(m == -np.inf, 0.0, np.exp(d))
        s = np.zeros(n.size)
        if live.size:
            s[live] = np.add.reduceat(e, ro[live])
            zr_row[live] = np.maximum.reduceat(np.abs(np.where(m == -np.inf, 0.0, d)), ro[live])
        y = np.where(m == -np.inf, 0.0, e / s[r])
    return y, z, m, zr_row[r], n[r].astype(np.float64)


def check_forward(ro, x, scale, got, where=""):
    """got (fp32, CSR order) against fp64 under the header's bound; NaN exactly where the reference is NaN"""
    got = np.asarray(got, np.float32)
    y64, z, m, zr, n = forward_f64(ro, x, scale)
    nan = np.isnan(y64)
    assert np.array_equal(np.isnan(got), nan), (where, np.argwhere(np.isnan(got) != nan)[:5])
    ok = ~nan
    g = got[ok].astype(np.float64)
    with np.errstate(all="ignore"):
        bound = (n[ok] + C_Y + np.abs(z[ok] - m[ok]) + zr[ok]) * U * y64[ok] + (n[ok] + 2) * TINY
    err = np.abs(g - y64[ok])
    bad = err > bound
    assert not bad.any(), (f"{where}: {int(bad.sum())} entries over the bound; first at {np.argwhere(bad)[0]}: "
                           f"got {g[bad][0]!r} want {y64[ok][bad][0]!r} bound {bound[bad][0]!r}")
    # every finite row sums to 1 within (n + c) u
    ro64 = np.asarray(ro, dtype=np.int64)
    lens = np.diff(ro64)
    live = np.nonzero(lens > 0)[0]
    if live.size:
        sums = np.add.reduceat(got.astype(np.float64), ro64[live])
        finite = ~np.isnan(sums) & (np.maximum.reduceat(y64, ro64[live]) > 0)
        tol = (lens[live] + C_Y) * U + (lens[live] + 2) * TINY
        assert (np.abs(sums - 1.0)[finite] <= tol[finite]).all(), (where, "row sums")
    return err
