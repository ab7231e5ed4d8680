"""Bit-exact fp32 twin of the SDDMM backward's gather-and-accumulate (oracle/spmm_oracle.c, oracle_gather_twin) and the
destination lists it runs over, built in numpy and never taken from the library:
  rows:    offsets = row_offsets, src = col_indices, eidx = arange(nnz)                  (Y = S_v X,   dA = S_dP B)
  columns: a stable argsort of col_indices, i.e. ascending row within each column    (Y = S_v^T X, dB = S_dP^T A)
Shared by tests/test_backward_host.py (the twin against hand-derived bits) and the GPU modules (the device against the
twin)."""
import ctypes as C

import numpy as np

CHUNK = 512   # BSMR_BACKWARD_CHUNK


def row_lists(ro, ci):
    ci = np.ascontiguousarray(ci, dtype=np.uint32)
    return np.ascontiguousarray(ro, dtype=np.uint32), ci, np.arange(ci.size, dtype=np.uint32)


def col_lists(rows, cols, ro, ci):
    ro64 = np.asarray(ro, dtype=np.int64)
    ci64 = np.asarray(ci, dtype=np.int64)
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(ro64))
    order = np.argsort(ci64, kind="stable")
    co = np.zeros(cols + 1, dtype=np.int64)
    np.add.at(co, ci64 + 1, 1)
    return (np.cumsum(co).astype(np.uint32), row_of[order].astype(np.uint32), order.astype(np.uint32))


def _bind(oracle):
    f = oracle.lib.oracle_gather_twin
    if f.argtypes is None:
        f.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6
        f.restype = None
    return f


def gather(oracle, lists, v, X, chunk=CHUNK):
    """Y[d] = the chunked fma chains of list d over v[eidx[t]] * X[src[t]]; lists = (offsets, src, eidx)"""
    offsets, src, eidx = (np.ascontiguousarray(a, dtype=np.uint32) for a in lists)
    v = np.ascontiguousarray(v, dtype=np.float32)
    X = np.ascontiguousarray(X, dtype=np.float32)
    assert X.ndim == 2 and v.ndim == 1
    assert eidx.size == 0 or int(eidx.max()) < v.size
    assert src.size == 0 or int(src.max()) < X.shape[0]
    num_dest, K = offsets.size - 1, X.shape[1]
    Y = np.empty((num_dest, K), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _bind(oracle)(num_dest, K, chunk, p(offsets), p(src), p(eidx), p(v), p(X), p(Y))
    return Y


def assert_twin(got, want, where=""):
    """bit for bit, except that where the twin is NaN the device must be NaN with any payload"""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    nan = np.isnan(want)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (nan & np.isnan(got))
    if not same.all():
        bad = np.argwhere(~same)
        i = tuple(bad[0])
        raise AssertionError(f"{where}: {bad.shape[0]} of {same.size} elements differ from the twin; first at {i}: "
                             f"got {got[i]!r} (0x{int(got.view(np.uint32)[i]):08x}), "
                             f"twin {want[i]!r} (0x{int(want.view(np.uint32)[i]):08x})")
