"""References of the fused sparse attention (include/bsmr_hip.h "Fused sparse attention"), built in numpy and
never taken from the library:
  * forward_f64 / check_forward: O in fp64 over z = fl32(scale p) with the contract's special values, and the header's
    bound  |O - O64| <= (2n + 2 Z_r + 10) u sum_t w64_t |V[c_t,k]| + (n + 2) 2^-126 max_t |V[c_t,k]|;
  * exact_forward: the exact twin for scores that are one constant per row mixed with -inf.  Then e is exactly 1 or 0,
    s is the count of the finite entries and O = fl32(gather_twin(e, V) / s) bit for bit (oracle_gather_twin keeps the
    chunked fma chains and the chunk order of the partials; fp32 division is correctly rounded in numpy as on the device);
  * row_dot: the D twin.  Lane l of 32 chains fmaf(dO_k, O_k, .) over k = l, l + 32, ... from +0 - oracle_gather_twin at
    K = 1 over one destination per (row, lane) - and the 32 partials meet in a butterfly over the offsets 16, 8, 4, 2, 1,
    each step one np.float32 addition;
  * values_backward: dP = fl32(fl32(W * fl32(dW - D)) * scale) from given W and D, all in np.float32.
Shared by tests/test_attention_host.py (the twins against hand-derived bits) and the GPU modules."""
import numpy as np

from gather_twin import gather, row_lists
from softmax_twin import TINY, U, row_of, z_of

C_O = 10   # the constant of the header's bound


def forward_f64(ro, ci, p, scale, V):
    """(O64 [M, K], bound [M, K], m64 [M], s64 [M]) over z = fl32(scale p); NaN rows where the contract has them"""
    ro = np.asarray(ro, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    V = np.asarray(V, dtype=np.float64)
    M, K = ro.size - 1, V.shape[1]
    z = z_of(p, scale).astype(np.float64)
    O = np.zeros((M, K))
    bound = np.zeros((M, K))
    m_row = np.full(M, -np.inf)
    s_row = np.zeros(M)
    for r in range(M):
        b, e = ro[r], ro[r + 1]
        n = e - b
        if n == 0:
            continue
        with np.errstate(all="ignore"):
            m = np.max(z[b:e]) if not np.isnan(z[b:e]).any() else np.nan
            m_row[r] = m
            if m == -np.inf:
                continue
            d = z[b:e] - m
            ex = np.exp(d)
            s = ex.sum()
            s_row[r] = s
            w = ex / s
            x = V[ci[b:e]]
            O[r] = w @ x if np.isfinite(s) else np.nan
            if np.isfinite(s):
                zr = np.abs(d[np.isfinite(d)]).max()
                bound[r] = (2 * n + 2 * zr + C_O) * U * (w @ np.abs(x)) + (n + 2) * TINY * np.abs(x).max(axis=0)
    return O, bound, m_row, s_row


def check_forward(ro, ci, p, scale, V, got, where=""):
    """got (fp32 [M, K]) against fp64 under the header's bound; NaN exactly where the reference is NaN"""
    got = np.asarray(got, np.float32)
    O, bound, _, _ = forward_f64(ro, ci, p, scale, V)
    nan = np.isnan(O)
    assert np.array_equal(np.isnan(got), nan), (where, np.argwhere(np.isnan(got) != nan)[:5])
    err = np.abs(got.astype(np.float64) - O)
    bad = ~nan & (err > bound)
    assert not bad.any(), (f"{where}: {int(bad.sum())} elements over the bound; first at {np.argwhere(bad)[0]}: "
                           f"got {got[bad][0]!r} want {O[bad][0]!r} bound {bound[bad][0]!r}")
    with np.errstate(all="ignore"):
        return np.nanmax(np.where(bound > 0, err / bound, 0.0)) if err.size else 0.0


def exact_scores(ro, rng, dead_rows=()):
    """scores that are one constant per row mixed with -inf (at least one finite entry per row, except `dead_rows`,
    which are all -inf); returns (p, e) with e the exact weights before normalisation"""
    ro = np.asarray(ro, dtype=np.int64)
    r = row_of(ro)
    const = rng.integers(-6, 7, ro.size - 1).astype(np.float32) * np.float32(0.5)
    live = rng.random(r.size) < 0.7
    lens = np.diff(ro)
    live[ro[:-1][lens > 0]] = True          # the first entry of every row stays finite
    live[np.isin(r, list(dead_rows))] = False
    p = np.where(live, const[r], -np.inf).astype(np.float32)
    return p, live.astype(np.float32)


def exact_forward(oracle, ro, ci, e, V):
    """(O, m is left to the caller, s) for exact weights e in {0, 1}"""
    ro = np.asarray(ro, dtype=np.int64)
    acc = gather(oracle, row_lists(ro, ci), e, V)
    idx = np.arange(e.size, dtype=np.uint32)
    s = gather(oracle, (ro, idx, idx), e, np.ones((e.size, 1), np.float32))[:, 0]
    with np.errstate(all="ignore"):
        O = np.where(s[:, None] > 0, acc / s[:, None], np.float32(0)).astype(np.float32)
    return O, s


def butterfly(parts):
    """parts [..., 32] fp32 -> the value every lane holds after x + partner over the offsets 16, 8, 4, 2, 1"""
    x = np.asarray(parts, np.float32).copy()
    lanes = np.arange(32)
    with np.errstate(all="ignore"):
        for off in (16, 8, 4, 2, 1):
            x = (x + x[..., lanes ^ off]).astype(np.float32)
    assert np.isnan(x).any() or (x == x[..., :1]).all()   # fp32 addition commutes: every lane ends with the same value
    return x[..., 0]


def row_dot(oracle, dO, O):
    """D[r] = dO_r . O_r in the contract's order; dO, O fp32 [M, K], K a multiple of 32"""
    dO = np.ascontiguousarray(dO, np.float32)
    O = np.ascontiguousarray(O, np.float32)
    M, K = O.shape
    steps = K // 32
    # destination (r, l) lists the elements k = l, l + 32, ... of row r: flat index r K + l + 32 i
    r, l, i = np.meshgrid(np.arange(M), np.arange(32), np.arange(steps), indexing="ij")
    idx = (r * K + l + 32 * i).reshape(-1).astype(np.uint32)
    offsets = (np.arange(M * 32 + 1) * steps).astype(np.uint32)
    parts = gather(oracle, (offsets, idx, idx), dO.reshape(-1), O.reshape(-1, 1))[:, 0]   # (at most 16 steps: never chunked)
    return butterfly(parts.reshape(M, 32))


def values_backward(ro, W, dW, D, scale):
    """dP = ((W (dW - D)) scale), each step rounded to fp32"""
    W = np.asarray(W, np.float32)
    dW = np.asarray(dW, np.float32)
    D = np.asarray(D, np.float32)
    with np.errstate(all="ignore"):
        return ((W * (dW - D[row_of(ro)])).astype(np.float32) * np.float32(scale)).astype(np.float32)
