"""Bit-exact fp32 twin of the blocked SpMM (include/bsmr_hip.h "Blocked SpMM"), built on tests/gather_twin.py:

  B  = gather(lists of all 16 positions of every block of the row's panel, chunk = 0: one chain), over v1 = v + [0.0]
       (empty cells point at the appended element) and X1 = X + one zero row (padding columns point at row N);
  R  = gather(residue lists: the row's entries that no block cell holds, ascending CSR index, the default chunk);
  Y  = np.float32(B + R) where the row's panel has blocks, R elsewhere (rows in no panel have empty lists: +0).

The lists come from the RPHM arrays and the CSR in numpy, never from the library.  Also here: the test pattern shared by
tests/test_spmm_blocked_host.py and tests/test_gpu_spmm_blocked.py, and numpy counts of what bsmr_blocked_check reports."""
import numpy as np

from gather_twin import CHUNK, gather

NULL = 0xFFFFFFFF
U = 2.0 ** -24


def blocked_pattern(seed=5, cols=2000):
    """128 rows: 6 groups of 16 rows over 40 shared columns each (row 0 of group 0 with 1 100 columns of its own on top:
    a residue row of three chunks; every other row with r % 3 == 0 keeps a shared column with probability 0.75: empty
    cells), 27 rows of 1 - 29 random columns (panels without blocks), 5 empty rows; all rows shuffled."""
    rng = np.random.default_rng(seed)
    per_row = []
    for g in range(6):
        shared = rng.choice(cols, 40, replace=False)
        for r in range(16):
            if g == 0 and r == 0:
                own = rng.choice(np.setdiff1d(np.arange(cols), shared), 1100, replace=False)
                per_row.append(np.concatenate([shared, own]))
            elif r % 3 == 0:
                per_row.append(shared[rng.random(40) < 0.75])
            else:
                per_row.append(shared)
    for _ in range(27):
        per_row.append(rng.choice(cols, int(rng.integers(1, 30)), replace=False))
    per_row += [np.zeros(0, dtype=np.int64)] * 5
    per_row = [np.sort(per_row[i]).astype(np.uint32) for i in rng.permutation(len(per_row))]
    ro = np.zeros(len(per_row) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([p.size for p in per_row])
    return len(per_row), cols, ro, np.concatenate(per_row).astype(np.uint32)


def copy_arrays(arrays):
    return {k: np.array(a, dtype=np.uint32, copy=True) for k, a in arrays.items()}


def in_block(nnz, arrays):
    """bool per CSR index: the entry lies in a block cell"""
    flag = np.zeros(nnz, dtype=bool)
    bv = np.asarray(arrays["blockValues"], dtype=np.uint32)
    flag[bv[bv != NULL]] = True
    return flag


def numpy_stats(M, N, ro, ci, arrays):
    """what bsmr_blocked_check reports, counted here"""
    bo = np.asarray(arrays["blockOffsets"], dtype=np.int64)
    per_panel = np.diff(bo)
    dense = in_block(ci.size, arrays)
    row_of = np.repeat(np.arange(M), np.diff(ro.astype(np.int64)))
    res_len = np.bincount(row_of[~dense], minlength=M)
    return {
        "panels": int(per_panel.size),
        "panels_with_blocks": int((per_panel > 0).sum()),
        "blocks": int(bo[-1]),
        "block_entries": int(dense.sum()),
        "padding_columns": int((np.asarray(arrays["denseCols"]) == N).sum()),
        "residue_entries": int((~dense).sum()),
        "max_residue_row": int(res_len.max()) if M else 0,
        "split_residue_rows": int((res_len > CHUNK).sum()),
        "max_blocks_per_panel": int(per_panel.max()) if per_panel.size else 0,
        "residue_items": int(np.maximum(1, -(-res_len // CHUNK)).sum()),
    }


def block_lists(M, N, nnz, arrays):
    """(offsets, src, eidx) of the block chains - src N = the appended zero row, eidx nnz = the appended 0.0 - and the
    bool per row `its panel has blocks`"""
    rr = np.asarray(arrays["reorderedRows"], dtype=np.int64)
    bo = np.asarray(arrays["blockOffsets"], dtype=np.int64)
    dc = np.asarray(arrays["denseCols"], dtype=np.uint32).reshape(-1, 16)
    bv = np.asarray(arrays["blockValues"], dtype=np.uint32).reshape(-1, 16, 16)
    src = [np.zeros(0, np.uint32)] * M
    eidx = [np.zeros(0, np.uint32)] * M
    has = np.zeros(M, dtype=bool)
    for p in range(bo.size - 1):
        b0, b1 = bo[p], bo[p + 1]
        if b1 == b0:
            continue
        for i in range(16):
            if 16 * p + i >= rr.size:
                break
            r = rr[16 * p + i]
            has[r] = True
            src[r] = dc[b0:b1].reshape(-1)                                  # blocks in order, j = 0 .. 15 inside
            cell = bv[b0:b1, i, :].reshape(-1)
            eidx[r] = np.where(cell == NULL, np.uint32(nnz), cell).astype(np.uint32)
    offsets = np.zeros(M + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([s.size for s in src])
    cat = lambda parts: np.concatenate(parts).astype(np.uint32) if offsets[-1] else np.zeros(0, np.uint32)
    return (offsets, cat(src), cat(eidx)), has


def residue_lists(M, ro, ci, arrays):
    keep = ~in_block(ci.size, arrays)
    row_of = np.repeat(np.arange(M), np.diff(ro.astype(np.int64)))
    offsets = np.zeros(M + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(np.bincount(row_of[keep], minlength=M))
    return offsets, ci[keep].astype(np.uint32), np.flatnonzero(keep).astype(np.uint32)


class BlockedTwin:
    """the lists of one (CSR, RPHM), built once; twin(v, X) per operand set"""

    def __init__(self, oracle, M, N, ro, ci, arrays):
        self.oracle, self.M, self.N, self.nnz = oracle, M, N, int(ci.size)
        self.ro, self.ci = np.asarray(ro, dtype=np.uint32), np.asarray(ci, dtype=np.uint32)
        self.bl, self.has_blocks = block_lists(M, N, self.nnz, arrays)
        self.rl = residue_lists(M, self.ro, self.ci, arrays)

    def parts(self, v, X):
        v = np.ascontiguousarray(v, dtype=np.float32)
        X = np.ascontiguousarray(X, dtype=np.float32)
        v1 = np.concatenate([v, np.zeros(1, np.float32)])
        X1 = np.concatenate([X, np.zeros((1, X.shape[1]), np.float32)])
        B = gather(self.oracle, self.bl, v1, X1, chunk=0)
        R = gather(self.oracle, self.rl, v1, X1)
        return B, R

    def twin(self, v, X):
        B, R = self.parts(v, X)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.where(self.has_blocks[:, None], (B + R).astype(np.float32), R)

    def fp64(self, v, X):
        """(Y64, bound): the exact product and (max(16 nb, n_r) + 4) u sum|v||x| + the underflow term per row"""
        v64, X64 = np.asarray(v, np.float64), np.asarray(X, np.float64)
        row_of = np.repeat(np.arange(self.M), np.diff(self.ro.astype(np.int64)))
        Y = np.zeros((self.M, X64.shape[1]))
        S = np.zeros_like(Y)
        np.add.at(Y, row_of, v64[:, None] * X64[self.ci])
        np.add.at(S, row_of, np.abs(v64)[:, None] * np.abs(X64[self.ci]))
        n_block = np.diff(self.bl[0].astype(np.int64))        # 16 nb
        n_res = np.diff(self.rl[0].astype(np.int64))
        n = np.maximum(n_block, n_res) + 4
        return Y, n[:, None] * U * S + ((n_block + n_res + 2) * 2.0 ** -149)[:, None]
