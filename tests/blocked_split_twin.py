"""Bit-exact fp32 twin of the blocked SpMM with split panels (include/bsmr_hip.h "Blocked SpMM", segment_blocks = S),
built on tests/blocked_twin.py:

  B  = gather(the block lists of BlockedTwin, chunk = 16 S): the 16 S positions of S consecutive blocks are one segment,
       its own fmaf chain from +0; the segment sums are added in segment order.  S = 0 is chunk = 0, one chain;
  R, Y as in BlockedTwin.twin.

This is the chunk rule of oracle_gather_twin applied to the block list, so the twin needs no code of its own.  Also here:
numpy counts of the four statistics that bsmr_blocked_check_split adds, and the error bound of the split form."""
import numpy as np

from blocked_twin import U, BlockedTwin
from gather_twin import gather


def split_chunk(S):
    """the chunk of the block lists for segment_blocks = S.  A list's length is a uint32, so 16 S >= 2^32 cuts nothing:
    one chain, which the oracle spells chunk = 0"""
    S = int(S)
    return 0 if S == 0 or 16 * S >= 2 ** 32 else 16 * S


def split_stats(arrays, S):
    """segment_blocks, split_panels, segments, max_blocks_per_segment as bsmr_blocked_check_split reports them"""
    nb = np.diff(np.asarray(arrays["blockOffsets"], dtype=np.int64))
    nb = nb[nb > 0]
    longest = int(nb.max()) if nb.size else 0
    if S == 0:
        return {"segment_blocks": 0, "split_panels": 0, "segments": int(nb.size), "max_blocks_per_segment": longest}
    return {"segment_blocks": int(S), "split_panels": int((nb > S).sum()), "segments": int((-(-nb // S)).sum()),
            "max_blocks_per_segment": min(int(S), longest)}


class SplitTwin(BlockedTwin):
    def blocks_of_row(self):
        """nb of every row's panel (0 for the rows of panels without blocks and the rows in no panel)"""
        return np.diff(self.bl[0].astype(np.int64)) // 16

    def split_rows(self, S):
        """bool per row: its panel is cut into more than one segment"""
        return self.blocks_of_row() > S if S else np.zeros(self.M, dtype=bool)

    def twin(self, v, X, S=0):
        v = np.ascontiguousarray(v, dtype=np.float32)
        X = np.ascontiguousarray(X, dtype=np.float32)
        v1 = np.concatenate([v, np.zeros(1, np.float32)])
        X1 = np.concatenate([X, np.zeros((1, X.shape[1]), np.float32)])
        B = gather(self.oracle, self.bl, v1, X1, chunk=split_chunk(S))
        R = gather(self.oracle, self.rl, v1, X1)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.where(self.has_blocks[:, None], (B + R).astype(np.float32), R)

    def fp64(self, v, X, S=0):
        """(Y64, bound): (max(16 min(nb, S) + ceil(nb / S) - 1, n_r) + 4) u sum|v||x| + the underflow term per row: a term
        passes at most 16 min(nb, S) roundings of its segment chain, then at most ceil(nb / S) - 1 additions of partials"""
        Y, unsplit = BlockedTwin.fp64(self, v, X)
        if S == 0:
            return Y, unsplit
        del unsplit
        v64, X64 = np.asarray(v, np.float64), np.asarray(X, np.float64)
        row_of = np.repeat(np.arange(self.M), np.diff(self.ro.astype(np.int64)))
        A = np.zeros_like(Y)
        np.add.at(A, row_of, np.abs(v64)[:, None] * np.abs(X64[self.ci]))
        nb = self.blocks_of_row()
        n_res = np.diff(self.rl[0].astype(np.int64))
        n_block = np.where(nb > 0, 16 * np.minimum(nb, S) + -(-nb // S) - 1, 0)
        n = np.maximum(n_block, n_res) + 4
        return Y, n[:, None] * U * A + ((16 * nb + n_res + 2) * 2.0 ** -149)[:, None]
