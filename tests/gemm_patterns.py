"""Patterns of ONE macro-tile of the GEMM engine whose (wave, pass) entry lists are known by construction, for the tests of
the mask passes (csrc/gemm_kernels.hpp: gemmMaskPass): tests/test_gemm_pass_host.py checks the construction on the CPU,
tests/test_gpu_gemm_passes.py runs the kernels on them.

With the natural row order (row_mode = ROWS_IDENTITY), no balancing (gemm_balance_columns = 0) and every row holding an
entry, row i of the matrix is row i of the macro-tile and column j its column slot j.  Wave (wm, wn) of the 2 x 4 owns
rows [128 wm, 128 wm + 128) x columns [16 n wn, 16 n wn + 16 n), n = blocks / 4; its tile t = 16-row tile * n + 16-column
tile belongs to pass t // 16.  Every row gets one entry in the LAST column (waves 3 and 7), so that no row is empty;
everything else goes where the case says, and waves 1, 2, 4, 5, 6 hold nothing at all."""
import ctypes as C
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
ROWS = 256


def pass_cells(blocks, q):
    """(row, column) cells of wave 0's pass q in a 256 x 16*blocks macro-tile, in (row, column) order"""
    n = blocks // 4
    cells = []
    for tm in range(8):
        cols = [16 * tn + c for tn in range(n) if (tm * n + tn) // 16 == q for c in range(16)]
        cells += [(16 * tm + r, c) for r in range(16) for c in cols]
    return cells


def pattern(blocks, per_pass):
    """CSR pattern with per_pass[q] entries in wave 0's pass q (its first cells) and one entry per row in the last column"""
    cols = 16 * blocks
    entries = {(i, cols - 1) for i in range(ROWS)}
    for q, count in enumerate(per_pass):
        cells = pass_cells(blocks, q)
        assert count <= len(cells)
        entries.update(cells[:count])
    entries = sorted(entries)
    ro = np.zeros(ROWS + 1, dtype=np.uint32)
    for i, _ in entries:
        ro[i + 1] += 1
    return ROWS, cols, np.cumsum(ro).astype(np.uint32), np.array([j for _, j in entries], dtype=np.uint32)


# blocks -> the cases: entries of wave 0 per pass.  A trip of the kernels is 256 words at 16 x 20 and 512 at 16 x 16: lists
# one short of a trip (one padding word), exactly a trip, one entry more (a second trip of one batch), two trips, two
# trips and one entry (16 x 16: 1025, a third trip); an empty pass between two others; an empty first pass
CASES = {
    20: [(255,), (256,), (257,), (512,), (513,), (300, 0, 70), (0, 9, 0)],
    16: [(511,), (512,), (513,), (1025,), (0, 600), (40, 0)],
}


def longest_list(engine, blocks, per_pass):
    """longest (wave, pass) list of packGemm on the pattern, in words (lists are padded to a multiple of 4), and the return
    code of the brute-force reading of the format (tests/native/plancheck.hip: plancheck_gemm)"""
    rows, cols, ro, ci = pattern(blocks, per_pass)
    lib = C.CDLL(str(REPO / "tests" / "native" / "libplancheck.so"))
    lib.plancheck_gemm.restype = C.c_int
    lib.plancheck_gemm.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    arrays = engine.Pipeline(csr, alpha=0.3, delta=0.0, row_mode=engine.ROWS_IDENTITY, device=-1).arrays()
    keep = {k: np.ascontiguousarray(arrays[k], dtype=np.uint32) for k in
            ("reorderedRows", "denseCols", "blockOffsets", "blockValues", "sparseValueOffsets",
             "sparseValues", "sparseRelativeRows", "sparseColIndices")}
    d = engine.RphmDesc()
    d.M, d.N, d.nnz = rows, cols, csr.nnz
    d.num_nonzero_rows = keep["reorderedRows"].size
    d.num_row_panels = keep["blockOffsets"].size - 1
    cast = lambda a: a.ctypes.data_as(engine.u32p)
    d.reordered_rows, d.dense_cols = cast(keep["reorderedRows"]), cast(keep["denseCols"])
    d.block_offsets, d.block_values = cast(keep["blockOffsets"]), cast(keep["blockValues"])
    d.sparse_value_offsets, d.sparse_values = cast(keep["sparseValueOffsets"]), cast(keep["sparseValues"])
    d.sparse_relative_rows, d.sparse_col_indices = cast(keep["sparseRelativeRows"]), cast(keep["sparseColIndices"])
    out = (C.c_uint64 * 11)()
    rc = lib.plancheck_gemm(C.byref(d), 16, blocks, 0, out)
    return rc, int(out[7]), int(out[0]), int(out[1])
