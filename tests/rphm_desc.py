"""bsmr_rphm_desc views of RPHM arrays for the host-side checks of tests/native/plancheck.hip: from the host pipeline
(its own row order) or from the Python oracle with any row order.  The numpy arrays a desc points into are returned with
it and must be kept alive as long as the desc is used.  stream_check calls plancheck_stream, the host reading of the
streaming format."""
import ctypes as C
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent

KEYS = ("reorderedRows", "denseCols", "blockOffsets", "blockValues", "sparseValueOffsets",
        "sparseValues", "sparseRelativeRows", "sparseColIndices")


def desc_from_arrays(engine, rows, cols, nnz, arrays):
    """(desc, keep): the RphmDesc of RPHM-layout arrays and the uint32 copies it points into"""
    keep = {k: np.ascontiguousarray(arrays[k], dtype=np.uint32) for k in KEYS}
    d = engine.RphmDesc()
    d.M, d.N, d.nnz = rows, cols, nnz
    d.num_nonzero_rows = keep["reorderedRows"].size
    d.num_row_panels = keep["blockOffsets"].size - 1
    cast = lambda a: a.ctypes.data_as(engine.u32p)
    d.reordered_rows, d.dense_cols = cast(keep["reorderedRows"]), cast(keep["denseCols"])
    d.block_offsets, d.block_values = cast(keep["blockOffsets"]), cast(keep["blockValues"])
    d.sparse_value_offsets, d.sparse_values = cast(keep["sparseValueOffsets"]), cast(keep["sparseValues"])
    d.sparse_relative_rows, d.sparse_col_indices = cast(keep["sparseRelativeRows"]), cast(keep["sparseColIndices"])
    return d, keep


def pipeline_desc(engine, rows, cols, ro, ci, alpha, delta):
    """(csr, desc, keep) of the host pipeline's RPHM for (alpha, delta)"""
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    arrays = engine.Pipeline(csr, alpha=alpha, delta=delta, device=-1).arrays()
    d, keep = desc_from_arrays(engine, rows, cols, csr.nnz, arrays)
    return csr, d, keep


def oracle_arrays(rows, cols, ro, ci, order, delta):
    """RPHM arrays of the Python oracle (oracle/bsmr_oracle.py) for the row order `order` (None: natural order)"""
    import bsmr_oracle
    ro = np.ascontiguousarray(ro, dtype=np.uint32)
    ci = np.ascontiguousarray(ci, dtype=np.uint32)
    if order is None:
        order = bsmr_oracle.no_reorder_rows(rows, ro)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    cr = bsmr_oracle.col_reordering(rows, cols, ro, ci, order, delta)
    rp = bsmr_oracle.rphm(rows, cols, ro, ci, order, cr)
    return {"reorderedRows": order, "denseCols": cr["denseCols"], "blockOffsets": rp["blockOffsets"],
            "blockValues": rp["blockValues"], "sparseValueOffsets": cr["sparseValueOffsets"],
            "sparseValues": rp["sparseValues"], "sparseRelativeRows": rp["sparseRelativeRows"],
            "sparseColIndices": rp["sparseColIndices"]}


# plancheck_stream (tests/native/plancheck.hip): the encodings it reports, its report and the PackOptions it takes
MASK, WIN8, DIRECT16, DIRECT32, NO_TILES = 0, 1, 2, 4, 255
STREAM_REPORT = ("encoding", "items", "blocks", "dense", "residue", "residue_items", "staged", "too_wide", "promoted",
                 "evicted", "mutated", "pack_status", "max_item_blocks")
# (bsmr::PackOptions' own defaults, except order_window: 128 columns instead of 8192, so that item order 2 has more than
# one window to sort by on the small patterns of the host grid; a caller that mirrors a device plan passes 8192)
STREAM_DEFAULTS = dict(group=1, blocks_per_item=32, sparse_per_item=256, wide=0, column_order=1, staged=1, mask_tiles=1,
                       free_residue=0, item_order=0, order_window=128, item_span=0)
_plancheck = None


def stream_check(d, ro, ci, promote=0, evict=0, mutate=0, **options):
    """Packs the desc `d` of the CSR (ro, ci) with bsmr::PackOptions `options` - after promotion / eviction if asked for,
    with one of streamMutate's defects if asked for - and reads the plan as the kernels do.  Returns (code, report)."""
    global _plancheck
    u32p = C.POINTER(C.c_uint32)
    if _plancheck is None:
        _plancheck = C.CDLL(str(REPO / "tests" / "native" / "libplancheck.so"))
        _plancheck.plancheck_stream.restype = C.c_int
        _plancheck.plancheck_stream.argtypes = [C.c_void_p, u32p, u32p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int,
                                                C.POINTER(C.c_uint64)]
    o = dict(STREAM_DEFAULTS, **options)
    assert len(o) == len(STREAM_DEFAULTS), options
    ro, ci = np.ascontiguousarray(ro, dtype=np.uint32), np.ascontiguousarray(ci, dtype=np.uint32)
    packed = (C.c_int32 * 11)(*(o[k] for k in STREAM_DEFAULTS))
    out = (C.c_uint64 * 13)()
    rc = _plancheck.plancheck_stream(C.byref(d), ro.ctypes.data_as(u32p), ci.ctypes.data_as(u32p), packed, promote, evict,
                                     mutate, out)
    return rc, dict(zip(STREAM_REPORT, (int(v) for v in out)))


DIGEST_PARTS = ("groupRows", "rowBase", "winLen", "winMask", "blockCols", "tiles", "blockMask", "items",
                "numItems", "numBlocks", "numTiles", "unionColumns", "maskForm")


def format_digest(engine, plan):
    """bsmr_plan_format_digest by name: FNV-1a of each array of the plan's dense format in device memory, and its counts"""
    out = (C.c_uint64 * 13)()
    assert engine.hip().bsmr_plan_format_digest(plan, out) == engine.OK
    return dict(zip(DIGEST_PARTS, (int(v) for v in out)))
