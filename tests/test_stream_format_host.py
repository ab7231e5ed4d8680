"""The streaming plan format (csrc/plan_pack.hpp: packPlan / packResidue) read on the host the way denseStream,
denseGroups, their fp32 / any-K / in-kernel-conversion siblings and the residue kernels read it
(tests/native/plancheck.hip: plancheck_stream).  For every work item in launch order, block, panel, lane and register
the destination is decoded per encoding (mask form, 8-bit windows, 16- and 32-bit direct offsets) and must be the CSR
index of the entry at the block's column and the group's row - rows and columns taken from the CSR, not from the RPHM.
blockMask, the per-item windows (rowBase / winLen / winMask), the item cuts and the panel and free residue are held to
what the kernels assume; every CSR index is reached exactly once.  No GPU.

The boundaries are the code's own: kWindowMax = 255 (0xFF is the null offset of an 8-bit tile), 0xFFFF the null offset of
a 16-bit tile.  The last test applies one defect at a time to a packed plan and expects the check to name it."""
import numpy as np
import pytest

import synth
from rphm_desc import (DIRECT16, DIRECT32, MASK, NO_TILES, STREAM_DEFAULTS as DEFAULTS, WIN8, desc_from_arrays, oracle_arrays,
                       pipeline_desc, stream_check)

BAD_PLAN = 200 + 6                     # plancheck_stream: 200 + packPlan's status (BSMR_ERR_BAD_PLAN)


@pytest.fixture(scope="module")
def streamcheck(engine):
    def run(case, **kwargs):
        """case: (desc, keep, ro, ci) of `described`.  Returns (code, report)."""
        d, _, ro, ci = case
        return stream_check(d, ro, ci, **kwargs)
    return run


def described(engine, rows, cols, ro, ci, delta, order=None):
    """the RPHM of the host pipeline (its own row order), or of the oracle for the row order `order`"""
    ro, ci = np.ascontiguousarray(ro, dtype=np.uint32), np.ascontiguousarray(ci, dtype=np.uint32)
    if order is None:
        _, d, keep = pipeline_desc(engine, rows, cols, ro, ci, 0.3, delta)
    else:
        d, keep = desc_from_arrays(engine, rows, cols, int(ci.size), oracle_arrays(rows, cols, ro, ci, order, delta))
    return d, keep, ro, ci


# ------------------------------------------------------------------------------------------------------------------
# patterns
# ------------------------------------------------------------------------------------------------------------------
PATTERNS = {
    "rand-150x220": lambda: synth.random_pattern(150, 220, 5000, seed=11, empty_rows=9),
    "rand-130x500": lambda: synth.random_pattern(130, 500, 4000, seed=21, empty_rows=4),
    "community-330": lambda: synth.community_graph(n=330, avg_degree=40, communities=6, seed=32),
    "nips-330x1500": lambda: synth.nips_like(rows=330, cols=1500, nnz=42000, seed=3),
    "outlier-row": lambda: synth.outlier_row_pattern(),
    "file-order-rows": lambda: synth.file_order_rows(False),
    "file-order-rows-sorted": lambda: synth.file_order_rows(True),
    "tiny-5x5": lambda: synth.random_pattern(5, 5, 2, seed=12),
    "one-row": lambda: synth.random_pattern(1, 40, 30, seed=71),
}
LARGE = ("nips-330x1500", "outlier-row")        # ~43 000 entries: ten times the others' time per check
DELTAS = (0.0, 0.1, 0.3, 1.1)


def option_grid(large):
    """Every value of every option, combinations trimmed: groups x blocks per item x the three destination forms in full;
    the other options each against the groups or forms they interact with."""
    forms = (dict(), dict(mask_tiles=0), dict(staged=0))
    if large:
        grid = [dict(group=g, blocks_per_item=b, **forms[(g + b) % 3]) for g in (1, 2, 4) for b in (1, 3, 32)]
    else:
        grid = [dict(group=g, blocks_per_item=b, **f) for g in (1, 2, 4) for b in (1, 3, 32) for f in forms]
    grid += [dict(group=g, wide=1) for g in ((1, 4) if large else (1, 2, 4))]
    grid += [dict(group=g, column_order=0, staged=s, blocks_per_item=3) for g, s in (((1, 1), (4, 0)) if large else ((1, 1), (1, 0), (4, 1), (4, 0)))]
    grid += [dict(free_residue=1, sparse_per_item=32), dict(free_residue=1), dict(sparse_per_item=32, blocks_per_item=3)]
    grid += [dict(item_order=o, item_span=s, group=g, blocks_per_item=3)
             for o in (1, 2) for s in (0, 64) for g in ((1,) if large else (1, 4))]
    grid += [dict(item_span=64), dict(item_span=64, group=2, blocks_per_item=3, mask_tiles=0)]
    return grid


RULES = (dict(), dict(mask_tiles=0, blocks_per_item=3), dict(group=2), dict(group=4, staged=0))   # with promotion / eviction


def check_report(r, nnz, o, where):
    """what the report must say whatever the pattern"""
    o = dict(DEFAULTS, **o)
    assert r["dense"] + r["residue"] == nnz, where
    assert (r["encoding"] in (MASK, WIN8)) == bool(r["staged"]) or r["encoding"] == NO_TILES, where
    assert (r["encoding"] == NO_TILES) == (r["blocks"] == 0), where
    if o["wide"]:
        assert r["encoding"] in (DIRECT32, NO_TILES) and not r["too_wide"], where
    elif not o["staged"]:
        assert r["encoding"] in (DIRECT16, DIRECT32, NO_TILES) and not r["too_wide"], where
    elif r["blocks"]:
        assert r["too_wide"] == (r["encoding"] in (DIRECT16, DIRECT32)), where
    if not o["mask_tiles"]:
        assert r["encoding"] != MASK, where
    assert r["items"] >= -(-r["blocks"] // max(1, o["blocks_per_item"])), where
    assert r["residue_items"] >= -(-r["residue"] // max(32, o["sparse_per_item"])), where


@pytest.mark.parametrize("name", list(PATTERNS))
def test_stream_format_reads_back_as_the_csr(engine, streamcheck, name):
    """Every pattern x delta x row order (the pipeline's and a shuffled one) x the option grid: the check returns 0.
    With promotion and eviction applied first (a smaller grid): 0 again, and where a rule applies the entries it reports
    are the entries that changed sides."""
    rows, cols, ro, ci = PATTERNS[name]()
    nnz = int(np.asarray(ci).size)
    shuffled = np.random.default_rng(5).permutation(rows).astype(np.uint32)
    grid = option_grid(name in LARGE)
    seen = {"encodings": set(), "promoted": 0, "evicted": 0, "checks": 0}
    for delta in DELTAS:
        for order in (None, shuffled):
            if name in LARGE and order is not None and delta in (0.0, 1.1):
                continue                      # (the large patterns: the shuffled order where the plan is a hybrid)
            case = described(engine, rows, cols, ro, ci, delta, order)
            for o in grid:
                where = f"{name} delta={delta} order={'pipeline' if order is None else 'shuffled'} {o}"
                rc, r = streamcheck(case, **o)
                assert rc == 0, f"{where}: invariant {rc} violated: {r}"
                check_report(r, nnz, o, where)
                seen["encodings"].add(r["encoding"])
                seen["checks"] += 1
            for o in RULES[:2] if name in LARGE else RULES:
                rc, plain = streamcheck(case, **o)
                assert rc == 0, (name, delta, o, rc)
                for promote, evict in ((1, 0), (0, 1), (1, 1)):
                    where = f"{name} delta={delta} order={'pipeline' if order is None else 'shuffled'} {o} promote={promote} evict={evict}"
                    rc, r = streamcheck(case, promote=promote, evict=evict, **o)
                    assert rc == 0, f"{where}: invariant {rc} violated: {r}"
                    check_report(r, nnz, o, where)
                    assert r["dense"] == plain["dense"] + r["promoted"] - r["evicted"], where      # the entries moved, no others
                    assert r["residue"] == plain["residue"] - r["promoted"] + r["evicted"], where
                    if not promote:
                        assert r["promoted"] == 0, where
                    if not evict:
                        assert r["evicted"] == 0, where
                    if r["evicted"] and dict(DEFAULTS, **o)["group"] == 1 and dict(DEFAULTS, **o)["staged"] and not promote:
                        assert plain["too_wide"] and not r["too_wide"] and r["encoding"] in (MASK, WIN8), where
                    seen["promoted"] += r["promoted"]
                    seen["evicted"] += r["evicted"]
                    seen["checks"] += 1
    print(f"{name}: {seen['checks']} plans checked, encodings {sorted(seen['encodings'])}, promoted {seen['promoted']}, evicted {seen['evicted']}")
    # the cases are what they are meant to be
    if name in ("rand-150x220", "community-330", "nips-330x1500"):
        assert seen["promoted"] > 0 and {MASK, WIN8, DIRECT16, DIRECT32, NO_TILES} <= seen["encodings"], seen
    if name in ("outlier-row", "nips-330x1500"):
        assert seen["evicted"] > 0, seen
    if name == "file-order-rows":
        assert MASK not in seen["encodings"] and WIN8 not in seen["encodings"], seen     # every block is wider than a window


def test_file_order_rows_take_direct_offsets(engine, streamcheck):
    """Unsorted CSR rows: the staged form is asked for, one block spans more than a window, the plan falls back to 16-bit
    offsets from the row's first dense entry; the same rows sorted keep their windows."""
    for delta in (0.0, 0.1):
        rc, r = streamcheck(described(engine, *synth.file_order_rows(False), delta))
        assert rc == 0 and r["too_wide"] == 1 and r["staged"] == 0 and r["encoding"] == DIRECT16, (rc, r)
        rc, r = streamcheck(described(engine, *synth.file_order_rows(True), delta))
        assert rc == 0 and r["too_wide"] == 0 and r["staged"] == 1 and r["encoding"] == (MASK if delta == 0.0 else WIN8), (rc, r)


# ------------------------------------------------------------------------------------------------------------------
# boundaries
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 2, 4])
def test_window_width_boundary(engine, streamcheck, H):
    for F, wide in ((239, False), (240, True)):
        case = described(engine, *synth.window_pattern(F), 0.3)
        for mask_tiles in (0, 1):
            rc, r = streamcheck(case, group=H, mask_tiles=mask_tiles)
            assert rc == 0, (F, H, rc, r)
            assert r["dense"] == 256 and r["residue"] == F and r["blocks"] == 1, (F, r)
            assert r["too_wide"] == wide and r["staged"] == (not wide), (F, H, r)
            # (never the mask form: row 0's residue entries lie between its dense ones, whose offsets are not consecutive)
            assert r["encoding"] == (DIRECT16 if wide else WIN8), (F, H, r)
        rc, r = streamcheck(case, group=H, evict=1)
        assert rc == 0 and r["too_wide"] == 0 and (r["evicted"] > 0) == wide, (F, H, rc, r)


@pytest.mark.parametrize("n,encoding", [(65535, DIRECT16), (65536, DIRECT32), (65537, DIRECT32)])
def test_offset_width_boundary(engine, streamcheck, n, encoding):
    case = described(engine, *synth.long_row_pattern(n), 0.0)
    for H in (1, 4):
        rc, r = streamcheck(case, group=H)
        assert rc == 0, (n, H, rc, r)
        assert r["dense"] == n + 15 * 40 and r["residue"] == 0, r
        assert r["too_wide"] == 1 and r["encoding"] == encoding, (n, H, r)     # the packer's own choice, nothing forced
    rc, r = streamcheck(case, staged=0)
    assert rc == 0 and r["too_wide"] == 0 and r["encoding"] == encoding, (n, rc, r)


def repeated_entries_pattern():
    """64 x 48, 20 columns per row, three of them stored twice (tests/test_plan_host.py:
    test_promotion_with_repeated_entries)"""
    rows, cols = 64, 48
    rng = np.random.default_rng(3)
    ci, ro = [], [0]
    for _ in range(rows):
        c = np.sort(rng.choice(cols, size=20, replace=False))
        ci.extend(np.sort(np.concatenate([c, c[:3]])).tolist())
        ro.append(len(ci))
    return rows, cols, np.array(ro, dtype=np.uint32), np.array(ci, dtype=np.uint32)


def test_repeated_entries(engine, streamcheck):
    """The same (row, column) stored twice (CSR.from_arrays takes it; the file loaders do not).  While the column stays in
    the residue both copies are entries of the plan, and a promoted block cell takes one of them.  Where the RPHM makes
    the column dense its block cell holds one copy, the other has no place, and packPlan refuses the arrays
    (BSMR_ERR_BAD_PLAN, include/bsmr_hip.h at bsmr_plan_create)."""
    rows, cols, ro, ci = repeated_entries_pattern()
    case = described(engine, rows, cols, ro, ci, 1.1)
    for o in (dict(), dict(free_residue=1), dict(group=4, sparse_per_item=32)):
        rc, r = streamcheck(case, **o)
        assert rc == 0 and r["residue"] == ci.size and r["dense"] == 0, (o, rc, r)
        rc, r = streamcheck(case, promote=1, **o)
        assert rc == 0 and r["promoted"] == ci.size - 3 * rows and r["residue"] == 3 * rows, (o, rc, r)   # the second copies stay
    for delta in (0.0, 0.3):
        rc, r = streamcheck(described(engine, rows, cols, ro, ci, delta))
        assert rc == BAD_PLAN and r["pack_status"] == 6, (delta, rc, r)


# ------------------------------------------------------------------------------------------------------------------
# the check can fail
# ------------------------------------------------------------------------------------------------------------------
# mutation (tests/native/plancheck.hip: streamMutate): (what, delta, options, the invariant that must name it).
# Why these codes: 6 an entry in a tile the kernels skip; 14 a tile the kernels compute that holds nothing; 17 a window
# position the LDS-staged kernel would store from LDS nobody wrote; 8 a result the LDS-staged kernel would not store; 7 an
# offset at or past winLen; 12 / 13 the entry reached is not the one at the group's row / the block's column (a shifted or
# exchanged base lands on a neighbour in the same CSR row, whose column differs); 25 a CSR index reached twice.
MUTATIONS = {
    1: ("two offsets of an 8-bit tile row swapped", 0.1, dict(), 13),
    2: ("a set blockMask bit cleared", 0.1, dict(), 6),
    3: ("a clear blockMask bit set", 0.1, dict(group=4), 14),
    4: ("a winMask bit set that nobody owns", 0.1, dict(), 17),
    5: ("an owned winMask bit cleared", 0.1, dict(), 8),
    6: ("a winLen shortened by one", 0.1, dict(), 7),
    7: ("one added to a rowBase", 0.1, dict(), 13),
    8: ("two blockCols of a block swapped", 0.1, dict(), 13),
    9: ("two groupRows swapped", 0.1, dict(), 12),
    10: ("rowBase / winLen / winMask exchanged between two items of a group", 0.1, dict(blocks_per_item=3), 13),
    11: ("a residue entry repeated in place of its neighbour", 0.1, dict(), 25),
    12: ("a mask-form first byte bumped", 0.0, dict(), 13),
    13: ("a bit of a mask-form column mask moved", 0.0, dict(), 13),
}
# the same defects on the other encodings and forms that have a place for them
MORE_MUTATIONS = [(2, 0.0, dict(), 6), (5, 0.0, dict(), 8), (6, 0.0, dict(), 7), (7, 0.0, dict(), 13), (9, 0.0, dict(), 12),
                  (10, 0.0, dict(blocks_per_item=3), 13), (2, 0.1, dict(staged=0), 6), (8, 0.1, dict(wide=1), 13),
                  (9, 0.1, dict(staged=0, group=2), 12), (11, 0.1, dict(free_residue=1), 25), (3, 0.1, dict(group=2, staged=0), 14)]


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_every_mutation_is_rejected(engine, streamcheck, mutation):
    what, delta, o, code = MUTATIONS[mutation]
    case = described(engine, *PATTERNS["rand-150x220"](), delta)
    rc, r = streamcheck(case, **o)
    assert rc == 0 and r["encoding"] == (MASK if delta == 0.0 else WIN8), (what, rc, r)     # sound before the defect
    rc, r = streamcheck(case, mutate=mutation, **o)
    assert r["mutated"] == 1, f"{what}: the plan has no place for it"
    assert rc == code, f"{what}: expected invariant {code}, got {rc}"
    for m, d2, o2, code2 in MORE_MUTATIONS:
        if m != mutation:
            continue
        case2 = described(engine, *PATTERNS["rand-150x220"](), d2)
        assert streamcheck(case2, **o2)[0] == 0
        rc, r = streamcheck(case2, mutate=m, **o2)
        assert r["mutated"] == 1 and rc == code2, (what, d2, o2, rc, r)
