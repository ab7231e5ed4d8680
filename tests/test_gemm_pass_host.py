"""packGemm deals the rows of a row half over the half's PASSES as well (csrc/gemm_format.hpp, step 0a), so that the
(wave, pass) entry lists of the mask epilogue come out about equally long: the kernels take one trip of 256 words (8 x 5
tile blocks) or 512 words (8 x 4) per list in straight-line code and loop only for what is longer.  Checked through
tests/native/plancheck.hip, which reads the format the way the kernel does; no GPU."""
import pytest

import gemm_patterns
import synth
from test_plan_host import gemmcheck  # noqa: F401  (the fixture)


def test_headline_lists_fit_one_trip_or_nearly(gemmcheck):
    """The bench's headline pattern: with the rows' position in their half = the dealing round, the heaviest rows all sat in
    pass 0 and its longest list held 448 words at 16 x 20 (861 lists above one trip of 256); dealt over the passes by entry
    count the longest is 280.  The caps leave room for another tie order, not for the old placement."""
    rows, cols, ro, ci = synth.nips_like()
    rc, r = gemmcheck(rows, cols, ro, ci, 0.3, 0.0, 16, 20)
    print("16 x 20:", r)
    assert rc == 0, f"invariant {rc} violated: {r}"
    assert r["entries"] == r["rphm_dense"] > 0
    assert r["longest_list"] <= 320, r
    rc, r = gemmcheck(rows, cols, ro, ci, 0.3, 0.0, 16, 16)
    print("16 x 16:", r)
    assert rc == 0, f"invariant {rc} violated: {r}"
    assert r["longest_list"] <= 512, r


def test_small_pattern_with_a_ragged_last_group(gemmcheck):
    """21 panels (a ragged second row group) x 94 column blocks at 16 x 20: 588 words before, 288 dealt over the passes."""
    rows, cols, ro, ci = synth.nips_like(rows=330, cols=1500, nnz=42000, seed=3)
    rc, r = gemmcheck(rows, cols, ro, ci, 0.3, 0.0, 16, 20)
    print(r)
    assert rc == 0, f"invariant {rc} violated: {r}"
    assert r["entries"] == r["rphm_dense"] > 0
    assert r["longest_list"] <= 320, r


@pytest.mark.parametrize("blocks", sorted(gemm_patterns.CASES))
def test_one_tile_patterns_make_the_lists_they_claim(engine, blocks):
    """The constructed patterns of tests/test_gpu_gemm_passes.py: one macro-tile, the format passes the brute-force reading,
    and the longest list is wave 0's - exactly the case's entry count, padded to 4 words."""
    for per_pass in gemm_patterns.CASES[blocks]:
        rc, longest, items, entries = gemm_patterns.longest_list(engine, blocks, per_pass)
        assert rc == 0 and items == 1, (per_pass, rc, items)
        assert entries == sum(per_pass) + gemm_patterns.ROWS
        if max(per_pass) > 64:          # (the last column's lists hold at most 64 entries)
            assert longest == (max(per_pass) + 3) // 4 * 4, (per_pass, longest)
