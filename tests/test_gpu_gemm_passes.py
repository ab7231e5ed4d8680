"""The mask passes of the GEMM engine (csrc/gemm_kernels.hpp: gemmMaskPass) at the list lengths where they change path: a
first trip of 256 words (256 x 320 macro-tiles) or 512 words (256 x 256) in straight-line code, issued for empty lists
too, and an overflow loop that requests a trip ahead.  One macro-tile, natural row and column order, so that a (wave,
pass) list is what the pattern says (tests/gemm_patterns.py; checked on the CPU in tests/test_gemm_pass_host.py): lists
one short of a trip, exactly a trip, one entry more, two trips, two trips and an entry; an empty pass between two others,
an empty first pass, waves without any entry.  P is prefilled with NaN; the result must be the streaming engine's bit for
bit (same casts, same MFMA, same k order), which also says that every entry was stored."""
import numpy as np
import pytest

import gemm_patterns
from test_gpu_gemm import _run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("mode", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("K,fp32", [(64, 1), (128, 1), (256, 0)], ids=["k64_fp32", "k128_fp32", "k256_16bit"])
@pytest.mark.parametrize("blocks", sorted(gemm_patterns.CASES))
def test_lists_around_the_trip_lengths_are_bit_identical_to_the_streaming_engine(engine, blocks, K, fp32, mode):
    for per_pass in gemm_patterns.CASES[blocks]:
        rows, cols, ro, ci = gemm_patterns.pattern(blocks, per_pass)
        csr = engine.CSR.from_arrays(rows, cols, ro, ci)
        arrays = engine.Pipeline(csr, alpha=0.3, delta=0.0, row_mode=engine.ROWS_IDENTITY, device=-1).arrays()
        A = engine.make_data(rows * K, 5489)
        B = engine.make_data(cols * K, 5490)
        ref, _ = _run(engine, rows, cols, csr.nnz, arrays, K, A, B, mode, engine.plan_options(fold_dense_below=0, convert_in_kernel=0))
        assert not np.isnan(ref).any()
        extra = dict(sparse_lowp=0) if fp32 else {}     # (as tests/test_gpu_gemm.py runs the kernel on fp32 operands)
        got, (group, tiles) = _run(engine, rows, cols, csr.nnz, arrays, K, A, B, mode,
                                   engine.plan_options(fold_dense_below=0, dense_engine=engine.ENGINE_GEMM, gemm_panels=16, gemm_blocks=blocks,
                                                       gemm_fp32=fp32, gemm_balance_columns=0, **extra))
        assert group == 16 and tiles == 16 * blocks, (per_pass, group, tiles)       # the engine ran, on one macro-tile
        assert not np.isnan(got).any(), (per_pass, int(np.isnan(got).sum()))
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), per_pass
