"""The GEMM engine's kernel on the caller's fp32 operands (denseGemmCvt, csrc/gemm_kernels.hpp) takes B's chunks of a 32-k
slice - 8 columns x 128 bytes each, NB / 4 per wave - into registers, as it takes A's, and rounds them from there into the
16-bit LDS stage; the 8 x 5 tile blocks (16 x 20) have one set of registers that holds A's chunks and B's in turn.  What
can go wrong there, beyond what test_gpu_gemm_fp32_pipeline.py pins:
  * a chunk of B rounded into another chunk's rows of the stage, into A's part of it or into the wrong stage - B non-zero
    only in the columns of ONE chunk position of a wave and in ONE slice, for every position (the fifth, which only
    NB = 20 has and A has not, included) and slice: P is the integer product;
  * a set rounded as the other operand's turn - A and B non-zero in slice s only, values from disjoint sets;
  * a piece of the ragged last column block read past B's end - not-a-numbers stand behind both operands.
Small integers, exact in fp16 and bf16; all four macro-tile shapes x K = 64, 128 x both modes."""
import numpy as np
import pytest

from test_gpu_gemm_fp32_pipeline import SHAPES, _Plan, _fp32_options, _pattern, _small_integers, _streamed
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = [(64, 0), (64, 1), (128, 0), (128, 1)]


def _entries():
    rows, cols, ro, ci = _pattern()
    return np.repeat(np.arange(rows), np.diff(ro.astype(np.int64))), ci.astype(np.int64)


def _slice_mask(K, s):
    only = np.zeros(K, dtype=np.int64)
    only[32 * s:32 * s + 32] = 1
    return only


@pytest.mark.parametrize("K,mode", CASES)
@pytest.mark.parametrize("panels,blocks", SHAPES)
def test_every_chunk_of_b_reaches_its_rows_of_the_stage(engine, panels, blocks, K, mode):
    """A strip of 16 * blocks columns is 2 * blocks chunks of 8; chunk c is position c mod (blocks / 4) of the wave that
    owns it.  B keeps its values in the columns of one position and in one slice, and is zero elsewhere."""
    rows, cols, _, _ = _pattern()
    r, c = _entries()
    A, fullB = _small_integers((rows, K), 31 + K), _small_integers((cols, K), 32 + K)
    per_wave = blocks // 4
    position = ((np.arange(cols) % (16 * blocks)) // 8) % per_wave
    with _Plan(engine, _fp32_options(engine, panels, blocks)) as plan:
        for j in range(per_wave):
            for s in range(K // 32):
                B = fullB * (position == j)[:, None] * _slice_mask(K, s)
                want = np.einsum("ek,ek->e", A[r], B[c]).astype(np.float32)
                got = plan.call(K, A, B, mode)
                assert np.array_equal(got, want), (j, s, int((got != want).sum()))
        assert plan.group(K) == panels, "the GEMM engine must have served the calls at this shape"


@pytest.mark.parametrize("K,mode", CASES)
@pytest.mark.parametrize("panels,blocks", SHAPES)
def test_a_set_of_registers_is_rounded_as_the_operand_it_holds(engine, panels, blocks, K, mode):
    """A in +-{1, 2} and B in +-{3, 4}, both non-zero in slice s only: every term of an entry is one of +-{3, 4, 6, 8}.  A set
    taken for the other operand's turn puts A's values where B's belong (or the other way round): other terms, another sum."""
    rows, cols, _, _ = _pattern()
    r, c = _entries()
    rng = np.random.default_rng(41 + K)
    fullA = rng.integers(1, 3, size=(rows, K)) * rng.choice(np.array([-1, 1]), size=(rows, K))
    fullB = rng.integers(3, 5, size=(cols, K)) * rng.choice(np.array([-1, 1]), size=(cols, K))
    with _Plan(engine, _fp32_options(engine, panels, blocks)) as plan:
        for s in range(K // 32):
            A, B = fullA * _slice_mask(K, s), fullB * _slice_mask(K, s)
            want = np.einsum("ek,ek->e", A[r], B[c]).astype(np.float32)
            got = plan.call(K, A, B, mode)
            assert np.array_equal(got, want), (s, int((got != want).sum()))
        assert plan.group(K) == panels


@pytest.mark.parametrize("K,mode", CASES)
@pytest.mark.parametrize("panels,blocks", SHAPES)
def test_the_ragged_last_column_block_reads_nothing_behind_b(engine, panels, blocks, K, mode):
    """The pattern's last 16-column block is 12 wide, and B ends with its last column: the operands are the heads of buffers
    whose tails hold not-a-numbers, P is filled with them.  None may come out, and P is the streaming engine's on the
    16-bit copies, bit for bit."""
    rows, cols, _, _ = _pattern()
    A, B, ref = _streamed(engine, K, mode)
    dev = _dev()
    tail = 64 * K
    tA = torch.full((rows * K + tail,), float("nan"), dtype=torch.float32, device=dev)
    tB = torch.full((cols * K + tail,), float("nan"), dtype=torch.float32, device=dev)
    tA[:rows * K].copy_(torch.from_numpy(A))
    tB[:cols * K].copy_(torch.from_numpy(B))
    with _Plan(engine, _fp32_options(engine, panels, blocks)) as plan:
        tP = torch.full((plan.nnz,), float("nan"), dtype=torch.float32, device=dev)
        engine.sddmm(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), mode, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        got = tP.cpu().numpy()
        assert plan.group(K) == panels
    assert not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
