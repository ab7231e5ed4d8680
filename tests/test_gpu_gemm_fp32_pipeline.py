"""The GEMM engine's kernel on the caller's fp32 operands (denseGemmCvt, csrc/gemm_kernels.hpp) keeps requests two slices
ahead: B's fp32 slices through two private LDS stages, A's rows through registers, one in-order counter for both.  What
can go wrong there is a slice taken from the wrong stage, registers of the wrong slice, or a wait that lets a request pass
that has not landed - so the results are pinned bit for bit, and on operands where every 32-k slice is told apart exactly:
  * all four macro-tile shapes x K = 64 (no steady-state iteration of the K loop) and 128 (exactly one) x fp16 / bf16
    against the streaming engine on the 16-bit copies, entry by entry as uint32, on a pattern with a ragged last row
    group and a ragged last 16-column block;
  * small integers, exact in fp16 and bf16, with A (then B) non-zero in ONE slice only: P is the integer product;
  * one batched call and one graph replay: bit-identical to the plain call."""
import functools

import numpy as np
import pytest

import synth
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(16, 16), (16, 20), (8, 16), (8, 20)]
ROWS, COLS = 330, 1500          # 21 panels: the last row group is ragged; 1500 = 93 * 16 + 12: so is the last column block


@functools.lru_cache(maxsize=None)
def _pattern():
    rows, cols, ro, ci = synth.nips_like(rows=ROWS, cols=COLS, nnz=42000, seed=3)
    return rows, cols, ro, ci


@functools.lru_cache(maxsize=None)
def _arrays(engine):
    rows, cols, ro, ci = _pattern()
    csr = engine.CSR.from_arrays(rows, cols, ro, ci)
    return csr.nnz, engine.Pipeline(csr, alpha=0.3, delta=0.0, device=-1).arrays()      # all-dense plan


class _Plan:
    """a plan of the pattern with fixed options; call(K, A, B, mode) -> P as numpy (NaN where nothing was written)"""

    def __init__(self, engine, options):
        self.engine = engine
        rows, cols, _, _ = _pattern()
        self.nnz, arrays = _arrays(engine)
        st, self.plan = engine.plan_from_arrays(rows, cols, self.nnz, arrays, device=0, options=options)
        assert st == engine.OK, st

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.engine.plan_destroy(self.plan)

    def call(self, K, A, B, mode):
        dev = _dev()
        tA, tB = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32).ravel()).to(dev), torch.from_numpy(
            np.ascontiguousarray(B, dtype=np.float32).ravel()).to(dev)
        tP = torch.full((self.nnz,), float("nan"), dtype=torch.float32, device=dev)
        self.engine.sddmm(self.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), mode, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        return tP.cpu().numpy()

    def group(self, K):
        import ctypes as C
        g, t, u = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self.engine.hip().bsmr_plan_dense_choice(self.plan, K, C.byref(g), C.byref(t), C.byref(u))
        return g.value


def _fp32_options(engine, panels, blocks):
    return engine.plan_options(fold_dense_below=0, dense_engine=engine.ENGINE_GEMM, gemm_panels=panels, gemm_blocks=blocks, gemm_fp32=1,
                               sparse_lowp=0)


@functools.lru_cache(maxsize=None)
def _streamed(engine, K, mode):
    """the streaming engine on the 16-bit copies of make_data operands: computed once per (K, mode), never written to"""
    rows, cols, _, _ = _pattern()
    A, B = engine.make_data(rows * K, 5489), engine.make_data(cols * K, 5490)
    with _Plan(engine, engine.plan_options(fold_dense_below=0, convert_in_kernel=0)) as ref:
        P = ref.call(K, A, B, mode)
    assert not np.isnan(P).any()
    P.setflags(write=False)
    return A, B, P


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("panels,blocks", SHAPES)
def test_fp32_operand_kernel_is_bit_identical_to_the_streaming_engine(engine, panels, blocks, K, mode):
    A, B, ref = _streamed(engine, K, mode)
    with _Plan(engine, _fp32_options(engine, panels, blocks)) as plan:
        got = plan.call(K, A, B, mode)
        assert plan.group(K) == panels, "the GEMM engine must have served the call at this shape"
    assert not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _small_integers(shape, seed):
    """integers -4 .. 4 without 0: exact in fp16 and bf16; a dot product over K <= 128 of them stays below 2^24"""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 5, size=shape) * rng.choice(np.array([-1, 1]), size=shape)
    return v.astype(np.int64)


@pytest.mark.parametrize("K,mode", [(64, 0), (64, 1), (128, 0), (128, 1)])
@pytest.mark.parametrize("panels,blocks", SHAPES)
def test_every_slice_reaches_the_mfma_from_its_own_stage_and_registers(engine, panels, blocks, K, mode):
    """A non-zero only in 32-k slice s (run 1), B non-zero only in slice s (run 2), for every s: P equals the integer
    product exactly.  A stale or swapped fp32 stage of B, or A registers of another slice, is a wrong integer."""
    rows, cols, ro, ci = _pattern()
    r = np.repeat(np.arange(rows), np.diff(ro.astype(np.int64)))
    c = ci.astype(np.int64)
    fullA, fullB = _small_integers((rows, K), 11 + K), _small_integers((cols, K), 12 + K)
    with _Plan(engine, _fp32_options(engine, panels, blocks)) as plan:
        for s in range(K // 32):
            only = np.zeros(K, dtype=np.int64)
            only[32 * s:32 * s + 32] = 1
            for A, B in ((fullA * only, fullB), (fullA, fullB * only)):
                want = np.einsum("ek,ek->e", A[r], B[c]).astype(np.float32)
                got = plan.call(K, A, B, mode)
                assert np.array_equal(got, want), (s, "A" if A is not fullA else "B", int((got != want).sum()))
        assert plan.group(K) == panels


@pytest.mark.parametrize("panels,blocks,K,mode", [(16, 20, 128, 0), (8, 16, 64, 1)])
def test_an_installed_fp32_kernel_choice_computes_the_slice_products(engine, panels, blocks, K, mode):
    """The plans above reach the fp32-operand kernel through the plan's rule (gemm_fp32 = 1), which no query reports for
    an untuned plan.  Here the choice is installed by hand on a tunable plan (bsmr_plan_set_tuned: GEMM engine, this
    macro-tile, cvt_in_kernel = 1 - "launches exactly its kernels") and read back, so the slice-tagged products below are
    the fp32-operand kernel's whatever the rule does."""
    rows, cols, ro, ci = _pattern()
    r = np.repeat(np.arange(rows), np.diff(ro.astype(np.int64)))
    c = ci.astype(np.int64)
    fullA, fullB = _small_integers((rows, K), 21 + K), _small_integers((cols, K), 22 + K)
    with _Plan(engine, engine.plan_options(fold_dense_below=0, dense_engine=engine.ENGINE_TUNED, sparse_lowp=0)) as plan:
        choice = dict(engine=engine.ENGINE_GEMM, group=panels, blocks_per_item=blocks, format=-1, b_only=-1, overlap=-1, cvt_in_kernel=1, waves=0)
        engine.plan_set_tuned(plan.plan, K, choice, mode)
        kept = engine.plan_get_tuned(plan.plan, K, mode)
        assert kept["engine"] == engine.ENGINE_GEMM and kept["cvt_in_kernel"] == 1 and kept["group"] == panels and kept["blocks_per_item"] == blocks
        for s in range(K // 32):
            only = np.zeros(K, dtype=np.int64)
            only[32 * s:32 * s + 32] = 1
            for A, B in ((fullA * only, fullB), (fullA, fullB * only)):
                want = np.einsum("ek,ek->e", A[r], B[c]).astype(np.float32)
                got = plan.call(K, A, B, mode)
                assert np.array_equal(got, want), (s, int((got != want).sum()))
        assert plan.group(K) == panels


def test_batched_call_and_graph_replay_on_fp32_operands(engine):
    """16 x 20 panels x blocks, K = 128: bsmr_sddmm_batch over two problems and a replayed capture of the plain call are
    bit-identical to plain calls."""
    K, mode, nb = 128, 0, 2
    rows, cols, _, _ = _pattern()
    dev = _dev()
    A = np.concatenate([engine.make_data(rows * K, 100 + b) for b in range(nb)])
    B = np.concatenate([engine.make_data(cols * K, 200 + b) for b in range(nb)])
    with _Plan(engine, _fp32_options(engine, 16, 20)) as plan:
        plain = [plan.call(K, A[b * rows * K:(b + 1) * rows * K], B[b * cols * K:(b + 1) * cols * K], mode) for b in range(nb)]
        assert plan.group(K) == 16 and not np.isnan(plain[0]).any() and not np.isnan(plain[1]).any()
        tA, tB = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
        tP = torch.full((nb * plan.nnz,), float("nan"), dtype=torch.float32, device=dev)
        engine.sddmm_batch(plan.plan, K, tA.data_ptr(), tB.data_ptr(), tP.data_ptr(), nb, mode, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        got = tP.cpu().numpy().reshape(nb, plan.nnz)
        for b in range(nb):
            assert np.array_equal(got[b].view(np.uint32), plain[b].view(np.uint32)), f"batch {b}"
        # captured: the plain call on problem 0's operands; replayed, and replayed on problem 1's values behind the same pointers
        assert engine.hip().bsmr_plan_reserve(plan.plan, K) == engine.OK
        one = torch.full((plan.nnz,), float("nan"), dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            engine.sddmm(plan.plan, K, tA.data_ptr(), tB.data_ptr(), one.data_ptr(), mode, side.cuda_stream)
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                engine.sddmm(plan.plan, K, tA.data_ptr(), tB.data_ptr(), one.data_ptr(), mode, torch.cuda.current_stream(dev).cuda_stream)
        one.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(one.cpu().numpy().view(np.uint32), plain[0].view(np.uint32))
        tA[:rows * K].copy_(tA[rows * K:2 * rows * K])
        tB[:cols * K].copy_(tB[cols * K:2 * cols * K])
        one.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(one.cpu().numpy().view(np.uint32), plain[1].view(np.uint32))
