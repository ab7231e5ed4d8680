// The fused softmax . V of sparse attention and its backward (include/bsmr_hip.h "Fused sparse attention"), on the SDDMM
// backward's per-pattern handle: its row lists and row chunk table drive csrc/attention_kernels.hpp as they drive
// bsmr_spmm's row direction.
//
// Workspace of a call with (Kv, num_batches), in floats: the region bsmr_backward_reserve(Kv, num_batches) covers
// (chunk partials [b][slots][Kv], then the permuted values - so the transposed bsmr_spmm of the same step fits), and
// behind it the two regions of these calls: the partial row sums [b][numSlots[0]] and D [b][M].  The offsets depend on
// (Kv, num_batches) alone, never on what the workspace holds.
// Included at the end of bsmr_capi.hip, after softmax_capi.hpp.
#pragma once

#include <cmath>
#include <initializer_list>

#include "attention_kernels.hpp"

namespace {

uint64_t attnSumsOffset(const bsmr_backward* bw, uint32_t Kv, uint32_t nb) { return workFloatsFor(bw, Kv, nb, bw->permuteV); }

uint64_t attnWorkFloats(const bsmr_backward* bw, uint32_t Kv, uint32_t nb) {
    return attnSumsOffset(bw, Kv, nb) + ((uint64_t)bw->numSlots[0] + bw->M) * nb;
}

// The checks of all four calls, before any device call.  mode16: the call has a compute_mode (F16 / BF16 only).
// rows: the operand matrices (16-byte aligned); values: the value arrays (4-byte aligned); out: arrays that are
// written even with nnz = 0 and so are NULL only when S has no rows.  Everything else may be NULL only with nnz = 0.
int checkAttentionCall(const bsmr_backward* bw, uint32_t Kv, float scale, bool mode16, int mode, uint32_t nb,
                       std::initializer_list<const void*> rows, std::initializer_list<const void*> values,
                       std::initializer_list<const void*> out) {
    if (!bw || !std::isfinite(scale)) return BSMR_ERR_INVALID_ARG;
    if (Kv == 0 || (Kv & 31u)) return BSMR_ERR_UNSUPPORTED_K;
    if (mode16 && mode != BSMR_COMPUTE_F16 && mode != BSMR_COMPUTE_BF16) return BSMR_ERR_INVALID_ARG;
    if (nb > 65535u) return BSMR_ERR_INVALID_ARG;
    for (const void* p : rows)
        if ((bw->nnz && !p) || !aligned16(p)) return BSMR_ERR_INVALID_ARG;
    for (const void* p : values)
        if ((bw->nnz && !p) || !aligned4(p)) return BSMR_ERR_INVALID_ARG;
    for (const void* p : out)
        if (bw->M && !p) return BSMR_ERR_INVALID_ARG;
    return BSMR_OK;
}

uint32_t attnShortBlocks(const bsmr_backward* bw) { return (uint32_t)(((uint64_t)bw->M + 3u) / 4u); }

// m of every row: the pass in front of the gather
int launchAttnRowMax(const bsmr_backward* bw, float scale, const float* P, float* m, uint32_t nb, hipStream_t s) {
    const uint32_t shortBlocks = attnShortBlocks(bw);
    if (shortBlocks + bw->numSplits[0]) {
        hipLaunchKernelGGL(bsmr::attnRowMax, dim3(shortBlocks + bw->numSplits[0], nb), dim3(256), 0, s, bw->rowOffsets,
                           bw->splits[0], bw->M, shortBlocks, scale, P, m, (uint64_t)bw->nnz);
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

// withMode with the fp32 arm of attnReduce and attnRowDot: MODE -1 for an fp32 O
template <typename F>
auto withModeOrF32(int mode, F&& fn) {
    return mode == BSMR_COMPUTE_F16 ? fn(Int<0>{}) : mode == BSMR_COMPUTE_BF16 ? fn(Int<1>{}) : fn(Int<-1>{});
}

// The split rows: the pass behind the gather.  mode: BSMR_COMPUTE_F32 for an fp32 O, else its 16-bit format.
int launchAttnReduce(const bsmr_backward* bw, uint32_t Kv, const float* partial, const float* sPart, const float* m, void* O,
                     float* sOut, uint32_t nb, int mode, hipStream_t s) {
    if (bw->numSplits[0]) {
        const uint64_t threads = (uint64_t)bw->numSplits[0] * (Kv / 4u);
        const dim3 rgrid((uint32_t)((threads + 255u) / 256u), nb);
        withModeOrF32(mode, [&](auto MODE) {
            hipLaunchKernelGGL(bsmr::attnReduce<MODE()>, rgrid, dim3(256), 0, s, bw->splits[0], bw->numSplits[0], partial, sPart,
                               m, O, sOut, Kv, bw->M, bw->numSlots[0]);
        });
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

// t: the element types of V and O as in runGather (O has V's 16-bit format, or t.mode's with fp8 / fp4 rows; y16 is not read)
int runAttention(bsmr_backward* bw, uint32_t Kv, float scale, const float* P, const void* V, void* O, float* m, float* sOut,
                 uint32_t nb, hipStream_t s, const GatherTypes& t = {}) {
    if (int st = growWork(bw, attnWorkFloats(bw, Kv, nb))) return st;
    float* partial = bw->work;
    float* sPart = bw->work + attnSumsOffset(bw, Kv, nb);
    const uint32_t M = bw->M, slots = bw->numSlots[0];
    const uint64_t nnz = bw->nnz, xB = (uint64_t)bw->N * Kv;
    if (int st = launchAttnRowMax(bw, scale, P, m, nb, s)) return st;
    const RowKind kind = rowKind(t);
    const GatherGeometry g = gatherGeometry(bw, Kv, bw->numItems[0], nb, kind);
    if (g.units) {
        // (what every attention gather takes; `mx`: the two MX arguments of the fp8 kernels)
        auto launch = [&](auto kernel, auto* X, auto* Out, auto... mx) {
            hipLaunchKernelGGL(kernel, g.grid, dim3(256), 0, s, bw->items[0], bw->numItems[0], g.slices, bw->colIndices, scale, P,
                               m, X, Out, sOut, partial, sPart, Kv, M, slots, nnz, xB, mx...);
        };
        uint16_t* O16 = static_cast<uint16_t*>(O);
        if (kind == RowKind::FP8) {
            const uint8_t* V8 = static_cast<const uint8_t*>(V);
            withGatherShape<RowKind::FP8>(g, [&](auto W, auto LANES) {
                withMode(t.mode, [&](auto MODE) {
                    withFp8(t.fp8, [&](auto FMT) {
                        if (t.scales) launch(bsmr::attnGather8<W(), LANES(), MODE(), FMT(), true>, V8, O16, t.scales, xB / 32u);
                        else launch(bsmr::attnGather8<W(), LANES(), MODE(), FMT()>, V8, O16, kNoScales, (uint64_t)0);
                    });
                });
            });
        } else if (kind == RowKind::FP4) {   // xB elements of a batch are xB / 2 bytes of codes and xB / 32 scale bytes
            const uint8_t* V4 = static_cast<const uint8_t*>(V);
            withGatherShape<RowKind::FP4>(g, [&](auto W, auto LANES) {
                withMode(t.mode, [&](auto MODE) {
                    hipLaunchKernelGGL((bsmr::attnGather4<W(), LANES(), MODE()>), g.grid, dim3(256), 0, s, bw->items[0],
                                       bw->numItems[0], g.slices, bw->colIndices, scale, P, m, V4, O16, sOut, partial, sPart, Kv, M,
                                       slots, nnz, xB / 2u, t.scales, xB / 32u);
                });
            });
        } else if (kind == RowKind::B16) {
            withGatherShape<RowKind::B16>(g, [&](auto W, auto LANES) {
                withMode(t.mode, [&](auto MODE) {
                    launch(bsmr::attnGather16<W(), LANES(), MODE()>, static_cast<const uint16_t*>(V), O16);
                });
            });
        } else {
            withGatherShape<RowKind::F32>(g, [&](auto W, auto) {
                launch(bsmr::attnGather<W()>, static_cast<const float*>(V), static_cast<float*>(O));
            });
        }
        BSMR_HIP(hipGetLastError());
    }
    return launchAttnReduce(bw, Kv, partial, sPart, m, O, sOut, nb, t.mode, s);
}

int runAttentionBackward(bsmr_backward* bw, uint32_t Kv, float scale, const float* P, const float* m, const float* sIn,
                         const float* dW, const void* O, const void* dO, float* dP, float* Wout, uint32_t nb, int mode,
                         hipStream_t s) {
    if (int st = growWork(bw, attnWorkFloats(bw, Kv, nb))) return st;
    float* D = bw->work + attnSumsOffset(bw, Kv, nb) + (uint64_t)bw->numSlots[0] * nb;
    const uint64_t rows = (uint64_t)bw->M * nb;
    const dim3 dgrid((uint32_t)((rows + 7u) / 8u));
    withModeOrF32(mode, [&](auto MODE) { hipLaunchKernelGGL(bsmr::attnRowDot<MODE()>, dgrid, dim3(256), 0, s, O, dO, D, rows, Kv); });
    BSMR_HIP(hipGetLastError());
    const uint32_t shortBlocks = attnShortBlocks(bw);
    hipLaunchKernelGGL(bsmr::attnValuesBackward, dim3(shortBlocks + bw->numSplits[0], nb), dim3(256), 0, s, bw->rowOffsets,
                       bw->splits[0], bw->M, shortBlocks, scale, P, m, sIn, D, dW, dP, Wout, (uint64_t)bw->nnz);
    BSMR_HIP(hipGetLastError());
    return BSMR_OK;
}

}  // namespace

extern "C" {

int bsmr_sparse_attention_reserve(bsmr_backward* bw, uint32_t Kv, uint32_t num_batches) {
    if (int st = checkBackwardCall(bw, Kv, num_batches)) return st;
    BSMR_HIP(hipSetDevice(bw->device));
    return growWork(bw, attnWorkFloats(bw, Kv, std::max(num_batches, 1u)));
}

int bsmr_sparse_attention(bsmr_backward* bw, uint32_t Kv, float scale, const float* P_dev, const float* V_dev, float* O_dev,
                          float* m_dev, float* s_dev, uint32_t num_batches, void* stream) {
    if (int st = checkAttentionCall(bw, Kv, scale, false, 0, num_batches, {V_dev}, {P_dev}, {O_dev, m_dev, s_dev})) return st;
    if (!aligned16(O_dev) || !aligned4(m_dev) || !aligned4(s_dev)) return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    return runAttention(bw, Kv, scale, P_dev, V_dev, O_dev, m_dev, s_dev, num_batches, static_cast<hipStream_t>(stream));
}

int bsmr_sparse_attention_16(bsmr_backward* bw, uint32_t Kv, float scale, const float* P_dev, const void* V16_dev,
                             void* O16_dev, float* m_dev, float* s_dev, uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkAttentionCall(bw, Kv, scale, true, compute_mode, num_batches, {V16_dev}, {P_dev}, {O16_dev, m_dev, s_dev}))
        return st;
    if (!aligned16(O16_dev) || !aligned4(m_dev) || !aligned4(s_dev)) return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    return runAttention(bw, Kv, scale, P_dev, V16_dev, O16_dev, m_dev, s_dev, num_batches, static_cast<hipStream_t>(stream),
                        {compute_mode, true});
}

int bsmr_sparse_attention_backward(bsmr_backward* bw, uint32_t Kv, float scale, const float* P_dev, const float* m_dev,
                                   const float* s_dev, const float* dW_dev, const float* O_dev, const float* dO_dev,
                                   float* dP_dev, float* W_dev, uint32_t num_batches, void* stream) {
    if (int st = checkAttentionCall(bw, Kv, scale, false, 0, num_batches, {O_dev, dO_dev},
                                    {P_dev, m_dev, s_dev, dW_dev, dP_dev, W_dev}, {}))
        return st;
    if (num_batches == 0 || bw->nnz == 0) return BSMR_OK;   // no entry: nothing to write
    BSMR_HIP(hipSetDevice(bw->device));
    return runAttentionBackward(bw, Kv, scale, P_dev, m_dev, s_dev, dW_dev, O_dev, dO_dev, dP_dev, W_dev, num_batches,
                                BSMR_COMPUTE_F32, static_cast<hipStream_t>(stream));
}

int bsmr_sparse_attention_backward_16(bsmr_backward* bw, uint32_t Kv, float scale, const float* P_dev, const float* m_dev,
                                      const float* s_dev, const float* dW_dev, const void* O16_dev, const void* dO16_dev,
                                      float* dP_dev, float* W_dev, uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkAttentionCall(bw, Kv, scale, true, compute_mode, num_batches, {O16_dev, dO16_dev},
                                    {P_dev, m_dev, s_dev, dW_dev, dP_dev, W_dev}, {}))
        return st;
    if (num_batches == 0 || bw->nnz == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    return runAttentionBackward(bw, Kv, scale, P_dev, m_dev, s_dev, dW_dev, O16_dev, dO16_dev, dP_dev, W_dev, num_batches,
                                compute_mode, static_cast<hipStream_t>(stream));
}

}  // extern "C"
