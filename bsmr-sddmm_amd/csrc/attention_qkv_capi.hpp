// One-pass sparse attention (include/bsmr_hip.h "One-pass sparse attention"): the checks, the workspace and the launches of
// csrc/attention_qkv_kernels.hpp on the SDDMM backward's per-pattern handle - the row lists and the row chunk table that
// drive bsmr_spmm's row direction and the fused softmax . V.
//
// Workspace of a call with (Kv, num_batches), in floats, from the start of the handle's workspace: the chunk partial rows
// [b][slots][Kv], then s_c [b][slots], then m_c [b][slots] (slots = the row direction's chunk slots).  Nothing of size nnz;
// a handle without split rows needs none.  The offsets depend on (Kv, num_batches) alone.
// The kernels and their launches are a translation unit of their own, csrc/attention_qkv.hip (attention_qkv_launch.hpp).
// Included at the end of bsmr_capi.hip, after attention_capi.hpp.
#pragma once

#include "attention_qkv_launch.hpp"

namespace {

constexpr uint32_t kQkvMaxK = 512;   // one wave holds a whole row of Q (K) and of acc (Kv)

bool qkvDim(uint32_t k) { return k != 0 && (k & 31u) == 0 && k <= kQkvMaxK; }

uint64_t qkvWorkFloats(const bsmr_backward* bw, uint32_t Kv, uint32_t nb) { return (uint64_t)bw->numSlots[0] * (Kv + 2u) * nb; }

int runAttentionQkv(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const uint16_t* Q, const uint16_t* Kt,
                    const uint16_t* V, uint16_t* O, float* m, float* sOut, uint32_t nb, int mode, hipStream_t s) {
    if (int st = growWork(bw, qkvWorkFloats(bw, Kv, nb))) return st;
    const uint32_t slots = bw->numSlots[0];
    float* partial = bw->work;
    float* sPart = bw->work + (uint64_t)slots * Kv * nb;
    float* mPart = sPart + (uint64_t)slots * nb;
    BSMR_HIP(bsmrLaunchAttnQkv(bw->items[0].get(), bw->numItems[0], bw->splits[0].get(), bw->numSplits[0], bw->colIndices, scale, Q, Kt, V, O,
                               m, sOut, partial, sPart, mPart, K, Kv, bw->M, bw->N, slots, nb, mode == BSMR_COMPUTE_BF16, s));
    return BSMR_OK;
}

}  // namespace

extern "C" {

int bsmr_sparse_attention_qkv_reserve(bsmr_backward* bw, uint32_t K, uint32_t Kv, uint32_t num_batches) {
    if (!bw) return BSMR_ERR_INVALID_ARG;
    if (!qkvDim(K) || !qkvDim(Kv)) return BSMR_ERR_UNSUPPORTED_K;
    if (num_batches > 65535u) return BSMR_ERR_INVALID_ARG;
    BSMR_HIP(hipSetDevice(bw->device));
    return growWork(bw, qkvWorkFloats(bw, Kv, std::max(num_batches, 1u)));
}

int bsmr_sparse_attention_qkv_16(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                 const void* Kt16_dev, const void* V16_dev, void* O16_dev, float* m_dev, float* s_dev,
                                 uint32_t num_batches, int compute_mode, void* stream) {
    if (!bw || !std::isfinite(scale)) return BSMR_ERR_INVALID_ARG;
    if (!qkvDim(K) || !qkvDim(Kv)) return BSMR_ERR_UNSUPPORTED_K;
    // (the order of bsmr_sparse_attention_16 from here on: compute_mode, the batches, then the pointers)
    if (int st = checkAttentionCall(bw, Kv, scale, true, compute_mode, num_batches, {Q16_dev, Kt16_dev, V16_dev}, {},
                                    {O16_dev, m_dev, s_dev}))
        return st;
    if (!aligned16(O16_dev) || !aligned4(m_dev) || !aligned4(s_dev)) return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    return runAttentionQkv(bw, K, Kv, scale, static_cast<const uint16_t*>(Q16_dev), static_cast<const uint16_t*>(Kt16_dev),
                           static_cast<const uint16_t*>(V16_dev), static_cast<uint16_t*>(O16_dev), m_dev, s_dev, num_batches,
                           compute_mode, static_cast<hipStream_t>(stream));
}

}  // extern "C"
