// One-pass sparse attention with grouped key/value heads on a quantised KV cache (include/bsmr_hip.h "One-pass grouped-head
// sparse attention on fp8, MXFP8 and MXFP4 keys and values"): the checks of the ungrouped quantised calls
// (csrc/attention_qkv_kv_capi.hpp, attentionQkvKvCheck), then kv_group and the grouped limit on K and Kv; the workspace of
// csrc/attention_qkv_capi.hpp (fp32 partials indexed by query head: same layout, same reserve call) and the launch of
// csrc/attention_qkv_gqa_kv_kernels.hpp, a translation unit of its own (csrc/attention_qkv_gqa_kv.hip).
// Included at the end of bsmr_capi.hip, after attention_qkv_kv_capi.hpp and attention_qkv_gqa_capi.hpp (kQkvGqaMaxK).
#pragma once

#include "attention_qkv_launch.hpp"

namespace {

int attentionQkvGqaKvCall(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16, const void* Kt,
                          const void* Kts, const void* V, const void* Vs, void* O16, float* m, float* sOut, uint32_t nb,
                          uint32_t group, int mode, int fp8Format, bool fp4, bool mx, void* stream) {
    if (int st = attentionQkvKvCheck(bw, K, Kv, scale, Q16, Kt, Kts, V, Vs, O16, m, sOut, nb, mode, fp8Format, fp4, mx)) return st;
    if (group == 0 || nb % group != 0) return BSMR_ERR_INVALID_ARG;
    if (group > 1 && (K > kQkvGqaMaxK || Kv > kQkvGqaMaxK)) return BSMR_ERR_UNSUPPORTED_K;
    if (group == 1)   // the ungrouped call itself: the same kernel and bits, K and Kv up to 512
        return attentionQkvKvCall(bw, K, Kv, scale, Q16, Kt, Kts, V, Vs, O16, m, sOut, nb, mode, fp8Format, fp4, mx, stream);
    if (nb == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, qkvWorkFloats(bw, Kv, nb))) return st;
    const uint32_t slots = bw->numSlots[0];
    float* partial = bw->work;
    float* sPart = bw->work + (uint64_t)slots * Kv * nb;
    float* mPart = sPart + (uint64_t)slots * nb;
    BSMR_HIP(bsmrLaunchAttnQkvGqaKv(bw->items[0].get(), bw->numItems[0], bw->splits[0].get(), bw->numSplits[0], bw->colIndices,
                                    scale, static_cast<const uint16_t*>(Q16), static_cast<const uint8_t*>(Kt),
                                    static_cast<const uint8_t*>(Kts), static_cast<const uint8_t*>(V),
                                    static_cast<const uint8_t*>(Vs), static_cast<uint16_t*>(O16), m, sOut, partial, sPart, mPart, K,
                                    Kv, bw->M, bw->N, slots, nb, group, mode == BSMR_COMPUTE_BF16, fp4 ? kQkvKvE2M1 : fp8Format, mx,
                                    static_cast<hipStream_t>(stream)));
    return BSMR_OK;
}

}  // namespace

extern "C" {

int bsmr_sparse_attention_qkv_gqa_kv8(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                      const void* Kt8_dev, const void* V8_dev, void* O16_dev, float* m_dev, float* s_dev,
                                      uint32_t num_batches, uint32_t kv_group, int compute_mode, int fp8_format, void* stream) {
    return attentionQkvGqaKvCall(bw, K, Kv, scale, Q16_dev, Kt8_dev, nullptr, V8_dev, nullptr, O16_dev, m_dev, s_dev, num_batches,
                                 kv_group, compute_mode, fp8_format, false, false, stream);
}

int bsmr_sparse_attention_qkv_gqa_kv8_mx(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                         const void* Kt8_dev, const void* Kt_scales_dev, const void* V8_dev,
                                         const void* V_scales_dev, void* O16_dev, float* m_dev, float* s_dev,
                                         uint32_t num_batches, uint32_t kv_group, int compute_mode, int fp8_format,
                                         void* stream) {
    return attentionQkvGqaKvCall(bw, K, Kv, scale, Q16_dev, Kt8_dev, Kt_scales_dev, V8_dev, V_scales_dev, O16_dev, m_dev, s_dev,
                                 num_batches, kv_group, compute_mode, fp8_format, false, true, stream);
}

int bsmr_sparse_attention_qkv_gqa_kv4_mx(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                         const void* Kt4_dev, const void* Kt_scales_dev, const void* V4_dev,
                                         const void* V_scales_dev, void* O16_dev, float* m_dev, float* s_dev,
                                         uint32_t num_batches, uint32_t kv_group, int compute_mode, void* stream) {
    return attentionQkvGqaKvCall(bw, K, Kv, scale, Q16_dev, Kt4_dev, Kt_scales_dev, V4_dev, V_scales_dev, O16_dev, m_dev, s_dev,
                                 num_batches, kv_group, compute_mode, 0, true, true, stream);
}

}  // extern "C"
