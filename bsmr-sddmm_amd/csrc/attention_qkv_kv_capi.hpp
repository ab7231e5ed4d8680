// One-pass sparse attention on a quantised KV cache (include/bsmr_hip.h "One-pass sparse attention on fp8, MXFP8 and MXFP4
// keys and values"): the checks of bsmr_sparse_attention_qkv_16 and of the _x8_mx / _x4_mx calls, the workspace of
// csrc/attention_qkv_capi.hpp (the partials are fp32 whatever the KV format: same layout, same reserve call) and the
// launches of csrc/attention_qkv_kv_kernels.hpp, a translation unit of their own (csrc/attention_qkv_kv.hip).
// Included at the end of bsmr_capi.hip, after fp4_capi.hpp (validFp8, is16).
#pragma once

#include "attention_qkv_launch.hpp"

namespace {

static_assert(kQkvKvE4M3 == BSMR_FP8_E4M3 && kQkvKvE5M2 == BSMR_FP8_E5M2, "an fp8_format is passed on as the KV format");

// fp4: e2m1 codes (fp8Format is then unused), otherwise fp8 codes of the caller's fp8Format; mx: the call carries block
// scales (NULL only with nnz = 0).  The checks of a quantised one-pass call, grouped or not, in the documented order.
int attentionQkvKvCheck(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16, const void* Kt, const void* Kts,
                        const void* V, const void* Vs, void* O16, float* m, float* sOut, uint32_t nb, int mode, int fp8Format,
                        bool fp4, bool mx) {
    if (!bw || !std::isfinite(scale)) return BSMR_ERR_INVALID_ARG;
    if (!qkvDim(K) || !qkvDim(Kv)) return BSMR_ERR_UNSUPPORTED_K;
    if (fp4 ? !is16(mode) : !validFp8(mode, fp8Format)) return BSMR_ERR_INVALID_ARG;
    if (int st = checkAttentionCall(bw, Kv, scale, true, mode, nb, {Q16, Kt, V}, {}, {O16, m, sOut})) return st;
    if ((mx && bw->nnz && (!Kts || !Vs)) || !aligned16(O16) || !aligned4(m) || !aligned4(sOut)) return BSMR_ERR_INVALID_ARG;
    return BSMR_OK;
}

int attentionQkvKvCall(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16, const void* Kt, const void* Kts,
                       const void* V, const void* Vs, void* O16, float* m, float* sOut, uint32_t nb, int mode, int fp8Format,
                       bool fp4, bool mx, void* stream) {
    if (int st = attentionQkvKvCheck(bw, K, Kv, scale, Q16, Kt, Kts, V, Vs, O16, m, sOut, nb, mode, fp8Format, fp4, mx)) return st;
    if (nb == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, qkvWorkFloats(bw, Kv, nb))) return st;
    const uint32_t slots = bw->numSlots[0];
    float* partial = bw->work;
    float* sPart = bw->work + (uint64_t)slots * Kv * nb;
    float* mPart = sPart + (uint64_t)slots * nb;
    BSMR_HIP(bsmrLaunchAttnQkvKv(bw->items[0].get(), bw->numItems[0], bw->splits[0].get(), bw->numSplits[0], bw->colIndices, scale,
                                 static_cast<const uint16_t*>(Q16), static_cast<const uint8_t*>(Kt),
                                 static_cast<const uint8_t*>(Kts), static_cast<const uint8_t*>(V), static_cast<const uint8_t*>(Vs),
                                 static_cast<uint16_t*>(O16), m, sOut, partial, sPart, mPart, K, Kv, bw->M, bw->N, slots, nb,
                                 mode == BSMR_COMPUTE_BF16, fp4 ? kQkvKvE2M1 : fp8Format, mx, static_cast<hipStream_t>(stream)));
    return BSMR_OK;
}

}  // namespace

extern "C" {

int bsmr_sparse_attention_qkv_kv8(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                  const void* Kt8_dev, const void* V8_dev, void* O16_dev, float* m_dev, float* s_dev,
                                  uint32_t num_batches, int compute_mode, int fp8_format, void* stream) {
    return attentionQkvKvCall(bw, K, Kv, scale, Q16_dev, Kt8_dev, nullptr, V8_dev, nullptr, O16_dev, m_dev, s_dev, num_batches,
                              compute_mode, fp8_format, false, false, stream);
}

int bsmr_sparse_attention_qkv_kv8_mx(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                     const void* Kt8_dev, const void* Kt_scales_dev, const void* V8_dev,
                                     const void* V_scales_dev, void* O16_dev, float* m_dev, float* s_dev, uint32_t num_batches,
                                     int compute_mode, int fp8_format, void* stream) {
    return attentionQkvKvCall(bw, K, Kv, scale, Q16_dev, Kt8_dev, Kt_scales_dev, V8_dev, V_scales_dev, O16_dev, m_dev, s_dev,
                              num_batches, compute_mode, fp8_format, false, true, stream);
}

int bsmr_sparse_attention_qkv_kv4_mx(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                     const void* Kt4_dev, const void* Kt_scales_dev, const void* V4_dev,
                                     const void* V_scales_dev, void* O16_dev, float* m_dev, float* s_dev, uint32_t num_batches,
                                     int compute_mode, void* stream) {
    return attentionQkvKvCall(bw, K, Kv, scale, Q16_dev, Kt4_dev, Kt_scales_dev, V4_dev, V_scales_dev, O16_dev, m_dev, s_dev,
                              num_batches, compute_mode, 0, true, true, stream);
}

}  // extern "C"
