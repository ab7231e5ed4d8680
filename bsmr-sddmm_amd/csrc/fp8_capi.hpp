// fp8 keys and values (include/bsmr_hip.h "fp8 keys and values"): the column-side operand of the SDDMM, the SpMM and the
// fused attention as OCP fp8 bytes.  bsmr_sddmm_b8 widens B into the plan's 16-bit workspace and runs bsmr_sddmm_16's
// body on it; bsmr_spmm_x8 and bsmr_sparse_attention_x8 gather the bytes themselves (csrc/fp8_kernels.hpp) on the lists,
// chunk table and workspace of their 16-bit forms.  The _mx entry points ("MX block scales") are the same
// bodies with a scales pointer: the pass and the gathers multiply each widened element by its block's E8M0 scale.
// Included at the end of bsmr_capi.hip, after attention_capi.hpp.
#pragma once

#include "fp8_kernels.hpp"

namespace {

bool validFp8(int mode, int fmt) { return is16(mode) && (fmt == BSMR_FP8_E4M3 || fmt == BSMR_FP8_E5M2); }

// scales NULL: out16 = widen(in8); otherwise out16 = narrow(dq(in8, scales)), count a multiple of 32
int launchWidenFp8(const void* in8, const void* scales, void* out16, uint64_t count, int mode, int fmt, hipStream_t s) {
    if (count == 0) return BSMR_OK;
    // one thread per 16 elements, grid-stride beyond 4096 blocks; the first block also takes the last count % 16 elements
    const dim3 grid((uint32_t)std::min<uint64_t>(std::max<uint64_t>((count / 16u + 255u) / 256u, 1u), 256u * 16u));
    const uint8_t* in = static_cast<const uint8_t*>(in8);
    uint16_t* out = static_cast<uint16_t*>(out16);
    withMode(mode, [&](auto MODE) {
        withFp8(fmt, [&](auto FMT) {
            if (scales)
                hipLaunchKernelGGL((bsmr::widenFp8Mx<MODE(), FMT()>), grid, dim3(256), 0, s, in, static_cast<const uint8_t*>(scales), out,
                                   count);
            else
                hipLaunchKernelGGL((bsmr::widenFp8<MODE(), FMT()>), grid, dim3(256), 0, s, in, out, count);
        });
    });
    BSMR_HIP(hipGetLastError());
    return BSMR_OK;
}

// The bodies of the entry points.  mx: the call carries MX block scales, checked with the other pointers (NULL only where
// nothing is read, any alignment: byte loads); without mx `scales` is NULL and the unscaled kernels run.
int widenFp8Call(const void* in8, const void* scales, bool mx, void* out16, uint64_t count, int mode, int fmt, void* stream) {
    if (!validFp8(mode, fmt)) return BSMR_ERR_INVALID_ARG;
    if (mx && (count & 31u)) return BSMR_ERR_INVALID_ARG;
    if (count == 0) return BSMR_OK;
    if (!in8 || !out16 || (mx && !scales) || !aligned16(in8) || !aligned16(out16)) return BSMR_ERR_INVALID_ARG;
    return launchWidenFp8(in8, scales, out16, count, mode, fmt, static_cast<hipStream_t>(stream));
}

int sddmmB8Call(bsmr_plan* plan, uint32_t K, const void* A16_dev, const void* B8_dev, const void* scales, bool mx, float* P_dev,
                uint32_t num_batches, int compute_mode, int fp8_format, void* stream) {
    if (!plan) return BSMR_ERR_INVALID_ARG;
    if (K == 0 || (K & 31u)) return BSMR_ERR_UNSUPPORTED_K;
    if (!validFp8(compute_mode, fp8_format)) return BSMR_ERR_INVALID_ARG;
    plan = servedFor(plan, K, compute_mode);
    const bool reads = plan->nnz != 0;   // nnz = 0: nothing is read or written
    if ((reads && (!A16_dev || !B8_dev || !P_dev || (mx && !scales))) || !aligned16(A16_dev) || !aligned16(B8_dev) ||
        !aligned4(P_dev))
        return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0 || !reads) return BSMR_OK;
    if (num_batches > 65535u || (uint64_t)K * num_batches > 0xFFFFFFFFull) return BSMR_ERR_INVALID_ARG;
    BSMR_HIP(hipSetDevice(plan->device));
    // the batches are contiguous: one workspace and one widening pass cover all of them, as in bsmr_sddmm_batch
    if (int st = reserve(plan, K * num_batches)) return st;
    if (int st = launchWidenFp8(B8_dev, scales, plan->B16.get(), (uint64_t)plan->N * K * num_batches, compute_mode, fp8_format,
                                static_cast<hipStream_t>(stream)))
        return st;
    return runSddmm16(plan, K, A16_dev, plan->B16.get(), P_dev, num_batches, compute_mode, stream);
}

int spmmX8Call(bsmr_backward* bw, uint32_t K, int transpose, const float* v_dev, const void* X8_dev, const void* scales, bool mx,
               void* Y16_dev, uint32_t num_batches, int compute_mode, int fp8_format, void* stream) {
    if (int st = checkSpmmCall(bw, K, validFp8(compute_mode, fp8_format), transpose, num_batches, v_dev, X8_dev, Y16_dev, scales, mx))
        return st;
    if (num_batches == 0) return BSMR_OK;
    // the fp8 case of bsmr_spmm_16's gather: its lists, chunk table, workspace and reduce
    return spmmCall(bw, K, transpose, v_dev, X8_dev, Y16_dev, num_batches, stream,
                    {compute_mode, true, fp8_format, static_cast<const uint8_t*>(scales)});
}

int attentionX8Call(bsmr_backward* bw, uint32_t Kv, float scale, const float* P_dev, const void* V8_dev, const void* scales,
                    bool mx, void* O16_dev, float* m_dev, float* s_dev, uint32_t num_batches, int compute_mode, int fp8_format,
                    void* stream) {
    if (int st = checkAttentionCall(bw, Kv, scale, true, compute_mode, num_batches, {V8_dev}, {P_dev}, {O16_dev, m_dev, s_dev}))
        return st;
    if (!validFp8(compute_mode, fp8_format)) return BSMR_ERR_INVALID_ARG;
    if ((mx && bw->nnz && !scales) || !aligned16(O16_dev) || !aligned4(m_dev) || !aligned4(s_dev)) return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    // with nnz = 0 no gather item reads V8 or the scales: a NULL scales pointer then only selects the unscaled kernel
    return runAttention(bw, Kv, scale, P_dev, V8_dev, O16_dev, m_dev, s_dev, num_batches, static_cast<hipStream_t>(stream),
                        {compute_mode, true, fp8_format, static_cast<const uint8_t*>(scales)});
}

}  // namespace

extern "C" {

int bsmr_widen_fp8(const void* in8_dev, void* out16_dev, uint64_t count, int compute_mode, int fp8_format, void* stream) {
    return widenFp8Call(in8_dev, nullptr, false, out16_dev, count, compute_mode, fp8_format, stream);
}

int bsmr_widen_fp8_mx(const void* in8_dev, const void* scales_dev, void* out16_dev, uint64_t count, int compute_mode,
                      int fp8_format, void* stream) {
    return widenFp8Call(in8_dev, scales_dev, true, out16_dev, count, compute_mode, fp8_format, stream);
}

int bsmr_sddmm_b8(bsmr_plan* plan, uint32_t K, const void* A16_dev, const void* B8_dev, float* P_dev, uint32_t num_batches,
                  int compute_mode, int fp8_format, void* stream) {
    return sddmmB8Call(plan, K, A16_dev, B8_dev, nullptr, false, P_dev, num_batches, compute_mode, fp8_format, stream);
}

int bsmr_sddmm_b8_mx(bsmr_plan* plan, uint32_t K, const void* A16_dev, const void* B8_dev, const void* B_scales_dev,
                     float* P_dev, uint32_t num_batches, int compute_mode, int fp8_format, void* stream) {
    return sddmmB8Call(plan, K, A16_dev, B8_dev, B_scales_dev, true, P_dev, num_batches, compute_mode, fp8_format, stream);
}

int bsmr_spmm_x8(bsmr_backward* bw, uint32_t K, int transpose, const float* v_dev, const void* X8_dev, void* Y16_dev,
                 uint32_t num_batches, int compute_mode, int fp8_format, void* stream) {
    return spmmX8Call(bw, K, transpose, v_dev, X8_dev, nullptr, false, Y16_dev, num_batches, compute_mode, fp8_format, stream);
}

int bsmr_spmm_x8_mx(bsmr_backward* bw, uint32_t K, int transpose, const float* v_dev, const void* X8_dev,
                    const void* X_scales_dev, void* Y16_dev, uint32_t num_batches, int compute_mode, int fp8_format,
                    void* stream) {
    return spmmX8Call(bw, K, transpose, v_dev, X8_dev, X_scales_dev, true, Y16_dev, num_batches, compute_mode, fp8_format,
                      stream);
}

int bsmr_sparse_attention_x8(bsmr_backward* bw, uint32_t Kv, float scale, const float* P_dev, const void* V8_dev, void* O16_dev,
                             float* m_dev, float* s_dev, uint32_t num_batches, int compute_mode, int fp8_format, void* stream) {
    return attentionX8Call(bw, Kv, scale, P_dev, V8_dev, nullptr, false, O16_dev, m_dev, s_dev, num_batches, compute_mode,
                           fp8_format, stream);
}

int bsmr_sparse_attention_x8_mx(bsmr_backward* bw, uint32_t Kv, float scale, const float* P_dev, const void* V8_dev,
                                const void* V_scales_dev, void* O16_dev, float* m_dev, float* s_dev, uint32_t num_batches,
                                int compute_mode, int fp8_format, void* stream) {
    return attentionX8Call(bw, Kv, scale, P_dev, V8_dev, V_scales_dev, true, O16_dev, m_dev, s_dev, num_batches, compute_mode,
                           fp8_format, stream);
}

}  // extern "C"
