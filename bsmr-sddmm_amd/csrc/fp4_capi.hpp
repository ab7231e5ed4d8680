// MXFP4 keys and values (include/bsmr_hip.h "MXFP4 keys and values"): the column-side operand of the SDDMM, the SpMM and
// the fused attention as OCP e2m1 codes, two per byte, under E8M0 block scales.  The entry points are the _mx ones of
// csrc/fp8_capi.hpp without an fp8_format, and their bodies follow those line by line: bsmr_sddmm_b4_mx dequantises B into
// the plan's 16-bit workspace and runs bsmr_sddmm_16's body on it; bsmr_spmm_x4_mx and bsmr_sparse_attention_x4_mx gather
// the nibbles themselves (csrc/fp4_kernels.hpp) on the lists, chunk table and workspace of their 16-bit forms.  The scales
// are mandatory: there is no unscaled fp4 call.
// Included at the end of bsmr_capi.hip, after fp8_capi.hpp.
#pragma once

#include "fp4_kernels.hpp"

namespace {

// out16 = narrow(dq(in4, scales)), count (elements) a multiple of 32
int launchWidenFp4(const void* in4, const void* scales, void* out16, uint64_t count, int mode, hipStream_t s) {
    if (count == 0) return BSMR_OK;
    // one thread per block of 32 elements, grid-stride beyond 2048 blocks
    const dim3 grid((uint32_t)std::min<uint64_t>((count / 32u + 255u) / 256u, 256u * 8u));
    withMode(mode, [&](auto MODE) {
        hipLaunchKernelGGL(bsmr::widenFp4Mx<MODE()>, grid, dim3(256), 0, s, static_cast<const uint8_t*>(in4),
                           static_cast<const uint8_t*>(scales), static_cast<uint16_t*>(out16), count);
    });
    BSMR_HIP(hipGetLastError());
    return BSMR_OK;
}

}  // namespace

extern "C" {

int bsmr_widen_fp4_mx(const void* in4_dev, const void* scales_dev, void* out16_dev, uint64_t count, int compute_mode,
                      void* stream) {
    if (!is16(compute_mode) || (count & 31u)) return BSMR_ERR_INVALID_ARG;
    if (count == 0) return BSMR_OK;
    if (!in4_dev || !out16_dev || !scales_dev || !aligned16(in4_dev) || !aligned16(out16_dev)) return BSMR_ERR_INVALID_ARG;
    return launchWidenFp4(in4_dev, scales_dev, out16_dev, count, compute_mode, static_cast<hipStream_t>(stream));
}

int bsmr_sddmm_b4_mx(bsmr_plan* plan, uint32_t K, const void* A16_dev, const void* B4_dev, const void* B_scales_dev,
                     float* P_dev, uint32_t num_batches, int compute_mode, void* stream) {
    if (!plan) return BSMR_ERR_INVALID_ARG;
    if (K == 0 || (K & 31u)) return BSMR_ERR_UNSUPPORTED_K;
    if (!is16(compute_mode)) return BSMR_ERR_INVALID_ARG;
    plan = servedFor(plan, K, compute_mode);
    const bool reads = plan->nnz != 0;   // nnz = 0: nothing is read or written
    if ((reads && (!A16_dev || !B4_dev || !P_dev || !B_scales_dev)) || !aligned16(A16_dev) || !aligned16(B4_dev) ||
        !aligned4(P_dev))
        return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0 || !reads) return BSMR_OK;
    if (num_batches > 65535u || (uint64_t)K * num_batches > 0xFFFFFFFFull) return BSMR_ERR_INVALID_ARG;
    BSMR_HIP(hipSetDevice(plan->device));
    // the batches are contiguous: one workspace and one dequantising pass cover all of them, as in bsmr_sddmm_b8_mx
    if (int st = reserve(plan, K * num_batches)) return st;
    if (int st = launchWidenFp4(B4_dev, B_scales_dev, plan->B16.get(), (uint64_t)plan->N * K * num_batches, compute_mode,
                                static_cast<hipStream_t>(stream)))
        return st;
    return runSddmm16(plan, K, A16_dev, plan->B16.get(), P_dev, num_batches, compute_mode, stream);
}

int bsmr_spmm_x4_mx(bsmr_backward* bw, uint32_t K, int transpose, const float* v_dev, const void* X4_dev,
                    const void* X_scales_dev, void* Y16_dev, uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkSpmmCall(bw, K, is16(compute_mode), transpose, num_batches, v_dev, X4_dev, Y16_dev, X_scales_dev, true))
        return st;
    if (num_batches == 0) return BSMR_OK;
    // the fp4 case of bsmr_spmm_16's gather: its lists, chunk table, workspace and reduce
    return spmmCall(bw, K, transpose, v_dev, X4_dev, Y16_dev, num_batches, stream,
                    {compute_mode, true, -1, static_cast<const uint8_t*>(X_scales_dev), true});
}

int bsmr_sparse_attention_x4_mx(bsmr_backward* bw, uint32_t Kv, float scale, const float* P_dev, const void* V4_dev,
                                const void* V_scales_dev, void* O16_dev, float* m_dev, float* s_dev, uint32_t num_batches,
                                int compute_mode, void* stream) {
    if (int st = checkAttentionCall(bw, Kv, scale, true, compute_mode, num_batches, {V4_dev}, {P_dev}, {O16_dev, m_dev, s_dev}))
        return st;
    if ((bw->nnz && !V_scales_dev) || !aligned16(O16_dev) || !aligned4(m_dev) || !aligned4(s_dev)) return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    // with nnz = 0 there is no gather item: neither V4 nor the scales are read, the outputs are still written
    return runAttention(bw, Kv, scale, P_dev, V4_dev, O16_dev, m_dev, s_dev, num_batches, static_cast<hipStream_t>(stream),
                        {compute_mode, true, -1, static_cast<const uint8_t*>(V_scales_dev), true});
}

}  // extern "C"
