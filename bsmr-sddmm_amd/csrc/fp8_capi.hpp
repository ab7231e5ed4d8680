// fp8 keys and values (include/bsmr_hip.h "fp8 keys and values"): the column-side operand of the SDDMM, the SpMM and the
// fused attention as OCP fp8 bytes.  bsmr_sddmm_b8 widens B into the plan's 16-bit workspace and runs bsmr_sddmm_16's
// body on it; bsmr_spmm_x8 and bsmr_sparse_attention_x8 gather the bytes themselves (csrc/fp8_kernels.hpp) on the lists,
// chunk table and workspace of their 16-bit forms.  The _mx entry points ("MX block scales") are the same
// bodies with a scales pointer: the pass and the gathers multiply each widened element by its block's E8M0 scale.
// Included at the end of bsmr_capi.hip, after attention_capi.hpp.
#pragma once

#include "fp8_kernels.hpp"

namespace {

bool validFp8(int mode, int fmt) {
    return (mode == BSMR_COMPUTE_F16 || mode == BSMR_COMPUTE_BF16) && (fmt == BSMR_FP8_E4M3 || fmt == BSMR_FP8_E5M2);
}

// the call `LAUNCH(MODE, FMT)` for the run-time (mode, fmt)
#define BSMR_FP8_DISPATCH(LAUNCH)                                                                                         \
    do {                                                                                                                  \
        if (mode == BSMR_COMPUTE_F16) {                                                                                   \
            if (fmt == BSMR_FP8_E4M3) { LAUNCH(0, 0); } else { LAUNCH(0, 1); }                                            \
        } else {                                                                                                          \
            if (fmt == BSMR_FP8_E4M3) { LAUNCH(1, 0); } else { LAUNCH(1, 1); }                                            \
        }                                                                                                                 \
    } while (0)

// scales NULL: out16 = widen(in8); otherwise out16 = narrow(dq(in8, scales)), count a multiple of 32
int launchWidenFp8(const void* in8, const void* scales, void* out16, uint64_t count, int mode, int fmt, hipStream_t s) {
    if (count == 0) return BSMR_OK;
    // one thread per 16 elements, grid-stride beyond 4096 blocks; the first block also takes the last count % 16 elements
    const dim3 grid((uint32_t)std::min<uint64_t>(std::max<uint64_t>((count / 16u + 255u) / 256u, 1u), 256u * 16u));
#define BSMR_WIDEN8(MODE, FMT)                                                                                            \
    hipLaunchKernelGGL((bsmr::widenFp8<MODE, FMT>), grid, dim3(256), 0, s, static_cast<const uint8_t*>(in8),              \
                       static_cast<uint16_t*>(out16), count)
#define BSMR_WIDEN8MX(MODE, FMT)                                                                                          \
    hipLaunchKernelGGL((bsmr::widenFp8Mx<MODE, FMT>), grid, dim3(256), 0, s, static_cast<const uint8_t*>(in8),            \
                       static_cast<const uint8_t*>(scales), static_cast<uint16_t*>(out16), count)
    if (scales) BSMR_FP8_DISPATCH(BSMR_WIDEN8MX);
    else BSMR_FP8_DISPATCH(BSMR_WIDEN8);
#undef BSMR_WIDEN8MX
#undef BSMR_WIDEN8
    BSMR_HIP(hipGetLastError());
    return BSMR_OK;
}

constexpr const uint8_t* kNoScales = nullptr;   // the E of a gather without MX: never read

// Source bytes per lane of the fp8 gathers for slice width W (csrc/fp8_kernels.hpp "Lane layout")
constexpr uint32_t lanes8For(uint32_t W) { return W >= 128u ? 16u : 8u; }

// Y16 = round(S_v widen(X8)) (dir 0) or round(S_v^T widen(X8)) (dir 1); the workspace is already large enough.
// E8 non-NULL: the MX block scales of X8 ([b][rows][K / 32] bytes), the gather runs on dq(X8, E8)
int runSpmm8(bsmr_backward* bw, uint32_t K, int dir, const float* v, const uint8_t* X8, const uint8_t* E8, uint16_t* Y16,
             uint32_t nb, int mode, int fmt, hipStream_t s) {
    const uint32_t rowsX = dir ? bw->M : bw->N, rowsY = dir ? bw->N : bw->M;
    const uint64_t nnz = bw->nnz, xB = (uint64_t)rowsX * K, yB = (uint64_t)rowsY * K, pB = (uint64_t)bw->numSlots[dir] * K;
    const uint64_t eB = xB / 32u;
    float* partial = bw->work;
    GatherLists L;
    if (int st = spmmLists(bw, K, dir, v, nb, s, L)) return st;
    const uint32_t W = K % 256u == 0 ? 256u : K % 128u == 0 ? 128u : K % 64u == 0 ? 64u : 32u;
    const uint32_t slices = K / W;
    const uint64_t units = (uint64_t)L.numItems * slices;
    const uint64_t unitsPerBlock = 4u * (64u / (W / lanes8For(W)));
    const dim3 grid((uint32_t)((units + unitsPerBlock - 1) / unitsPerBlock), nb);
    if (units) {
#define BSMR_SPMM8(MODE, FMT)                                                                                             \
    if (E8 && L.map)                                                                                                      \
        hipLaunchKernelGGL((bsmr::spmmGather8<WW, lanes8For(WW), true, MODE, FMT, true>), grid, dim3(256), 0, s, L.items, \
                           L.numItems, slices, L.src, L.map, v, X8, Y16, partial, K, nnz, xB, yB, pB, E8, eB);            \
    else if (E8)                                                                                                          \
        hipLaunchKernelGGL((bsmr::spmmGather8<WW, lanes8For(WW), false, MODE, FMT, true>), grid, dim3(256), 0, s,         \
                           L.items, L.numItems, slices, L.src, L.map, v, X8, Y16, partial, K, nnz, xB, yB, pB, E8, eB);   \
    else if (L.map)                                                                                                       \
        hipLaunchKernelGGL((bsmr::spmmGather8<WW, lanes8For(WW), true, MODE, FMT>), grid, dim3(256), 0, s, L.items,       \
                           L.numItems, slices, L.src, L.map, v, X8, Y16, partial, K, nnz, xB, yB, pB, kNoScales, 0);      \
    else                                                                                                                  \
        hipLaunchKernelGGL((bsmr::spmmGather8<WW, lanes8For(WW), false, MODE, FMT>), grid, dim3(256), 0, s, L.items,      \
                           L.numItems, slices, L.src, L.map, v, X8, Y16, partial, K, nnz, xB, yB, pB, kNoScales, 0)
        switch (W) {
        case 256: { constexpr uint32_t WW = 256; BSMR_FP8_DISPATCH(BSMR_SPMM8); break; }
        case 128: { constexpr uint32_t WW = 128; BSMR_FP8_DISPATCH(BSMR_SPMM8); break; }
        case 64: { constexpr uint32_t WW = 64; BSMR_FP8_DISPATCH(BSMR_SPMM8); break; }
        default: { constexpr uint32_t WW = 32; BSMR_FP8_DISPATCH(BSMR_SPMM8); break; }
        }
#undef BSMR_SPMM8
        BSMR_HIP(hipGetLastError());
    }
    if (L.numSplits) {   // the reduction of the 16-bit forms, unchanged
        const uint64_t threads = (uint64_t)L.numSplits * (K / 4u);
        const dim3 rgrid((uint32_t)((threads + 255u) / 256u), nb);
        if (mode == BSMR_COMPUTE_F16)
            hipLaunchKernelGGL(bsmr::spmmReduce16<0>, rgrid, dim3(256), 0, s, L.splits, L.numSplits, partial, Y16, K, yB, pB);
        else
            hipLaunchKernelGGL(bsmr::spmmReduce16<1>, rgrid, dim3(256), 0, s, L.splits, L.numSplits, partial, Y16, K, yB, pB);
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

// runAttention with fp8 rows of V and O in mode's 16-bit format; E8 non-NULL: on dq(V8, E8), as in runSpmm8
int runAttention8(bsmr_backward* bw, uint32_t Kv, float scale, const float* P, const uint8_t* V8, const uint8_t* E8,
                  uint16_t* O16, float* m, float* sOut, uint32_t nb, int mode, int fmt, hipStream_t s) {
    if (int st = growWork(bw, attnWorkFloats(bw, Kv, nb))) return st;
    float* partial = bw->work;
    float* sPart = bw->work + attnSumsOffset(bw, Kv, nb);
    const uint32_t M = bw->M, slots = bw->numSlots[0];
    const uint64_t nnz = bw->nnz, xB = (uint64_t)bw->N * Kv, eB = xB / 32u;
    if (int st = launchAttnRowMax(bw, scale, P, m, nb, s)) return st;
    const uint32_t W = Kv % 256u == 0 ? 256u : Kv % 128u == 0 ? 128u : Kv % 64u == 0 ? 64u : 32u;
    const uint32_t slices = Kv / W;
    const uint64_t units = (uint64_t)bw->numItems[0] * slices;
    const uint64_t unitsPerBlock = 4u * (64u / (W / lanes8For(W)));
    const dim3 grid((uint32_t)((units + unitsPerBlock - 1) / unitsPerBlock), nb);
    if (units) {
#define BSMR_ATTN8(MODE, FMT)                                                                                             \
    if (E8)                                                                                                               \
        hipLaunchKernelGGL((bsmr::attnGather8<WW, lanes8For(WW), MODE, FMT, true>), grid, dim3(256), 0, s, bw->items[0],  \
                           bw->numItems[0], slices, bw->colIndices, scale, P, m, V8, O16, sOut, partial, sPart, Kv, M,    \
                           slots, nnz, xB, E8, eB);                                                                       \
    else                                                                                                                  \
    hipLaunchKernelGGL((bsmr::attnGather8<WW, lanes8For(WW), MODE, FMT>), grid, dim3(256), 0, s, bw->items[0],            \
                       bw->numItems[0], slices, bw->colIndices, scale, P, m, V8, O16, sOut, partial, sPart, Kv, M, slots, \
                       nnz, xB, kNoScales, 0)
        switch (W) {
        case 256: { constexpr uint32_t WW = 256; BSMR_FP8_DISPATCH(BSMR_ATTN8); break; }
        case 128: { constexpr uint32_t WW = 128; BSMR_FP8_DISPATCH(BSMR_ATTN8); break; }
        case 64: { constexpr uint32_t WW = 64; BSMR_FP8_DISPATCH(BSMR_ATTN8); break; }
        default: { constexpr uint32_t WW = 32; BSMR_FP8_DISPATCH(BSMR_ATTN8); break; }
        }
#undef BSMR_ATTN8
        BSMR_HIP(hipGetLastError());
    }
    return launchAttnReduce(bw, Kv, partial, sPart, m, O16, sOut, nb, mode, s);
}

#undef BSMR_FP8_DISPATCH

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
    if (int st = checkBackwardCall(bw, K, num_batches)) return st;
    if (!validFp8(compute_mode, fp8_format)) return BSMR_ERR_INVALID_ARG;
    if (transpose != 0 && transpose != 1) return BSMR_ERR_INVALID_ARG;
    const bool reads = bw->nnz != 0;   // as bsmr_spmm_16: nnz = 0 reads neither v nor X, Y is still written with zeros
    if ((reads && (!v_dev || !X8_dev || (mx && !scales))) || !Y16_dev || !aligned4(v_dev) || !aligned16(X8_dev) ||
        !aligned16(Y16_dev))
        return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, workFloatsFor(bw, K, num_batches, bw->permuteV && transpose))) return st;
    return runSpmm8(bw, K, transpose, v_dev, static_cast<const uint8_t*>(X8_dev), static_cast<const uint8_t*>(scales),
                    static_cast<uint16_t*>(Y16_dev), num_batches, compute_mode, fp8_format, static_cast<hipStream_t>(stream));
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
    return runAttention8(bw, Kv, scale, P_dev, static_cast<const uint8_t*>(V8_dev), static_cast<const uint8_t*>(scales),
                         static_cast<uint16_t*>(O16_dev), m_dev, s_dev, num_batches, compute_mode, fp8_format,
                         static_cast<hipStream_t>(stream));
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
