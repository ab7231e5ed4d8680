// The row softmax over S's pattern and its backward (include/bsmr_hip.h "Sparse row softmax"), on the SDDMM backward's
// per-pattern handle: its row offsets and its row chunk table (the rows longer than BSMR_BACKWARD_CHUNK) pick the
// kernel of each row (csrc/softmax_kernels.hpp).  No workspace and no allocation: every call is capturable.
// Included at the end of bsmr_capi.hip, after backward_capi.hpp.
#pragma once

#include <cmath>
#include <initializer_list>

#include "softmax_kernels.hpp"

namespace {

// the checks of both calls, before any device call: `arrays` (the call's value arrays) may be NULL only with nnz = 0
// and are whole floats (4-byte aligned)
int checkSoftmaxCall(const bsmr_backward* bw, float scale, std::initializer_list<const void*> arrays, uint32_t nb) {
    if (!bw || !std::isfinite(scale) || nb > 65535u) return BSMR_ERR_INVALID_ARG;
    for (const void* p : arrays)
        if ((bw->nnz && !p) || !aligned4(p)) return BSMR_ERR_INVALID_ARG;
    return BSMR_OK;
}

}  // namespace

extern "C" {

int bsmr_sparse_softmax(bsmr_backward* bw, float scale, const float* X_dev, float* Y_dev, uint32_t num_batches,
                        void* stream) {
    if (int st = checkSoftmaxCall(bw, scale, {X_dev, Y_dev}, num_batches)) return st;
    if (num_batches == 0 || bw->nnz == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((uint32_t)(((uint64_t)bw->M + 3u) / 4u), num_batches);   // 4 short rows per block
    hipLaunchKernelGGL(bsmr::softmaxShort, grid, dim3(256), 0, s, bw->rowOffsets, bw->M, scale, X_dev, Y_dev,
                       (uint64_t)bw->nnz);
    BSMR_HIP(hipGetLastError());
    if (bw->numSplits[0]) {
        hipLaunchKernelGGL(bsmr::softmaxLong, dim3(bw->numSplits[0], num_batches), dim3(256), 0, s, bw->rowOffsets,
                           bw->splits[0], scale, X_dev, Y_dev, (uint64_t)bw->nnz);
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

int bsmr_sparse_softmax_backward(bsmr_backward* bw, float scale, const float* Y_dev, const float* dY_dev, float* dX_dev,
                                 uint32_t num_batches, void* stream) {
    if (int st = checkSoftmaxCall(bw, scale, {Y_dev, dY_dev, dX_dev}, num_batches)) return st;
    if (num_batches == 0 || bw->nnz == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((uint32_t)(((uint64_t)bw->M + 3u) / 4u), num_batches);
    hipLaunchKernelGGL(bsmr::softmaxShortBackward, grid, dim3(256), 0, s, bw->rowOffsets, bw->M, scale, Y_dev, dY_dev,
                       dX_dev, (uint64_t)bw->nnz);
    BSMR_HIP(hipGetLastError());
    if (bw->numSplits[0]) {
        hipLaunchKernelGGL(bsmr::softmaxLongBackward, dim3(bw->numSplits[0], num_batches), dim3(256), 0, s,
                           bw->rowOffsets, bw->splits[0], scale, Y_dev, dY_dev, dX_dev, (uint64_t)bw->nnz);
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

}  // extern "C"
