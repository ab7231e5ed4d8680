// One-pass sparse attention over the RPHM's blocks: the translation unit of attnQkvBlocks / attnQkvBlkMerge
// (csrc/attention_qkv_blocked_kernels.hpp) and their launches.  Built like csrc/attention_qkv.hip: without packed fp32
// operations (Makefile, QKV_FLAGS), on helper headers that define no kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsmr_hip.h"
#include "attention_qkv_dispatch.hpp"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_blocked_kernels.hpp"

namespace {

struct QkvBlkCall {
    const void* units;
    uint32_t numUnits;
    bool segments;
    const uint32_t* panelRows;
    const bsmr::u32x4 *cells, *cols;
    const float* zeros;
    const BsmrAttnBlkRow* rows;
    uint32_t numRows;
    float scale;
    const uint16_t *Q, *Kt, *V;
    uint16_t* O;
    float *m, *s;
    const float *partial, *sPart, *mPart;
    uint32_t numSlots;
    float *bPart, *bs, *bm;
    uint32_t K, Kv, M, N, nb;
    hipStream_t stream;
};

// fn(NL, G): the unroll class of the score loop for K and the 64-feature groups a wave carries for Kv
template <typename F>
void withBlkShape(uint32_t K, uint32_t Kv, F&& fn) {
    withPieces<16>(K / 32u, [&](auto NL) {
        if (Kv <= 64u) fn(NL, Int<1>{});
        else fn(NL, Int<2>{});
    });
}

template <int MODE>
hipError_t launch(const QkvBlkCall& c) {
    if (!c.numUnits) return hipSuccess;   // (no panel has blocks: no row is merged here either)
    withBlkShape(c.K, c.Kv, [&](auto NL, auto G) {
        const uint32_t slabs = (c.Kv + 64u * G() - 1u) / (64u * G());
        const dim3 grid((uint32_t)(((uint64_t)c.numUnits * slabs + 3u) / 4u), c.nb);
        hipLaunchKernelGGL((bsmr::attnQkvBlocks<MODE, NL(), G()>), grid, dim3(256), 0, c.stream, c.units, c.numUnits,
                           c.segments ? 1u : 0u, slabs, c.panelRows, c.cells, c.cols, c.zeros, c.scale, c.Q, c.Kt, c.V, c.bPart,
                           c.bs, c.bm, c.K, c.Kv, c.M, c.N);
    });
    if (hipError_t e = hipGetLastError()) return e;
    const uint64_t threads = (uint64_t)c.numRows * (c.Kv / 4u);
    const dim3 grid((uint32_t)((threads + 255u) / 256u), c.nb);
    hipLaunchKernelGGL(bsmr::attnQkvBlkMerge<MODE>, grid, dim3(256), 0, c.stream, c.rows, c.numRows, c.partial, c.sPart, c.mPart,
                       c.numSlots, c.bPart, c.bs, c.bm, c.numUnits, c.O, c.m, c.s, c.Kv, c.M);
    return hipGetLastError();
}

}  // namespace

hipError_t bsmrLaunchAttnQkvBlocks(const void* units, uint32_t numUnits, bool segments, const uint32_t* panelRows,
                                   const bsmr::u32x4* cells, const bsmr::u32x4* cols, const float* zeros,
                                   const BsmrAttnBlkRow* rows, uint32_t numRows, float scale, const uint16_t* Q,
                                   const uint16_t* Kt, const uint16_t* V, uint16_t* O, float* m, float* s, const float* partial,
                                   const float* sPart, const float* mPart, uint32_t numSlots, float* bPart, float* bs, float* bm,
                                   uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numBatches, bool bf16,
                                   hipStream_t stream) {
    const QkvBlkCall c{units, numUnits, segments, panelRows, cells, cols, zeros, rows, numRows, scale, Q, Kt, V, O, m, s, partial,
                       sPart, mPart, numSlots, bPart, bs, bm, K, Kv, M, N, numBatches, stream};
    return bf16 ? launch<1>(c) : launch<0>(c);
}
