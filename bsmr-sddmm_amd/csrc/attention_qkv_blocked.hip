// One-pass sparse attention over the RPHM's blocks: the translation unit of attnQkvBlocks / attnQkvBlkMerge
// (csrc/attention_qkv_blocked_kernels.hpp) and their launches.  Built like csrc/attention_qkv.hip - without packed fp32
// operations (Makefile, QKV_FLAGS) and with the namespace of the shared kernel headers renamed, here to bsmr_qkvb, so that
// its copies of their non-template kernels (those of attention_qkv.hip and spmmBlocks, spmmBlocksSeg, spmmBlocksFinish)
// are distinct symbols.  They are emitted into this unit's code object and never launched.
#define bsmr bsmr_qkvb

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bsmr_hip.h"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_blocked_kernels.hpp"

namespace {

template <int N>
using Int = std::integral_constant<int, N>;

// fn(NL, G): the unroll class of the score loop for K and the 64-feature groups a wave carries for Kv
template <typename F>
void withBlkShape(uint32_t K, uint32_t Kv, F&& fn) {
    auto groups = [&](auto NL) {
        if (Kv <= 64u) fn(NL, Int<1>{});
        else fn(NL, Int<2>{});
    };
    const uint32_t kc = K / 32u;
    if (kc <= 1u) groups(Int<1>{});
    else if (kc <= 2u) groups(Int<2>{});
    else if (kc <= 4u) groups(Int<4>{});
    else if (kc <= 8u) groups(Int<8>{});
    else groups(Int<16>{});
}

template <int MODE>
hipError_t launch(const void* units, uint32_t numUnits, bool segments, const uint32_t* panelRows, const bsmr::u32x4* cells,
                  const bsmr::u32x4* cols, const float* zeros, const BsmrAttnBlkRow* rows, uint32_t numRows, float scale,
                  const uint16_t* Q, const uint16_t* Kt, const uint16_t* V, uint16_t* O, float* m, float* s,
                  const float* partial, const float* sPart, const float* mPart, uint32_t numSlots, float* bPart, float* bs,
                  float* bm, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t nb, hipStream_t stream) {
    if (!numUnits) return hipSuccess;   // (no panel has blocks: no row is merged here either)
    withBlkShape(K, Kv, [&](auto NL, auto G) {
        const uint32_t slabs = (Kv + 64u * G() - 1u) / (64u * G());
        const dim3 grid((uint32_t)(((uint64_t)numUnits * slabs + 3u) / 4u), nb);
        hipLaunchKernelGGL((bsmr::attnQkvBlocks<MODE, NL(), G()>), grid, dim3(256), 0, stream, units, numUnits,
                           segments ? 1u : 0u, slabs, panelRows, cells, cols, zeros, scale, Q, Kt, V, bPart, bs, bm, K, Kv, M, N);
    });
    if (hipError_t e = hipGetLastError()) return e;
    const uint64_t threads = (uint64_t)numRows * (Kv / 4u);
    const dim3 grid((uint32_t)((threads + 255u) / 256u), nb);
    hipLaunchKernelGGL(bsmr::attnQkvBlkMerge<MODE>, grid, dim3(256), 0, stream, rows, numRows, partial, sPart, mPart, numSlots,
                       bPart, bs, bm, numUnits, O, m, s, Kv, M);
    return hipGetLastError();
}

}  // namespace

hipError_t bsmrLaunchAttnQkvBlocks(const void* units, uint32_t numUnits, bool segments, const uint32_t* panelRows,
                                   const void* cells, const void* cols, const float* zeros, const BsmrAttnBlkRow* rows,
                                   uint32_t numRows, float scale, const uint16_t* Q, const uint16_t* Kt, const uint16_t* V,
                                   uint16_t* O, float* m, float* s, const float* partial, const float* sPart,
                                   const float* mPart, uint32_t numSlots, float* bPart, float* bs, float* bm, uint32_t K,
                                   uint32_t Kv, uint32_t M, uint32_t N, uint32_t numBatches, bool bf16, hipStream_t stream) {
    const auto* ce = static_cast<const bsmr::u32x4*>(cells);
    const auto* co = static_cast<const bsmr::u32x4*>(cols);
    return bf16 ? launch<1>(units, numUnits, segments, panelRows, ce, co, zeros, rows, numRows, scale, Q, Kt, V, O, m, s, partial,
                            sPart, mPart, numSlots, bPart, bs, bm, K, Kv, M, N, numBatches, stream)
                : launch<0>(units, numUnits, segments, panelRows, ce, co, zeros, rows, numRows, scale, Q, Kt, V, O, m, s, partial,
                            sPart, mPart, numSlots, bPart, bs, bm, K, Kv, M, N, numBatches, stream);
}
