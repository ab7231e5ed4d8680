// One-pass sparse attention: the translation unit of attnQkv / attnQkvMerge (csrc/attention_qkv_kernels.hpp) and their
// launches.  It is compiled apart from bsmr_capi.hip because it is built without packed fp32 operations (Makefile,
// QKV_FLAGS), which is a property of a whole compilation.
// The kernel headers it shares with bsmr_capi.hip also define nine non-template kernels (batchedTranspose, spmmReduce,
// spmmPermute, the four softmax kernels, attnRowMax, attnValuesBackward).  A second definition of bsmr::attnRowMax
// would clash at link time, so in this unit the namespace of those headers is bsmr_qkv: its copies of the nine kernels
// are distinct symbols.  They are emitted into this unit's code object and never launched.
#define bsmr bsmr_qkv

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bsmr_hip.h"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_kernels.hpp"

namespace {

template <int N>
using Int = std::integral_constant<int, N>;

// fn(NL, VC): the unroll classes of attnQkv for (K, Kv) as compile-time constants
template <typename F>
void withQkvShape(uint32_t K, uint32_t Kv, F&& fn) {
    auto values = [&](auto NL) {
        if (Kv <= 128u) fn(NL, Int<1>{});
        else if (Kv <= 256u) fn(NL, Int<2>{});
        else fn(NL, Int<4>{});
    };
    const uint32_t kc = K / 32u;
    if (kc <= 1u) values(Int<1>{});
    else if (kc <= 2u) values(Int<2>{});
    else if (kc <= 4u) values(Int<4>{});
    else if (kc <= 8u) values(Int<8>{});
    else values(Int<16>{});
}

template <int MODE>
hipError_t launch(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits, uint32_t numSplits,
                  const uint32_t* src, float scale, const uint16_t* Q, const uint16_t* Kt, const uint16_t* V, uint16_t* O,
                  float* m, float* s, float* partial, float* sPart, float* mPart, uint32_t K, uint32_t Kv, uint32_t M,
                  uint32_t N, uint32_t numSlots, uint32_t nb, hipStream_t stream) {
    if (numItems) {
        const dim3 grid((numItems + 3u) / 4u, nb);
        withQkvShape(K, Kv, [&](auto NL, auto VC) {
            hipLaunchKernelGGL((bsmr::attnQkv<MODE, NL(), VC()>), grid, dim3(256), 0, stream, items, numItems, src, scale, Q, Kt,
                               V, O, m, s, partial, sPart, mPart, K, Kv, M, N, numSlots);
        });
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (numSplits) {   // only a handle with split rows launches the merge
        const uint64_t threads = (uint64_t)numSplits * (Kv / 4u);
        const dim3 grid((uint32_t)((threads + 255u) / 256u), nb);
        hipLaunchKernelGGL(bsmr::attnQkvMerge<MODE>, grid, dim3(256), 0, stream, splits, numSplits, partial, sPart, mPart, O, m, s,
                           Kv, M, numSlots);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace

// (items / splits arrive untyped: bsmr_capi.hip's BwItem and this unit's are the same layout under two names)
hipError_t bsmrLaunchAttnQkv(const void* items, uint32_t numItems, const void* splits, uint32_t numSplits, const uint32_t* src,
                             float scale, const uint16_t* Q, const uint16_t* Kt, const uint16_t* V, uint16_t* O, float* m,
                             float* s, float* partial, float* sPart, float* mPart, uint32_t K, uint32_t Kv, uint32_t M,
                             uint32_t N, uint32_t numSlots, uint32_t numBatches, bool bf16, hipStream_t stream) {
    const auto* it = static_cast<const bsmr::BwItem*>(items);
    const auto* sp = static_cast<const bsmr::BwSplit*>(splits);
    return bf16 ? launch<1>(it, numItems, sp, numSplits, src, scale, Q, Kt, V, O, m, s, partial, sPart, mPart, K, Kv, M, N,
                            numSlots, numBatches, stream)
                : launch<0>(it, numItems, sp, numSplits, src, scale, Q, Kt, V, O, m, s, partial, sPart, mPart, K, Kv, M, N,
                            numSlots, numBatches, stream);
}
