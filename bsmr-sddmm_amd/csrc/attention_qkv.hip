// One-pass sparse attention: the translation unit of attnQkv / attnQkvMerge (csrc/attention_qkv_kernels.hpp) and their
// launches.  It is compiled apart from bsmr_capi.hip because it is built without packed fp32 operations (Makefile,
// QKV_FLAGS), which is a property of a whole compilation.  It shares device helpers with bsmr_capi.hip
// through headers that define no kernel, so its code object holds the kernels it launches and no other.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsmr_hip.h"
#include "attention_qkv_dispatch.hpp"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_kernels.hpp"

namespace {

struct QkvCall {
    const bsmr::BwItem* items;
    uint32_t numItems;
    const bsmr::BwSplit* splits;
    uint32_t numSplits;
    const uint32_t* src;
    float scale;
    const uint16_t *Q, *Kt, *V;
    uint16_t* O;
    float *m, *s, *partial, *sPart, *mPart;
    uint32_t K, Kv, M, N, numSlots, nb;
    hipStream_t stream;
};

// fn(NL, VC): the unroll classes of attnQkv for (K, Kv) as compile-time constants
template <typename F>
void withQkvShape(uint32_t K, uint32_t Kv, F&& fn) {
    withPieces<16>(K / 32u, [&](auto NL) {
        if (Kv <= 128u) fn(NL, Int<1>{});
        else if (Kv <= 256u) fn(NL, Int<2>{});
        else fn(NL, Int<4>{});
    });
}

template <int MODE>
hipError_t launch(const QkvCall& c) {
    if (c.numItems) {
        const dim3 grid((c.numItems + 3u) / 4u, c.nb);
        withQkvShape(c.K, c.Kv, [&](auto NL, auto VC) {
            hipLaunchKernelGGL((bsmr::attnQkv<MODE, NL(), VC()>), grid, dim3(256), 0, c.stream, c.items, c.numItems, c.src,
                               c.scale, c.Q, c.Kt, c.V, c.O, c.m, c.s, c.partial, c.sPart, c.mPart, c.K, c.Kv, c.M, c.N,
                               c.numSlots);
        });
        if (hipError_t e = hipGetLastError()) return e;
    }
    return bsmrLaunchAttnQkvMerge(c.splits, c.numSplits, c.partial, c.sPart, c.mPart, c.O, c.m, c.s, c.Kv, c.M, c.numSlots, c.nb,
                                  MODE == 1, c.stream);
}

}  // namespace

hipError_t bsmrLaunchAttnQkv(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits, uint32_t numSplits,
                             const uint32_t* src, float scale, const uint16_t* Q, const uint16_t* Kt, const uint16_t* V,
                             uint16_t* O, float* m, float* s, float* partial, float* sPart, float* mPart, uint32_t K, uint32_t Kv,
                             uint32_t M, uint32_t N, uint32_t numSlots, uint32_t numBatches, bool bf16, hipStream_t stream) {
    const QkvCall c{items, numItems, splits, numSplits, src, scale, Q, Kt, V, O, m, s, partial, sPart, mPart, K, Kv, M, N,
                    numSlots, numBatches, stream};
    return bf16 ? launch<1>(c) : launch<0>(c);
}

hipError_t bsmrLaunchAttnQkvMerge(const bsmr::BwSplit* splits, uint32_t numSplits, const float* partial, const float* sPart,
                                  const float* mPart, uint16_t* O, float* m, float* s, uint32_t Kv, uint32_t M,
                                  uint32_t numSlots, uint32_t numBatches, bool bf16, hipStream_t stream) {
    if (!numSplits) return hipSuccess;   // only a handle with split rows launches the merge
    const uint64_t threads = (uint64_t)numSplits * (Kv / 4u);
    const dim3 grid((uint32_t)((threads + 255u) / 256u), numBatches);
    hipLaunchKernelGGL(bf16 ? bsmr::attnQkvMerge<1> : bsmr::attnQkvMerge<0>, grid, dim3(256), 0, stream, splits, numSplits, partial,
                       sPart, mPart, O, m, s, Kv, M, numSlots);
    return hipGetLastError();
}
