// One-pass sparse attention on a quantised KV cache: the translation unit of attnQkvKv (csrc/attention_qkv_kv_kernels.hpp)
// and its launches; the merge of split rows is csrc/attention_qkv.hip's (bsmrLaunchAttnQkvMerge).  Like that unit it is built
// without packed fp32 operations (Makefile, QKV_FLAGS; DESIGN.md 18 departure (4)), and it is a unit of its own so that its
// 90 instantiations compile beside the 30 of attention_qkv.hip, not behind them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsmr_hip.h"
#include "attention_qkv_dispatch.hpp"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_kv_kernels.hpp"

namespace {

struct QkvKvCall {
    const bsmr::BwItem* items;
    uint32_t numItems;
    const bsmr::BwSplit* splits;
    uint32_t numSplits;
    const uint32_t* src;
    float scale;
    const uint16_t* Q;
    const uint8_t *Kt, *Ks, *V, *Vs;
    uint16_t* O;
    float *m, *s, *partial, *sPart, *mPart;
    uint32_t K, Kv, M, N, numSlots, nb;
    hipStream_t stream;
};

template <int MODE, int FMT, bool MX>
hipError_t launch(const QkvKvCall& c) {
    if (c.numItems) {
        const dim3 grid((c.numItems + 3u) / 4u, c.nb);
        withPieces<16>(c.K / 32u, [&](auto NL) {   // the unroll class of the dot loop (attention_qkv.hip's classes)
            auto go = [&](auto VC) {
                hipLaunchKernelGGL((bsmr::attnQkvKv<MODE, FMT, MX, NL(), VC()>), grid, dim3(256), 0, c.stream, c.items, c.numItems,
                                   c.src, c.scale, c.Q, c.Kt, c.Ks, c.V, c.Vs, c.O, c.m, c.s, c.partial, c.sPart, c.mPart, c.K,
                                   c.Kv, c.M, c.N, c.numSlots);
            };
            // a lane's word of codes is 4 features of fp8, 8 of fp4: 64 lanes cover 256 / 512 features per value chunk
            if constexpr (FMT == 2) go(Int<1>{});
            else if (c.Kv <= 256u) go(Int<1>{});
            else go(Int<2>{});
        });
        if (hipError_t e = hipGetLastError()) return e;
    }
    // the merge of split rows: fp32 partials, whatever the KV format
    return bsmrLaunchAttnQkvMerge(c.splits, c.numSplits, c.partial, c.sPart, c.mPart, c.O, c.m, c.s, c.Kv, c.M, c.numSlots, c.nb,
                                  MODE == 1, c.stream);
}

template <int MODE>
hipError_t launchFormat(const QkvKvCall& c, int kvFormat, bool mx) {
    if (kvFormat == kQkvKvE2M1) return launch<MODE, 2, true>(c);
    if (kvFormat == kQkvKvE5M2) return mx ? launch<MODE, 1, true>(c) : launch<MODE, 1, false>(c);
    return mx ? launch<MODE, 0, true>(c) : launch<MODE, 0, false>(c);
}

}  // namespace

hipError_t bsmrLaunchAttnQkvKv(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits, uint32_t numSplits,
                               const uint32_t* src, float scale, const uint16_t* Q, const uint8_t* Kt, const uint8_t* Ks,
                               const uint8_t* V, const uint8_t* Vs, uint16_t* O, float* m, float* s, float* partial, float* sPart,
                               float* mPart, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots,
                               uint32_t numBatches, bool bf16, int kvFormat, bool mx, hipStream_t stream) {
    const QkvKvCall c{items, numItems, splits, numSplits, src, scale, Q, Kt, Ks, V, Vs, O, m, s, partial, sPart, mPart, K, Kv, M, N,
                      numSlots, numBatches, stream};
    return bf16 ? launchFormat<1>(c, kvFormat, mx) : launchFormat<0>(c, kvFormat, mx);
}
