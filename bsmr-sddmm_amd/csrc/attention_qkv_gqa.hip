// One-pass sparse attention with grouped key/value heads: the translation unit of attnQkvGqa
// (csrc/attention_qkv_gqa_kernels.hpp) and its launch; the merge of split rows is csrc/attention_qkv.hip's
// (bsmrLaunchAttnQkvMerge).  Like its siblings it is built without packed fp32 operations (Makefile, QKV_FLAGS; DESIGN.md 18
// departure (4)) and includes helper headers only, plus attention_qkv_kernels.hpp for kQkvTile: attnQkv is not instantiated
// here, so the code object holds attnQkvGqa's 48 instantiations and no other kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsmr_hip.h"
#include "attention_qkv_dispatch.hpp"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_gqa_kernels.hpp"

namespace {

struct QkvGqaCall {
    const bsmr::BwItem* items;
    uint32_t numItems;
    const bsmr::BwSplit* splits;
    uint32_t numSplits;
    const uint32_t* src;
    float scale;
    const uint16_t *Q, *Kt, *V;
    uint16_t* O;
    float *m, *s, *partial, *sPart, *mPart;
    uint32_t K, Kv, M, N, numSlots, nb, g;
    hipStream_t stream;
};

// fn(G): the heads one wave serves - the smallest of 2, 4, 8 that holds min(g, 8)
template <typename F>
void withHeads(uint32_t g, F&& fn) {
    if (g <= 2u) fn(Int<2>{});
    else if (g <= 4u) fn(Int<4>{});
    else fn(Int<8>{});
}

template <int MODE>
hipError_t launch(const QkvGqaCall& c) {
    if (c.numItems) {
        withHeads(c.g, [&](auto G) {
            const uint32_t subs = (c.g + G() - 1u) / G();   // sub-groups of a KV group, G consecutive heads each
            const dim3 grid((c.numItems + 3u) / 4u, c.nb / c.g * subs);   // (subs <= g: at most nb)
            withPieces<8>(c.K / 32u, [&](auto NL) {
                auto go = [&](auto VC) {
                    hipLaunchKernelGGL((bsmr::attnQkvGqa<MODE, NL(), VC(), G()>), grid, dim3(256), 0, c.stream, c.items,
                                       c.numItems, c.src, c.scale, c.Q, c.Kt, c.V, c.O, c.m, c.s, c.partial, c.sPart, c.mPart,
                                       c.K, c.Kv, c.M, c.N, c.numSlots, c.g, subs);
                };
                if (c.Kv <= 128u) go(Int<1>{});
                else go(Int<2>{});
            });
        });
        if (hipError_t e = hipGetLastError()) return e;
    }
    // the merge of split rows: the partials are indexed by query head, as attnQkv leaves them
    return bsmrLaunchAttnQkvMerge(c.splits, c.numSplits, c.partial, c.sPart, c.mPart, c.O, c.m, c.s, c.Kv, c.M, c.numSlots, c.nb,
                                  MODE == 1, c.stream);
}

}  // namespace

hipError_t bsmrLaunchAttnQkvGqa(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits, uint32_t numSplits,
                                const uint32_t* src, float scale, const uint16_t* Q, const uint16_t* Kt, const uint16_t* V,
                                uint16_t* O, float* m, float* s, float* partial, float* sPart, float* mPart, uint32_t K,
                                uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots, uint32_t numBatches, uint32_t kvGroup,
                                bool bf16, hipStream_t stream) {
    const QkvGqaCall c{items, numItems, splits, numSplits, src, scale, Q, Kt, V, O, m, s, partial, sPart, mPart, K, Kv, M, N,
                       numSlots, numBatches, kvGroup, stream};
    return bf16 ? launch<1>(c) : launch<0>(c);
}
