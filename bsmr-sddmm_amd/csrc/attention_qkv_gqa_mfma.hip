// One-pass sparse attention with grouped key/value heads on the MFMA: the translation unit of attnQkvGqaMfma
// (csrc/attention_qkv_gqa_mfma_kernels.hpp) and its launch; the merge of split rows is csrc/attention_qkv.hip's
// (bsmrLaunchAttnQkvMerge).  Like its siblings it is built without packed fp32 operations (Makefile, QKV_FLAGS; DESIGN.md 18
// departure (4)) and includes helper headers only: the code object holds attnQkvGqaMfma's 24 instantiations and no other
// kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsmr_hip.h"
#include "attention_qkv_dispatch.hpp"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_gqa_mfma_kernels.hpp"

namespace {

struct QkvGqaMfmaCall {
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

template <int MODE>
hipError_t launch(const QkvGqaMfmaCall& c) {
    if (c.numItems) {
        const uint32_t subs = (c.g + bsmr::kQkvMfmaHeads - 1u) / bsmr::kQkvMfmaHeads;   // sub-groups of a KV group
        const dim3 grid((c.numItems + 3u) / 4u, c.nb / c.g * subs);                       // (subs <= g: at most nb)
        withPieces<8>(c.K / 32u, [&](auto NL) {
            auto go = [&](auto VC) {
                hipLaunchKernelGGL((bsmr::attnQkvGqaMfma<MODE, NL(), VC()>), grid, dim3(256), 0, c.stream, c.items, c.numItems,
                                   c.src, c.scale, c.Q, c.Kt, c.V, c.O, c.m, c.s, c.partial, c.sPart, c.mPart, c.K, c.Kv, c.M,
                                   c.N, c.numSlots, c.g, subs);
            };
            if (c.Kv <= 64u) go(Int<1>{});   // VC: chunks of 64 features
            else if (c.Kv <= 128u) go(Int<2>{});
            else go(Int<4>{});
        });
        if (hipError_t e = hipGetLastError()) return e;
    }
    // the merge of split rows: the partials are indexed by query head, as attnQkv leaves them
    return bsmrLaunchAttnQkvMerge(c.splits, c.numSplits, c.partial, c.sPart, c.mPart, c.O, c.m, c.s, c.Kv, c.M, c.numSlots, c.nb,
                                  MODE == 1, c.stream);
}

}  // namespace

hipError_t bsmrLaunchAttnQkvGqaMfma(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits,
                                    uint32_t numSplits, const uint32_t* src, float scale, const uint16_t* Q, const uint16_t* Kt,
                                    const uint16_t* V, uint16_t* O, float* m, float* s, float* partial, float* sPart,
                                    float* mPart, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots,
                                    uint32_t numBatches, uint32_t kvGroup, bool bf16, hipStream_t stream) {
    const QkvGqaMfmaCall c{items, numItems, splits, numSplits, src, scale, Q, Kt, V, O, m, s, partial, sPart, mPart, K, Kv, M, N,
                           numSlots, numBatches, kvGroup, stream};
    return bf16 ? launch<1>(c) : launch<0>(c);
}
