// One-pass sparse attention with grouped key/value heads on a quantised KV cache: the translation unit of attnQkvGqaKv
// (csrc/attention_qkv_gqa_kv_kernels.hpp) and its launch; the merge of split rows is csrc/attention_qkv.hip's
// (bsmrLaunchAttnQkvMerge).  Like its siblings it is built without packed fp32 operations (Makefile, QKV_FLAGS; DESIGN.md 18
// departure (4)).  The kernel headers it includes for their helpers (qkvWiden, QkvPiece, qkvGqaQLds) define attnQkvKv and
// attnQkvGqa as templates only: neither is instantiated here, so the code object holds attnQkvGqaKv's 80 instantiations
// (2 MODE x 5 (FMT, MX) x 4 NL x 2 G) and no other kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsmr_hip.h"
#include "attention_qkv_dispatch.hpp"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_gqa_kv_kernels.hpp"

namespace {

struct QkvGqaKvCall {
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
    uint32_t K, Kv, M, N, numSlots, nb, g;
    hipStream_t stream;
};

// fn(G): the heads one wave serves - 4 up to g = 4, else 8.  There is no G = 2 class as attention_qkv_gqa.hip has: with it
// this unit compiled slower than every other one-pass unit, so g = 2 runs in G = 4 with two clamped heads.
template <typename F>
void withHeads(uint32_t g, F&& fn) {
    if (g <= 4u) fn(Int<4>{});
    else fn(Int<8>{});
}

template <int MODE, int FMT, bool MX>
hipError_t launch(const QkvGqaKvCall& c) {
    if (c.numItems) {
        withHeads(c.g, [&](auto G) {
            const uint32_t subs = (c.g + G() - 1u) / G();   // sub-groups of a KV group, G consecutive heads each
            const dim3 grid((c.numItems + 3u) / 4u, c.nb / c.g * subs);   // (subs <= g: at most nb)
            withPieces<8>(c.K / 32u, [&](auto NL) {   // one value chunk covers Kv <= 256 in every format: no VC class
                hipLaunchKernelGGL((bsmr::attnQkvGqaKv<MODE, FMT, MX, NL(), G()>), grid, dim3(256), 0, c.stream, c.items,
                                   c.numItems, c.src, c.scale, c.Q, c.Kt, c.Ks, c.V, c.Vs, c.O, c.m, c.s, c.partial, c.sPart,
                                   c.mPart, c.K, c.Kv, c.M, c.N, c.numSlots, c.g, subs);
            });
        });
        if (hipError_t e = hipGetLastError()) return e;
    }
    // the merge of split rows: fp32 partials indexed by query head, whatever the KV format
    return bsmrLaunchAttnQkvMerge(c.splits, c.numSplits, c.partial, c.sPart, c.mPart, c.O, c.m, c.s, c.Kv, c.M, c.numSlots, c.nb,
                                  MODE == 1, c.stream);
}

template <int MODE>
hipError_t launchFormat(const QkvGqaKvCall& c, int kvFormat, bool mx) {
    if (kvFormat == kQkvKvE2M1) return launch<MODE, 2, true>(c);
    if (kvFormat == kQkvKvE5M2) return mx ? launch<MODE, 1, true>(c) : launch<MODE, 1, false>(c);
    return mx ? launch<MODE, 0, true>(c) : launch<MODE, 0, false>(c);
}

}  // namespace

hipError_t bsmrLaunchAttnQkvGqaKv(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits, uint32_t numSplits,
                                  const uint32_t* src, float scale, const uint16_t* Q, const uint8_t* Kt, const uint8_t* Ks,
                                  const uint8_t* V, const uint8_t* Vs, uint16_t* O, float* m, float* s, float* partial,
                                  float* sPart, float* mPart, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots,
                                  uint32_t numBatches, uint32_t kvGroup, bool bf16, int kvFormat, bool mx, hipStream_t stream) {
    const QkvGqaKvCall c{items, numItems, splits, numSplits, src, scale, Q, Kt, Ks, V, Vs, O, m, s, partial, sPart, mPart, K, Kv, M,
                         N, numSlots, numBatches, kvGroup, stream};
    return bf16 ? launchFormat<1>(c, kvFormat, mx) : launchFormat<0>(c, kvFormat, mx);
}
