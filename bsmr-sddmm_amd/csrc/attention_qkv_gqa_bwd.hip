// One-pass backward of sparse attention with grouped key/value heads: the translation unit of attnQkvGqaBwdQ /
// attnQkvGqaBwdKV (csrc/attention_qkv_gqa_bwd_kernels.hpp) and their launches; the reduce of split destinations is
// csrc/attention_qkv_bwd.hip's (bsmrLaunchAttnQkvBwdReduce).  Built like its siblings without packed fp32 operations
// (Makefile, QKV_FLAGS).  It includes attention_qkv_bwd_kernels.hpp for the per-entry statements and instantiates none of
// its kernels: the code object holds the 32 + 48 instantiations of this unit's two kernels and no other kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsmr_hip.h"
#include "attention_qkv_dispatch.hpp"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_gqa_bwd_kernels.hpp"

namespace {

struct QkvGqaBwdCall {
    const BsmrAttnBwdLists &rows, &cols;
    float scale;
    const uint16_t *Q, *Kt, *V, *dO;
    const float *m, *s, *D;
    uint16_t *dQ, *dKt, *dV;
    float *rowPart, *colPart;
    uint32_t K, Kv, M, N, nb, g;
    hipStream_t stream;
};

// fn(G): the heads one wave of the row side serves for the class NL and a group of g - the largest of 1, 2, 4 with
// G NL <= 8 (the accumulators take 8 NL G registers per lane), and no more than hold g
template <int NL, typename F>
void withRowHeads(uint32_t g, F&& fn) {
    if constexpr (NL >= 8) fn(Int<1>{});
    else if constexpr (NL == 4) fn(Int<2>{});
    else if (g <= 2u) fn(Int<2>{});
    else fn(Int<4>{});
}

template <int MODE>
hipError_t launch(const QkvGqaBwdCall& c) {
    const uint32_t kvHeads = c.nb / c.g;
    if (c.dQ && c.rows.numItems) {
        withPieces<8>(c.K / 32u, [&](auto NL) {
            withRowHeads<NL()>(c.g, [&](auto G) {
                const uint32_t subs = (c.g + G() - 1u) / G();   // sub-groups of a KV group, G consecutive heads each
                const dim3 grid((c.rows.numItems + 3u) / 4u, kvHeads * subs);   // (subs <= g: at most nb)
                withPieces<8>(c.Kv / 32u, [&](auto NLV) {
                    hipLaunchKernelGGL((bsmr::attnQkvGqaBwdQ<MODE, NL(), NLV(), G()>), grid, dim3(256), 0, c.stream, c.rows.items,
                                       c.rows.numItems, c.rows.src, c.scale, c.Q, c.Kt, c.V, c.dO, c.m, c.s, c.D, c.dQ, c.rowPart,
                                       c.K, c.Kv, c.M, c.N, c.rows.numSlots, c.g, subs);
                });
            });
        });
        if (hipError_t e = hipGetLastError()) return e;
        // the row partials are indexed by query head, as attnQkvBwdQ leaves them
        if (hipError_t e = bsmrLaunchAttnQkvBwdReduce(c.rows, c.rowPart, c.K, 0u, c.dQ, c.K, c.M, c.nb, MODE == 1, c.stream)) return e;
    }
    if ((c.dKt || c.dV) && c.cols.numItems) {
        const dim3 grid((c.cols.numItems + 3u) / 4u, kvHeads);
        withPieces<8>(c.K / 32u, [&](auto NL) {
            withPieces<8>(c.Kv / 32u, [&](auto NLV) {
                hipLaunchKernelGGL((bsmr::attnQkvGqaBwdKV<MODE, NL(), NLV()>), grid, dim3(256), 0, c.stream, c.cols.items,
                                   c.cols.numItems, c.cols.src, c.scale, c.Q, c.Kt, c.V, c.dO, c.m, c.s, c.D, c.dKt, c.dV, c.colPart,
                                   c.K, c.Kv, c.M, c.N, c.cols.numSlots, c.g);
            });
        });
        if (hipError_t e = hipGetLastError()) return e;
        // the column partials hold one sum per KV head: the reduce runs on b / g batches
        const uint32_t stride = c.K + c.Kv;
        if (c.dKt)
            if (hipError_t e = bsmrLaunchAttnQkvBwdReduce(c.cols, c.colPart, stride, 0u, c.dKt, c.K, c.N, kvHeads, MODE == 1, c.stream))
                return e;
        if (c.dV)
            if (hipError_t e = bsmrLaunchAttnQkvBwdReduce(c.cols, c.colPart, stride, c.K, c.dV, c.Kv, c.N, kvHeads, MODE == 1, c.stream))
                return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t bsmrLaunchAttnQkvGqaBwd(const BsmrAttnBwdLists& rows, const BsmrAttnBwdLists& cols, float scale, const uint16_t* Q,
                                   const uint16_t* Kt, const uint16_t* V, const uint16_t* dO, const float* m, const float* s,
                                   const float* D, uint16_t* dQ, uint16_t* dKt, uint16_t* dV, float* rowPart, float* colPart,
                                   uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numBatches, uint32_t kvGroup,
                                   bool bf16, hipStream_t stream) {
    const QkvGqaBwdCall c{rows, cols, scale, Q, Kt, V, dO, m, s, D, dQ, dKt, dV, rowPart, colPart, K, Kv, M, N, numBatches, kvGroup,
                          stream};
    return bf16 ? launch<1>(c) : launch<0>(c);
}
