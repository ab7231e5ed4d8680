// One-pass backward of sparse attention: the translation unit of attnQkvBwdQ / attnQkvBwdKV / attnQkvBwdReduce
// (csrc/attention_qkv_bwd_kernels.hpp) and their launches; attnQkvBwdReduce has its home here, and the unit of the grouped
// backward ends with it too (bsmrLaunchAttnQkvBwdReduce).  Built like csrc/attention_qkv.hip: without packed fp32
// operations (Makefile, QKV_FLAGS), on helper headers that define no kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsmr_hip.h"
#include "attention_qkv_dispatch.hpp"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_bwd_kernels.hpp"

namespace {

struct QkvBwdCall {
    const BsmrAttnBwdLists &rows, &cols;
    float scale;
    const uint16_t *Q, *Kt, *V, *dO;
    const float *m, *s, *D;
    uint16_t *dQ, *dKt, *dV;
    float *rowPart, *colPart;
    uint32_t K, Kv, M, N, nb;
    hipStream_t stream;
};

// fn(NL, NLV): the unroll classes of both kernels for (K, Kv) as compile-time constants
template <typename F>
void withBwdShape(uint32_t K, uint32_t Kv, F&& fn) {
    withPieces<8>(K / 32u, [&](auto NL) { withPieces<8>(Kv / 32u, [&](auto NLV) { fn(NL, NLV); }); });
}

template <int MODE>
hipError_t launch(const QkvBwdCall& c) {
    auto reduce = [&](const BsmrAttnBwdLists& L, const float* partial, uint32_t stride, uint32_t offset, uint16_t* out,
                      uint32_t width, uint32_t outRows) {
        const uint64_t threads = (uint64_t)L.numSplits * (width / 4u);
        const dim3 grid((uint32_t)((threads + 255u) / 256u), c.nb);
        hipLaunchKernelGGL(bsmr::attnQkvBwdReduce<MODE>, grid, dim3(256), 0, c.stream, L.splits, L.numSplits, partial, stride, offset,
                           out, width, outRows, L.numSlots);
    };
    if (c.dQ && c.rows.numItems) {
        const dim3 grid((c.rows.numItems + 3u) / 4u, c.nb);
        withBwdShape(c.K, c.Kv, [&](auto NL, auto NLV) {
            hipLaunchKernelGGL((bsmr::attnQkvBwdQ<MODE, NL(), NLV()>), grid, dim3(256), 0, c.stream, c.rows.items, c.rows.numItems,
                               c.rows.src, c.scale, c.Q, c.Kt, c.V, c.dO, c.m, c.s, c.D, c.dQ, c.rowPart, c.K, c.Kv, c.M, c.N,
                               c.rows.numSlots);
        });
        if (hipError_t e = hipGetLastError()) return e;
        if (c.rows.numSplits) reduce(c.rows, c.rowPart, c.K, 0u, c.dQ, c.K, c.M);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if ((c.dKt || c.dV) && c.cols.numItems) {
        const dim3 grid((c.cols.numItems + 3u) / 4u, c.nb);
        withBwdShape(c.K, c.Kv, [&](auto NL, auto NLV) {
            hipLaunchKernelGGL((bsmr::attnQkvBwdKV<MODE, NL(), NLV()>), grid, dim3(256), 0, c.stream, c.cols.items, c.cols.numItems,
                               c.cols.src, c.scale, c.Q, c.Kt, c.V, c.dO, c.m, c.s, c.D, c.dKt, c.dV, c.colPart, c.K, c.Kv, c.M, c.N,
                               c.cols.numSlots);
        });
        if (hipError_t e = hipGetLastError()) return e;
        if (c.cols.numSplits && c.dKt) reduce(c.cols, c.colPart, c.K + c.Kv, 0u, c.dKt, c.K, c.N);
        if (c.cols.numSplits && c.dV) reduce(c.cols, c.colPart, c.K + c.Kv, c.K, c.dV, c.Kv, c.N);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t bsmrLaunchAttnQkvBwd(const BsmrAttnBwdLists& rows, const BsmrAttnBwdLists& cols, float scale, const uint16_t* Q,
                                const uint16_t* Kt, const uint16_t* V, const uint16_t* dO, const float* m, const float* s,
                                const float* D, uint16_t* dQ, uint16_t* dKt, uint16_t* dV, float* rowPart, float* colPart,
                                uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numBatches, bool bf16,
                                hipStream_t stream) {
    const QkvBwdCall c{rows, cols, scale, Q, Kt, V, dO, m, s, D, dQ, dKt, dV, rowPart, colPart, K, Kv, M, N, numBatches, stream};
    return bf16 ? launch<1>(c) : launch<0>(c);
}

// The reduce alone, for the unit of the grouped backward.  launch() above keeps its own launch statement, and this entry
// reaches the kernel through a template of its own: the compiler emits a unit's kernels in the order in which they are
// first instantiated, and the unit's assembly is compared byte for byte with its earlier one.
namespace {
template <int MODE>
hipError_t launchReduce(const BsmrAttnBwdLists& L, const float* partial, uint32_t stride, uint32_t offset, uint16_t* out,
                        uint32_t width, uint32_t outRows, uint32_t nb, hipStream_t stream) {
    const uint64_t threads = (uint64_t)L.numSplits * (width / 4u);
    const dim3 grid((uint32_t)((threads + 255u) / 256u), nb);
    hipLaunchKernelGGL(bsmr::attnQkvBwdReduce<MODE>, grid, dim3(256), 0, stream, L.splits, L.numSplits, partial, stride, offset, out,
                       width, outRows, L.numSlots);
    return hipGetLastError();
}
}  // namespace

hipError_t bsmrLaunchAttnQkvBwdReduce(const BsmrAttnBwdLists& lists, const float* partial, uint32_t stride, uint32_t offset,
                                      uint16_t* out, uint32_t width, uint32_t outRows, uint32_t numBatches, bool bf16,
                                      hipStream_t stream) {
    if (!lists.numSplits) return hipSuccess;   // only a direction with split destinations launches the reduce
    return bf16 ? launchReduce<1>(lists, partial, stride, offset, out, width, outRows, numBatches, stream)
                : launchReduce<0>(lists, partial, stride, offset, out, width, outRows, numBatches, stream);
}
