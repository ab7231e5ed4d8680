// One-pass backward of sparse attention: the translation unit of attnQkvBwdQ / attnQkvBwdKV / attnQkvBwdReduce
// (csrc/attention_qkv_bwd_kernels.hpp) and their launches.  Built like csrc/attention_qkv.hip - without packed fp32
// operations (Makefile, QKV_FLAGS) and with the namespace of the shared kernel headers renamed, here to bsmr_qkvbw, so
// that its copies of their non-template kernels are distinct symbols.  They are emitted into this unit's code object and
// never launched.
#define bsmr bsmr_qkvbw

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bsmr_hip.h"
#include "attention_qkv_launch.hpp"
#include "attention_qkv_bwd_kernels.hpp"

namespace {

template <int N>
using Int = std::integral_constant<int, N>;

// fn(NL, NLV): the unroll classes of both kernels for (K, Kv) as compile-time constants
template <typename F>
void withBwdShape(uint32_t K, uint32_t Kv, F&& fn) {
    auto pieces = [](uint32_t n, auto&& f) {
        if (n <= 1u) f(Int<1>{});
        else if (n <= 2u) f(Int<2>{});
        else if (n <= 4u) f(Int<4>{});
        else f(Int<8>{});
    };
    pieces(K / 32u, [&](auto NL) { pieces(Kv / 32u, [&](auto NLV) { fn(NL, NLV); }); });
}

template <int MODE>
hipError_t launch(const BsmrAttnBwdLists& rows, const BsmrAttnBwdLists& cols, float scale, const uint16_t* Q, const uint16_t* Kt,
                  const uint16_t* V, const uint16_t* dO, const float* m, const float* s, const float* D, uint16_t* dQ,
                  uint16_t* dKt, uint16_t* dV, float* rowPart, float* colPart, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N,
                  uint32_t nb, hipStream_t stream) {
    const auto* rowItems = static_cast<const bsmr::BwItem*>(rows.items);
    const auto* colItems = static_cast<const bsmr::BwItem*>(cols.items);
    auto reduce = [&](const BsmrAttnBwdLists& L, const float* partial, uint32_t stride, uint32_t offset, uint16_t* out,
                      uint32_t width, uint32_t outRows) {
        const uint64_t threads = (uint64_t)L.numSplits * (width / 4u);
        const dim3 grid((uint32_t)((threads + 255u) / 256u), nb);
        hipLaunchKernelGGL(bsmr::attnQkvBwdReduce<MODE>, grid, dim3(256), 0, stream, static_cast<const bsmr::BwSplit*>(L.splits),
                           L.numSplits, partial, stride, offset, out, width, outRows, L.numSlots);
    };
    if (dQ && rows.numItems) {
        const dim3 grid((rows.numItems + 3u) / 4u, nb);
        withBwdShape(K, Kv, [&](auto NL, auto NLV) {
            hipLaunchKernelGGL((bsmr::attnQkvBwdQ<MODE, NL(), NLV()>), grid, dim3(256), 0, stream, rowItems, rows.numItems, rows.src,
                               scale, Q, Kt, V, dO, m, s, D, dQ, rowPart, K, Kv, M, N, rows.numSlots);
        });
        if (hipError_t e = hipGetLastError()) return e;
        if (rows.numSplits) reduce(rows, rowPart, K, 0u, dQ, K, M);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if ((dKt || dV) && cols.numItems) {
        const dim3 grid((cols.numItems + 3u) / 4u, nb);
        withBwdShape(K, Kv, [&](auto NL, auto NLV) {
            hipLaunchKernelGGL((bsmr::attnQkvBwdKV<MODE, NL(), NLV()>), grid, dim3(256), 0, stream, colItems, cols.numItems, cols.src,
                               scale, Q, Kt, V, dO, m, s, D, dKt, dV, colPart, K, Kv, M, N, cols.numSlots);
        });
        if (hipError_t e = hipGetLastError()) return e;
        if (cols.numSplits && dKt) reduce(cols, colPart, K + Kv, 0u, dKt, K, N);
        if (cols.numSplits && dV) reduce(cols, colPart, K + Kv, K, dV, Kv, N);
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
    return bf16 ? launch<1>(rows, cols, scale, Q, Kt, V, dO, m, s, D, dQ, dKt, dV, rowPart, colPart, K, Kv, M, N, numBatches, stream)
                : launch<0>(rows, cols, scale, Q, Kt, V, dO, m, s, D, dQ, dKt, dV, rowPart, colPart, K, Kv, M, N, numBatches, stream);
}
