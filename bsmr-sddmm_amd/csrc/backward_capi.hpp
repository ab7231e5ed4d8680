// The SDDMM backward (include/bsmr_hip.h "SDDMM backward"): a per-pattern handle holding S's CSR, its transpose and the
// chunked work lists of both directions, and the two calls that run csrc/spmm_kernels.hpp on them.
//
// Host side (no device call before everything is validated, so that a CPU test can check the rejections):
//   * the transpose is a stable counting sort by column: within a column, entries in ascending row = ascending CSR index;
//   * every destination list (a row for dA, a column for dB) longer than BSMR_BACKWARD_CHUNK is cut into chunks of that
//     length; the chunk table (which destinations are split, their workspace rows) depends on the pattern alone;
//   * the rows are scheduled in row_order (then every row it omits, in natural order), the columns in natural order -
//     rows with similar column sets run side by side and reuse the same rows of B in L2.
// Included at the end of bsmr_capi.hip.
#pragma once

#include "spmm_blocked_kernels.hpp"   // (includes spmm_kernels.hpp)
#include "fp8_kernels.hpp"            // the fp8 arms of runGather and runAttention (includes attention_kernels.hpp)
#include "fp4_kernels.hpp"            // ... and the MXFP4 arms

// Device format of bsmr_backward_attach_blocks (csrc/blocked_capi.hpp).  Residue lists: [0] the rows outside panels with
// blocks (destination = the row of Y), [1] the rows of panels with blocks (destination = their staging row); the chunk
// slots of both are numbered through.  segs / splitPanels exist only on a handle attached with segment_blocks >= 1.
struct BwBlocked {
    DevArray<bsmr::BlkPanel> panels;    // [numPanels]      panels with blocks
    DevArray<uint32_t> panelRows;       // [16 numPanels]   row of S or kBlkNull
    DevArray<bsmr::u32x4> cells;        // [64 blocks]      cells[b][lane][s]
    DevArray<bsmr::u32x4> cols;         // [4 blocks]       cols[b][k][s]
    DevArray<float> zeros;              // [4]              +0: what an empty cell and a padding column load
    DevArray<uint32_t> resCols;         // [residue]        s(t) of the residue lists: row by row, ascending CSR index
    DevArray<uint32_t> resIdx;          // [residue]        e(t)
    DevArray<bsmr::BwItem> items[2];
    DevArray<bsmr::BwSplit> splits[2];
    DevArray<bsmr::BlkSegment> segs;        // [numSegs]        segment_blocks >= 1: the work units, panel by panel
    DevArray<bsmr::BlkSplit> splitPanels;   // [numSplitPanels] the panels cut into two or more segments
    uint32_t numPanels = 0, numItems[2] = {0, 0}, numSplits[2] = {0, 0}, numSlots = 0;
    uint32_t segmentBlocks = 0, numSegs = 0, numSplitPanels = 0, numPartials = 0;   // numPartials: segments of split panels
    bsmr_blocked_stats stats{};
};

struct bsmr_backward {
    int device = 0;
    uint32_t M = 0, N = 0, nnz = 0;
    DevArray<uint32_t> rowOffsets;    // [M+1]  S's row offsets (the softmax, csrc/softmax_capi.hpp)
    DevArray<uint32_t> colIndices;    // [nnz]  s(t) of the row direction
    DevArray<uint32_t> cscRows;       // [nnz]  s(t) of the column direction
    DevArray<uint32_t> cscToCsr;      // [nnz]  e(t) of the column direction
    DevArray<bsmr::BwItem> items[2];
    DevArray<bsmr::BwSplit> splits[2];
    uint32_t numItems[2] = {0, 0}, numSplits[2] = {0, 0}, numSlots[2] = {0, 0}, maxLen[2] = {0, 0};
    bool permuteV = true;             // dB reads dP permuted into CSC order by a pass of its own (measured faster on 3 of
                                      // the 4 lab shapes); BSMR_BACKWARD_PERMUTE=0: through csc_to_csr in place
    uint64_t indexBytes = 0;
    int lanes16 = 0;                  // elements per lane of spmmGather16: 0 = the measured choice per slice width
                                      // (DESIGN 11); BSMR_GATHER16_LANES=4 / 8 at create: that layout for every width
    DevArray<float> work;             // chunk partials (+ permuted dP) (+ 16-bit copies of the gathered operands),
    uint64_t workFloats = 0;          // grown on demand
    std::unique_ptr<BwBlocked> blocked;   // bsmr_backward_attach_blocks
};

namespace {

// CSR checks shared by bsmr_csr_transpose and bsmr_backward_create
int checkCsr(uint32_t M, uint32_t N, uint32_t nnz, const uint32_t* ro, const uint32_t* ci) {
    if (!ro || (nnz && !ci)) return BSMR_ERR_INVALID_ARG;
    if (ro[0] != 0 || ro[M] != nnz) return BSMR_ERR_INVALID_ARG;
    for (uint32_t r = 0; r < M; ++r)
        if (ro[r + 1] < ro[r]) return BSMR_ERR_INVALID_ARG;
    for (uint32_t t = 0; t < nnz; ++t)
        if (ci[t] >= N) return BSMR_ERR_INVALID_ARG;
    return BSMR_OK;
}

void csrTranspose(uint32_t M, uint32_t N, uint32_t nnz, const uint32_t* ro, const uint32_t* ci, uint32_t* co,
                  uint32_t* cscRows, uint32_t* cscToCsr) {
    std::fill(co, co + N + 1, 0u);
    for (uint32_t t = 0; t < nnz; ++t) ++co[ci[t] + 1];
    for (uint32_t c = 0; c < N; ++c) co[c + 1] += co[c];
    std::vector<uint32_t> next(co, co + N);
    for (uint32_t r = 0; r < M; ++r)
        for (uint32_t t = ro[r]; t < ro[r + 1]; ++t) {
            const uint32_t p = next[ci[t]]++;
            cscRows[p] = r;
            cscToCsr[p] = t;
        }
}

// Work lists of one direction: offsets[numDest + 1] are the list bounds, `order` the schedule of the destinations.
void buildItems(const uint32_t* offsets, uint32_t numDest, const std::vector<uint32_t>& order,
                std::vector<bsmr::BwItem>& items, std::vector<bsmr::BwSplit>& splits, uint32_t& numSlots, uint32_t& maxLen) {
    constexpr uint32_t C = BSMR_BACKWARD_CHUNK;
    std::vector<uint32_t> firstSlot(numDest, bsmr::kBwDirect);
    numSlots = maxLen = 0;
    for (uint32_t d = 0; d < numDest; ++d) {   // the chunk table: natural destination order, whatever the schedule
        const uint32_t len = offsets[d + 1] - offsets[d];
        maxLen = std::max(maxLen, len);
        if (len > C) {
            const uint32_t chunks = (len + C - 1) / C;
            firstSlot[d] = numSlots;
            splits.push_back({d, numSlots, chunks, 0});
            numSlots += chunks;
        }
    }
    items.reserve(numDest + numSlots);
    for (uint32_t d : order) {
        const uint32_t b = offsets[d], e = offsets[d + 1];
        if (firstSlot[d] == bsmr::kBwDirect) {
            items.push_back({d, b, e, bsmr::kBwDirect});
            continue;
        }
        for (uint32_t k = 0, t = b; t < e; ++k, t += C) items.push_back({d, t, std::min(e, t + C), firstSlot[d] + k});
    }
}

uint64_t workFloatsFor(const bsmr_backward* bw, uint32_t K, uint32_t nb, bool withPermute) {
    uint64_t slots = std::max(bw->numSlots[0], bw->numSlots[1]);
    // attached blocks: the residue's chunk partials, then 16 fp32 staging rows per panel with blocks, then 16 fp32
    // partial rows per segment of a split panel
    if (bw->blocked)
        slots = std::max<uint64_t>(slots, (uint64_t)bw->blocked->numSlots + 16ull * bw->blocked->numPanels +
                                              16ull * bw->blocked->numPartials);
    return (slots * K + (withPermute ? bw->nnz : 0u)) * nb;
}

// The 16-bit copies of a *_mode call lie behind that call's partials and permuted values, on the next 16 bytes
// (hipMalloc aligns the workspace itself); two 16-bit elements per float of the workspace.
uint64_t lowpOffset(const bsmr_backward* bw, uint32_t K, uint32_t nb, bool withPermute) {
    return (workFloatsFor(bw, K, nb, withPermute) + 3u) & ~3ull;
}

bool validMode(int mode) { return mode == BSMR_COMPUTE_F16 || mode == BSMR_COMPUTE_BF16 || mode == BSMR_COMPUTE_F32; }

// fp32 -> fp16 / bf16, round to nearest even: the forward's own pass (convertOperands) in plain order over one or two
// contiguous arrays of n0 / n1 elements (multiples of 32); one launch
int roundOperands(int mode, const float* X0, uint64_t n0, uint16_t* O0, const float* X1, uint64_t n1, uint16_t* O1,
                  hipStream_t s) {
    const uint64_t n8 = (n0 + n1) / 8u;
    if (n8 == 0) return BSMR_OK;
    const dim3 grid((uint32_t)std::min<uint64_t>((n8 + bsmr::kThreads - 1) / bsmr::kThreads, 256u * 16u));
    withMode(mode, [&](auto MODE) {
        hipLaunchKernelGGL(bsmr::convertOperands<MODE()>, grid, dim3(bsmr::kThreads), 0, s, X0, n0 / 8u, X1, n1 / 8u, O0, O1, false);
    });
    BSMR_HIP(hipGetLastError());
    return BSMR_OK;
}

// Elements per lane of spmmGather16 for slice width W: 8 (16-byte loads) or 4 (8-byte loads).  W = 256 and 128 (DESIGN
// 11): 8 is up to 1.4x faster on the large shapes, 4 is 1.2x faster on the small nips-like one, where fp32 beats both.
// W = 64 and 32 are not measured: they keep the fp32 kernel's groups of 16 / 8 lanes.
uint32_t lanes16For(const bsmr_backward* bw, uint32_t W) {
    if (bw->lanes16) return (uint32_t)bw->lanes16;
    return W >= 128u ? 8u : 4u;
}

int growWork(bsmr_backward* bw, uint64_t floats) {
    if (floats <= bw->workFloats) return BSMR_OK;
    bw->workFloats = 0;
    // (alloc frees the old workspace before it asks for the new one: the largest allocation is never held twice)
    if (!allocOk(bw->work, floats, "hipMalloc(backward workspace)")) return BSMR_ERR_OOM;
    bw->workFloats = floats;
    return BSMR_OK;
}

int checkBackwardCall(const bsmr_backward* bw, uint32_t K, uint32_t nb) {
    if (!bw) return BSMR_ERR_INVALID_ARG;
    if (K == 0 || (K & 31u)) return BSMR_ERR_UNSUPPORTED_K;
    if (nb > 65535u) return BSMR_ERR_INVALID_ARG;
    return BSMR_OK;
}

// The work lists of one gather: items / splits as built by buildItems, src = s(t), map = e(t) or NULL for e(t) = t.
struct GatherLists {
    const bsmr::BwItem* items;
    uint32_t numItems;
    const bsmr::BwSplit* splits;
    uint32_t numSplits;
    const uint32_t* src;
    const uint32_t* map;
};

// ---- the launch of a gather (spmmGather*, attnGather*): its geometry and its compile-time shape, stated once ----------
// What the gathered rows are: fp32, fp16 / bf16, OCP fp8 bytes, or OCP e2m1 nibbles under MX block scales.
enum class RowKind { F32, B16, FP8, FP4 };

// Source bytes per lane of the fp8 gathers for slice width W (csrc/fp8_kernels.hpp "Lane layout")
constexpr uint32_t lanes8For(uint32_t W) { return W >= 128u ? 16u : 8u; }

// Source elements per lane of the fp4 gathers for slice width W (csrc/fp4_kernels.hpp "Lane layout"): 16-, 16-, 8- and
// 4-byte loads
constexpr uint32_t lanes4For(uint32_t W) { return W >= 128u ? 32u : W == 64u ? 16u : 8u; }

constexpr const uint8_t* kNoScales = nullptr;   // the E of an fp8 gather without MX: never read

// the fp8 format of a call: FMT 0 = e4m3fn, 1 = e5m2 (callers have refused every other format)
template <typename F>
auto withFp8(int fmt, F&& fn) {
    return fmt == BSMR_FP8_E4M3 ? fn(Int<0>{}) : fn(Int<1>{});
}

struct GatherGeometry {
    uint32_t W;        // slice width: the largest of 256, 128, 64, 32 that divides K
    uint32_t slices;   // per row
    uint32_t lanes;    // elements (fp8: bytes, fp4: nibbles) a lane loads at once; 0 for fp32 rows: one layout per W
    uint64_t units;    // items x slices: a unit is one slice of one item
    dim3 grid;
};

GatherGeometry gatherGeometry(const bsmr_backward* bw, uint32_t K, uint32_t numItems, uint32_t nb, RowKind kind) {
    GatherGeometry g;
    g.W = K % 256u == 0 ? 256u : K % 128u == 0 ? 128u : K % 64u == 0 ? 64u : 32u;
    g.slices = K / g.W;
    g.units = (uint64_t)numItems * g.slices;
    g.lanes = kind == RowKind::F32   ? 0u
              : kind == RowKind::B16 ? lanes16For(bw, g.W)
              : kind == RowKind::FP8 ? lanes8For(g.W)
                                     : lanes4For(g.W);
    // four waves per block; a unit takes W / lanes lanes of a wave - of fp32 rows W / 4, and the whole wave from W = 128 on
    const uint64_t unitsPerBlock =
        kind == RowKind::F32 ? 4u * (g.W >= 128u ? 1u : 64u / (g.W / 4u)) : 4u * (64u / (g.W / g.lanes));
    g.grid = dim3((uint32_t)((g.units + unitsPerBlock - 1) / unitsPerBlock), nb);
    return g;
}

// fn(W, LANES) with g's slice width and lane layout as compile-time constants.  KIND says which pairs exist, so a caller
// instantiates its kernel for exactly these: fp32 rows every W (LANES = 0, not a template argument of those kernels);
// 16-bit rows every W x {4, 8} (BSMR_GATHER16_LANES forces either); fp8 rows (256, 16), (128, 16), (64, 8), (32, 8) alone;
// fp4 rows (256, 32), (128, 32), (64, 16), (32, 8) alone.
template <RowKind KIND, typename F>
void withGatherShape(const GatherGeometry& g, F&& fn) {
    auto width = [&](auto W) {
        if constexpr (KIND == RowKind::F32) fn(W, Int<0>{});
        else if constexpr (KIND == RowKind::FP8) fn(W, Int<(int)lanes8For(W())>{});
        else if constexpr (KIND == RowKind::FP4) fn(W, Int<(int)lanes4For(W())>{});
        else if (g.lanes == 8u) fn(W, Int<8>{});
        else fn(W, Int<4>{});
    };
    switch (g.W) {
    case 256: width(Int<256>{}); break;
    case 128: width(Int<128>{}); break;
    case 64: width(Int<64>{}); break;
    default: width(Int<32>{}); break;
    }
}

// The element types of a gather.  mode BSMR_COMPUTE_F32: fp32 rows of X into fp32 rows of Y.  Otherwise the rows of X
// are mode's 16-bit format, and with y16 so are the rows of Y (else fp32).  fp8 >= 0: X holds bytes of that fp8 format
// instead, widened to mode (y16 is then set); scales non-NULL: each multiplied by its MX block scale ([b][rows][K / 32]).
// fp4: X holds e2m1 codes, two per byte, under `scales` (y16 is set, fp8 is not read).
struct GatherTypes {
    int mode = BSMR_COMPUTE_F32;
    bool y16 = false;
    int fp8 = -1;
    const uint8_t* scales = nullptr;
    bool fp4 = false;
};

RowKind rowKind(const GatherTypes& t) {
    return t.fp4 ? RowKind::FP4 : t.fp8 >= 0 ? RowKind::FP8 : t.mode != BSMR_COMPUTE_F32 ? RowKind::B16 : RowKind::F32;
}

// The gather and the reduction of its split destinations over one set of lists.  vB / xB / yB / pB: the batch strides of
// v, X, Y and the partials, in elements.
int runGather(const bsmr_backward* bw, const GatherLists& L, uint32_t K, const float* v, const void* Xrows, void* Yout,
              float* partial, uint64_t vB, uint64_t xB, uint64_t yB, uint64_t pB, uint32_t nb, hipStream_t s,
              const GatherTypes& t = {}) {
    const RowKind kind = rowKind(t);
    const GatherGeometry g = gatherGeometry(bw, K, L.numItems, nb, kind);
    const uint64_t nnz = vB;
    if (g.units) {
        // (what every spmm gather takes; `scales`: the two MX arguments of the fp8 kernels)
        auto launch = [&](auto kernel, auto* X, auto* Y, auto... scales) {
            hipLaunchKernelGGL(kernel, g.grid, dim3(256), 0, s, L.items, L.numItems, g.slices, L.src, L.map, v, X, Y, partial, K,
                               nnz, xB, yB, pB, scales...);
        };
        const bool map = L.map != nullptr;
        if (kind == RowKind::FP8) {
            const uint8_t* X8 = static_cast<const uint8_t*>(Xrows);
            uint16_t* Y16 = static_cast<uint16_t*>(Yout);
            const uint64_t eB = xB / 32u;
            withGatherShape<RowKind::FP8>(g, [&](auto W, auto LANES) {
                withFlag(map, [&](auto MAP) {
                    withMode(t.mode, [&](auto MODE) {
                        withFp8(t.fp8, [&](auto FMT) {
                            if (t.scales) launch(bsmr::spmmGather8<W(), LANES(), MAP(), MODE(), FMT(), true>, X8, Y16, t.scales, eB);
                            else launch(bsmr::spmmGather8<W(), LANES(), MAP(), MODE(), FMT()>, X8, Y16, kNoScales, (uint64_t)0);
                        });
                    });
                });
            });
        } else if (kind == RowKind::FP4) {   // xB elements of a batch are xB / 2 bytes of codes and xB / 32 scale bytes
            const uint8_t* X4 = static_cast<const uint8_t*>(Xrows);
            uint16_t* Y16 = static_cast<uint16_t*>(Yout);
            auto launch4 = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, g.grid, dim3(256), 0, s, L.items, L.numItems, g.slices, L.src, L.map, v, X4, Y16, partial,
                                   K, nnz, xB / 2u, yB, pB, t.scales, xB / 32u);
            };
            withGatherShape<RowKind::FP4>(g, [&](auto W, auto LANES) {
                withFlag(map, [&](auto MAP) {
                    withMode(t.mode, [&](auto MODE) { launch4(bsmr::spmmGather4<W(), LANES(), MAP(), MODE()>); });
                });
            });
        } else if (kind == RowKind::B16) {
            const uint16_t* X16 = static_cast<const uint16_t*>(Xrows);
            withGatherShape<RowKind::B16>(g, [&](auto W, auto LANES) {
                withFlag(map, [&](auto MAP) {
                    withMode(t.mode, [&](auto MODE) {
                        withFlag(t.y16, [&](auto OUT16) {
                            using YT = std::conditional_t<OUT16(), uint16_t, float>;   // the finished rows in the format of X, or fp32
                            launch(bsmr::spmmGather16<W(), LANES(), MAP(), MODE(), YT>, X16, static_cast<YT*>(Yout));
                        });
                    });
                });
            });
        } else {
            withGatherShape<RowKind::F32>(g, [&](auto W, auto) {
                withFlag(map, [&](auto MAP) {
                    launch(bsmr::spmmGather<W(), MAP()>, static_cast<const float*>(Xrows), static_cast<float*>(Yout));
                });
            });
        }
        BSMR_HIP(hipGetLastError());
    }
    if (L.numSplits) {
        const uint64_t threads = (uint64_t)L.numSplits * (K / 4u);
        const dim3 rgrid((uint32_t)((threads + 255u) / 256u), nb);
        if (t.y16)
            withMode(t.mode, [&](auto MODE) {
                hipLaunchKernelGGL(bsmr::spmmReduce16<MODE()>, rgrid, dim3(256), 0, s, L.splits, L.numSplits, partial,
                                   static_cast<uint16_t*>(Yout), K, yB, pB);
            });
        else
            hipLaunchKernelGGL(bsmr::spmmReduce, rgrid, dim3(256), 0, s, L.splits, L.numSplits, partial,
                               static_cast<float*>(Yout), K, yB, pB);
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

// The lists of direction dir (0: rows, 1: columns) for a call with (K, nb); the workspace is already large enough.  With
// permuteV the column direction first writes v in CSC order behind the partials of the workspace: v then points there.
int spmmLists(bsmr_backward* bw, uint32_t K, int dir, const float*& v, uint32_t nb, hipStream_t s, GatherLists& L) {
    const uint32_t* map = dir ? bw->cscToCsr : nullptr;
    if (dir && bw->permuteV && bw->nnz) {   // dP in CSC order, behind the partials of the workspace
        float* vT = bw->work + (uint64_t)bw->numSlots[dir] * K * nb;
        hipLaunchKernelGGL(bsmr::spmmPermute, dim3((bw->nnz + 255u) / 256u, nb), dim3(256), 0, s, bw->cscToCsr, bw->nnz, v, vT);
        BSMR_HIP(hipGetLastError());
        v = vT;
        map = nullptr;
    }
    L = GatherLists{bw->items[dir], bw->numItems[dir], bw->splits[dir], bw->numSplits[dir],
                    dir ? bw->cscRows : bw->colIndices, map};
    return BSMR_OK;
}

// Y = S_v X (dir 0) or S_v^T X (dir 1) for num_batches batches; the workspace is already large enough.
int runSpmm(bsmr_backward* bw, uint32_t K, int dir, const float* v, const void* Xrows, void* Yout, uint32_t nb, hipStream_t s,
            const GatherTypes& t = {}) {
    const uint32_t rowsX = dir ? bw->M : bw->N, rowsY = dir ? bw->N : bw->M;
    const uint64_t xB = (uint64_t)rowsX * K, yB = (uint64_t)rowsY * K, pB = (uint64_t)bw->numSlots[dir] * K;
    GatherLists L;
    if (int st = spmmLists(bw, K, dir, v, nb, s, L)) return st;
    return runGather(bw, L, K, v, Xrows, Yout, bw->work, bw->nnz, xB, yB, pB, nb, s, t);
}

bool is16(int mode) { return mode == BSMR_COMPUTE_F16 || mode == BSMR_COMPUTE_BF16; }

// The checks of every bsmr_spmm* entry point, in the order their statuses promise: the handle, K (UNSUPPORTED_K), the
// batches, then what the entry point itself accepts as compute mode and fp8 format (modeOk), transpose, the pointers.
// nnz = 0 reads neither v nor X nor the scales (torch hands out NULL for a zero-element tensor); Y is still written with
// zeros.  mx: the call carries MX block scales (any alignment: byte loads).
int checkSpmmCall(const bsmr_backward* bw, uint32_t K, bool modeOk, int transpose, uint32_t nb, const void* v, const void* X,
                  const void* Y, const void* scales = nullptr, bool mx = false) {
    if (int st = checkBackwardCall(bw, K, nb)) return st;
    if (!modeOk || (transpose != 0 && transpose != 1)) return BSMR_ERR_INVALID_ARG;
    const bool reads = bw->nnz != 0;
    if ((reads && (!v || !X || (mx && !scales))) || !Y || !aligned4(v) || !aligned16(X) || !aligned16(Y))
        return BSMR_ERR_INVALID_ARG;
    return BSMR_OK;
}

// ... and of the three bsmr_sddmm_backward* ones: an output that is NULL is not computed and its operand not looked at
int checkSddmmBackwardCall(const bsmr_backward* bw, uint32_t K, bool modeOk, uint32_t nb, const void* dP, const void* A,
                           const void* B, const void* dA, const void* dB) {
    if (int st = checkBackwardCall(bw, K, nb)) return st;
    if (!modeOk) return BSMR_ERR_INVALID_ARG;
    const bool reads = bw->nnz != 0;   // as bsmr_spmm: nnz = 0 reads no operand, the outputs are still zeroed
    if ((reads && !dP) || !aligned4(dP) || (dA && ((reads && !B) || !aligned16(B) || !aligned16(dA))) ||
        (dB && ((reads && !A) || !aligned16(A) || !aligned16(dB))))
        return BSMR_ERR_INVALID_ARG;
    return BSMR_OK;
}

// The body of the bsmr_spmm* entry points that gather the caller's rows as they are (checked, num_batches >= 1)
int spmmCall(bsmr_backward* bw, uint32_t K, int transpose, const float* v, const void* X, void* Y, uint32_t nb, void* stream,
             const GatherTypes& t = {}) {
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, workFloatsFor(bw, K, nb, bw->permuteV && transpose))) return st;
    return runSpmm(bw, K, transpose, v, X, Y, nb, static_cast<hipStream_t>(stream), t);
}

// ... and of bsmr_sddmm_backward and _16: dA = S_dP B, dB = S_dP^T A, each only where asked for
int sddmmBackwardCall(bsmr_backward* bw, uint32_t K, const float* dP, const void* A, const void* B, void* dA, void* dB,
                      uint32_t nb, void* stream, const GatherTypes& t = {}) {
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, workFloatsFor(bw, K, nb, bw->permuteV && dB))) return st;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (dA)
        if (int st = runSpmm(bw, K, 0, dP, B, dA, nb, s, t)) return st;
    if (dB)
        if (int st = runSpmm(bw, K, 1, dP, A, dB, nb, s, t)) return st;
    return BSMR_OK;
}

}  // namespace

extern "C" {

int bsmr_csr_transpose(uint32_t M, uint32_t N, uint32_t nnz, const uint32_t* row_offsets, const uint32_t* col_indices,
                       uint32_t* col_offsets, uint32_t* csc_rows, uint32_t* csc_to_csr) {
    if (!col_offsets || (nnz && (!csc_rows || !csc_to_csr))) return BSMR_ERR_INVALID_ARG;
    if (int st = checkCsr(M, N, nnz, row_offsets, col_indices)) return st;
    csrTranspose(M, N, nnz, row_offsets, col_indices, col_offsets, csc_rows, csc_to_csr);
    return BSMR_OK;
}

int bsmr_backward_create(bsmr_backward** out, int device, uint32_t M, uint32_t N, uint32_t nnz, const uint32_t* row_offsets,
                         const uint32_t* col_indices, const uint32_t* row_order, uint32_t num_ordered_rows) {
    if (!out) return BSMR_ERR_INVALID_ARG;
    *out = nullptr;
    if (num_ordered_rows && !row_order) return BSMR_ERR_INVALID_ARG;
    if (int st = checkCsr(M, N, nnz, row_offsets, col_indices)) return st;
    std::vector<uint32_t> order;
    try {
        std::vector<uint8_t> seen(M, 0);
        order.reserve(M);
        for (uint32_t i = 0; i < num_ordered_rows; ++i) {
            const uint32_t r = row_order[i];
            if (r >= M || seen[r]) return BSMR_ERR_INVALID_ARG;
            seen[r] = 1;
            order.push_back(r);
        }
        for (uint32_t r = 0; r < M; ++r)
            if (!seen[r]) order.push_back(r);
    } catch (const std::bad_alloc&) {
        return BSMR_ERR_OOM;
    }
    if (int st = useDevice(device)) return st;
    std::unique_ptr<bsmr_backward> bw;
    try {
        bw.reset(new bsmr_backward());
        bw->device = device;
        bw->M = M;
        bw->N = N;
        bw->nnz = nnz;
        const char* perm = std::getenv("BSMR_BACKWARD_PERMUTE");
        bw->permuteV = !perm || std::atoi(perm) != 0;
        const char* lanes = std::getenv("BSMR_GATHER16_LANES");
        const int l16 = lanes ? std::atoi(lanes) : 0;
        bw->lanes16 = l16 == 4 || l16 == 8 ? l16 : 0;
        std::vector<uint32_t> co(N + 1u), cscRows(nnz), cscToCsr(nnz), ci(col_indices, col_indices + nnz);
        csrTranspose(M, N, nnz, row_offsets, col_indices, co.data(), cscRows.data(), cscToCsr.data());
        std::vector<uint32_t> cols(N);
        for (uint32_t c = 0; c < N; ++c) cols[c] = c;
        std::vector<bsmr::BwItem> items[2];
        std::vector<bsmr::BwSplit> splits[2];
        buildItems(row_offsets, M, order, items[0], splits[0], bw->numSlots[0], bw->maxLen[0]);
        buildItems(co.data(), N, cols, items[1], splits[1], bw->numSlots[1], bw->maxLen[1]);
        if (items[0].size() > 0xFFFFFFFFull || items[1].size() > 0xFFFFFFFFull) return BSMR_ERR_INVALID_ARG;
        uint64_t& bytes = bw->indexBytes;
        if (int st = upload(bw->rowOffsets, std::vector<uint32_t>(row_offsets, row_offsets + M + 1u), bytes)) return st;
        if (int st = upload(bw->colIndices, ci, bytes)) return st;
        if (int st = upload(bw->cscRows, cscRows, bytes)) return st;
        if (int st = upload(bw->cscToCsr, cscToCsr, bytes)) return st;
        for (int d = 0; d < 2; ++d) {
            if (int st = upload(bw->items[d], items[d], bytes)) return st;
            if (int st = upload(bw->splits[d], splits[d], bytes)) return st;
            bw->numItems[d] = (uint32_t)items[d].size();
            bw->numSplits[d] = (uint32_t)splits[d].size();
        }
    } catch (const std::bad_alloc&) {
        return BSMR_ERR_OOM;
    }
    *out = bw.release();
    return BSMR_OK;
}

int bsmr_backward_destroy(bsmr_backward* bw) {
    if (!bw) return BSMR_OK;
    (void)hipSetDevice(bw->device);
    delete bw;
    return BSMR_OK;
}

int bsmr_backward_reserve(bsmr_backward* bw, uint32_t K, uint32_t num_batches) {
    if (int st = checkBackwardCall(bw, K, num_batches)) return st;
    BSMR_HIP(hipSetDevice(bw->device));
    return growWork(bw, workFloatsFor(bw, K, std::max(num_batches, 1u), bw->permuteV));
}

int bsmr_backward_get_stats(const bsmr_backward* bw, bsmr_backward_stats* out, size_t out_size) {
    if (!bw || !out) return BSMR_ERR_INVALID_ARG;
    bsmr_backward_stats full{};
    full.chunk = BSMR_BACKWARD_CHUNK;
    full.split_rows = bw->numSplits[0];
    full.split_cols = bw->numSplits[1];
    full.max_row_length = bw->maxLen[0];
    full.max_col_length = bw->maxLen[1];
    full.row_items = bw->numItems[0];
    full.col_items = bw->numItems[1];
    full.device_index_bytes = bw->indexBytes;
    full.workspace_bytes = bw->workFloats * sizeof(float);
    full.permute_values = bw->permuteV ? 1u : 0u;
    memcpy(out, &full, std::min(out_size, sizeof(full)));   // (the struct only grows at its end)
    return BSMR_OK;
}

int bsmr_spmm(bsmr_backward* bw, uint32_t K, int transpose, const float* v_dev, const float* X_dev, float* Y_dev,
              uint32_t num_batches, void* stream) {
    if (int st = checkSpmmCall(bw, K, true, transpose, num_batches, v_dev, X_dev, Y_dev)) return st;
    if (num_batches == 0) return BSMR_OK;
    return spmmCall(bw, K, transpose, v_dev, X_dev, Y_dev, num_batches, stream);
}

int bsmr_sddmm_backward(bsmr_backward* bw, uint32_t K, const float* dP_dev, const float* A_dev, const float* B_dev,
                        float* dA_dev, float* dB_dev, uint32_t num_batches, void* stream) {
    if (int st = checkSddmmBackwardCall(bw, K, true, num_batches, dP_dev, A_dev, B_dev, dA_dev, dB_dev)) return st;
    if (num_batches == 0 || (!dA_dev && !dB_dev)) return BSMR_OK;
    return sddmmBackwardCall(bw, K, dP_dev, A_dev, B_dev, dA_dev, dB_dev, num_batches, stream);
}

int bsmr_backward_reserve_mode(bsmr_backward* bw, uint32_t K, uint32_t num_batches, int compute_mode) {
    if (int st = checkBackwardCall(bw, K, num_batches)) return st;
    if (!validMode(compute_mode)) return BSMR_ERR_INVALID_ARG;
    if (compute_mode == BSMR_COMPUTE_F32) return bsmr_backward_reserve(bw, K, num_batches);
    BSMR_HIP(hipSetDevice(bw->device));
    // the largest covered call: bsmr_sddmm_backward_mode with both outputs (copies of A and of B)
    const uint32_t nb = std::max(num_batches, 1u);
    return growWork(bw, lowpOffset(bw, K, nb, bw->permuteV) + ((uint64_t)bw->M + bw->N) * K * nb / 2u);
}

int bsmr_spmm_mode(bsmr_backward* bw, uint32_t K, int transpose, const float* v_dev, const float* X_dev, float* Y_dev,
                   uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkSpmmCall(bw, K, validMode(compute_mode), transpose, num_batches, v_dev, X_dev, Y_dev)) return st;
    if (num_batches == 0) return BSMR_OK;
    if (compute_mode == BSMR_COMPUTE_F32) return spmmCall(bw, K, transpose, v_dev, X_dev, Y_dev, num_batches, stream);
    BSMR_HIP(hipSetDevice(bw->device));
    const uint64_t n = bw->nnz ? (uint64_t)(transpose ? bw->M : bw->N) * K * num_batches : 0u;   // nnz = 0 reads no X
    const uint64_t off = lowpOffset(bw, K, num_batches, bw->permuteV && transpose);
    if (int st = growWork(bw, off + n / 2u)) return st;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    uint16_t* X16 = reinterpret_cast<uint16_t*>(bw->work + off);
    if (int st = roundOperands(compute_mode, X_dev, n, X16, nullptr, 0, nullptr, s)) return st;
    return runSpmm(bw, K, transpose, v_dev, X16, Y_dev, num_batches, s, {compute_mode});
}

int bsmr_spmm_lowp(bsmr_backward* bw, uint32_t K, int transpose, const float* v_dev, const void* X16_dev, float* Y_dev,
                   uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkSpmmCall(bw, K, is16(compute_mode), transpose, num_batches, v_dev, X16_dev, Y_dev)) return st;
    if (num_batches == 0) return BSMR_OK;
    return spmmCall(bw, K, transpose, v_dev, X16_dev, Y_dev, num_batches, stream, {compute_mode});
}

int bsmr_spmm_16(bsmr_backward* bw, uint32_t K, int transpose, const float* v_dev, const void* X16_dev, void* Y16_dev,
                 uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkSpmmCall(bw, K, is16(compute_mode), transpose, num_batches, v_dev, X16_dev, Y16_dev)) return st;
    if (num_batches == 0) return BSMR_OK;
    return spmmCall(bw, K, transpose, v_dev, X16_dev, Y16_dev, num_batches, stream, {compute_mode, true});
}

int bsmr_sddmm_backward_16(bsmr_backward* bw, uint32_t K, const float* dP_dev, const void* A16_dev, const void* B16_dev,
                           void* dA16_dev, void* dB16_dev, uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkSddmmBackwardCall(bw, K, is16(compute_mode), num_batches, dP_dev, A16_dev, B16_dev, dA16_dev, dB16_dev))
        return st;
    if (num_batches == 0 || (!dA16_dev && !dB16_dev)) return BSMR_OK;
    return sddmmBackwardCall(bw, K, dP_dev, A16_dev, B16_dev, dA16_dev, dB16_dev, num_batches, stream, {compute_mode, true});
}

int bsmr_sddmm_backward_mode(bsmr_backward* bw, uint32_t K, const float* dP_dev, const float* A_dev, const float* B_dev,
                             float* dA_dev, float* dB_dev, uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkSddmmBackwardCall(bw, K, validMode(compute_mode), num_batches, dP_dev, A_dev, B_dev, dA_dev, dB_dev))
        return st;
    if (num_batches == 0 || (!dA_dev && !dB_dev)) return BSMR_OK;
    if (compute_mode == BSMR_COMPUTE_F32)
        return sddmmBackwardCall(bw, K, dP_dev, A_dev, B_dev, dA_dev, dB_dev, num_batches, stream);
    BSMR_HIP(hipSetDevice(bw->device));
    // B is gathered by dA, A by dB: only what a requested product reads is rounded, B16 first, A16 behind it
    const bool reads = bw->nnz != 0;
    const uint64_t nB = reads && dA_dev ? (uint64_t)bw->N * K * num_batches : 0u;
    const uint64_t nA = reads && dB_dev ? (uint64_t)bw->M * K * num_batches : 0u;
    const uint64_t off = lowpOffset(bw, K, num_batches, bw->permuteV && dB_dev);
    if (int st = growWork(bw, off + (nA + nB) / 2u)) return st;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    uint16_t* B16 = reinterpret_cast<uint16_t*>(bw->work + off);
    uint16_t* A16 = B16 + nB;
    if (int st = roundOperands(compute_mode, A_dev, nA, A16, B_dev, nB, B16, s)) return st;
    if (dA_dev)
        if (int st = runSpmm(bw, K, 0, dP_dev, B16, dA_dev, num_batches, s, {compute_mode})) return st;
    if (dB_dev)
        if (int st = runSpmm(bw, K, 1, dP_dev, A16, dB_dev, num_batches, s, {compute_mode})) return st;
    return BSMR_OK;
}

}  // extern "C"
