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
    if (mode == BSMR_COMPUTE_F16)
        hipLaunchKernelGGL(bsmr::convertOperands<0>, grid, dim3(bsmr::kThreads), 0, s, X0, n0 / 8u, X1, n1 / 8u, O0, O1, false);
    else
        hipLaunchKernelGGL(bsmr::convertOperands<1>, grid, dim3(bsmr::kThreads), 0, s, X0, n0 / 8u, X1, n1 / 8u, O0, O1, false);
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

template <int W, int VE, typename... Args>
void launchGather16(bool map, int mode, dim3 grid, hipStream_t s, Args... args) {
    if (mode == BSMR_COMPUTE_F16) {
        if (map) hipLaunchKernelGGL((bsmr::spmmGather16<W, VE, true, 0>), grid, dim3(256), 0, s, args...);
        else hipLaunchKernelGGL((bsmr::spmmGather16<W, VE, false, 0>), grid, dim3(256), 0, s, args...);
    } else {
        if (map) hipLaunchKernelGGL((bsmr::spmmGather16<W, VE, true, 1>), grid, dim3(256), 0, s, args...);
        else hipLaunchKernelGGL((bsmr::spmmGather16<W, VE, false, 1>), grid, dim3(256), 0, s, args...);
    }
}

// ... with the finished rows stored in the format of X (bsmr_spmm_16, bsmr_sddmm_backward_16)
template <int W, int VE, typename... Args>
void launchGather16Out(bool map, int mode, dim3 grid, hipStream_t s, Args... args) {
    if (mode == BSMR_COMPUTE_F16) {
        if (map) hipLaunchKernelGGL((bsmr::spmmGather16<W, VE, true, 0, uint16_t>), grid, dim3(256), 0, s, args...);
        else hipLaunchKernelGGL((bsmr::spmmGather16<W, VE, false, 0, uint16_t>), grid, dim3(256), 0, s, args...);
    } else {
        if (map) hipLaunchKernelGGL((bsmr::spmmGather16<W, VE, true, 1, uint16_t>), grid, dim3(256), 0, s, args...);
        else hipLaunchKernelGGL((bsmr::spmmGather16<W, VE, false, 1, uint16_t>), grid, dim3(256), 0, s, args...);
    }
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

// The gather and the reduction of its split destinations over one set of lists.  xMode says what the rows of X are: fp32
// (spmmGather), or fp16 / bf16 (spmmGather16).  y16 (16-bit X only): Yout holds xMode's format too; otherwise fp32.
// vB / xB / yB / pB: the batch strides of v, X, Y and the partials, in elements.
int runGather(const bsmr_backward* bw, const GatherLists& L, uint32_t K, const float* v, const void* Xrows, void* Yout,
              float* partial, uint64_t vB, uint64_t xB, uint64_t yB, uint64_t pB, uint32_t nb, hipStream_t s, int xMode,
              bool y16) {
    const bool lowp = xMode != BSMR_COMPUTE_F32;
    float* Y = y16 ? nullptr : static_cast<float*>(Yout);
    uint16_t* Y16 = y16 ? static_cast<uint16_t*>(Yout) : nullptr;
    const float* X = lowp ? nullptr : static_cast<const float*>(Xrows);
    const uint16_t* X16 = lowp ? static_cast<const uint16_t*>(Xrows) : nullptr;
    const uint64_t nnz = vB;
    const uint32_t* src = L.src;
    const uint32_t* map = L.map;
    const uint32_t W = K % 256u == 0 ? 256u : K % 128u == 0 ? 128u : K % 64u == 0 ? 64u : 32u;
    const uint32_t slices = K / W;
    const uint64_t units = (uint64_t)L.numItems * slices;
    const uint32_t VE = lowp ? lanes16For(bw, W) : 0u;
    const uint64_t unitsPerBlock = lowp ? 4u * (64u / (W / VE)) : 4u * (W >= 128u ? 1u : 64u / (W / 4u));
    const dim3 grid((uint32_t)((units + unitsPerBlock - 1) / unitsPerBlock), nb);
    if (units && y16) {
#define BSMR_SPMM16_OUT_LAUNCH(WW)                                                                                           \
    if (VE == 8u)                                                                                                            \
        launchGather16Out<WW, 8>(map != nullptr, xMode, grid, s, L.items, L.numItems, slices, src, map, v, X16,              \
                                 Y16, partial, K, nnz, xB, yB, pB);                                                          \
    else                                                                                                                     \
        launchGather16Out<WW, 4>(map != nullptr, xMode, grid, s, L.items, L.numItems, slices, src, map, v, X16,              \
                                 Y16, partial, K, nnz, xB, yB, pB)
        switch (W) {
        case 256: BSMR_SPMM16_OUT_LAUNCH(256); break;
        case 128: BSMR_SPMM16_OUT_LAUNCH(128); break;
        case 64: BSMR_SPMM16_OUT_LAUNCH(64); break;
        default: BSMR_SPMM16_OUT_LAUNCH(32); break;
        }
#undef BSMR_SPMM16_OUT_LAUNCH
        BSMR_HIP(hipGetLastError());
    } else if (units && lowp) {
#define BSMR_SPMM16_LAUNCH(WW)                                                                                               \
    if (VE == 8u)                                                                                                            \
        launchGather16<WW, 8>(map != nullptr, xMode, grid, s, L.items, L.numItems, slices, src, map, v, X16, Y,              \
                              partial, K, nnz, xB, yB, pB);                                                                  \
    else                                                                                                                     \
        launchGather16<WW, 4>(map != nullptr, xMode, grid, s, L.items, L.numItems, slices, src, map, v, X16, Y,              \
                              partial, K, nnz, xB, yB, pB)
        switch (W) {
        case 256: BSMR_SPMM16_LAUNCH(256); break;
        case 128: BSMR_SPMM16_LAUNCH(128); break;
        case 64: BSMR_SPMM16_LAUNCH(64); break;
        default: BSMR_SPMM16_LAUNCH(32); break;
        }
#undef BSMR_SPMM16_LAUNCH
        BSMR_HIP(hipGetLastError());
    } else if (units) {
#define BSMR_SPMM_LAUNCH(WW, MAP)                                                                                            \
    hipLaunchKernelGGL((bsmr::spmmGather<WW, MAP>), grid, dim3(256), 0, s, L.items, L.numItems, slices, src,                 \
                       map, v, X, Y, partial, K, nnz, xB, yB, pB)
        const bool m = map != nullptr;
        switch (W) {
        case 256: if (m) BSMR_SPMM_LAUNCH(256, true); else BSMR_SPMM_LAUNCH(256, false); break;
        case 128: if (m) BSMR_SPMM_LAUNCH(128, true); else BSMR_SPMM_LAUNCH(128, false); break;
        case 64: if (m) BSMR_SPMM_LAUNCH(64, true); else BSMR_SPMM_LAUNCH(64, false); break;
        default: if (m) BSMR_SPMM_LAUNCH(32, true); else BSMR_SPMM_LAUNCH(32, false); break;
        }
#undef BSMR_SPMM_LAUNCH
        BSMR_HIP(hipGetLastError());
    }
    if (L.numSplits && y16) {
        const uint64_t threads = (uint64_t)L.numSplits * (K / 4u);
        const dim3 rgrid((uint32_t)((threads + 255u) / 256u), nb);
        if (xMode == BSMR_COMPUTE_F16)
            hipLaunchKernelGGL(bsmr::spmmReduce16<0>, rgrid, dim3(256), 0, s, L.splits, L.numSplits, partial, Y16, K, yB, pB);
        else
            hipLaunchKernelGGL(bsmr::spmmReduce16<1>, rgrid, dim3(256), 0, s, L.splits, L.numSplits, partial, Y16, K, yB, pB);
        BSMR_HIP(hipGetLastError());
    } else if (L.numSplits) {
        const uint64_t threads = (uint64_t)L.numSplits * (K / 4u);
        hipLaunchKernelGGL(bsmr::spmmReduce, dim3((uint32_t)((threads + 255u) / 256u), nb), dim3(256), 0, s, L.splits,
                           L.numSplits, partial, Y, K, yB, pB);
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

// Y = S_v X (dir 0) or S_v^T X (dir 1) for num_batches batches; the workspace is already large enough.  xMode / y16 as
// runGather.
int runSpmm(bsmr_backward* bw, uint32_t K, int dir, const float* v, const void* Xrows, void* Yout, uint32_t nb, hipStream_t s,
            int xMode = BSMR_COMPUTE_F32, bool y16 = false) {
    const uint32_t rowsX = dir ? bw->M : bw->N, rowsY = dir ? bw->N : bw->M;
    const uint64_t xB = (uint64_t)rowsX * K, yB = (uint64_t)rowsY * K, pB = (uint64_t)bw->numSlots[dir] * K;
    GatherLists L;
    if (int st = spmmLists(bw, K, dir, v, nb, s, L)) return st;
    return runGather(bw, L, K, v, Xrows, Yout, bw->work, bw->nnz, xB, yB, pB, nb, s, xMode, y16);
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
    if (int st = checkBackwardCall(bw, K, num_batches)) return st;
    if (transpose != 0 && transpose != 1) return BSMR_ERR_INVALID_ARG;
    // nnz = 0 reads neither v nor X (torch hands out NULL for a zero-element tensor); Y is still written with zeros
    const bool reads = bw->nnz != 0;
    if ((reads && (!v_dev || !X_dev)) || !Y_dev || !aligned4(v_dev) || !aligned16(X_dev) || !aligned16(Y_dev))
        return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, workFloatsFor(bw, K, num_batches, bw->permuteV && transpose))) return st;
    return runSpmm(bw, K, transpose, v_dev, X_dev, Y_dev, num_batches, static_cast<hipStream_t>(stream));
}

int bsmr_sddmm_backward(bsmr_backward* bw, uint32_t K, const float* dP_dev, const float* A_dev, const float* B_dev,
                        float* dA_dev, float* dB_dev, uint32_t num_batches, void* stream) {
    if (int st = checkBackwardCall(bw, K, num_batches)) return st;
    const bool reads = bw->nnz != 0;   // as bsmr_spmm: nnz = 0 reads no operand, the outputs are still zeroed
    if ((reads && !dP_dev) || !aligned4(dP_dev) || (dA_dev && ((reads && !B_dev) || !aligned16(B_dev) || !aligned16(dA_dev))) ||
        (dB_dev && ((reads && !A_dev) || !aligned16(A_dev) || !aligned16(dB_dev))))
        return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0 || (!dA_dev && !dB_dev)) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, workFloatsFor(bw, K, num_batches, bw->permuteV && dB_dev))) return st;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (dA_dev)
        if (int st = runSpmm(bw, K, 0, dP_dev, B_dev, dA_dev, num_batches, s)) return st;
    if (dB_dev)
        if (int st = runSpmm(bw, K, 1, dP_dev, A_dev, dB_dev, num_batches, s)) return st;
    return BSMR_OK;
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
    if (int st = checkBackwardCall(bw, K, num_batches)) return st;
    if (!validMode(compute_mode)) return BSMR_ERR_INVALID_ARG;
    if (compute_mode == BSMR_COMPUTE_F32) return bsmr_spmm(bw, K, transpose, v_dev, X_dev, Y_dev, num_batches, stream);
    if (transpose != 0 && transpose != 1) return BSMR_ERR_INVALID_ARG;
    const bool reads = bw->nnz != 0;
    if ((reads && (!v_dev || !X_dev)) || !Y_dev || !aligned4(v_dev) || !aligned16(X_dev) || !aligned16(Y_dev))
        return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    const uint64_t n = reads ? (uint64_t)(transpose ? bw->M : bw->N) * K * num_batches : 0u;   // nnz = 0 reads no X
    const uint64_t off = lowpOffset(bw, K, num_batches, bw->permuteV && transpose);
    if (int st = growWork(bw, off + n / 2u)) return st;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    uint16_t* X16 = reinterpret_cast<uint16_t*>(bw->work + off);
    if (int st = roundOperands(compute_mode, X_dev, n, X16, nullptr, 0, nullptr, s)) return st;
    return runSpmm(bw, K, transpose, v_dev, X16, Y_dev, num_batches, s, compute_mode);
}

int bsmr_spmm_lowp(bsmr_backward* bw, uint32_t K, int transpose, const float* v_dev, const void* X16_dev, float* Y_dev,
                   uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkBackwardCall(bw, K, num_batches)) return st;
    if (compute_mode != BSMR_COMPUTE_F16 && compute_mode != BSMR_COMPUTE_BF16) return BSMR_ERR_INVALID_ARG;
    if (transpose != 0 && transpose != 1) return BSMR_ERR_INVALID_ARG;
    const bool reads = bw->nnz != 0;
    if ((reads && (!v_dev || !X16_dev)) || !Y_dev || !aligned4(v_dev) || !aligned16(X16_dev) || !aligned16(Y_dev))
        return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, workFloatsFor(bw, K, num_batches, bw->permuteV && transpose))) return st;
    return runSpmm(bw, K, transpose, v_dev, X16_dev, Y_dev, num_batches, static_cast<hipStream_t>(stream), compute_mode);
}

int bsmr_spmm_16(bsmr_backward* bw, uint32_t K, int transpose, const float* v_dev, const void* X16_dev, void* Y16_dev,
                 uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkBackwardCall(bw, K, num_batches)) return st;
    if (compute_mode != BSMR_COMPUTE_F16 && compute_mode != BSMR_COMPUTE_BF16) return BSMR_ERR_INVALID_ARG;
    if (transpose != 0 && transpose != 1) return BSMR_ERR_INVALID_ARG;
    const bool reads = bw->nnz != 0;
    if ((reads && (!v_dev || !X16_dev)) || !Y16_dev || !aligned4(v_dev) || !aligned16(X16_dev) || !aligned16(Y16_dev))
        return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, workFloatsFor(bw, K, num_batches, bw->permuteV && transpose))) return st;
    return runSpmm(bw, K, transpose, v_dev, X16_dev, Y16_dev, num_batches, static_cast<hipStream_t>(stream), compute_mode, true);
}

int bsmr_sddmm_backward_16(bsmr_backward* bw, uint32_t K, const float* dP_dev, const void* A16_dev, const void* B16_dev,
                           void* dA16_dev, void* dB16_dev, uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkBackwardCall(bw, K, num_batches)) return st;
    if (compute_mode != BSMR_COMPUTE_F16 && compute_mode != BSMR_COMPUTE_BF16) return BSMR_ERR_INVALID_ARG;
    const bool reads = bw->nnz != 0;
    if ((reads && !dP_dev) || !aligned4(dP_dev) ||
        (dA16_dev && ((reads && !B16_dev) || !aligned16(B16_dev) || !aligned16(dA16_dev))) ||
        (dB16_dev && ((reads && !A16_dev) || !aligned16(A16_dev) || !aligned16(dB16_dev))))
        return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0 || (!dA16_dev && !dB16_dev)) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, workFloatsFor(bw, K, num_batches, bw->permuteV && dB16_dev))) return st;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (dA16_dev)
        if (int st = runSpmm(bw, K, 0, dP_dev, B16_dev, dA16_dev, num_batches, s, compute_mode, true)) return st;
    if (dB16_dev)
        if (int st = runSpmm(bw, K, 1, dP_dev, A16_dev, dB16_dev, num_batches, s, compute_mode, true)) return st;
    return BSMR_OK;
}

int bsmr_sddmm_backward_mode(bsmr_backward* bw, uint32_t K, const float* dP_dev, const float* A_dev, const float* B_dev,
                             float* dA_dev, float* dB_dev, uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkBackwardCall(bw, K, num_batches)) return st;
    if (!validMode(compute_mode)) return BSMR_ERR_INVALID_ARG;
    if (compute_mode == BSMR_COMPUTE_F32)
        return bsmr_sddmm_backward(bw, K, dP_dev, A_dev, B_dev, dA_dev, dB_dev, num_batches, stream);
    const bool reads = bw->nnz != 0;
    if ((reads && !dP_dev) || !aligned4(dP_dev) || (dA_dev && ((reads && !B_dev) || !aligned16(B_dev) || !aligned16(dA_dev))) ||
        (dB_dev && ((reads && !A_dev) || !aligned16(A_dev) || !aligned16(dB_dev))))
        return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0 || (!dA_dev && !dB_dev)) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    // B is gathered by dA, A by dB: only what a requested product reads is rounded, B16 first, A16 behind it
    const uint64_t nB = reads && dA_dev ? (uint64_t)bw->N * K * num_batches : 0u;
    const uint64_t nA = reads && dB_dev ? (uint64_t)bw->M * K * num_batches : 0u;
    const uint64_t off = lowpOffset(bw, K, num_batches, bw->permuteV && dB_dev);
    if (int st = growWork(bw, off + (nA + nB) / 2u)) return st;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    uint16_t* B16 = reinterpret_cast<uint16_t*>(bw->work + off);
    uint16_t* A16 = B16 + nB;
    if (int st = roundOperands(compute_mode, A_dev, nA, A16, B_dev, nB, B16, s)) return st;
    if (dA_dev)
        if (int st = runSpmm(bw, K, 0, dP_dev, B16, dA_dev, num_batches, s, compute_mode)) return st;
    if (dB_dev)
        if (int st = runSpmm(bw, K, 1, dP_dev, A16, dB_dev, num_batches, s, compute_mode)) return st;
    return BSMR_OK;
}

}  // extern "C"
