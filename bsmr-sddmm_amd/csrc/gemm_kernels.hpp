// Output-stationary GEMM engine of the dense part (round 4) for gfx950: format csrc/gemm_format.hpp.
//
// What it computes is the dense part of the reference's SDDMM (reference src/sddmmKernel.cu:213-351; K loop :274-330,
// masked scatter :331-348): for every stored entry (i, j) that the plan keeps on the dense path, P[e] = sum_k A[i,k] B[k,j],
// fp16 / bf16 operands, fp32 accumulation - bit for bit what convertOperands + denseStream produce (same casts, same MFMA
// instruction, the k steps of an entry accumulated in the same order into one accumulator).
//
// One workgroup = one macro-tile of C: TM = 16 PM reordered rows x TN = 16 NB natural columns, 8 waves as 2 (M) x 4 (N),
// wave (wm, wn) owns the m x n = (PM / 2) x (NB / 4) block of 16 x 16 tiles at rows wm TM / 2, columns wn TN / 4 and keeps
// its accumulators (4 m n registers) for the whole K loop.
//   * K is cut into slices of 64.  A slice of the operands - TM rows of A (gathered by row id: a row is K contiguous
//     elements) and TN columns of the column-major B (contiguous) x 64 k = 128-byte rows - is an LDS STAGE; two stages.
//     Every wave issues its share of a stage's LDS-DMA (buffer_load ... lds, 1 KiB = 8 rows per instruction, no registers):
//     PM / 4 + NB / 4 instructions per wave and slice.  The 16-byte pieces of a row are XOR-swizzled on the SOURCE address
//     (piece ^ ((row >> 1) & 7)), the image itself is lane-linear as LDS-DMA requires; the fragment reads apply the same XOR
//     and are bank-conflict free (a ds_read_b128 is served in groups of 16 lanes: rows 0-3, 12-15 at k-group g and rows
//     4-11 at g + 1 land on 16 different 16-byte slots of the 256-byte bank row).
//   * Per slice and 32-k step a wave reads m + n fragments (ds_read_b128) and issues m n MFMAs (v_mfma_f32_16x16x32): one
//     fragment of A feeds n MFMAs, one of B feeds m (the sweep engine of round 3: at most 4 and 1).  The loads of slice
//     t + 1 are issued at the top of slice t and waited for (this wave's own) behind its MFMAs; ONE workgroup barrier per
//     slice publishes the landed stage and frees the other one.  (What hipcc makes of it, and it is what one wants: the
//     fragment reads of slice t stay in front of the barrier, its MFMAs move behind it - register-only instructions are not
//     ordered by the barrier - and run beside the DMA issue and the fragment reads of slice t + 1.)
//   * Epilogue = the sparse mask: the stages are dead, every wave takes 16 KiB of them as its private slab.  Per pass of 16
//     tiles: accumulators -> slab (ds_write_b128 per tile), then one lane per STORED entry: entry word -> slab value and the
//     row's first index (a table of the macro-tile in LDS) -> one store.  The words of a (wave, pass) list are contiguous
//     and ordered by (row, column): 64 lanes read 256 contiguous bytes and write runs of P.  Entry words are read once per
//     launch, i.e. from HBM: the first trip of a pass (four or eight batches of 64) is requested a pass or two ahead (pass
//     0's with the first stage where the K loop is short, else in front of the last slice's MFMAs), and the passes are
//     shaped so that the waits hipcc counts in front of a trip leave the younger requests and all stores outstanding
//     (gemmMaskPass).
//   * SRC32: the caller's fp32 operands, no conversion pass (K <= 128).  A stage then holds 32 k (rows of 128 bytes again:
//     same DMA shape, K / 32 slices); a fragment is two ds_read_b128 (8 consecutive k as fp32) rounded in registers with the
//     casts of convertOperands, so the MFMA operands - and P - are bit for bit those of conversion pass + 16-bit kernel.
//     The XOR of the 16-byte pieces is another one (a lane's two pieces are neighbours; the 16 lanes a read is served in
//     hold rows 0-3, 12-15 at pieces 2 g, 2 g + 1 and rows 4-11 at 2 g + 2, 2 g + 3): piece ^ swz32(row), below.
// Measured (tools/probes/gemm_probe.hip, MI355X): 4096^2 Bernoulli(0.1), K = 512, bf16: the K loop runs at 1.5 us per slice
// = 1.4 PFLOP/s executed, the rate of the guide's 256^2 8-phase GEMM template on random data; what is left is the fixed
// part (launch, first stage, epilogue).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_format.hpp"
#include "sddmm_kernels.hpp"

namespace bsmr {

constexpr uint32_t kGemmBK = 64;                                   // k per LDS stage (16-bit operands; fp32 operands: 32)
constexpr uint32_t kGemmRowBytes = kGemmBK * 2u;                   // one row / column of a stage: 128 bytes either way
// the XOR that spreads a row's eight 16-byte pieces over the LDS banks, 16-bit and fp32 stages
__host__ __device__ constexpr uint32_t gemmSwz16(uint32_t row) { return (row >> 1) & 7u; }
__host__ __device__ constexpr uint32_t gemmSwz32(uint32_t row) { return ((row >> 1) & 1u) | (((row >> 3) & 1u) * 6u); }
constexpr uint32_t gemmStageBytes(int PM, int NB) { return (uint32_t)(PM + NB) * 16u * kGemmRowBytes; }
constexpr uint32_t kGemmSlabBytes = kGemmPassTiles * 1024u;         // a wave's slab: 16 tiles of 64 lanes x 16 bytes
// two stages, reused as the eight waves' slabs by the epilogue
constexpr uint32_t gemmRingBytes(int PM, int NB) {
    return 2u * gemmStageBytes(PM, NB) > kGemmWaves * kGemmSlabBytes ? 2u * gemmStageBytes(PM, NB) : kGemmWaves * kGemmSlabBytes;
}
constexpr size_t gemmLdsBytes(int PM, int NB) { return gemmRingBytes(PM, NB) + (size_t)PM * 16u * 4u; }

#if defined(BSMR_GEMM_LAB)
// labSkip: bit 0 MFMAs, 1 fragment reads (denseGemmCvt: the rounding step), 2 DMAs, 3 slab writes, 4 entry loads, 5 stores,
// 6 denseGemmCvt's fragment reads.  labStamps (may be null): per (workgroup, wave) ten readings of the 100 MHz clock -
// 0 entry, 1 first stage requested, 2 own share of it landed, 3 first barrier passed, 4 K loop left, 5 + q pass q done;
// denseGemmCvt: 8 = ticks the wave stood at the K loop's waits for its operands (summed over the slices), 9 = ticks from
// the end of that wait to the slice's barrier passed (rounding, re-issue, barrier; summed).
constexpr uint32_t kGemmLabStamps = 10;
#define GEMM_LAB_ARG , uint32_t labSkip, unsigned long long* labStamps
#define GEMM_LAB_SKIP(bit) (labSkip & (1u << (bit)))
#define GEMM_LAB_STAMPS unsigned long long labStamp[kGemmLabStamps] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, labSpan = 0
#define GEMM_LAB_STAMP(i) labStamp[i] = __builtin_amdgcn_s_memrealtime()
#define GEMM_LAB_SPAN_BEGIN labSpan = __builtin_amdgcn_s_memrealtime()
#define GEMM_LAB_SPAN_END(i) labStamp[i] += __builtin_amdgcn_s_memrealtime() - labSpan
#define GEMM_LAB_STAMPS_OUT                                                                              \
    if (labStamps && lane == 0)                                                                          \
        for (uint32_t i = 0; i < kGemmLabStamps; ++i) labStamps[((size_t)blockIdx.x * kGemmWaves + wave) * kGemmLabStamps + i] = labStamp[i]
#else
#define GEMM_LAB_ARG
#define GEMM_LAB_SKIP(bit) false
#define GEMM_LAB_STAMPS
#define GEMM_LAB_STAMP(i)
#define GEMM_LAB_SPAN_BEGIN
#define GEMM_LAB_SPAN_END(i)
#define GEMM_LAB_STAMPS_OUT
#endif

// lab builds: a value that feeds a part left out stays computed (the host pass does not know the register constraint)
__device__ __forceinline__ void gemmKeep(const u32x4& x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" ::"v"(x));
#else
    (void)x;
#endif
}

// The epilogue's dump of one accumulator tile into the wave's slab (gemmSlabSlot: register j of the 64 lanes = the 256 bytes at
// 256 j).  ds_write_addtid_b32 stores 4 bytes per lane at M0[15:0] + offset + 4 lane in 2 cycles per wave-instruction - four of
// them 8 cycles where one ds_write_b128 takes 13 (MI355X_MICROARCH.md, LDS): the slab passes are bound by exactly this
// transfer.  M0 holds 16 bits: tiles at 64 KiB and above (the slabs of waves 4 - 7) are reached through the immediate
// (kGemmDumpHigh + 256 j <= 65532).  One wait state between the write of M0 and its use (the assembler does not see into
// the statement); LDS operations of a wave complete in order, so the entry reads that follow need no wait of their own.
constexpr uint32_t kGemmDumpHigh = 64764u;
__device__ __forceinline__ void gemmDumpTile(const f32x4& a, uint32_t tileAddr, bool high) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
    if (!high)
        asm volatile("s_mov_b32 m0, %4\n\ts_nop 0\n\tds_write_addtid_b32 %0\n\tds_write_addtid_b32 %1 offset:256\n\t"
                     "ds_write_addtid_b32 %2 offset:512\n\tds_write_addtid_b32 %3 offset:768"
                     ::"v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "s"(tileAddr) : "memory", "m0");
    else
        asm volatile("s_mov_b32 m0, %4\n\ts_nop 0\n\tds_write_addtid_b32 %0 offset:64764\n\tds_write_addtid_b32 %1 offset:65020\n\t"
                     "ds_write_addtid_b32 %2 offset:65276\n\tds_write_addtid_b32 %3 offset:65532"
                     ::"v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "s"(tileAddr - kGemmDumpHigh) : "memory", "m0");
#pragma clang diagnostic pop
#else
    (void)a; (void)tileAddr; (void)high;
#endif
}
// LDS byte address of a pointer into the dynamic allocation
__device__ __forceinline__ uint32_t gemmLdsAddress(const void* p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}

// This wave's share of one stage: ADMAS + BDMAS LDS-DMA instructions of 1 KiB (8 rows of 128 bytes), voff = the lane's
// byte offset of its piece in slice 0, kOff = the slice's byte offset inside a row.  (A function of its own: a buffer
// resource cannot be captured by a lambda of a kernel that the host pass instantiates too.)
template <uint32_t DMAS>
__device__ __forceinline__ void gemmStagePart(const uint8_t* src, uint32_t srcBytes, uint8_t* dst, uint32_t wave, const uint32_t* voff, uint32_t kOff) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(src), 0, srcBytes, 0x00020000);
#pragma unroll
    for (uint32_t j = 0; j < DMAS; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(dst + (wave * DMAS + j) * 1024u), 16, voff[j], kOff, 0, 0);
}
// The epilogue's store of one entry: a buffer store whose byte offset is out of range for the lanes without an entry (the
// hardware drops those), so that the pass is straight-line code.  Under `if (entry) P[dst] = val` every batch of 64 entries
// was a branch around a store: the compiler could not count the stores between a batch of entry words and its use any
// more, waited with vmcnt(2), (1), (0) for words that had landed long before - and with them for the acknowledgements of
// the stores issued in between (stores and loads share the counter on gfx9).
__device__ __forceinline__ void gemmStoreEntry(float* P, bool live, uint32_t index, float val) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(P, 0, 0xFFFFFFFC, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, val), rsrc, live ? index << 2 : 0xFFFFFFFFu, 0, 0);
}
// ---- the mask pass, shared by denseGemm and denseGemmCvt
// A TRIP is C batches of 64 entry words (C = 4 where the accumulators leave few registers, else 8).  Reads past a list stay
// inside `words`: a trip is requested at most one trip past the end of a list, and kGemmWordSlack covers two trips of 512.
template <uint32_t C>
__device__ __forceinline__ void gemmLoadWords(const uint32_t* __restrict__ words, uint32_t e0, uint32_t lane, uint32_t (&w)[C], bool skip) {
    // (e0 is wave-uniform: a scalar base, the lane's offset - one register for every request of the kernel - and an immediate)
    const uint32_t* __restrict__ base = words + e0;
#pragma unroll
    for (uint32_t u = 0; u < C; ++u) w[u] = skip ? kGemmNoEntry : base[u * kWave + lane];
}
// One trip: the words of list positions e .. e + 64 C - 1 (the list ends at `last`), one lane per stored entry: slab value and
// the row's first index -> one store.  Straight-line: the 2 C LDS reads go out together, the C stores back to back.  (A
// padding word - and any word past the list - reads slot <= 4095 and row <= HALF - 1: inside the slab and the table.)
template <uint32_t C, uint32_t HALF>
__device__ __forceinline__ void gemmMaskTrip(const float* slab, const uint32_t* rowTable, float* P, uint32_t e, uint32_t last, uint32_t lane,
                                             const uint32_t (&w)[C], bool skipStores) {
#pragma unroll
    for (uint32_t u = 0; u < C; ++u) {
        const bool live = e + u * kWave + lane < last && w[u] != kGemmNoEntry;
        const float val = slab[w[u] & 4095u];
        const uint32_t dst = rowTable[(w[u] >> 12) & (HALF - 1u)] + (w[u] >> 19);
        if (!skipStores) gemmStoreEntry(P, live, dst, val);
    }
}
// Pass q of a wave over words[myList[q] .. myList[q + 1]).  Its first trip's words are in wAhead[q & 1], requested a pass or
// more ago (DEEP: two passes ahead, where the registers allow it); the first trip of the pass that takes these registers
// next is requested here, before anything of this pass is used.  What this shape is for is the waits hipcc counts in
// front of the first trip.  Loads and stores share one in-order counter (vmcnt), so "the words have landed" can only be
// said as "at most N younger operations are outstanding", and only where the compiler can count them:
//   * the first trip is peeled out of the loop and issued unconditionally (an empty list issues C out-of-range stores).
//     Inside `for (e = first; ...) { if (e != first) load(w); ... }` the registers of `w` were carried round the loop, the
//     first trip's wait was merged with a later trip's - where `w` is the youngest load - and every pass began with
//     vmcnt(0): a full round trip for the next pass's words requested four instructions earlier, and the drain of
//     every store of the pass before;
//   * a list longer than one trip requests its second trip BEFORE the first trip's first use, and the overflow loop requests
//     trip t + 1 before it works on trip t, so that no trip's words are waited for behind the stores just issued.
template <uint32_t C, uint32_t HALF, uint32_t Q, bool DEEP>
__device__ __forceinline__ void gemmMaskPass(const uint32_t* __restrict__ words, const float* slab, const uint32_t* rowTable, float* P,
                                             const uint32_t (&myList)[Q + 1u], uint32_t q, uint32_t lane, uint32_t (&wAhead)[2][C],
                                             bool skipLoads, bool skipStores) {
    const uint32_t first = myList[q], last = myList[q + 1u];
    uint32_t w[C];
#pragma unroll
    for (uint32_t u = 0; u < C; ++u) w[u] = wAhead[q & 1u][u];
    if (DEEP) {
        if (q + 2u < Q) gemmLoadWords<C>(words, myList[q + 2u], lane, wAhead[q & 1u], skipLoads);
    } else if (q + 1u < Q) {
        gemmLoadWords<C>(words, last, lane, wAhead[(q + 1u) & 1u], skipLoads);   // (lists follow each other)
    }
    constexpr uint32_t T = C * kWave;
    const bool more = first + T < last;   // (wave-uniform)
    uint32_t over[C];
    if (more) gemmLoadWords<C>(words, first + T, lane, over, skipLoads);
    gemmMaskTrip<C, HALF>(slab, rowTable, P, first, last, lane, w, skipStores);
    if (more) {
        // (the request stands at the top of the body and its registers are copied at the bottom, with nothing conditional in
        // between: written as two register sets and a body unrolled by two, hipcc sank each request below the loop's exit
        // test, i.e. back to where the words are needed)
        for (uint32_t e = first + T; e < last; e += T) {
            uint32_t ahead[C];
            gemmLoadWords<C>(words, e + T, lane, ahead, skipLoads);
            gemmMaskTrip<C, HALF>(slab, rowTable, P, e, last, lane, over, skipStores);
#pragma unroll
            for (uint32_t u = 0; u < C; ++u) over[u] = ahead[u];
        }
    }
}
template <uint32_t ADMAS, uint32_t BDMAS>
__device__ __forceinline__ void gemmStage(const uint8_t* A, uint32_t aBytes, const uint8_t* B, uint32_t bBytes, uint8_t* stage, uint32_t bAt,
                                          uint32_t wave, const uint32_t* voffA, const uint32_t* voffB, uint32_t kOff) {
    gemmStagePart<BDMAS>(B, bBytes, stage + bAt, wave, voffB, kOff);
    gemmStagePart<ADMAS>(A, aBytes, stage, wave, voffA, kOff);
}
// Row id of this lane's row in a chunk of 8 rows whose ids lie at `rows8` (a wave-uniform address), written as eight loads of
// uniform addresses and a select.  hipcc does not keep them scalar: it folds the select into the address and emits ONE
// global_load_dword per chunk at rows8 + 4 sub.  denseGemm issues them all before the first DMA and waits for each chunk's
// ids with a counted vmcnt in front of its DMA, so no DMA waits for ids it does not need, and no id waits for a DMA.
// denseGemmCvt<4, 16, 20, 0>: nine, four for the A rows and five for the B columns, beside the row table's word; the
// fence in front of its first operand request makes them all land (vmcnt(8) .. (0)) before that request goes out.
__device__ __forceinline__ uint32_t gemmRowOfLane(const uint32_t* __restrict__ rows8, uint32_t sub) {
    uint32_t id = rows8[0];
#pragma unroll
    for (uint32_t k = 1; k < 8; ++k) id = sub == k ? rows8[k] : id;
    return id;
}

// grid: numItems x batches.  gridG / gridS: row groups / column strips of the format; fullGrid != 0: every macro-tile is an
// item and item i's place follows from i alone (gemmItemPlace), so nothing waits for the item record.
// KT: slices of K (64 k each on 16-bit operands, 32 k each on fp32 operands).
template <int KT, int PM, int NB, int MODE, bool SRC32 = false>
__global__ void __launch_bounds__(kGemmWaves * kWave, 2)
denseGemm(const void* __restrict__ Aop, const void* __restrict__ Bop, uint32_t aBytes, uint32_t bBytes,
          const uint32_t* __restrict__ panelRows, const uint32_t* __restrict__ colOf, const GemmItem* __restrict__ items,
          const uint32_t* __restrict__ rowStart,
          const uint32_t* __restrict__ lists, const uint32_t* __restrict__ words, float* __restrict__ P, uint32_t N,
          uint32_t gridG, uint32_t gridS, uint32_t fullGrid, Batch batch GEMM_LAB_ARG) {
    constexpr uint32_t ESZ = SRC32 ? 4u : 2u, K = (kGemmRowBytes / ESZ) * KT, TM = PM * 16u, TN = NB * 16u;
    constexpr uint32_t KSUB = SRC32 ? 1u : 2u;                                  // 32-k MFMA steps per slice
    constexpr uint32_t m = PM / kGemmWavesM, n = NB / kGemmWavesN, Q = (m * n + kGemmPassTiles - 1u) / kGemmPassTiles, L = kGemmWaves * Q;
    constexpr uint32_t ADMAS = PM / 4u, BDMAS = NB / 4u;                        // LDS-DMA instructions per wave and slice
    static_assert(PM % 4 == 0 && NB % 4 == 0, "a stage is filled in whole 1-KiB pieces per wave");
    constexpr uint32_t stageBytes = gemmStageBytes(PM, NB), bAt = TM * kGemmRowBytes;
    constexpr uint32_t rowTableAt = gemmRingBytes(PM, NB);
    // batches of 64 entry words requested together (fewer where the accumulators leave few registers)
    constexpr uint32_t kGemmWordChunk = m * n > 32u ? 4u : 8u;
    // how the epilogue dumps the accumulators (below): the 8 x 5 tile blocks of this kernel keep to plain 4-byte stores
    constexpr bool kPlainDump = m * n > 32u;

    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t itemId = xcdContiguous(blockIdx.x, gridDim.x);
    uint32_t group, firstBlock, listBase;
    if (fullGrid) {
        gemmItemPlace(itemId, gridG, gridS, group, firstBlock);
        firstBlock *= (uint32_t)NB;
        listBase = itemId * (L + 1u);
    } else {
        const GemmItem item = items[itemId];
        group = item.group;
        firstBlock = item.firstBlock;
        listBase = item.listBase;
    }
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t wm = wave / kGemmWavesN, wn = wave % kGemmWavesN;
    const uint32_t r = lane & 15u, g = lane >> 4;
    GEMM_LAB_STAMPS;
    GEMM_LAB_STAMP(0);

    const uint8_t* Ab = static_cast<const uint8_t*>(Aop) + (size_t)blockIdx.y * batch.strideA * ESZ;
    const uint8_t* Bb = static_cast<const uint8_t*>(Bop) + (size_t)blockIdx.y * batch.strideB * ESZ;
    P += (size_t)blockIdx.y * batch.strideP;

    // my pieces of a stage: DMA instruction i = wave * DMAS + j moves rows 8 i .. 8 i + 7, lane l the 16-byte slot l & 7 of
    // row 8 i + (l >> 3); the piece that belongs in that slot is slot ^ swz(row)
    uint32_t voffA[ADMAS], voffB[BDMAS];
#pragma unroll
    for (uint32_t j = 0; j < BDMAS; ++j) {
        const uint32_t col = 8u * (wave * BDMAS + j) + (lane >> 3);
        const uint32_t id = gemmRowOfLane(colOf + (size_t)firstBlock * 16u + 8u * (wave * BDMAS + j), lane >> 3);   // the column in this slot
        voffB[j] = id * (K * ESZ) + (((lane & 7u) ^ (SRC32 ? gemmSwz32(col) : gemmSwz16(col))) << 4);
    }
    if (!GEMM_LAB_SKIP(2)) gemmStagePart<BDMAS>(Bb, bBytes, lds + bAt, wave, voffB, 0u);
#pragma unroll
    for (uint32_t j = 0; j < ADMAS; ++j) {
        const uint32_t row = 8u * (wave * ADMAS + j) + (lane >> 3);
        const uint32_t id = gemmRowOfLane(panelRows + (size_t)group * TM + 8u * (wave * ADMAS + j), lane >> 3);
        voffA[j] = id * (K * ESZ) + (((lane & 7u) ^ (SRC32 ? gemmSwz32(row) : gemmSwz16(row))) << 4);
    }
    if (!GEMM_LAB_SKIP(2)) gemmStagePart<ADMAS>(Ab, aBytes, lds, wave, voffA, 0u);
    GEMM_LAB_STAMP(1);
    // the macro-tile's table of first indices, one row per thread
    if (threadIdx.x < TM) reinterpret_cast<uint32_t*>(lds + rowTableAt)[threadIdx.x] = rowStart[(size_t)itemId * TM + threadIdx.x];
    // entry lists of this wave: words[myList[q] .. myList[q + 1]) is pass q's
    uint32_t myList[Q + 1];
#pragma unroll
    for (uint32_t q = 0; q <= Q; ++q) myList[q] = lists[listBase + wave * Q + q];

    // fragment addresses: row / column r of a tile, k-group g.  16-bit: piece 4 s + g of the 128-byte row sits at slot
    // (4 s + g) ^ (r >> 1) (s = 1 is s = 0's address ^ 64).  fp32: pieces 2 g and 2 g + 1 at (2 g) ^ swz32(r) and that ^ 1.
    const uint32_t fragOff = r * kGemmRowBytes + ((SRC32 ? (2u * g) ^ gemmSwz32(r) : g ^ gemmSwz16(r)) << 4);
    const uint32_t aRead = wm * (TM / 2u) * kGemmRowBytes + fragOff;
    const uint32_t bRead = bAt + wn * (TN / 4u) * kGemmRowBytes + fragOff;

    f32x4 acc[m][n];
#pragma unroll
    for (uint32_t i = 0; i < m; ++i)
#pragma unroll
        for (uint32_t j = 0; j < n; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // entry words, a trip of kGemmWordChunk batches of 64 at a time
    auto loadWords = [&](uint32_t e0, uint32_t (&w)[kGemmWordChunk]) { gemmLoadWords<kGemmWordChunk>(words, e0, lane, w, GEMM_LAB_SKIP(4)); };
    // the first words of the passes' lists are requested two passes ahead where the registers allow it (a pass is shorter
    // than the words' way from HBM: 0.1-0.2 us per launch at 256 x 256; the 8 x 5 tile blocks have no registers left for
    // it - 3 to 8 spilled, 0.25 us lost - and stay one pass ahead)
    constexpr bool kDeepWords = Q >= 2u && m * n <= 32u;
    uint32_t wAhead[2][kGemmWordChunk];
    // pass 0's first entry words: an HBM round trip (they are read once per launch).  A short K loop does not cover it from
    // the top of its last slice, so up to four slices request them before the loop and carry the registers through it - as
    // soon as the list bounds are known: in front of the wait for the first stage, whose round trip they share.  (Requested
    // behind the first barrier they stood right in front of slice 0's vmcnt(0), below which hipcc sinks that slice's
    // MFMAs: the K loop waited for words the epilogue needs KT slices later.  BSMR_GEMM_LATE_WORDS: lab, that form.)
    constexpr bool kEarlyWords = KT <= 4 && !kPlainDump;
    auto firstWords = [&]() {
        loadWords(myList[0], wAhead[0]);
        if (kDeepWords) loadWords(myList[1], wAhead[1]);
    };
#if !defined(BSMR_GEMM_LATE_WORDS)
    if (kEarlyWords) firstWords();
#endif

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    GEMM_LAB_STAMP(2);
    __builtin_amdgcn_s_barrier();
    GEMM_LAB_STAMP(3);
#if defined(BSMR_GEMM_LATE_WORDS)
    if (kEarlyWords) firstWords();
#endif

#pragma unroll
    for (uint32_t t = 0; t < (uint32_t)KT; ++t) {
        if (t + 1u < (uint32_t)KT && !GEMM_LAB_SKIP(2))   // slice t + 1 -> the other stage
            gemmStage<ADMAS, BDMAS>(Ab, aBytes, Bb, bBytes, lds + ((t + 1u) & 1u) * stageBytes, bAt, wave, voffA, voffB, (t + 1u) * kGemmRowBytes);
        if (!kEarlyWords && t + 1u == (uint32_t)KT) firstWords();   // ... a long loop: behind its last slice's DMAs
        const uint8_t* base = lds + (t & 1u) * stageBytes;
#pragma unroll
        for (uint32_t s = 0; s < KSUB; ++s) {
            // fragment of row / column tile `tile` at base address `at`: 16-bit operands as they lie; fp32 operands rounded here
            auto fragment = [&](uint32_t at, uint32_t tile, uint32_t tag) -> u32x4 {
                if (GEMM_LAB_SKIP(1)) return u32x4{lane, t, tile, s + tag};
                const uint8_t* src = base + ((at + tile * 16u * kGemmRowBytes) ^ (s << 6));
                if constexpr (SRC32) {
                    const f32x4 lo = *reinterpret_cast<const f32x4*>(src);
                    const f32x4 hi = *reinterpret_cast<const f32x4*>(reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(src) ^ 16u));
                    return packLowp<MODE>(lo, hi);
                } else {
                    return *reinterpret_cast<const u32x4*>(src);
                }
            };
            u32x4 bf[n];
#pragma unroll
            for (uint32_t j = 0; j < n; ++j) bf[j] = fragment(bRead, j, 0u);
#pragma unroll
            for (uint32_t i = 0; i < m; ++i) {
                const u32x4 af = fragment(aRead, i, 2u);
                if (!GEMM_LAB_SKIP(0)) {
#pragma unroll
                    for (uint32_t j = 0; j < n; ++j) acc[i][j] = mfma16<MODE>(af, bf[j], acc[i][j]);
                } else {
                    gemmKeep(af);
#pragma unroll
                    for (uint32_t j = 0; j < n; ++j) gemmKeep(bf[j]);
                }
            }
        }
        // slice t + 1 has landed (this wave's pieces), everybody has read slice t: the stages change roles
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    // ---- the sparse mask: slab passes over the wave's tiles
    GEMM_LAB_STAMP(4);
    float* slab = reinterpret_cast<float*>(lds) + wave * (kGemmPassTiles * 256u);
    const uint32_t slabAddr = __builtin_amdgcn_readfirstlane(gemmLdsAddress(slab));
    const uint32_t* rowTable = reinterpret_cast<const uint32_t*>(lds + rowTableAt) + wm * (TM / 2u);
#pragma unroll
    for (uint32_t q = 0; q < Q; ++q) {
        if (!GEMM_LAB_SKIP(3)) {
            if (kPlainDump) {
                // (the two forms of the ds_write_addtid dump below, laid out one after the other, cost the 8 x 5 tile blocks of
                // this kernel 5 to 14 spilled registers - 256 x 320 at K = 512: 21.5 us against 20.3 with one plain 4-byte
                // store per register, which keeps the slab's layout; denseGemmCvt has the registers)
#pragma unroll
                for (uint32_t tp = 0; tp < kGemmPassTiles; ++tp) {
                    const uint32_t tIdx = q * kGemmPassTiles + tp;
                    if (tIdx < m * n) {
#pragma unroll
                        for (uint32_t j = 0; j < 4u; ++j) slab[tp * 256u + j * 64u + lane] = acc[tIdx / n][tIdx % n][j];
                    }
                }
            } else if (slabAddr < 0x10000u) {
#pragma unroll
                for (uint32_t tp = 0; tp < kGemmPassTiles; ++tp) {
                    const uint32_t tIdx = q * kGemmPassTiles + tp;
                    if (tIdx < m * n) gemmDumpTile(acc[tIdx / n][tIdx % n], slabAddr + tp * 1024u, false);
                }
            } else {
#pragma unroll
                for (uint32_t tp = 0; tp < kGemmPassTiles; ++tp) {
                    const uint32_t tIdx = q * kGemmPassTiles + tp;
                    if (tIdx < m * n) gemmDumpTile(acc[tIdx / n][tIdx % n], slabAddr + tp * 1024u, true);
                }
            }
        }
        // (the plain dump is ordinary code: without a fence hipcc's scheduler moves the pass's requests and LDS reads up
        // between its stores, and the longer live ranges cost these 8 x 5 tile blocks 12 to 28 bytes of scratch at KT = 2 / 4 -
        // whose reloads count on vmcnt and were waited for with vmcnt(0) in front of the first trip)
        if (kPlainDump) __builtin_amdgcn_sched_barrier(0);
        gemmMaskPass<kGemmWordChunk, TM / 2u, Q, kDeepWords>(words, slab, rowTable, P, myList, q, lane, wAhead, GEMM_LAB_SKIP(4), GEMM_LAB_SKIP(5));
        GEMM_LAB_STAMP(5u + q);
    }
    GEMM_LAB_STAMPS_OUT;
}

// ---------------------------------------------------------------------------------------------------------------------
// The same macro-tile kernel on the caller's fp32 operands with ONE shared rounding per element (K = 64, 128).
//
// denseGemm<..., SRC32> lets every wave round the fragments it reads: the four waves of a row half round the same rows of A,
// the two waves of a column quarter the same columns of B - 2.9 times the casts the operands need, all of them in front of
// the MFMAs of an in-order wave (measured, nips-like K = 128: 13.4 us against 9.1 us for the kernel on 16-bit copies).  Here
// a slice of 32 k is rounded once, by the wave that requested it, into a 16-bit LDS image:
//   A  a wave's PM / 4 chunks of 8 rows x 128 bytes come into REGISTERS (buffer loads through the resource that bounds
//      them as it bounded the DMAs: 4 registers per chunk, lane l = piece l & 7 of row l >> 3) and are rounded from there;
//   F  B's fp32 image, TWO stages of TN rows x 128 bytes, filled by LDS-DMA, lane-linear (piece = slot: nothing reads it
//      by fragment).  A wave's share of F is PRIVATE to it: the wave that issued the DMAs of a 1-KiB chunk is the one
//      that rounds it, so its own counted wait orders everything and no barrier guards F;
//   H  two stages of (TM + TN) rows x 64 bytes of fp16 / bf16 (rows of 32 k), written by the rounding step - 64 lanes take
//      1 KiB of a slice (registers or F, read linearly), round with the casts of convertOperands, write 8 bytes each - and
//      read as MFMA fragments (ds_read_b128 of piece g of row r at slot g ^ swzH(r): conflict-free for the 16-lane groups
//      a read is served in, as are the 8-byte writes).
// Requests run two slices ahead.  vmcnt is ONE in-order counter, so the order of issue is part of the design: at the end
// of slice t a wave requests A(t + 2), THEN B(t + 3); behind the MFMAs of slice t + 1 it waits with vmcnt(NB / 4) - A(t + 2)
// and everything older, B(t + 2) with it, have landed, the DMAs of B(t + 3) stay outstanding - rounds both into
// H[t & 1] and re-issues.  (A second fp32 stage for A too does not fit: 2 x 72 + 72 KiB at 256 x 320.)  ONE barrier per
// slice publishes H[(t + 1) & 1]; everybody's reads of it, two slices ago, ended before the barrier in between.  Same
// casts, same MFMA, same order of k steps: bit-identical to the conversion pass + 16-bit kernels.
constexpr uint32_t kGemmHalfRowBytes = 64u;                        // a row of an H stage: 32 k of 16 bits
__host__ __device__ constexpr uint32_t gemmSwzH(uint32_t row) { return (4u - ((row >> 2) & 3u)) & 3u; }   // 0, 3, 2, 1
// two fp32 stages of B, two 16-bit stages of both operands; reused as the eight waves' slabs by the epilogue
constexpr uint32_t gemmCvtRingBytes(int PM, int NB) {
    const uint32_t used = 2u * (uint32_t)NB * 16u * kGemmRowBytes + 2u * (uint32_t)(PM + NB) * 16u * kGemmHalfRowBytes;
    return used > kGemmWaves * kGemmSlabBytes ? used : kGemmWaves * kGemmSlabBytes;
}
constexpr size_t gemmCvtLdsBytes(int PM, int NB) { return gemmCvtRingBytes(PM, NB) + (size_t)PM * 16u * 4u; }
static_assert(gemmCvtLdsBytes(16, 20) <= 160u * 1024u && gemmCvtLdsBytes(16, 16) <= 160u * 1024u && gemmCvtLdsBytes(8, 20) <= 160u * 1024u &&
              gemmCvtLdsBytes(8, 16) <= 160u * 1024u, "the fp32 kernel's LDS fits a CU's 160 KiB");

// A wave's chunks of an A slice into registers: the addresses (voff, kOff) and the bounds (the buffer resource over the
// caller's aBytes: a piece that does not lie inside reads as zero) of the LDS-DMA form, gemmStagePart.
template <uint32_t CHUNKS>
__device__ __forceinline__ void gemmLoadChunks(const uint8_t* src, uint32_t srcBytes, const uint32_t* voff, uint32_t kOff, f32x4 (&v)[CHUNKS]) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(src), 0, srcBytes, 0x00020000);
#pragma unroll
    for (uint32_t j = 0; j < CHUNKS; ++j) v[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff[j], kOff, 0));
}
// "at most N of my younger requests are outstanding" (N is part of the instruction).  The registers the wait is for pass
// through it: their casts are register-only, and instruction selection placed those of the K = 64 instances in front of the
// fence and the wait, right behind the slice's first MFMA, with hipcc's own vmcnt(3) .. (0) - the wave stood there.
template <uint32_t N, uint32_t CHUNKS>
__device__ __forceinline__ void gemmWaitRequests(f32x4 (&landed)[CHUNKS]) {
    static_assert(N < 64u, "vmcnt holds six bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (uint32_t j = 0; j < CHUNKS; ++j) asm volatile("" : "+v"(landed[j]));
#endif
}
// four fp32 of a row -> 8 bytes of an H stage, the casts of convertOperands
template <int MODE>
__device__ __forceinline__ void gemmRoundPiece(const f32x4& v, uint8_t* dst) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 h;
    if constexpr (MODE == 0) {
        typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
        f16x4 o;
        o[0] = (_Float16)v[0]; o[1] = (_Float16)v[1]; o[2] = (_Float16)v[2]; o[3] = (_Float16)v[3];
        h = __builtin_bit_cast(u32x2, o);
    } else {
        typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
        bf16x4 o;
        o[0] = (__bf16)v[0]; o[1] = (__bf16)v[1]; o[2] = (__bf16)v[2]; o[3] = (__bf16)v[3];
        h = __builtin_bit_cast(u32x2, o);
    }
    *reinterpret_cast<u32x2*>(dst) = h;
}

template <int KT, int PM, int NB, int MODE>
__global__ void __launch_bounds__(kGemmWaves * kWave, 2)
denseGemmCvt(const float* __restrict__ Aop, const float* __restrict__ Bop, uint32_t aBytes, uint32_t bBytes,
             const uint32_t* __restrict__ panelRows, const uint32_t* __restrict__ colOf, const GemmItem* __restrict__ items,
             const uint32_t* __restrict__ rowStart,
             const uint32_t* __restrict__ lists, const uint32_t* __restrict__ words, float* __restrict__ P, uint32_t N,
             uint32_t gridG, uint32_t gridS, uint32_t fullGrid, Batch batch GEMM_LAB_ARG) {
    constexpr uint32_t K = 32u * KT, TM = PM * 16u, TN = NB * 16u, ROWS = TM + TN;
    constexpr uint32_t m = PM / kGemmWavesM, n = NB / kGemmWavesN, Q = (m * n + kGemmPassTiles - 1u) / kGemmPassTiles, L = kGemmWaves * Q;
    constexpr uint32_t ADMAS = PM / 4u, BDMAS = NB / 4u;   // 1-KiB chunks of a slice per wave, 8 rows each: A's (registers), B's (F)
    constexpr uint32_t fBytes = TN * kGemmRowBytes, hBytes = ROWS * kGemmHalfRowBytes, bAtH = TM * kGemmHalfRowBytes;
    constexpr uint32_t hAt = 2u * fBytes, rowTableAt = gemmCvtRingBytes(PM, NB);
    static_assert(hAt + 2u * hBytes <= rowTableAt, "F's two stages and H's two lie in front of the row table");
    constexpr uint32_t kGemmWordChunk = m * n > 32u ? 4u : 8u;

    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t itemId = xcdContiguous(blockIdx.x, gridDim.x);
    uint32_t group, firstBlock, listBase;
    if (fullGrid) {
        gemmItemPlace(itemId, gridG, gridS, group, firstBlock);
        firstBlock *= (uint32_t)NB;
        listBase = itemId * (L + 1u);
    } else {
        const GemmItem item = items[itemId];
        group = item.group;
        firstBlock = item.firstBlock;
        listBase = item.listBase;
    }
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t wm = wave / kGemmWavesN, wn = wave % kGemmWavesN;
    const uint32_t r = lane & 15u, g = lane >> 4;
    GEMM_LAB_STAMPS;
    GEMM_LAB_STAMP(0);
    const uint8_t* Ab = reinterpret_cast<const uint8_t*>(Aop) + (size_t)blockIdx.y * batch.strideA * 4u;
    const uint8_t* Bb = reinterpret_cast<const uint8_t*>(Bop) + (size_t)blockIdx.y * batch.strideB * 4u;
    P += (size_t)blockIdx.y * batch.strideP;

    // my chunks of a slice: chunk c = wave * ADMAS + j of A (wave * BDMAS + j of B) holds rows 8 c .. 8 c + 7, lane l the piece
    // l & 7 (k = 4 (l & 7) .. + 3) of row 8 c + (l >> 3); where the rounded piece goes in H: row * 64 + 16 (slot) + 8 (half)
    uint32_t voffA[ADMAS], voffB[BDMAS];
    const uint32_t piece = lane & 7u;
#pragma unroll
    for (uint32_t j = 0; j < ADMAS; ++j)
        voffA[j] = gemmRowOfLane(panelRows + (size_t)group * TM + 8u * (wave * ADMAS + j), lane >> 3) * (K * 4u) + (piece << 4);
#pragma unroll
    for (uint32_t j = 0; j < BDMAS; ++j)
        voffB[j] = gemmRowOfLane(colOf + (size_t)firstBlock * 16u + 8u * (wave * BDMAS + j), lane >> 3) * (K * 4u) + (piece << 4);
    // (the row table's words are asked for in front of the operands: whoever uses them then waits for nothing younger)
    uint32_t myRowStart = 0;
    if (threadIdx.x < TM) myRowStart = rowStart[(size_t)itemId * TM + threadIdx.x];
    // The requests of a slice, A's THEN B's (header): the fences keep hipcc's scheduler from moving the DMAs in front of the
    // register loads, after which its own wait for the registers would be a wait for the youngest DMAs too.
    f32x4 aNext[ADMAS];
#pragma unroll
    for (uint32_t j = 0; j < ADMAS; ++j) aNext[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto requestA = [&](uint32_t slice) {
        __builtin_amdgcn_sched_barrier(0);
        if (slice < (uint32_t)KT && !GEMM_LAB_SKIP(2)) gemmLoadChunks<ADMAS>(Ab, aBytes, voffA, slice * kGemmRowBytes, aNext);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto requestB = [&](uint32_t slice) {   // into F's stage slice & 1
        __builtin_amdgcn_sched_barrier(0);
        if (slice < (uint32_t)KT && !GEMM_LAB_SKIP(2)) gemmStagePart<BDMAS>(Bb, bBytes, lds + (slice & 1u) * fBytes, wave, voffB, slice * kGemmRowBytes);
        __builtin_amdgcn_sched_barrier(0);
    };
    requestA(0u);
    requestB(0u);
    GEMM_LAB_STAMP(1);
    uint32_t myList[Q + 1];
#pragma unroll
    for (uint32_t q = 0; q <= Q; ++q) myList[q] = lists[listBase + wave * Q + q];

    // rounding step: my chunks of a slice -> stage `to` of H.  B's reads of F are issued together, A's registers are rounded
    // while they are on their way, then B's: written chunk by chunk (read, round, write, read ...) every read waited for the
    // write in front of it - the compiler cannot know that F and H do not overlap.
    // (addresses: a chunk's place in F is one register plus j KiB + the stage; its rows' places in H are two registers per
    // operand - the swizzle of row 8 c + (lane >> 3) depends on c's parity only - plus j * 512 + the stage)
    const uint32_t fOfB = wave * BDMAS * 1024u + lane * 16u;
    auto hOf = [&](uint32_t part, uint32_t firstChunk, uint32_t odd) {
        const uint32_t quarter = (2u * (firstChunk + odd) + (lane >> 5)) & 3u;            // (row >> 2) & 3 of the lane's row
        return hAt + part + firstChunk * 512u + (lane >> 3) * kGemmHalfRowBytes + (((piece >> 1) ^ ((4u - quarter) & 3u)) << 4) + ((piece & 1u) << 3);
    };
    const uint32_t hOfA[2] = {hOf(0u, wave * ADMAS, 0u), hOf(0u, wave * ADMAS, 1u)};
    const uint32_t hOfB[2] = {hOf(bAtH, wave * BDMAS, 0u), hOf(bAtH, wave * BDMAS, 1u)};
    auto roundChunks = [&](uint32_t slice) {
        if (GEMM_LAB_SKIP(1)) return;
        const uint32_t to = (slice & 1u) * hBytes;
        f32x4 v[BDMAS];
#pragma unroll
        for (uint32_t j = 0; j < BDMAS; ++j) v[j] = *reinterpret_cast<const f32x4*>(lds + (slice & 1u) * fBytes + fOfB + j * 1024u);
#pragma unroll
        for (uint32_t j = 0; j < ADMAS; ++j) gemmRoundPiece<MODE>(aNext[j], lds + hOfA[j & 1u] + j * 512u + to);
#pragma unroll
        for (uint32_t j = 0; j < BDMAS; ++j) gemmRoundPiece<MODE>(v[j], lds + hOfB[j & 1u] + j * 512u + to);
    };

    // fragment addresses in an H stage: piece g of row / column r at slot g ^ swzH(r)
    const uint32_t fragOff = r * kGemmHalfRowBytes + ((g ^ gemmSwzH(r)) << 4);
    const uint32_t aRead = wm * (TM / 2u) * kGemmHalfRowBytes + fragOff;
    const uint32_t bRead = bAtH + wn * (TN / 4u) * kGemmHalfRowBytes + fragOff;

    f32x4 acc[m][n];
#pragma unroll
    for (uint32_t i = 0; i < m; ++i)
#pragma unroll
        for (uint32_t j = 0; j < n; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // entry words as in denseGemm: pass 0's first trip rides along with the first stage's round trip where the loop is short
    // (not in the 8 x 5 tile blocks: with A's 16 registers carried through the MFMAs the four words were spilled, and a
    // spill's store and reload count on vmcnt; they request them at the top of the last slice)
    auto loadWords = [&](uint32_t e0, uint32_t (&w)[kGemmWordChunk]) { gemmLoadWords<kGemmWordChunk>(words, e0, lane, w, GEMM_LAB_SKIP(4)); };
    constexpr bool kDeepWords = Q >= 2u && m * n <= 32u;
    uint32_t wAhead[2][kGemmWordChunk];
    constexpr bool kEarlyWords = KT <= 4 && m * n <= 32u;
    auto firstWords = [&]() {
        loadWords(myList[0], wAhead[0]);
        if (kDeepWords) loadWords(myList[1], wAhead[1]);
    };
#if !defined(BSMR_GEMM_LATE_WORDS)
    if (kEarlyWords) firstWords();
#endif

    // slice 0: B(1) requested behind the entry words, so that the wait below leaves nothing but B(1) outstanding; A(0) and
    // B(0) landed (my chunks), rounded into H[0]; A(1), then B(2) requested; H[0] published
    requestB(1u);
    if (KT > 1) gemmWaitRequests<BDMAS>(aNext); else gemmWaitRequests<0>(aNext);
    GEMM_LAB_STAMP(2);
    if (threadIdx.x < TM) reinterpret_cast<uint32_t*>(lds + rowTableAt)[threadIdx.x] = myRowStart;   // (read behind the K loop's barriers)
    roundChunks(0u);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    requestA(1u);
    requestB(2u);
    __builtin_amdgcn_s_barrier();
    GEMM_LAB_STAMP(3);
#if defined(BSMR_GEMM_LATE_WORDS)
    if (kEarlyWords) firstWords();
#endif

#pragma unroll
    for (uint32_t t = 0; t < (uint32_t)KT; ++t) {
        if (!kEarlyWords && t + 1u == (uint32_t)KT) {   // (fenced: hipcc sank the requests behind the slice's MFMAs)
            firstWords();
            __builtin_amdgcn_sched_barrier(0);
        }
        const uint8_t* base = lds + hAt + (t & 1u) * hBytes;
        u32x4 bf[n];
#pragma unroll
        for (uint32_t j = 0; j < n; ++j)
            bf[j] = GEMM_LAB_SKIP(6) ? u32x4{lane, t, j, 0u} : *reinterpret_cast<const u32x4*>(base + bRead + j * 16u * kGemmHalfRowBytes);
#pragma unroll
        for (uint32_t i = 0; i < m; ++i) {
            if (i + 1u == m && t + 1u < (uint32_t)KT) {
                // my chunks of slice t + 1 have landed - A(t + 1) and, requested before it, B(t + 1); B(t + 2)'s DMAs stay
                // outstanding.  The last wait of the loop is vmcnt(0): nothing is on its way when the epilogue takes the
                // LDS.  (MFMAs are register-only: without the fence hipcc moves the wait, and its own waits for A's
                // registers, in front of the slice's MFMAs - the wave then stands there with nothing issued.  The last
                // row tile's MFMAs stay behind the wait and run beside the rounding.)
                __builtin_amdgcn_sched_barrier(0);
                GEMM_LAB_SPAN_BEGIN;
                if (t + 2u < (uint32_t)KT) gemmWaitRequests<BDMAS>(aNext); else gemmWaitRequests<0>(aNext);
                GEMM_LAB_SPAN_END(8);
                GEMM_LAB_SPAN_BEGIN;
            }
            const u32x4 af = GEMM_LAB_SKIP(6) ? u32x4{lane, t, i, 2u} : *reinterpret_cast<const u32x4*>(base + aRead + i * 16u * kGemmHalfRowBytes);
            if (!GEMM_LAB_SKIP(0)) {
#pragma unroll
                for (uint32_t j = 0; j < n; ++j) acc[i][j] = mfma16<MODE>(af, bf[j], acc[i][j]);
            } else {
                gemmKeep(af);
#pragma unroll
                for (uint32_t j = 0; j < n; ++j) gemmKeep(bf[j]);
            }
        }
        if (t + 1u < (uint32_t)KT) {
            // round them into the other stage of H, then the registers take A(t + 2) and the stage of F just read (this
            // wave's own reads of it are over: lgkmcnt(0)) takes B(t + 3)
            roundChunks(t + 1u);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            requestA(t + 2u);
            requestB(t + 3u);
        } else {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            GEMM_LAB_SPAN_BEGIN;
        }
        __builtin_amdgcn_s_barrier();
        GEMM_LAB_SPAN_END(9);
    }

    // ---- the sparse mask: slab passes over the wave's tiles (as denseGemm)
    GEMM_LAB_STAMP(4);
    float* slab = reinterpret_cast<float*>(lds) + wave * (kGemmPassTiles * 256u);
    const uint32_t slabAddr = __builtin_amdgcn_readfirstlane(gemmLdsAddress(slab));
    const uint32_t* rowTable = reinterpret_cast<const uint32_t*>(lds + rowTableAt) + wm * (TM / 2u);
#pragma unroll
    for (uint32_t q = 0; q < Q; ++q) {
        if (!GEMM_LAB_SKIP(3)) {
            if (slabAddr < 0x10000u) {
#pragma unroll
                for (uint32_t tp = 0; tp < kGemmPassTiles; ++tp) {
                    const uint32_t tIdx = q * kGemmPassTiles + tp;
                    if (tIdx < m * n) gemmDumpTile(acc[tIdx / n][tIdx % n], slabAddr + tp * 1024u, false);
                }
            } else {
#pragma unroll
                for (uint32_t tp = 0; tp < kGemmPassTiles; ++tp) {
                    const uint32_t tIdx = q * kGemmPassTiles + tp;
                    if (tIdx < m * n) gemmDumpTile(acc[tIdx / n][tIdx % n], slabAddr + tp * 1024u, true);
                }
            }
        }
        gemmMaskPass<kGemmWordChunk, TM / 2u, Q, kDeepWords>(words, slab, rowTable, P, myList, q, lane, wAhead, GEMM_LAB_SKIP(4), GEMM_LAB_SKIP(5));
        GEMM_LAB_STAMP(5u + q);
    }
    GEMM_LAB_STAMPS_OUT;
}

}  // namespace bsmr
