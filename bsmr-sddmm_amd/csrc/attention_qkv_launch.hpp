// The entries of the one-pass attention units (csrc/attention_qkv*.hip), as bsmr_capi.hip calls them for a checked call.
// The lists and the block format are the types of the helper headers, which both sides include: one definition, checked by
// the compiler.  bf16: the 16-bit format, false = fp16.  Every entry returns the launch status.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "backward_lists.hpp"   // BwItem, BwSplit
#include "blocked_format.hpp"   // BlkPanel, BlkSegment
#include "lowp_device.hpp"      // u32x4

// The entries of csrc/attention_qkv.hip.  bsmrLaunchAttnQkv: attnQkv over the handle's row-direction BwItem list, then the
// merge of its BwSplit table.  bsmrLaunchAttnQkvMerge: attnQkvMerge (csrc/attention_qkv_kernels.hpp) alone, when there is a
// split row; the unit of the quantised KV cache ends with it too, so the kernel has one home.
hipError_t bsmrLaunchAttnQkv(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits, uint32_t numSplits,
                             const uint32_t* src, float scale, const uint16_t* Q, const uint16_t* Kt, const uint16_t* V,
                             uint16_t* O, float* m, float* s, float* partial, float* sPart, float* mPart, uint32_t K, uint32_t Kv,
                             uint32_t M, uint32_t N, uint32_t numSlots, uint32_t numBatches, bool bf16, hipStream_t stream);
hipError_t bsmrLaunchAttnQkvMerge(const bsmr::BwSplit* splits, uint32_t numSplits, const float* partial, const float* sPart,
                                  const float* mPart, uint16_t* O, float* m, float* s, uint32_t Kv, uint32_t M,
                                  uint32_t numSlots, uint32_t numBatches, bool bf16, hipStream_t stream);

// The one entry of csrc/attention_qkv_gqa.hip: bsmrLaunchAttnQkv for grouped key/value heads - attnQkvGqa
// (csrc/attention_qkv_gqa_kernels.hpp), ending in bsmrLaunchAttnQkvMerge.  Q, O, m, s and the partials have numBatches query
// heads, Kt and V numBatches / kvGroup heads; query head h reads KV head h / kvGroup.  kvGroup >= 2 divides numBatches, K and
// Kv are at most 256 (the caller checked).
hipError_t bsmrLaunchAttnQkvGqa(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits, uint32_t numSplits,
                                const uint32_t* src, float scale, const uint16_t* Q, const uint16_t* Kt, const uint16_t* V,
                                uint16_t* O, float* m, float* s, float* partial, float* sPart, float* mPart, uint32_t K,
                                uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots, uint32_t numBatches, uint32_t kvGroup,
                                bool bf16, hipStream_t stream);

// The one entry of csrc/attention_qkv_gqa_mfma.hip: bsmrLaunchAttnQkvGqa's arguments on attnQkvGqaMfma
// (csrc/attention_qkv_gqa_mfma_kernels.hpp: both products on the MFMA, up to 16 heads of a group per wave), ending in
// bsmrLaunchAttnQkvMerge.  kvGroup >= 1 divides numBatches, K and Kv are at most 256 (the caller checked).
hipError_t bsmrLaunchAttnQkvGqaMfma(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits,
                                    uint32_t numSplits, const uint32_t* src, float scale, const uint16_t* Q, const uint16_t* Kt,
                                    const uint16_t* V, uint16_t* O, float* m, float* s, float* partial, float* sPart,
                                    float* mPart, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots,
                                    uint32_t numBatches, uint32_t kvGroup, bool bf16, hipStream_t stream);

// The one entry of csrc/attention_qkv_bwd.hip: attnQkvBwdQ over the row direction's lists when dQ is asked for, attnQkvBwdKV
// over the column direction's when dKt or dV is, each followed by attnQkvBwdReduce for its split destinations
// (csrc/attention_qkv_bwd_kernels.hpp).  A gradient that is NULL is not computed.  D [b][M]: dO_r . O_r, already written on
// the stream; rowPart [b][rows.numSlots][K] and colPart [b][cols.numSlots][K + Kv]: the chunk partials, written here.
struct BsmrAttnBwdLists {   // one direction of the handle, on the device
    const bsmr::BwItem* items;     // [numItems]
    uint32_t numItems;
    const bsmr::BwSplit* splits;   // [numSplits]
    uint32_t numSplits;
    const uint32_t* src;    // colIndices (rows) or cscRows (columns)
    uint32_t numSlots;
};
hipError_t bsmrLaunchAttnQkvBwd(const BsmrAttnBwdLists& rows, const BsmrAttnBwdLists& cols, float scale, const uint16_t* Q,
                                const uint16_t* Kt, const uint16_t* V, const uint16_t* dO, const float* m, const float* s,
                                const float* D, uint16_t* dQ, uint16_t* dKt, uint16_t* dV, float* rowPart, float* colPart,
                                uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numBatches, bool bf16,
                                hipStream_t stream);
// bsmrLaunchAttnQkvBwdReduce: attnQkvBwdReduce alone, when `lists` has a split destination; the unit of the grouped backward
// ends with it too, so the kernel has one home.  A slot's row of `partial` [numBatches][lists.numSlots] is `stride` floats,
// the gradient's `width` floats lie at `offset` in it; out [numBatches][outRows][width].
hipError_t bsmrLaunchAttnQkvBwdReduce(const BsmrAttnBwdLists& lists, const float* partial, uint32_t stride, uint32_t offset,
                                      uint16_t* out, uint32_t width, uint32_t outRows, uint32_t numBatches, bool bf16,
                                      hipStream_t stream);

// The one entry of csrc/attention_qkv_gqa_bwd.hip: bsmrLaunchAttnQkvBwd for grouped key/value heads - attnQkvGqaBwdQ and
// attnQkvGqaBwdKV (csrc/attention_qkv_gqa_bwd_kernels.hpp), each followed by bsmrLaunchAttnQkvBwdReduce.  Q, dO, m, s, D, dQ
// and rowPart have numBatches query heads; Kt, V, dKt, dV and colPart [b / g][cols.numSlots][K + Kv] numBatches / kvGroup
// heads; query head h reads KV head h / kvGroup.  kvGroup >= 2 divides numBatches (the caller checked).
hipError_t bsmrLaunchAttnQkvGqaBwd(const BsmrAttnBwdLists& rows, const BsmrAttnBwdLists& cols, float scale, const uint16_t* Q,
                                   const uint16_t* Kt, const uint16_t* V, const uint16_t* dO, const float* m, const float* s,
                                   const float* D, uint16_t* dQ, uint16_t* dKt, uint16_t* dV, float* rowPart, float* colPart,
                                   uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numBatches, uint32_t kvGroup,
                                   bool bf16, hipStream_t stream);

// A row of a panel with blocks, as attnQkvBlkMerge (csrc/attention_qkv_blocked_kernels.hpp) merges it: its residue chunks
// on the slots resFirst ... of attnQkv's partial area, then its block units on the rows blkFirst, blkFirst + 16, ... of
// the block partial area (a unit owns 16 consecutive rows, one per row of its panel).
struct BsmrAttnBlkRow {
    uint32_t dest;       // the row of S
    uint32_t resFirst;
    uint32_t resCount;   // 0: the row has no residue entry
    uint32_t blkFirst;
    uint32_t blkCount;   // >= 1
};

// The one entry of csrc/attention_qkv_blocked.hip: attnQkvBlocks over the RPHM's blocks, then attnQkvBlkMerge.  units:
// BlkSegment[numUnits] if `segments`, else BlkPanel[numUnits] (one of two types, so untyped); cells / cols / panelRows /
// zeros: the device format of bsmr_backward_attach_blocks; rows: BsmrAttnBlkRow[numRows].  partial / sPart / mPart
// [b][numSlots]: what attnQkv left for the residue chunks; bPart [b][16 numUnits][Kv], bs and bm [b][16 numUnits]: the block
// partials, written here.
hipError_t bsmrLaunchAttnQkvBlocks(const void* units, uint32_t numUnits, bool segments, const uint32_t* panelRows,
                                   const bsmr::u32x4* cells, const bsmr::u32x4* cols, const float* zeros,
                                   const BsmrAttnBlkRow* rows, uint32_t numRows, float scale, const uint16_t* Q,
                                   const uint16_t* Kt, const uint16_t* V, uint16_t* O, float* m, float* s, const float* partial,
                                   const float* sPart, const float* mPart, uint32_t numSlots, float* bPart, float* bs, float* bm,
                                   uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numBatches, bool bf16,
                                   hipStream_t stream);

// The one entry of csrc/attention_qkv_kv.hip: bsmrLaunchAttnQkv for attnQkvKv (csrc/attention_qkv_kv_kernels.hpp), ending in
// bsmrLaunchAttnQkvMerge.  Kt / V: the codes as the cache holds them; kvFormat: their format (the fp8 values are
// BSMR_FP8_E4M3 / _E5M2); mx: Ks / Vs are the E8M0 block scales (always with e2m1), otherwise they are not read.
enum : int { kQkvKvE4M3 = 0, kQkvKvE5M2 = 1, kQkvKvE2M1 = 2 };
hipError_t bsmrLaunchAttnQkvKv(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits, uint32_t numSplits,
                               const uint32_t* src, float scale, const uint16_t* Q, const uint8_t* Kt, const uint8_t* Ks,
                               const uint8_t* V, const uint8_t* Vs, uint16_t* O, float* m, float* s, float* partial, float* sPart,
                               float* mPart, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots,
                               uint32_t numBatches, bool bf16, int kvFormat, bool mx, hipStream_t stream);

// The one entry of csrc/attention_qkv_gqa_kv.hip: bsmrLaunchAttnQkvKv for grouped key/value heads - attnQkvGqaKv
// (csrc/attention_qkv_gqa_kv_kernels.hpp), ending in bsmrLaunchAttnQkvMerge.  Q, O, m, s and the partials have numBatches
// query heads; Kt, V, Ks and Vs numBatches / kvGroup heads; query head h reads KV head h / kvGroup.  kvGroup >= 2 divides
// numBatches, K and Kv are at most 256 (the caller checked).
hipError_t bsmrLaunchAttnQkvGqaKv(const bsmr::BwItem* items, uint32_t numItems, const bsmr::BwSplit* splits, uint32_t numSplits,
                                  const uint32_t* src, float scale, const uint16_t* Q, const uint8_t* Kt, const uint8_t* Ks,
                                  const uint8_t* V, const uint8_t* Vs, uint16_t* O, float* m, float* s, float* partial,
                                  float* sPart, float* mPart, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots,
                                  uint32_t numBatches, uint32_t kvGroup, bool bf16, int kvFormat, bool mx, hipStream_t stream);
