// The one entry of csrc/attention_qkv.hip: the launches of attnQkv and attnQkvMerge (csrc/attention_qkv_kernels.hpp) for a
// checked call.  items / splits: the handle's row-direction BwItem list and BwSplit table on the device (untyped here: the
// kernel headers are private to that translation unit).  bf16: the 16-bit format, false = fp16.  Returns the launch status.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

hipError_t bsmrLaunchAttnQkv(const void* items, uint32_t numItems, const void* splits, uint32_t numSplits, const uint32_t* src,
                             float scale, const uint16_t* Q, const uint16_t* Kt, const uint16_t* V, uint16_t* O, float* m,
                             float* s, float* partial, float* sPart, float* mPart, uint32_t K, uint32_t Kv, uint32_t M,
                             uint32_t N, uint32_t numSlots, uint32_t numBatches, bool bf16, hipStream_t stream);
