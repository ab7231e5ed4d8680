// The work lists of the gather kernels as the device reads them (built by csrc/backward_capi.hpp): one BwItem per list or
// chunk of a long list, one BwSplit per destination whose list was cut.  Formats only - no kernel is defined here - so
// the gather kernels (csrc/spmm_kernels.hpp), the one-pass attention units and their launch entries
// (csrc/attention_qkv_launch.hpp) share one definition.
#pragma once

#include <stdint.h>

namespace bsmr {

constexpr uint32_t kBwDirect = 0xFFFFFFFFu;   // BwItem.slot: the item owns its whole list and writes Y[dest]

struct BwItem {
    uint32_t dest;    // destination row of Y
    uint32_t begin;   // [begin, end): positions in the direction's list array (CSR index or CSC position)
    uint32_t end;
    uint32_t slot;    // workspace row of this chunk's partial sum, or kBwDirect
};

struct BwSplit {      // a destination whose list was cut into numSlots chunks (partials at firstSlot ...)
    uint32_t dest;
    uint32_t firstSlot;
    uint32_t numSlots;
    uint32_t pad;
};

}  // namespace bsmr
