// The work units of the kernels over the RPHM's dense 16 x 16 blocks as the device reads them (built by
// bsmr_backward_attach_blocks[_split], csrc/blocked_capi.hpp; the cell and column layout: csrc/spmm_blocked_kernels.hpp).
// Formats only - no kernel is defined here - so the blocked SpMM and the blocked one-pass attention unit share one
// definition.
#pragma once

#include <stdint.h>

namespace bsmr {

constexpr uint32_t kBlkNull = 0xFFFFFFFFu;   // an empty cell; a row of a ragged last panel that does not exist

struct BlkPanel {          // a row panel that has blocks; its ordinal q owns rows [16 q, 16 q + 16) of the staging area
    uint32_t firstBlock;
    uint32_t numBlocks;
};

struct BlkSegment {        // S >= 1: `numBlocks` consecutive blocks of panel ordinal `panel`
    uint32_t firstBlock;
    uint32_t numBlocks;
    uint32_t panel;
    uint32_t partial;      // its slot (16 rows) of the partial area, or kBlkNull: the segment is the whole panel
};

struct BlkSplit {          // a panel cut into numSegments >= 2 segments, on the partial slots firstPartial ...
    uint32_t panel;
    uint32_t firstPartial;
    uint32_t numSegments;
};

}  // namespace bsmr
