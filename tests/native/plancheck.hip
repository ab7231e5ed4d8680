// Test infrastructure (not shipped): the host side of bsmr_plan_create - residue promotion (plan_promote.hpp)
// and packing (plan_pack.hpp) - callable without a GPU, with the invariants a device plan relies on checked here:
// every stored entry is computed exactly once, a promoted entry sits in the block cell of its own row and column.
#include <chrono>
#include <cstdint>
#include <vector>

#include "plan_pack.hpp"
#include "plan_promote.hpp"
#include "tile_format.hpp"

namespace {
double nowUs() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

// out[0] promoted (0/1), [1] promoted entries, [2] promoted blocks, [3] blocks after, [4] residue entries after,
// [5] packPlan status, [6] packed dense entries, [7] packed residue entries, [8] promotion us, [9] packing us,
// [10] B columns gathered by the dense blocks ungrouped, [11] with 4 panels per group,
// [12] bytes per index-tile element (1 = windowed 8-bit, 2 / 4 = offsets from the row's first dense entry).
// Returns 0, or the number of the first violated invariant.
extern "C" int plancheck_promote(const bsmr_rphm_desc* in, uint32_t minAverage, uint64_t minEntries, uint64_t smallDense,
                                 uint32_t minColumnDegree, uint32_t headMin, uint64_t* out) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    const uint32_t P = in->num_row_panels;
    bsmr::PromotedRphm pr;
    double t0 = nowUs();
    const bool did = bsmr::promoteSparseBlocks(*in, minAverage, minEntries, smallDense, minColumnDegree, headMin, pr);
    out[8] = (uint64_t)(nowUs() - t0);
    const bsmr_rphm_desc* d = did ? &pr.desc : in;
    out[0] = did;
    out[1] = pr.promotedEntries;
    out[2] = pr.promotedBlocks;
    out[3] = d->block_offsets[P];
    out[4] = d->sparse_value_offsets[P];
    if (did) {
        if (d->block_offsets[P] != in->block_offsets[P] + pr.promotedBlocks) return 1;
        if (d->sparse_value_offsets[P] + pr.promotedEntries != in->sparse_value_offsets[P]) return 2;
        // where every residue entry of the input went
        std::vector<uint8_t> seen(in->nnz, 0);
        for (uint32_t q = 0; q < P; ++q) {
            const uint64_t own = in->block_offsets[q + 1] - in->block_offsets[q];
            const uint64_t b0 = d->block_offsets[q], b1 = d->block_offsets[q + 1];
            if (b1 - b0 < own) return 3;
            // the panel's own blocks come first, unchanged
            for (uint64_t b = 0; b < own; ++b) {
                for (uint32_t i = 0; i < 16; ++i)
                    if (d->dense_cols[(b0 + b) * 16 + i] != in->dense_cols[(in->block_offsets[q] + b) * 16 + i]) return 4;
                for (uint32_t i = 0; i < 256; ++i)
                    if (d->block_values[(b0 + b) * 256 + i] != in->block_values[(in->block_offsets[q] + b) * 256 + i]) return 5;
            }
            // promoted blocks: a column appears once per panel, cells hold entries of that (row, column)
            for (uint64_t b = b0 + own; b < b1; ++b)
                for (uint32_t i = 0; i < 256; ++i) {
                    const uint32_t v = d->block_values[b * 256 + i];
                    if (v == kNone) continue;
                    if (v >= in->nnz || seen[v]) return 6;
                    seen[v] = 1;
                }
            for (uint32_t i = d->sparse_value_offsets[q]; i < d->sparse_value_offsets[q + 1]; ++i) {
                const uint32_t v = d->sparse_values[i];
                if (v >= in->nnz || seen[v]) return 7;
                seen[v] = 2;
            }
            // every input residue entry of the panel is in exactly one of the two, at its own row and column
            for (uint32_t i = in->sparse_value_offsets[q]; i < in->sparse_value_offsets[q + 1]; ++i) {
                const uint32_t v = in->sparse_values[i], row = in->sparse_relative_rows[i], col = in->sparse_col_indices[i];
                if (!seen[v]) return 8;
                if (seen[v] == 1) {
                    bool found = false;
                    for (uint64_t b = b0 + own; b < b1 && !found; ++b)
                        for (uint32_t c = 0; c < 16 && !found; ++c)
                            found = d->dense_cols[b * 16 + c] == col && d->block_values[b * 256 + row * 16 + c] == v;
                    if (!found) return 9;
                }
            }
            // residue order of what stays is the input's order
            uint32_t at = d->sparse_value_offsets[q];
            for (uint32_t i = in->sparse_value_offsets[q]; i < in->sparse_value_offsets[q + 1]; ++i) {
                if (seen[in->sparse_values[i]] != 2) continue;
                if (d->sparse_values[at] != in->sparse_values[i] || d->sparse_relative_rows[at] != in->sparse_relative_rows[i] ||
                    d->sparse_col_indices[at] != in->sparse_col_indices[i])
                    return 10;
                ++at;
            }
            if (at != d->sparse_value_offsets[q + 1]) return 11;
            // no column twice among the promoted blocks of a panel
            std::vector<uint32_t> cols(d->dense_cols + (b0 + own) * 16, d->dense_cols + b1 * 16);
            std::sort(cols.begin(), cols.end());
            for (size_t i = 1; i < cols.size(); ++i)
                if (cols[i] == cols[i - 1] && cols[i] != in->N) return 12;
        }
    }
    bsmr::PackOptions opt;
    opt.blocksPerItem = 8;
    bsmr::PackedPlan pk;
    t0 = nowUs();
    out[5] = (uint64_t)(int64_t)bsmr::packPlan(d, opt, pk);
    out[9] = (uint64_t)(nowUs() - t0);
    out[10] = bsmr::countUnionColumns(d, 1);
    out[11] = bsmr::countUnionColumns(d, 4);
    out[12] = !pk.tiles8.empty() || !pk.tilesMask.empty() ? 1 : !pk.tiles16.empty() ? 2 : !pk.tiles32.empty() ? 4 : 0;
    out[6] = pk.numDenseEntries;
    out[7] = pk.numSparseEntries;
    return 0;
}

// The "tiles" dense format (csrc/tile_format.hpp) packed for H panels per group and checked the way the kernel reads
// it: every dense entry of the RPHM is listed exactly once, in a block that holds its column at the listed slot, on
// the listed row of its group, and row base + offset is its CSR index; entry lists start on multiples of 4 and are
// ordered by (row, column); a block's mask has exactly the panels that own an entry; counts fit the LDS room.
// out[0] blocks, [1] tiles, [2] union columns, [3] entries, [4] items, [5] entry cap, [6] bytes, [7..9] census blocks / tiles / columns.
extern "C" int plancheck_tiles(const bsmr_rphm_desc* d, uint32_t H, uint32_t blocksPerItem, uint64_t* out) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    bsmr::HostDense hd;
    int st = bsmr::collectDense(d, hd);
    if (st != BSMR_OK) return 100 + st;
    bsmr::TileFormatHost f;
    st = bsmr::packTiles(hd, H, blocksPerItem, f);
    if (st != BSMR_OK) return 200 + st;
    const bsmr::TileCensus census = bsmr::tileCensus(hd, H);
    out[0] = f.numBlocks; out[1] = f.numTiles; out[2] = f.unionColumns; out[3] = f.numEntries;
    out[4] = f.items.size(); out[5] = f.entryCap; out[6] = f.bytes();
    out[7] = census.blocks; out[8] = census.tiles; out[9] = census.unionColumns;
    const uint32_t R = 16 * H;
    // expected: CSR index -> (original row, column) from the RPHM
    std::vector<uint32_t> wantRow(d->nnz, kNone), wantCol(d->nnz, kNone);
    uint64_t denseEntries = 0;
    for (uint32_t p = 0; p < d->num_row_panels; ++p)
        for (uint64_t b = d->block_offsets[p]; b < d->block_offsets[p + 1]; ++b)
            for (uint32_t i = 0; i < 256; ++i) {
                const uint32_t v = d->block_values[b * 256 + i];
                if (v == kNone) continue;
                const size_t slot = (size_t)p * 16 + i / 16;
                wantRow[v] = slot < d->num_nonzero_rows ? d->reordered_rows[slot] : kNone;
                wantCol[v] = d->dense_cols[b * 16 + i % 16];
                ++denseEntries;
            }
    if (f.numEntries != denseEntries) return 1;
    std::vector<uint8_t> seen(d->nnz, 0);
    std::vector<uint8_t> blockSeen(f.numBlocks, 0);
    uint64_t tiles = 0, cols = 0;
    for (size_t it = 0; it < f.items.size(); ++it) {
        const bsmr::TileItem& item = f.items[it];
        if (item.count == 0 || item.count > bsmr::kTileMaxItemBlocks || item.first + item.count > f.numBlocks) return 2;
        if (it && f.blockCols[(size_t)f.items[it - 1].first * 16] > f.blockCols[(size_t)item.first * 16]) return 3;  // column order
        for (uint32_t b = item.first; b < item.first + item.count; ++b) {
            if (blockSeen[b]++) return 4;
            const uint32_t start = f.blockInfo[4 * (size_t)b], mask = f.blockInfo[4 * (size_t)b + 1] & 0xFFFFu;
            const uint32_t n = f.blockInfo[4 * (size_t)b + 1] >> 16;
            uint32_t quarter[4] = {0, 0, 0, 0};
            if (start % 4 || n == 0 || n > f.entryCap || (size_t)start + (n + 255) / 256 * 256 > f.entries.size()) return 5;
            uint32_t got = 0, last = 0;
            for (uint32_t e = 0; e < n; ++e) {
                const uint32_t w = f.entries[start + e];
                const uint32_t row = w & 255u, slot = (w >> 8) & 15u, off = w >> 12;
                if (row < R) ++quarter[row / (4 * H)];
                if (row >= R) return 6;
                const uint32_t idx = f.itemRowBase[it * R + row] + off;
                if (idx >= d->nnz || seen[idx]++) return 7;
                if (f.groupRows[(size_t)item.group * R + row] != wantRow[idx]) return 8;
                if (f.blockCols[(size_t)b * 16 + slot] != wantCol[idx]) return 9;
                const uint32_t key = row * 16 + slot;
                if (e && key < last) return 10;   // (row, column) order
                last = key;
                got |= 1u << (row / 16);
            }
            if (got != mask) return 11;
            if ((quarter[0] | (quarter[1] << 16)) != f.blockInfo[4 * (size_t)b + 2] ||
                (quarter[2] | (quarter[3] << 16)) != f.blockInfo[4 * (size_t)b + 3]) return 19;
            tiles += __builtin_popcount(mask);
            for (uint32_t c = 0; c < 16; ++c) {
                if (c && f.blockCols[(size_t)b * 16 + c] != 0 && f.blockCols[(size_t)b * 16 + c] <= f.blockCols[(size_t)b * 16 + c - 1]) return 12;
                if (f.blockCols[(size_t)b * 16 + c] >= d->N) return 13;
            }
        }
    }
    for (uint64_t b = 0; b < f.numBlocks; ++b)
        if (!blockSeen[b]) return 14;
    for (uint32_t v = 0; v < d->nnz; ++v)
        if ((wantRow[v] != kNone) != (seen[v] != 0)) return 15;
    if (tiles != f.numTiles) return 16;
    (void)cols;
    if (census.blocks > f.numBlocks || census.unionColumns != f.unionColumns) return 17;   // (blocks cut at the entry cap add to the census)
    if (census.blocks == f.numBlocks && census.tiles != f.numTiles) return 18;
    return 0;
}

#include "sweep_format.hpp"

// csrc/sweep_format.hpp read the way denseSweep reads it: every dense entry of the RPHM is listed exactly once, in
// the (item, wave, block) list of its row group / panel / column block, with the slab slot of its accumulator cell.
// out[0] items, [1] words, [2] groups, [3] strips, [4] most entries in one (wave, block) step, [5] bytes.
extern "C" int plancheck_sweep(const bsmr_rphm_desc* d, uint32_t W, uint32_t PW, uint32_t stripBlocks, uint64_t* out) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    bsmr::HostDense hd;
    int st = bsmr::collectDense(d, hd);
    if (st != BSMR_OK) return 100 + st;
    bsmr::SweepFormatHost f;
    st = bsmr::packSweep(hd, W, PW, stripBlocks, f);
    if (st != BSMR_OK) return 200 + st;
    out[0] = f.items.size(); out[1] = hd.entries(); out[2] = f.numGroups; out[3] = f.numStrips;
    out[4] = f.maxStepEntries; out[5] = f.bytes();
    std::vector<uint32_t> wantRow(d->nnz, kNone), wantCol(d->nnz, kNone);
    uint64_t denseEntries = 0;
    for (uint32_t p = 0; p < d->num_row_panels; ++p)
        for (uint64_t b = d->block_offsets[p]; b < d->block_offsets[p + 1]; ++b)
            for (uint32_t i = 0; i < 256; ++i) {
                const uint32_t v = d->block_values[b * 256 + i];
                if (v == kNone) continue;
                const size_t slot = (size_t)p * 16 + i / 16;
                wantRow[v] = slot < d->num_nonzero_rows ? d->reordered_rows[slot] : kNone;
                wantCol[v] = d->dense_cols[b * 16 + i % 16];
                ++denseEntries;
            }
    if (hd.entries() != denseEntries) return 1;
    const uint32_t GP = W * PW, NCB = (d->N + 15) / 16;
    if (f.items.size() != (size_t)f.numGroups * f.numStrips) return 2;
    if (f.panelRows.size() != (size_t)f.numGroups * GP * 16) return 3;
    std::vector<uint8_t> seen(d->nnz, 0);
    std::vector<uint32_t> blockCover(NCB, 0);
    uint64_t expectStart = 0;
    for (size_t it = 0; it < f.items.size(); ++it) {
        const bsmr::SweepItem& item = f.items[it];
        if (item.group >= f.numGroups || item.numBlocks == 0 || item.numBlocks > bsmr::kSweepMaxBlocks ||
            item.firstBlock + item.numBlocks > NCB)
            return 4;
        if (it / f.numGroups != item.firstBlock / stripBlocks || it % f.numGroups != item.group) return 5;   // strip-major
        if (item.group == 0)
            for (uint32_t b = 0; b < item.numBlocks; ++b) ++blockCover[item.firstBlock + b];
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t* starts = &f.starts[(size_t)item.startsBase + (size_t)w * (item.numBlocks + 1)];
            if (starts[0] != expectStart) return 6;    // the lists follow each other without gaps
            for (uint32_t b = 0; b < item.numBlocks; ++b) {
                if (starts[b + 1] < starts[b] || starts[b + 1] - starts[b] > ((f.maxStepEntries + 3u) & ~3u) || starts[b] % 4) return 7;
                for (uint32_t e = starts[b]; e < starts[b + 1]; ++e) {
                    const uint32_t word = f.words[e], slot = word & 1023u, rw = (word >> 10) & 63u, off = word >> 16;
                    if (word == bsmr::kSweepNoEntry) {   // padding to a multiple of 4 words, at the end of the list only
                        if (starts[b + 1] - e > 3) return 17;
                        continue;
                    }
                    if (e + 1 < starts[b + 1] && f.words[e + 1] != bsmr::kSweepNoEntry && e > starts[b] && f.words[e - 1] == bsmr::kSweepNoEntry) return 18;
                    if (rw >= 16 * PW) return 8;
                    const uint32_t j = rw / 16, r = rw % 16;
                    if (slot >= PW * 256 || slot / 256 != j) return 9;
                    const uint32_t reg = slot & 3u, lane = (slot >> 2) & 63u;
                    if (reg != (r & 3u) || lane / 16 != r / 4) return 10;   // accumulator layout: lane = 16 (r / 4) + c, register r % 4
                    const uint32_t c = lane & 15u;
                    const uint32_t idx = f.rowStart[(it * W + w) * (16 * PW) + rw] + off;
                    if (idx >= d->nnz || seen[idx]++) return 11;
                    if (f.panelRows[((size_t)item.group * GP + w * PW + j) * 16 + r] != wantRow[idx]) return 12;
                    if ((item.firstBlock + b) * 16 + c != wantCol[idx]) return 13;
                }
            }
            expectStart = starts[item.numBlocks];
        }
        if (expectStart - f.starts[item.startsBase] > f.maxItemWords) return 19;
    }
    if (f.words.size() < expectStart + bsmr::kSweepWordSlack) return 14;   // the loaders move an item's words in whole pseudo-images
    for (uint32_t b = 0; b < NCB; ++b)
        if (blockCover[b] != 1) return 15;
    for (uint32_t v = 0; v < d->nnz; ++v)
        if ((wantRow[v] != kNone) != (seen[v] != 0)) return 16;
    return 0;
}

#include "gemm_format.hpp"

// csrc/gemm_format.hpp read the way denseGemm reads it: every dense entry of the RPHM is listed exactly once, in the
// (item, wave, pass) list of its macro-tile / panel / column block, with the slab slot of its accumulator cell; the item
// order is gemmItemPlace's; lists are ordered by (row, column).
// out[0] items, [1] entries, [2] groups, [3] strips, [4] full grid, [5] bytes, [6] tiles, [7] longest list.
extern "C" int plancheck_gemm(const bsmr_rphm_desc* d, uint32_t PM, uint32_t NB, uint32_t balance, uint64_t* out) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    bsmr::HostDense hd;
    int st = bsmr::collectDense(d, hd);
    if (st != BSMR_OK) return 100 + st;
    bsmr::GemmFormatHost f;
    st = bsmr::packGemm(hd, PM, NB, f, balance != 0);
    if (st != BSMR_OK) return 200 + st;
    out[0] = f.items.size(); out[1] = hd.entries(); out[2] = f.numGroups; out[3] = f.numStrips; out[4] = f.fullGrid;
    out[5] = f.bytes(); out[6] = f.numTiles; out[7] = f.maxListWords;
    std::vector<uint32_t> wantRow(d->nnz, kNone), wantCol(d->nnz, kNone);
    uint64_t denseEntries = 0;
    for (uint32_t p = 0; p < d->num_row_panels; ++p)
        for (uint64_t b = d->block_offsets[p]; b < d->block_offsets[p + 1]; ++b)
            for (uint32_t i = 0; i < 256; ++i) {
                const uint32_t v = d->block_values[b * 256 + i];
                if (v == kNone) continue;
                const size_t slot = (size_t)p * 16 + i / 16;
                wantRow[v] = slot < d->num_nonzero_rows ? d->reordered_rows[slot] : kNone;
                wantCol[v] = d->dense_cols[b * 16 + i % 16];
                ++denseEntries;
            }
    if (hd.entries() != denseEntries) return 1;
    if (denseEntries == 0) return f.items.empty() ? 0 : 2;
    const uint32_t TM = PM * 16, m = PM / bsmr::kGemmWavesM, n = NB / bsmr::kGemmWavesN;
    const uint32_t Q = (m * n + bsmr::kGemmPassTiles - 1) / bsmr::kGemmPassTiles, L = bsmr::kGemmWaves * Q;
    if (f.passes != Q || f.panelRows.size() != (size_t)f.numGroups * TM) return 3;
    // colOf: every column that holds a dense entry in exactly one slot (unused slots name column 0); natural order without
    // balancing; with it, the strips' entry counts differ by at most two columns' worth (the columns were dealt by
    // descending count, back and forth) - counted below from the lists themselves
    if (f.colOf.size() != (size_t)f.numStrips * NB * 16) return 21;
    std::vector<uint32_t> degree(d->N, 0);
    uint32_t maxDegree = 0;
    for (uint32_t v = 0; v < d->nnz; ++v)
        if (wantCol[v] != kNone) maxDegree = std::max(maxDegree, ++degree[wantCol[v]]);
    {
        std::vector<uint32_t> slots(d->N, 0);
        for (size_t q = 0; q < f.colOf.size(); ++q) {
            const uint32_t c = f.colOf[q];
            if (c >= d->N) return 22;
            if (!balance && q < d->N && c != q) return 23;
            ++slots[c];
        }
        for (uint32_t c = 1; c < d->N; ++c)
            if (degree[c] ? slots[c] != 1 : slots[c] > 1) return 24;
        if (slots[0] == 0) return 25;
    }
    std::vector<uint64_t> perStrip(f.numStrips, 0);
    if (f.rowStart.size() != f.items.size() * TM || f.lists.size() != f.items.size() * (L + 1)) return 4;
    if (f.fullGrid != (f.items.size() == (size_t)f.numGroups * f.numStrips)) return 5;
    std::vector<uint8_t> seen(d->nnz, 0);
    uint64_t expectStart = 0, place = 0;
    for (size_t it = 0; it < f.items.size(); ++it) {
        const bsmr::GemmItem& item = f.items[it];
        if (item.group >= f.numGroups || item.firstBlock % NB || item.firstBlock / NB >= f.numStrips) return 6;
        if (item.listBase != it * (L + 1)) return 7;
        // the order of gemmItemPlace, macro-tiles without entries left out
        for (;; ++place) {
            if (place >= (uint64_t)f.numGroups * f.numStrips) return 8;
            uint32_t g, s;
            bsmr::gemmItemPlace((uint32_t)place, f.numGroups, f.numStrips, g, s);
            if (g == item.group && s == item.firstBlock / NB) break;
        }
        ++place;
        uint64_t itemEntries = 0;
        for (uint32_t w = 0; w < bsmr::kGemmWaves; ++w)
            for (uint32_t q = 0; q < Q; ++q) {
                const uint32_t b = f.lists[item.listBase + w * Q + q], e = f.lists[item.listBase + w * Q + q + 1];
                if (b != expectStart || e < b || (e - b) % 4 || e - b > f.maxListWords) return 9;   // lists follow each other, padded to 4
                expectStart = e;
                const uint32_t wm = w / bsmr::kGemmWavesN, wn = w % bsmr::kGemmWavesN;
                uint64_t lastKey = 0;
                bool padding = false;
                for (uint32_t i = b; i < e; ++i) {
                    const uint32_t word = f.words[i];
                    if (word == bsmr::kGemmNoEntry) {
                        if (e - i > 3) return 10;   // padding only at the end of a list
                        padding = true;
                        continue;
                    }
                    if (padding) return 11;
                    const uint32_t slot = word & 4095u, rw = (word >> 12) & 127u, off = word >> 19;
                    const uint32_t tp = slot >> 8, reg = (slot >> 6) & 3u, lane = slot & 63u;   // gemmSlabSlot
                    const uint32_t t = q * bsmr::kGemmPassTiles + tp;
                    if (t >= m * n || rw >= m * 16) return 12;
                    const uint32_t tm = t / n, tn = t % n, r = rw % 16;
                    if (rw / 16 != tm || reg != (r & 3u) || lane / 16 != r / 4) return 13;   // accumulator layout
                    const uint32_t c = lane & 15u;
                    const uint32_t rowInTile = wm * (TM / 2) + rw, colInTile = (wn * n + tn) * 16 + c;
                    const uint32_t idx = f.rowStart[it * TM + rowInTile] + off;
                    if (off >= bsmr::kGemmMaxOffset || idx >= d->nnz || seen[idx]++) return 14;
                    if (f.panelRows[(size_t)item.group * TM + rowInTile] != wantRow[idx]) return 15;
                    if (f.colOf[(size_t)item.firstBlock * 16 + colInTile] != wantCol[idx]) return 16;
                    const uint64_t key = ((uint64_t)rw << 32) | off;
                    if (i > b && key < lastKey) return 17;   // (row, position in P) order
                    lastKey = key;
                    ++itemEntries;
                    ++perStrip[item.firstBlock / NB];
                }
            }
        if (itemEntries == 0) return 18;   // macro-tiles without entries are not items
    }
    if (f.words.size() < expectStart + bsmr::kGemmWordSlack) return 19;
    for (uint32_t v = 0; v < d->nnz; ++v)
        if ((wantRow[v] != kNone) != (seen[v] != 0)) return 20;
    out[8] = *std::max_element(perStrip.begin(), perStrip.end());
    out[9] = *std::min_element(perStrip.begin(), perStrip.end());
    // where the natural order is lopsided (a natural strip above twice the mean), hot columns (more than twice the average
    // count) are dealt evenly and the others lie in natural order: no strip then holds more than its even share of the hot
    // entries (within two columns' worth) plus a full strip of columns at the threshold; otherwise the order is the natural one
    {
        const uint32_t S = f.numStrips, TN = NB * 16;
        uint64_t fullest = 0;
        for (uint32_t st = 0; st < S; ++st) {
            uint64_t sum = 0;
            for (uint64_t c = (uint64_t)st * TN; c < std::min<uint64_t>(d->N, (uint64_t)(st + 1) * TN); ++c) sum += degree[c];
            fullest = std::max(fullest, sum);
        }
        const bool lopsided = fullest * S > 2ull * denseEntries;
        out[10] = lopsided;
        const uint64_t threshold = 2ull * denseEntries / std::max<uint32_t>(1u, d->N) + 1ull;
        uint64_t hotEntries = 0;
        for (uint32_t c = 0; c < d->N; ++c)
            if (degree[c] > threshold) hotEntries += degree[c];
        if (balance && lopsided && out[8] > hotEntries / S + 2ull * maxDegree + (uint64_t)TN * threshold) return 26;
        if (balance && !lopsided)
            for (uint32_t c = 0; c < d->N; ++c)
                if (f.colOf[c] != c) return 27;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
#include "plan_evict.hpp"

// csrc/plan_evict.hpp on the host: packs `d` (default layout), evicts the outlier entries if a (block, row) is too wide for
// the 8-bit windows, packs again.  Checked here: every stored entry keeps its (panel, row in panel, column) and has exactly
// one place afterwards - a block cell or the residue -, the panels' column lists and block counts are unchanged, and no
// (new block, row) of the result spans kWindowMax or more.
// out[0] too wide before, [1] entries evicted, [2] too wide after, [3] tile bytes after (1 = 8-bit windows),
// [4] dense entries after, [5] residue entries after, [6] dense entries before.
extern "C" int plancheck_evict(const bsmr_rphm_desc* d, uint64_t* out) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    const uint32_t P = d->num_row_panels;
    bsmr::PackOptions opt;
    bsmr::PackedPlan before;
    if (bsmr::packPlan(d, opt, before) != BSMR_OK) return 1;
    out[0] = before.tooWide;
    out[6] = before.numDenseEntries;
    bsmr::EvictedRphm ev;
    if (bsmr::evictWideRows(d, ev) != BSMR_OK) return 2;
    out[1] = ev.evicted;
    const bsmr_rphm_desc* e = ev.evicted ? &ev.desc : d;
    // the place of every entry, before and after
    auto places = [&](const bsmr_rphm_desc* x, std::vector<uint64_t>& where, std::vector<uint8_t>& dense) -> int {
        where.assign(x->nnz, ~0ull);
        dense.assign(x->nnz, 0);
        for (uint32_t q = 0; q < P; ++q) {
            for (uint64_t b = x->block_offsets[q]; b < x->block_offsets[q + 1]; ++b)
                for (uint32_t i = 0; i < 256; ++i) {
                    const uint32_t v = x->block_values[b * 256 + i];
                    if (v == kNone) continue;
                    if (v >= x->nnz || where[v] != ~0ull) return 3;
                    where[v] = ((uint64_t)q << 40) | ((uint64_t)(i / 16) << 32) | x->dense_cols[b * 16 + i % 16];
                    dense[v] = 1;
                }
            for (uint32_t i = x->sparse_value_offsets[q]; i < x->sparse_value_offsets[q + 1]; ++i) {
                const uint32_t v = x->sparse_values[i];
                if (v >= x->nnz || where[v] != ~0ull) return 4;
                where[v] = ((uint64_t)q << 40) | ((uint64_t)x->sparse_relative_rows[i] << 32) | x->sparse_col_indices[i];
            }
        }
        return 0;
    };
    std::vector<uint64_t> w0, w1;
    std::vector<uint8_t> d0, d1;
    if (int rc = places(d, w0, d0)) return rc;
    if (int rc = places(e, w1, d1)) return rc + 10;
    uint64_t moved = 0;
    for (uint32_t v = 0; v < d->nnz; ++v) {
        if (w0[v] != w1[v]) return 5;
        if (d1[v] && !d0[v]) return 6;   // nothing becomes dense
        moved += d0[v] && !d1[v];
    }
    if (moved != ev.evicted) return 7;
    for (uint32_t q = 0; q <= P; ++q)
        if (e->block_offsets[q] != d->block_offsets[q]) return 8;
    for (uint64_t i = 0; i < (uint64_t)d->block_offsets[P] * 16; ++i)
        if (e->dense_cols[i] != d->dense_cols[i]) return 9;
    bsmr::PackedPlan after;
    if (bsmr::packPlan(e, opt, after) != BSMR_OK) return 20;
    out[2] = after.tooWide;
    out[3] = after.staged ? 1 : (after.tiles16.empty() ? 4 : 2);
    out[4] = after.numDenseEntries;
    out[5] = after.numSparseEntries;
    if (after.numDenseEntries + after.numSparseEntries != d->nnz) return 21;
    if (ev.evicted && after.numDenseEntries + ev.evicted != before.numDenseEntries) return 22;
    if (ev.evicted && after.numBlocks != before.numBlocks) return 23;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The streaming format (csrc/plan_pack.hpp: packPlan / packResidue) read the way denseStream, denseGroups and their
// fp32 / any-K / in-kernel-conversion siblings and the residue kernels read it (csrc/sddmm_kernels.hpp): every index a
// kernel forms stays inside its array, and every CSR index is reached exactly once, from the tile cell of its own row
// and column or from one residue entry.  The expected row and column of a CSR index come from the CSR itself.
namespace {

constexpr uint32_t kStreamNone = 0xFFFFFFFFu;

int streamEncoding(const bsmr::PackedPlan& pk) {
    return !pk.tilesMask.empty() ? 0 : !pk.tiles8.empty() ? 1 : !pk.tiles16.empty() ? 2 : !pk.tiles32.empty() ? 4 : 255;
}

// destination offset of accumulator element (lane, i) of tile t, as scatterTile decodes it; false: no entry
bool streamDecode(const bsmr::PackedPlan& pk, int enc, size_t t, uint32_t lane, uint32_t i, uint32_t& off) {
    const uint32_t g = lane >> 4, c = lane & 15u;
    if (enc == 0) {
        const uint32_t* w = &pk.tilesMask[t * 12 + g * 3];
        const uint32_t m = ((i < 2 ? w[0] : w[1]) >> (16 * (i & 1))) & 0xFFFFu;
        if (!((m >> c) & 1u)) return false;
        off = ((w[2] >> (8 * i)) & 0xFFu) + (uint32_t)__builtin_popcount(m & ((1u << c) - 1u));
        return true;
    }
    if (enc == 1) { off = pk.tiles8[t * 256 + lane * 4 + i]; return off != 0xFFu; }
    if (enc == 2) { off = pk.tiles16[t * 256 + lane * 4 + i]; return off != 0xFFFFu; }
    off = pk.tiles32[t * 256 + lane * 4 + i];
    return off != 0xFFFFFFFFu;
}

struct StreamPlace {   // where the dense part computes a CSR index: launch position of the item, block, lane, register
    uint32_t item = kStreamNone, block = kStreamNone, cell = kStreamNone;
    bool operator==(const StreamPlace& o) const { return item == o.item && block == o.block && cell == o.cell; }
};

// Returns 0 or the number of the first violated invariant (1 .. 33).
int streamCheck(const bsmr_rphm_desc* d, const uint32_t* ro, const uint32_t* ci, const bsmr::PackOptions& opt,
                const bsmr::PackedPlan& pk, std::vector<StreamPlace>& place) {
    const uint32_t H = pk.H, R = 16 * H, P = d->num_row_panels, G = pk.numGroups;
    const int enc = streamEncoding(pk);
    const bool windowed = enc == 0 || enc == 1;
    const size_t numItems = pk.denseItems.size(), NB = pk.numBlocks;
    place.assign(d->nnz, StreamPlace());
    std::vector<uint32_t> rowOf(d->nnz);
    for (uint32_t r = 0; r < d->M; ++r)
        for (uint32_t t = ro[r]; t < ro[r + 1]; ++t) rowOf[t] = r;
    // sizes of the arrays the kernels index
    if (H != (opt.group == 2 || opt.group == 4 ? (uint32_t)opt.group : 1u) || G != (P + H - 1) / H) return 1;
    if (pk.panelRows.size() != (size_t)P * 16 || pk.groupRows.size() != (size_t)G * R || pk.blockCols.size() != NB * 16 ||
        pk.blockMask.size() != NB)
        return 1;
    if (NB && enc == 255) return 1;
    if (enc != 255 && windowed != pk.staged) return 1;
    if (NB) {
        const size_t tiles = NB * H;
        const size_t have = enc == 0 ? pk.tilesMask.size() / 12 : enc == 1 ? pk.tiles8.size() / 256 : enc == 2 ? pk.tiles16.size() / 256 : pk.tiles32.size() / 256;
        if (have != tiles) return 1;
        if (pk.rowBase.size() != (windowed ? numItems : (size_t)G) * R) return 1;
        if (windowed && (pk.winLen.size() != numItems * R || pk.winMask.size() != numItems * R * (bsmr::kWindow / 32))) return 1;
    }
    for (const uint32_t row : pk.groupRows)
        if (row >= d->M) return 33;   // (padding rows of a ragged last group are gathered from A like any other)
    for (const uint32_t row : pk.panelRows)
        if (row >= d->M) return 33;
    // the blocks of every group, from the RPHM: its distinct dense columns, 16 to a block
    std::vector<uint64_t> groupFirst((size_t)G + 1, 0);
    {
        std::vector<uint32_t> stamp((size_t)d->N + 1, 0);
        for (uint32_t gi = 0; gi < G; ++gi) {
            uint64_t distinct = 0;
            for (uint32_t p = gi * H; p < std::min(P, (gi + 1) * H); ++p)
                for (uint64_t i = (uint64_t)d->block_offsets[p] * 16; i < (uint64_t)d->block_offsets[p + 1] * 16; ++i) {
                    const uint32_t col = d->dense_cols[i];
                    if (col >= d->N || stamp[col] == gi + 1) continue;
                    stamp[col] = gi + 1;
                    ++distinct;
                }
            groupFirst[gi + 1] = groupFirst[gi] + (distinct + 15) / 16;
        }
    }
    if (groupFirst[G] != NB) return 29;
    std::vector<uint8_t> seen(d->nnz, 0), blockSeen(NB, 0);
    uint64_t dense = 0;
    std::vector<uint8_t> own((size_t)R * 256);
    for (size_t it = 0; it < numItems; ++it) {
        const bsmr::DenseItem& item = pk.denseItems[it];
        if (item.count == 0 || item.group >= G || (uint64_t)item.first + item.count > NB) return 2;
        if (item.count > (uint32_t)std::max(1, opt.blocksPerItem)) return 3;
        if (item.first < groupFirst[item.group] || (uint64_t)item.first + item.count > groupFirst[item.group + 1]) return 29;
        std::fill(own.begin(), own.end(), (uint8_t)0);
        for (uint32_t b = item.first; b < item.first + item.count; ++b) {
            if (blockSeen[b]++) return 4;
            if (opt.itemSpan && pk.blockCols[(size_t)b * 16] / opt.itemSpan != pk.blockCols[(size_t)item.first * 16] / opt.itemSpan) return 30;
            for (uint32_t c = 0; c < 16; ++c)
                if (pk.blockCols[(size_t)b * 16 + c] >= d->N) return 5;
            for (uint32_t k = 0; k < H; ++k) {
                const bool masked = (pk.blockMask[b] >> k) & 1u;
                const size_t t = (size_t)b * H + k;
                uint32_t got = 0;
                for (uint32_t lane = 0; lane < 64; ++lane)
                    for (uint32_t i = 0; i < 4; ++i) {
                        uint32_t off = 0;
                        if (!streamDecode(pk, enc, t, lane, i, off)) continue;
                        ++got;
                        if (!masked) return 6;   // denseGroups and the one-wave kernels skip the tile: the entry is never computed
                        const uint32_t row = k * 16 + 4 * (lane >> 4) + i, c = lane & 15u;
                        uint64_t base;
                        if (windowed) {
                            const size_t slot = it * R + row;
                            base = pk.rowBase[slot];
                            if (off >= bsmr::kWindowMax || off >= pk.winLen[slot]) return 7;
                            if (!((pk.winMask[slot * 8 + off / 32] >> (off % 32)) & 1u)) return 8;   // the LDS-staged form would not store it
                            if (own[(size_t)row * 256 + off]++) return 9;
                        } else {
                            base = pk.rowBase[(size_t)item.group * R + row];
                        }
                        const uint64_t idx = base + off;
                        if (idx >= d->nnz) return 10;
                        if (pk.groupRows[(size_t)item.group * R + row] != rowOf[idx]) return 12;
                        if (pk.blockCols[(size_t)b * 16 + c] != ci[idx]) return 13;
                        if (seen[idx]++) return 11;
                        place[idx].item = (uint32_t)it;
                        place[idx].block = b;
                        place[idx].cell = (k << 8) | (lane << 2) | i;
                        ++dense;
                    }
                if (masked && !got) return 14;
            }
        }
        if (windowed)
            for (uint32_t row = 0; row < R; ++row) {
                const size_t slot = it * R + row;
                const uint32_t len = pk.winLen[slot];
                if (len > bsmr::kWindowMax) return 15;
                if (len && (uint64_t)pk.rowBase[slot] + len > d->nnz) return 16;
                for (uint32_t j = 0; j < bsmr::kWindow; ++j) {
                    const bool bit = (pk.winMask[slot * 8 + j / 32] >> (j % 32)) & 1u;
                    if (bit && j >= len) return 18;
                    if (bit != (own[(size_t)row * 256 + j] != 0)) return 17;   // a bit nobody wrote: stale LDS would reach P
                }
            }
    }
    for (size_t b = 0; b < NB; ++b)
        if (!blockSeen[b]) return 19;
    if (dense != pk.numDenseEntries) return 20;
    // the residue, as residueEntries - the one body of sparseEntries and sparseEntriesLowp - walks it
    const uint64_t numSparse = pk.numSparseEntries;
    if (pk.entryCol.size() != numSparse || pk.entryDst.size() != numSparse ||
        (pk.freeResidue ? pk.entryRowId.size() : pk.entryRow.size()) != numSparse)
        return 1;
    uint64_t sparse = 0;
    std::vector<uint8_t> entrySeen(numSparse, 0);
    for (const bsmr::SparseItem& item : pk.sparseItems) {
        if (item.count == 0 || item.count > (uint32_t)std::max(32, opt.sparsePerItem) || (uint64_t)item.start + item.count > numSparse) return 21;
        if (pk.freeResidue ? item.panel != kStreamNone : item.panel >= P) return pk.freeResidue ? 23 : 24;
        for (uint32_t e = item.start; e < item.start + item.count; ++e) {
            if (entrySeen[e]++) return 22;
            uint32_t row;
            if (pk.freeResidue) {
                row = pk.entryRowId[e];
            } else {
                if (pk.entryRow[e] >= 16) return 24;
                row = pk.panelRows[(size_t)item.panel * 16 + pk.entryRow[e]];
            }
            const uint32_t idx = pk.entryDst[e];
            if (idx >= d->nnz || seen[idx]) return 25;
            seen[idx] = 1;
            if (rowOf[idx] != row || ci[idx] != pk.entryCol[e] || pk.entryCol[e] >= d->N) return 26;
            ++sparse;
        }
    }
    if (sparse != numSparse) return 27;
    for (uint32_t v = 0; v < d->nnz; ++v)
        if (seen[v] != 1) return 28;
    return 0;
}

// One deliberate defect in a packed plan (the proof that streamCheck can fail).  Returns false where the plan offers no
// place for it.
bool streamMutate(bsmr::PackedPlan& pk, int mutate) {
    const uint32_t H = pk.H, R = 16 * H;
    const int enc = streamEncoding(pk);
    const bool windowed = enc == 0 || enc == 1;
    const size_t numItems = pk.denseItems.size(), NB = pk.numBlocks;
    switch (mutate) {
    case 1:   // two offsets of one 8-bit tile row change places
        if (enc != 1) return false;
        for (size_t t = 0; t < NB * H; ++t)
            for (uint32_t row = 0; row < 16; ++row) {
                int first = -1;
                for (uint32_t c = 0; c < 16; ++c) {
                    const size_t at = t * 256 + ((row >> 2) * 16 + c) * 4 + (row & 3);
                    if (pk.tiles8[at] == 0xFF) continue;
                    if (first < 0) { first = (int)at; continue; }
                    std::swap(pk.tiles8[(size_t)first], pk.tiles8[at]);
                    return true;
                }
            }
        return false;
    case 2:   // a set blockMask bit cleared
        for (size_t b = 0; b < NB; ++b)
            if (pk.blockMask[b]) { pk.blockMask[b] &= (uint8_t)(pk.blockMask[b] - 1); return true; }
        return false;
    case 3:   // a clear blockMask bit (of a panel the kernels look at) set
        for (size_t b = 0; b < NB; ++b)
            for (uint32_t k = 0; k < H; ++k)
                if (!((pk.blockMask[b] >> k) & 1u)) { pk.blockMask[b] |= (uint8_t)(1u << k); return true; }
        return false;
    case 4:   // a winMask bit inside a window that no tile of the item writes
        if (!windowed) return false;
        for (size_t slot = 0; slot < numItems * R; ++slot)
            for (uint32_t j = 0; j < pk.winLen[slot]; ++j)
                if (!((pk.winMask[slot * 8 + j / 32] >> (j % 32)) & 1u)) { pk.winMask[slot * 8 + j / 32] |= 1u << (j % 32); return true; }
        return false;
    case 5:   // an owned winMask bit cleared
        if (!windowed) return false;
        for (size_t w = 0; w < pk.winMask.size(); ++w)
            if (pk.winMask[w]) { pk.winMask[w] &= pk.winMask[w] - 1; return true; }
        return false;
    case 6:   // a window one position shorter
        if (!windowed) return false;
        for (size_t slot = 0; slot < numItems * R; ++slot)
            if (pk.winLen[slot]) { --pk.winLen[slot]; return true; }
        return false;
    case 7:   // a window base one entry further (a window of two or more entries: the shifted indices stay inside the CSR row)
        if (!windowed) return false;
        for (size_t slot = 0; slot < numItems * R; ++slot)
            if (pk.winLen[slot] >= 2) { ++pk.rowBase[slot]; return true; }
        return false;
    case 8:   // two columns of a block change places (the first two: every stored column holds an entry)
        for (size_t b = 0; b < NB; ++b)
            if (pk.blockCols[b * 16] != pk.blockCols[b * 16 + 1]) { std::swap(pk.blockCols[b * 16], pk.blockCols[b * 16 + 1]); return true; }
        return false;
    case 9: { // two rows of a group change places: the rows of the first entry the dense part holds and of its neighbour
        for (size_t it = 0; it < numItems; ++it) {
            const bsmr::DenseItem& item = pk.denseItems[it];
            for (uint32_t b = item.first; b < item.first + item.count; ++b)
                for (uint32_t k = 0; k < H; ++k)
                    for (uint32_t lane = 0; lane < 64; ++lane)
                        for (uint32_t i = 0; i < 4; ++i) {
                            uint32_t off;
                            if (!streamDecode(pk, enc, (size_t)b * H + k, lane, i, off)) continue;
                            const size_t row = (size_t)item.group * R + k * 16 + 4 * (lane >> 4) + i, other = row ^ 1u;
                            if (pk.groupRows[row] == pk.groupRows[other]) continue;
                            std::swap(pk.groupRows[row], pk.groupRows[other]);
                            return true;
                        }
        }
        return false;
    }
    case 10: {  // the per-item arrays of two items of one group change places (a wrong permutation in the item sort)
        if (!windowed) return false;
        for (size_t a = 0; a < numItems; ++a)
            for (size_t b = a + 1; b < numItems; ++b) {
                if (pk.denseItems[a].group != pk.denseItems[b].group) continue;
                if (std::equal(pk.rowBase.begin() + a * R, pk.rowBase.begin() + (a + 1) * R, pk.rowBase.begin() + b * R)) continue;
                std::swap_ranges(pk.rowBase.begin() + a * R, pk.rowBase.begin() + (a + 1) * R, pk.rowBase.begin() + b * R);
                std::swap_ranges(pk.winLen.begin() + a * R, pk.winLen.begin() + (a + 1) * R, pk.winLen.begin() + b * R);
                std::swap_ranges(pk.winMask.begin() + a * R * 8, pk.winMask.begin() + (a + 1) * R * 8, pk.winMask.begin() + b * R * 8);
                return true;
            }
        return false;
    }
    case 11:  // a residue entry repeated in place of its neighbour
        for (const bsmr::SparseItem& item : pk.sparseItems) {
            if (item.count < 2) continue;
            const uint32_t e = item.start;
            if (pk.entryDst[e + 1] == pk.entryDst[e]) continue;
            pk.entryDst[e + 1] = pk.entryDst[e];
            pk.entryCol[e + 1] = pk.entryCol[e];
            if (pk.freeResidue) pk.entryRowId[e + 1] = pk.entryRowId[e];
            else pk.entryRow[e + 1] = pk.entryRow[e];
            return true;
        }
        return false;
    case 12:  // mask form: the first offset of a tile row with two or more entries, plus one
    case 13:  // mask form: one bit of a tile row's column mask moved to the free column next to it
        if (enc != 0) return false;
        for (size_t t = 0; t < NB * H; ++t)
            for (uint32_t row = 0; row < 16; ++row) {
                uint32_t* w = &pk.tilesMask[t * 12 + (row >> 2) * 3];
                const uint32_t i = row & 3u, shift = 16 * (i & 1);
                uint32_t& word = i < 2 ? w[0] : w[1];
                const uint32_t m = (word >> shift) & 0xFFFFu;
                if (mutate == 12) {
                    if (__builtin_popcount(m) < 2 || ((w[2] >> (8 * i)) & 0xFFu) >= 0xFEu) continue;
                    w[2] += 1u << (8 * i);
                    return true;
                }
                const size_t b = t / H;
                for (uint32_t c = 0; c + 1 < 16; ++c)
                    if (((m >> c) & 3u) == 1u && pk.blockCols[b * 16 + c] != pk.blockCols[b * 16 + c + 1]) {
                        word ^= 3u << (shift + c);
                        return true;
                    }
            }
        return false;
    default: return false;
    }
}

// FNV-1a over every array of the plan a kernel reads
uint64_t streamDigest(const bsmr::PackedPlan& pk) {
    uint64_t h = 0xcbf29ce484222325ull;
    auto add = [&h](const void* ptr, size_t bytes) {
        const uint8_t* b = static_cast<const uint8_t*>(ptr);
        for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    };
    auto vec = [&add](const auto& v) { add(v.data(), v.size() * sizeof(v[0])); };
    vec(pk.panelRows); vec(pk.groupRows); vec(pk.rowBase); vec(pk.winLen); vec(pk.winMask); vec(pk.blockCols);
    vec(pk.tiles8); vec(pk.tilesMask); vec(pk.tiles16); vec(pk.tiles32); vec(pk.blockMask); vec(pk.denseItems);
    vec(pk.entryCol); vec(pk.entryDst); vec(pk.entryRow); vec(pk.entryRowId); vec(pk.sparseItems);
    return h;
}

}  // namespace

// options: [0] group, [1] blocksPerItem, [2] sparsePerItem, [3] forceWideTiles, [4] columnOrder, [5] staged, [6] maskTiles,
// [7] freeResidue, [8] itemOrder, [9] orderWindow, [10] itemSpan (the fields of bsmr::PackOptions).  promote / evict: run
// promoteSparseBlocks (a panel's residue averaging 16 entries per block, no other condition) / evictWideRows on the arrays
// first.  mutate: 0, or one of streamMutate's defects, applied between packing and checking.
// out[0] encoding (0 mask form, 1 8-bit windows, 2 / 4 bytes per direct offset, 255 no dense tiles), [1] dense items,
// [2] blocks, [3] dense entries, [4] residue entries, [5] residue items, [6] staged, [7] tooWide, [8] promoted entries,
// [9] evicted entries, [10] the mutation changed the plan (a digest of its arrays before and after), [11] packPlan status, [12] blocks of the largest dense item.
// Returns 0; 1 .. 33 the first violated invariant (streamCheck); 31 the mask form and the 8-bit form of the same options
// disagree on where an entry is computed, 32 the 8-bit form itself is wrong; 200 + status when packPlan refuses the arrays;
// 300 + status from evictWideRows; 900 when the plan has no place for the mutation.
extern "C" int plancheck_stream(const bsmr_rphm_desc* d, const uint32_t* rowOffsets, const uint32_t* colIndices, const int32_t* options,
                                int promote, int evict, int mutate, uint64_t* out) {
    bsmr::PackOptions opt;
    opt.group = options[0];
    opt.blocksPerItem = options[1];
    opt.sparsePerItem = options[2];
    opt.forceWideTiles = options[3] != 0;
    opt.columnOrder = options[4] != 0;
    opt.staged = options[5] != 0;
    opt.maskTiles = options[6] != 0;
    opt.freeResidue = options[7];
    opt.itemOrder = options[8];
    opt.orderWindow = (uint32_t)options[9];
    opt.itemSpan = (uint32_t)options[10];
    for (int i = 0; i < 13; ++i) out[i] = 0;
    bsmr::PromotedRphm pr;
    bsmr::EvictedRphm ev;
    if (promote && bsmr::promoteSparseBlocks(*d, 16, 0, 0, 0, 0, pr)) {
        d = &pr.desc;
        out[8] = pr.promotedEntries;
    }
    if (evict) {
        if (const int st = bsmr::evictWideRows(d, ev)) return 300 + st;
        if (ev.evicted) d = &ev.desc;
        out[9] = ev.evicted;
    }
    bsmr::PackedPlan pk;
    const int st = bsmr::packPlan(d, opt, pk);
    out[11] = (uint64_t)(int64_t)st;
    if (st != BSMR_OK) return 200 + st;
    out[0] = (uint64_t)streamEncoding(pk);
    out[1] = pk.denseItems.size();
    out[2] = pk.numBlocks;
    out[3] = pk.numDenseEntries;
    out[4] = pk.numSparseEntries;
    out[5] = pk.sparseItems.size();
    out[6] = pk.staged;
    out[7] = pk.tooWide;
    for (const bsmr::DenseItem& item : pk.denseItems) out[12] = std::max<uint64_t>(out[12], item.count);
    if (mutate) {
        const uint64_t before = streamDigest(pk);
        if (!streamMutate(pk, mutate)) return 900;
        out[10] = streamDigest(pk) != before;   // the defect really is in the arrays the check reads
        if (!out[10]) return 900;
    }
    std::vector<StreamPlace> place;
    if (const int rc = streamCheck(d, rowOffsets, colIndices, opt, pk, place)) return rc;
    if (streamEncoding(pk) == 0) {   // the same options without the mask form: the same place for every entry
        bsmr::PackOptions plain = opt;
        plain.maskTiles = false;
        bsmr::PackedPlan pk8;
        if (bsmr::packPlan(d, plain, pk8) != BSMR_OK || streamEncoding(pk8) != 1) return 32;
        std::vector<StreamPlace> place8;
        if (streamCheck(d, rowOffsets, colIndices, plain, pk8, place8)) return 32;
        if (!(place == place8)) return 31;
    }
    return 0;
}
