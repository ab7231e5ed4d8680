/*
 * bsmr_hip.h -- C ABI of libbsmr_hip.so, the MI355X (gfx950) device side of the
 * BSMR-SDDMM engine.
 *
 * This is the drop-in boundary for the reference's device layer.  What it
 * replaces in CX9898/BSMR-SDDMM (paths relative to the reference checkout):
 *
 *   bsmr_plan_create     <- the twelve h2d() uploads at the end of RPHM::RPHM
 *                           (src/BSMR.cpp:252-264); takes the same host arrays
 *                           the reference's RPHM holds (include/BSMR.hpp:133-158)
 *   bsmr_plan_create_ex  <- the same with every construction rule passed explicitly (bsmr_plan_options)
 *   bsmr_plan_destroy    <- ~RPHM / dev::vector destructors (include/devVector.cuh:54-126)
 *   bsmr_sddmm           <- sddmm_gpu(M,N,K, A_dev, B_dev, rphm, P_dev, logger) and
 *                           sddmm_gpu_k32(...) (include/sddmmKernel.cuh:25-39,
 *                           src/sddmmKernel.cu:2540-2762): device pointers in,
 *                           P written in S's CSR order
 *   bsmr_sddmm_timed     <- the 10x event-timed loop inside those launchers
 *                           (src/sddmmKernel.cu:2561-2565,2650-2653)
 *   bsmr_sddmm_host      <- sddmm_gpu(Matrix A, Matrix B, rphm, CSR P, logger)
 *                           (src/sddmmKernel.cu:2518-2538): host operands in, host P out
 *   bsmr_sddmm_batch / bsmr_batched_transpose
 *                        <- sddmm_gpu_batch / batchedMatrixTranspose (include/sddmmKernel.cuh:41-51,
 *                           src/sddmmKernel.cu:2764-2869, 2486-2515)
 *   bsmr_cluster_rows    <- bsa_rowReordering_gpu (src/rowReordering.cu:1027-1095): the row
 *                           clustering on the device, same row order and cluster count
 *   bsmr_col_reorder*    <- colReordering_cpu + the index arrays of RPHM::RPHM (src/colReordering.cu:274-404,
 *                           src/BSMR.cpp:83-265) on the device; the reference's colReordering_gpu (:146-241) is unfinished
 *   bsmr_convert_operands / bsmr_sddmm_lowp
 *                        <- no reference counterpart (the reference converts to
 *                           TF32 in registers); lets a caller that already holds
 *                           fp16/bf16 operands skip the per-call conversion
 *   bsmr_sharded_*       <- no reference counterpart (the reference is single-GPU): row-range shards over the
 *                           GPUs of one node, one RCCL gather-v of P per step
 *   bsmr_backward_*      <- no reference counterpart (the reference has no backward): a per-pattern handle with S's
 *                           CSR, its transpose and the chunked work lists of dA = S_dP B and dB = S_dP^T A
 *   bsmr_csr_transpose   <- no reference counterpart: the host transpose bsmr_backward_create uploads
 *   bsmr_spmm / bsmr_sddmm_backward
 *                        <- no reference counterpart: Y = S_v X / S_v^T X and the two SDDMM gradients
 *   bsmr_spmm_mode / bsmr_sddmm_backward_mode / bsmr_spmm_lowp / bsmr_backward_reserve_mode
 *                        <- no reference counterpart: the same products with the gathered operand read as fp16 / bf16 rows
 *   bsmr_sddmm_16 / bsmr_spmm_16 / bsmr_sddmm_backward_16
 *                        <- no reference counterpart: the forward, the SpMM and the two gradients for a caller that holds
 *                           fp16 / bf16 tensors only - 16-bit operands in, 16-bit Y / dA / dB out, the values stay fp32
 *   bsmr_sparse_softmax / bsmr_sparse_softmax_backward
 *                        <- no reference counterpart: the row softmax over S's pattern and its gradient
 *   bsmr_blocked_check[_split] / bsmr_backward_attach_blocks[_split] / bsmr_spmm_blocked / bsmr_spmm_blocked_16
 *                        <- no reference counterpart: Y = S_v X over the RPHM's dense 16 x 16 blocks on the fp32 MFMA
 *   bsmr_mem_info        <- cudaMemGetInfo in calculateBlockSize (src/rowReordering.cu:1010-1013)
 *   bsmr_dev_alloc / bsmr_dev_free / bsmr_memcpy_h2d / bsmr_memcpy_d2h / bsmr_dev_memset
 *                        <- dev::vector<T> ctor/dtor and h2d()/d2h() (include/devVector.cuh:54-126,
 *                           170-229): raw device buffers owned by the caller
 *
 * Only PODs and raw pointers cross.  Every function returns a status code and
 * never throws or aborts.  A plan is bound to one device; calls on one plan
 * must come from one thread at a time.  `stream` is a hipStream_t passed as
 * void* (NULL = the default stream); all device work of a call is ordered on it.
 */
#ifndef BSMR_HIP_H
#define BSMR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSMR_OK                 0
#define BSMR_ERR_INVALID_ARG    1  /* NULL or misaligned pointer, inconsistent sizes */
#define BSMR_ERR_NO_DEVICE      2  /* no usable gfx950 device / bad device index  */
#define BSMR_ERR_HIP            3  /* a HIP runtime call failed (see last error)  */
#define BSMR_ERR_UNSUPPORTED_K  4  /* K == 0 or K not a multiple of 32            */
#define BSMR_ERR_OOM            5  /* host or device allocation failed            */
#define BSMR_ERR_BAD_PLAN       6  /* index arrays violate the RPHM invariants    */

/* Arithmetic of the dense-block path (the sparse residual path is always fp32). */
#define BSMR_COMPUTE_F16   0  /* operands rounded RNE to fp16, fp32 accumulate (default;
                                 same 10-bit mantissa as the reference's TF32)       */
#define BSMR_COMPUTE_BF16  1  /* operands rounded RNE to bf16, fp32 accumulate         */
#define BSMR_COMPUTE_F32   2  /* exact fp32 (v_mfma_f32_16x16x4_f32), 1/16 MFMA rate   */

typedef struct bsmr_plan bsmr_plan;

/* Host-side index arrays of one reordered matrix: exactly the members of the
 * reference's RPHM before upload.  All arrays are read during plan_create and
 * need not outlive it. */
typedef struct bsmr_rphm_desc {
    uint32_t M, N, nnz;
    uint32_t num_row_panels;          /* ceil(num_nonzero_rows / 16)                          */
    uint32_t num_nonzero_rows;        /* length of reordered_rows                             */
    const uint32_t *reordered_rows;   /* [num_nonzero_rows] original row of each panel row    */
    const uint32_t *dense_cols;       /* [16 * block_offsets[P]] column ids, N = padding      */
    const uint32_t *block_offsets;    /* [P+1] dense 16x16 blocks before each panel           */
    const uint32_t *block_values;     /* [256 * block_offsets[P]] CSR index or 0xFFFFFFFF,
                                         row-major 16x16 per block                            */
    const uint32_t *sparse_value_offsets; /* [P+1] sparse entries before each panel           */
    const uint32_t *sparse_values;        /* CSR index of each sparse entry                   */
    const uint32_t *sparse_relative_rows; /* row inside the panel, 0..15                      */
    const uint32_t *sparse_col_indices;   /* column id                                        */
} bsmr_rphm_desc;

typedef struct bsmr_plan_stats {
    uint32_t num_row_panels;
    uint64_t num_dense_blocks;    /* 16-column blocks of the grouped device format */
    uint64_t num_dense_entries;   /* nnz covered by the dense path  */
    uint64_t num_sparse_entries;  /* nnz covered by the sparse path */
    uint64_t dense_work_items;    /* waves launched by the dense kernel        */
    uint64_t sparse_work_items;   /* workgroups launched by the sparse kernel  */
    uint64_t device_index_bytes;  /* bytes of plan metadata resident in HBM    */
    uint32_t group_size;          /* row panels whose dense columns share one B gather (1, 2, 4) */
    uint64_t num_dense_tiles;     /* non-empty 16x16 (panel, block) tiles = MFMA tiles executed   */
    uint64_t union_columns;       /* B columns gathered per SDDMM by the dense path               */
    /* second dense format (4 panels per group) kept for gather-bound calls; 0 = not built */
    uint32_t grouped_group_size;
    uint64_t grouped_dense_tiles;
    uint64_t grouped_union_columns;
    uint64_t sparse_lowp;             /* 1: in the F16/BF16 modes the residue reads the converted operands too (for every K;
                                       * bsmr_plan_sparse_choice reports calls that do so from a K upwards) */
    uint64_t folded_dense_entries;    /* entries of a small dense part (RPHM) that the plan computes with the residue */
    uint64_t free_residue;            /* 1: residue entries run in global column order, not per panel */
    uint64_t promoted_sparse_entries; /* residue entries (RPHM) that the plan computes as extra dense blocks */
} bsmr_plan_stats;

/* 1 when the promotion rule of this plan ran as kernels (bsmr_plan_options.promote_on_device), 0 when on the host. */
int bsmr_plan_promoted_on_device(const bsmr_plan *plan, int *yes);

/* Kernel timings of the last bsmr_sddmm_timed call, milliseconds per iteration. */
typedef struct bsmr_timing {
    float total_ms;    /* convert + dense + sparse, wall on the stream          */
    float convert_ms;  /* fp32 -> fp16/bf16 operand pass (0 in F32 mode)        */
    float dense_ms;    /* dense-block MFMA kernel                               */
    float sparse_ms;   /* residual sparse kernel                                */
} bsmr_timing;

const char *bsmr_strerror(int status);
/* Text of the last HIP error seen by this library on the calling thread. */
const char *bsmr_last_hip_error(void);

int bsmr_device_count(int *count);
int bsmr_mem_info(int device, size_t *free_bytes, size_t *total_bytes);
int bsmr_device_name(int device, char *buf, size_t buflen);

/* Caller-owned device buffers on `device` (synchronous copies). */
int bsmr_dev_alloc(int device, size_t bytes, void **out);
int bsmr_dev_free(void *ptr);
int bsmr_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int bsmr_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
int bsmr_dev_memset(void *dst_dev, int value, size_t bytes);
int bsmr_device_synchronize(int device);

/* Every rule of plan construction that is not a function of the RPHM arrays.  Zero-initialise, call
 * bsmr_plan_options_default, change what is needed, pass to bsmr_plan_create_ex: a plan's layout, kernels and
 * precision class are then a function of (desc, options) alone.  Fields named like the BSMR_<NAME> environment
 * variables of bsmr_plan_options_from_env (the override used by tests, the CLI and bsmr_plan_create). */
#define BSMR_ENGINE_STREAM  0  /* dense part: per-panel streaming kernels (denseStream / denseGroups), the default */
#define BSMR_ENGINE_TILES   1  /* dense part: "tiles" format, H panels per wave-private B image (denseTiles)     */
#define BSMR_ENGINE_SHARED  2  /* dense part: "tiles" format, B images shared by the 4 waves of a workgroup        */
#define BSMR_ENGINE_SWEEP   4  /* dense part computed like a GEMM: row groups x strips of B in natural column order,
                                  B streamed once by loader waves, no gather (denseSweep, csrc/sweep_kernels.hpp)  */
#define BSMR_ENGINE_GEMM    5  /* dense part as an output-stationary masked GEMM (round 4): a workgroup owns a macro-tile of C
                                  (row panels x natural 16-column blocks), accumulators stay in registers over the K loop,
                                  A rows and B columns arrive K-slice by K-slice through an LDS double buffer, every wave
                                  multiplies an m x n block of 16 x 16 tiles (denseGemm, csrc/gemm_kernels.hpp)           */
#define BSMR_ENGINE_TUNED   3  /* the plan keeps what every engine needs; calls use the streaming engine until
                                  bsmr_plan_tune has timed the three for their (K, mode) and then the fastest          */
typedef struct bsmr_plan_options {
    uint32_t struct_size;           /* sizeof(bsmr_plan_options) of the caller                                        */
    int32_t  dense_engine;          /* BSMR_ENGINE_*                                                    [DENSE_ENGINE] */
    /* which kernel computes an entry (the RPHM's own dense / sparse split is never changed) */
    int32_t  fold_dense_below;      /* a dense part with fewer entries runs with the residue (32768)  [FOLD_DENSE_BELOW] */
    int32_t  promote_average;       /* residue -> extra dense blocks when a panel averages this many
                                       entries per 16 columns (16; 0 = never)                          [PROMOTE_AVERAGE] */
    int32_t  promote_min_entries_k; /* ... plans without a dense part: only if this many thousand move (1000) [PROMOTE_MIN_ENTRIES_K] */
    int32_t  promote_column_degree; /* ... only patterns with nnz / N at least this (32)          [PROMOTE_COLUMN_DEGREE] */
    int32_t  promote_head;          /* ... leading blocks of other panels with this many entries (0 = none) [PROMOTE_HEAD] */
    /* device format of the dense part, streaming engine */
    int32_t  dense_group;           /* panels per group: 0 = both formats, chosen per call; 1, 2, 4        [DENSE_GROUP] */
    int32_t  dense_blocks_per_item; /* 0 = from the plan's shape                                  [DENSE_BLOCKS_PER_WG] */
    int32_t  stream_waves;          /* 1 or 4 waves per workgroup of denseStream (1)                       [STREAM_WAVES] */
    int32_t  output_mode;           /* 0 = 16/32-bit offsets, 1 = 8-bit windows (default), 2 = windows staged in LDS [OUTPUT_MODE] */
    int32_t  force_tile32;          /* 32-bit destination tiles                                            [FORCE_TILE32] */
    int32_t  column_order;          /* blocks / items / residue in column order (1)                        [COLUMN_ORDER] */
    int32_t  dense_stream;          /* streaming kernel for ungrouped formats (1)                          [DENSE_STREAM] */
    int32_t  dense_batch;           /* blocks per LDS batch of denseGroups at K = 128 (0 = 4)               [DENSE_BATCH] */
    /* device format of the dense part, tiles / shared engines */
    int32_t  tile_group;            /* panels per group, 0 = cost model                                      [TILE_GROUP] */
    int32_t  tile_blocks_per_item;  /* 0 = from the plan's shape                                            [TILE_BLOCKS] */
    int32_t  tile_depth;            /* ring depth of denseTiles, 0 = default                                 [TILE_DEPTH] */
    /* residue */
    int32_t  sparse_entries_per_item; /* (256)                                                [SPARSE_ENTRIES_PER_WG] */
    int32_t  sparse_lowp;           /* residue from the fp16/bf16 copies whenever they exist (1)             [SPARSE_LOWP] */
    int32_t  sparse_lpe;            /* lanes per entry: 0 = tuned shape per K; 4, 8, 16                        [SPARSE_LPE] */
    int32_t  free_residue;          /* 1: entries in global column order instead of per panel (0)          [FREE_RESIDUE] */
    /* operand conversion */
    int32_t  convert_in_kernel;     /* -1 = by size of the dense part; 0 / 1                           [CONVERT_IN_KERNEL] */
    int32_t  convert_sliced;        /* B converted by the XCD that gathers it while it fits the L2s (1)  [CONVERT_SLICED] */
    int32_t  b_only;                /* plans without a dense part may convert B alone (1)                         [B_ONLY] */
    int32_t  b_only_work_m;         /* ... from this many million residue entries x K (100)                [B_ONLY_WORK_M] */
    /* launch */
    int32_t  overlap_streams;       /* dense and residue kernels of a hybrid plan on two streams joined by events:
                                       -1 = when both parts are large enough, 0 = never, 1 = always      [OVERLAP_STREAMS] */
    int32_t  mask_tiles;            /* destination tiles as 16-bit column masks + first offsets (48 instead of 256 bytes
                                       per tile; needs consecutive entries per tile row): 1 = whenever possible, 0 = never,
                                       -1 = when the 8-bit tiles would exceed the 32 MiB of L2 (default)     [MASK_TILES] */
    /* plan build */
    int32_t  pack_on_device;        /* the dense part's device format built by kernels from the uploaded RPHM arrays
                                       (csrc/pack_device.hpp; byte-identical to the host packer, which still does every
                                       layout but the default one): 1 = whenever possible, 0 = never,
                                       -1 = from 4096 dense blocks (default)                               [PACK_ON_DEVICE] */
    /* device format of the dense part, sweep engine (fields added in round 3: older callers' struct_size leaves the defaults) */
    int32_t  sweep_panels;          /* panels per consumer wave (a row group is 4 x this many panels): 0 = by K; 1, 2, 4
                                                                                                              [SWEEP_PANELS] */
    int32_t  sweep_strip_blocks;    /* 16-column blocks of B per work item: 0 = from the plan's shape; <= 63   [SWEEP_BLOCKS] */
    int32_t  sweep_fp32;            /* sweep kernel on the caller's fp32 operands, rounded in registers (no conversion
                                       pass; a residue then runs its fp32 kernel): -1 = for K <= 128 when the plan has no
                                       residue (default), 0 = never, 1 = whenever K <= 128                     [SWEEP_FP32] */
    int32_t  sweep_waves;           /* consumer waves per workgroup: 0 = 4; 4, 8                                [SWEEP_WAVES] */
    int32_t  sweep_per_cu;          /* workgroups per CU the LDS ring is sized for: 0 = 1; 1, 2 (2: four consumer waves only)
                                                                                                              [SWEEP_PER_CU] */
    int32_t  k_hint;                /* 0 (default): the plan-time rules above (promotion of the residue, folding of a small
                                       dense part) are thresholds fitted once, K unknown.  > 0: the inner dimension the plan
                                       will mostly be called with - the plan keeps a copy of the RPHM arrays, and
                                       bsmr_plan_tune builds it under the other settings of those rules too
                                       (BSMR_VARIANT_*), times whole calls and lets the fastest serve the plan  [K_HINT] */
    int32_t  promote_on_device;     /* the promotion rule as kernels (csrc/promote_device.hpp), its blocks handed to the device
                                       packer without crossing PCIe: -1 = from 2^20 residue entries when the plan's layout
                                       and engine allow, 0 = never, 1 = whenever they allow.  Same plan, byte for byte
                                                                                                         [PROMOTE_ON_DEVICE] */
    /* device format of the dense part, GEMM engine (fields added in round 4) */
    int32_t  gemm_panels;           /* row panels per macro-tile: 0 = from the plan's shape (a model of the launch's rounds);
                                       8, 16                                                                   [GEMM_PANELS] */
    int32_t  gemm_blocks;           /* 16-column blocks of B per macro-tile: 0 = from the plan's shape; 12, 16, 20 (with 16
                                       panels), 16, 20 (with 8)                                                 [GEMM_BLOCKS] */
    int32_t  gemm_fp32;             /* GEMM kernel on the caller's fp32 operands, rounded in registers (K = 64, 128; no
                                       conversion pass; a residue then runs its fp32 kernel): -1 = when the plan has no
                                       residue (default), 0 = never, 1 = whenever K allows                        [GEMM_FP32] */
    int32_t  gemm_balance_columns;  /* 1 (default): the columns of B are dealt over the column strips by their number of dense
                                       entries, so that every macro-tile's mask epilogue holds about as many entries (hot
                                       columns - graphs, bag-of-words - otherwise gather in a few macro-tiles the launch waits
                                       for); 0: natural column order                                   [GEMM_BALANCE_COLUMNS] */
    int32_t  evict_wide_rows;       /* 1 (default): when a (block, row) of the dense part spans 255 or more entries of its row
                                       (a long row with many residue entries between two dense columns of its panel), the
                                       entries outside the densest window of 254 become residue, so that the plan keeps
                                       its 8-bit tiles; only while that moves at most 1 / 16 of the dense entries.  0: such
                                       a plan takes direct 16-bit offsets for all blocks                  [EVICT_WIDE_ROWS] */
} bsmr_plan_options;
int bsmr_plan_options_default(bsmr_plan_options *opt);
/* defaults, then every BSMR_<NAME> variable that is set */
int bsmr_plan_options_from_env(bsmr_plan_options *opt);

/* bsmr_plan_create = bsmr_plan_create_ex with bsmr_plan_options_from_env.  options == NULL: the defaults.
 * Every stored entry needs one place in the RPHM arrays: a block cell or a residue entry.  A CSR that stores the same
 * (row, column) twice keeps both copies only while that column is in the residue of the row's panel; where the column is
 * dense there, its block cell holds one copy, the arrays no longer account for nnz entries and the plan is refused with
 * BSMR_ERR_BAD_PLAN.  (The file loaders refuse such matrices; callers that build the CSR themselves must merge repeats.) */
int bsmr_plan_create(bsmr_plan **out, int device, const bsmr_rphm_desc *desc);
int bsmr_plan_create_ex(bsmr_plan **out, int device, const bsmr_rphm_desc *desc,
                        const bsmr_plan_options *options);
int bsmr_plan_destroy(bsmr_plan *plan);
int bsmr_plan_get_stats(const bsmr_plan *plan, bsmr_plan_stats *out);

/* Host wall time bsmr_plan_create[_ex] spent, milliseconds: the plan rules (promotion, folding), packing the
 * device format (csrc/plan_pack.hpp), allocating + uploading it, and packing + uploading the second (grouped)
 * dense format where one is kept.  The reference has no counterpart (its RPHM constructor uploads the host
 * arrays as they are, src/BSMR.cpp:236-262); reported so that callers can see what a re-plan costs. */
typedef struct bsmr_plan_build_ms {
    float rules_ms, pack_ms, upload_ms, second_format_ms, total_ms;
} bsmr_plan_build_ms;
int bsmr_plan_build_times(const bsmr_plan *plan, bsmr_plan_build_ms *out);

/* The per-call choices are measured, not modelled: bsmr_plan_tune times, on the caller's operands (HIP events on
 * `stream`, 3 warm-up + 10 timed launches each), the dense part under each engine and format, for all-sparse plans the
 * fp32 residue against the B-only conversion, for hybrid plans one stream against two - and the plan uses the fastest
 * of each for every later call with the same (K, mode); the fitted rules (grouped format from 400 MB of gathers,
 * b_only_work_m, overlap from 4 M entries a side) only serve calls that were never tuned.
 * Needs a plan created with dense_engine = BSMR_ENGINE_TUNED; P is overwritten with the (correct) result.  The
 * reference has no counterpart: it tunes (alpha, delta) per matrix by sweeping (src/sddmm.cu:62-118). */
typedef struct bsmr_tune_report {
    int32_t chosen_engine;            /* BSMR_ENGINE_STREAM / _TILES / _SHARED / _SWEEP / _GEMM */
    int32_t chosen_group;             /* panels per group of the winner (streaming engine: 1, or 4 = the grouped format;
                                         sweep engine: panels per consumer wave) */
    int32_t chosen_blocks_per_item;   /* shared-B engine: blocks per work item where that was part of the search, else 0;
                                         sweep engine: blocks per strip */
    /* best dense-kernel time per launch of each candidate family, microseconds; < 0: not measured (no such format,
     * the engine does not serve this K, or nothing to choose from) */
    float   stream_us, grouped_us, tiles_us, shared_us;
    /* plans without a dense part: whole call with the fp32 residue kernel against B converted alone + 16-bit residue
     * (replaces the b_only_work_m threshold for this (K, mode)); -1 / < 0: does not apply */
    int32_t chosen_b_only;
    float   fp32_residue_us, b_only_us;
    /* hybrid plans: whole call on one stream against the residue kernel on the side stream; -1 / < 0: does not apply */
    int32_t chosen_overlap;
    float   one_stream_us, two_streams_us;
    /* K = 32 / 64: whole call with the conversion pass against the streaming dense kernel that reads the fp32 operands and
     * rounds them in registers (same results); -1 / < 0: does not apply */
    int32_t chosen_cvt_in_kernel;
    float   convert_pass_us, fp32_dense_us;
    /* sweep engine (round 3; appended): best dense-kernel time on 16-bit operands (comparable with stream_us ...), and whole
     * calls: the best 16-bit engine behind the conversion pass against the sweep kernel on the fp32 operands */
    float   sweep_us;
    float   lowp_call_us, sweep_fp32_call_us;
    int32_t chosen_sweep_fp32;        /* 1: the chosen engine is the sweep kernel on fp32 operands */
    /* plans created with k_hint > 0 (appended): whole-call time of the plan under each setting of the plan-time rules,
     * microseconds (< 0: not built - the same split as an earlier variant, or no hint), and the one that serves the plan */
    int32_t chosen_variant;           /* BSMR_VARIANT_* */
    float   variant_us[6];
    /* GEMM engine (round 4; appended): best dense-kernel time on 16-bit operands over the macro-tile shapes tried; when it is
     * chosen, chosen_group = panels and chosen_blocks_per_item = 16-column blocks per macro-tile */
    float   gemm_us;
    /* K = 64 / 128, whole calls: the GEMM kernel on the caller's fp32 operands (no conversion pass) against the best of the
     * rest (lowp_call_us, or sweep_fp32_call_us where that had won) */
    float   gemm_fp32_call_us;
    int32_t chosen_gemm_fp32;         /* 1: the chosen engine is the GEMM kernel on fp32 operands */
} bsmr_tune_report;
#define BSMR_VARIANT_RULES        0   /* the options the plan was created with                                    */
#define BSMR_VARIANT_AS_RPHM      1   /* the RPHM's split as it is: nothing promoted, nothing folded              */
#define BSMR_VARIANT_NO_PROMOTION 2   /* promote_average = 0                                                      */
#define BSMR_VARIANT_PROMOTE_24   3   /* promote_average = 24                                                     */
#define BSMR_VARIANT_PROMOTE_ALL  4   /* every panel's residue becomes blocks                                     */
#define BSMR_VARIANT_ALL_RESIDUE  5   /* the dense part folded into the residue                                   */
int bsmr_plan_tune(bsmr_plan *plan, uint32_t K, const float *A_dev, const float *B_dev, float *P_dev, int mode, void *stream,
                   bsmr_tune_report *report /* may be NULL */);
/* The same for callers compiled against another revision of this header: bsmr_tune_report only ever grows at its end, and at
 * most report_size bytes of it are written (bsmr_plan_tune writes sizeof(bsmr_tune_report) of THIS revision: a caller built
 * against an older header must call bsmr_plan_tune_sized with its own sizeof, INTEGRATION.md "ABI revisions"). */
int bsmr_plan_tune_sized(bsmr_plan *plan, uint32_t K, const float *A_dev, const float *B_dev, float *P_dev, int mode, void *stream,
                         bsmr_tune_report *report /* may be NULL */, size_t report_size);

/* What a tuned plan keeps per (K, mode), as plain numbers: bsmr_plan_get_tuned reads the choice bsmr_plan_tune made
 * (BSMR_ERR_INVALID_ARG when that (K, mode) was never tuned), bsmr_plan_set_tuned installs one WITHOUT timing anything -
 * a second process (a profiler pass, a later run on the same matrix) replays the measured choice of the first and launches
 * exactly its kernels.  The choice is validated (the engine must serve this K and its device format must be buildable:
 * BSMR_ERR_INVALID_ARG / BSMR_ERR_BAD_PLAN otherwise, the plan unchanged).  Refused: a field outside its range, an engine with
 * cvt_in_kernel = 1 that has no fp32-operand kernel for this K (_TILES and _SHARED have none at any K: BSMR_ERR_INVALID_ARG;
 * _STREAM K = 32 / 64 / 128, _SWEEP K <= 128, _GEMM K = 64 / 128 and not the 16 x 12 macro-tile), an engine other than _STREAM
 * on a plan without a dense part or at a K it does not serve, a GEMM macro-tile no kernel is built for, format = 1 where the
 * plan has no grouped format (BSMR_ERR_BAD_PLAN).  Plans created with k_hint keep their variant:
 * these two calls address the engines of the plan that serves the calls.  The reference has no counterpart. */
typedef struct bsmr_tuned_choice {
    uint32_t struct_size;     /* sizeof(bsmr_tuned_choice) of the caller */
    int32_t  engine;          /* BSMR_ENGINE_STREAM / _TILES / _SHARED / _SWEEP / _GEMM */
    int32_t  group;           /* tiles / shared: panels per group; sweep: panels per consumer wave; gemm: macro-tile rows / 16; 0 = the engine's rule */
    int32_t  blocks_per_item; /* shared: blocks per work item; sweep: blocks per strip; gemm: macro-tile columns / 16; 0 = the engine's rule */
    int32_t  format;          /* streaming engine: 0 = one panel per group, 1 = the grouped format, -1 = the rule */
    int32_t  b_only;          /* all-sparse plans: 1 = B converted alone, 0 = fp32 residue, -1 = the rule */
    int32_t  overlap;         /* hybrid plans: 1 = residue on the side stream, 0 = one stream, -1 = as the plan was built */
    int32_t  cvt_in_kernel;   /* 1 = fp32 operands rounded inside the dense kernel, 0 = conversion pass, -1 = the rule */
    int32_t  waves;           /* sweep: consumer waves; 0 = the rule */
} bsmr_tuned_choice;
int bsmr_plan_get_tuned(const bsmr_plan *plan, uint32_t K, int mode, bsmr_tuned_choice *out);
int bsmr_plan_set_tuned(bsmr_plan *plan, uint32_t K, int mode, const bsmr_tuned_choice *choice);

/* Fingerprint of the plan's first dense format as it lies in device memory: FNV-1a of groupRows, rowBase, winLen,
 * winMask, blockCols, the destination tiles (8-bit or mask form), blockMask and the work items, then the numbers of
 * items / blocks / tiles / union columns and 1 if the tiles are in the mask form (out[0..12]).  Two plans with equal
 * fingerprints launch identical dense work; used to check the device packer against the host packer. */
int bsmr_plan_format_digest(const bsmr_plan *plan, uint64_t out[13]);
/* Fingerprint of the dense entry lists a plan keeps for the formats of the tiles / shared / sweep / GEMM engines (plans
 * created with one of these engines or BSMR_ENGINE_TUNED): FNV-1a of the panels' offsets, the entries' columns, rows in
 * panel and CSR indices (out[0..3]), the number of entries (out[4]).  All zero for a plan that keeps none.  The lists are
 * written by the device packer (csrc/pack_device.hpp: collectEmit) or by the host (csrc/tile_format.hpp: collectDense);
 * used to check the one against the other. */
int bsmr_plan_entry_lists_digest(const bsmr_plan *plan, uint64_t out[5]);
/* Which dense format a call with inner dimension K uses (any out pointer may be NULL):
 * panels per group, MFMA tiles executed, B columns gathered.  For a plan whose engines were measured (bsmr_plan_tune)
 * the answer describes the engine of the call that was prepared last - ask right after the bsmr_sddmm call in question
 * (the untuned rules depend on K alone). */
int bsmr_plan_dense_choice(const bsmr_plan *plan, uint32_t K, uint32_t *group_size,
                           uint64_t *tiles, uint64_t *union_columns);

/* Row clustering of the BSMR pipeline on the device: bsa_rowReordering_gpu
 * (src/rowReordering.cu:1027-1095 = calculateDispersion :478-501 + get_permutation_gpu
 * :893-1007 + the removal of empty rows :1082-1090).  S as host CSR; reordered_rows has
 * room for `rows` ids and receives the non-empty rows in clustered order; num_clusters is
 * the value the reference logs as bsmr_numClusters.  Results are identical to the host
 * implementation behind BSMR::rowReordering.  BSMR_ERR_OOM: the rows x bins table does not
 * fit in half of the free device memory (or one row's histogram does not fit in LDS) - the
 * caller falls back to the host implementation. */
typedef struct bsmr_cluster_stats {
    float    elapsed_ms;        /* device time, uploads and downloads included        */
    uint32_t passes;            /* speculative passes launched that did work          */
    uint32_t similarities;      /* (representative, row) pairs judged                 */
    uint32_t exact_similarities;/* ... of which within 1e-4 of alpha (exact evaluation) */
    uint32_t threads_per_pair;  /* workgroup size = the reference's clustering block  */
    uint64_t table_bytes;       /* rows x bins histogram table                        */
    uint32_t dropped_seeds;     /* clusters started ahead of the older ones' decisions whose seed an older one took */
    uint32_t passes_ahead;      /* passes in which clusters judged rows the older clusters had not decided yet    */
} bsmr_cluster_stats;
int bsmr_cluster_rows(int device, uint32_t rows, uint32_t cols, const uint32_t *row_offsets,
                      const uint32_t *col_indices, uint32_t bin_width, float alpha,
                      uint32_t *reordered_rows, uint32_t *num_reordered, int32_t *num_clusters,
                      bsmr_cluster_stats *stats);
/* ... for callers compiled against another revision of this header (bsmr_cluster_stats only grows at its end): at most
 * stats_size bytes of it are written. */
int bsmr_cluster_rows_sized(int device, uint32_t rows, uint32_t cols, const uint32_t *row_offsets,
                            const uint32_t *col_indices, uint32_t bin_width, float alpha,
                            uint32_t *reordered_rows, uint32_t *num_reordered, int32_t *num_clusters,
                            bsmr_cluster_stats *stats, size_t stats_size);

/* Column reordering, dense / sparse split and the RPHM index arrays of the BSMR pipeline on the device:
 * colReordering_cpu (src/colReordering.cu:274-404; the reference's own GPU version, :146-241, is unfinished) followed by
 * the array part of RPHM::RPHM (src/BSMR.cpp:83-265).  S as host CSR, reordered_rows as BSMR::rowReordering returns
 * them (the non-empty rows in clustered order).  The results equal the host implementation's array for array:
 * bsmr_col_reorder computes them on `device`, bsmr_col_reorder_sizes tells how much room they need, and
 * bsmr_col_reorder_fetch copies them into the caller's arrays (any pointer may be NULL). */
typedef struct bsmr_colreorder bsmr_colreorder;
typedef struct bsmr_colreorder_sizes {
    uint32_t num_row_panels;
    uint64_t num_dense_cols;      /* length of denseCols  (multiples of 16 per panel)          */
    uint64_t num_sparse_cols;     /* length of sparseCols (padding sentinels included)          */
    uint64_t num_blocks;          /* dense 16 x 16 blocks: blockValues holds 256 words of each  */
    uint64_t num_sparse_entries;  /* length of sparseValues / sparseRelativeRows / sparseColIndices */
    float    elapsed_ms;          /* device time, uploads included                              */
} bsmr_colreorder_sizes;
int bsmr_col_reorder(bsmr_colreorder **out, int device, uint32_t rows, uint32_t cols, const uint32_t *row_offsets,
                     const uint32_t *col_indices, const uint32_t *reordered_rows, uint32_t num_reordered, float delta);
int bsmr_col_reorder_sizes(const bsmr_colreorder *h, bsmr_colreorder_sizes *out);
int bsmr_col_reorder_device(const bsmr_colreorder *h, int *device);   /* where the result lies */
int bsmr_col_reorder_fetch(const bsmr_colreorder *h, uint32_t *dense_cols, uint32_t *dense_col_offsets,
                           uint32_t *sparse_cols, uint32_t *sparse_col_offsets, uint32_t *sparse_value_offsets,
                           uint32_t *block_offsets, uint32_t *block_values, uint32_t *sparse_values,
                           uint32_t *sparse_relative_rows, uint32_t *sparse_col_indices);
int bsmr_col_reorder_free(bsmr_colreorder *h);
/* The plan straight from a bsmr_col_reorder result, on its device: the RPHM's big arrays (block values, the residue) are
 * read where they lie - the promotion rule and the device packer run on them - and only what host-side steps need comes
 * down.  The plan is the one bsmr_plan_create_ex builds from the fetched arrays, byte for byte; plans that need the arrays
 * on the host (engines other than the streaming one, layouts of the host packer, k_hint) fetch them and take that road.
 * reordered_rows as given to bsmr_col_reorder; options == NULL: bsmr_plan_options_from_env. */
int bsmr_plan_create_from_colreorder(bsmr_plan **out, const bsmr_colreorder *h, uint32_t M, uint32_t N, uint32_t nnz,
                                     const uint32_t *reordered_rows, uint32_t num_nonzero_rows,
                                     const bsmr_plan_options *options);

/* How the sparse residue of a call (K, compute_mode) will run: lanes that share one entry's
 * K-long dot product (the fp32 summation order of the residue depends on it; the CPU twin in
 * oracle/sddmm_oracle.c takes the same number) and whether it reads the fp16/bf16 copies. */
int bsmr_plan_sparse_choice(const bsmr_plan *plan, uint32_t K, int compute_mode,
                            uint32_t *lanes_per_entry, uint32_t *low_precision);

/* Which kernel computes each stored entry: flags_host[i] (i = CSR index, nnz bytes, host memory) becomes 1
 * when the plan computes entry i on the dense (MFMA) path and 0 when the residue kernel does.  This is the
 * reference's dense / sparse split (RPHM::blockValues_ / sparseValues_, reference src/BSMR.cpp:83-265) after the plan's own moves
 * (folded_dense_entries, promoted_sparse_entries); the accuracy contract of an entry follows its path. */
int bsmr_plan_dense_flags(const bsmr_plan *plan, uint8_t *flags_host);

/* Grow the plan's operand workspace for inner dimension K now (otherwise it
 * grows on first use, which allocates and therefore must not happen inside a
 * stream capture). */
int bsmr_plan_reserve(bsmr_plan *plan, uint32_t K);

/* ---- Alignment of device pointers ----
 * Every device entry point below checks its pointers before any device work and returns BSMR_ERR_INVALID_ARG for one
 * below the alignment its argument needs (a NULL that the call allows counts as aligned):
 *   16 bytes  the operand matrices and their 16-bit copies: A_dev, B_dev (fp32, bsmr_sddmm, _batch, _timed, _lowp,
 *             bsmr_plan_tune, bsmr_convert_operands, bsmr_sddmm_backward[_mode]), A16_dev, B16_dev (bsmr_convert_operands,
 *             bsmr_sddmm_lowp, bsmr_sddmm_16, bsmr_sddmm_backward_16), X_dev, Y_dev (bsmr_spmm[_mode]), X16_dev, Y_dev
 *             (bsmr_spmm_lowp), X16_dev, Y16_dev (bsmr_spmm_16, bsmr_spmm_blocked_16), X_dev, Y_dev (bsmr_spmm_blocked),
 *             dA_dev, dB_dev (bsmr_sddmm_backward[_mode]), dA16_dev,
 *             dB16_dev (bsmr_sddmm_backward_16).  The kernels move them 16 bytes at a time (global_load_dwordx4, LDS-DMA of
 *             16 bytes per lane, 16-byte stores of the conversion pass, float4 and 8 x 16-bit loads and stores in the
 *             backward); K is a multiple of 32, so every row, column and batch then starts on 16 bytes.
 *    4 bytes  the value arrays, read and written one float at a time: P_dev (all of the above), v_dev (bsmr_spmm[_mode],
 *             bsmr_spmm_lowp, bsmr_spmm_16, bsmr_spmm_blocked[_16]), dP_dev (bsmr_sddmm_backward[_mode],
 *             bsmr_sddmm_backward_16), X_dev / Y_dev /
 *             dY_dev / dX_dev of bsmr_sparse_softmax[_backward], and
 *             in_dev / out_dev of bsmr_batched_transpose.  A batch with an odd nnz puts its second problem on an odd
 *             float; that is within the contract.
 * No call reads or writes outside the extents its comment states (M K, N K, nnz elements, times num_batches), whatever
 * lies around them (tests/test_gpu_memory_contract.py).  bsmr_sddmm_host takes host pointers: no requirement. */

/* One SDDMM: A_dev is M x K row-major fp32, B_dev is K x N column-major fp32
 * (column j = K contiguous floats at B_dev + j*K), P_dev receives nnz floats in
 * S's CSR order.  Every element of P_dev is overwritten. */
int bsmr_sddmm(bsmr_plan *plan, uint32_t K, const float *A_dev, const float *B_dev,
               float *P_dev, int compute_mode, void *stream);

/* warmup + iters repetitions of bsmr_sddmm bracketed by HIP events on `stream`;
 * per-kernel times are measured in a second pass of `iters` repetitions with
 * events around each kernel. */
int bsmr_sddmm_timed(bsmr_plan *plan, uint32_t K, const float *A_dev, const float *B_dev,
                     float *P_dev, int compute_mode, void *stream, int warmup, int iters,
                     bsmr_timing *out);

/* sddmm_gpu_batch (include/sddmmKernel.cuh:41-47, src/sddmmKernel.cu:2764-2869): num_batches
 * independent problems over one sparsity plan, stored back to back - A: [b][M][K] row-major,
 * B: [b][N][K] (each K x N column-major), P: [b][nnz].  One conversion pass over all batches, then
 * the dense and residue kernels with the batch index in the grid's y dimension. */
int bsmr_sddmm_batch(bsmr_plan *plan, uint32_t K, const float *A_dev, const float *B_dev, float *P_dev,
                     uint32_t num_batches, int compute_mode, void *stream);

/* batchedMatrixTranspose (include/sddmmKernel.cuh:49-51, src/sddmmKernel.cu:2486-2515):
 * out[b] = transpose(in[b]) for num_batches row-major height x width matrices. */
int bsmr_batched_transpose(uint32_t width, uint32_t height, uint32_t num_batches, const float *in_dev,
                           float *out_dev, void *stream);

/* Convert fp32 operands once (mode F16 or BF16); A16_dev / B16_dev are M*K and
 * N*K 16-bit elements in the same layouts. */
int bsmr_convert_operands(bsmr_plan *plan, uint32_t K, const float *A_dev, const float *B_dev,
                          void *A16_dev, void *B16_dev, int compute_mode, void *stream);

/* SDDMM on pre-converted operands.  The dense path reads A16/B16.  The sparse residue reads
 * them too when bsmr_plan_stats.sparse_lowp is 1 (A_dev/B_dev may then be NULL); otherwise it
 * needs the fp32 A_dev/B_dev. */
int bsmr_sddmm_lowp(bsmr_plan *plan, uint32_t K, const void *A16_dev, const void *B16_dev,
                    const float *A_dev, const float *B_dev, float *P_dev, int compute_mode,
                    void *stream);

/* ---- one SDDMM over several GPUs of one node, from one process (the reference is single-GPU) ----
 * Row panels are independent, so the rows of S are cut into contiguous ranges (the caller's cost partition) and
 * every range is a problem of its own: shard_descs[i] is the RPHM of rows [row_begin[i], row_begin[i+1]) with LOCAL
 * row ids (built by the host pipeline on that slice), devices[i] the GPU it lives on.  A step runs bsmr_sddmm on
 * every device and gathers the compact outputs to devices[0] with one RCCL send/recv group (communicators are
 * created once, in bsmr_sharded_create, over the distinct devices of the list); P in S's CSR order is the concatenation
 * of the shards' outputs.  A device may be listed more than once (more shards than GPUs): a shard on the root's device
 * hands its part over with a device-to-device copy.  A range without rows or entries takes no part in a step. */
typedef struct bsmr_sharded bsmr_sharded;
typedef struct bsmr_sharded_timing {
    float    step_ms;      /* device time of one step (SDDMM on every device + gather), max over devices; the steps are
                              pipelined over two sets of output buffers: the gather of step i runs behind the SDDMM of i + 1 */
    float    wall_ms;      /* host wall time of one step                                                  */
    uint32_t num_devices;
    /* (round 4; appended - ABI revision 4) one un-pipelined step taken apart: */
    float    compute_ms;   /* SDDMM alone, max over devices                                               */
    float    gather_ms;    /* the gather-v alone: first part leaving to last part delivered               */
} bsmr_sharded_timing;
/* Revision of this header's struct layouts (4 = round 4: bsmr_sharded_timing, bsmr_tune_report, bsmr_cluster_stats and
 * bsmr_plan_options grew at their ends; 5: the SDDMM backward, bsmr_backward_* / bsmr_spmm / bsmr_sddmm_backward).  A
 * caller built against an older revision uses the *_sized entry points for the structs the library writes, or is
 * rebuilt. */
#define BSMR_ABI_REVISION 5
int bsmr_abi_revision(void);
int bsmr_sharded_create(bsmr_sharded **out, const int *devices, uint32_t num_devices,
                        const bsmr_rphm_desc *const *shard_descs, const uint32_t *row_begin,
                        const bsmr_plan_options *options);
int bsmr_sharded_destroy(bsmr_sharded *s);
/* total stored entries (length of P) and, if per_shard != NULL, every shard's share */
int bsmr_sharded_num_entries(const bsmr_sharded *s, uint64_t *total, uint64_t *per_shard);
/* Host operands in (A: all rows, row-major M x K; B: K x N column-major), host P out (S's CSR order): uploads every
 * shard's rows of A and a replica of B, one warm-up step, `iters` timed steps, download from the root. */
int bsmr_sharded_sddmm_host(bsmr_sharded *s, uint32_t K, const float *A_host, const float *B_host, float *P_host,
                            int compute_mode, int iters, bsmr_sharded_timing *timing);

/* ---- SDDMM backward (revision 5; no reference counterpart) ----
 * P = (A B^T) at S's stored positions has the gradients dA = S_dP B and dB = S_dP^T A; attention follows an SDDMM with
 * Y = S_v X.  All are one gather-and-accumulate: for destination d with list L(d), Y[d,:] = sum_{t in L(d)} v[e(t)] X[s(t),:]
 * (transpose 0: the rows of S, e(t) = t, s(t) = col_indices[t]; transpose 1: the columns of S, e(t) = csc_to_csr[t],
 * s(t) = csc_rows[t]).  X and Y are row-major with K contiguous floats per row (the layout of A and B), 16-byte aligned;
 * v and dP need the 4 bytes of a float ("Alignment of device pointers" above).
 *
 * Numerical contract: each destination's sum runs in its list's order (CSR order for rows, ascending row for columns) as
 * a sequential fp32 fma chain; a list longer than BSMR_BACKWARD_CHUNK is summed chunk by chunk and the partials are added
 * in chunk order.  No atomics: results are bitwise reproducible call to call, stream to stream, batch to batch and for
 * any row_order; a destination without entries is exactly 0; |Y - Y_exact| <= (n + 2) u sum|v||x| (n = list length,
 * u = 2^-24).  The chunk partials live in a workspace of the handle: calls on one handle are ordered by the caller.
 * Extents: every element index - s K of a source row, dest K of a destination row, the batch offsets b rows K and b nnz,
 * b slots K + slot K of a workspace row - is formed in 64 bits; M K, N K, nnz and slots K, each times num_batches, may
 * pass 2^32 elements (tests/test_gpu_backward_extents.py drives each of them past 2^32 elements, not only past 4 GiB). */
#define BSMR_BACKWARD_CHUNK 512u   /* entries per work item of a long list (cdna_hip_programming.md, Appendix B) */
typedef struct bsmr_backward bsmr_backward;
typedef struct bsmr_backward_stats {
    uint32_t chunk;               /* BSMR_BACKWARD_CHUNK                                          */
    uint32_t split_rows;          /* rows (dA destinations) cut into chunks                       */
    uint32_t split_cols;          /* columns (dB destinations) cut into chunks                    */
    uint32_t max_row_length;      /* longest row of S                                             */
    uint32_t max_col_length;      /* longest column of S                                          */
    uint32_t row_items;           /* work items (whole lists + chunks) of the row direction       */
    uint32_t col_items;           /* ... of the column direction                                  */
    uint32_t permute_values;      /* 1: the column direction permutes v into CSC order first (the default;
                                     BSMR_BACKWARD_PERMUTE=0 at create: read through csc_to_csr)  */
    uint64_t device_index_bytes;  /* index arrays resident on the device                          */
    uint64_t workspace_bytes;     /* chunk partials (+ permuted values, 16-bit copies) reserved so far */
} bsmr_backward_stats;
/* S as host CSR (row_offsets [M+1], col_indices [nnz]; read during the call only).  row_order: the order in which the
 * row destinations are scheduled (pass the pipeline's reordered_rows, the clustered order); it may list a subset, the
 * rows it omits follow in natural order.  NULL with num_ordered_rows = 0: natural order.  BSMR_ERR_INVALID_ARG, before
 * any device call: a duplicate or out-of-range row in row_order, row_offsets[0] != 0, non-monotone row_offsets,
 * row_offsets[M] != nnz, a column id >= N. */
int bsmr_backward_create(bsmr_backward **out, int device, uint32_t M, uint32_t N, uint32_t nnz,
                         const uint32_t *row_offsets, const uint32_t *col_indices,
                         const uint32_t *row_order, uint32_t num_ordered_rows);
int bsmr_backward_destroy(bsmr_backward *bw);
/* Grow the workspace for calls with (K, num_batches) now; calls covered by it allocate nothing (capturable). */
int bsmr_backward_reserve(bsmr_backward *bw, uint32_t K, uint32_t num_batches);
/* at most out_size bytes of the statistics are written (the struct only grows at its end) */
int bsmr_backward_get_stats(const bsmr_backward *bw, bsmr_backward_stats *out, size_t out_size);
/* Host only, no device: the transpose the handle uploads.  col_offsets [N+1]; csc_rows / csc_to_csr [nnz]: the row and
 * the CSR index of each entry, column by column, ascending row within a column.  Same argument checks as create. */
int bsmr_csr_transpose(uint32_t M, uint32_t N, uint32_t nnz, const uint32_t *row_offsets, const uint32_t *col_indices,
                       uint32_t *col_offsets, uint32_t *csc_rows, uint32_t *csc_to_csr);
/* Y = S_v X (transpose 0: X N x K, Y M x K) or S_v^T X (transpose 1: X M x K, Y N x K); v in S's CSR order; every
 * element of Y is overwritten.  Batches as bsmr_sddmm_batch: v [b][nnz], X / Y [b][rows][K], the batch in grid y.
 * With nnz = 0 nothing is read: v and X may be NULL (a zero-element tensor's pointer), Y is still all zeros. */
int bsmr_spmm(bsmr_backward *bw, uint32_t K, int transpose, const float *v_dev, const float *X_dev, float *Y_dev,
              uint32_t num_batches, void *stream);
/* dA = S_dP B (M x K), dB = S_dP^T A (N x K); either output may be NULL: that product is skipped.  With nnz = 0
 * dP, A and B may be NULL; the requested outputs are still all zeros. */
int bsmr_sddmm_backward(bsmr_backward *bw, uint32_t K, const float *dP_dev, const float *A_dev, const float *B_dev,
                        float *dA_dev, float *dB_dev, uint32_t num_batches, void *stream);

/* ---- fp16 / bf16 gather modes of the two calls above (revision 5, added without any layout change) ----
 * compute_mode = BSMR_COMPUTE_F32: exactly bsmr_spmm / bsmr_sddmm_backward / bsmr_backward_reserve - the same kernels,
 * the same bits, the same workspace.  BSMR_COMPUTE_F16 / _BF16: the gathered operand - X for bsmr_spmm_mode, B for dA and
 * A for dB - is read as 16-bit rows, half the gathered bytes; v / dP, the accumulation, the chunk partials and the outputs
 * stay fp32.  bsmr_spmm_mode and bsmr_sddmm_backward_mode round the operand(s) once per call (round to nearest even, the
 * casts of bsmr_convert_operands: fp16 subnormals kept, beyond the fp16 range +-inf, NaN stays NaN; one launch for A and
 * B) into the handle's workspace, behind the chunk partials and the permuted values on the next 16 bytes; only what a
 * requested product gathers is rounded.  bsmr_spmm_lowp takes rows the caller already holds in 16 bits (an output of
 * bsmr_convert_operands, a half / bfloat16 buffer; 16-byte aligned, [b][rows][K]): no pass, no workspace for X;
 * compute_mode says how to read them, BSMR_COMPUTE_F32 is BSMR_ERR_INVALID_ARG.
 *
 * Numerical contract: widening fp16 / bf16 to fp32 is exact, so the result is the fp32 contract of "SDDMM backward"
 * applied to (v, round_mode(X)), bit for bit - the same chains, chunks and fma - with the same reproducibility: call to
 * call, stream to stream, batch to batch, for any row_order, with or without BSMR_BACKWARD_PERMUTE, and whichever lane
 * layout the 16-bit kernel runs in.  With x~ = round_mode(x):
 *   |Y - S_v X| <= (n + 2) u sum|v||x~| + u16 sum|v||x|,  u = 2^-24, u16 = 2^-11 (fp16) or 2^-8 (bf16),
 * for X inside the 16-bit format's normal range.  As gradients of an SDDMM that ran in the same mode these are the
 * straight-through gradients of the function it computed: dA = S_dP round(B), dB = S_dP^T round(A).
 *
 * Arguments as the fp32 calls, checked before any device work: a NULL handle or a compute_mode outside {0, 1, 2} is
 * BSMR_ERR_INVALID_ARG, K = 0 or not a multiple of 32 BSMR_ERR_UNSUPPORTED_K; the same alignments; with nnz = 0 v and X
 * may be NULL and the outputs are all zeros; num_batches = 0 is a no-op, at most 65535 batches.  After
 * bsmr_backward_reserve_mode(K, num_batches, compute_mode) every one of these calls with that (K, num_batches or fewer,
 * mode) allocates nothing and can be captured in a graph. */
int bsmr_backward_reserve_mode(bsmr_backward *bw, uint32_t K, uint32_t num_batches, int compute_mode);
int bsmr_spmm_mode(bsmr_backward *bw, uint32_t K, int transpose, const float *v_dev, const float *X_dev, float *Y_dev,
                   uint32_t num_batches, int compute_mode, void *stream);
int bsmr_sddmm_backward_mode(bsmr_backward *bw, uint32_t K, const float *dP_dev, const float *A_dev, const float *B_dev,
                             float *dA_dev, float *dB_dev, uint32_t num_batches, int compute_mode, void *stream);
int bsmr_spmm_lowp(bsmr_backward *bw, uint32_t K, int transpose, const float *v_dev, const void *X16_dev, float *Y_dev,
                   uint32_t num_batches, int compute_mode, void *stream);

/* ---- fp16 / bf16 tensors end to end (revision 5, added without any layout change; no reference counterpart) ----
 * For a caller that holds 16-bit tensors only (a model under autocast): no fp32 copy of an operand is read, made or
 * written.  compute_mode is BSMR_COMPUTE_F16 or BSMR_COMPUTE_BF16 and says how every 16-bit array of the call is read and
 * written; BSMR_COMPUTE_F32 is BSMR_ERR_INVALID_ARG.  The value arrays P, v and dP stay fp32: scores and softmax weights
 * are never 16-bit.
 *
 * bsmr_sddmm_16: bsmr_sddmm_batch on the caller's 16-bit operands (A16 [b][M][K], B16 [b][N][K], P [b][nnz]; the batch in
 * grid y; num_batches = 0 is a no-op, at most 65535 batches, K * num_batches below 2^32).  The dense part runs the 16-bit
 * kernel of the engine the plan selects for (K, compute_mode), the residue always its 16-bit kernel - whatever sparse_lowp,
 * convert_in_kernel, b_only, sweep_fp32 or gemm_fp32 say about the road of fp32 operands: no fp32 operand, no conversion
 * pass and no operand workspace exist here (nothing to reserve; a tiles / sweep / GEMM format is still built on the first
 * call that needs it).  Every entry is the fp32-accumulated product of the given 16-bit values: on a plan whose fp32 road
 * runs the conversion pass, bit for bit what bsmr_sddmm_lowp returns for the same copies.  A hybrid plan overlaps its two
 * kernels under the rule of bsmr_sddmm; a plan tuned with k_hint serves (K, compute_mode) with its variant.
 *
 * bsmr_spmm_16 / bsmr_sddmm_backward_16: the gather of bsmr_spmm_lowp (same lists, chunks, fma chains, lane layouts) with
 * one addition - the single store of a finished destination row rounds to the 16-bit format (round to nearest even, fp16
 * subnormals kept, +-inf beyond the range, NaN stays NaN: the casts of bsmr_convert_operands), 8 or 16 bytes per lane.
 * Chunk partials stay fp32 in the workspace and are added in fp32: exactly one rounding per output element.
 *   Y16 = round_mode(Y),  Y = the fp32 contract of "SDDMM backward" applied to (v, widen(X16)), bit for bit
 * with all of its reproducibility: call to call, stream to stream, batch to batch, for any row_order, with or without
 * BSMR_BACKWARD_PERMUTE, in either lane layout (BSMR_GATHER16_LANES).  A destination without entries is +0; a NaN in v
 * reaches its destination row only.  bsmr_sddmm_backward_16: dA16 = round(S_dP widen(B16)) (M x K), dB16 =
 * round(S_dP^T widen(A16)) (N x K); either output may be NULL: that product is skipped.  Neither call runs a conversion
 * pass or uses the 16-bit region of the workspace: after bsmr_backward_reserve(K, num_batches) they allocate nothing and
 * can be captured in a graph.
 *
 * Checked before any device work, in this order: a NULL plan / handle (BSMR_ERR_INVALID_ARG), K = 0 or not a multiple of
 * 32 (BSMR_ERR_UNSUPPORTED_K), compute_mode, then the pointers: 16 bytes for every 16-bit array, 4 for the value arrays
 * ("Alignment of device pointers").  With nnz = 0 the inputs may be NULL and the outputs are still all zeros
 * (bsmr_sddmm_16 has nothing to write).  No call touches memory outside M K / N K 16-bit elements and nnz floats, times
 * num_batches.  The gathers of this section and of the gather modes above index like "SDDMM backward": 16-bit rows are
 * read and stored at element indices past 2^32 (8 GiB), and the copies the _mode calls make may hold more than 2^32
 * elements each (tests/test_gpu_backward_extents.py, case R). */
int bsmr_sddmm_16(bsmr_plan *plan, uint32_t K, const void *A16_dev, const void *B16_dev, float *P_dev,
                  uint32_t num_batches, int compute_mode, void *stream);
int bsmr_spmm_16(bsmr_backward *bw, uint32_t K, int transpose, const float *v_dev, const void *X16_dev,
                 void *Y16_dev, uint32_t num_batches, int compute_mode, void *stream);
int bsmr_sddmm_backward_16(bsmr_backward *bw, uint32_t K, const float *dP_dev, const void *A16_dev,
                           const void *B16_dev, void *dA16_dev, void *dB16_dev, uint32_t num_batches,
                           int compute_mode, void *stream);

/* ---- Sparse row softmax (revision 5, added without any layout change; no reference counterpart) ----
 * The middle step of sparse attention (SDDMM -> softmax -> SpMM) on the same handle: values in S's CSR order, row r
 * owning positions [row_offsets[r], row_offsets[r+1]).  Per row, each step one IEEE-rounded fp32 operation:
 *   forward   z_t = fl32(scale x_t);  m = max_t z_t;  e_t = expf(z_t - m) (the accurate expf);  s = sum_t e_t;
 *             y_t = e_t / s (IEEE division)
 *   backward  g = sum_t y_t dY_t;  dX_t = fl32(fl32(y_t fl32(dY_t - g)) scale)
 * Summation order of s and g: that of bsmr_spmm's rows - a sequential fp32 chain in CSR order from +0 (s: s + e_t, g:
 * fmaf(y_t, dY_t, g)), a row longer than BSMR_BACKWARD_CHUNK summed chunk by chunk with the partials added in chunk
 * order.  It depends on the pattern alone: results are bitwise reproducible call to call, stream to stream, batch to
 * batch, in place or not, and for any row_order.  The backward is exactly that twin (oracle_gather_twin at K = 1).
 * Special values: a row whose entries are all -inf (m = -inf) gives exact zeros (and, with finite dY, a zero gradient);
 * any other -inf entry gives exactly 0; a NaN or +inf z anywhere in a row makes that whole row NaN and no other; a row
 * with one finite entry gives exactly 1; rows without entries are not touched.
 * Forward bound against fp64 over the same z (u = 2^-24, n the row length, Z_r = max_j |z_j - m|):
 *   |y_t - y64_t| <= (n + 6 + |z_t - m| + Z_r) u y64_t + (n + 2) 2^-126,   |sum_t y_t - 1| <= (n + 6) u + (n + 2) 2^-126.
 * Batches: values [b][nnz], the batch in grid y (b <= 65535).  Y may alias X, dX may alias dY.  num_batches = 0 is a
 * no-op; a NULL handle, a non-finite scale or a NULL array with nnz > 0 is BSMR_ERR_INVALID_ARG; with nnz = 0 the arrays
 * may be NULL.  Neither call allocates (no workspace): both can be captured in a graph.  b nnz is formed in 64 bits:
 * num_batches * nnz may pass 2^32 entries (tests/test_gpu_backward_extents.py, case V). */
int bsmr_sparse_softmax(bsmr_backward *bw, float scale, const float *X_dev, float *Y_dev,
                        uint32_t num_batches, void *stream);
int bsmr_sparse_softmax_backward(bsmr_backward *bw, float scale, const float *Y_dev, const float *dY_dev,
                                 float *dX_dev, uint32_t num_batches, void *stream);

/* ---- Fused sparse attention: softmax . V in one gather (revision 5, added without any layout change) ----
 * O = softmax_rows(scale P) V without the weights ever being stored: the softmax's row sum rides inside bsmr_spmm's row
 * gather as one more accumulator.  Same handle, lists, chunks and lane layouts as bsmr_spmm (transpose 0); P [b][nnz] in
 * S's CSR order, V [b][N][Kv], O [b][M][Kv], m and s [b][M].  Per row r of n entries, each step one IEEE fp32 operation
 * (u = 2^-24):
 *   forward   z_t = fl(scale p_t);  m = max_t z_t (any NaN z makes m NaN);  e_t = expf(fl(z_t - m)), the accurate expf,
 *             and 0 when m = -inf;  s = sum_t e_t;  acc_k = sum_t fmaf(e_t, V[c_t,k], .);  O_k = acc_k / s (IEEE division)
 *   s and acc run in bsmr_spmm's order: a sequential chain from +0 in CSR order; a row longer than BSMR_BACKWARD_CHUNK is
 *   cut into the handle's chunks, and the partials of acc and of s are added in chunk order.
 *   O_k is exactly +0 when m = -inf or the row is empty (then m = -inf, s = 0).  A NaN or +inf score makes its row of O
 *   (and its m or s) NaN and no other; a row with one finite entry returns that row of V bit for bit (e = 1, s = 1).
 *   backward  w_t = fl(e_t / s), e_t recomputed as above from (p_t, m, s), 0 when m = -inf;
 *             D = dO_r . O_r in this order: lane l of 32 runs the fma chain fmaf(dO_k, O_k, .) over k = l, l + 32, ...
 *             ascending from +0; the 32 partials are added by a butterfly over the lane offsets 16, 8, 4, 2, 1 (x + partner;
 *             fp32 addition commutes, so all lanes hold the same bits);
 *             dP_t = fl(fl(w_t fl(dW_t - D)) scale), with dW = sddmm(dO, V) from the caller;  W_t = w_t is written out
 *             for the transposed bsmr_spmm that gives dV.  dP may alias dW.  D lives in the workspace.
 * No atomics: bitwise reproducible call to call, stream to stream, batch to batch and for any row_order.
 * Forward bound against fp64 over the same z (Z_r = max_j |z_j - m|, w64 the fp64 weights):
 *   |O_k - O64_k| <= (2n + 2 Z_r + 10) u sum_t w64_t |V[c_t,k]| + (n + 2) 2^-126 max_t |V[c_t,k]|.
 * W obeys the bound of y in "Sparse row softmax".
 * The _16 forms: V, O, dO and the saved O are fp16 / bf16 rows (compute_mode BSMR_COMPUTE_F16 / _BF16, as in bsmr_spmm_16);
 * P, m, s, dW, dP and W stay fp32.  Rows are widened exactly, sums are fp32, O16 = round(O) once (the casts of
 * bsmr_convert_operands): bit for bit the fp32 call on widen(V16), rounded.  D is taken on the saved, ROUNDED O (the usual
 * flash-attention choice): against the D of the unrounded O that moves it by at most u16 sum_k |dO_k| |O_k| (u16 = 2^-11
 * fp16, 2^-8 bf16).
 * bsmr_sparse_attention_reserve(Kv, num_batches): the workspace of the four calls - what bsmr_backward_reserve(Kv,
 * num_batches) covers, and behind it the partial row sums and D; afterwards covered calls allocate nothing.
 * Checked before any device call, in this order: a NULL handle or a non-finite scale (BSMR_ERR_INVALID_ARG), Kv = 0 or
 * not a multiple of 32 (BSMR_ERR_UNSUPPORTED_K), compute_mode of a _16 call, more than 65535 batches, then the pointers:
 * 16 bytes for V, O and dO, 4 for P, m, s, dW, dP and W.  num_batches = 0 is a no-op.  With nnz = 0 the inputs may be
 * NULL; the forward still writes O = 0, m = -inf, s = 0.  (b M + r) Kv, b nnz and (b slots + slot) Kv are formed in 64
 * bits: O, the value arrays and the workspace may each pass 2^32 elements (tests/test_gpu_backward_extents.py, cases O,
 * S and V). */
int bsmr_sparse_attention_reserve(bsmr_backward *bw, uint32_t Kv, uint32_t num_batches);
int bsmr_sparse_attention(bsmr_backward *bw, uint32_t Kv, float scale, const float *P_dev, const float *V_dev,
                          float *O_dev, float *m_dev, float *s_dev, uint32_t num_batches, void *stream);
int bsmr_sparse_attention_16(bsmr_backward *bw, uint32_t Kv, float scale, const float *P_dev, const void *V16_dev,
                             void *O16_dev, float *m_dev, float *s_dev, uint32_t num_batches, int compute_mode,
                             void *stream);
int bsmr_sparse_attention_backward(bsmr_backward *bw, uint32_t Kv, float scale, const float *P_dev, const float *m_dev,
                                   const float *s_dev, const float *dW_dev, const float *O_dev, const float *dO_dev,
                                   float *dP_dev, float *W_dev, uint32_t num_batches, void *stream);
int bsmr_sparse_attention_backward_16(bsmr_backward *bw, uint32_t Kv, float scale, const float *P_dev,
                                      const float *m_dev, const float *s_dev, const float *dW_dev, const void *O16_dev,
                                      const void *dO16_dev, float *dP_dev, float *W_dev, uint32_t num_batches,
                                      int compute_mode, void *stream);

/* ---- fp8 keys and values (revision 5, added without any layout change; no reference counterpart) ----
 * The column-side operand - B / Kt of the SDDMM, X / V of the SpMM and of the fused attention - may be OCP fp8, one byte per
 * element, as an fp8 KV cache holds it: fp8_format BSMR_FP8_E4M3 (e4m3fn: no infinity, two NaN codes) or BSMR_FP8_E5M2 (two
 * infinities, six NaN codes).  The row-side operand (A / Q) and the outputs (Y, O) are fp16 or bf16: compute_mode is
 * BSMR_COMPUTE_F16 or BSMR_COMPUTE_BF16, the format of every 16-bit array of the call and the format the fp8 operand is
 * widened to; BSMR_COMPUTE_F32 or any other value is BSMR_ERR_INVALID_ARG, and so is an fp8_format outside {0, 1}.  P, v, m,
 * s and every sum stay fp32.  The fp8 format is an argument of these functions alone: the _mode, _lowp and _16 entry points
 * accept the compute modes they accepted before.
 *
 * Numerical contract.  Every code of both formats is a value of fp16 and of bf16, so widening is exact: +-0 keeps its
 * sign, subnormals widen exactly, e5m2 +-inf stays +-inf, every NaN code becomes a NaN.  An fp8 call is, bit for bit, the
 * 16-bit call on the widened operand:
 *   bsmr_widen_fp8(in8, out16, count)     out16[i] = widen(in8[i]) in compute_mode's format; count elements, any count
 *   bsmr_sddmm_b8(A16, B8)             == bsmr_sddmm_16(A16, widen(B8))
 *   bsmr_spmm_x8(v, X8)                == bsmr_spmm_16(v, widen(X8))              both directions
 *   bsmr_sparse_attention_x8(P, V8)    == bsmr_sparse_attention_16(P, widen(V8))  O16, m and s
 * with the reproducibility of those calls.  No scale factor is applied: a per-tensor scale of K folds into the attention
 * scale and one of V into the output, by the caller.
 *
 * bsmr_sddmm_b8 widens B8 ([b][N][K] bytes) into the plan's 16-bit workspace on the call's stream - the workspace of
 * bsmr_sddmm_batch for K * num_batches, allocated on the first call that needs it - and runs bsmr_sddmm_16 on (A16, that
 * copy); A16 is read in place.  bsmr_spmm_x8 and bsmr_sparse_attention_x8 make no copy: the gathers of their _16 forms
 * read the bytes (rows of K bytes, row and batch offsets formed in 64 bits) and widen in registers.  Same lists, chunks and
 * fma chains; fp32 chunk partials in the workspace that bsmr_backward_reserve / bsmr_sparse_attention_reserve size; one
 * rounding per output element.  The backward of the fused attention is bsmr_sparse_attention_backward_16 on (O16, dO16).
 *
 * Checked before any device work, in the order of the _16 forms: a NULL plan / handle or a non-finite scale
 * (BSMR_ERR_INVALID_ARG), K = 0 or not a multiple of 32 (BSMR_ERR_UNSUPPORTED_K), compute_mode and fp8_format, then the
 * pointers - 16 bytes for the fp8 and the 16-bit arrays, 4 for P, v, m and s - and more than 65535 batches.  num_batches =
 * 0 is a no-op; with nnz = 0 the inputs may be NULL and nothing is read.  bsmr_widen_fp8: count = 0 is a no-op whatever
 * the pointers; otherwise both must be non-NULL and 16-byte aligned.  It runs on the current device. */
#define BSMR_FP8_E4M3 0   /* OCP e4m3fn (torch.float8_e4m3fn) */
#define BSMR_FP8_E5M2 1   /* OCP e5m2   (torch.float8_e5m2)   */
int bsmr_widen_fp8(const void *in8_dev, void *out16_dev, uint64_t count, int compute_mode, int fp8_format, void *stream);
int bsmr_sddmm_b8(bsmr_plan *plan, uint32_t K, const void *A16_dev, const void *B8_dev, float *P_dev,
                  uint32_t num_batches, int compute_mode, int fp8_format, void *stream);
int bsmr_spmm_x8(bsmr_backward *bw, uint32_t K, int transpose, const float *v_dev, const void *X8_dev, void *Y16_dev,
                 uint32_t num_batches, int compute_mode, int fp8_format, void *stream);
int bsmr_sparse_attention_x8(bsmr_backward *bw, uint32_t Kv, float scale, const float *P_dev, const void *V8_dev,
                             void *O16_dev, float *m_dev, float *s_dev, uint32_t num_batches, int compute_mode,
                             int fp8_format, void *stream);

/* ---- MX block scales on the fp8 operand (MXFP8; revision 5, added without any layout change; no reference counterpart) ----
 * The fp8 operand of the four calls above with the block scales of the OCP Microscaling format, as an MXFP8 KV cache holds
 * them: `scales` is a uint8 array [b][rows][K / 32], contiguous (batch stride rows * K / 32), one E8M0 byte per 32
 * consecutive elements of a row.  It is read by byte loads and may have any alignment.  Code e means 2^(e - 127): e = 0 is
 * 2^-127 (an fp32 subnormal), e = 254 is 2^127, e = 255 is NaN, as torch.float8_e8m0fnu decodes it.
 *
 * Numerical contract.  dq(X8, E)[r][k] = widen(X8[r][k]) * 2^(E[r][k / 32] - 127): one IEEE fp32 multiplication of the
 * exactly widened code.  Subnormal results are kept, overflow gives +-inf, +-0 keeps its sign, e5m2's +-inf stays +-inf, a
 * NaN code or scale code 255 gives NaN.  The element is dequantised first and then enters the fma chain; the scale is not
 * folded into the weight (w * 2^s agrees in range but is another function at the ends of the range).  With narrow = the
 * cast of the 16-bit forms (round to nearest even, fp16 subnormals kept, +-inf beyond the range):
 *   bsmr_widen_fp8_mx(in8, scales, out16, count)   out16[i] = narrow(dq(in8, scales)[i]); count a multiple of 32
 *   bsmr_sddmm_b8_mx(A16, B8, Bs)               == bsmr_sddmm_16(A16, narrow(dq(B8, Bs)))
 *   bsmr_spmm_x8_mx(v, X8, Xs)                  == narrow(bsmr_spmm(v, dq(X8, Xs))): the fp32 gather contract of "SDDMM
 *                                                  backward" on dq, each output rounded once; both directions
 *   bsmr_sparse_attention_x8_mx(P, V8, Vs)      == bsmr_sparse_attention(P, dq(V8, Vs)) with O rounded once; m and s are
 *                                                  bit for bit those of the fp32 call
 * With every scale code 127 each call equals its unscaled call above in bits.
 * The narrowing in bsmr_sddmm_b8_mx is exact, wherever the product is finite, with BSMR_COMPUTE_BF16 for e4m3 with scale
 * codes >= 3 and e5m2 with scale codes >= 10; with BSMR_COMPUTE_F16 only for shifts e - 127 in [-15, 7] (e4m3) and [-8, 0]
 * (e5m2).  Outside these ranges it rounds or overflows to +-inf: use bf16 beside an MXFP8 Kt.
 *
 * Each function has the argument list of its unscaled form with the scales directly after the fp8 pointer, and its
 * checks in the same order; the scales pointer is checked with the other pointers: NULL is BSMR_ERR_INVALID_ARG unless
 * nnz = 0 (count = 0 for bsmr_widen_fp8_mx), no alignment is demanded.  bsmr_widen_fp8_mx: a count that is not a
 * multiple of 32 is BSMR_ERR_INVALID_ARG.  bsmr_sddmm_b8_mx dequantises into the plan's 16-bit workspace as bsmr_sddmm_b8
 * widens; the two gathers read one scale byte per source row and lane and make no copy.  Workspaces, lists, chunks and
 * reproducibility are those of the unscaled calls. */
int bsmr_widen_fp8_mx(const void *in8_dev, const void *scales_dev, void *out16_dev, uint64_t count, int compute_mode,
                      int fp8_format, void *stream);
int bsmr_sddmm_b8_mx(bsmr_plan *plan, uint32_t K, const void *A16_dev, const void *B8_dev, const void *B_scales_dev,
                     float *P_dev, uint32_t num_batches, int compute_mode, int fp8_format, void *stream);
int bsmr_spmm_x8_mx(bsmr_backward *bw, uint32_t K, int transpose, const float *v_dev, const void *X8_dev,
                    const void *X_scales_dev, void *Y16_dev, uint32_t num_batches, int compute_mode, int fp8_format,
                    void *stream);
int bsmr_sparse_attention_x8_mx(bsmr_backward *bw, uint32_t Kv, float scale, const float *P_dev, const void *V8_dev,
                                const void *V_scales_dev, void *O16_dev, float *m_dev, float *s_dev, uint32_t num_batches,
                                int compute_mode, int fp8_format, void *stream);

/* ---- MXFP4 keys and values (revision 5, added without any layout change; no reference counterpart) ----
 * The column-side operand of the four calls above in the smallest OCP Microscaling format, as an MXFP4 KV cache holds it.
 *   Element  OCP e2m1, 4 bits: bit 3 the sign, bits 2:0 the magnitude code; codes 0 .. 7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6.
 *            No infinity, no NaN; code 8 is -0 and keeps its sign.
 *   Packing  element 2i of a row is the low nibble (bits 3:0) of byte i, element 2i + 1 the high nibble - the layout of
 *            torch.float4_e2m1fn_x2.  A row of K elements is K / 2 bytes (K a positive multiple of 32: a multiple of 16
 *            bytes), the batch stride rows * K / 2 bytes; the array is 16-byte aligned.
 *   Scales   exactly those of "MX block scales": uint8 [b][rows][K / 32], one E8M0 code per 32 consecutive elements (16
 *            bytes), contiguous, read by byte loads at any alignment; code e is 2^(e - 127), e = 0 the fp32 subnormal
 *            2^-127, e = 255 NaN.  They are mandatory: there is no unscaled fp4 call; scale code 127 gives the plain values.
 *
 * Numerical contract.  dq(X4, E)[r][k] = widen(code[r][k]) * 2^(E[r][k / 32] - 127): one IEEE fp32 multiplication of the
 * exactly widened code, made before the element enters the fma chain (the scale is not folded into the weight).  The
 * product is exact for every scale code 0 .. 254 (subnormal results are kept: 0.5 * 2^-127 = 2^-128), finite for every
 * code up to scale code 252; from 253 on the large magnitudes overflow to +-inf; scale code 255 makes every element NaN,
 * the zeros included.  With narrow = the cast of the 16-bit forms:
 *   bsmr_widen_fp4_mx(in4, scales, out16, count)   out16[i] = narrow(dq(in4, scales)[i]); count elements, a multiple of 32
 *                                                  (in4 holds count / 2 bytes)
 *   bsmr_sddmm_b4_mx(A16, B4, Bs)               == bsmr_sddmm_16(A16, narrow(dq(B4, Bs)))
 *   bsmr_spmm_x4_mx(v, X4, Xs)                  == narrow(bsmr_spmm(v, dq(X4, Xs))), each output rounded once; both directions
 *   bsmr_sparse_attention_x4_mx(P, V4, Vs)      == bsmr_sparse_attention(P, dq(V4, Vs)) with O rounded once; m and s are
 *                                                  bit for bit those of the fp32 call
 * Every e2m1 value is an e4m3 value, so each call also equals, bit for bit, its _x8_mx / _b8_mx form (BSMR_FP8_E4M3) on
 * the re-encoded codes with the same scales.  The narrowing in bsmr_sddmm_b4_mx is exact with BSMR_COMPUTE_BF16 for all
 * 256 scale codes (a bf16 has fp32's exponent range and e2m1 needs two significand bits); with BSMR_COMPUTE_F16 it is
 * exact only for shifts e - 127 in [-23, 13] (scale codes 104 .. 140) - below, 0.5 and 1.5 fall under fp16's smallest
 * subnormal step, above, 6 * 2^14 overflows.  Use bf16 beside an MXFP4 Kt.
 *
 * compute_mode is BSMR_COMPUTE_F16 or BSMR_COMPUTE_BF16.  Checked before any device work, in the order of the fp8 forms:
 * a NULL plan / handle or a non-finite scale (BSMR_ERR_INVALID_ARG), K = 0 or not a multiple of 32
 * (BSMR_ERR_UNSUPPORTED_K), compute_mode, then the pointers - 16 bytes for the fp4 and the 16-bit arrays, 4 for P, v, m
 * and s; the scales NULL only where nothing is read (nnz = 0; count = 0), at any alignment - and more than 65535 batches.
 * num_batches = 0 is a no-op behind them.  bsmr_widen_fp4_mx: a count that is not a multiple of 32 is
 * BSMR_ERR_INVALID_ARG, count = 0 a no-op whatever the pointers.  bsmr_sddmm_b4_mx dequantises into the plan's 16-bit
 * workspace as bsmr_sddmm_b8_mx does; the two gathers read K / 2 bytes per source row (row and batch offsets formed in
 * 64 bits) and one scale byte per source row and lane, and make no copy.  Workspaces (bsmr_backward_reserve /
 * bsmr_sparse_attention_reserve), lists, chunks and reproducibility are those of the 16-bit calls.
 * Out of scope: MXFP6, fp8 scales per 16 elements (NVFP4), fp4 on the scaled MFMA of the dense engine, fp4 outputs or
 * row-side operands. */
int bsmr_widen_fp4_mx(const void *in4_dev, const void *scales_dev, void *out16_dev, uint64_t count, int compute_mode,
                      void *stream);
int bsmr_sddmm_b4_mx(bsmr_plan *plan, uint32_t K, const void *A16_dev, const void *B4_dev, const void *B_scales_dev,
                     float *P_dev, uint32_t num_batches, int compute_mode, void *stream);
int bsmr_spmm_x4_mx(bsmr_backward *bw, uint32_t K, int transpose, const float *v_dev, const void *X4_dev,
                    const void *X_scales_dev, void *Y16_dev, uint32_t num_batches, int compute_mode, void *stream);
int bsmr_sparse_attention_x4_mx(bsmr_backward *bw, uint32_t Kv, float scale, const float *P_dev, const void *V4_dev,
                                const void *V_scales_dev, void *O16_dev, float *m_dev, float *s_dev, uint32_t num_batches,
                                int compute_mode, void *stream);

/* ---- Blocked SpMM:Y = S_v X over the RPHM's dense 16 x 16 blocks (revision 5, added without any layout change) ----
 * The row direction of bsmr_spmm with the dense part of the reordering put to use: in a row panel the 16 columns of a
 * dense block are shared by 16 output rows, so a row of X is read once per block instead of once per stored entry and the
 * block is multiplied on v_mfma_f32_16x16x4_f32.  Opt-in: a handle serves these calls after
 * bsmr_backward_attach_blocks; every other call on it is unchanged.  Only Y = S_v X (the rows of S as destinations); the
 * column direction (transpose = 1, dB, dX) stays on the gather.
 *
 * Numerical contract.  Row r is row i of panel p (r = reordered_rows[16 p + i]), the panel's blocks are b0 .. b(nb-1) in
 * block_offsets order.
 *   Block chain  B[r,k]: one sequential fp32 fmaf chain from +0 over the blocks in order and, inside a block, over the
 *                column positions j = 0 .. 15 in order: acc = fmaf(a_ij, x_j[k], acc), with a_ij = v[t] where
 *                block_values[b][i][j] = t is a CSR index and +0 where the cell is empty (0xFFFFFFFF); x_j is row
 *                dense_cols[16 b + j] of X and, for a padding column (id N), a row of +0 that is never loaded.  This is
 *                what the instruction computes when MFMA s of a block takes the positions 4 s .. 4 s + 3: a k-ordered fmaf
 *                chain with one rounding per product (the exact-fp32 forward kernel is pinned to the same fact,
 *                oracle_dense_f32_twin).
 *   Residue      R[r,k]: the gather contract of "SDDMM backward" applied to the row's residue entries in ascending CSR
 *                index - one chain from +0, a list longer than BSMR_BACKWARD_CHUNK cut into chunks, the partials added in
 *                chunk order.
 *   Result       Y[r,k] = fl(B[r,k] + R[r,k]), one fp32 addition, for the rows of panels that have at least one block;
 *                Y[r,:] = R[r,:], the same bits, for the rows of panels without blocks; rows in no panel (empty rows)
 *                are exactly +0.
 * No atomics: every element has one writer, results are bitwise reproducible call to call, stream to stream and batch to
 * batch.  They depend on the attached RPHM (its block order and its dense / residue split), so unlike bsmr_spmm they are
 * NOT independent of the reordering: another row_order, alpha or delta gives another summation order.
 * Empty cells - the one semantic difference from bsmr_spmm: an empty cell multiplies +0 by a value of X that the gather
 * never reads for that row.  With finite X this changes nothing (fmaf(0, x, acc) = acc, apart from -0 -> +0).  If X[c,k]
 * is +-inf or NaN, every row of every panel that holds c as a block column but does not store (r, c) gets NaN in feature
 * k, where the gather leaves that row alone; rows that store c behave as in the gather.
 * Error bound:  |Y - Y64| <= (max(16 nb, n_r) + 4) u sum|v||x|,  u = 2^-24, n_r the row's residue count (each term passes
 * at most 16 nb roundings of the block chain or n_r + 1 of the residue, then one more addition; two units cover second
 * order), plus the subnormal term of DESIGN.md 10 where products underflow.
 * 16-bit form (bsmr_spmm_blocked_16): X is fp16 / bf16 rows, widened exactly; the contract above applies to the widened
 * values; Y16 = round(Y) is applied once, after the final addition (B and R are added in fp32), with the casts of
 * bsmr_spmm_16.
 *
 * Split panels.  bsmr_backward_attach_blocks_split takes segment_blocks = S.  S = 0 means no splitting: the contract above,
 * word for word.  With S >= 1 the blocks b0 .. b(nb-1) of a panel are cut into ceil(nb / S) consecutive segments of S
 * blocks, the last one shorter, in block_offsets order, and the block chain above is replaced by
 *   Segment chain  each segment is its own fp32 fmaf chain from +0 over its blocks in order and the positions j = 0 .. 15
 *                inside each block, exactly as the block chain runs; empty cells and padding columns behave as above.
 *   Block part   B[r,k] = ((p0 + p1) + p2) + ..., fp32 additions of the segment sums in segment order.
 *   Result       Y = fl(B + R), rounded once in the 16-bit form; R is unchanged.
 * This is the chunk rule of the residue applied to the block list with a chunk of 16 S positions.  A panel with nb <= S has
 * one segment and keeps the unsplit bits; S >= max_blocks_per_panel reproduces bsmr_backward_attach_blocks bit for bit.
 * The result is still bitwise reproducible, with no atomics and one writer per element (a segment of a split panel writes
 * fp32 partial rows of the workspace, one more kernel adds them in order); the empty-cell rule is unchanged.
 * Error bound:  (max(16 min(nb, S) + ceil(nb / S) - 1, n_r) + 4) u sum|v||x|, plus the subnormal term as above.
 *
 * bsmr_blocked_check: host only, no device, like bsmr_csr_transpose - whether `desc` is a partition of the CSR into block
 * cells and residue entries, and its statistics.  BSMR_ERR_INVALID_ARG: a NULL argument, a CSR that bsmr_backward_create
 * would refuse, desc->M / N / nnz different from M / N / nnz.  BSMR_ERR_BAD_PLAN: a CSR index missing from, or listed twice
 * across, block_values and sparse_values; a block cell whose entry's row is not reordered_rows[16 p + i] or whose column
 * is not dense_cols[16 b + j]; a non-empty cell in a padding column; a column id above N; a residue entry whose (relative
 * row, column) disagrees with the CSR; a non-monotone offset array (or one that does not start at 0); a duplicate or
 * out-of-range reordered_rows; num_row_panels other than ceil(num_nonzero_rows / 16).  Otherwise the statistics are
 * written, at most out_size bytes of them (the struct only grows at its end).
 * bsmr_blocked_check_split is the same check with the segment statistics of S = segment_blocks filled in;
 * bsmr_blocked_check is its S = 0 call.
 *
 * bsmr_backward_attach_blocks: runs the same check against the handle's CSR before any device call, then builds and uploads
 * the device format: per block 64 bytes of column ids and 1 KiB of cells (CSR index or null) in the lane order of the
 * kernel, per panel with blocks its rows, and the residue as per-row gather lists (every row of S has one, in ascending
 * CSR index, chunked by BSMR_BACKWARD_CHUNK; rows of panels without blocks write Y, rows of panels with blocks an fp32
 * staging row).  A second attach on one handle is BSMR_ERR_INVALID_ARG.  bsmr_backward_attach_blocks_split: the same with
 * segment_blocks = S (any value; the handle keeps it, bsmr_spmm_blocked[_16] need no argument for it), and for S >= 1 one
 * 16-byte record per segment and 12 bytes per split panel on top; bsmr_backward_attach_blocks is its S = 0 call, same
 * argument rules and error codes.  bsmr_backward_get_blocked_stats: the statistics of the attached desc and S with
 * device_index_bytes filled in; BSMR_ERR_BAD_PLAN without attached blocks.
 * Workspace, in this order: the chunk partials of the residue [b][slots][K]; the staging rows, 16 K floats per panel with
 * blocks and batch; the segment partials, 16 K floats per segment of a split panel and batch.  On a handle with attached
 * blocks bsmr_backward_reserve(K, num_batches) covers all three (the layout of every other call is unchanged: chunk
 * partials first); after it the blocked calls allocate nothing and can be captured in a graph.
 *
 * bsmr_spmm_blocked / bsmr_spmm_blocked_16 follow the argument rules of bsmr_spmm / bsmr_spmm_16 (transpose 0), checked
 * before any device work: a NULL handle is BSMR_ERR_INVALID_ARG, K = 0 or not a multiple of 32 BSMR_ERR_UNSUPPORTED_K, more
 * than 65535 batches or a compute_mode other than BSMR_COMPUTE_F16 / _BF16 BSMR_ERR_INVALID_ARG, a handle without attached
 * blocks BSMR_ERR_BAD_PLAN, then the pointers (16 bytes for X and Y, 4 for v).  num_batches = 0 is a no-op; with nnz = 0 v
 * and X may be NULL and Y is all zeros.  Nothing is read outside v and X or written outside Y (M K, N K, nnz elements, times
 * num_batches); all addresses are formed in 64 bits.  One wave's serial loop runs over a panel's blocks on a handle
 * attached with S = 0 (max_blocks_per_panel says how long the longest is) and over a segment's, at most S, with S >= 1
 * (max_blocks_per_segment; `segments` is the number of such loops per group of 64 features and batch). */
typedef struct bsmr_blocked_stats {
    uint32_t panels;               /* row panels of the desc                                                  */
    uint32_t panels_with_blocks;
    uint64_t blocks;               /* dense 16 x 16 blocks                                                    */
    uint64_t block_entries;        /* stored entries in block cells: fill = block_entries / (256 blocks)      */
    uint64_t padding_columns;      /* block columns with the id N                                             */
    uint64_t residue_entries;
    uint32_t max_residue_row;      /* most residue entries of one row                                         */
    uint32_t split_residue_rows;   /* rows whose residue is longer than BSMR_BACKWARD_CHUNK                   */
    uint32_t max_blocks_per_panel;
    uint32_t residue_items;        /* work items of the residue gather: one per row of S (a row without residue
                                      zeroes its destination), one per chunk of a split row                   */
    uint64_t device_index_bytes;   /* bsmr_backward_get_blocked_stats: the arrays attach uploaded; 0 from bsmr_blocked_check */
    /* split panels; with S = 0: 0, 0, panels_with_blocks, max_blocks_per_panel */
    uint32_t segment_blocks;       /* S                                                                        */
    uint32_t split_panels;         /* panels with more than S blocks                                           */
    uint32_t segments;             /* work units: over the panels with blocks, the sum of ceil(nb / S)         */
    uint32_t max_blocks_per_segment;
} bsmr_blocked_stats;
int bsmr_blocked_check(uint32_t M, uint32_t N, uint32_t nnz, const uint32_t *row_offsets, const uint32_t *col_indices,
                       const bsmr_rphm_desc *desc, bsmr_blocked_stats *out, size_t out_size);
int bsmr_blocked_check_split(uint32_t M, uint32_t N, uint32_t nnz, const uint32_t *row_offsets, const uint32_t *col_indices,
                             const bsmr_rphm_desc *desc, uint32_t segment_blocks, bsmr_blocked_stats *out, size_t out_size);
int bsmr_backward_attach_blocks(bsmr_backward *bw, const bsmr_rphm_desc *desc);
int bsmr_backward_attach_blocks_split(bsmr_backward *bw, const bsmr_rphm_desc *desc, uint32_t segment_blocks);
int bsmr_backward_get_blocked_stats(const bsmr_backward *bw, bsmr_blocked_stats *out, size_t out_size);
int bsmr_spmm_blocked(bsmr_backward *bw, uint32_t K, const float *v_dev, const float *X_dev, float *Y_dev,
                      uint32_t num_batches, void *stream);
int bsmr_spmm_blocked_16(bsmr_backward *bw, uint32_t K, const float *v_dev, const void *X16_dev, void *Y16_dev,
                         uint32_t num_batches, int compute_mode, void *stream);

/* Host operands in, host P out (upload, `iters` timed repetitions after one
 * warm-up, download).  ms_per_iter may be NULL. */
int bsmr_sddmm_host(bsmr_plan *plan, uint32_t K, const float *A_host, const float *B_host,
                    float *P_host, int compute_mode, int iters, float *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* BSMR_HIP_H */
