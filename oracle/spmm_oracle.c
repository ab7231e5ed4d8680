/*
 * oracle/spmm_oracle.c -- TEST INFRASTRUCTURE ONLY.
 *
 * Bit-exact fp32 twin of the SDDMM backward's gather-and-accumulate
 * (bsmr-sddmm_amd/csrc/spmm_kernels.hpp; include/bsmr_hip.h "SDDMM backward",
 * DESIGN.md section 9).  The product never links, imports or calls it.
 *
 * The caller supplies the destination lists (built independently of the
 * library, e.g. a stable argsort transpose in numpy):
 *   Y[d,k] = sum over t in [offsets[d], offsets[d+1]) of v[eidx[t]] * X[src[t],k]
 * Contract restated:
 *   - each list runs as a sequential fmaf chain in list order from acc = +0.0f;
 *   - a list longer than `chunk` entries is cut into consecutive chunks of
 *     `chunk` entries, each its own chain from +0.0f, and the chunk partials
 *     are added left to right: ((p0 + p1) + p2) + ...;
 *   - subnormals are kept (no flush), NaN and inf propagate as IEEE says.
 * Built with -ffp-contract=off, so the chunk sums are separate adds.
 * X and Y are row-major with K floats per row.
 */
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>

void oracle_gather_twin(uint32_t num_dest, uint32_t K, uint32_t chunk,
                        const uint32_t *offsets, const uint32_t *src, const uint32_t *eidx,
                        const float *v, const float *X, float *Y)
{
#pragma omp parallel
    {
        float *acc = (float *)malloc(sizeof(float) * (K ? K : 1));
#pragma omp for schedule(dynamic, 16)
        for (int64_t d = 0; d < (int64_t)num_dest; ++d) {
            const uint32_t b = offsets[d], e = offsets[d + 1];
            float *y = Y + (size_t)d * K;
            uint32_t c0 = b;
            do {   /* one chunk: its own chain from +0, k innermost so that a source row is read contiguously */
                const uint32_t c1 = (chunk && e - c0 > chunk) ? c0 + chunk : e;   /* chunk 0: one chain */
                for (uint32_t k = 0; k < K; ++k) acc[k] = 0.0f;
                for (uint32_t t = c0; t < c1; ++t) {
                    const float w = v[eidx[t]];
                    const float *x = X + (size_t)src[t] * K;
                    for (uint32_t k = 0; k < K; ++k) acc[k] = fmaf(w, x[k], acc[k]);
                }
                for (uint32_t k = 0; k < K; ++k) y[k] = (c0 == b) ? acc[k] : y[k] + acc[k];
                c0 = c1;
            } while (c0 < e);
        }
        free(acc);
    }
}
