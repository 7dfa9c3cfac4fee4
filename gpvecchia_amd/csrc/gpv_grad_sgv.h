// gpv_grad_sgv.h — launcher of the gradient pass of the cond.yz='SGV' log-likelihood (gpv_grad_sgv.hip), the last of the three
// passes behind gpv_plan_loglik_grad_sgv.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpv_grad.h"

namespace gpv {

constexpr int kSgvRowLd = 5;           // doubles per row of row_terms: -1/2 c_{k,p} over the kernel parameters of gpv_grad.h
constexpr int kSgvNV = 8;              // values per partial: {the kSgvRowLd sums, -, failed, rows}

struct SgvGradArgs {
    // rec, locs, z, nn, rowid, rows, P, dim, locs_ld, cov and the family's constants as for launch_grad; row_terms
    // [rows][kSgvRowLd] by OUTPUT row or nullptr, block_part [grid][kSgvNV], totals [kSgvNV]
    GradArgs g;
    // the index data of the plan (gpv_api.hip, sgv_prepare), by STORED set:
    const uint8_t *cpos;     // [rows][P] position of the entry among the entries of the set's posterior column; 0xFF: the entry is
                             //           conditioned on as observed z, or missing
    const int4 *setrec;      // [rows] {offset of the column's block in S, its first entry in crow / pair, entries, ordered index k}
    const int32_t *crow;     // PostArgs::crow: ordered index of every column entry
    const int2 *pair;        // SelinvArgs::pair, tp, S, vars: Sigma = W^-1 on the pattern, as gpv_plan_selinv's pass leaves it
    const uint8_t *tp;
    const double *S;
    const double *vars;
    const double *mu;        // [Nlocs] W^-1 z2 by ordered index (the mean sweep's u; the posterior mean is its negative)
};

// workgroups of the launch: the wavefront cap of grad_grid (the bucket of 64 runs one wavefront per workgroup, the others four)
int grad_sgv_grid(int p, int64_t rows, int cus);
// both launches (the set pass, then the fixed-order sum of its partials) on `stream`; p: entries per row (m + 1)
hipError_t launch_grad_sgv(int p, const SgvGradArgs &a, int grid, hipStream_t stream);

}  // namespace gpv
