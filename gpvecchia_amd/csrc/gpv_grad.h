// gpv_grad.h — launcher of the value-and-gradient kernel of the cond.yz='z' log-likelihood (gpv_grad.hip).  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpv_bessel.hpp"

namespace gpv {

constexpr int kGradMaxP = 64;          // longest row (m + 1) the kernel takes: one lane per row of the block
constexpr int kGradNV = 8;             // values per row / partial: {l, d/d(kernel parameter 0..4), failed, rows}
constexpr int kGradRowLd = 6;          // doubles per row of GradArgs::row_terms: {l_k, its derivatives}
// kernel parameters, in this order (the smoothness of "matern" is not one of them):
//   matern: variance, range, nugget                      esqe: variance 1, range 1, variance 2, range 2, nugget
//   matern at a general smoothness (COV_MATERN_GEN, the _nu entries): variance, range, smoothness, nugget
//   matern_scaledim (kCovScaled05 / 15 / 25, dimension <= 3): variance, range_1, range_2, range_3, nugget; the kernels always
//   carry three ranges, a coordinate the plan does not have differs by exactly 0 in every pair, its slot sums exact zeros and
//   the host drops it.  Five slots are what kGradNV and kFisherTri hold, hence the limit of three dimensions.
constexpr int kCovScaled05 = 6, kCovScaled15 = 7, kCovScaled25 = 8;   // GradArgs::cov beyond CovKind: COV_MATERN05 / 15 / 25 + 6
constexpr int kGradWavesPerBlock = 4;
// Grid cap: 4 workgroups of 4 wavefronts per CU, 4096 wavefronts on the 256 CUs of an MI355X.  At n = 40 000 every wavefront
// then takes 9 or 10 conditioning sets; the per-workgroup partials (kGradNV doubles each) stay a few KB.
constexpr int kGradBlocksPerCU = 4;

struct GradArgs {
    const double *rec;       // SetArgs::rec   (dim <= 3: {c0, c1, c2, datum})
    const double *locs;      // SetArgs::locs  (dim > 3)
    const double *z;         // SetArgs::z     (dim > 3)
    const int32_t *nn;       // [rows][P], valid entries right-aligned (gpv_plan_create compacts them), -1 = missing
    const int32_t *rowid;    // [rows] output row of each stored set
    double *row_terms;       // [rows][kGradRowLd] by OUTPUT row, or nullptr; NaN in a row whose block was not positive definite
    double *block_part;      // [grid][kGradNV] per-workgroup partials
    double *totals;          // [kGradNV] their sum in workgroup order (second launch)
    int64_t rows;
    int P;                   // row stride of nn (the plan's compiled row length; may be shorter than the bucket)
    int dim, locs_ld;
    int cov;                 // CovKind: COV_MATERN05 / 15 / 25 / COV_ESQE / COV_MATERN_GEN, or kCovScaled05 / 15 / 25
    double sA, cA, irA;      // matern: sigma^2, sqrt(2 nu)/range, 1/range        esqe: s1, 1/r1, 1/r1     scaled: sigma^2, sqrt(2 nu), 1/range_1
    double sB, cB, irB;      // esqe: s2, 1/r2^2, 1/r2                                                  scaled: 1/range_3, -, 1/range_2
    double nug;
    // COV_MATERN_GEN only (sA = sigma^2, cA = irA = 1/range): the smoothness and its constants, and the launch's tables of the
    // e^s-scaled value, range derivative and smoothness derivative (gpv_bessel.hpp, MaternDTab), or gmt_nseg = 0: no table
    MaternDerivConst gen;
    const double *gmt;       // [gmt_nseg][MaternDTab::ROW]
    int gmt_base, gmt_nseg;  // segment of s = (bits(s) >> 49) - gmt_base
    // kCovScaled*: rec is the copy with the coordinates divided by their ranges (launch_scale_locs), sA = sigma^2, cA = 1, sqrt(3),
    // sqrt(5) (range 1), and the three inverse ranges 1 / range_t (0 for an absent coordinate) stand in irA, irB, sB, which
    // these kinds do not use otherwise.  No member of their own: the argument block keeps the layout every other kernel was
    // compiled against (the general-nu replicate kernels reload arguments inside their loops and change with it).
};

// the Fisher mode of the kernel (kSetsFisher) takes the same GradArgs with longer rows and partials: after {l_k, derivatives} comes
// the upper triangle (row-major, i <= j) of the row's expected information over the kernel parameters, 6 entries for matern, 10
// for matern at a general smoothness and 15 for esqe and matern_scaledim, zeros behind them
constexpr int kFisherTri = 15;
constexpr int kFisherRowLd = kGradRowLd + kFisherTri;    // doubles per row of row_terms
constexpr int kFisherNV = kGradNV + kFisherTri;          // values per partial: the kGradNV of the gradient, then the triangle

// the replicate mode (kSetsRep, gpv_rep_kernel.hpp): the same rows, partials and totals as the Fisher mode, summed over R
// replicates of the data.  The kernel reads no datum of GradArgs (rec's fourth slot, z) but the replicates below.
constexpr int kRepChunk = 8;           // replicates a lane reads and reduces together; RP is a multiple of it
struct RepArgs {
    GradArgs g;
    const double *Z;         // [Nlocs][RP] the replicates by internal position, zeros in the columns R .. RP - 1; 16-byte aligned
    int R, RP;
};
// padded replicate count
inline int rep_rp(int R) { return (R + kRepChunk - 1) / kRepChunk * kRepChunk; }

// row-length bucket of a row of p entries (16, 32 or 64), 0: too long
inline int grad_bucket(int p) { return p <= 16 ? 16 : (p <= 32 ? 32 : (p <= kGradMaxP ? 64 : 0)); }
// workgroups of the launch for `rows` sets on a device of `cus` compute units
int grad_grid(int64_t rows, int cus);
// both launches (the set pass, then the fixed-order sum of its partials) on `stream`; p: entries per row (m + 1)
hipError_t launch_grad(int p, const GradArgs &a, int grid, hipStream_t stream);
// the same for value, gradient and information: row_terms [rows][kFisherRowLd], block_part [grid][kFisherNV], totals [kFisherNV]
hipError_t launch_fisher(int p, const GradArgs &a, int grid, hipStream_t stream);
// the same for R replicates: buffers of a.g as for launch_fisher
hipError_t launch_rep(int p, const RepArgs &a, int grid, hipStream_t stream);
// in: R columns of length n, n apart (ORDERED layout) -> Z[newpos[i]][rp], zeros in the columns R .. rp - 1
hipError_t launch_rep_pack(const double *in, const int32_t *newpos, int64_t n, int R, int rp, double *Z, hipStream_t stream);

}  // namespace gpv
