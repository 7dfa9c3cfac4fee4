// gpv_whiten.h — launchers of the whitening pass and of the Gram pass behind gpv_plan_whiten (gpv_whiten.hip).  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpv {

constexpr int kWhitenMaxCols = 16;     // columns per call (gpv_whiten_max_cols)
// Geometry of the whitening pass: 16 lanes per conditioning set, four sets per wavefront, four wavefronts per workgroup.  With CP
// the padded column count (1, 2, 4, 8, 16) the 16 lanes of a set are 16 / CP neighbour slots x CP columns: one neighbour's CP
// values are one contiguous read of 8 CP bytes, and a wavefront instruction gathers 64 / CP neighbours' rows.
constexpr int kWhitenLanes = 16;
constexpr int kWhitenThreads = 256;
constexpr int kWhitenSetsPerBlock = kWhitenThreads / kWhitenLanes;
constexpr int kWhitenBlocksPerCU = 5;  // grid cap: what is resident at once (73 to 85 VGPRs: 5 wavefronts per SIMD, 5 workgroups per CU)
constexpr int kWhitenNV = 2;           // per-workgroup partials of the pass: {sum log(tau + 1/d^2), failed rows}
// Gram pass: one 16 x 16 tile per workgroup of 256 threads (thread = one entry), rows staged through LDS kGramRows at a time
constexpr int kGramThreads = 256;
constexpr int kGramRows = 64;
constexpr int kGramBlocksPerCU = 2;
constexpr int kGramTile = kWhitenMaxCols * kWhitenMaxCols;
constexpr int kWhitenTotals = kGramTile + kWhitenNV;     // totals: the 16 x 16 Gram matrix (row-major), then the kWhitenNV sums

struct WhitenArgs {
    const double *L;         // [rows][P] U entries by OUTPUT row, left-aligned, the row's own entry d_k last (SetArgs::Lentries)
    const int32_t *nn;       // [rows][P] internal position of each neighbour, valid entries right-aligned, -1 = missing
    const int32_t *rowid;    // [rows] output row of each stored set
    const double *nuggets;   // [Nlocs] nuggets by internal position, or nullptr: nug_scalar
    const double *B;         // [Nlocs][CP] the columns by internal position, zero in the columns >= ncols
    double *E;               // [rows][CP] whitened columns by OUTPUT row; NaN in a row whose block was not positive definite
    double *part;            // [grid][kWhitenNV] per-workgroup partials
    int64_t rows;
    int P;
    double nug_scalar;
};

// padded column count of a call with ncols columns: the next power of two
inline int whiten_cp(int ncols) { int cp = 1; while (cp < ncols) cp <<= 1; return cp; }
int whiten_grid(int64_t rows, int cus);
int whiten_gram_grid(int64_t rows, int cus);
// in: ncols columns of length n, n apart (ORDERED layout) -> B[newpos[i]][cp], zeros in the columns ncols .. cp - 1
hipError_t launch_whiten_pack(const double *in, const int32_t *newpos, int64_t n, int ncols, int cp, double *B, hipStream_t s);
// E[n][cp] -> out: ncols columns of length n, n apart
hipError_t launch_whiten_unpack(const double *E, int64_t n, int ncols, int cp, double *out, hipStream_t s);
// the whitening pass (one launch): E and the per-workgroup partials
hipError_t launch_whiten(const WhitenArgs &a, int cp, int grid, hipStream_t s);
// the Gram pass: per-workgroup partial tiles of E^T E (gpart: [ggrid][kGramTile]), then ONE workgroup that adds the tiles and the
// whitening pass's partials (wpart: [wgrid][kWhitenNV]) in workgroup order into totals[kWhitenTotals]
hipError_t launch_whiten_gram(const double *E, int64_t n, int cp, int ggrid, double *gpart, const double *wpart, int wgrid,
                              double *totals, hipStream_t s);

}  // namespace gpv
