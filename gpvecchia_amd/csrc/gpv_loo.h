// gpv_loo.h — launchers of the transposed whitening pass and of the leave-one-out epilogue behind gpv_plan_whiten_t /
// gpv_plan_precision / gpv_plan_loo (gpv_loo.hip), and the host builder of the transposed index.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace gpv {

// Geometry: that of the whitening pass (gpv_whiten.h).  16 lanes per location (transposed pass) or per conditioning set (forward
// pass), laid out as (16 / CP entry slots) x (CP columns), CP the padded column count (1, 2, 4, 8, 16).  Whatever CP is, a sum
// over a list of entries is taken over 16 VIRTUAL slots (entry t of the list goes to slot t mod 16, ascending inside a slot) and
// the 16 slot sums are added in one fixed tree (slot bit 3 first, bit 0 last): a lane keeps CP of the virtual slots in
// registers, the rest of the tree crosses lanes.  A column's bits therefore do not depend on the call's other columns.
constexpr int kLooLanes = 16;
constexpr int kLooMaxCols = 16;                    // = kWhitenMaxCols
constexpr int kLooThreads = 256;
constexpr int kLooGroupsPerBlock = kLooThreads / kLooLanes;
constexpr int kLooBlocksPerCU = 4;                 // grid cap of the forward, transposed and scale passes
constexpr int kLooNScores = 6;                     // gpv_loo_nscores(), GPV_LOO_NSCORES
constexpr int kLooScoreThreads = 256;
constexpr int kLooScoreBlocksPerCU = 2;            // grid cap (per column) of the score pass

struct LooArgs {
    const double *L;         // [rows][P] U entries by OUTPUT row, left-aligned, the row's own entry d_k last (SetArgs::Lentries)
    const int32_t *nn;       // [rows][P] internal position of each neighbour, valid entries right-aligned, -1 = missing
    const int32_t *rowid;    // [rows] output row of each stored set
    const double *nuggets;   // [Nlocs] nuggets by internal position, or nullptr: nug_scalar
    const int32_t *colptr;   // [Nlocs + 1] where the column of each internal position starts in col
    const int32_t *owner;    // [Nlocs] flat offset of the own entry of the (first) set that ends in the position, -1: none
    const int32_t *col;      // [colptr[Nlocs]] flat offsets (output row x P + left-aligned slot: an index into L) of the entries
                             // whose neighbour is the position, ascending in stored-set order
    double *g;               // [rows] by OUTPUT row: 1 / (d_k s_k), s_k = sqrt(tau_k + 1/d_k^2); NaN in a failed row
    unsigned *nfail;         // ONE counter: rows whose block was not positive definite (an integer count: order-free)
    const double *B;         // [Nlocs][CP] columns by internal position (forward pass: in)
    double *E;               // [rows][CP] columns by OUTPUT row (forward pass: out; transposed pass: in)
    double *R;               // [Nlocs][CP] T^T E by internal position (transposed pass: out)
    double *q;               // [Nlocs] diag(T^T T) by internal position (transposed pass: out)
    int64_t rows, n;
    int P;
    uint64_t pmagic;         // ceil(2^64 / P), 0 for P = 1: flat offset -> output row without a division (loo_pmagic)
    double nug_scalar;
};

inline uint64_t loo_pmagic(int P) { return P <= 1 ? 0 : ~(uint64_t)0 / (uint64_t)P + 1; }
int loo_grid(int64_t items, int cus);
int loo_score_grid(int64_t n, int cus);
// The transposed index of a plan's index arrays (host).  Returns 0, 1 (rows x P >= 2^31: the flat offsets are int32) or 2 (an
// index out of range, a missing entry behind a valid one).  colptr: n + 1 starts; owner: n; col: colptr[n] offsets.
int loo_build_index(const int32_t *nn, const int32_t *rowid, int64_t rows, int64_t n, int P,
                                    std::vector<int32_t> &colptr, std::vector<int32_t> &owner, std::vector<int32_t> &col);
// in: ncols columns of length n, n apart -> out[map ? map[i] : i][cp], zeros in the columns ncols .. cp - 1
hipError_t launch_loo_pack(const double *in, const int32_t *map, int64_t n, int ncols, int cp, double *out, hipStream_t s);
// in[map ? map[i] : i][cp] -> out: ncols columns of length n, n apart
hipError_t launch_loo_unpack(const double *in, const int32_t *map, int64_t n, int ncols, int cp, double *out, hipStream_t s);
// the scale pre-pass: g and the counter of failed rows (cleared by the caller)
hipError_t launch_loo_scale(const LooArgs &a, int grid, hipStream_t s);
// E = T B
hipError_t launch_loo_forward(const LooArgs &a, int cp, int grid, hipStream_t s);
// R = T^T E, q = diag(T^T T)
hipError_t launch_loo_transposed(const LooArgs &a, int cp, int grid, hipStream_t s);
// the leave-one-out epilogue on ORDERED column-major data: Z, RM [ncols][n], q [n].  RM holds r = Q z on entry and the
// leave-one-out mean on return; var[i] = 1 / q[i]; part: [ncols][grid][kLooNScores]; scores: [ncols][kLooNScores]
hipError_t launch_loo_scores(const double *Z, double *RM, const double *q, double *var, int64_t n, int ncols, int grid,
                                             double *part, double *scores, hipStream_t s);

}  // namespace gpv
