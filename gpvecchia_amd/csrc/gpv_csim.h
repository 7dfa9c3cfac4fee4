// gpv_csim.h — launchers of the conditional simulation of a cond.yz='z' plan over a map (gpv_plan_cond_sim, gpv_csim.hip): the
// factor pass (one solve per prediction location over its mixed neighbour list) and the level-scheduled sweep that turns the
// coefficients into means and draws.  Not installed.
#pragma once
#include "gpv_krige.h"

namespace gpv {

constexpr int kCsimLanes = 16;                     // lanes per row of the sweep: (16 / CP neighbour slots) x (CP columns)
constexpr int kCsimMaxCols = 16;                   // = kKrigeMaxCols = kUnwhitenMaxCols
constexpr int kCsimWideThreads = 256;              // a WIDE level: workgroups of 256 threads, 16 rows each
constexpr int kCsimWideRows = kCsimWideThreads / kCsimLanes;
constexpr int kCsimNarrowThreads = 1024;           // a run of NARROW levels: ONE workgroup, 64 rows per step
constexpr int kCsimNarrowRows = kCsimNarrowThreads / kCsimLanes;
constexpr int kCsimNarrow = 256;                   // rows of a narrow level at most (gpv_unwhiten.h: the same figure)
constexpr int64_t kCsimChunk = 1 << 18;            // rows per launch of the factor pass by default

// The factor pass.  k: the krige pass's arguments (records, covariance, nuggets, data columns); of them q, mean and var are not
// read, nnq is the list of ALL sweep rows and nq the rows of this launch.
struct CsimFactorArgs {
    KrigeArgs k;
    const double *qall;      // [nrows][dim] every prediction location of the call, in sweep order
    int64_t row0;            // first sweep row of this launch
    int64_t nrows;           // sweep rows of the call: the stride of a
    int64_t Nlocs;           // ids 1 .. Nlocs: ORDERED observations; Nlocs + 1 + p: sweep row p
    double *coef;            // [nrows][m] out: c_ij on the slots that hold a prediction location, 0 elsewhere
    double *sd;              // [nrows] out
    double *a;               // [ncols][nrows] out: sum over the observation slots of c_ij z_j
};

struct CsimSweepArgs {
    const double *coef;      // [nrows][m]
    const int32_t *nn;       // [nrows][m]
    double *X;               // [nrows][CP]: the right-hand sides on entry, the solution on return; read AND written
    const int32_t *order;    // [nrows] sweep rows level by level, ascending inside a level
    const int32_t *levptr;   // [levels + 1] (read by the narrow-run launch only)
    int64_t Nlocs;
    int m;
};

hipError_t launch_csim_factor(const CsimFactorArgs &a, int grid, hipStream_t s);
// X[i][cp] <- in[c * ld + i] (times sd[i] when sd is given), zeros in the columns ncols .. cp - 1
hipError_t launch_csim_pack(const double *in, int64_t ld, const double *sd, int64_t n, int ncols, int cp, double *X, hipStream_t s);
// out[c * n + i] <- X[i][cp]
hipError_t launch_csim_unpack(const double *X, int64_t n, int ncols, int cp, double *out, hipStream_t s);
// X[i][16] <- sd[i] * the standard normals of (seed, id0 + i, draws draw0 .. draw0 + 15) (gpv_philox.hpp); draw0 a multiple of 16
hipError_t launch_csim_normals(double *X, const double *sd, int64_t n, uint64_t seed, int64_t id0, int64_t draw0, hipStream_t s);
// one wide level: the rows order[lo .. hi)
hipError_t launch_csim_wide(const CsimSweepArgs &a, int cp, int64_t lo, int64_t hi, hipStream_t s);
// one run of narrow levels lev0 .. lev1 - 1 in ONE workgroup
hipError_t launch_csim_narrow(const CsimSweepArgs &a, int cp, int lev0, int lev1, hipStream_t s);

}  // namespace gpv
