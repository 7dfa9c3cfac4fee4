// gpv_unwhiten.h — launchers of the colouring pass behind gpv_plan_unwhiten / gpv_plan_simulate (gpv_unwhiten.hip).  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpv {

// Geometry: that of the whitening pass (gpv_whiten.h).  16 lanes per conditioning set, laid out as (16 / CP neighbour slots) x
// (CP columns), CP the padded column count (1, 2, 4, 8, 16); the CP values of one location are contiguous.
constexpr int kUnwhitenLanes = 16;
constexpr int kUnwhitenMaxCols = 16;               // = kWhitenMaxCols
// a WIDE level is one launch of workgroups of 256 threads (16 sets each) over the level's slice of the level-ordered set list
constexpr int kUnwhitenWideThreads = 256;
constexpr int kUnwhitenWideSets = kUnwhitenWideThreads / kUnwhitenLanes;
// a run of consecutive NARROW levels (at most kUnwhitenNarrow rows each) is one launch of ONE workgroup of 1024 threads, 64 sets
// per step, with a workgroup barrier between the levels: a level of that width is at most four steps of the one workgroup,
// about what the launch costs that it replaces, and most narrow levels are one step
constexpr int kUnwhitenNarrowThreads = 1024;
constexpr int kUnwhitenNarrowSets = kUnwhitenNarrowThreads / kUnwhitenLanes;
constexpr int kUnwhitenNarrow = 256;               // gpv_unwhiten_narrow()

struct UnwhitenArgs {
    const double *L;         // [rows][P] U entries by OUTPUT row, left-aligned, the row's own entry d_k last (SetArgs::Lentries)
    const int32_t *nn;       // [rows][P] internal position of each neighbour, valid entries right-aligned, -1 = missing
    const int32_t *rowid;    // [rows] output row of each stored set
    const double *nuggets;   // [Nlocs] nuggets by internal position, or nullptr: nug_scalar
    const double *E;         // [rows][CP] the standard columns by OUTPUT row, zero in the columns >= ncols
    double *B;               // [Nlocs][CP] the coloured columns by internal position: read (earlier levels) AND written
    const int32_t *order;    // [rows] stored sets level by level, ascending inside a level
    const int32_t *levptr;   // [levels + 1] where each level starts in `order` (read by the narrow-run launch only)
    unsigned *nfail;         // ONE counter: rows whose block was not positive definite (an integer count: order-free)
    int P;
    double nug_scalar;
};

// in: ncols columns of length n, n apart (ORDERED layout) -> E[k][cp], zeros in the columns ncols .. cp - 1
hipError_t launch_unwhiten_pack(const double *in, int64_t n, int ncols, int cp, double *E, hipStream_t s);
// B[newpos[i]][cp] -> out: ncols columns of length n, n apart (ORDERED layout)
hipError_t launch_unwhiten_unpack(const double *B, const int32_t *newpos, int64_t n, int ncols, int cp,
                                                       double *out, hipStream_t s);
// E[k][16] <- the standard normals of ordered location k, draws draw0 .. draw0 + 15 (gpv_philox.hpp); draw0 a multiple of 16
hipError_t launch_unwhiten_normals(double *E, int64_t n, uint64_t seed, int64_t draw0, hipStream_t s);
// one wide level: the sets order[lo .. hi)
hipError_t launch_unwhiten_wide(const UnwhitenArgs &a, int cp, int64_t lo, int64_t hi, hipStream_t s);
// one run of narrow levels lev0 .. lev1 - 1 in ONE workgroup
hipError_t launch_unwhiten_narrow(const UnwhitenArgs &a, int cp, int lev0, int lev1, hipStream_t s);

}  // namespace gpv
