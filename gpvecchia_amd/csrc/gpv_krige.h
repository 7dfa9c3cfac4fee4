// gpv_krige.h — local kriging of a cond.yz='z' plan at new locations (gpv_plan_krige): the search for the nearest
// observations of query points (gpv_nn.hip) and the launcher of the predict pass (gpv_krige.hip).  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpv_bessel.hpp"

namespace gpv {

// ---- query search (gpv_nn.hip, part of every link) ---------------------------------------------------------------------------
// The observations of a search, resident on the device for the queries of every chunk: the coordinates by index (row-major,
// one burst of padding behind them, for the brute-force kernel's unguarded scalar loads), the eligibility bytes, and, in one
// to three dimensions from kQnnGridFrom searchable points on, the uniform grid over the searchable points (eligible, every
// coordinate finite).  Built from host arrays, freed by qnn_free.
constexpr int64_t kQnnGridFrom = 2048;
struct QnnGrid {
    int g[3];                 // cells per dimension
    double lo[3], inv[3];     // cell of x: (int)((x - lo) * inv), clamped
    double hmin;              // the smallest cell edge
};
struct QnnIndex {
    int64_t n = 0;
    int dim = 0;
    double *d_locs = nullptr;         // [n + 8][dim]
    unsigned char *d_elig = nullptr;  // [n + 8] 1: may enter a list (eligible and finite); padding 0
    bool grid = false;
    QnnGrid G;
    double *d_sxyz = nullptr;         // [ns][dim] coordinates of the searchable points in cell order
    int32_t *d_sidx = nullptr;        // [ns] their indices, ascending inside a cell
    int32_t *d_cstart = nullptr;      // [cells + 1]
};
// locs: n x dim column-major (host); eligible: [n] bytes or nullptr (all).  Returns hipSuccess and a filled index, or the
// failing call's status with everything freed.
hipError_t qnn_build(const double *locs, int64_t n, int dim, const unsigned char *eligible, QnnIndex &ix);
void qnn_free(QnnIndex &ix);
// d_q: [nq][dim] row-major queries on the device; d_out: [nq][m] 1-based indices by ascending distance, 0-padded
hipError_t qnn_search(const QnnIndex &ix, const double *d_q, int64_t nq, int m, int32_t *d_out, hipStream_t s);

// ---- ordered search (gpv_nn.hip): gpv_find_ordered_nn with the shard's rows written from `out` on, ld apart ------------------
// Statuses and arithmetic: those of gpv_find_ordered_nn.  out[r - row_begin + s * ld], s = 0 .. m; ld >= row_end - row_begin.
int ordered_nn_rows(int device, const double *locs, int64_t n, int dim, int m, int64_t row_begin, int64_t row_end, int *out, int64_t ld);

// ---- the predict pass (gpv_krige.hip) ---------------------------------------------------------------------------------------
constexpr int kKrigeMaxP = 64;         // m + 1: the neighbours and the query, one lane each
constexpr int kKrigeMaxCols = 16;
constexpr int kKrigeWavesPerBlock = 4;
constexpr int kKrigeBlocksPerCU = 4;
constexpr int64_t kKrigeChunk = 1 << 18;   // queries per chunk by default: 2 MB of coordinates, 31 MB of neighbours at m = 30
// covariance kinds of KrigeArgs::cov: CovKind's COV_MATERN05 / 15 / 25, COV_ESQE, COV_MATERN_GEN; matern_scaledim is one of the
// Matern kinds with nscale = the dimension: coordinate differences are multiplied by inv[t] = 1 / range_t before they are squared

struct KrigeArgs {
    const double *rec;       // the plan's records: dim <= 3: [Nlocs][4] {c0, c1, c2, datum}; else [Nlocs][locs_ld] coordinates
    const double *z;         // dim > 3: the plan's data by internal position (used when Z == nullptr)
    const int32_t *newpos;   // [Nlocs] internal position of each ORDERED location
    const double *nuggets;   // [Nlocs] by ORDERED location, or nullptr: nug
    const double *Z;         // [Nlocs][zld] data columns by internal position, or nullptr: the plan's one column
    const double *q;         // [nq][dim] the chunk's queries
    const int32_t *nnq;      // [nq][m] ORDERED ids, 1-based, 0 = none
    double *mean;            // [ncols][nq] out
    double *var;             // [nq] out
    unsigned *nfail;         // ONE counter, added to
    int64_t nq;
    int m, dim, locs_ld, ncols, zld;
    int cov, nscale;
    double sA, cA, sB, cB, nug;
    double inv[8];           // nscale > 0: 1 / range_t
    MaternDerivConst gen;    // COV_MATERN_GEN (sA = sigma^2, cA = 1 / range): GradArgs::gen, gmt, gmt_base, gmt_nseg
    const double *gmt;
    int gmt_base, gmt_nseg;
};

int krige_grid(int64_t nq, int cus);
hipError_t launch_krige(const KrigeArgs &a, int grid, hipStream_t s);

}  // namespace gpv
