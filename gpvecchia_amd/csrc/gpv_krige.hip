// gpv_krige.hip — the predict pass of gpv_plan_krige: local kriging of a cond.yz='z' model at new locations, gfx950, FP64.
//
// Under the 'z' model a prediction location ordered last conditions on its m nearest observations J and on nothing else, so
// its predictive distribution is one (|J| + 1) x (|J| + 1) solve.  With the query as the LAST row,
//     S = C(J u q, J u q) + diag(tau_J, 0),   u = S^-1 e_last:
//     var_y = 1 / u_last,   mean_c = -(sum_{j in J} u_j z_{j,c}) / u_last   for each data column c
// (u_last is the reciprocal of the Schur complement of the query: the cancelling difference sigma^2 - k'K^-1 k is never formed).
// Appending the location to the plan as its last row gives loglik([z; z0]) = loglik(z) + log N(z0; mean, var_y + tau_0): the
// pass predicts with the model the likelihood scores.
//
// Geometry: that of gpv_grad.hip.  One wavefront per query, grid-stride over the chunk's queries; lane i owns row i of the block
// in registers; one kernel per row-length bucket PB in {16, 32, 64}; rows that are no neighbour (the bucket's padding IN FRONT,
// the 0-padding of a short neighbour list, lanes beyond PB) are identity rows and contribute exact zeros.  Gauss-Jordan
// elimination without pivoting, the pivot row handed out by __builtin_amdgcn_readlane, one right-hand side (e_last); the pivots
// are those of the Cholesky factorisation, so "pivot <= 0 or NaN" is the set kernels' failure test.  A failed query gets NaN
// and is counted.  Builtins only, no inline assembly.
//
// Reading: the neighbours are ORDERED ids, translated by the plan's newpos to the plan's resident records (coordinates, the
// plan's datum), its resident data (dim > 3) or the call's columns by internal position; the nuggets by ordered id.
// Reduction: every column's sum over the lanes is the same butterfly (wave_sum), so a column's bits depend neither on the
// other columns of the call nor on how the queries are chunked.
// matern_scaledim: coordinate differences are multiplied by 1 / range_t before they are squared (every other family: by 1,
// which is exact), any dimension up to 8.
#include "gpv_krige.h"
#include "gpv_internal.h"
#include "gpv_krige_dev.hpp"

namespace gpv {

namespace {

template <int PB, int COV>
__global__ void __launch_bounds__(64 * kKrigeWavesPerBlock, (PB == 16 ? 3 : (PB == 32 ? 2 : 1))) gpv_krige_kernel(const KrigeArgs A)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool packed = A.dim <= 3;
    const int64_t nwaves = (int64_t)gridDim.x * kKrigeWavesPerBlock;
    unsigned nbad = 0;
    for (int64_t k = (int64_t)blockIdx.x * kKrigeWavesPerBlock + wave; k < A.nq; k += nwaves) {
        // ---- gather: lane i takes slot m + 1 - PB + i of {neighbour 0 .. m - 1, the query}; the query sits in lane PB - 1
        const int slot = A.m + 1 - PB + lane;
        const bool isq = slot == A.m;
        const int id = (slot >= 0 && slot < A.m) ? A.nnq[k * A.m + slot] - 1 : -1;
        const bool nb = id >= 0;
        const bool valid = nb || isq;
        const int64_t v = nb ? (int64_t)A.newpos[id] : 0;
        const double tau = nb ? (A.nuggets ? A.nuggets[id] : A.nug) : (isq ? 0.0 : 1.0);
        double a[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) a[j] = 0.0;
        for (int t = 0; t < A.dim; ++t) {
            const double x = nb ? A.rec[v * (packed ? 4 : A.locs_ld) + t] : (isq ? A.q[k * A.dim + t] : 0.0);
            double sc = A.inv[0];                                     // (selects at constant indices: a run-time index would
#pragma unroll                                                        //  send the argument block's array through scratch)
            for (int i = 1; i < 8; ++i) sc = (t == i) ? A.inv[i] : sc;
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                const double df = (x - readlane_d(x, j)) * sc;
                a[j] = __builtin_fma(df, df, a[j]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- C on the valid rows and columns, zero elsewhere; the nugget joins the diagonal where the pivot is read
        const int vhi = __double2hiint(valid ? 1.0 : 0.0);
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double vj = __hiloint2double(__builtin_amdgcn_readlane(vhi, j), 0);
            const bool live = valid && vj != 0.0;
            a[j] = krige_cov<COV>(live ? a[j] : 0.0, A) * (valid ? vj : 0.0);
            __builtin_amdgcn_sched_barrier(0);                        // one exp at a time: PB interleaved ones spill
        }
        // ---- Gauss-Jordan with the right-hand side e_last
        double r1 = (lane == PB - 1) ? 1.0 : 0.0, dg = 1.0;          // dg: 1 / pivot of the lane's own row
        bool fail = false;
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double d = readlane_d(a[j], j) + readlane_d(tau, j);
            fail |= !(d > 0.0);                                      // (uniform: every lane holds the same pivot)
            const bool pivot = lane == j;
            const double inv = 1.0 / d;
            // the multiplier with one correction step: exactly 1 where the row's entry IS the pivot (a query on an observation:
            // their rows are the same bits), so with no nugget there the query's row cancels to exact zeros and its own pivot
            // fails the test instead of passing it as a rounding residue of either sign
            const double f0 = a[j] * inv;
            const double f = pivot ? 0.0 : __builtin_fma(__builtin_fma(-f0, d, a[j]), inv, f0);
            dg = pivot ? inv : dg;
#pragma unroll
            for (int c = j + 1; c < PB; ++c) a[c] = __builtin_fma(-f, readlane_d(a[c], j), a[c]);
            r1 = __builtin_fma(-f, readlane_d(r1, j), r1);
            __builtin_amdgcn_sched_barrier(0);
        }
        const double u = r1 * dg;                                    // exact zeros on the rows that are no neighbour
        const double ul = readlane_d(u, PB - 1);
        fail |= !(ul > 0.0);
        nbad += fail ? 1u : 0u;
        // ---- the columns: one butterfly each, lane c keeps column c
        double mine = 0.0;
        if (A.Z == nullptr) {
            const double zi = nb ? (packed ? A.rec[v * 4 + 3] : A.z[v]) : 0.0;
            mine = -wave_sum(u * zi) / ul;
        } else {
            const double *zr = A.Z + v * A.zld;
#pragma unroll 1
            for (int c0 = 0; c0 < A.ncols; c0 += 4) {                 // (zld is a multiple of 4: zeros behind the last column)
                double s4[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) s4[c] = u * (nb ? zr[c0 + c] : 0.0);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double s = -wave_sum(s4[c]) / ul;
                    mine = (lane == c0 + c) ? s : mine;
                }
            }
        }
        const double nan = __builtin_nan("");
        if (lane < A.ncols) A.mean[(int64_t)lane * A.nq + k] = fail ? nan : mine;
        if (lane == PB - 1) A.var[k] = fail ? nan : 1.0 / ul;
    }
    if (lane == 0 && nbad) atomicAdd(A.nfail, nbad);                 // (an integer count: order-free)
}

template <int PB>
hipError_t launch_bucket(const KrigeArgs &a, int grid, hipStream_t s)
{
    const dim3 g((unsigned)grid), b(64 * kKrigeWavesPerBlock);
    switch (a.cov) {
        case COV_MATERN05: hipLaunchKernelGGL((gpv_krige_kernel<PB, COV_MATERN05>), g, b, 0, s, a); break;
        case COV_MATERN15: hipLaunchKernelGGL((gpv_krige_kernel<PB, COV_MATERN15>), g, b, 0, s, a); break;
        case COV_MATERN25: hipLaunchKernelGGL((gpv_krige_kernel<PB, COV_MATERN25>), g, b, 0, s, a); break;
        case COV_ESQE: hipLaunchKernelGGL((gpv_krige_kernel<PB, COV_ESQE>), g, b, 0, s, a); break;
        case COV_MATERN_GEN: hipLaunchKernelGGL((gpv_krige_kernel<PB, COV_MATERN_GEN>), g, b, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

int krige_grid(int64_t nq, int cus)
{
    int64_t grid = (nq + kKrigeWavesPerBlock - 1) / kKrigeWavesPerBlock;
    const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * kKrigeBlocksPerCU;
    if (grid > cap) grid = cap;
    return (int)(grid < 1 ? 1 : grid);
}

hipError_t launch_krige(const KrigeArgs &a, int grid, hipStream_t s)
{
    const int p = a.m + 1;
    if (grid < 1 || a.nq < 0 || a.m < 1 || p > kKrigeMaxP || a.ncols < 1 || a.ncols > kKrigeMaxCols || a.dim < 1 || a.dim > 8)
        return hipErrorInvalidValue;
    if (a.Z != nullptr && (a.zld < a.ncols || a.zld % 4 != 0)) return hipErrorInvalidValue;
    if (a.Z == nullptr && a.ncols != 1) return hipErrorInvalidValue;
    if (a.nq == 0) return hipSuccess;
    return p <= 16 ? launch_bucket<16>(a, grid, s) : (p <= 32 ? launch_bucket<32>(a, grid, s) : launch_bucket<64>(a, grid, s));
}

}  // namespace gpv
