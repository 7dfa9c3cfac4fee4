// gpv_krige_groups.hip — the joint predict pass of gpv_plan_krige_groups: grouped local kriging of a cond.yz='z' model, gfx950, FP64.
//
// A group G of g prediction locations ordered last, member i conditioning on one shared set J of observations and on the
// members before it, is a valid Vecchia model whose predictive distribution of G is that of the (|J| + g)-row block
//     S = C(J u G, J u G) + diag(tau_J, 0_G),   J in front, G last.
// Eliminating the J pivots (rows below each pivot only, no back-substitution) leaves
//     Sigma_G = K_GG - K_GJ (K_JJ + tau_J)^-1 K_JG      in the trailing g x g block, and
//     -mean_{i,c}                                        on row i of the right-hand side [z_{J,c}; 0_G] of data column c.
// With weights w: group mean_c = sum_i w_i mean_{i,c}, group var = w' Sigma_G w.  All of the latent field y.
//
// Geometry: that of gpv_krige.hip.  One wavefront per group, grid-stride over the groups of one row bucket PB in {16, 32, 64}
// (the launch's list: a group's bucket is a function of its m + g alone, so its bits depend on nothing else in the call); lane i
// owns row i of S in registers; the members sit in the last g lanes of the bucket, the m neighbour slots in front of them, the
// bucket's padding in front of those.  Rows that are no neighbour and no member (padding, the 0-padding of a short neighbour
// list, lanes beyond PB) are identity rows and contribute exact zeros.  The pivot row is handed out by
// __builtin_amdgcn_readlane.  The multipliers stay in the eliminated columns (a[j] = f, the Fisher body of
// gpv_grad_set_pass.inc) and are replayed on the data columns four at a time afterwards: no column rides through the
// elimination.  A group fails when a J pivot is not > 0 (or NaN) or a diagonal entry of Sigma_G is not > 0: everything of it is
// NaN and it is counted.  Builtins only, no inline assembly.
//
// Reductions: a row of Sigma_G times w is one sequential loop over the columns; the sums over the members are the butterfly
// wave_sum.  One order each, whatever else the call holds.  Every value is written by one lane.
#include "gpv_krige_groups.h"
#include "gpv_krige_dev.hpp"

namespace gpv {

namespace {

template <int PB, int COV>
__global__ void __launch_bounds__(64 * kKrigeWavesPerBlock, (PB == 16 ? 3 : (PB == 32 ? 2 : 1))) gpv_krige_groups_kernel(const KrigeGroupArgs G)
{
    const KrigeArgs &A = G.k;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool packed = A.dim <= 3;
    const int64_t nwaves = (int64_t)gridDim.x * kKrigeWavesPerBlock;
    const double nan = __builtin_nan("");
    unsigned nbad = 0;
    for (int64_t it = (int64_t)blockIdx.x * kKrigeWavesPerBlock + wave; it < G.nlist; it += nwaves) {
        // ---- the group (the same in every lane: scalar registers)
        const int k = __builtin_amdgcn_readfirstlane(G.list[it]);
        const int q0 = __builtin_amdgcn_readfirstlane(G.gptr[k]);
        const int g = __builtin_amdgcn_readfirstlane(G.gptr[k + 1]) - q0;
        const int nJ = PB - g;                                       // pivots to eliminate: the padding and the neighbour slots
        // ---- gather: lane i takes slot m + g - PB + i of {neighbour 0 .. m - 1, member 0 .. g - 1}
        const int slot = A.m - nJ + lane;
        const int mi = lane - nJ;                                    // the member, where 0 <= mi < g
        const bool isq = mi >= 0 && lane < PB;
        const int id = (slot >= 0 && slot < A.m) ? A.nnq[(int64_t)k * A.m + slot] - 1 : -1;
        const bool nb = id >= 0;
        const bool valid = nb || isq;
        const int64_t v = nb ? (int64_t)A.newpos[id] : 0;
        const int64_t qi = isq ? (int64_t)q0 + mi : 0;
        const double tau = nb ? (A.nuggets ? A.nuggets[id] : A.nug) : (isq ? 0.0 : 1.0);
        const double w = isq ? G.w[qi] : 0.0;
        double a[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) a[j] = 0.0;
        for (int t = 0; t < A.dim; ++t) {
            const double x = nb ? A.rec[v * (packed ? 4 : A.locs_ld) + t] : (isq ? A.q[qi * A.dim + t] : 0.0);
            double sc = A.inv[0];                                     // (selects at constant indices: no scratch)
#pragma unroll
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
        // ---- Gauss elimination of the J pivots, the rows below each; the multiplier stays in the eliminated column
        bool fail = false;
#pragma unroll
        for (int j = 0; j < PB - 1; ++j) {
            if (j < nJ) {                                            // (uniform: g >= 1, so the last column is never a pivot)
                const double d = readlane_d(a[j], j) + readlane_d(tau, j);
                fail |= !(d > 0.0);                                  // (uniform: every lane holds the same pivot)
                const double inv = 1.0 / d;
                // the multiplier with one correction step: exactly 1 where the row's entry IS the pivot (a member on an
                // observation: their rows are the same bits), so with no nugget there the member's row cancels to exact zeros
                // and its variance fails the test instead of passing it as a rounding residue of either sign
                const double f0 = a[j] * inv;
                const double f = lane > j ? __builtin_fma(__builtin_fma(-f0, d, a[j]), inv, f0) : 0.0;
#pragma unroll
                for (int c = j + 1; c < PB; ++c) a[c] = __builtin_fma(-f, readlane_d(a[c], j), a[c]);
                a[j] = f;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- Sigma_G: the diagonal, the failure test, the row times w
        double dg = 0.0, t = 0.0;
#pragma unroll
        for (int c = 0; c < PB; ++c) {
            dg = (lane == c) ? a[c] : dg;
            t = __builtin_fma(c >= nJ ? a[c] : 0.0, readlane_d(w, c), t);
        }
        fail |= __ballot(isq && !(dg > 0.0)) != 0ull;
        nbad += fail ? 1u : 0u;
        const double gv = wave_sum(isq ? w * t : 0.0);
        if (isq) A.var[qi] = fail ? nan : dg;
        if (lane == 0) G.gvar[k] = fail ? nan : gv;
        if (G.cov != nullptr) {                                      // the lower triangle, row-major: member mi writes its row
            double *cv = G.cov + G.coff[k] + ((int64_t)mi * (mi + 1)) / 2 - nJ;
#pragma unroll
            for (int c = 0; c < PB; ++c)
                if (isq && c >= nJ && c <= lane) cv[c] = fail ? nan : a[c];
        }
        // ---- the columns: the multipliers replayed on four right-hand sides at a time
        const double *zr = A.Z ? A.Z + v * A.zld : nullptr;
#pragma unroll 1
        for (int c0 = 0; c0 < A.ncols; c0 += 4) {                     // (zld is a multiple of 4: zeros behind the last column)
            double r4[4];
            if (A.Z == nullptr) {
                r4[0] = nb ? (packed ? A.rec[v * 4 + 3] : A.z[v]) : 0.0;
                r4[1] = r4[2] = r4[3] = 0.0;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) r4[c] = nb ? zr[c0 + c] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < PB - 1; ++j) {
                if (j < nJ) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) r4[c] = __builtin_fma(-a[j], readlane_d(r4[c], j), r4[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c0 + c < A.ncols) {                              // (uniform)
                    const double mu = -r4[c];
                    const double gm = wave_sum(isq ? w * mu : 0.0);
                    if (isq) A.mean[(int64_t)(c0 + c) * A.nq + qi] = fail ? nan : mu;
                    if (lane == 0) G.gmean[(int64_t)(c0 + c) * G.ng + k] = fail ? nan : gm;
                }
            }
        }
    }
    if (lane == 0 && nbad) atomicAdd(A.nfail, nbad);                 // (an integer count: order-free)
}

template <int PB>
hipError_t launch_bucket(const KrigeGroupArgs &a, int grid, hipStream_t s)
{
    const dim3 g((unsigned)grid), b(64 * kKrigeWavesPerBlock);
    switch (a.k.cov) {
        case COV_MATERN05: hipLaunchKernelGGL((gpv_krige_groups_kernel<PB, COV_MATERN05>), g, b, 0, s, a); break;
        case COV_MATERN15: hipLaunchKernelGGL((gpv_krige_groups_kernel<PB, COV_MATERN15>), g, b, 0, s, a); break;
        case COV_MATERN25: hipLaunchKernelGGL((gpv_krige_groups_kernel<PB, COV_MATERN25>), g, b, 0, s, a); break;
        case COV_ESQE: hipLaunchKernelGGL((gpv_krige_groups_kernel<PB, COV_ESQE>), g, b, 0, s, a); break;
        case COV_MATERN_GEN: hipLaunchKernelGGL((gpv_krige_groups_kernel<PB, COV_MATERN_GEN>), g, b, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_krige_groups(const KrigeGroupArgs &a, int bucket, int grid, hipStream_t s)
{
    const KrigeArgs &k = a.k;
    if (grid < 1 || a.nlist < 0 || a.ng < a.nlist || k.nq < a.nlist || k.m < 1 || k.m + 1 > kKrigeGroupMaxRows || k.ncols < 1 ||
        k.ncols > kKrigeMaxCols || k.dim < 1 || k.dim > 8 || bucket < 0 || bucket >= kKrigeGroupBuckets)
        return hipErrorInvalidValue;
    if (k.m + 1 > (16 << bucket)) return hipErrorInvalidValue;      // a bucket too small for the neighbours and one member
    if (k.Z != nullptr && (k.zld < k.ncols || k.zld % 4 != 0)) return hipErrorInvalidValue;
    if (k.Z == nullptr && k.ncols != 1) return hipErrorInvalidValue;
    if (a.nlist == 0) return hipSuccess;
    return bucket == 0 ? launch_bucket<16>(a, grid, s) : (bucket == 1 ? launch_bucket<32>(a, grid, s) : launch_bucket<64>(a, grid, s));
}

}  // namespace gpv
