// gpv_csim.hip — conditional simulation of a cond.yz='z' model over a map (gpv_plan_cond_sim), gfx950, FP64.
//
// The prediction locations s_0 .. s_{nq-1} are ordered after all observations, in a sweep order; s_i conditions on N_i, its m
// nearest points among the observations and s_0 .. s_{i-1}: J_i (observations, conditioned on through z: the nugget on the
// diagonal) and P_i (earlier prediction locations, conditioned on through the latent y: no nugget).  With s_i as the LAST row,
//     S = C(N_i u s_i, N_i u s_i) + diag(tau_J, 0_P, 0),   u = S^-1 e_last:
//     c_ij = -u_j / u_last,   sd_i = 1 / sqrt(u_last),   y_i = sum_J c_ij z_j + sum_P c_ip y_p + sd_i eps_i,
// so (I - B) Y = A + D E with B the strictly lower-triangular matrix of the c_ip: one sparse unit-triangular operator serves the
// means (right-hand side A) and the deviation fields (right-hand side D E).
//
// Factor pass: the geometry and the elimination of gpv_krige.hip (one wavefront per location, lane i owns row i, one kernel per
// row-length bucket PB in {16, 32, 64}, the corrected multiplier), over a MIXED neighbour list: an id in [1, Nlocs] is an ORDERED
// observation, read as the krige pass reads it; an id in (Nlocs, Nlocs + i] is sweep row id - Nlocs - 1, its coordinates come
// from the call's resident locations and its nugget is 0.  Out: the coefficients on the slots that hold a prediction location
// (lane j writes its own slot), sd, and for every data column the sum over the observation slots by the same butterfly
// (wave_sum): a column's bits depend neither on the other columns nor on how the rows are chunked.  "A pivot <= 0 or NaN, or
// u_last <= 0" fails the location: NaN in sd, a and coef, one count.  A location that coincides with an earlier prediction
// location of its list has a row of the same bits, the corrected multiplier is exactly 1, and its pivot is exactly 0: it fails.
//
// Sweep: x_i = r_i + sum_slots coef[i][t] x[nbr_t], level by level (level(i) = 0 if P_i is empty, else 1 + max level(p); the
// schedule is built on the host).  The geometry and the synchronisation of gpv_unwhiten.hip: 16 lanes per row = (16 / CP slots)
// x (CP columns); a wide level is one launch, a maximal run of narrow levels is ONE launch of one 1024-thread workgroup with
// __syncthreads() between the levels; plain loads and stores through one non-restrict pointer; no flags, nothing spins, no
// workgroup waits for another.  NaN reaches the dependants of a failed location by arithmetic alone.
// Summation order: slot t of a row belongs to the partial sum t mod 16, each partial sum adds its slots in ascending order, and
// the 16 partial sums meet in one fixed tree (offsets 8, 4, 2, 1).  A lane holds 16 / NS of them in registers and joins those
// first, the lanes of the row then meet by xor shuffles: the tree is the same at every CP, so a column's bits depend on neither
// CP nor the other columns.
// Builtins only, no inline assembly.
#include "gpv_csim.h"
#include "gpv_internal.h"
#include "gpv_krige_dev.hpp"
#include "gpv_philox.hpp"

namespace gpv {

namespace {

template <int PB, int COV>
__global__ void __launch_bounds__(64 * kKrigeWavesPerBlock, (PB == 16 ? 3 : (PB == 32 ? 2 : 1))) gpv_csim_factor_kernel(const CsimFactorArgs F)
{
    const KrigeArgs &A = F.k;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool packed = A.dim <= 3;
    const int64_t nwaves = (int64_t)gridDim.x * kKrigeWavesPerBlock;
    unsigned nbad = 0;
    for (int64_t kk = (int64_t)blockIdx.x * kKrigeWavesPerBlock + wave; kk < A.nq; kk += nwaves) {
        const int64_t k = F.row0 + kk;                                // the sweep row
        // ---- gather: lane i takes slot m + 1 - PB + i of {neighbour 0 .. m - 1, the location}; the location sits in lane PB - 1
        const int slot = A.m + 1 - PB + lane;
        const bool isq = slot == A.m;
        const int64_t id = (slot >= 0 && slot < A.m) ? (int64_t)A.nnq[k * A.m + slot] - 1 : -1;
        const bool nb = id >= 0;
        const bool ob = nb && id < F.Nlocs;                           // an observation; nb && !ob: an earlier prediction location
        const bool valid = nb || isq;
        const int64_t v = ob ? (int64_t)A.newpos[id] : 0;
        const int64_t pr = isq ? k : (nb && !ob ? id - F.Nlocs : 0);  // the row of qall a lane that is no observation reads
        const double tau = ob ? (A.nuggets ? A.nuggets[id] : A.nug) : (valid ? 0.0 : 1.0);
        double a[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) a[j] = 0.0;
        for (int t = 0; t < A.dim; ++t) {
            const double x = ob ? A.rec[v * (packed ? 4 : A.locs_ld) + t] : (valid ? F.qall[pr * A.dim + t] : 0.0);
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
        // ---- Gauss-Jordan with the right-hand side e_last (gpv_krige.hip: the multiplier with one correction step is exactly 1
        // where the row's entry IS the pivot)
        double r1 = (lane == PB - 1) ? 1.0 : 0.0, dg = 1.0;
        bool fail = false;
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double d = readlane_d(a[j], j) + readlane_d(tau, j);
            fail |= !(d > 0.0);                                      // (uniform: every lane holds the same pivot)
            const bool pivot = lane == j;
            const double inv = 1.0 / d;
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
        const double nan = __builtin_nan("");
        // ---- the coefficients: lane j writes its own slot
        if (slot >= 0 && slot < A.m) F.coef[k * A.m + slot] = fail ? nan : ((nb && !ob) ? -u / ul : 0.0);
        // ---- the columns over the observation slots: one butterfly each, lane c keeps column c
        double mine = 0.0;
        if (A.Z == nullptr) {
            const double zi = ob ? (packed ? A.rec[v * 4 + 3] : A.z[v]) : 0.0;
            mine = -wave_sum(u * zi) / ul;
        } else {
            const double *zr = A.Z + v * A.zld;
#pragma unroll 1
            for (int c0 = 0; c0 < A.ncols; c0 += 4) {                 // (zld is a multiple of 4: zeros behind the last column)
                double s4[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) s4[c] = u * (ob ? zr[c0 + c] : 0.0);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double s = -wave_sum(s4[c]) / ul;
                    mine = (lane == c0 + c) ? s : mine;
                }
            }
        }
        if (lane < A.ncols) F.a[(int64_t)lane * F.nrows + k] = fail ? nan : mine;
        if (lane == PB - 1) F.sd[k] = fail ? nan : 1.0 / sqrt(ul);
    }
    if (lane == 0 && nbad) atomicAdd(A.nfail, nbad);                 // (an integer count: order-free)
}

template <int PB>
hipError_t launch_factor_bucket(const CsimFactorArgs &a, int grid, hipStream_t s)
{
    const dim3 g((unsigned)grid), b(64 * kKrigeWavesPerBlock);
    switch (a.k.cov) {
        case COV_MATERN05: hipLaunchKernelGGL((gpv_csim_factor_kernel<PB, COV_MATERN05>), g, b, 0, s, a); break;
        case COV_MATERN15: hipLaunchKernelGGL((gpv_csim_factor_kernel<PB, COV_MATERN15>), g, b, 0, s, a); break;
        case COV_MATERN25: hipLaunchKernelGGL((gpv_csim_factor_kernel<PB, COV_MATERN25>), g, b, 0, s, a); break;
        case COV_ESQE: hipLaunchKernelGGL((gpv_csim_factor_kernel<PB, COV_ESQE>), g, b, 0, s, a); break;
        case COV_MATERN_GEN: hipLaunchKernelGGL((gpv_csim_factor_kernel<PB, COV_MATERN_GEN>), g, b, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) gpv_csim_pack_kernel(const double *__restrict__ in, int64_t ld, const double *__restrict__ sd,
                                                            int64_t n, int ncols, int cp, double *__restrict__ X)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * cp) return;
    const int64_t i = t / cp;
    const int c = (int)(t - i * cp);
    const double v = c < ncols ? in[(int64_t)c * ld + i] : 0.0;
    X[t] = (sd != nullptr && c < ncols) ? sd[i] * v : v;
}

__global__ void __launch_bounds__(256) gpv_csim_unpack_kernel(const double *__restrict__ X, int64_t n, int ncols, int cp,
                                                              double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * ncols) return;
    const int64_t c = t / n, i = t - c * n;
    out[t] = X[i * cp + c];
}

// one thread per (sweep row, draw pair): a Box-Muller pair is two adjacent columns, one 16-byte store
__global__ void __launch_bounds__(256) gpv_csim_normals_kernel(double *X, const double *__restrict__ sd, int64_t n, uint64_t seed,
                                                               int64_t id0, int64_t draw0)
{
    constexpr int PAIRS = kCsimMaxCols / 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = t / PAIRS;
    const int p = (int)(t % PAIRS);
    if (i >= n) return;
    double2 v;
    draws_normal_pair(seed, (uint64_t)(id0 + i), (uint64_t)(draw0 / 2 + p), v.x, v.y);
    const double s = sd[i];
    v.x *= s;
    v.y *= s;
    *reinterpret_cast<double2 *>(X + i * kCsimMaxCols + 2 * p) = v;
}

// Sweep row i by the 16 lanes of one group (lig = lane in the group); every lane of the group takes the same path.  `on`: the
// group holds a row of its own (the others repeat the slice's last row and write nothing, so that all 64 lanes of a wavefront
// reach the cross-lane sums).
template <int CP>
__device__ __forceinline__ void csim_row(const CsimSweepArgs &A, const int32_t i, const bool on, const int lig)
{
    constexpr int NS = kCsimLanes / CP;                // neighbour slots of a row's 16 lanes
    const int c = lig & (CP - 1), sl = lig / CP;
    const int m = A.m;
    const int32_t *const nr = A.nn + (int64_t)i * m;
    const double *const cr = A.coef + (int64_t)i * m;
    double acc[CP];                                    // the partial sums sl + NS j, j = 0 .. CP - 1, of this lane's column
#pragma unroll
    for (int j = 0; j < CP; ++j) acc[j] = 0.0;
    for (int t0 = 0; t0 < m; t0 += kCsimLanes) {
#pragma unroll
        for (int j = 0; j < CP; ++j) {
            // every load is unconditional, from an address that is always valid (the row's last slot; the row's own entry of
            // X), and what does not count is replaced by zeros afterwards: no branch stands between the loads, so the slots of
            // a lane are in flight together.  fma(0, 0, acc) leaves acc as it is.
            const int t = t0 + sl + NS * j;
            const int tt = t < m ? t : m - 1;
            const int64_t p = (int64_t)nr[tt] - A.Nlocs - 1;                  // >= 0: a sweep row (an earlier level's)
            const bool use = t < m && p >= 0;
            const double cf = cr[tt];
            const double x = A.X[(use ? p : (int64_t)i) * CP + c];
            acc[j] = __builtin_fma(use ? cf : 0.0, use ? x : 0.0, acc[j]);
        }
    }
#pragma unroll
    for (int h = CP / 2; h > 0; h >>= 1)               // the tree's offsets 8 .. NS: in registers
#pragma unroll
        for (int j = 0; j < h; ++j) acc[j] += acc[j + h];
    double v = acc[0];
#pragma unroll
    for (int off = kCsimLanes / 2; off >= CP; off >>= 1) v += __shfl_xor(v, off, kCsimLanes);      // offsets NS / 2 .. 1: across the slots
    const double r = A.X[(int64_t)i * CP + c];
    if (on && sl == 0) A.X[(int64_t)i * CP + c] = r + v;
}

template <int CP>
__global__ void __launch_bounds__(kCsimWideThreads) gpv_csim_wide_kernel(const CsimSweepArgs A, const int64_t lo, const int64_t hi)
{
    const int grp = threadIdx.x >> 4, lig = threadIdx.x & 15;
    const int64_t i = lo + (int64_t)blockIdx.x * kCsimWideRows + grp;      // (the grid covers [lo, hi): blockIdx.x * 16 < hi - lo)
    const bool on = i < hi;
    csim_row<CP>(A, A.order[on ? i : hi - 1], on, lig);
}

template <int CP>
__global__ void __launch_bounds__(kCsimNarrowThreads) gpv_csim_narrow_kernel(const CsimSweepArgs A, const int lev0, const int lev1)
{
    const int grp = threadIdx.x >> 4, lig = threadIdx.x & 15;
    for (int lev = lev0; lev < lev1; ++lev) {          // every bound below is the same for the whole workgroup
        const int32_t lo = A.levptr[lev], hi = A.levptr[lev + 1];
        for (int32_t i0 = lo; i0 < hi; i0 += kCsimNarrowRows) {
            const bool on = i0 + grp < hi;
            csim_row<CP>(A, A.order[on ? i0 + grp : hi - 1], on, lig);
        }
        __syncthreads();                               // this level's stores to X are visible to the workgroup's next loads
    }
}

bool csim_cp_ok(int cp) { return cp >= 1 && cp <= kCsimMaxCols && (cp & (cp - 1)) == 0; }

}  // namespace

hipError_t launch_csim_factor(const CsimFactorArgs &a, int grid, hipStream_t s)
{
    const int p = a.k.m + 1;
    if (grid < 1 || a.k.nq < 0 || a.row0 < 0 || a.row0 + a.k.nq > a.nrows || a.k.m < 1 || p > kKrigeMaxP || a.k.ncols < 1 ||
        a.k.ncols > kKrigeMaxCols || a.k.dim < 1 || a.k.dim > 8)
        return hipErrorInvalidValue;
    if (a.k.Z != nullptr && (a.k.zld < a.k.ncols || a.k.zld % 4 != 0)) return hipErrorInvalidValue;
    if (a.k.Z == nullptr && a.k.ncols != 1) return hipErrorInvalidValue;
    if (!a.qall || !a.coef || !a.sd || !a.a || !a.k.nnq || !a.k.nfail) return hipErrorInvalidValue;
    if (a.k.nq == 0) return hipSuccess;
    return p <= 16 ? launch_factor_bucket<16>(a, grid, s) : (p <= 32 ? launch_factor_bucket<32>(a, grid, s) : launch_factor_bucket<64>(a, grid, s));
}

hipError_t launch_csim_pack(const double *in, int64_t ld, const double *sd, int64_t n, int ncols, int cp, double *X, hipStream_t s)
{
    if (n < 1 || ld < n || ncols < 1 || ncols > cp || !csim_cp_ok(cp)) return hipErrorInvalidValue;
    const int64_t blocks = (n * cp + 255) / 256;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_csim_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, ld, sd, n, ncols, cp, X);
    return hipGetLastError();
}

hipError_t launch_csim_unpack(const double *X, int64_t n, int ncols, int cp, double *out, hipStream_t s)
{
    if (n < 1 || ncols < 1 || ncols > cp || !csim_cp_ok(cp)) return hipErrorInvalidValue;
    const int64_t blocks = (n * ncols + 255) / 256;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_csim_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, X, n, ncols, cp, out);
    return hipGetLastError();
}

hipError_t launch_csim_normals(double *X, const double *sd, int64_t n, uint64_t seed, int64_t id0, int64_t draw0, hipStream_t s)
{
    const int64_t blocks = (n * (kCsimMaxCols / 2) + 255) / 256;
    if (n < 1 || id0 < 0 || draw0 < 0 || (draw0 % kCsimMaxCols) != 0 || blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_csim_normals_kernel, dim3((unsigned)blocks), dim3(256), 0, s, X, sd, n, seed, id0, draw0);
    return hipGetLastError();
}

hipError_t launch_csim_wide(const CsimSweepArgs &a, int cp, int64_t lo, int64_t hi, hipStream_t s)
{
    if (lo < 0 || hi <= lo || a.m < 1) return hipErrorInvalidValue;
    const int64_t blocks = (hi - lo + kCsimWideRows - 1) / kCsimWideRows;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    const dim3 g((unsigned)blocks), b(kCsimWideThreads);
    switch (cp) {
        case 1: hipLaunchKernelGGL(gpv_csim_wide_kernel<1>, g, b, 0, s, a, lo, hi); break;
        case 2: hipLaunchKernelGGL(gpv_csim_wide_kernel<2>, g, b, 0, s, a, lo, hi); break;
        case 4: hipLaunchKernelGGL(gpv_csim_wide_kernel<4>, g, b, 0, s, a, lo, hi); break;
        case 8: hipLaunchKernelGGL(gpv_csim_wide_kernel<8>, g, b, 0, s, a, lo, hi); break;
        case 16: hipLaunchKernelGGL(gpv_csim_wide_kernel<16>, g, b, 0, s, a, lo, hi); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_csim_narrow(const CsimSweepArgs &a, int cp, int lev0, int lev1, hipStream_t s)
{
    if (lev0 < 0 || lev1 <= lev0 || a.m < 1 || !a.levptr) return hipErrorInvalidValue;
    const dim3 g(1), b(kCsimNarrowThreads);
    switch (cp) {
        case 1: hipLaunchKernelGGL(gpv_csim_narrow_kernel<1>, g, b, 0, s, a, lev0, lev1); break;
        case 2: hipLaunchKernelGGL(gpv_csim_narrow_kernel<2>, g, b, 0, s, a, lev0, lev1); break;
        case 4: hipLaunchKernelGGL(gpv_csim_narrow_kernel<4>, g, b, 0, s, a, lev0, lev1); break;
        case 8: hipLaunchKernelGGL(gpv_csim_narrow_kernel<8>, g, b, 0, s, a, lev0, lev1); break;
        case 16: hipLaunchKernelGGL(gpv_csim_narrow_kernel<16>, g, b, 0, s, a, lev0, lev1); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gpv
