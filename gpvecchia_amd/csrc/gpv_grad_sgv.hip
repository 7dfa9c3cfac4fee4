// gpv_grad_sgv.hip — the per-set pass of the analytic gradient of the cond.yz='SGV' log-likelihood (gpv_plan_loglik_grad_sgv),
// gfx950, FP64.  It runs behind an evaluation with the posterior mean and the selected inverse of the posterior factor
// (gpv_selinv.hip) and reads what they leave: mu~ = W^-1 z2 and Sigma = W^-1 on the pattern of the factor.  DESIGN.md §4p.
//
// Set k has the valid entries J, its own point last (l), flags c_j (1: conditioned on as latent y, c_l = 1):
//     S = C(J, J) + tau diag(1 - c),   u = S^-1 e_l,   M = u / sqrt(u_l)            (the row of Lentries; M_l = d_k)
//     a_k = sum_{c_j = 0} M_j z_j,   s_k = sum_{c_j = 1} M_j mu~_j,   delta_k = a_k - s_k
//     v = Sigma_LL m_k      over the latent members L of the set: the entries of posterior column k, all inside the pattern
// -2 l is linear in dM once delta, v and mu~ are known, so with
//     f_j = 2 delta_k z_j (observed j),  2 (v_j - delta_k mu~_j) (latent j),  and -2 / M_l more at the own point
// one further solve w~ = S^-1 f replaces one solve per parameter (the adjoint of dM_p = -y_p / sqrt(u_l) + 1/2 u (y_p)_l /
// u_l^{3/2}, y_p = S^-1 D_p u): with D_p = dS/dtheta_p elementwise (the nugget: diag(1 - c)) and t_p = D_p u,
//     c_{k,p} = -(w~'t_p) / sqrt(u_l) + 1/2 (f'u)(u't_p) / u_l^{3/2},   d l / d theta_p = -1/2 sum_k c_{k,p}
// and column k of the nugget gets 1/tau - (Sigma_kk + (z_k + mu~_k)^2) / tau^2 in addition.
//
// Geometry as in gpv_grad.hip: one wavefront per conditioning set, grid-stride, lane i owns row i of the block, one object per
// row-length bucket PB in {16, 32, 64}, short rows padded IN FRONT with rows of tau I.  The sweep keeps its multipliers (the
// information mode of gpv_grad_set_pass.inc), w~ replays them.  The tile of Sigma is gathered as the level kernel of
// gpv_selinv.hip gathers it for column k (rows PB + 1 doubles apart in LDS), with the column's own entries as its last row and
// column; it is indexed by the POSITION of an entry in the posterior column (SgvGradArgs::cpos), which is where the lanes
// deposit m_k and fetch v.  Every sum has one fixed order, nothing is atomic.  Builtins and plain C++ only.
#include "gpv_grad_sgv.h"
#include "gpv_internal.h"

namespace gpv {

#ifdef GPV_SGV_PB

namespace {

__device__ __forceinline__ double readlane_d(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);    // the same tree in every lane: all lanes end equal
    return v;
}

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The families of this pass (matern at nu = 0.5, 1.5, 2.5 and esqe): value and derivative kernels of a pair from its squared
// distance, the formulas of grad_cov / grad_dcov (gpv_grad.hip), which stay private to that unit so that its code objects do
// not move.
template <int COV> constexpr int sgv_npar() { return COV == COV_ESQE ? 4 : 2; }

template <int COV>
__device__ __forceinline__ double sgv_cov(double r2, const GradArgs &A)
{
    const double r = sqrt(r2);
    if constexpr (COV == COV_MATERN05) {
        return A.sA * exp(-(r * A.cA));
    } else if constexpr (COV == COV_MATERN15) {
        const double t = r * A.cA, e = exp(-t);
        return A.sA * __builtin_fma(t, e, e);
    } else if constexpr (COV == COV_MATERN25) {
        const double t = r * A.cA;
        return A.sA * exp(-t) * __builtin_fma(t, __builtin_fma(t, 1.0 / 3.0, 1.0), 1.0);
    } else {
        return __builtin_fma(A.sA, exp(-(r * A.cA)), A.sB * exp(-(r2 * A.cB)));
    }
}

template <int COV>
__device__ __forceinline__ void sgv_dcov(double r2, const GradArgs &A, double (&d)[sgv_npar<COV>()])
{
    const double r = sqrt(r2);
    if constexpr (COV == COV_MATERN05) {
        const double t = r * A.cA, e = exp(-t);
        d[0] = e;
        d[1] = A.sA * e * t * A.irA;
    } else if constexpr (COV == COV_MATERN15) {
        const double t = r * A.cA, e = exp(-t);
        d[0] = __builtin_fma(t, e, e);
        d[1] = A.sA * (t * t) * e * A.irA;
    } else if constexpr (COV == COV_MATERN25) {
        const double t = r * A.cA, e = exp(-t), t3 = t * t * (1.0 / 3.0);
        d[0] = e * __builtin_fma(t, __builtin_fma(t, 1.0 / 3.0, 1.0), 1.0);
        d[1] = A.sA * e * t3 * (1.0 + t) * A.irA;
    } else {
        const double t = r * A.cA, e1 = exp(-t), s = r2 * A.cB, e2 = exp(-s);
        d[0] = e1;
        d[1] = A.sA * e1 * t * A.irA;
        d[2] = e2;
        d[3] = A.sB * e2 * (2.0 * s) * A.irB;
    }
}

// wavefronts per workgroup: the tile of the bucket of 64 is 33 KB, one wavefront per workgroup keeps four workgroups on a CU
template <int PB> constexpr int sgv_waves() { return PB == 64 ? 1 : kGradWavesPerBlock; }
// doubles of one wavefront's LDS: the tile, then m_k and v by position in the posterior column
template <int PB> constexpr int sgv_lds() { return PB * (PB + 1) + 2 * PB; }

template <int PB, int COV>
__global__ void __launch_bounds__(64 * sgv_waves<PB>()) gpv_grad_sgv_kernel(const SgvGradArgs B)
{
    constexpr int WPB = sgv_waves<PB>(), NPAR = sgv_npar<COV>(), NP1 = NPAR + 1, TL = PB + 1;
    const GradArgs &A = B.g;
    __shared__ double s_part[WPB][kSgvNV];
    __shared__ double s_tile[WPB][sgv_lds<PB>()];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool packed = A.dim <= 3;
    const int64_t nwaves = (int64_t)gridDim.x * WPB;
    double *const tile = s_tile[wave], *const ml = tile + PB * TL, *const vl = ml + PB;
    double acc[kSgvNV];
#pragma unroll
    for (int t = 0; t < kSgvNV; ++t) acc[t] = 0.0;

    for (int64_t k = (int64_t)blockIdx.x * WPB + wave; k < A.rows; k += nwaves) {
        // ---- gather: lane i of the bucket takes entry P - PB + i of the stored row (the valid entries are its LAST n0)
        const int e = A.P - PB + lane;
        const int v = (lane < PB && e >= 0) ? A.nn[k * A.P + e] : -1;
        const bool valid = v >= 0;
        const int cp = valid ? (int)B.cpos[k * A.P + e] : 0xFF;
        const bool lat = cp != 0xFF;                                  // conditioned on as latent y: an entry of posterior column k
        const int4 sr = B.setrec[k];
        const int cb = sr.x, first = sr.y, cnt = sr.z, m = sr.z - 1;
        const unsigned long long vmask = __ballot(valid);
        const bool own_ok = (vmask >> (PB - 1)) & 1ull;
        const double zi = valid ? (packed ? A.rec[(int64_t)v * 4 + 3] : (A.z ? A.z[v] : 0.0)) : 0.0;
        const double mui = lat ? B.mu[B.crow[(size_t)first + cp]] : 0.0;
        const double skk = B.vars[sr.w];
        double xc[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) xc[t] = (packed && valid && t < A.dim) ? A.rec[(int64_t)v * 4 + t] : 0.0;
        // ---- squared distances, then C on the valid rows and columns, zero elsewhere
        double a[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) a[j] = 0.0;
        for (int t = 0; t < A.dim; ++t) {
            const double x = valid ? (packed ? A.rec[(int64_t)v * 4 + t] : A.locs[(int64_t)v * A.locs_ld + t]) : 0.0;
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                const double df = x - readlane_d(x, j);
                a[j] = __builtin_fma(df, df, a[j]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const int vhi = __double2hiint(valid ? 1.0 : 0.0);
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double vj = __hiloint2double(__builtin_amdgcn_readlane(vhi, j), 0);
            a[j] = sgv_cov<COV>(a[j], A) * (valid ? vj : 0.0);
            __builtin_amdgcn_sched_barrier(0);                        // one exp at a time
        }
        // ---- Gauss-Jordan with the right-hand side e_last; tau joins the diagonal where c_j = 0 (a padded row is tau times an
        // identity row); a[j] <- the multiplier of step j, for the replay
        const double nugl = lat ? 0.0 : A.nug;
        double r1 = (lane == PB - 1) ? 1.0 : 0.0, dg = 1.0;           // dg: 1 / pivot of the lane's own row
        bool fail = !own_ok;
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double d = readlane_d(a[j], j) + readlane_d(nugl, j);
            fail |= !(d > 0.0);                                      // (uniform: every lane holds the same pivot)
            const bool pivot = lane == j;
            const double inv = 1.0 / d;
            const double f = pivot ? 0.0 : a[j] * inv;
            dg = pivot ? inv : dg;
#pragma unroll
            for (int c = j + 1; c < PB; ++c) a[c] = __builtin_fma(-f, readlane_d(a[c], j), a[c]);
            r1 = __builtin_fma(-f, readlane_d(r1, j), r1);
            a[j] = f;
            __builtin_amdgcn_sched_barrier(0);
        }
        const double u = r1 * dg;                                     // exact zeros on the padded rows
        const double ul = readlane_d(u, PB - 1), sq = sqrt(ul);
        const double M = u / sq;
        // ---- the tile of Sigma over the entries of posterior column k: the pairs inside N(k) from their columns' blocks through
        // the match records (gpv_selinv.hip, selinv_column), the pairs with k itself from the column's own block, Sigma_kk
        if (lat) ml[cp] = M;
        int2 pr = make_int2(0, 0);
        if (lane < m) pr = B.pair[(size_t)first + lane];
        for (int f0 = 0; f0 < m; f0 += 4) {
            int pos[4], cbf[4];
            double sv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = f0 + q, ff = f < m ? f : m - 1;
                cbf[q] = __builtin_amdgcn_ds_bpermute(ff << 2, pr.x);
                const int tq = __builtin_amdgcn_ds_bpermute(ff << 2, pr.y);
                pos[q] = (f < m && lane <= f) ? (int)B.tp[(size_t)tq + lane] : 0xFF;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) sv[q] = pos[q] != 0xFF ? B.S[(size_t)cbf[q] + 1 + pos[q]] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = f0 + q;
                if (f < m && lane <= f) {
                    tile[f * TL + lane] = sv[q];
                    tile[lane * TL + f] = sv[q];
                }
            }
        }
        if (lane < m) {
            const double so = B.S[(size_t)cb + 1 + lane];
            tile[m * TL + lane] = so;
            tile[lane * TL + m] = so;
        }
        if (lane == m) tile[m * TL + m] = skk;
        wave_lds_sync();
        double vs = 0.0;
        if (lane < cnt)
            for (int f = 0; f < cnt; ++f) vs = __builtin_fma(tile[f * TL + lane], ml[f], vs);
        if (lane < cnt) vl[lane] = vs;
        wave_lds_sync();
        const double vi = lat ? vl[cp] : 0.0;
        // ---- f and w~ = S^-1 f by one replay of the kept multipliers
        const double ak = wave_sum((valid && !lat) ? M * zi : 0.0);
        const double sk = wave_sum(lat ? M * mui : 0.0);
        const double dl = ak - sk;
        double fv = !valid ? 0.0 : (lat ? 2.0 * (vi - dl * mui) : 2.0 * dl * zi);
        if (lane == PB - 1) fv -= 2.0 / sq;
        double y = fv;
#pragma unroll
        for (int j = 0; j < PB; ++j) y = __builtin_fma(-a[j], readlane_d(y, j), y);
        const double wt = y * dg;
        // ---- pair pass: tt_p = sum_j D_p(lane, j) u_j, zero on the padded rows; the distances again from the coordinates, summed
        // over the coordinates in the order of the first pass
        double tt[NPAR];
#pragma unroll
        for (int p = 0; p < NPAR; ++p) tt[p] = 0.0;
        const int j0 = vmask ? __ffsll((long long)vmask) - 1 : 0;    // the columns in front of the first valid one hold u_j = 0
#pragma unroll 1
        for (int j = j0; j < PB; ++j) {
            double q2 = 0.0;
            if (packed) {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const double df = xc[t] - readlane_d(xc[t], j);
                    q2 = __builtin_fma(df, df, q2);
                }
            } else {
                for (int t = 0; t < A.dim; ++t) {
                    const double x = valid ? A.locs[(int64_t)v * A.locs_ld + t] : 0.0;
                    const double df = x - readlane_d(x, j);
                    q2 = __builtin_fma(df, df, q2);
                }
            }
            double d[NPAR];
            sgv_dcov<COV>(q2, A, d);
            const double uj = readlane_d(u, j);
#pragma unroll
            for (int p = 0; p < NPAR; ++p) tt[p] = __builtin_fma(d[p], uj, tt[p]);
        }
        // ---- epilogue: -1/2 c_{k,p}; the nugget's block is (1 - c) o u, and its column gets the explicit terms
        const double fu = wave_sum(fv * u);
        double val[kSgvRowLd];
#pragma unroll
        for (int p = 0; p < NP1; ++p) {
            const double tp = p < NPAR ? (valid ? tt[p] : 0.0) : ((valid && !lat) ? u : 0.0);
            const double ap = wave_sum(u * tp), bp = wave_sum(wt * tp);
            double c = -bp / sq + 0.5 * fu * ap / (ul * sq);
            if (p == NPAR) {
                const double zk = readlane_d(zi, PB - 1) + readlane_d(mui, PB - 1);
                c += 1.0 / A.nug - (skk + zk * zk) / (A.nug * A.nug);
            }
            val[p] = -0.5 * c;
        }
#pragma unroll
        for (int p = NP1; p < kSgvRowLd; ++p) val[p] = 0.0;
        acc[7] += 1.0;
        if (fail) {
            acc[6] += 1.0;
        } else {
#pragma unroll
            for (int p = 0; p < kSgvRowLd; ++p) acc[p] += val[p];
        }
        if (A.row_terms != nullptr && lane < kSgvRowLd) {
            double mine = 0.0;
#pragma unroll
            for (int p = 0; p < kSgvRowLd; ++p) mine = (lane == p) ? val[p] : mine;
            A.row_terms[(int64_t)A.rowid[k] * kSgvRowLd + lane] = fail ? __builtin_nan("") : mine;
        }
        wave_lds_sync();                                              // (the tile is reused by the wavefront's next set)
    }
    // ---- per-workgroup partials, waves added in wave order
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < kSgvNV; ++t) s_part[wave][t] = acc[t];
    }
    __syncthreads();
    if (threadIdx.x < kSgvNV) {
        double s = 0.0;
        for (int wv = 0; wv < WPB; ++wv) s += s_part[wv][threadIdx.x];
        A.block_part[(int64_t)blockIdx.x * kSgvNV + threadIdx.x] = s;
    }
}

}  // namespace

#define GPV_SGV_NAME2(pb) launch_grad_sgv_pb##pb
#define GPV_SGV_NAME(pb) GPV_SGV_NAME2(pb)
hipError_t GPV_SGV_NAME(GPV_SGV_PB)(const SgvGradArgs &a, int grid, hipStream_t stream)
{
    constexpr int PB = GPV_SGV_PB;
    const dim3 g((unsigned)grid), b(64 * sgv_waves<PB>());
    switch (a.g.cov) {
        case COV_MATERN05: hipLaunchKernelGGL((gpv_grad_sgv_kernel<PB, COV_MATERN05>), g, b, 0, stream, a); break;
        case COV_MATERN15: hipLaunchKernelGGL((gpv_grad_sgv_kernel<PB, COV_MATERN15>), g, b, 0, stream, a); break;
        case COV_MATERN25: hipLaunchKernelGGL((gpv_grad_sgv_kernel<PB, COV_MATERN25>), g, b, 0, stream, a); break;
        case COV_ESQE: hipLaunchKernelGGL((gpv_grad_sgv_kernel<PB, COV_ESQE>), g, b, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

#else  // the launcher that picks the bucket, and the second launch

hipError_t launch_grad_sgv_pb16(const SgvGradArgs &a, int grid, hipStream_t stream);
hipError_t launch_grad_sgv_pb32(const SgvGradArgs &a, int grid, hipStream_t stream);
hipError_t launch_grad_sgv_pb64(const SgvGradArgs &a, int grid, hipStream_t stream);

namespace {
// totals[t] = sum over the workgroups, in workgroup order: the same bits for the same launch geometry
__global__ void __launch_bounds__(64) gpv_grad_sgv_total_kernel(const double *part, int grid, double *totals)
{
    if (threadIdx.x < kSgvNV) {
        double s = 0.0;
        for (int b = 0; b < grid; ++b) s += part[(int64_t)b * kSgvNV + threadIdx.x];
        totals[threadIdx.x] = s;
    }
}
}  // namespace

int grad_sgv_grid(int p, int64_t rows, int cus)
{
    const int wpb = grad_bucket(p) == 64 ? 1 : kGradWavesPerBlock;
    int64_t grid = (rows + wpb - 1) / wpb;
    const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * kGradBlocksPerCU * (kGradWavesPerBlock / wpb);
    if (grid > cap) grid = cap;
    return (int)(grid < 1 ? 1 : grid);
}

hipError_t launch_grad_sgv(int p, const SgvGradArgs &a, int grid, hipStream_t stream)
{
    const int bucket = grad_bucket(p);
    if (grid < 1 || a.g.rows < 0 || bucket == 0) return hipErrorInvalidValue;
    if (!a.cpos || !a.setrec || !a.crow || !a.pair || !a.tp || !a.S || !a.vars || !a.mu) return hipErrorInvalidValue;
    const hipError_t e = bucket == 16 ? launch_grad_sgv_pb16(a, grid, stream)
                                      : (bucket == 32 ? launch_grad_sgv_pb32(a, grid, stream) : launch_grad_sgv_pb64(a, grid, stream));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gpv_grad_sgv_total_kernel, dim3(1), dim3(64), 0, stream, a.g.block_part, grid, a.g.totals);
    return hipGetLastError();
}

#endif

}  // namespace gpv
