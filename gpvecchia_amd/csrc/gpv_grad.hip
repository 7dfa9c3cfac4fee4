// gpv_grad.hip — value and analytic gradient of the cond.yz='z' Vecchia log-likelihood (gpv_plan_loglik_grad), gfx950, FP64.
//
// The likelihood is a sum of independent conditional densities, one per conditioning set.  With S' = C(J, J) + tau I over the
// valid entries J of a row (the set's own point last), u = S'^-1 e_last, w = S'^-1 z_J, q = u'z_J:
//     l_k        = 1/2 log u_last - 1/2 q^2 / u_last - 1/2 log 2 pi
//     dl_k/dtheta = -1/2 a / u_last + q b / u_last - 1/2 q^2 a / u_last^2,   a = u'D u, b = w'D u, D = dS'/dtheta elementwise
// (d u_last = -a and d q = -b).  D is never stored: once u and w are known a second pass over the pairs evaluates the derivative
// kernels from the coordinates again and accumulates the bilinear forms of all parameters together.
//
// Geometry: one wavefront per conditioning set, grid-stride over the sets; lane i owns row i of the block in registers, the
// kernel is compiled per row-length bucket PB in {16, 32, 64} (one object each) and rows shorter than PB are padded IN FRONT
// with rows of tau I, which contribute exact zeros.  Entries of the pivot row reach the other lanes through
// __builtin_amdgcn_readlane at compile-time lane numbers, i.e. as SGPR operands of the v_fma_f64 that uses them.
//
// Solve: Gauss-Jordan elimination without pivoting on the full symmetric rows, the two right-hand sides (e_last, z_J) carried
// along.  Its pivots are those of the Cholesky factorisation (the Schur complements' diagonals), so "pivot <= 0 or NaN" is the
// set kernel's failure test; per lane it costs the PB^2/2 fused multiply-adds of a lane-per-row Cholesky and needs neither of
// the two triangular solves, whose column access across lanes a register-resident factor cannot give.  For positive definite
// blocks it is forward stable; the accuracy tests hold it to 1e-8 per row against a long-double Cholesky.
//
// The second pass RE-EVALUATES exp from the recomputed distances instead of keeping r and e^{-cr} of the first pass: keeping
// them costs 2 PB more live doubles per lane through the elimination (256 VGPRs at PB = 64).
//
// Builtins only, no inline assembly: the compiler owns every read-lane wait state.
#include "gpv_grad.h"
#include "gpv_internal.h"

namespace gpv {

#ifdef GPV_GRAD_PB

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

template <int COV>
struct CovTraits {
    static constexpr int NPAR = (COV == COV_ESQE) ? 4 : (COV == COV_MATERN_GEN ? 3 : 2);   // covariance parameters differentiated
};

// ---- general smoothness (COV_MATERN_GEN): variance, range AND smoothness are differentiated ---------------------------------
// The three functions of a pair, free of sigma^2 and rho (gpv_bessel.hpp: C / sigma^2, c_nu s^{nu+1} K_{nu-1}, d(C / sigma^2)/dnu),
// come from the launch's tables, read from global memory (a few KB for the few octaves a plan's distances span: cache resident),
// times one exp(-s); a pair outside the tables takes the quadrature in ONE out-of-line copy (rare, divergent, large).  s = 0
// (coincident points, and the pairs of padded entries, which gen_r2 sends there) is {1, 0, 0} without either.
struct Gen3 { double f[3]; };
static __device__ __attribute__((noinline)) Gen3 gen_direct(const double s, const MaternDerivConst kc)
{
    Gen3 o;
    matern_general_derivs(s, kc, 0, o.f);
    return o;
}
template <int NF>
__device__ __forceinline__ void gen_eval(const double r2, const GradArgs &A, double (&f)[NF])
{
    const double s = sqrt(r2) * A.cA;
    const int seg = matern_dtab_segment(s, A.gmt_base);
    if ((unsigned)seg < (unsigned)A.gmt_nseg) {
        const double *row = A.gmt + (size_t)seg * MaternDTab::ROW;
        const double u = matern_dtab_u(s), e = exp(-s);
#pragma unroll
        for (int q = 0; q < NF; ++q) f[q] = e * matern_dtab_poly(row + q * MaternDTab::N, u);
    } else if (s == 0.0) {
        f[0] = 1.0;
#pragma unroll
        for (int q = 1; q < NF; ++q) f[q] = 0.0;
    } else {
        const Gen3 o = gen_direct(s, A.gen);
#pragma unroll
        for (int q = 0; q < NF; ++q) f[q] = o.f[q];
    }
}
// the squared distance a pair is evaluated at: a pair with a padded entry contributes nothing whatever its value, and at 0 it
// costs nothing (the other families pay one exp for it)
template <int COV>
__device__ __forceinline__ double gen_r2(const double r2, const bool live)
{
    if constexpr (COV == COV_MATERN_GEN) return live ? r2 : 0.0;
    else return r2;
}

// covariance of a pair from its squared distance: the formulas of cov_from_r2 (gpv_sets_kernel.hpp); r2 == 0 gives the
// variance exactly (t = 0, exp(0) = 1)
template <int COV>
__device__ __forceinline__ double grad_cov(double r2, const GradArgs &A)
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
    } else if constexpr (COV == COV_MATERN_GEN) {
        double f[1];
        gen_eval<1>(r2, A, f);
        return A.sA * f[0];
    } else {
        return __builtin_fma(A.sA, exp(-(r * A.cA)), A.sB * exp(-(r2 * A.cB)));
    }
}

// derivative kernels of a pair (variance, range [, variance 2, range 2]); at r2 == 0: 1 and exactly 0
template <int COV>
__device__ __forceinline__ void grad_dcov(double r2, const GradArgs &A, double (&d)[CovTraits<COV>::NPAR])
{
    const double r = sqrt(r2);
    if constexpr (COV == COV_MATERN05) {
        const double t = r * A.cA, e = exp(-t);
        d[0] = e;
        d[1] = A.sA * e * t * A.irA;                                   // sigma^2 e^{-r/rho} r / rho^2
    } else if constexpr (COV == COV_MATERN15) {
        const double t = r * A.cA, e = exp(-t);
        d[0] = __builtin_fma(t, e, e);
        d[1] = A.sA * (t * t) * e * A.irA;                             // sigma^2 c^2 r^2 e^{-cr} / rho
    } else if constexpr (COV == COV_MATERN25) {
        const double t = r * A.cA, e = exp(-t), t3 = t * t * (1.0 / 3.0);
        d[0] = e * __builtin_fma(t, __builtin_fma(t, 1.0 / 3.0, 1.0), 1.0);
        d[1] = A.sA * e * t3 * (1.0 + t) * A.irA;                      // sigma^2 e^{-cr} (c^2 r^2 / 3)(1 + cr) / rho
    } else if constexpr (COV == COV_MATERN_GEN) {
        double f[3];
        gen_eval<3>(r2, A, f);
        d[0] = f[0];
        d[1] = A.sA * A.irA * f[1];                                    // sigma^2 c_nu s^{nu+1} K_{nu-1}(s) / rho
        d[2] = A.sA * f[2];
    } else {
        const double t = r * A.cA, e1 = exp(-t), s = r2 * A.cB, e2 = exp(-s);
        d[0] = e1;
        d[1] = A.sA * e1 * t * A.irA;                                  // s1 e^{-r/r1} r / r1^2
        d[2] = e2;
        d[3] = A.sB * e2 * (2.0 * s) * A.irB;                          // s2 e^{-(r/r2)^2} 2 r^2 / r2^3
    }
}

template <int PB, int COV>
__global__ void __launch_bounds__(64 * kGradWavesPerBlock, (PB == 16 ? 3 : (PB == 32 ? 2 : 1)))
    gpv_grad_kernel(const GradArgs A)
{
    constexpr int NPAR = CovTraits<COV>::NPAR;
    __shared__ double s_part[kGradWavesPerBlock][kGradNV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool packed = A.dim <= 3;
    const int64_t nwaves = (int64_t)gridDim.x * kGradWavesPerBlock;
    double acc[kGradNV];
#pragma unroll
    for (int t = 0; t < kGradNV; ++t) acc[t] = 0.0;

    for (int64_t k = (int64_t)blockIdx.x * kGradWavesPerBlock + wave; k < A.rows; k += nwaves) {
        // ---- gather: lane i of the bucket takes entry P - PB + i of the stored row (the valid entries are its LAST n0)
        const int e = A.P - PB + lane;
        const int v = (lane < PB && e >= 0) ? A.nn[k * A.P + e] : -1;
        const bool valid = v >= 0;
        const unsigned long long vmask = __ballot(valid);
        const bool own_ok = (vmask >> (PB - 1)) & 1ull;
        const double zi = valid ? (packed ? A.rec[(int64_t)v * 4 + 3] : (A.z ? A.z[v] : 0.0)) : 0.0;
        double a[PB];
        auto distances = [&]() {                                      // a[j] <- squared distance of (lane, j), src/dist.cpp:12-14
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
        };
        distances();
        // ---- C on the valid rows and columns, zero elsewhere (a product with the 0 / 1 flags of both entries: no per-column
        // lane masks to keep); tau joins the diagonal where the pivot is read, so a padded row is tau times an identity row
        const int vhi = __double2hiint(valid ? 1.0 : 0.0);
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double vj = __hiloint2double(__builtin_amdgcn_readlane(vhi, j), 0);
            a[j] = grad_cov<COV>(gen_r2<COV>(a[j], valid && vj != 0.0), A) * (valid ? vj : 0.0);
            __builtin_amdgcn_sched_barrier(0);                        // one exp at a time: PB interleaved ones spill
        }
        // ---- Gauss-Jordan with the right-hand sides e_last and z_J
        double r1 = (lane == PB - 1) ? 1.0 : 0.0, r2 = zi, dg = 1.0;   // dg: 1 / pivot of the lane's own row
        bool fail = !own_ok;
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double d = readlane_d(a[j], j) + A.nug;
            fail |= !(d > 0.0);                                      // (uniform: every lane holds the same pivot)
            const bool pivot = lane == j;
            const double inv = 1.0 / d;                               // (needed on both sides of the select: stays branch-free)
            const double f = pivot ? 0.0 : a[j] * inv;
            dg = pivot ? inv : dg;
#pragma unroll
            for (int c = j + 1; c < PB; ++c) {
                a[c] = __builtin_fma(-f, readlane_d(a[c], j), a[c]);
            }
            r1 = __builtin_fma(-f, readlane_d(r1, j), r1);
            r2 = __builtin_fma(-f, readlane_d(r2, j), r2);
            __builtin_amdgcn_sched_barrier(0);
        }
        const double u = r1 * dg, w = r2 * dg;                        // exact zeros on the padded rows
        // ---- second pair pass: t_p = sum_j D_p(lane, j) u_j
        distances();
        double tp[NPAR];
#pragma unroll
        for (int p = 0; p < NPAR; ++p) tp[p] = 0.0;
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            double d[NPAR];
            grad_dcov<COV>(gen_r2<COV>(a[j], valid && ((vmask >> j) & 1ull)), A, d);
            const double uj = readlane_d(u, j);
#pragma unroll
            for (int p = 0; p < NPAR; ++p) tp[p] = __builtin_fma(d[p], uj, tp[p]);
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- row terms (every lane ends with the same values)
        const double ul = readlane_d(u, PB - 1);
        const double q = wave_sum(u * zi);
        double val[kGradRowLd];
        val[0] = 0.5 * log(ul) - 0.5 * q * q / ul - 0.91893853320467274178;   // 1/2 log 2 pi
#pragma unroll
        for (int p = 0; p <= NPAR; ++p) {
            const double ai = wave_sum(p < NPAR ? u * tp[p] : u * u);          // the nugget's block is the identity
            const double bi = wave_sum(p < NPAR ? w * tp[p] : w * u);
            val[1 + p] = -0.5 * ai / ul + q * bi / ul - 0.5 * q * q * ai / (ul * ul);
        }
#pragma unroll
        for (int p = NPAR + 2; p < kGradRowLd; ++p) val[p] = 0.0;
        acc[7] += 1.0;
        if (fail) {
            acc[6] += 1.0;
        } else {
#pragma unroll
            for (int p = 0; p < kGradRowLd; ++p) acc[p] += val[p];
        }
        if (A.row_terms != nullptr && lane < kGradRowLd) {
            double mine = 0.0;
#pragma unroll
            for (int p = 0; p < kGradRowLd; ++p) mine = (lane == p) ? val[p] : mine;
            A.row_terms[(int64_t)A.rowid[k] * kGradRowLd + lane] = fail ? __builtin_nan("") : mine;
        }
    }
    // ---- per-workgroup partials, waves added in wave order
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < kGradNV; ++t) s_part[wave][t] = acc[t];
    }
    __syncthreads();
    if (threadIdx.x < kGradNV) {
        double s = 0.0;
        for (int wv = 0; wv < kGradWavesPerBlock; ++wv) s += s_part[wv][threadIdx.x];
        A.block_part[(int64_t)blockIdx.x * kGradNV + threadIdx.x] = s;
    }
}

#include "gpv_fisher_kernel.hpp"
#include "gpv_rep_kernel.hpp"

}  // namespace

#define GPV_GRAD_NAME2(pb) launch_grad_pb##pb
#define GPV_GRAD_NAME(pb) GPV_GRAD_NAME2(pb)
hipError_t GPV_GRAD_NAME(GPV_GRAD_PB)(const GradArgs &a, int grid, hipStream_t stream)
{
    constexpr int PB = GPV_GRAD_PB;
    const dim3 g((unsigned)grid), b(64 * kGradWavesPerBlock);
    switch (a.cov) {
        case COV_MATERN05: hipLaunchKernelGGL((gpv_grad_kernel<PB, COV_MATERN05>), g, b, 0, stream, a); break;
        case COV_MATERN15: hipLaunchKernelGGL((gpv_grad_kernel<PB, COV_MATERN15>), g, b, 0, stream, a); break;
        case COV_MATERN25: hipLaunchKernelGGL((gpv_grad_kernel<PB, COV_MATERN25>), g, b, 0, stream, a); break;
        case COV_ESQE: hipLaunchKernelGGL((gpv_grad_kernel<PB, COV_ESQE>), g, b, 0, stream, a); break;
        case COV_MATERN_GEN: hipLaunchKernelGGL((gpv_grad_kernel<PB, COV_MATERN_GEN>), g, b, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

#define GPV_FISHER_NAME2(pb) launch_fisher_pb##pb
#define GPV_FISHER_NAME(pb) GPV_FISHER_NAME2(pb)
hipError_t GPV_FISHER_NAME(GPV_GRAD_PB)(const GradArgs &a, int grid, hipStream_t stream)
{
    constexpr int PB = GPV_GRAD_PB;
    const dim3 g((unsigned)grid), b(64 * kGradWavesPerBlock);
    switch (a.cov) {
        case COV_MATERN05: hipLaunchKernelGGL((gpv_fisher_kernel<PB, COV_MATERN05>), g, b, 0, stream, a); break;
        case COV_MATERN15: hipLaunchKernelGGL((gpv_fisher_kernel<PB, COV_MATERN15>), g, b, 0, stream, a); break;
        case COV_MATERN25: hipLaunchKernelGGL((gpv_fisher_kernel<PB, COV_MATERN25>), g, b, 0, stream, a); break;
        case COV_ESQE: hipLaunchKernelGGL((gpv_fisher_kernel<PB, COV_ESQE>), g, b, 0, stream, a); break;
        case COV_MATERN_GEN: hipLaunchKernelGGL((gpv_fisher_kernel<PB, COV_MATERN_GEN>), g, b, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

#define GPV_REP_NAME2(pb) launch_rep_pb##pb
#define GPV_REP_NAME(pb) GPV_REP_NAME2(pb)
hipError_t GPV_REP_NAME(GPV_GRAD_PB)(const RepArgs &a, int grid, hipStream_t stream)
{
    constexpr int PB = GPV_GRAD_PB;
    const dim3 g((unsigned)grid), b(64 * kGradWavesPerBlock);
    switch (a.g.cov) {
        case COV_MATERN05: hipLaunchKernelGGL((gpv_rep_kernel<PB, COV_MATERN05>), g, b, 0, stream, a); break;
        case COV_MATERN15: hipLaunchKernelGGL((gpv_rep_kernel<PB, COV_MATERN15>), g, b, 0, stream, a); break;
        case COV_MATERN25: hipLaunchKernelGGL((gpv_rep_kernel<PB, COV_MATERN25>), g, b, 0, stream, a); break;
        case COV_ESQE: hipLaunchKernelGGL((gpv_rep_kernel<PB, COV_ESQE>), g, b, 0, stream, a); break;
        case COV_MATERN_GEN: hipLaunchKernelGGL((gpv_rep_kernel<PB, COV_MATERN_GEN>), g, b, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

#else  // the launcher that picks the bucket, and the second launch

hipError_t launch_grad_pb16(const GradArgs &a, int grid, hipStream_t stream);
hipError_t launch_grad_pb32(const GradArgs &a, int grid, hipStream_t stream);
hipError_t launch_grad_pb64(const GradArgs &a, int grid, hipStream_t stream);

namespace {
// totals[t] = sum over the workgroups, in workgroup order: the same bits for the same launch geometry
__global__ void __launch_bounds__(64) gpv_grad_total_kernel(const double *part, int grid, double *totals)
{
    if (threadIdx.x < kGradNV) {
        double s = 0.0;
        for (int b = 0; b < grid; ++b) s += part[(int64_t)b * kGradNV + threadIdx.x];
        totals[threadIdx.x] = s;
    }
}
}  // namespace

hipError_t launch_fisher_pb16(const GradArgs &a, int grid, hipStream_t stream);
hipError_t launch_fisher_pb32(const GradArgs &a, int grid, hipStream_t stream);
hipError_t launch_fisher_pb64(const GradArgs &a, int grid, hipStream_t stream);

namespace {
__global__ void __launch_bounds__(64) gpv_fisher_total_kernel(const double *part, int grid, double *totals)
{
    if (threadIdx.x < kFisherNV) {
        double s = 0.0;
        for (int b = 0; b < grid; ++b) s += part[(int64_t)b * kFisherNV + threadIdx.x];
        totals[threadIdx.x] = s;
    }
}
}  // namespace

hipError_t launch_rep_pb16(const RepArgs &a, int grid, hipStream_t stream);
hipError_t launch_rep_pb32(const RepArgs &a, int grid, hipStream_t stream);
hipError_t launch_rep_pb64(const RepArgs &a, int grid, hipStream_t stream);

namespace {
// the replicates as they arrive (columns of the ORDERED rows) -> rows by internal position, any padded count rp
__global__ void __launch_bounds__(256) gpv_rep_pack_kernel(const double *__restrict__ in, const int32_t *__restrict__ newpos,
                                                           int64_t n, int R, int rp, double *__restrict__ Z)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * rp) return;
    const int64_t i = t / rp;
    const int c = (int)(t - i * rp);
    Z[(int64_t)newpos[i] * rp + c] = c < R ? in[(int64_t)c * n + i] : 0.0;
}
}  // namespace

int grad_grid(int64_t rows, int cus)
{
    int64_t grid = (rows + kGradWavesPerBlock - 1) / kGradWavesPerBlock;
    const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * kGradBlocksPerCU;
    if (grid > cap) grid = cap;
    return (int)(grid < 1 ? 1 : grid);
}

hipError_t launch_grad(int p, const GradArgs &a, int grid, hipStream_t stream)
{
    if (grid < 1 || a.rows < 0) return hipErrorInvalidValue;
    hipError_t e;
    switch (grad_bucket(p)) {
        case 16: e = launch_grad_pb16(a, grid, stream); break;
        case 32: e = launch_grad_pb32(a, grid, stream); break;
        case 64: e = launch_grad_pb64(a, grid, stream); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gpv_grad_total_kernel, dim3(1), dim3(64), 0, stream, a.block_part, grid, a.totals);
    return hipGetLastError();
}

hipError_t launch_fisher(int p, const GradArgs &a, int grid, hipStream_t stream)
{
    if (grid < 1 || a.rows < 0) return hipErrorInvalidValue;
    hipError_t e;
    switch (grad_bucket(p)) {
        case 16: e = launch_fisher_pb16(a, grid, stream); break;
        case 32: e = launch_fisher_pb32(a, grid, stream); break;
        case 64: e = launch_fisher_pb64(a, grid, stream); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gpv_fisher_total_kernel, dim3(1), dim3(64), 0, stream, a.block_part, grid, a.totals);
    return hipGetLastError();
}

hipError_t launch_rep(int p, const RepArgs &a, int grid, hipStream_t stream)
{
    if (grid < 1 || a.g.rows < 0 || a.Z == nullptr || a.R < 1 || a.RP < a.R || a.RP % kRepChunk != 0) return hipErrorInvalidValue;
    hipError_t e;
    switch (grad_bucket(p)) {
        case 16: e = launch_rep_pb16(a, grid, stream); break;
        case 32: e = launch_rep_pb32(a, grid, stream); break;
        case 64: e = launch_rep_pb64(a, grid, stream); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gpv_fisher_total_kernel, dim3(1), dim3(64), 0, stream, a.g.block_part, grid, a.g.totals);
    return hipGetLastError();
}

hipError_t launch_rep_pack(const double *in, const int32_t *newpos, int64_t n, int R, int rp, double *Z, hipStream_t stream)
{
    if (n < 1 || R < 1 || rp < R) return hipErrorInvalidValue;
    const int64_t blocks = (n * rp + 255) / 256;
    hipLaunchKernelGGL(gpv_rep_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, in, newpos, n, R, rp, Z);
    return hipGetLastError();
}

#endif

}  // namespace gpv
