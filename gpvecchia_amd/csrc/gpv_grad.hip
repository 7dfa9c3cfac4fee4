// gpv_grad.hip — value and analytic gradient of the cond.yz='z' Vecchia log-likelihood (gpv_plan_loglik_grad), gfx950, FP64, and
// the set pass its two siblings share with it: with the expected information (gpv_plan_loglik_fisher) and summed over replicates
// (gpv_rep_kernel.hpp).  Every phase of a conditioning set is written once, in gpv_grad_set_pass.inc, the body of all three
// kernels.
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
#include <type_traits>
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
    static constexpr bool SCALED = COV >= kCovScaled05;                // matern_scaledim: one range per coordinate
    static constexpr int BASE = SCALED ? COV - kCovScaled05 : COV;      // the isotropic family its value is (at range 1)
    static constexpr int NPAR = (COV == COV_ESQE || SCALED) ? 4 : (COV == COV_MATERN_GEN ? 3 : 2);   // covariance parameters differentiated
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
template <int COVK>
__device__ __forceinline__ double grad_cov(double r2, const GradArgs &A)
{
    constexpr int COV = CovTraits<COVK>::BASE;                          // (matern_scaledim: on the scaled coordinates, cA = sqrt(2 nu))
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

// matern_scaledim: variance and the three ranges.  r2 = h^2 is the squared distance of the scaled coordinates, dq[t] the squared
// difference of scaled coordinate t, c = A.cA = sqrt(2 nu) (1 at nu = 0.5):
//     dC/drange_t = g(h) dq[t] / range_t,   g = sigma^2 e^{-h} / h,  sigma^2 c^2 e^{-ch},  sigma^2 e^{-ch} (c^2 / 3)(1 + ch)
// At h = 0 every dq[t] is 0; nu = 0.5 would form 0 / 0 there and takes g = 0 instead (the derivative of e^{-h} along a range at a
// coincident pair is 0: h does not move).  An absent coordinate has dq[t] = 0 and an inverse range of 0: exact zeros.
template <int COV>
__device__ __forceinline__ void grad_dcov_scaled(double r2, const double (&dq)[3], const GradArgs &A, double (&d)[4])
{
    const double r = sqrt(r2), t = r * A.cA, e = exp(-t);
    double g;
    if constexpr (COV == kCovScaled05) {
        d[0] = e;
        g = r2 > 0.0 ? A.sA * e / r : 0.0;
    } else if constexpr (COV == kCovScaled15) {
        d[0] = __builtin_fma(t, e, e);
        g = A.sA * (A.cA * A.cA) * e;
    } else {
        d[0] = e * __builtin_fma(t, __builtin_fma(t, 1.0 / 3.0, 1.0), 1.0);
        g = A.sA * e * (A.cA * A.cA * (1.0 / 3.0)) * (1.0 + t);
    }
    d[1] = g * dq[0] * A.irA;                                          // (the inverse ranges: GradArgs)
    d[2] = g * dq[1] * A.irB;
    d[3] = g * dq[2] * A.sB;
}

#include "gpv_rep_kernel.hpp"      // rep_reduce_scatter, and what the replicate mode computes

// a[j] <- squared distance of (lane, j), src/dist.cpp:12-14.  Text and no function, like every phase: see the kernel below
#define GPV_FILL_DISTANCES                                                                                              \
    _Pragma("unroll") for (int j = 0; j < PB; ++j) a[j] = 0.0;                                                          \
    for (int t = 0; t < A.dim; ++t) {                                                                                   \
        const double x = valid ? (packed ? A.rec[(int64_t)v * 4 + t] : A.locs[(int64_t)v * A.locs_ld + t]) : 0.0;       \
        _Pragma("unroll") for (int j = 0; j < PB; ++j) {                                                                \
            const double df = x - readlane_d(x, j);                                                                     \
            a[j] = __builtin_fma(df, df, a[j]);                                                                         \
        }                                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
    }

// ---- the three kernels: the sets of one wavefront, grid-stride ------------------------------------------------------------------
// Every phase of a conditioning set is written once, in the one body gpv_grad_set_pass.inc that each kernel includes; KIND
// selects what a kernel does with it:
//   kSetsGrad    value and gradient: its own pair pass, unrolled, with a[] as scratch for the distances (faster)
//   kSetsFisher  with the expected information: the sweep keeps its multipliers, pair pass tt[], replay y[], triangle (below)
//   kSetsRep     the same summed over the R replicates of Z (gpv_rep_kernel.hpp) instead of the plan's column: the sweep carries
//                no data right-hand side and the row terms are sums over the replicates; nothing else differs from kSetsFisher
// The phases are NOT functions of their own, and the body is text inside each __global__ function.  Behind a function boundary
// (forced inline or not, a lambda, a member function that returns a flag, a device function around the whole body) the compiler
// sees the same arithmetic but schedules and allocates it differently: the sweep gains a third more wait states, and the
// general-nu kernels at PB = 16, which sit at their register cap, spill more and run up to 10 % slower.  Included
// as text, under the kernels' old names, the three code objects are what three separate bodies gave, instruction for instruction
// and at the same offsets (one kernel template with KIND as a parameter gives the same instructions 0x300 bytes further on, and
// two legs at m = 60 then measure 0.4 - 0.9 % slower).  kSetsGrad fills the distances through a lambda, twice, as gpv_grad_kernel
// always did; the other two expand the same text in place.
//
// The information, per set, with t_i = D_i u (t = u for the nugget), a_i = u't_i and y_j = S'^-1 t_j:
//     F_k[i, j] = t_i'y_j / u_last - 1/2 a_i a_j / u_last^2
// which is 1/2 tr(S'^-1 D_i S'^-1 D_j) of the block minus the same trace of its leading block without the set's own point: with
// L L' = S' only the last row of L^-1 D_i L^-T differs between the two, and that row is (L^-1 D_i v)' with v = u / sqrt(u_last).
// It is the expectation of -d2 l_k / dtheta_i dtheta_j under the exact process.  The solves y_j REPLAY the elimination instead of
// repeating it: after step j of the sweep column j of the block is dead, so the step's multiplier is kept there (and 1 / pivot in
// dg); a further right-hand side then costs PB fused multiply-adds and read-lanes.  The pair pass that forms t_i therefore may
// not use a[] as scratch: it recomputes each pair's squared distance inside its loop over the columns, from coordinates held in
// registers (dimension <= 3) or loaded per (column, coordinate), summing over the coordinates in the order of the first pass, so
// the distances are the same bits.  That loop indexes no register array and is not unrolled over the whole row.
enum { kSetsGrad, kSetsFisher, kSetsRep };
#define GPV_GRAD_BOUNDS __launch_bounds__(64 * kGradWavesPerBlock, (PB == 16 ? 3 : (PB == 32 ? 2 : 1)))
template <int PB, int COV>
__global__ void GPV_GRAD_BOUNDS gpv_grad_kernel(const GradArgs A)
{
    constexpr int KIND = kSetsGrad;
    const double *const repZ = nullptr;
    constexpr int repR = 0, repRP = 0;
#include "gpv_grad_set_pass.inc"
}

template <int PB, int COV>
__global__ void GPV_GRAD_BOUNDS gpv_fisher_kernel(const GradArgs A)
{
    constexpr int KIND = kSetsFisher;
    const double *const repZ = nullptr;
    constexpr int repR = 0, repRP = 0;
#include "gpv_grad_set_pass.inc"
}

template <int PB, int COV>
__global__ void GPV_GRAD_BOUNDS gpv_rep_kernel(const RepArgs B)
{
    constexpr int KIND = kSetsRep;
    const GradArgs &A = B.g;
    const double *const repZ = B.Z;
    const int repR = B.R, repRP = B.RP;
#include "gpv_grad_set_pass.inc"
}

#undef GPV_FILL_DISTANCES

template <int KIND, int COV, class ARGS>
void launch_one(dim3 g, dim3 b, hipStream_t stream, const ARGS &a)
{
    constexpr int PB = GPV_GRAD_PB;
    if constexpr (KIND == kSetsGrad) hipLaunchKernelGGL((gpv_grad_kernel<PB, COV>), g, b, 0, stream, a);
    else if constexpr (KIND == kSetsFisher) hipLaunchKernelGGL((gpv_fisher_kernel<PB, COV>), g, b, 0, stream, a);
    else hipLaunchKernelGGL((gpv_rep_kernel<PB, COV>), g, b, 0, stream, a);
}

template <int KIND, class ARGS>
hipError_t launch_cov(const int cov, const ARGS &a, const int grid, hipStream_t stream)
{
    const dim3 g((unsigned)grid), b(64 * kGradWavesPerBlock);
    switch (cov) {
        case COV_MATERN05: launch_one<KIND, COV_MATERN05>(g, b, stream, a); break;
        case COV_MATERN15: launch_one<KIND, COV_MATERN15>(g, b, stream, a); break;
        case COV_MATERN25: launch_one<KIND, COV_MATERN25>(g, b, stream, a); break;
        case COV_ESQE: launch_one<KIND, COV_ESQE>(g, b, stream, a); break;
        case COV_MATERN_GEN: launch_one<KIND, COV_MATERN_GEN>(g, b, stream, a); break;
        case kCovScaled05: launch_one<KIND, kCovScaled05>(g, b, stream, a); break;
        case kCovScaled15: launch_one<KIND, kCovScaled15>(g, b, stream, a); break;
        case kCovScaled25: launch_one<KIND, kCovScaled25>(g, b, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

#define GPV_GRAD_NAME2(kind, pb) launch_##kind##_pb##pb
#define GPV_GRAD_NAME(kind, pb) GPV_GRAD_NAME2(kind, pb)
hipError_t GPV_GRAD_NAME(grad, GPV_GRAD_PB)(const GradArgs &a, int grid, hipStream_t stream)
{
    return launch_cov<kSetsGrad>(a.cov, a, grid, stream);
}
hipError_t GPV_GRAD_NAME(fisher, GPV_GRAD_PB)(const GradArgs &a, int grid, hipStream_t stream)
{
    return launch_cov<kSetsFisher>(a.cov, a, grid, stream);
}
hipError_t GPV_GRAD_NAME(rep, GPV_GRAD_PB)(const RepArgs &a, int grid, hipStream_t stream)
{
    return launch_cov<kSetsRep>(a.g.cov, a, grid, stream);
}

#else  // the launcher that picks the bucket, and the second launch

#define GPV_GRAD_BUCKETS(kind, ARGS)                                                 \
    hipError_t launch_##kind##_pb16(const ARGS &a, int grid, hipStream_t stream); \
    hipError_t launch_##kind##_pb32(const ARGS &a, int grid, hipStream_t stream); \
    hipError_t launch_##kind##_pb64(const ARGS &a, int grid, hipStream_t stream);
GPV_GRAD_BUCKETS(grad, GradArgs)
GPV_GRAD_BUCKETS(fisher, GradArgs)
GPV_GRAD_BUCKETS(rep, RepArgs)

namespace {
// totals[t] = sum over the workgroups, in workgroup order: the same bits for the same launch geometry
template <int NV>
__global__ void __launch_bounds__(64) gpv_grad_total_kernel(const double *part, int grid, double *totals)
{
    if (threadIdx.x < NV) {
        double s = 0.0;
        for (int b = 0; b < grid; ++b) s += part[(int64_t)b * NV + threadIdx.x];
        totals[threadIdx.x] = s;
    }
}
}  // namespace

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

namespace {
// both launches of a call: the set pass of the row's bucket (pb[] = its launchers for 16, 32, 64), then the sum of its partials
template <int NV, class ARGS>
hipError_t launch_sets(int p, const ARGS &a, const GradArgs &g, int grid, hipStream_t stream,
                       hipError_t (*const (&pb)[3])(const ARGS &, int, hipStream_t))
{
    const int bucket = grad_bucket(p);
    if (grid < 1 || g.rows < 0 || bucket == 0) return hipErrorInvalidValue;
    const hipError_t e = pb[bucket == 16 ? 0 : (bucket == 32 ? 1 : 2)](a, grid, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gpv_grad_total_kernel<NV>, dim3(1), dim3(64), 0, stream, g.block_part, grid, g.totals);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_grad(int p, const GradArgs &a, int grid, hipStream_t stream)
{
    return launch_sets<kGradNV>(p, a, a, grid, stream, {launch_grad_pb16, launch_grad_pb32, launch_grad_pb64});
}

hipError_t launch_fisher(int p, const GradArgs &a, int grid, hipStream_t stream)
{
    return launch_sets<kFisherNV>(p, a, a, grid, stream, {launch_fisher_pb16, launch_fisher_pb32, launch_fisher_pb64});
}

hipError_t launch_rep(int p, const RepArgs &a, int grid, hipStream_t stream)
{
    if (a.Z == nullptr || a.R < 1 || a.RP < a.R || a.RP % kRepChunk != 0) return hipErrorInvalidValue;
    return launch_sets<kFisherNV>(p, a, a.g, grid, stream, {launch_rep_pb16, launch_rep_pb32, launch_rep_pb64});
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
