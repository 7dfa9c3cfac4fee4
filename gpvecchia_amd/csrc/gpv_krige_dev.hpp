// gpv_krige_dev.hpp — device helpers the two local-kriging passes share (gpv_krige.hip, gpv_krige_groups.hip): a double handed
// out of another lane, the wave's butterfly sum and the covariance of a pair from its squared distance.  Not installed.
#pragma once
#include "gpv_krige.h"
#include "gpv_internal.h"

namespace gpv {

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

// general smoothness: C / sigma^2 at s = r / range from the call's table (gpv_bessel.hpp, MaternDTab: the gradient kernels'),
// times one exp(-s); outside the table the quadrature in ONE out-of-line copy; s = 0 is exactly 1
static __device__ __attribute__((noinline)) double gen_direct(const double s, const MaternDerivConst kc)
{
    double f[3];
    matern_general_derivs(s, kc, 0, f);
    return f[0];
}
__device__ __forceinline__ double gen_value(const double r2, const KrigeArgs &A)
{
    const double s = sqrt(r2) * A.cA;
    const int seg = matern_dtab_segment(s, A.gmt_base);
    if ((unsigned)seg < (unsigned)A.gmt_nseg)
        return exp(-s) * matern_dtab_poly(A.gmt + (size_t)seg * MaternDTab::ROW, matern_dtab_u(s));
    if (s == 0.0) return 1.0;
    return gen_direct(s, A.gen);
}

// covariance of a pair from its squared distance: the formulas of cov_from_r2 (gpv_sets_kernel.hpp); r2 == 0 gives the variance
template <int COV>
__device__ __forceinline__ double krige_cov(double r2, const KrigeArgs &A)
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
        return A.sA * gen_value(r2, A);
    } else {
        return __builtin_fma(A.sA, exp(-(r * A.cA)), A.sB * exp(-(r2 * A.cB)));
    }
}

}  // namespace

}  // namespace gpv
