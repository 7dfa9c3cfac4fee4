// gpv_bessel.hpp — modified Bessel function of the second kind K_nu(x), real order nu >= 0, x > 0, FP64,
// for the general-smoothness branch of the Matern covariance (reference: src/Matern.cpp:72-84, which calls
// boost::math::cyl_bessel_k; Boost is a third-party dependency absent from the reference tree).
//
// Method (own derivation from the integral representation, no series / continued-fraction routine restated):
//     K_mu(x) = int_0^inf exp(-x cosh t) cosh(mu t) dt                      (Abramowitz & Stegun 9.6.24)
// is the integral of an entire, even function that decays doubly exponentially, so the plain trapezoidal rule converges
// geometrically in 1/h (the classical result for analytic integrands on the real line; Trefethen & Weideman, SIAM Review
// 56 (2014) 385).  Pushing the contour to Im t = d multiplies the integrand by at most exp(x (1 - cos d)), the rule's
// error is exp(-2 pi d / h) times that: with d = pi/2 the relative error is exp(x - pi^2 / h), with the optimal
// d = 2 pi / (h x) for large x it is exp(-2 pi^2 / (h^2 x)).  Step h = min(pi^2 / (x + 44), 0.66 / sqrt(x)) keeps both
// below 1e-19; the sum stops when a term falls below 1e-19 of it, after 12 .. 70 points (more only for x < 1e-9).  All
// terms are positive: no cancellation anywhere, for any order and argument.  What is summed is the SCALED function
// e^x K_mu(x), from exp(-x (cosh t - 1)) with cosh t - 1 = 2 sinh^2(t/2), so nothing underflows for large x.
// Orders above 1/2: nu = n + mu, |mu| <= 1/2; K_mu and K_{mu+1} share the exponential weights, then the recurrence
// K_{v+1} = K_{v-1} + (2v/x) K_v, which is stable upwards.  Measured against 40-digit mpmath: <= 1e-15 relative for
// nu <= 11, <= 5e-15 at nu = 60 (the recurrence's n/2 ulp), x from 1e-8 to 700.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

namespace gpv {

// e^x K_nu(x), nu >= 0, x > 0
__host__ __device__ inline double bessel_k_scaled(const double nu, const double x)
{
    const int n_up = (int)(nu + 0.5);
    const double mu = nu - (double)n_up;
    double k0, k1;
    if (x > 746.0) {
        // the callers multiply by e^-x = 0 out here; Hankel's expansion, three terms (relative error < 1e-6 mu^6 / x^3)
        const double a0 = 4.0 * mu * mu, a1 = 4.0 * (mu + 1.0) * (mu + 1.0), r8 = 0.125 / x;
        const double pre = sqrt(1.57079632679489661923 / x);
        k0 = pre * (1.0 + (a0 - 1.0) * r8 * (1.0 + (a0 - 9.0) * 0.5 * r8));
        k1 = pre * (1.0 + (a1 - 1.0) * r8 * (1.0 + (a1 - 9.0) * 0.5 * r8));
    } else {
        const double h1 = 9.8696044010893586188 / (x + 44.0), h2 = 0.66 / sqrt(x);
        const double h = h1 < h2 ? h1 : h2;
        double sum0 = 0.5, sum1 = 0.5;                              // the t = 0 node carries half weight
        for (int j = 1; j < 6000; ++j) {
            const double t = (double)j * h;
            const double sh = sinh(0.5 * t);
            const double arg = 2.0 * x * sh * sh;                   // x (cosh t - 1)
            if (arg > 745.0) break;
            const double w = exp(-arg);
            const double gm = exp(mu * t), g1 = gm * exp(t);
            const double c0 = 0.5 * (gm + 1.0 / gm);                // cosh(mu t)
            const double c1 = 0.5 * (g1 + 1.0 / g1);                // cosh((mu + 1) t)
            sum0 = __builtin_fma(w, c0, sum0);
            sum1 = __builtin_fma(w, c1, sum1);
            if (w * c1 < 1e-19 * sum1) break;
        }
        k0 = h * sum0;
        k1 = h * sum1;
    }
    const double two_over_x = 2.0 / x;
    for (int i = 1; i <= n_up; ++i) {
        const double up = __builtin_fma((mu + (double)i) * two_over_x, k1, k0);
        k0 = k1;
        k1 = up;
    }
    return k0;
}

__host__ __device__ inline double bessel_k_nu(const double nu, const double x) { return exp(-x) * bessel_k_scaled(nu, x); }

// sigma^2 2^{1-nu}/Gamma(nu) s^nu K_nu(s) = normcon s^nu K_nu(s), s = dist/range  (src/Matern.cpp:73,80; the reference applies
// no sqrt(2 nu) scaling there)
__host__ __device__ inline double matern_general(const double s, const double normcon, const double nu)
{
    return normcon * exp(nu * log(s) - s) * bessel_k_scaled(nu, s);
}

// ---- per-launch table of h(s) = s^nu K_nu(s) e^s ------------------------------------------------------------------
// nu is fixed inside a launch and h is smooth and slowly varying away from s = 0, so the host fits it once per
// evaluation on the segments [2^e (1 + m/8), 2^e (1 + (m+1)/8)), m = 0..7 (segment index = the exponent and the three
// leading mantissa bits of s: one shift).  Per segment the function is interpolated at 11 Chebyshev points (degree 10: the
// nearest singularity, s = 0, is at least 17 half-widths from the centre, so the truncation error is below 34^-11 ~ 1.4e-17
// relative) and the interpolant is stored in the MONOMIAL basis of u = (s - centre) / half-width: its coefficients decay like
// 17^-k (Taylor radius over half-width), so Horner's rule on |u| <= 1 has no cancellation and costs 10 FMAs.  u needs no
// table entry: with s = 2^e (1 + f), u = 2 frac(8 f) - 1, i.e. the mantissa shifted left by three bits, read as a number
// g in [1, 2): u = 2 g - 3.  The caller's constant factor is multiplied into the coefficients.
// One segment is one 96-byte row {scale a_0 .. scale a_10, 0}: what the set kernel pays for per pair is LDS bandwidth
// (rows are gathered by every lane's own distance), so the row is as short as the accuracy allows: round 2 began with
// four segments per octave at degree 12 in the Chebyshev basis (128-byte rows, Clenshaw).  The device multiplies by
// exp(-s); distances outside the tabulated range are evaluated by the quadrature above.
// Round 3: the rows of the segments BELOW s = 4 (binary exponent < FOLD_EXP) hold the covariance itself, scale s^nu K_nu(s),
// with exp(-s) folded in: there the half-width is at most 1/8, exp(-s) is as well approximated as h (its Taylor terms fall
// like (1/8)^k / k!, 3e-18 at k = 11), and a wave whose 64 arguments all lie below 4 -- every pair of a plan whose range
// is not far below its neighbour distances -- skips the 18 instructions of exp(-s) per pair.
// Row format (round 3: 72 bytes instead of 96, so that the LDS window of the set kernel spans 8 octaves instead of 6 in the same
// space; a lane whose segment misses the window waits for a row from global memory, and 23 % of the pair rounds had such a
// lane with 6 octaves, 2 % with 8): a_0 .. a_6 as doubles, a_7 .. a_10 as FLOATS relative to 2^E, E = the binary exponent of
// a_0 (two per double slot, low word first).  a_k falls like 17^-k, so the tail a_7 u^7 + .. is below 2.4e-9 |a_0| and its
// float rounding (6e-8) below 1.5e-16; it is evaluated in FP32 as well and joins the FP64 Horner chain through one
// conversion and one multiplication by 2^E (the exponent bits of a_0).
// Round 6, GPV_MT_F64 = 1: SIXTEEN segments per octave at degree 8, all nine coefficients doubles — the same 72 bytes per
// row (what a pair pays in LDS bandwidth), no FP32 tail: 8 FMAs where the mixed row costs 6 FMAs + conversion, three FP32
// FMAs, the 2^E extraction, conversion back and a multiplication.  The nearest singularity (s = 0) is at least 33 half-widths
// from a segment's centre: interpolation error ~ 66^-9 = 4e-17 relative, coefficients decay like 33^-k.  A window of 8
// octaves is then 128 rows = 9.2 KB: it fits where ONE eight-wavefront workgroup per CU shares it (gpv_sets_kernel.hpp, wpb).
#ifndef GPV_MT_F64
#define GPV_MT_F64 0
#endif
struct MaternTab {
#if GPV_MT_F64
    static constexpr int DEG = 8, NDBL = 9, ROW = 9, LSPO = 4, SPO = 1 << LSPO;
#else
    static constexpr int DEG = 10, NDBL = 7, ROW = 9, LSPO = 3, SPO = 1 << LSPO;   // degree, double coefficients, doubles per row, segments per octave
#endif
    static constexpr bool ALLF64 = NDBL == DEG + 1;
    static constexpr int FOLD_EXP = 2;                                      // segments with binary exponent < 2 carry exp(-s)
};
// the host side of the format: monomial coefficients a[0..DEG] (already scaled) -> one row
inline void matern_tab_pack_row(const double *a, double *row)
{
    for (int j = 0; j < MaternTab::NDBL; ++j) row[j] = a[j];
    if (MaternTab::ALLF64) return;
    int E = 0;
    if (a[0] != 0.0 && std::isfinite(a[0])) (void)std::frexp(a[0], &E), E -= 1;       // a_0 = m 2^E, 1 <= |m| < 2
    float t[4];
    for (int k = 0; k < 4; ++k) {
        const double v = std::ldexp(a[MaternTab::NDBL + k], -E);
        t[k] = (std::fabs(v) < 3.0e38) ? (float)v : (v > 0 ? 3.0e38f : -3.0e38f);
        if (v != v) t[k] = (float)v;
    }
    std::memcpy(row + MaternTab::NDBL, t, sizeof(t));
}
#define GPV_MT_FOLD_BELOW 4.0                                               // = 2^FOLD_EXP
__device__ __forceinline__ int matern_tab_segment(const double s, const int base)
{
    return (int)(__double_as_longlong(s) >> (52 - MaternTab::LSPO)) - base;
}
// r[0..6] = a_0 .. a_6, r[7] = {t_7, t_8}, r[8] = {t_9, t_10} (floats)
__device__ __forceinline__ double matern_tab_poly(const double (&r)[MaternTab::ROW], const double s)
{
    // g = the mantissa of s shifted left by LSPO bits under the exponent of 1.0, u = 2 g - 3; as two 32-bit halves: a funnel
    // shift, a shift and an and-or (the 64-bit form cost a quarter-rate 64-bit shift and two needless ands)
    const unsigned lo = (unsigned)__double2loint(s), hi = (unsigned)__double2hiint(s);
    const unsigned ghi = (__builtin_amdgcn_alignbit(hi, lo, 32 - MaternTab::LSPO) & 0x000FFFFFu) | 0x3FF00000u;
    const double u = __builtin_fma(__hiloint2double((int)ghi, (int)(lo << MaternTab::LSPO)), 2.0, -3.0);
    if constexpr (MaternTab::ALLF64) {
        double p = r[MaternTab::DEG];
#pragma unroll
        for (int k = MaternTab::DEG - 1; k >= 0; --k) p = __builtin_fma(p, u, r[k]);
        return p;
    }
    const float uf = (float)u;
    float t = __builtin_fmaf(__int_as_float(__double2hiint(r[8])), uf, __int_as_float(__double2loint(r[8])));
    t = __builtin_fmaf(t, uf, __int_as_float(__double2hiint(r[7])));
    t = __builtin_fmaf(t, uf, __int_as_float(__double2loint(r[7])));
    const double pw = __hiloint2double(__double2hiint(r[0]) & 0x7FF00000, 0);      // 2^E
    double p = __builtin_fma((double)t * pw, u, r[6]);
    p = __builtin_fma(p, u, r[5]);
    p = __builtin_fma(p, u, r[4]);
    p = __builtin_fma(p, u, r[3]);
    p = __builtin_fma(p, u, r[2]);
    p = __builtin_fma(p, u, r[1]);
    return __builtin_fma(p, u, r[0]);
}

// The same quadrature for MANY arguments at one order (the table fit below evaluates K_nu ~1.5e3 times per likelihood
// evaluation): with a common step the nodes t_j = j h, their weights' exponents q_j = 2 sinh^2(t_j / 2) and the factors
// cosh(mu t_j), cosh((mu + 1) t_j) do not depend on x, so one argument costs one exp per node instead of four
// transcendental functions.  Three classes of x share a step each (the step bound of bessel_k_scaled at the class's upper end).
struct BesselQuadNodes {
    double mu = 0.0, h = 0.0;
    int n_up = 0;
    std::vector<double> q, c0, c1;
    void init(double nu, double x_hi)
    {
        n_up = (int)(nu + 0.5);
        mu = nu - (double)n_up;
        const double h1 = 9.8696044010893586188 / (x_hi + 44.0), h2 = 0.66 / std::sqrt(x_hi);
        h = h1 < h2 ? h1 : h2;
        q.clear(); c0.clear(); c1.clear();
    }
    void extend(size_t n)                                // nodes 1 .. n
    {
        for (size_t j = q.size() + 1; j <= n; ++j) {
            const double t = (double)j * h, sh = std::sinh(0.5 * t);
            const double gm = std::exp(mu * t), g1 = gm * std::exp(t);
            q.push_back(2.0 * sh * sh);
            c0.push_back(0.5 * (gm + 1.0 / gm));
            c1.push_back(0.5 * (g1 + 1.0 / g1));
        }
    }
    // nodes needed for arguments down to x_lo: until x_lo q_j > 745 (the weight underflows) -- the sums stop earlier
    void reserve_for(double x_lo)
    {
        const double t_end = 2.0 * std::asinh(std::sqrt(0.5 * 760.0 / x_lo));
        extend((size_t)(t_end / h) + 2);
    }
    double scaled(double x) const                        // e^x K_nu(x)
    {
        double s0 = 0.5, s1 = 0.5;
        for (size_t j = 0; j < q.size(); ++j) {
            const double a = x * q[j];
            if (a > 745.0) break;
            const double w = std::exp(-a);
            s0 = std::fma(w, c0[j], s0);
            s1 = std::fma(w, c1[j], s1);
            if (w * c1[j] < 1e-19 * s1) break;
        }
        double k0 = h * s0, k1 = h * s1;
        const double two_over_x = 2.0 / x;
        for (int i = 1; i <= n_up; ++i) {
            const double up = std::fma((mu + (double)i) * two_over_x, k1, k0);
            k0 = k1;
            k1 = up;
        }
        return k0;
    }
};

// Which segments a table for arguments in [smin, smax] holds: binary exponent of the first one, index base for
// matern_tab_segment, their number.  *full (may be nullptr): 1 when [smin, smax] lies inside the tabulated range (nothing was
// cut at either end).  Returns false when there is nothing to tabulate.
inline bool matern_tab_range(double smin, double smax, int max_seg, int *e_lo_out, int *base_idx, int *nseg, int *full = nullptr)
{
    if (full) *full = 0;
    constexpr int SPO = MaternTab::SPO;
    int e_lo = (int)std::floor(std::log2(smin)), e_hi = (int)std::floor(std::log2(smax));
    bool cut = false;
    if (e_lo < -200) { e_lo = -200; cut = true; }
    if (e_hi > 8) { e_hi = 8; cut = true; }                   // s < 512: K_nu(s) e^s stays in range; beyond, the value is ~0 anyway
    if (e_hi < e_lo) { *nseg = 0; *base_idx = 0; *e_lo_out = 0; return false; }
    if ((e_hi - e_lo + 1) * SPO > max_seg) { e_lo = e_hi + 1 - max_seg / SPO; cut = true; }
    if (full) *full = cut ? 0 : 1;
    *e_lo_out = e_lo;
    *base_idx = (e_lo + 1023) << MaternTab::LSPO;
    *nseg = (e_hi - e_lo + 1) * SPO;
    return true;
}

// The fit on the host (the evaluation path fits on the device: gpv_matern_tab_kernel, gpv_aux_kernels.hip; this one is kept
// as its cross-check, GPV_MATERN_TABLE_HOST=1)
inline void matern_tab_build(double nu, double smin, double smax, double scale, double *rows /* nseg x ROW */, int *base_idx,
                             int *nseg, int max_seg, int *full = nullptr)
{
    constexpr int N = MaternTab::DEG + 1, SPO = MaternTab::SPO;
    int e_lo = 0;
    if (!matern_tab_range(smin, smax, max_seg, &e_lo, base_idx, nseg, full)) return;
    const int e_hi = e_lo + *nseg / SPO - 1;
    double cs[N][N];
    for (int k = 0; k < N; ++k)
        for (int j = 0; j < N; ++j) cs[k][j] = std::cos(3.14159265358979323846 * k * (j + 0.5) / N);
    // T_k(u) = sum_j tk[k][j] u^j (integers up to 2^9: exact)
    double tk[N][N] = {};
    tk[0][0] = 1.0;
    tk[1][1] = 1.0;
    for (int k = 2; k < N; ++k)
        for (int j = 0; j < N; ++j) tk[k][j] = (j > 0 ? 2.0 * tk[k - 1][j - 1] : 0.0) - tk[k - 2][j];
    // shared quadrature nodes: arguments up to 6, up to 56, up to 746 (the table ends below 512)
    const double s_lo = std::ldexp(1.0, e_lo), s_hi = std::ldexp(1.0, e_hi + 1);
    const double cls_hi[3] = {6.0, 56.0, 746.0};
    BesselQuadNodes nodes[3];
    for (int c = 0; c < 3; ++c) {
        const double lo = (c == 0) ? 0.0 : cls_hi[c - 1];           // the class takes arguments in (lo, cls_hi[c]]
        if (s_hi <= lo || s_lo > cls_hi[c]) continue;               // no table argument falls into it
        nodes[c].init(nu, cls_hi[c]);
        nodes[c].reserve_for(lo > s_lo ? lo : s_lo);
    }
    auto kscaled = [&](double x) {
        const int c = x <= cls_hi[0] ? 0 : (x <= cls_hi[1] ? 1 : 2);
        return nodes[c].q.empty() ? bessel_k_scaled(nu, x) : nodes[c].scaled(x);
    };
    // rows are independent: a few host threads keep the fit well below the kernel's time
    const int nseg_ = *nseg;
    auto fit_rows = [&](int seg_b, int seg_e) {
    for (int seg = seg_b; seg < seg_e; ++seg) {
        const int e = e_lo + seg / SPO, m = seg % SPO;
        const double c = std::ldexp(1.0 + (m + 0.5) / SPO, e), hw = std::ldexp(1.0, e - 1 - MaternTab::LSPO);
        double f[N];
        for (int j = 0; j < N; ++j) {
            const double s = c + hw * cs[1][j];
            f[j] = std::exp(nu * std::log(s) - (e < MaternTab::FOLD_EXP ? s : 0.0)) * kscaled(s);
        }
        long double ch[N];
        for (int k = 0; k < N; ++k) {
            long double a = 0.0L;
            for (int j = 0; j < N; ++j) a += (long double)f[j] * (long double)cs[k][j];
            ch[k] = a * (k == 0 ? 1.0L : 2.0L) / N;
        }
        double mono[N];
        for (int j = 0; j < N; ++j) {
            long double a = 0.0L;
            for (int k = N - 1; k >= j; --k) a += ch[k] * (long double)tk[k][j];     // smallest terms first
            mono[j] = (double)(a * (long double)scale);
        }
        matern_tab_pack_row(mono, rows + (size_t)seg * MaternTab::ROW);
    }
    };
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)(hw ? (hw > 4 ? 4 : hw) : 2);             // ~0.5 ms of work in all: more threads cost more than they save
    if (nseg_ < 16 * nt) nt = 1;
    if (nt <= 1) {
        fit_rows(0, nseg_);
    } else {
        std::vector<std::thread> th;
        const int chunk = (nseg_ + nt - 1) / nt;
        for (int t = 0; t < nt; ++t) {
            const int b0 = t * chunk, e0 = (b0 + chunk < nseg_) ? b0 + chunk : nseg_;
            if (b0 < e0) th.emplace_back(fit_rows, b0, e0);
        }
        for (auto &x : th) x.join();
    }
}

// ---- derivatives of the general-nu Matern in range and in nu (gpv_plan_loglik_grad_nu / _fisher_nu) ---------------------
// C(r) / sigma^2 = c_nu s^nu K_nu(s), s = r / rho, c_nu = 2^{1-nu} / Gamma(nu).  With d/ds [s^nu K_nu] = -s^nu K_{nu-1}:
//     dC/drho = sigma^2 c_nu s^{nu+1} K_{nu-1}(s) / rho,
//     dC/dnu  = C (ln s - ln 2 - psi(nu)) + sigma^2 c_nu s^nu dK_nu(s)/dnu,
//     dK_nu(x)/dnu = int_0^inf exp(-x cosh t) t sinh(nu t) dt        (the representation above, differentiated under the integral):
// the integrand is entire, decays doubly exponentially and every term of its trapezoidal sum has the sign of nu, so the nodes,
// the step and the weights exp(-x (cosh t - 1)) of bessel_k_scaled serve it as they are.
// Orders above 1/2 climb from mu, mu + 1 (nu = n + mu, |mu| <= 1/2) by the recurrence and its derivative in the order,
//     K_{v+1} = K_{v-1} + (2v/x) K_v,        K'_{v+1} = K'_{v-1} + (2/x) K_v + (2v/x) K'_v,
// carried in the scaled quantities A_i = (x/2)^i K_{mu+i}, B_i = (x/2)^i K'_{mu+i}:
//     A_{i+1} = (x/2)^2 A_{i-1} + (mu+i) A_i,     B_{i+1} = (x/2)^2 B_{i-1} + A_i + (mu+i) B_i,
// which hold no division by x: A_n stays near Gamma(nu) / 2 (2/x)^mu as x -> 0, where K_nu itself overflows for large nu.
// Then s^nu K_nu = 2^n s^mu A_n and s^{nu+1} K_{nu-1} = 2^{n-1} s^{mu+2} A_{n-1}.
// K_{nu-1} for nu < 1/2 (n = 0) is K_{1-mu}: it has its own weight cosh((1 - mu) t) in the shared sum, because the downward
// recurrence K_{mu+1} - (2 mu / x) K_mu cancels catastrophically at small x.
struct BesselTriple {
    double a_n;      // e^x (x/2)^n K_nu(x)
    double a_m;      // n >= 1: e^x (x/2)^{n-1} K_{nu-1}(x);  n = 0: e^x K_{1-nu}(x)
    double b_n;      // e^x (x/2)^n dK_nu(x)/dnu
    int n_up;
    double mu;
};

// from e^x {K_mu, K_{mu+1}, K_{1-mu}, K'_mu, K'_{mu+1}}(x) to the triple: the climb
__host__ __device__ inline BesselTriple bessel_k_triple_climb(const int n_up, const double mu, const double x, const double k0,
                                                              const double k1, const double km, const double d0, const double d1)
{
    BesselTriple o;
    o.n_up = n_up;
    o.mu = mu;
    if (n_up == 0) {
        o.a_n = k0; o.a_m = km; o.b_n = d0;
        return o;
    }
    // A_0 = K_mu, A_1 = (x/2) K_{mu+1}; the same for B
    const double hx = 0.5 * x, hx2 = hx * hx;
    double a0 = k0, a1 = hx * k1, b0 = d0, b1 = hx * d1;
    for (int i = 1; i < n_up; ++i) {
        const double v = mu + (double)i;
        const double an = __builtin_fma(v, a1, hx2 * a0);
        const double bn = __builtin_fma(v, b1, __builtin_fma(hx2, b0, a1));
        a0 = a1; a1 = an;
        b0 = b1; b1 = bn;
    }
    o.a_n = a1; o.a_m = a0; o.b_n = b1;
    return o;
}

// one pass over the quadrature nodes, 0 < x; beyond x = 746 (the callers' e^-x is 0 there) Hankel's expansion, three terms
__host__ __device__ inline BesselTriple bessel_k_triple_scaled(const double nu, const double x)
{
    const int n_up = (int)(nu + 0.5);
    const double mu = nu - (double)n_up;
    double k0, k1, d0, d1, km;
    if (x > 746.0) {
        const double r8 = 0.125 / x, pre = sqrt(1.57079632679489661923 / x);
        const double m1 = mu + 1.0, m2 = 1.0 - mu;
        const double a0 = 4.0 * mu * mu, a1 = 4.0 * m1 * m1, a2 = 4.0 * m2 * m2;
        k0 = pre * (1.0 + (a0 - 1.0) * r8 * (1.0 + (a0 - 9.0) * 0.5 * r8));
        k1 = pre * (1.0 + (a1 - 1.0) * r8 * (1.0 + (a1 - 9.0) * 0.5 * r8));
        km = pre * (1.0 + (a2 - 1.0) * r8 * (1.0 + (a2 - 9.0) * 0.5 * r8));
        d0 = pre * 8.0 * mu * r8 * (1.0 + (a0 - 5.0) * r8);          // d/d mu of the same three terms
        d1 = pre * 8.0 * m1 * r8 * (1.0 + (a1 - 5.0) * r8);
    } else {
        const double h1 = 9.8696044010893586188 / (x + 44.0), h2 = 0.66 / sqrt(x);
        const double h = h1 < h2 ? h1 : h2;
        double sum0 = 0.5, sum1 = 0.5, summ = 0.5, sd0 = 0.0, sd1 = 0.0;   // t sinh(.) vanishes at the t = 0 node
        for (int j = 1; j < 6000; ++j) {
            const double t = (double)j * h;
            const double sh = sinh(0.5 * t);
            const double arg = 2.0 * x * sh * sh;                   // x (cosh t - 1)
            if (arg > 745.0) break;
            const double w = exp(-arg);
            const double et = exp(t), gm = exp(mu * t), g1 = gm * et, g2 = et / gm;
            const double c1 = 0.5 * (g1 + 1.0 / g1);                // cosh((mu + 1) t): the largest of the five factors / t
            sum0 = __builtin_fma(w, 0.5 * (gm + 1.0 / gm), sum0);
            sum1 = __builtin_fma(w, c1, sum1);
            summ = __builtin_fma(w, 0.5 * (g2 + 1.0 / g2), summ);   // cosh((1 - mu) t)
            const double wt = w * t;
            sd0 = __builtin_fma(wt, 0.5 * (gm - 1.0 / gm), sd0);    // t sinh(mu t)
            sd1 = __builtin_fma(wt, 0.5 * (g1 - 1.0 / g1), sd1);    // t sinh((mu + 1) t)
            if (w * c1 < 1e-19 * sum1 && wt * c1 < 1e-19 * sd1) break;
        }
        k0 = h * sum0; k1 = h * sum1; km = h * summ; d0 = h * sd0; d1 = h * sd1;
    }
    return bessel_k_triple_climb(n_up, mu, x, k0, k1, km, d0, d1);
}

// Constants of one smoothness, prepared on the host (the C++ library has no digamma: gpv_digamma, gpv_api.hip)
struct MaternDerivConst {
    double nu;
    double lnc;      // ln c_nu = (1 - nu) ln 2 - lgamma(nu)
    double lpsi;     // ln 2 + psi(nu)
};

// The smoothness derivative at SMALL s.  There C (ln s - ln 2 - psi) and c_nu s^nu dK/dnu are two terms of size ln(1/s) whose sum
// is O(s^min(2 nu, 2) ln s): formed from the triple it keeps an ABSOLUTE error of a few 1e-15, which the bilinear forms u'Du of a
// plan whose range is far above its distances multiply by |u|_1^2 ~ 1e4 (measured: the smoothness column of the totals missed the
// 1e-8 bar at range 50).  Below s = kDnuSmallS it is therefore taken from the mixture representation
//     C / sigma^2 = E[exp(-s^2 / (4 T))],  T ~ Gamma(nu)            (K_nu(s) = 1/2 (s/2)^-nu int_0^inf e^{-t - s^2/(4t)} t^{nu-1} dt)
//     d/dnu       = -1 / Gamma(nu) int_0^inf e^-t t^{nu-1} (ln t - psi(nu)) (1 - exp(-s^2 / (4t))) dt       (E[ln T] = psi(nu)),
// whose integrand holds the small factor 1 - exp(-s^2 / 4t) explicitly (expm1): no cancellation beyond the O(1) one between
// t < e^psi and t > e^psi, RELATIVE error ~1e-15.  With t = e^x the integrand is entire in x and bounded in |Im x| < pi/2 by
// exp(nu (1 - cos y)) times its size on the axis: the trapezoidal rule with h = min(0.28, sqrt(0.57 / nu)) errs by < 1e-15
// (exp(-pi^2 / h), and exp(-2 pi^2 / (h^2 nu)) at the optimal shift for large nu).  It runs from where e^{nu x} has fallen to
// e^-36 below min(ln(s^2/4), -4) up to t = 2 nu + 50; a few hundred nodes of two exponentials and one expm1, for the table fit
// and for pairs outside the tables only.  (Below nu ~ 0.01 the node count is capped and the left tail is cut short.)
// Returns the partial sum over the nodes j_lo + lane, j_lo + lane + nlanes, ...: the table fit shares it among 64 lanes.
constexpr double kDnuSmallS = 0.25;
__host__ __device__ inline double matern_dnu_small_part(const double s, const MaternDerivConst &k, const int lane, const int nlanes)
{
    const double ln2 = 0.69314718055994530942;
    const double a = 0.25 * s * s, nu = k.nu, psi = k.lpsi - ln2, lg = (1.0 - nu) * ln2 - k.lnc;   // lg = lgamma(nu)
    const double h0 = sqrt(0.57 / nu), h = h0 < 0.28 ? h0 : 0.28;
    const double la = log(a), x_lo = (la < -4.0 ? la : -4.0) - 36.0 / nu, x_hi = log(2.0 * nu + 50.0);
    const int j_hi = (int)ceil(x_hi / h);
    const double jl = floor(x_lo / h);
    const int j_lo = (jl < (double)(j_hi - 20000)) ? j_hi - 20000 : (int)jl;
    double acc = 0.0;
    for (int j = j_lo + lane; j <= j_hi; j += nlanes) {
        const double x = (double)j * h, ex = exp(x);
        acc = __builtin_fma(exp(nu * x - ex - lg) * (x - psi), expm1(-a / ex), acc);
    }
    return h * acc;
}

// the three functions from the triple (0 < s); small_dnu: the smoothness derivative by matern_dnu_small_part, summed over its lanes
// (taken for s < kDnuSmallS)
__host__ __device__ inline void matern_derivs_from_triple(const double s, const MaternDerivConst &k, const int scaled,
                                                          const BesselTriple &b, const double small_dnu, double (&out)[3])
{
    const double ls = log(s);
    // E = c_nu 2^n s^mu [e^-s]
    const double E = exp(k.lnc + (double)b.n_up * 0.69314718055994530942 + b.mu * ls - (scaled ? 0.0 : s));
    out[0] = E * b.a_n;
    out[1] = (b.n_up == 0) ? E * s * b.a_m : E * (0.5 * s * s) * b.a_m;
    out[2] = (s < kDnuSmallS) ? (scaled ? small_dnu * exp(s) : small_dnu) : __builtin_fma(out[0], ls - k.lpsi, E * b.b_n);
}

// out = {C / sigma^2, (rho / sigma^2) dC/drho = c_nu s^{nu+1} K_{nu-1}(s), (1 / sigma^2) dC/dnu} at s = r / rho >= 0.
// scaled != 0: all three times e^s (what the per-launch tables hold).  s = 0: exactly {1, 0, 0}.  Where e^{-s} underflows all
// three are exact zeros (never 0 * Inf).
__host__ __device__ inline void matern_general_derivs(const double s, const MaternDerivConst &k, const int scaled, double (&out)[3])
{
    if (!(s > 0.0)) {
        out[0] = (s == 0.0) ? 1.0 : s;                              // (a NaN distance stays NaN)
        out[1] = (s == 0.0) ? 0.0 : s;
        out[2] = (s == 0.0) ? 0.0 : s;
        return;
    }
    if (!scaled && s > 745.0) {
        out[0] = out[1] = out[2] = 0.0;
        return;
    }
    const double small_dnu = (s < kDnuSmallS) ? matern_dnu_small_part(s, k, 0, 1) : 0.0;
    matern_derivs_from_triple(s, k, scaled, bessel_k_triple_scaled(k.nu, s), small_dnu, out);
}

// ---- per-launch tables of the three functions above, e^s-scaled, for the pair passes of the gradient and Fisher kernels ----
// Segments as MaternTab's mixed rows (eight per octave, degree 10, monomial basis in u), but ALL coefficients doubles and three
// functions per segment: a row is {a_0..a_10 of e^s f_0, of e^s f_1, of e^s f_2}, 33 doubles.  The rows are read from global
// memory, not gathered from LDS, so the 72-byte budget behind the FP32 tail of the value row does not apply, and its premise (a_0
// dominates the row to 2^-24 of the FP64 part) would have to be established for f_1 and f_2, which fall like s^min(2 nu, 2) ln s
// towards s = 0, before it could be used: all-double rows need no such argument.
// The device multiplies by exp(-s) (one exp per pair, what the closed forms pay); arguments outside the table take
// matern_general_derivs.  Fitted by gpv_matern_dtab_kernel (gpv_aux_kernels.hip).
struct MaternDTab {
    static constexpr int DEG = 10, N = DEG + 1, NF = 3, ROW = NF * N, LSPO = 3, SPO = 1 << LSPO;
    static constexpr int MAX_SEG = 80 * SPO;                                // 80 octaves
};
inline bool matern_dtab_range(double smin, double smax, int *e_lo_out, int *base_idx, int *nseg)
{
    constexpr int SPO = MaternDTab::SPO;
    *nseg = 0; *base_idx = 0; *e_lo_out = 0;
    if (!(smin > 0.0) || !(smax >= smin) || !std::isfinite(smax)) return false;
    int e_lo = (int)std::floor(std::log2(smin)), e_hi = (int)std::floor(std::log2(smax));
    if (e_lo < -200) e_lo = -200;
    if (e_hi > 8) e_hi = 8;                                                  // s < 512, as the value table
    if (e_hi < e_lo) return false;
    if ((e_hi - e_lo + 1) * SPO > MaternDTab::MAX_SEG) e_lo = e_hi + 1 - MaternDTab::MAX_SEG / SPO;
    *e_lo_out = e_lo;
    *base_idx = (e_lo + 1023) << MaternDTab::LSPO;
    *nseg = (e_hi - e_lo + 1) * SPO;
    return true;
}
__device__ __forceinline__ int matern_dtab_segment(const double s, const int base)
{
    return (int)(__double_as_longlong(s) >> (52 - MaternDTab::LSPO)) - base;
}
// u = 2 g - 3 with g the mantissa of s shifted left by LSPO bits under the exponent of 1.0 (matern_tab_poly)
__device__ __forceinline__ double matern_dtab_u(const double s)
{
    const unsigned lo = (unsigned)__double2loint(s), hi = (unsigned)__double2hiint(s);
    const unsigned ghi = (__builtin_amdgcn_alignbit(hi, lo, 32 - MaternDTab::LSPO) & 0x000FFFFFu) | 0x3FF00000u;
    return __builtin_fma(__hiloint2double((int)ghi, (int)(lo << MaternDTab::LSPO)), 2.0, -3.0);
}
__device__ __forceinline__ double matern_dtab_poly(const double *a, const double u)
{
    double p = a[MaternDTab::DEG];
#pragma unroll
    for (int k = MaternDTab::DEG - 1; k >= 0; --k) p = __builtin_fma(p, u, a[k]);
    return p;
}

}  // namespace gpv
