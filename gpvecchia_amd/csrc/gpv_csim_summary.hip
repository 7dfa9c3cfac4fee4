// gpv_csim_summary.hip — the folds of gpv_plan_cond_sim_summary, gfx950, FP64: summaries of the conditional draws of a
// cond.yz='z' model over a map, taken from each batch of 16 swept draws X[nq][16] (gpv_csim.hip) while it is on the device.
//
// The latent draw of location i and column c is y = mu_i + X[i][c], mu_i = mean_i + offset_i (two rounded adds; nothing here is
// contracted into an fma, so the host's (mean + offset) + dev has the same bits).  g: the link (0 identity, 1 exp, 2 logistic).
// A location is live when its mean is not NaN; the others take no part in anything.
//
// Geometry: that of the sweep, 16 lanes per row, lane c = column c, so a row of X is one 128-byte line per group of 16 lanes.
//   accumulate  one group per location: d = g(y) - g(mu) on the requested columns (exact zeros on the others), the 16 columns
//               meet in one fixed tree (xor offsets 8, 4, 2, 1), lane 0 adds into the running S1, S2; the counts of y > thr_t
//               are one ballot each.  Batches follow each other on one stream: ascending order.
//   fold        a region's member list is cut from its start into chunks of kCsumChunkRows entries; one group folds one chunk,
//               entry after entry in ascending order (kCsumStepRows entries are loaded together, then added one by one), each
//               lane its own column: total = sum w g(y), max and min of y, areas = sum w [y > thr_t], over the live members.  A
//               region of one chunk is finished there; the chunks of a longer one leave partials that a second launch joins in
//               ascending order, one group per region (it also writes the empty regions).  So 16 raster cells of ten pixels
//               share a workgroup, a region of 10^6 pixels is 7813 chunks, and a column's bits depend on the region's own
//               list and weights alone: not on the other regions, their number, the other columns or the grid.
//   finish      mc_mean = g(mu) + S1 / N, mc_var = (S2 - S1^2 / N) / (N - 1) clamped at 0, exceed = count / N; NaN where a
//               location is not live.
// No floating-point atomics and no atomics at all; no LDS; plain vector loads and stores; builtins only.
#include "gpv_csim_summary.h"

#include <cmath>

#pragma clang fp contract(off)

namespace gpv {

namespace {

template <int LINK>
__device__ __forceinline__ double csum_link(const double y)
{
    if constexpr (LINK == 1) return exp(y);
    else if constexpr (LINK == 2) return 1.0 / (1.0 + exp(-y));
    else return y;
}

__global__ void __launch_bounds__(kCsumThreads) gpv_csum_prepare_kernel(const double *__restrict__ mean, const double *__restrict__ offset,
                                                                        int64_t nq, double *__restrict__ mu, uint8_t *__restrict__ live)
{
    const int64_t i = (int64_t)blockIdx.x * kCsumThreads + threadIdx.x;
    if (i >= nq) return;
    const double m = mean[i];
    mu[i] = offset ? m + offset[i] : m;
    live[i] = m == m ? 1 : 0;
}

template <int LINK>
__global__ void __launch_bounds__(kCsumThreads) gpv_csum_accum_kernel(const CsumArgs A, const unsigned colmask)
{
    const int c = threadIdx.x & (kCsumCols - 1), lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kCsumGroups + (threadIdx.x >> 4);
    const bool row = i < A.nq;                         // (the others repeat the last row and write nothing: every lane of a
    const int64_t ii = row ? i : A.nq - 1;             //  wavefront reaches the cross-lane sums)
    const bool live = row && A.live[ii] != 0;
    const bool on = live && ((colmask >> c) & 1u);
    const double mu = A.mu[ii];
    const double y = mu + A.X[ii * kCsumCols + c];
    const double d = on ? csum_link<LINK>(y) - csum_link<LINK>(mu) : 0.0;
    double s1 = d, s2 = d * d;
#pragma unroll
    for (int off = kCsumCols / 2; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off, kCsumCols);
        s2 += __shfl_xor(s2, off, kCsumCols);
    }
    const int sh = lane & ~(kCsumCols - 1);
    uint32_t n[kCsumMaxThr];
#pragma unroll
    for (int t = 0; t < kCsumMaxThr; ++t) {
        n[t] = 0;
        if (t < A.nthr) n[t] = (uint32_t)__popcll((__ballot(on && y > A.thr[t]) >> sh) & 0xFFFFull);
    }
    if (live && c == 0) {
        A.S1[i] += s1;
        A.S2[i] += s2;
#pragma unroll
        for (int t = 0; t < kCsumMaxThr; ++t)
            if (t < A.nthr) A.cnt[(int64_t)t * A.nq + i] += n[t];
    }
}

// what a group holds of its column: the fold of some entries, and how two of them meet
struct CsumAcc {
    double tot, mx, mn, ar[kCsumMaxThr];
};

__device__ __forceinline__ void csum_acc_init(CsumAcc &a)
{
    a.tot = 0.0;
    a.mx = -INFINITY;
    a.mn = INFINITY;
#pragma unroll
    for (int t = 0; t < kCsumMaxThr; ++t) a.ar[t] = 0.0;
}

// the result of region `reg`, column c; no live member: max = min = NaN (then mx = -inf < mn = +inf, and only then)
__device__ __forceinline__ void csum_write_result(const CsumArgs &A, const CsumAcc &a, const int64_t reg, const int c)
{
    const bool none = a.mx < a.mn;
    const double nan = __builtin_nan("");
    A.rtot[(int64_t)c * A.nreg + reg] = a.tot;
    A.rmax[(int64_t)c * A.nreg + reg] = none ? nan : a.mx;
    A.rmin[(int64_t)c * A.nreg + reg] = none ? nan : a.mn;
#pragma unroll
    for (int t = 0; t < kCsumMaxThr; ++t)
        if (t < A.nthr) A.rarea[((int64_t)c * A.nthr + t) * A.nreg + reg] = a.ar[t];
}

template <int LINK>
__global__ void __launch_bounds__(kCsumThreads) gpv_csum_fold_kernel(const CsumArgs A)
{
    const int c = threadIdx.x & (kCsumCols - 1);
    const int64_t k = (int64_t)blockIdx.x * kCsumGroups + (threadIdx.x >> 4);
    if (k >= A.nchunks) return;                        // (nothing below crosses lanes)
    const CsumChunk ch = A.chunk[k];
    CsumAcc a;
    csum_acc_init(a);
    for (int e0 = 0; e0 < ch.len; e0 += kCsumStepRows) {
        double w[kCsumStepRows], y[kCsumStepRows];
        bool lv[kCsumStepRows];
#pragma unroll
        for (int s = 0; s < kCsumStepRows; ++s) {     // every load from an address that is always valid: the chunk's last entry
            const bool in = e0 + s < ch.len;
            const int64_t e = ch.beg + (in ? e0 + s : ch.len - 1);
            const int64_t i = A.regidx[e];
            w[s] = A.regw ? A.regw[e] : 1.0;
            lv[s] = in && A.live[i] != 0;
            y[s] = A.mu[i] + A.X[i * kCsumCols + c];
        }
#pragma unroll
        for (int s = 0; s < kCsumStepRows; ++s) {     // ascending; what does not count adds an exact zero
            const double ws = lv[s] ? w[s] : 0.0;
            const double gy = lv[s] ? csum_link<LINK>(y[s]) : 0.0;
            a.tot += ws * gy;
            a.mx = lv[s] ? fmax(a.mx, y[s]) : a.mx;
            a.mn = lv[s] ? fmin(a.mn, y[s]) : a.mn;
#pragma unroll
            for (int t = 0; t < kCsumMaxThr; ++t)
                if (t < A.nthr) a.ar[t] += (lv[s] && y[s] > A.thr[t]) ? w[s] : 0.0;
        }
    }
    if (ch.slot < 0) {
        csum_write_result(A, a, ch.reg, c);
        return;
    }
    double *const p = A.part + ch.slot * (int64_t)((3 + A.nthr) * kCsumCols) + c;
    p[0] = a.tot;
    p[kCsumCols] = a.mx;
    p[2 * kCsumCols] = a.mn;
#pragma unroll
    for (int t = 0; t < kCsumMaxThr; ++t)
        if (t < A.nthr) p[(3 + t) * kCsumCols] = a.ar[t];
}

__global__ void __launch_bounds__(kCsumThreads) gpv_csum_join_kernel(const CsumArgs A)
{
    const int c = threadIdx.x & (kCsumCols - 1);
    const int64_t k = (int64_t)blockIdx.x * kCsumGroups + (threadIdx.x >> 4);
    if (k >= A.njoin) return;
    const CsumJoin j = A.join[k];
    const int64_t stride = (int64_t)(3 + A.nthr) * kCsumCols;
    CsumAcc a;
    csum_acc_init(a);
    const double *p = A.part + j.slot0 * stride + c;
#pragma unroll 4
    for (int s = 0; s < j.nslots; ++s, p += stride) {  // ascending
        a.tot += p[0];
        a.mx = fmax(a.mx, p[kCsumCols]);
        a.mn = fmin(a.mn, p[2 * kCsumCols]);
#pragma unroll
        for (int t = 0; t < kCsumMaxThr; ++t)
            if (t < A.nthr) a.ar[t] += p[(3 + t) * kCsumCols];
    }
    csum_write_result(A, a, j.reg, c);
}

__global__ void __launch_bounds__(kCsumThreads) gpv_csum_finish_kernel(const CsumArgs A, const int link, const double N, double *out)
{
    const int64_t i = (int64_t)blockIdx.x * kCsumThreads + threadIdx.x;
    if (i >= A.nq) return;
    const bool live = A.live[i] != 0;
    const double nan = __builtin_nan("");
    const double m = A.mu[i], s1 = A.S1[i], s2 = A.S2[i];
    const double gm = link == 1 ? csum_link<1>(m) : (link == 2 ? csum_link<2>(m) : m);
    const double v = (s2 - s1 * s1 / N) / (N - 1.0);
    out[i] = live ? m : nan;
    out[A.nq + i] = live ? gm + s1 / N : nan;
    out[2 * A.nq + i] = live ? (v > 0.0 ? v : 0.0) : nan;
#pragma unroll
    for (int t = 0; t < kCsumMaxThr; ++t)
        if (t < A.nthr) out[(int64_t)(3 + t) * A.nq + i] = live ? (double)A.cnt[(int64_t)t * A.nq + i] / N : nan;
}

bool csum_blocks(int64_t items, int per_block, unsigned &blocks)
{
    const int64_t b = (items + per_block - 1) / per_block;
    if (items < 1 || b > 0x7FFFFFFF) return false;
    blocks = (unsigned)b;
    return true;
}

bool csum_args_ok(const CsumArgs &a, int link)
{
    return a.nq >= 1 && a.nthr >= 0 && a.nthr <= kCsumMaxThr && link >= 0 && link <= 2 && a.X && a.mu && a.live;
}

}  // namespace

hipError_t launch_csum_prepare(const double *mean, const double *offset, int64_t nq, double *mu, uint8_t *live, hipStream_t s)
{
    unsigned blocks = 0;
    if (!mean || !mu || !live || !csum_blocks(nq, kCsumThreads, blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_csum_prepare_kernel, dim3(blocks), dim3(kCsumThreads), 0, s, mean, offset, nq, mu, live);
    return hipGetLastError();
}

hipError_t launch_csum_accum(const CsumArgs &a, int link, unsigned colmask, hipStream_t s)
{
    unsigned blocks = 0;
    if (!csum_args_ok(a, link) || !a.S1 || !a.S2 || (a.nthr > 0 && !a.cnt) || colmask == 0 || colmask > 0xFFFFu ||
        !csum_blocks(a.nq, kCsumGroups, blocks))
        return hipErrorInvalidValue;
    const dim3 g(blocks), b(kCsumThreads);
    if (link == 0) hipLaunchKernelGGL(gpv_csum_accum_kernel<0>, g, b, 0, s, a, colmask);
    else if (link == 1) hipLaunchKernelGGL(gpv_csum_accum_kernel<1>, g, b, 0, s, a, colmask);
    else hipLaunchKernelGGL(gpv_csum_accum_kernel<2>, g, b, 0, s, a, colmask);
    return hipGetLastError();
}

hipError_t launch_csum_fold(const CsumArgs &a, int link, hipStream_t s)
{
    if (!csum_args_ok(a, link) || a.nreg < 1 || a.nchunks < 0 || a.njoin < 0 || !a.rtot || !a.rmax || !a.rmin || (a.nthr > 0 && !a.rarea))
        return hipErrorInvalidValue;
    if (a.nchunks > 0) {
        unsigned blocks = 0;
        if (!a.chunk || !a.regidx || !csum_blocks(a.nchunks, kCsumGroups, blocks)) return hipErrorInvalidValue;
        const dim3 g(blocks), b(kCsumThreads);
        if (link == 0) hipLaunchKernelGGL(gpv_csum_fold_kernel<0>, g, b, 0, s, a);
        else if (link == 1) hipLaunchKernelGGL(gpv_csum_fold_kernel<1>, g, b, 0, s, a);
        else hipLaunchKernelGGL(gpv_csum_fold_kernel<2>, g, b, 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.njoin > 0) {
        unsigned blocks = 0;
        if (!a.join || !a.part || !csum_blocks(a.njoin, kCsumGroups, blocks)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(gpv_csum_join_kernel, dim3(blocks), dim3(kCsumThreads), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_csum_finish(const CsumArgs &a, int link, int64_t ndraws, double *out, hipStream_t s)
{
    unsigned blocks = 0;
    if (!csum_args_ok(a, link) || !a.S1 || !a.S2 || (a.nthr > 0 && !a.cnt) || ndraws < 2 || !out || !csum_blocks(a.nq, kCsumThreads, blocks))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_csum_finish_kernel, dim3(blocks), dim3(kCsumThreads), 0, s, a, link, (double)ndraws, out);
    return hipGetLastError();
}

}  // namespace gpv
