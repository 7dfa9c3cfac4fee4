// gpv_whiten.hip — the Vecchia whitening operator of an evaluation applied to a block of columns, and their Gram matrix (gfx950).
//
// For row k of a cond.yz = 'z' plan with stored U entries L_kj (j in J_k), own entry d_k and nugget tau_k, column b whitens to
//     e_k(b) = (b_k + (sum_j L_kj b_j) / d_k) / sqrt(tau_k + 1/d_k^2),        logdet = sum_k log(tau_k + 1/d_k^2):
// the standardised conditional residual of z_k given its neighbours' z under C + tau I, the density sums[2] / sums[3] describe.
// The factor is already in HBM (GPV_WANT_U), so this is a streaming pass over Lentries and the neighbour indices plus a gather
// of the columns, not a second factorisation.
//
// Whitening pass.  16 lanes per set, laid out as (16 / CP neighbour slots) x (CP columns), CP = padded column count: the CP
// values of one neighbour are contiguous (B is row-major by internal position), so a 16-lane group reads 16 / CP neighbours'
// rows per instruction and a wavefront 64 / CP.  Any row length goes through the one loop; nothing is instantiated per P.
// Gram pass.  G = E^T E with plain FMAs out of LDS, one 16 x 16 tile entry per thread: the pass moves 8 CP bytes per row and
// does CP^2 FMAs on them, far below the FP64 rate, so the matrix pipe would buy nothing.  Per-workgroup tiles, then one
// workgroup adds them in workgroup order: no tickets, no spinning, the same bits every call.  a * b == b * a in IEEE
// arithmetic and both triangles accumulate in the same order, so G is exactly symmetric.
#include "gpv_whiten.h"

namespace gpv {
namespace {

__global__ void __launch_bounds__(256) gpv_whiten_pack_kernel(const double *__restrict__ in, const int32_t *__restrict__ newpos,
                                                              int64_t n, int ncols, int cp, double *__restrict__ B)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * cp) return;
    const int64_t i = t / cp;
    const int c = (int)(t - i * cp);
    B[(int64_t)newpos[i] * cp + c] = c < ncols ? in[(int64_t)c * n + i] : 0.0;
}

__global__ void __launch_bounds__(256) gpv_whiten_unpack_kernel(const double *__restrict__ E, int64_t n, int ncols, int cp,
                                                                double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * ncols) return;
    const int64_t c = t / n, i = t - c * n;
    out[t] = E[i * cp + c];
}

template <int CP>
__global__ void __launch_bounds__(kWhitenThreads) gpv_whiten_kernel(const WhitenArgs A)
{
    constexpr int NS = kWhitenLanes / CP;              // neighbour slots of a set's 16 lanes
    __shared__ double s_part[kWhitenThreads / 64][kWhitenNV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> 4, lig = lane & 15;
    const int c = lig & (CP - 1), sl = lig / CP;
    const int P = A.P;
    double ld = 0.0, nf = 0.0;                         // (kept by the first lane of every group)
    const int64_t stride = (int64_t)gridDim.x * kWhitenSetsPerBlock;
    // the trip count is the same for a whole wavefront: the cross-lane sums below always see all 64 lanes
    for (int64_t s0 = (int64_t)blockIdx.x * kWhitenSetsPerBlock + wave * 4; s0 < A.rows; s0 += stride) {
        const bool on = s0 + grp < A.rows;
        const int64_t s = on ? s0 + grp : A.rows - 1;
        const int32_t *const nr = A.nn + s * P;
        // the row's own point first: its three reads depend on nothing below and overlap the count and the gathers
        const int32_t own = nr[P - 1];
        const bool have = own >= 0;
        const double bk = have ? A.B[(int64_t)own * CP + c] : 0.0;
        const double tau = have ? (A.nuggets != nullptr ? A.nuggets[own] : A.nug_scalar) : 0.0;
        int miss = 0;                                  // missing entries stand in front
        for (int q = lig; q < P; q += kWhitenLanes) miss += nr[q] < 0 ? 1 : 0;
#pragma unroll
        for (int off = 1; off < kWhitenLanes; off <<= 1) miss += __shfl_xor(miss, off, kWhitenLanes);
        const int n0 = P - miss;
        const int64_t kout = A.rowid[s];
        const double *const lr = A.L + kout * P;
        double acc = 0.0;
#pragma unroll 4
        for (int t = sl; t < n0 - 1; t += NS) {
            const int32_t idx = nr[miss + t];
            const double l = lr[t];
            const double b = idx >= 0 ? A.B[(int64_t)idx * CP + c] : 0.0;
            acc = __builtin_fma(l, b, acc);
        }
#pragma unroll
        for (int off = CP; off < kWhitenLanes; off <<= 1) acc += __shfl_xor(acc, off, kWhitenLanes);
        const double d = have ? lr[n0 - 1] : 0.0;      // (own >= 0: n0 >= 1)
        const bool fail = !(d > 0.0);                  // a block that was not positive definite left its row of U at zero
        const double sv = tau + 1.0 / (d * d);
        const double e = fail ? __builtin_nan("") : (bk + acc / d) / sqrt(sv);
        if (on && sl == 0) A.E[kout * CP + c] = e;
        if (on && lig == 0) {
            if (fail) nf += 1.0;
            else ld += log(sv);
        }
    }
    // ---- per-workgroup partials: groups in lane order, wavefronts in wavefront order
    double wl = 0.0, wf = 0.0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        wl += __shfl(ld, g * kWhitenLanes);
        wf += __shfl(nf, g * kWhitenLanes);
    }
    if (lane == 0) {
        s_part[wave][0] = wl;
        s_part[wave][1] = wf;
    }
    __syncthreads();
    if (threadIdx.x < kWhitenNV) {
        double sum = 0.0;
        for (int wv = 0; wv < kWhitenThreads / 64; ++wv) sum += s_part[wv][threadIdx.x];
        A.part[(int64_t)blockIdx.x * kWhitenNV + threadIdx.x] = sum;
    }
}

// partial tile of workgroup b over its contiguous rows; entry (i, j) of the 16 x 16 tile belongs to thread 16 i + j
template <int CP>
__global__ void __launch_bounds__(kGramThreads) gpv_whiten_gram_kernel(const double *__restrict__ E, int64_t n, double *gpart)
{
    __shared__ double tile[kGramRows * CP];
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    const bool act = i < CP && j < CP;                 // the columns >= CP of the zero-padded E contribute zeros
    const int64_t chunk = ((n + gridDim.x - 1) / gridDim.x + kGramRows - 1) / kGramRows * kGramRows;
    const int64_t r0 = (int64_t)blockIdx.x * chunk;
    const int64_t r1 = r0 + chunk < n ? r0 + chunk : n;
    double acc = 0.0;
    for (int64_t r = r0; r < r1; r += kGramRows) {
        const int64_t left = (r1 - r) * CP;            // doubles of E from row r to the end of the chunk
        for (int t = threadIdx.x; t < kGramRows * CP; t += kGramThreads) tile[t] = t < left ? E[r * CP + t] : 0.0;
        __syncthreads();
        if (act) {
#pragma unroll 8
            for (int q = 0; q < kGramRows; ++q) acc = __builtin_fma(tile[q * CP + i], tile[q * CP + j], acc);
        }
        __syncthreads();
    }
    gpart[(int64_t)blockIdx.x * kGramTile + threadIdx.x] = acc;
}

// totals: the tiles added in workgroup order (threads 0 .. 255, one entry each); the whitening pass's partials added in
// workgroup order inside 256 contiguous segments, then the segments in order (threads 256 .. 511)
__global__ void __launch_bounds__(512) gpv_whiten_total_kernel(const double *__restrict__ gpart, int ggrid,
                                                               const double *__restrict__ wpart, int wgrid, double *totals)
{
    __shared__ double seg[256][kWhitenNV];
    const int t = threadIdx.x;
    if (t < kGramTile) {
        double s = 0.0;
#pragma unroll 16
        for (int b = 0; b < ggrid; ++b) s += gpart[(int64_t)b * kGramTile + t];
        totals[t] = s;
    } else {
        const int w = t - kGramTile;
        const int per = (wgrid + 255) / 256;
        const int b0 = w * per, b1 = b0 + per < wgrid ? b0 + per : wgrid;
        double a = 0.0, f = 0.0;
        for (int b = b0; b < b1; ++b) {
            a += wpart[(int64_t)b * kWhitenNV];
            f += wpart[(int64_t)b * kWhitenNV + 1];
        }
        seg[w][0] = a;
        seg[w][1] = f;
    }
    __syncthreads();
    if (t >= kGramTile && t < kGramTile + kWhitenNV) {
        const int v = t - kGramTile;
        double s = 0.0;
        for (int w = 0; w < 256; ++w) s += seg[w][v];
        totals[kGramTile + v] = s;
    }
}

}  // namespace

int whiten_grid(int64_t rows, int cus)
{
    int64_t grid = (rows + kWhitenSetsPerBlock - 1) / kWhitenSetsPerBlock;
    const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * kWhitenBlocksPerCU;
    if (grid > cap) grid = cap;
    return (int)(grid < 1 ? 1 : grid);
}

int whiten_gram_grid(int64_t rows, int cus)
{
    int64_t grid = (rows + kGramRows - 1) / kGramRows;
    const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * kGramBlocksPerCU;
    if (grid > cap) grid = cap;
    return (int)(grid < 1 ? 1 : grid);
}

static bool whiten_cp_ok(int ncols, int cp) { return ncols >= 1 && ncols <= cp && cp <= kWhitenMaxCols && (cp & (cp - 1)) == 0; }

hipError_t launch_whiten_pack(const double *in, const int32_t *newpos, int64_t n, int ncols, int cp, double *B, hipStream_t s)
{
    if (n < 1 || !whiten_cp_ok(ncols, cp)) return hipErrorInvalidValue;
    const int64_t blocks = (n * cp + 255) / 256;
    hipLaunchKernelGGL(gpv_whiten_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, newpos, n, ncols, cp, B);
    return hipGetLastError();
}

hipError_t launch_whiten_unpack(const double *E, int64_t n, int ncols, int cp, double *out, hipStream_t s)
{
    if (n < 1 || !whiten_cp_ok(ncols, cp)) return hipErrorInvalidValue;
    const int64_t blocks = (n * ncols + 255) / 256;
    hipLaunchKernelGGL(gpv_whiten_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, E, n, ncols, cp, out);
    return hipGetLastError();
}

hipError_t launch_whiten(const WhitenArgs &a, int cp, int grid, hipStream_t s)
{
    if (grid < 1 || a.rows < 1 || a.P < 1) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(kWhitenThreads);
    switch (cp) {
        case 1: hipLaunchKernelGGL(gpv_whiten_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(gpv_whiten_kernel<2>, g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL(gpv_whiten_kernel<4>, g, b, 0, s, a); break;
        case 8: hipLaunchKernelGGL(gpv_whiten_kernel<8>, g, b, 0, s, a); break;
        case 16: hipLaunchKernelGGL(gpv_whiten_kernel<16>, g, b, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_whiten_gram(const double *E, int64_t n, int cp, int ggrid, double *gpart, const double *wpart, int wgrid,
                              double *totals, hipStream_t s)
{
    if (ggrid < 1 || wgrid < 1 || n < 1) return hipErrorInvalidValue;
    const dim3 g((unsigned)ggrid), b(kGramThreads);
    switch (cp) {
        case 1: hipLaunchKernelGGL(gpv_whiten_gram_kernel<1>, g, b, 0, s, E, n, gpart); break;
        case 2: hipLaunchKernelGGL(gpv_whiten_gram_kernel<2>, g, b, 0, s, E, n, gpart); break;
        case 4: hipLaunchKernelGGL(gpv_whiten_gram_kernel<4>, g, b, 0, s, E, n, gpart); break;
        case 8: hipLaunchKernelGGL(gpv_whiten_gram_kernel<8>, g, b, 0, s, E, n, gpart); break;
        case 16: hipLaunchKernelGGL(gpv_whiten_gram_kernel<16>, g, b, 0, s, E, n, gpart); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gpv_whiten_total_kernel, dim3(1), dim3(512), 0, s, gpart, ggrid, wpart, wgrid, totals);
    return hipGetLastError();
}

}  // namespace gpv
