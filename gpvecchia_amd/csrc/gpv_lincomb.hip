// gpv_lincomb.hip — Var(H y | z) = || R^-1 h ||^2 for many right-hand sides at once (R/vecchia_prediction.R:164-178,
// vecchia_lincomb; :223-244, the var.exact path of vecchia_var).
//
// W = R R^T with R upper triangular on the pattern of the latent block (gpv_posterior.hip), so h' W^-1 h = |x|^2 with
// R x = h: the solve the factor pass performs for ONE right-hand side while it factorises, here on its own, after the factor
// is complete, for kLincombNB right-hand sides interleaved as X[Nlocs][NB]:
//     x_k[j] = (h_k[j] - sum_{c > k, k in col c} R_kc x_c[j]) / R_kk ,      R_kc = C[cb_c + 1 + e_k].y .
// Same level schedule as the factor pass (column k waits for every column c > k that contains row k), one launch per level.
// A gathered x_c is a contiguous run of NB doubles used in full (the scalar sweeps use 8 or 16 bytes of every 128-byte line),
// and one pass over the records and the R values serves NB solves.
//
// One wavefront per column: the 64 lanes first fetch 64 row-list records and their R_kc in one coalesced trip each, then the
// lanes (NB right-hand sides x 64/NB slices of the chunk) walk the chunk with the record and the value broadcast from the
// lane that fetched them.  Every partial sum has a fixed order (slice: ascending entries; slices and waves: fixed trees) =>
// bitwise reproducible.  No floating-point atomics.
//
// Further down: the TRANSPOSED solve R^T X = E on the same buffer and batching (posterior draws, gpv_plan_solve_t), and the
// Monte-Carlo summaries of such draws with normals made on the device (gpv_plan_draws_summary).
#include "gpv_internal.h"
#include "gpv_posterior_ext.h"
#include "gpv_philox.hpp"
#include <atomic>

namespace gpv {

constexpr int NB = kLincombNB, kLcS = 64 / NB;          // right-hand sides per batch, slices of a chunk
static_assert(NB == 16 || NB == 32, "batch width");

// X <- 0, then X[idx][j] (+)= val over the CSR rows [row0, row0 + nb) of H: row j of the batch is column j of X
__global__ void __launch_bounds__(256) gpv_lincomb_zero_kernel(double *X, int64_t total)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) X[i] = 0.0;
}
// rows without a repeated index: one store per entry, blockIdx.y = row of the batch
__global__ void __launch_bounds__(256) gpv_lincomb_scatter_kernel(double *X, const int64_t *hptr, const int32_t *hidx,
                                                                  const double *hval, int64_t row0)
{
    const int j = blockIdx.y;
    const int64_t b = hptr[row0 + j], e = hptr[row0 + j + 1];
    for (int64_t q = b + (int64_t)blockIdx.x * 256 + threadIdx.x; q < e; q += (int64_t)gridDim.x * 256)
        X[(int64_t)hidx[q] * NB + j] = hval[q];
}
// any rows: one thread per row walks its entries in the order given (duplicates add in that order)
__global__ void __launch_bounds__(64) gpv_lincomb_scatter_serial_kernel(double *X, const int64_t *hptr, const int32_t *hidx,
                                                                        const double *hval, int64_t row0, int nb)
{
    const int j = threadIdx.x;
    if (j >= nb) return;
    for (int64_t q = hptr[row0 + j]; q < hptr[row0 + j + 1]; ++q) X[(int64_t)hidx[q] * NB + j] += hval[q];
}
hipError_t launch_lincomb_init(double *X, int64_t n, const int64_t *hptr, const int32_t *hidx, const double *hval, int64_t row0,
                               int nb, int64_t max_row_nnz, bool serial, hipStream_t s)
{
    if (n <= 0 || nb <= 0 || nb > NB) return hipErrorInvalidValue;
    const int64_t total = n * NB;
    const int zg = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(gpv_lincomb_zero_kernel, dim3(zg), dim3(256), 0, s, X, total);
    if (serial) {
        hipLaunchKernelGGL(gpv_lincomb_scatter_serial_kernel, dim3(1), dim3(64), 0, s, X, hptr, hidx, hval, row0, nb);
    } else if (max_row_nnz > 0) {
        const int gx = (int)((max_row_nnz + 255) / 256 < 256 ? (max_row_nnz + 255) / 256 : 256);
        hipLaunchKernelGGL(gpv_lincomb_scatter_kernel, dim3(gx, nb), dim3(256), 0, s, X, hptr, hidx, hval, row0);
    }
    return hipGetLastError();
}

__device__ __forceinline__ double lc_shfl(const double v, const int l)
{
    const int lo = __builtin_amdgcn_ds_bpermute(l << 2, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(l << 2, __double2hiint(v));
    return __hiloint2double(hi, lo);
}

// One column of the solve.  WPC = waves that share the column (hub rows with row lists of hundreds to thousands of entries
// in the narrow late levels: the 64-entry chunks are dealt round-robin to the waves, the partial sums meet in LDS in wave
// order).  MODE 1 (the columns of the dense top block): the row-list entries whose column is in the block (record .x < 0)
// are left to gpv_lincomb_top_kernel, and X_k <- h_k - (the other terms), undivided.
template <int WPC, int MODE>
__global__ void __launch_bounds__(WPC == 1 ? 256 : 64 * WPC) gpv_lincomb_level_kernel(const LincombArgs A, const int first,
                                                                                     const int count)
{
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int w = (WPC == 1) ? (int)(blockIdx.x * (blockDim.x >> 6)) + wib : (int)blockIdx.x;
    if (w >= count) return;                                   // (WPC > 1: never, the grid is the level)
    const int4 c0 = A.colrec[2 * (size_t)(first + w)];
    const int4 c1 = A.colrec[2 * (size_t)(first + w) + 1];
    const int k = c0.x, cnt = c0.z;
    const int qb = c0.w + 1, qe = c1.x;                       // row list of k without its first pair, the column itself
    const int j = lane & (NB - 1), sl = lane / NB;
    // the epilogue's operands leave with the first chunk's records
    const double hk = A.X[(size_t)k * NB + j];
    const double rkk = A.C[(size_t)c0.y + cnt].y;             // the diagonal: last entry of the column's block
    double acc = 0.0;
    for (int base = qb + ((WPC == 1) ? 0 : 64 * wib); base < qe; base += 64 * WPC) {
        const int q = base + lane;
        int cc = k;                                           // (a lane without a pair points at the column itself: a valid row)
        double rv = 0.0;
        if (q < qe) {
            const int2 r = A.lrec[q];
            const double v = A.C[r.y].y;
            if (MODE == 1 && r.x < 0) { cc = k; rv = 0.0; }
            else { cc = r.x; rv = v; }
        }
        const int m = (qe - base < 64) ? qe - base : 64;      // pairs of this chunk (wave uniform)
        for (int t = 0; t < m; t += 4 * kLcS) {
            double x[4], r[4];
            bool on[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = t + u * kLcS + sl;
                const int ee = e < 64 ? e : 63;
                on[u] = e < m;
                const int c = __builtin_amdgcn_ds_bpermute(ee << 2, cc);
                r[u] = lc_shfl(rv, ee);
                x[u] = A.X[(size_t)c * NB + j];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = on[u] ? __builtin_fma(r[u], x[u], acc) : acc;
        }
    }
    if constexpr (WPC > 1) {
        __shared__ double part[WPC][64];
        part[wib][lane] = acc;
        __syncthreads();
        if (wib != 0) return;
        acc = 0.0;
#pragma unroll
        for (int v = 0; v < WPC; ++v) acc += part[v][lane];
    }
    // the slices of a right-hand side: butterflies (a + b == b + a: every lane of a right-hand side ends with the same bits)
#pragma unroll
    for (int off = NB; off < 64; off <<= 1) acc += lc_shfl(acc, lane ^ off);
    if (lane < NB) A.X[(size_t)k * NB + j] = (MODE == 1) ? hk - acc : (hk - acc) / rkk;
}

hipError_t launch_lincomb_level(const LincombArgs &a, int first, int count, bool leaves, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    if (!leaves && count <= kLincombWide16) {
        hipLaunchKernelGGL((gpv_lincomb_level_kernel<16, 0>), dim3(count), dim3(1024), 0, s, a, first, count);
    } else if (!leaves && count <= kLincombWide8) {
        hipLaunchKernelGGL((gpv_lincomb_level_kernel<8, 0>), dim3(count), dim3(512), 0, s, a, first, count);
    } else {
        hipLaunchKernelGGL((gpv_lincomb_level_kernel<1, 0>), dim3((count + 3) / 4), dim3(256), 0, s, a, first, count);
    }
    return hipGetLastError();
}

// The dense top block (gpv_posterior_ext.h): K <= 128 columns that wait for everything and for each other.  After
// gpv_lincomb_level_kernel<16, 1> has taken the terms of the columns outside the block, ONE workgroup solves
// R_TT x_T = rhs_T by back substitution, last column first: R_TT in LDS (zero off the pattern), thread (g, j) keeps the
// right-hand side j of the rows g, g + G, .. in registers; per step the owner of row c publishes x_c[j] and every thread
// subtracts R_rc x_c[j] from its rows r < c.  A fixed order per entry => reproducible.
constexpr int kLcTop = kTopMax, kLcTopLd = kLcTop + 1;
constexpr int kLcTopG = 1024 / NB, kLcTopRows = kLcTop / kLcTopG;          // row groups, rows per thread
constexpr size_t kLcTopSmem = ((size_t)kLcTop * kLcTopLd + 2 * NB) * sizeof(double);
__global__ void __launch_bounds__(1024) gpv_lincomb_top_kernel(const LincombArgs A, const int K, const int2 *topinfo,
                                                              const uint8_t *toprows)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lctop_smem[];
    double *Rl = reinterpret_cast<double *>(lctop_smem);       // [row][column], rows kLcTopLd apart
    double *xc = Rl + (size_t)kLcTop * kLcTopLd;               // [2][NB]: x_c of the step, double buffered
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < kLcTop * kLcTopLd; i += 1024) Rl[i] = 0.0;
    __syncthreads();
    if (tid < kLcTop && tid >= K) Rl[tid * kLcTopLd + tid] = 1.0;
    for (int kk = wave; kk < K; kk += 16) {                    // column kk of the block: entry e (lane) sits in row toprows[kk][e]
        const int r = (int)toprows[kTopBlock * kk + lane];
        if (r != 0xFF) Rl[r * kLcTopLd + kk] = A.C[(size_t)topinfo[kk].y + 1 + lane].y;
    }
    const int j = tid & (NB - 1), g = tid / NB;
    double reg[kLcTopRows];
    int kcol[kLcTopRows];
#pragma unroll
    for (int r = 0; r < kLcTopRows; ++r) {
        const int row = g + r * kLcTopG;
        kcol[r] = row < K ? topinfo[row].x : -1;
        reg[r] = row < K ? A.X[(size_t)kcol[r] * NB + j] : 0.0;
    }
    __syncthreads();
    for (int c = K - 1; c >= 0; --c) {
        double *xb = xc + (c & 1) * NB;
        if (g == c % kLcTopG) {
            const double d = Rl[c * kLcTopLd + c];
#pragma unroll
            for (int r = 0; r < kLcTopRows; ++r)
                if (r == c / kLcTopG) { reg[r] = reg[r] / d; xb[j] = reg[r]; }
        }
        __syncthreads();
        const double xv = xb[j];
#pragma unroll
        for (int r = 0; r < kLcTopRows; ++r) {
            const int row = g + r * kLcTopG;
            if (row < c) reg[r] = __builtin_fma(-Rl[row * kLcTopLd + c], xv, reg[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < kLcTopRows; ++r)
        if (kcol[r] >= 0) A.X[(size_t)kcol[r] * NB + j] = reg[r];
}

hipError_t launch_lincomb_top(const LincombArgs &a, int first, int K, const int2 *topinfo, const uint8_t *toprows, hipStream_t s)
{
    if (K <= 0) return hipSuccess;
    if (K > kLcTop) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> done{0ull};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_relaxed) & bit)) {
        hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(&gpv_lincomb_top_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLcTopSmem);
        if (e1 != hipSuccess) return e1;
        done.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL((gpv_lincomb_level_kernel<16, 1>), dim3(K), dim3(1024), 0, s, a, first, K);
    hipLaunchKernelGGL(gpv_lincomb_top_kernel, dim3(1), dim3(1024), kLcTopSmem, s, a, K, topinfo, toprows);
    return hipGetLastError();
}

// ---- deterministic reductions: vars[j] = sum_k X[k][j]^2, G[i][j] = sum_k X[k][i] X[k][j] -------------------------------
// Fixed block partials (block b takes the rows b, b + kLincombBlocks, ..), then their sum in block order.  GRAM = false is
// the diagonal of GRAM = true computed by the same operations in the same order: diag(G) == vars bit for bit.
template <bool GRAM>
__global__ void __launch_bounds__(GRAM ? NB * NB : NB) gpv_lincomb_sq_stage1(const double *X, int64_t n, double *partials)
{
    const int j = threadIdx.x & (NB - 1), i = GRAM ? (int)(threadIdx.x / NB) : j;
    double acc = 0.0;
    for (int64_t k = blockIdx.x; k < n; k += gridDim.x) acc = __builtin_fma(X[k * NB + i], X[k * NB + j], acc);
    partials[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = acc;
}
template <bool GRAM>
__global__ void __launch_bounds__(GRAM ? NB * NB : NB) gpv_lincomb_sq_stage2(const double *partials, int nb, double *out)
{
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc += partials[(size_t)b * blockDim.x + threadIdx.x];
    out[threadIdx.x] = acc;
}
hipError_t launch_lincomb_vars(const double *X, int64_t n, double *partials, double *vars, hipStream_t s)
{
    hipLaunchKernelGGL((gpv_lincomb_sq_stage1<false>), dim3(kLincombBlocks), dim3(NB), 0, s, X, n, partials);
    hipLaunchKernelGGL((gpv_lincomb_sq_stage2<false>), dim3(1), dim3(NB), 0, s, (const double *)partials, kLincombBlocks, vars);
    return hipGetLastError();
}
hipError_t launch_lincomb_gram(const double *X, int64_t n, double *partials, double *gram, hipStream_t s)
{
    hipLaunchKernelGGL((gpv_lincomb_sq_stage1<true>), dim3(kLincombBlocks), dim3(NB * NB), 0, s, X, n, partials);
    hipLaunchKernelGGL((gpv_lincomb_sq_stage2<true>), dim3(1), dim3(NB * NB), 0, s, (const double *)partials, kLincombBlocks, gram);
    return hipGetLastError();
}

// ---- the transposed solve R^T X = E (posterior draws: e ~ N(0, I) => x = R^-T e has covariance W^-1) ------------------------
//     x_k[j] = (e_k[j] - sum_{c < k, c in col k} R_ck x_c[j]) / R_kk ,      R_ck = C[cb_k + 1 + l].y, l = position of c in col k.
// The gather form of the sweep above: column k reads ITS OWN entries (the rows crow[..] of the column, the self entry last),
// which is the recurrence of the scalar mean sweep (gpv_posterior.hip, gpv_mean_level_rec_kernel) for NB right-hand sides, on
// that sweep's ascending schedule (meanrec / levptr2), one launch per level, the dense top block first.
//
// One wavefront per column.  A column has at most 64 entries, so the lanes fetch its rows and R values in ONE coalesced trip;
// then the lanes (NB right-hand sides x kLcS slices) walk the entries, row and value broadcast from the lane that fetched
// them; a gathered x_c[0..NB) is one contiguous run.  A slice adds its entries in ascending order, the slices meet in slice
// order, every lane of a right-hand side executes the same operations whatever its j => bitwise reproducible, and a column
// of E gives the same bits at every position of its batch.
__global__ void __launch_bounds__(256) gpv_solvet_level_kernel(const SolveTArgs A, const int first, const int count)
{
    const int lane = threadIdx.x & 63;
    const int w = (int)(blockIdx.x * 4) + (int)(threadIdx.x >> 6);
    if (w >= count) return;
    const int4 rec = A.meanrec[first + w];
    const int k = rec.x, cnt = rec.z;
    const int j = lane & (NB - 1), sl = lane / NB;
    const double ek = A.X[(size_t)k * NB + j];
    int cc = k;                                               // (a lane without an entry points at the column itself: a valid row)
    double rv = 0.0;
    if (lane < cnt) {
        cc = A.crow[rec.w + lane];
        rv = A.C[(size_t)rec.y + 1 + lane].y;
    }
    const double rkk = lc_shfl(rv, cnt - 1);                  // the diagonal: last entry of the column
    const int m = cnt - 1;
    double acc = 0.0;
    for (int t = 0; t < m; t += 4 * kLcS) {
        double x[4], r[4];
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = t + u * kLcS + sl;
            const int ee = e < 64 ? e : 63;
            on[u] = e < m;
            const int c = __builtin_amdgcn_ds_bpermute(ee << 2, cc);
            r[u] = lc_shfl(rv, ee);
            x[u] = A.X[(size_t)c * NB + j];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = on[u] ? __builtin_fma(r[u], x[u], acc) : acc;
    }
    double tot = lc_shfl(acc, j);
#pragma unroll
    for (int s = 1; s < kLcS; ++s) tot += lc_shfl(acc, j + s * NB);
    if (lane < NB) A.X[(size_t)k * NB + j] = (ek - tot) / rkk;
}

hipError_t launch_solvet_level(const SolveTArgs &a, int first, int count, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(gpv_solvet_level_kernel, dim3((count + 3) / 4), dim3(256), 0, s, a, first, count);
    return hipGetLastError();
}

// The dense top block, FIRST here: the rows of a column of T are in T, so R_TT^T x_T = e_T is a forward substitution of its own.
// The layout of gpv_lincomb_top_kernel (R_TT in LDS, thread (g, j) keeps the right-hand side j of the columns g, g + G, ..),
// walked from the first column: the owner of column c publishes x_c[j], every thread subtracts R_c,cc x_c[j] from its columns
// cc > c (row c of R: consecutive words for consecutive g).
__global__ void __launch_bounds__(1024) gpv_solvet_top_kernel(const SolveTArgs A, const int K, const int2 *topinfo,
                                                             const uint8_t *toprows)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sttop_smem[];
    double *Rl = reinterpret_cast<double *>(sttop_smem);       // [row][column], rows kLcTopLd apart
    double *xc = Rl + (size_t)kLcTop * kLcTopLd;               // [2][NB]: x_c of the step, double buffered
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < kLcTop * kLcTopLd; i += 1024) Rl[i] = 0.0;
    __syncthreads();
    if (tid < kLcTop && tid >= K) Rl[tid * kLcTopLd + tid] = 1.0;
    for (int kk = wave; kk < K; kk += 16) {                    // column kk of the block: entry e (lane) sits in row toprows[kk][e]
        const int r = (int)toprows[kTopBlock * kk + lane];
        if (r != 0xFF) Rl[r * kLcTopLd + kk] = A.C[(size_t)topinfo[kk].y + 1 + lane].y;
    }
    const int j = tid & (NB - 1), g = tid / NB;
    double reg[kLcTopRows];
    int kcol[kLcTopRows];
#pragma unroll
    for (int r = 0; r < kLcTopRows; ++r) {
        const int col = g + r * kLcTopG;
        kcol[r] = col < K ? topinfo[col].x : -1;
        reg[r] = col < K ? A.X[(size_t)kcol[r] * NB + j] : 0.0;
    }
    __syncthreads();
    for (int c = 0; c < K; ++c) {
        double *xb = xc + (c & 1) * NB;
        if (g == c % kLcTopG) {
            const double d = Rl[c * kLcTopLd + c];
#pragma unroll
            for (int r = 0; r < kLcTopRows; ++r)
                if (r == c / kLcTopG) { reg[r] = reg[r] / d; xb[j] = reg[r]; }
        }
        __syncthreads();
        const double xv = xb[j];
#pragma unroll
        for (int r = 0; r < kLcTopRows; ++r) {
            const int col = g + r * kLcTopG;
            if (col > c) reg[r] = __builtin_fma(-Rl[c * kLcTopLd + col], xv, reg[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < kLcTopRows; ++r)
        if (kcol[r] >= 0) A.X[(size_t)kcol[r] * NB + j] = reg[r];
}

hipError_t launch_solvet_top(const SolveTArgs &a, int K, const int2 *topinfo, const uint8_t *toprows, hipStream_t s)
{
    if (K <= 0) return hipSuccess;
    if (K > kLcTop) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> done{0ull};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_relaxed) & bit)) {
        hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(&gpv_solvet_top_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLcTopSmem);
        if (e1 != hipSuccess) return e1;
        done.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(gpv_solvet_top_kernel, dim3(1), dim3(1024), kLcTopSmem, s, a, K, topinfo, toprows);
    return hipGetLastError();
}

// nb dense columns of E (ld apart) <-> the interleaved X[n][NB], 64 locations per block through an LDS tile so that both sides
// move whole lines; pack pads a short batch with zero columns
__global__ void __launch_bounds__(256) gpv_solvet_pack_kernel(double *X, const double *E, int64_t n, int64_t ld, int nb)
{
    __shared__ double tile[NB][65];
    const int64_t k0 = (int64_t)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int jj = ty; jj < NB; jj += 4) tile[jj][tx] = (jj < nb && k0 + tx < n) ? E[(int64_t)jj * ld + k0 + tx] : 0.0;
    __syncthreads();
    const int c = threadIdx.x & (NB - 1);
    for (int r = threadIdx.x / NB; r < 64; r += 256 / NB)
        if (k0 + r < n) X[(k0 + r) * NB + c] = tile[c][r];
}
__global__ void __launch_bounds__(256) gpv_solvet_unpack_kernel(const double *X, double *E, int64_t n, int64_t ld, int nb)
{
    __shared__ double tile[NB][65];
    const int64_t k0 = (int64_t)blockIdx.x * 64;
    const int c = threadIdx.x & (NB - 1);
    for (int r = threadIdx.x / NB; r < 64; r += 256 / NB) tile[c][r] = (k0 + r < n) ? X[(k0 + r) * NB + c] : 0.0;
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int jj = ty; jj < nb; jj += 4)
        if (k0 + tx < n) E[(int64_t)jj * ld + k0 + tx] = tile[jj][tx];
}
hipError_t launch_solvet_pack(double *X, const double *E, int64_t n, int64_t ld, int nb, hipStream_t s)
{
    if (n <= 0 || nb <= 0 || nb > NB || ld < n || (n + 63) / 64 > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_solvet_pack_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, X, E, n, ld, nb);
    return hipGetLastError();
}
hipError_t launch_solvet_unpack(const double *X, double *E, int64_t n, int64_t ld, int nb, hipStream_t s)
{
    if (n <= 0 || nb <= 0 || nb > NB || ld < n || (n + 63) / 64 > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_solvet_unpack_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, X, E, n, ld, nb);
    return hipGetLastError();
}

// ---- Monte-Carlo summaries of posterior draws (gpv_plan_draws_summary): normals made on the device, sums kept on the device --
// Per batch: gpv_draws_fill_kernel writes E ~ N(0, I) straight into X[Nlocs][NB] (gpv_philox.hpp: a function of seed, location
// and draw alone), the transposed sweep above turns it into X = R^-T E in place, and gpv_draws_accum_kernel folds
// y = mu + x into per-location sums, threshold counts and per-draw functionals.  After the last batch gpv_draws_finish_kernel
// turns the sums into mean, variance and exceedance probabilities.  Every sum has one fixed order; no floating-point atomics.

// One thread per (location, draw pair): a Box-Muller pair is two adjacent columns, stored as one 16-byte word, so a wavefront
// writes 64 / (NB / 2) whole rows.  draw0: the draw in column 0 (even).  Rows in front of skip_front and columns >= nb: zeros.
__global__ void __launch_bounds__(256) gpv_draws_fill_kernel(double *X, int64_t n, uint64_t seed, int64_t skip_front,
                                                             int64_t draw0, int nb)
{
    constexpr int PAIRS = NB / 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t k = t / PAIRS;
    const int p = (int)(t % PAIRS);
    if (k >= n) return;
    double2 v = make_double2(0.0, 0.0);
    if (k >= skip_front && 2 * p < nb) {
        draws_normal_pair(seed, (uint64_t)k, (uint64_t)(draw0 / 2 + p), v.x, v.y);
        if (2 * p + 1 >= nb) v.y = 0.0;
    }
    *reinterpret_cast<double2 *>(X + k * NB + 2 * p) = v;
}
hipError_t launch_draws_fill(double *X, int64_t n, uint64_t seed, int64_t skip_front, int64_t draw0, int nb, hipStream_t s)
{
    const int64_t blocks = (n * (NB / 2) + 255) / 256;
    if (n <= 0 || nb <= 0 || nb > NB || skip_front < 0 || draw0 < 0 || (draw0 & 1) || blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_draws_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, s, X, n, seed, skip_front, draw0, nb);
    return hipGetLastError();
}

template <int LINK>
__device__ __forceinline__ double draws_link(const double y)
{
    if constexpr (LINK == 1) return exp(y);
    else if constexpr (LINK == 2) return 1.0 / (1.0 + exp(-y));
    else return y;
}

// A workgroup walks tiles of 64 locations (tile = blockIdx.x, blockIdx.x + gridDim.x, ..).  Thread t keeps the column
// c = t % NB and the rows t / NB, t / NB + 256 / NB, .. of the tile: the NB columns of a location sit in NB adjacent lanes, so
// a count is one ballot and a popcount of the location's part of the mask.  d = g(y) - g(mu) goes through an LDS tile, and
// thread r < 64 adds row r's columns in ascending order before it adds the result into S1 / S2: one fixed order over all
// draws.  The per-draw maximum and sum over the selected locations stay in registers across the tiles, meet in LDS in
// row-group order, and leave as this workgroup's partial {max[NB], sum[NB]} (gpv_draws_stage2_kernel adds them in block order).
template <int LINK>
__global__ void __launch_bounds__(256) gpv_draws_accum_kernel(const DrawsArgs A, const int nb)
{
    constexpr int RPP = 256 / NB, PASSES = 64 / RPP;         // rows per pass, passes per tile
    __shared__ double dt[64][NB + 1];
    __shared__ double mu_s[64], gmu_s[64];
    __shared__ uint32_t ct[kDrawsMaxThr][64];
    __shared__ double pmax[RPP][NB], psum[RPP][NB];
    const int tid = threadIdx.x, c = tid & (NB - 1), g = tid / NB, lane = tid & 63;
    const bool colive = c < nb;
    const int64_t ntiles = (A.n + 63) / 64;
    double dmax = -INFINITY, dsum = 0.0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t k0 = tile * 64;
        if (tid < 64) {
            const int64_t k = k0 + tid;
            const double m = (k < A.n) ? A.mu[k] : 0.0;
            mu_s[tid] = m;
            gmu_s[tid] = draws_link<LINK>(m);
        }
        __syncthreads();
        double x[PASSES];
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            const int64_t k = k0 + g + i * RPP;
            x[i] = (k < A.n) ? A.X[k * NB + c] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            const int r = g + i * RPP;
            const int64_t k = k0 + r;
            const bool live = colive && k < A.n && k >= A.skip_front;
            const double y = mu_s[r] + x[i];
            const double gy = draws_link<LINK>(y);
            dt[r][c] = live ? gy - gmu_s[r] : 0.0;
            for (int th = 0; th < A.nthr; ++th) {
                const unsigned long long m = __ballot(live && y > A.thr[th]);
                if (c == 0) ct[th][r] = (uint32_t)__popcll((m >> (lane & ~(NB - 1))) & ((1ull << NB) - 1ull));
            }
            if (A.want_draw && live && (A.mask == nullptr || A.mask[k] != 0)) {
                dmax = fmax(dmax, gy);
                dsum += gy;
            }
        }
        __syncthreads();
        if (tid < 64) {
            const int64_t k = k0 + tid;
            if (k < A.n && k >= A.skip_front) {
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int cc = 0; cc < NB; ++cc) {
                    const double d = dt[tid][cc];
                    s1 += d;
                    s2 += d * d;
                }
                A.S1[k] += s1;
                A.S2[k] += s2;
                for (int th = 0; th < A.nthr; ++th) A.cnt[(int64_t)th * A.n + k] += ct[th][tid];
            }
        }
        __syncthreads();
    }
    if (!A.want_draw) return;
    pmax[g][c] = dmax;
    psum[g][c] = dsum;
    __syncthreads();
    if (tid < NB) {
        double mx = pmax[0][tid], sm = psum[0][tid];
#pragma unroll
        for (int gg = 1; gg < RPP; ++gg) { mx = fmax(mx, pmax[gg][tid]); sm += psum[gg][tid]; }
        A.part[((size_t)blockIdx.x * 2) * NB + tid] = mx;
        A.part[((size_t)blockIdx.x * 2 + 1) * NB + tid] = sm;
    }
}
// the workgroups' partials in block order: draw_max / draw_mean of the draws draw0 .. draw0 + nb - 1
__global__ void __launch_bounds__(NB) gpv_draws_stage2_kernel(const double *part, int nblocks, int nb, double nsel, double *draw_max,
                                                              double *draw_mean, int64_t draw0)
{
    const int c = threadIdx.x;
    if (c >= nb) return;
    double mx = -INFINITY, sm = 0.0;
    for (int b = 0; b < nblocks; ++b) {
        mx = fmax(mx, part[((size_t)b * 2) * NB + c]);
        sm += part[((size_t)b * 2 + 1) * NB + c];
    }
    draw_max[draw0 + c] = mx;
    draw_mean[draw0 + c] = sm / nsel;
}
int draws_accum_blocks(int64_t n)
{
    const int64_t ntiles = (n + 63) / 64;
    return (int)(ntiles < kDrawsBlocks ? ntiles : kDrawsBlocks);
}
hipError_t launch_draws_accum(const DrawsArgs &a, int link, int nb, int64_t draw0, double nsel, double *draw_max, double *draw_mean,
                              hipStream_t s)
{
    if (a.n <= 0 || nb <= 0 || nb > NB || a.nthr < 0 || a.nthr > kDrawsMaxThr || link < 0 || link > 2) return hipErrorInvalidValue;
    if (a.want_draw && (!draw_max || !draw_mean || !(nsel > 0.0))) return hipErrorInvalidValue;
    const int blocks = draws_accum_blocks(a.n);
    if (link == 0) hipLaunchKernelGGL(gpv_draws_accum_kernel<0>, dim3(blocks), dim3(256), 0, s, a, nb);
    else if (link == 1) hipLaunchKernelGGL(gpv_draws_accum_kernel<1>, dim3(blocks), dim3(256), 0, s, a, nb);
    else hipLaunchKernelGGL(gpv_draws_accum_kernel<2>, dim3(blocks), dim3(256), 0, s, a, nb);
    if (a.want_draw)
        hipLaunchKernelGGL(gpv_draws_stage2_kernel, dim3(1), dim3(NB), 0, s, (const double *)a.part, blocks, nb, nsel, draw_max,
                           draw_mean, draw0);
    return hipGetLastError();
}

// mean = g(mu) + S1 / N, var = (S2 - S1^2 / N) / (N - 1) clamped at 0, exceed = cnt / N; zeros in front of skip_front
__global__ void __launch_bounds__(256) gpv_draws_finish_kernel(const DrawsArgs A, const int link, const double N, double *mean,
                                                               double *var, double *exceed)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.n) return;
    const bool live = k >= A.skip_front;
    const double m = A.mu[k], s1 = A.S1[k], s2 = A.S2[k];
    const double gm = link == 1 ? draws_link<1>(m) : link == 2 ? draws_link<2>(m) : m;
    const double v = (s2 - s1 * s1 / N) / (N - 1.0);
    mean[k] = live ? gm + s1 / N : 0.0;
    var[k] = (live && v > 0.0) ? v : 0.0;
    for (int th = 0; th < A.nthr; ++th) exceed[(int64_t)th * A.n + k] = live ? (double)A.cnt[(int64_t)th * A.n + k] / N : 0.0;
}
hipError_t launch_draws_finish(const DrawsArgs &a, int link, int64_t ndraws, double *mean, double *var, double *exceed, hipStream_t s)
{
    if (a.n <= 0 || ndraws < 2 || (a.n + 255) / 256 > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_draws_finish_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a, link, (double)ndraws, mean,
                       var, exceed);
    return hipGetLastError();
}

}  // namespace gpv
