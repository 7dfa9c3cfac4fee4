// gpv_loo.hip — the TRANSPOSE of the Vecchia whitening operator of an evaluation, the precision products and the leave-one-out
// cross-validation built on it (gfx950).
//
// For row k of a cond.yz = 'z' plan with stored U entries L_kj (j in J_k), own entry d_k and nugget tau_k the whitening
// operator is (T b)_k = (b_k + (sum_j L_kj b_j) / d_k) / s_k, s_k = sqrt(tau_k + 1/d_k^2): T_kk = 1/s_k, T_kj = L_kj g_k with
// g_k = 1 / (d_k s_k), and T_kk = d_k g_k: every entry of row k of T is the STORED entry times g_k, the own entry included.
// The precision of the data vector is Q = T^T T, and for a Gaussian model
//     E[z_i | z_-i] = z_i - (Q z)_i / Q_ii,        Var[z_i | z_-i] = 1 / Q_ii.
// T^T needs the factor by column: "of which sets is location i a neighbour".  The transposed index (loo_build_index, built
// once per plan on the host: the structure does not depend on the parameters) lists, for every internal position, the flat
// offsets into L of the entries that name it; the pass GATHERS over that list, one lane group per location, and nothing is
// scattered: no float atomics, the same bits every call.
//
// Passes.  scale: g by output row, once per evaluation.  forward: E = T B.  transposed: R = T^T E and q = diag(T^T T) in one
// launch, any column length.  scores: the leave-one-out mean, variance and the six score sums per column from r = Q z and q,
// on column-major data in a launch of its own (see DESIGN.md §4q for why it is not fused).
// Order of every sum: 16 virtual slots and one fixed tree (gpv_loo.h), so a column's bits are those of a one-column call.
#include "gpv_loo.h"

namespace gpv {
namespace {

__device__ __forceinline__ int64_t row_of(uint32_t off, uint64_t magic)
{
    return magic ? (int64_t)__umul64hi((uint64_t)off, magic) : (int64_t)off;
}

// the 16 virtual slot sums of a lane group -> their total in every lane of the group that holds the column.  A lane holds the
// slots sl + (16 / CP) j, j = 0 .. CP - 1 (the HIGH bits of the slot number), so the tree takes bit 3 first and bit 0 last:
// inside the lane while the bit is one of j's, across lanes (xor of the slot bits above the column bits) afterwards.
template <int CP>
__device__ __forceinline__ double slot_tree(double (&acc)[CP])
{
#pragma unroll
    for (int h = CP / 2; h >= 1; h >>= 1)
#pragma unroll
        for (int j = 0; j < h; ++j) acc[j] += acc[j + h];
    double a = acc[0];
#pragma unroll
    for (int off = kLooLanes / 2; off >= CP; off >>= 1) a += __shfl_xor(a, off, kLooLanes);
    return a;
}

__global__ void __launch_bounds__(256) gpv_loo_pack_kernel(const double *__restrict__ in, const int32_t *__restrict__ map, int64_t n,
                                                           int ncols, int cp, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * cp) return;
    const int64_t i = t / cp;
    const int c = (int)(t - i * cp);
    const int64_t p = map != nullptr ? (int64_t)map[i] : i;
    out[p * cp + c] = c < ncols ? in[(int64_t)c * n + i] : 0.0;
}

__global__ void __launch_bounds__(256) gpv_loo_unpack_kernel(const double *__restrict__ in, const int32_t *__restrict__ map, int64_t n,
                                                             int ncols, int cp, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * ncols) return;
    const int64_t c = t / n, i = t - c * n;
    const int64_t p = map != nullptr ? (int64_t)map[i] : i;
    out[t] = in[p * cp + c];
}

// one 16-lane group per stored set: g of its output row
__global__ void __launch_bounds__(kLooThreads) gpv_loo_scale_kernel(const LooArgs A)
{
    const int lig = threadIdx.x & (kLooLanes - 1);
    const int P = A.P;
    const int64_t stride = (int64_t)gridDim.x * kLooGroupsPerBlock;
    for (int64_t s = (int64_t)blockIdx.x * kLooGroupsPerBlock + (threadIdx.x >> 4); s < A.rows; s += stride) {
        const int32_t *const nr = A.nn + s * P;
        int miss = 0;
        for (int q = lig; q < P; q += kLooLanes) miss += nr[q] < 0 ? 1 : 0;
#pragma unroll
        for (int off = 1; off < kLooLanes; off <<= 1) miss += __shfl_xor(miss, off, kLooLanes);
        if (lig == 0) {
            const int32_t own = nr[P - 1];
            const int64_t kout = A.rowid[s];
            const int n0 = P - miss;
            const double d = own >= 0 ? A.L[kout * P + n0 - 1] : 0.0;      // (own >= 0: n0 >= 1)
            const double tau = own >= 0 ? (A.nuggets != nullptr ? A.nuggets[own] : A.nug_scalar) : 0.0;
            const bool fail = !(d > 0.0);              // a block that was not positive definite left its row of U at zero
            A.g[kout] = fail ? __builtin_nan("") : 1.0 / (d * sqrt(tau + 1.0 / (d * d)));
            if (fail) atomicAdd(A.nfail, 1u);
        }
    }
}

// E = T B: the whitening pass (gpv_whiten.hip) with the slot order of this unit
template <int CP>
__global__ void __launch_bounds__(kLooThreads) gpv_loo_forward_kernel(const LooArgs A)
{
    constexpr int NS = kLooLanes / CP;
    const int lig = threadIdx.x & (kLooLanes - 1);
    const int c = lig & (CP - 1), sl = lig / CP;
    const int P = A.P;
    const int64_t stride = (int64_t)gridDim.x * kLooGroupsPerBlock;
    for (int64_t s = (int64_t)blockIdx.x * kLooGroupsPerBlock + (threadIdx.x >> 4); s < A.rows; s += stride) {
        const int32_t *const nr = A.nn + s * P;
        const int32_t own = nr[P - 1];
        const bool have = own >= 0;
        const double bk = have ? A.B[(int64_t)own * CP + c] : 0.0;
        const double tau = have ? (A.nuggets != nullptr ? A.nuggets[own] : A.nug_scalar) : 0.0;
        int miss = 0;
        for (int q = lig; q < P; q += kLooLanes) miss += nr[q] < 0 ? 1 : 0;
#pragma unroll
        for (int off = 1; off < kLooLanes; off <<= 1) miss += __shfl_xor(miss, off, kLooLanes);
        const int n0 = P - miss;
        const int64_t kout = A.rowid[s];
        const double *const lr = A.L + kout * P;
        double acc[CP];
#pragma unroll
        for (int j = 0; j < CP; ++j) acc[j] = 0.0;
        for (int t0 = 0; t0 < n0 - 1; t0 += kLooLanes) {
#pragma unroll
            for (int j = 0; j < CP; ++j) {
                const int t = t0 + sl + NS * j;
                if (t < n0 - 1) {
                    const int32_t idx = nr[miss + t];
                    const double l = lr[t];
                    const double b = idx >= 0 ? A.B[(int64_t)idx * CP + c] : 0.0;
                    acc[j] = __builtin_fma(l, b, acc[j]);
                }
            }
        }
        const double sum = slot_tree<CP>(acc);
        const double d = have ? lr[n0 - 1] : 0.0;
        const bool fail = !(d > 0.0);
        const double e = fail ? __builtin_nan("") : (bk + sum / d) / sqrt(tau + 1.0 / (d * d));
        if (sl == 0) A.E[kout * CP + c] = e;
    }
}

// R = T^T E, q = diag(T^T T): one 16-lane group per internal position, a gather over the position's column
template <int CP>
__global__ void __launch_bounds__(kLooThreads) gpv_loo_transposed_kernel(const LooArgs A)
{
    constexpr int NS = kLooLanes / CP;
    const int lig = threadIdx.x & (kLooLanes - 1);
    const int c = lig & (CP - 1), sl = lig / CP;
    const uint64_t magic = A.pmagic;
    const int64_t stride = (int64_t)gridDim.x * kLooGroupsPerBlock;
    for (int64_t i = (int64_t)blockIdx.x * kLooGroupsPerBlock + (threadIdx.x >> 4); i < A.n; i += stride) {
        const uint32_t t_begin = (uint32_t)A.colptr[i], t_end = (uint32_t)A.colptr[i + 1];       // (< 2^31: t0 + 15 cannot wrap)
        const int32_t oo = A.owner[i];
        double acc[CP], qa[CP];
#pragma unroll
        for (int j = 0; j < CP; ++j) acc[j] = qa[j] = 0.0;
        for (uint32_t t0 = t_begin; t0 < t_end; t0 += kLooLanes) {
#pragma unroll
            for (int j = 0; j < CP; ++j) {
                const uint32_t t = t0 + sl + NS * j;
                if (t < t_end) {
                    const uint32_t off = (uint32_t)A.col[t];
                    const int64_t k = row_of(off, magic);
                    const double w = A.L[off] * A.g[k];
                    acc[j] = __builtin_fma(w, A.E[k * CP + c], acc[j]);
                    qa[j] = __builtin_fma(w, w, qa[j]);
                }
            }
        }
        double r = slot_tree<CP>(acc);
        double q = slot_tree<CP>(qa);
        if (oo >= 0) {                                 // the position's own row: T_ii = d_i g_i
            const int64_t k = row_of((uint32_t)oo, magic);
            const double w = A.L[oo] * A.g[k];
            r = __builtin_fma(w, A.E[k * CP + c], r);
            q = __builtin_fma(w, w, q);
        }
        if (sl == 0) A.R[i * CP + c] = r;
        if (lig == 0) A.q[i] = q;
    }
}

// blockIdx.y = the column, blockIdx.x = a contiguous chunk of the ordered locations.  Thread t takes the locations t, t + 256,
// .. of the chunk; the 256 thread sums are added in a fixed tree.  Nothing here depends on the padded column count.
__global__ void __launch_bounds__(kLooScoreThreads) gpv_loo_score_kernel(const double *__restrict__ Z, double *__restrict__ RM,
                                                                         const double *__restrict__ q, double *__restrict__ var,
                                                                         int64_t n, double *__restrict__ part)
{
    __shared__ double red[kLooNScores][kLooScoreThreads];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * chunk;
    const int64_t r1 = r0 + chunk < n ? r0 + chunk : n;
    double a[kLooNScores] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = r0 + tid; i < r1; i += kLooScoreThreads) {
        const double qi = q[i], z = Z[(int64_t)c * n + i], r = RM[(int64_t)c * n + i];
        const double v = 1.0 / qi, sd = sqrt(v);
        const double d = r / qi;                       // z_i - mu_i
        const double s = r / sqrt(qi);
        RM[(int64_t)c * n + i] = z - d;
        if (c == 0 && var != nullptr) var[i] = v;
        const double Phi2m1 = erf(s * 0.70710678118654752440);             // 2 Phi(s) - 1
        const double phi = 0.39894228040143267794 * exp(-0.5 * s * s);
        a[0] += d * d;
        a[1] += fabs(d);
        a[2] += s * s;
        a[3] += log(v);
        a[4] += sd * (s * Phi2m1 + 2.0 * phi - 0.56418958354775628695);
        a[5] += fabs(s) <= 1.959963984540054 ? 1.0 : 0.0;
    }
#pragma unroll
    for (int v = 0; v < kLooNScores; ++v) red[v][tid] = a[v];
    __syncthreads();
    for (int h = kLooScoreThreads / 2; h >= 1; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int v = 0; v < kLooNScores; ++v) red[v][tid] += red[v][tid + h];
        }
        __syncthreads();
    }
    if (tid < kLooNScores) part[((int64_t)c * gridDim.x + blockIdx.x) * kLooNScores + tid] = red[tid][0];
}

// ONE workgroup: the partials of every (column, score) added in workgroup order
__global__ void __launch_bounds__(kLooMaxCols * kLooNScores) gpv_loo_total_kernel(const double *__restrict__ part, int grid, int ncols,
                                                                                  double *__restrict__ scores)
{
    const int t = threadIdx.x;
    if (t >= ncols * kLooNScores) return;
    const int c = t / kLooNScores, v = t - c * kLooNScores;
    double s = 0.0;
    for (int b = 0; b < grid; ++b) s += part[((int64_t)c * grid + b) * kLooNScores + v];
    scores[t] = s;
}

bool cp_ok(int ncols, int cp) { return ncols >= 1 && ncols <= cp && cp <= kLooMaxCols && (cp & (cp - 1)) == 0; }

}  // namespace

int loo_grid(int64_t items, int cus)
{
    int64_t grid = (items + kLooGroupsPerBlock - 1) / kLooGroupsPerBlock;
    const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * kLooBlocksPerCU;
    if (grid > cap) grid = cap;
    return (int)(grid < 1 ? 1 : grid);
}

int loo_score_grid(int64_t n, int cus)
{
    int64_t grid = (n + 4 * kLooScoreThreads - 1) / (4 * kLooScoreThreads);
    const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * kLooScoreBlocksPerCU;
    if (grid > cap) grid = cap;
    return (int)(grid < 1 ? 1 : grid);
}

int loo_build_index(const int32_t *nn, const int32_t *rowid, int64_t rows, int64_t n, int P, std::vector<int32_t> &colptr,
                    std::vector<int32_t> &owner, std::vector<int32_t> &col)
{
    if (rows < 0 || n < 0 || P < 1) return 2;
    if (rows * (int64_t)P >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31) - 1) return 1;
    if (!nn || !rowid) return 2;
    colptr.assign((size_t)n + 1, 0);
    owner.assign((size_t)n, -1);
    // first pass: validation, the owners, the column lengths (kept one ahead: colptr[i + 1] counts column i)
    std::vector<uint8_t> listed_own((size_t)rows, 0);  // the set's own entry goes into the column: its position has an owner already
    for (int64_t s = 0; s < rows; ++s) {
        const int32_t *nr = nn + s * P;
        const int64_t kout = rowid[s];
        if (kout < 0 || kout >= rows) return 2;
        int miss = 0;
        while (miss < P && nr[miss] < 0) ++miss;
        for (int q = miss; q < P; ++q)
            if (nr[q] < 0 || nr[q] >= n) return 2;     // (a missing entry behind a valid one: not the layout the kernels read)
        for (int q = miss; q < P - 1; ++q) colptr[(size_t)nr[q] + 1]++;
        if (miss < P) {
            const int32_t own = nr[P - 1];
            if (owner[(size_t)own] < 0) owner[(size_t)own] = (int32_t)(kout * P + (P - 1 - miss));
            else { listed_own[(size_t)s] = 1; colptr[(size_t)own + 1]++; }
        }
    }
    for (int64_t i = 0; i < n; ++i) colptr[(size_t)i + 1] += colptr[(size_t)i];
    col.assign((size_t)colptr[(size_t)n], 0);
    std::vector<int32_t> fill(colptr.begin(), colptr.end() - 1);
    for (int64_t s = 0; s < rows; ++s) {               // ascending stored sets: every column comes out in that order
        const int32_t *nr = nn + s * P;
        const int64_t kout = rowid[s];
        int miss = 0;
        while (miss < P && nr[miss] < 0) ++miss;
        const int last = listed_own[(size_t)s] ? P : P - 1;
        for (int q = miss; q < last; ++q) col[(size_t)fill[(size_t)nr[q]]++] = (int32_t)(kout * P + (q - miss));
    }
    return 0;
}

hipError_t launch_loo_pack(const double *in, const int32_t *map, int64_t n, int ncols, int cp, double *out, hipStream_t s)
{
    if (n < 1 || !cp_ok(ncols, cp)) return hipErrorInvalidValue;
    const int64_t blocks = (n * cp + 255) / 256;
    hipLaunchKernelGGL(gpv_loo_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, map, n, ncols, cp, out);
    return hipGetLastError();
}

hipError_t launch_loo_unpack(const double *in, const int32_t *map, int64_t n, int ncols, int cp, double *out, hipStream_t s)
{
    if (n < 1 || !cp_ok(ncols, cp)) return hipErrorInvalidValue;
    const int64_t blocks = (n * ncols + 255) / 256;
    hipLaunchKernelGGL(gpv_loo_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, map, n, ncols, cp, out);
    return hipGetLastError();
}

hipError_t launch_loo_scale(const LooArgs &a, int grid, hipStream_t s)
{
    if (grid < 1 || a.rows < 1 || a.P < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_loo_scale_kernel, dim3((unsigned)grid), dim3(kLooThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_loo_forward(const LooArgs &a, int cp, int grid, hipStream_t s)
{
    if (grid < 1 || a.rows < 1 || a.P < 1) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(kLooThreads);
    switch (cp) {
        case 1: hipLaunchKernelGGL(gpv_loo_forward_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(gpv_loo_forward_kernel<2>, g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL(gpv_loo_forward_kernel<4>, g, b, 0, s, a); break;
        case 8: hipLaunchKernelGGL(gpv_loo_forward_kernel<8>, g, b, 0, s, a); break;
        case 16: hipLaunchKernelGGL(gpv_loo_forward_kernel<16>, g, b, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_loo_transposed(const LooArgs &a, int cp, int grid, hipStream_t s)
{
    if (grid < 1 || a.n < 1 || a.P < 1) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(kLooThreads);
    switch (cp) {
        case 1: hipLaunchKernelGGL(gpv_loo_transposed_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(gpv_loo_transposed_kernel<2>, g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL(gpv_loo_transposed_kernel<4>, g, b, 0, s, a); break;
        case 8: hipLaunchKernelGGL(gpv_loo_transposed_kernel<8>, g, b, 0, s, a); break;
        case 16: hipLaunchKernelGGL(gpv_loo_transposed_kernel<16>, g, b, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_loo_scores(const double *Z, double *RM, const double *q, double *var, int64_t n, int ncols, int grid, double *part,
                             double *scores, hipStream_t s)
{
    if (grid < 1 || n < 1 || ncols < 1 || ncols > kLooMaxCols) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_loo_score_kernel, dim3((unsigned)grid, (unsigned)ncols), dim3(kLooScoreThreads), 0, s, Z, RM, q, var, n, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gpv_loo_total_kernel, dim3(1), dim3(kLooMaxCols * kLooNScores), 0, s, (const double *)part, grid, ncols, scores);
    return hipGetLastError();
}

}  // namespace gpv
