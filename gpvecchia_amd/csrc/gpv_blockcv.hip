// gpv_blockcv.hip — leave-block-out cross-validation of a cond.yz = 'z' plan (gfx950): for every held-out block B of at most
// 64 locations the dense precision block Q_BB of the data vector, its Cholesky factor and the solves that give, without
// refitting,
//     z_B | z_-B  ~  N( z_B - Q_BB^-1 (Q z)_B ,  Q_BB^-1 ).
// Q = T^T T with T the whitening operator of the evaluation (gpv_loo.hip: every entry of row k of T is the STORED entry times
// g_k, the own entry included), so Q_ab = sum over the sets k that hold both a and b of T_ka T_kb.  r = Q z comes from the
// forward and transposed passes of gpv_loo.hip; this unit adds what is missing.
//
// The block index (blockcv_build_index, host, structure only) lists for every block its members and the stored sets with at
// least one member in it, ascending.  The block pass walks that list ONCE per block: one wavefront per block, a lane per slot
// of the set, the in-block entries of the set spread by local index in LDS, then every lane that has one adds its products
// into ITS row of the packed lower triangle of Q_BB.  It gathers; nothing is scattered to memory; there is no floating-point
// atomic; a pair (a, b) gets at most one term per set, so the order of every sum is the order of the list.  Factor (left-looking
// Cholesky, one lane per row), the two triangular solves for the call's columns (right-hand sides in registers), the inverse
// of the factor in place and diag(Q_BB^-1) follow in the same kernel: Q_BB never leaves LDS.  A block's results depend on its
// own members alone: the sets that hold two of them come in the same order whatever else is labelled.
//
// The scores are a pass of their own on ordered column-major data, in the scheme of gpv_loo.hip's: thread t of a chunk takes
// every 256th location, one fixed tree, so a column's sums do not depend on the padded column count.
#include "gpv_blockcv.h"

#include <algorithm>

namespace gpv {
namespace {

__device__ __forceinline__ int tri_row(int i) { return i * (i + 1) / 2; }

template <int CP>
__global__ void __launch_bounds__(kBcvThreads) gpv_blockcv_kernel(const BlockCvArgs A)
{
    __shared__ double tri[kBcvTri];                    // lower triangle by rows: (i, j) at i (i + 1) / 2 + j, j <= i
    __shared__ double vec[kBcvMaxBlock];               // the current set's entries T_ka by local index a, 0: not in the set
    const int lane = threadIdx.x;                      // (one wavefront: every barrier below is this wavefront's own)
    const int P = A.P;
    const int mine = tri_row(lane);
    for (int64_t b = blockIdx.x; b < A.n_blocks; b += gridDim.x) {
        const int m0 = A.memptr[b], nb = A.memptr[b + 1] - m0;                       // 1 <= nb <= 64
        const bool act = lane < nb;
        const int64_t pos = act ? (int64_t)A.members[m0 + lane] : 0;
        for (int t = lane; t < tri_row(nb); t += kBcvThreads) tri[t] = 0.0;
        __syncthreads();
        // ---- assembly: the block's sets in their fixed order
        const int s0 = A.setptr[b], s1 = A.setptr[b + 1];
        for (int si = s0; si < s1; ++si) {
            const int64_t s = A.sets[si];
            const int32_t *const nr = A.nn + s * P;
            const int64_t kout = A.rowid[s];
            const double gk = A.g[kout];
            const double *const lr = A.L + kout * P;
            int miss = 0;
            for (int q0 = 0; q0 < P; q0 += kBcvThreads) {
                const int q = q0 + lane;
                miss += __popcll(__ballot(q < P && nr[q] < 0));
            }
            vec[lane] = 0.0;
            __syncthreads();
            for (int t0 = 0; t0 < P - miss; t0 += kBcvThreads) {                     // a lane per slot; rows go to 192 entries
                const int t = t0 + lane;
                if (t < P - miss) {
                    const int2 bl = A.blkloc[nr[miss + t]];
                    if ((int64_t)bl.x == b) vec[bl.y] = lr[t] * gk;                  // (a position is in a set once: one writer)
                }
            }
            __syncthreads();
            const double va = vec[lane];
            unsigned long long in_set = __ballot(va != 0.0);
            while (in_set) {                           // the in-block entries of the set, ascending local index: wave-uniform
                const int c = __ffsll((long long)in_set) - 1;
                in_set &= in_set - 1;
                const double vc = vec[c];
                if (va != 0.0 && c <= lane) tri[mine + c] = __builtin_fma(va, vc, tri[mine + c]);
            }
            __syncthreads();
        }
        // ---- Q_BB = R R^T, left-looking, lane i keeps row i; R overwrites the triangle
        bool bad = false;
        double piv_mine = 1.0;
        for (int j = 0; j < nb; ++j) {
            const int jrow = tri_row(j);
            const bool below = act && lane >= j;
            double sum = below ? tri[mine + j] : 0.0;
            for (int k = 0; k < j; ++k) {
                const double rjk = tri[jrow + k];
                if (below) sum = __builtin_fma(-tri[mine + k], rjk, sum);
            }
            const double piv = __shfl(sum, j, kBcvThreads);
            if (!(piv > 0.0)) { bad = true; break; }   // (wave-uniform)
            const double rjj = sqrt(piv);
            if (lane == j) piv_mine = piv;
            if (below) tri[mine + j] = lane == j ? rjj : sum / rjj;
            __syncthreads();
        }
        if (bad) {                                     // the block's outputs keep the caller's NaN fill
            if (lane == 0) atomicAdd(A.nbad, 1u);
            __syncthreads();
            continue;
        }
        // ---- R y = r_B, R^T delta = y for the call's columns
        double rhs[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) rhs[c] = act ? A.R[pos * CP + c] : 0.0;
        for (int j = 0; j < nb; ++j) {
            const double rjj = tri[tri_row(j) + j];
            const double rij = (act && lane > j) ? tri[mine + j] : 0.0;
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                const double yj = __shfl(rhs[c], j, kBcvThreads) / rjj;
                if (lane == j) rhs[c] = yj;
                else if (act && lane > j) rhs[c] = __builtin_fma(-rij, yj, rhs[c]);
            }
        }
        if (act) {
#pragma unroll
            for (int c = 0; c < CP; ++c) A.Y2[pos * CP + c] = rhs[c] * rhs[c];
        }
        for (int j = nb - 1; j >= 0; --j) {
            const int jrow = tri_row(j);
            const double rjj = tri[jrow + j];
            const double rji = lane < j ? tri[jrow + lane] : 0.0;
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                const double xj = __shfl(rhs[c], j, kBcvThreads) / rjj;
                if (lane == j) rhs[c] = xj;
                else if (lane < j) rhs[c] = __builtin_fma(-rji, xj, rhs[c]);
            }
        }
        if (act) {
#pragma unroll
            for (int c = 0; c < CP; ++c) A.D[pos * CP + c] = rhs[c];
        }
        // ---- X = R^-1 in place, last column first: X_ij = -(sum_{j < k <= i} X_ik R_kj) / R_jj; var_a = sum_i X_ia^2
        for (int j = nb - 1; j >= 0; --j) {
            const int jrow = tri_row(j);
            const double d = 1.0 / tri[jrow + j];
            double acc = 0.0;
            for (int k = j + 1; k < nb; ++k) {
                const double rkj = tri[tri_row(k) + j];
                if (act && lane >= k) acc = __builtin_fma(tri[mine + k], rkj, acc);
            }
            __syncthreads();                           // column j has been read: now it is rewritten
            if (act && lane > j) tri[mine + j] = -acc * d;
            else if (lane == j) tri[jrow + j] = d;
            __syncthreads();
        }
        double v = 0.0;
        for (int i = 0; i < nb; ++i) {
            if (act && i >= lane) {
                const double x = tri[tri_row(i) + lane];
                v = __builtin_fma(x, x, v);
            }
        }
        if (act) {
            A.var[pos] = v;
            A.nlp[pos] = -log(piv_mine);
        }
        __syncthreads();                               // the triangle is the next block's
    }
}

// blockIdx.y = the column, blockIdx.x = a contiguous chunk of the ordered locations; as gpv_loo_score_kernel
__global__ void __launch_bounds__(kBcvScoreThreads) gpv_blockcv_score_kernel(const double *__restrict__ Z, double *__restrict__ DM,
                                                                             const double *__restrict__ Y2, const double *__restrict__ var,
                                                                             const double *__restrict__ nlp, int64_t n,
                                                                             double *__restrict__ part)
{
    __shared__ double red[kBcvNScores][kBcvScoreThreads];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * chunk;
    const int64_t r1 = r0 + chunk < n ? r0 + chunk : n;
    double a[kBcvNScores] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = r0 + tid; i < r1; i += kBcvScoreThreads) {
        const double v = var[i], z = Z[(int64_t)c * n + i], d = DM[(int64_t)c * n + i];        // d = z_i - mu_i
        DM[(int64_t)c * n + i] = z - d;                // NaN where the location is kept or its block was bad
        if (!(v > 0.0)) continue;
        const double sd = sqrt(v);
        const double s = d / sd;
        const double Phi2m1 = erf(s * 0.70710678118654752440);             // 2 Phi(s) - 1
        const double phi = 0.39894228040143267794 * exp(-0.5 * s * s);
        a[0] += d * d;
        a[1] += fabs(d);
        a[2] += s * s;
        a[3] += log(v);
        a[4] += sd * (s * Phi2m1 + 2.0 * phi - 0.56418958354775628695);
        a[5] += fabs(s) <= 1.959963984540054 ? 1.0 : 0.0;
        a[6] += Y2[(int64_t)c * n + i];
        a[7] += nlp[i];
    }
#pragma unroll
    for (int v = 0; v < kBcvNScores; ++v) red[v][tid] = a[v];
    __syncthreads();
    for (int h = kBcvScoreThreads / 2; h >= 1; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int v = 0; v < kBcvNScores; ++v) red[v][tid] += red[v][tid + h];
        }
        __syncthreads();
    }
    if (tid < kBcvNScores) part[((int64_t)c * gridDim.x + blockIdx.x) * kBcvNScores + tid] = red[tid][0];
}

// ONE workgroup: the partials of every (column, score) added in workgroup order
__global__ void __launch_bounds__(kBcvMaxCols * kBcvNScores) gpv_blockcv_total_kernel(const double *__restrict__ part, int grid, int ncols,
                                                                                      double *__restrict__ scores)
{
    const int t = threadIdx.x;
    if (t >= ncols * kBcvNScores) return;
    const int c = t / kBcvNScores, v = t - c * kBcvNScores;
    double s = 0.0;
    for (int b = 0; b < grid; ++b) s += part[((int64_t)c * grid + b) * kBcvNScores + v];
    scores[t] = s;
}

}  // namespace

int blockcv_grid(int64_t n_blocks, int cus)
{
    const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * kBcvBlocksPerCU;
    const int64_t grid = n_blocks < cap ? n_blocks : cap;
    return (int)(grid < 1 ? 1 : grid);
}

int blockcv_score_grid(int64_t n, int cus)
{
    int64_t grid = (n + 4 * kBcvScoreThreads - 1) / (4 * kBcvScoreThreads);
    const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * kBcvScoreBlocksPerCU;
    if (grid > cap) grid = cap;
    return (int)(grid < 1 ? 1 : grid);
}

int blockcv_check_labels(const int32_t *block_of_ord, int64_t n, std::vector<int32_t> &ids, std::vector<int32_t> &sizes)
{
    if (!block_of_ord || n < 1 || n >= ((int64_t)1 << 31) - 1) return 3;
    std::vector<int32_t> count((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t lab = block_of_ord[i];
        if (lab < -1 || lab >= n) return 3;
        if (lab >= 0 && ++count[(size_t)lab] > kBcvMaxBlock) return 3;
    }
    sizes.clear();
    for (int64_t l = 0; l < n; ++l) {                  // empty labels are skipped: count becomes the block number
        const int32_t c = count[(size_t)l];
        count[(size_t)l] = c > 0 ? (int32_t)sizes.size() : -1;
        if (c > 0) sizes.push_back(c);
    }
    if (sizes.empty()) return 3;
    ids.assign((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i)
        if (block_of_ord[i] >= 0) ids[(size_t)i] = count[(size_t)block_of_ord[i]];
    return 0;
}

int blockcv_build_index(const int32_t *nn, const int32_t *rowid, int64_t rows, int64_t n, int P, const int32_t *newpos,
                        const int32_t *block_of_ord, BlockIndex &out)
{
    if (rows < 0 || n < 0 || P < 1) return 2;
    if (rows * (int64_t)P >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31) - 1) return 1;
    if (!nn || !rowid) return 2;
    std::vector<int32_t> ids, sizes;
    if (blockcv_check_labels(block_of_ord, n, ids, sizes) != 0) return 3;
    for (int64_t s = 0; s < rows; ++s) {               // the layout the kernel reads, as loo_build_index checks it
        const int32_t *nr = nn + s * P;
        if (rowid[s] < 0 || rowid[s] >= rows) return 2;
        int miss = 0;
        while (miss < P && nr[miss] < 0) ++miss;
        for (int q = miss; q < P; ++q)
            if (nr[q] < 0 || nr[q] >= n) return 2;
    }
    const int64_t nblk = (int64_t)sizes.size();
    BlockIndex ix;
    ix.n_blocks = nblk;
    ix.memptr.assign((size_t)nblk + 1, 0);
    for (int64_t b = 0; b < nblk; ++b) {
        ix.memptr[(size_t)b + 1] = ix.memptr[(size_t)b] + sizes[(size_t)b];
        ix.max_size = std::max(ix.max_size, (int)sizes[(size_t)b]);
    }
    ix.n_heldout = ix.memptr[(size_t)nblk];
    ix.members.assign((size_t)ix.n_heldout, 0);
    ix.blkloc.assign((size_t)n * 2, -1);
    std::vector<int32_t> fill((size_t)nblk, 0);
    std::vector<uint8_t> seen(newpos ? (size_t)n : 0, 0);
    for (int64_t i = 0; i < n; ++i) {                  // ascending ordered row: the members of every block come out in that order
        const int64_t p = newpos ? (int64_t)newpos[i] : i;
        if (newpos) {
            if (p < 0 || p >= n || seen[(size_t)p]) return 2;
            seen[(size_t)p] = 1;
        }
        const int32_t b = ids[(size_t)i];
        if (b < 0) continue;
        const int32_t loc = fill[(size_t)b]++;
        ix.members[(size_t)ix.memptr[(size_t)b] + loc] = (int32_t)p;
        ix.blkloc[(size_t)p * 2] = b;
        ix.blkloc[(size_t)p * 2 + 1] = loc;
    }
    // the set lists: a set enters the list of every block it has a member in, once (stamp: the last set that did)
    ix.setptr.assign((size_t)nblk + 1, 0);
    std::vector<int32_t> stamp((size_t)nblk, -1);
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            for (int64_t b = 0; b < nblk; ++b) ix.setptr[(size_t)b + 1] += ix.setptr[(size_t)b];
            ix.n_set_refs = ix.setptr[(size_t)nblk];
            ix.sets.assign((size_t)ix.n_set_refs, 0);
            std::fill(stamp.begin(), stamp.end(), -1);
            std::copy(ix.setptr.begin(), ix.setptr.end() - 1, fill.begin());
        }
        for (int64_t s = 0; s < rows; ++s) {           // ascending stored sets: every list comes out in that order
            const int32_t *nr = nn + s * P;
            for (int q = 0; q < P; ++q) {
                if (nr[q] < 0) continue;
                const int32_t b = ix.blkloc[(size_t)nr[q] * 2];
                if (b < 0 || stamp[(size_t)b] == (int32_t)s) continue;
                stamp[(size_t)b] = (int32_t)s;
                if (pass == 0) ix.setptr[(size_t)b + 1]++;
                else ix.sets[(size_t)fill[(size_t)b]++] = (int32_t)s;
            }
        }
    }
    out = std::move(ix);
    return 0;
}

hipError_t launch_blockcv_blocks(const BlockCvArgs &a, int cp, int grid, hipStream_t s)
{
    if (grid < 1 || a.n_blocks < 1 || a.P < 1) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(kBcvThreads);
    switch (cp) {
        case 1: hipLaunchKernelGGL(gpv_blockcv_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(gpv_blockcv_kernel<2>, g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL(gpv_blockcv_kernel<4>, g, b, 0, s, a); break;
        case 8: hipLaunchKernelGGL(gpv_blockcv_kernel<8>, g, b, 0, s, a); break;
        case 16: hipLaunchKernelGGL(gpv_blockcv_kernel<16>, g, b, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_blockcv_scores(const double *Z, double *DM, const double *Y2, const double *var, const double *nlp, int64_t n, int ncols,
                                 int grid, double *part, double *scores, hipStream_t s)
{
    if (grid < 1 || n < 1 || ncols < 1 || ncols > kBcvMaxCols) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_blockcv_score_kernel, dim3((unsigned)grid, (unsigned)ncols), dim3(kBcvScoreThreads), 0, s, Z, DM, Y2, var, nlp,
                       n, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gpv_blockcv_total_kernel, dim3(1), dim3(kBcvMaxCols * kBcvNScores), 0, s, (const double *)part, grid, ncols, scores);
    return hipGetLastError();
}

}  // namespace gpv
