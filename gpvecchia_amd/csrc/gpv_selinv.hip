// gpv_selinv.hip — the selected inverse of the posterior factor: Sigma = W^-1 on the pattern of R (W = R R^T, R upper triangular,
// gpv_posterior.hip), by the Takahashi recursion; its diagonal is every posterior variance at once (R/vecchia_prediction.R:193-221,
// the SelInv branch of vecchia_var).
//
// Column c of R holds the rows N(c) (all < c) and c itself, last.  From Sigma R = R^-T (lower triangular, diagonal 1 / R_cc):
//     Sigma_ic = -(1 / R_cc) sum_{k in N(c)} Sigma_ik R_kc                    i in N(c)
//     Sigma_cc = 1 / R_cc^2 - (1 / R_cc) sum_{k in N(c)} Sigma_ck R_kc .
// Sigma_ik (i <= k both in N(c)) is entry i of column k: column c waits for the columns of its own rows, which is the dependency
// of the transposed sweep R^T x = e, so the pass walks that sweep's ascending schedule (gpv_lincomb.hip, gpv_solvet_level_kernel):
// the dense top block first, then one launch per level.  A pair (i, k) whose row i is no entry of column k contributes 0 (the
// match record 0xFF: the zero-fill rule of the factor pass); where no pair is dropped the result is W^-1 exactly.
//
// One wavefront per column, lane e = entry e.  Lane f fetches the pair record of neighbour f; then for every neighbour f the
// lanes e <= f read their match record (f + 1 consecutive bytes) and Sigma_{e f} from column f's block (positions ascend with
// e: a nearly contiguous run) into BOTH triangles of a symmetric tile in LDS; lane e then adds row e of the tile against R_.c
// in ascending order.  The dot product of Sigma_cc is one butterfly.  Every sum has one fixed order, nothing is atomic:
// bitwise reproducible.  The factor is only read.
#include "gpv_selinv.h"
#include <atomic>

namespace gpv {

__device__ __forceinline__ double si_shfl(const double v, const int l)
{
    const int lo = __builtin_amdgcn_ds_bpermute(l << 2, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(l << 2, __double2hiint(v));
    return __hiloint2double(hi, lo);
}

// doubles of one column's LDS: the tile (rows LD + 1 apart: a lane per row and a lane per column are both conflict free), then R_.c
template <int LD> constexpr int selinv_lds() { return LD * (LD + 1) + LD; }

// the wavefront's column: rec = {k, block offset, entries <= LD, first entry}
template <int LD>
__device__ __forceinline__ void selinv_column(const SelinvArgs &A, const int4 rec, double *tile, const int lane)
{
    constexpr int TL = LD + 1;
    double *rl = tile + LD * TL;
    const int k = rec.x, cb = rec.y, cnt = rec.z, m = rec.z - 1;
    double rv = 0.0;
    int2 pr = make_int2(0, 0);
    if (lane < cnt) rv = A.C[(size_t)cb + 1 + lane].y;
    if (lane < m) pr = A.pair[(size_t)rec.w + lane];
    if (lane < LD) rl[lane] = rv;
    const double rcc = si_shfl(rv, m);
    // the symmetric matrix Sigma_{N(c) N(c)}: four neighbours' trips to memory in flight
    for (int f0 = 0; f0 < m; f0 += 4) {
        int pos[4], cbf[4];
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = f0 + u, ff = f < m ? f : m - 1;
            cbf[u] = __builtin_amdgcn_ds_bpermute(ff << 2, pr.x);
            const int tq = __builtin_amdgcn_ds_bpermute(ff << 2, pr.y);
            pos[u] = (f < m && lane <= f) ? (int)A.tp[(size_t)tq + lane] : 0xFF;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = pos[u] != 0xFF ? A.S[(size_t)cbf[u] + 1 + pos[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = f0 + u;
            if (f < m && lane <= f) {
                tile[f * TL + lane] = v[u];
                tile[lane * TL + f] = v[u];
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double s = 0.0;
    if (lane < m)
        for (int f = 0; f < m; ++f) s = __builtin_fma(tile[f * TL + lane], rl[f], s);
    const double sig = -s / rcc;                              // Sigma_ec, e < m
    double dot = lane < m ? sig * rv : 0.0;                   // sum_e Sigma_ec R_ec: a butterfly, every lane ends with the same bits
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dot += si_shfl(dot, lane ^ off);
    const double scc = (1.0 / rcc - dot) / rcc;
    if (lane < m) A.S[(size_t)cb + 1 + lane] = sig;
    if (lane == m) {
        A.S[(size_t)cb + 1 + m] = scc;
        A.vars[k] = scc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (the tile is reused by the wavefront's next column)
    __builtin_amdgcn_wave_barrier();
}

template <int LD, int WPB>
__global__ void __launch_bounds__(64 * WPB) gpv_selinv_level_kernel(const SelinvArgs A, const int first, const int count)
{
    __shared__ double lds[WPB][selinv_lds<LD>()];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int w = (int)blockIdx.x * WPB + wib;
    if (w >= count) return;
    selinv_column<LD>(A, A.rec[(size_t)first + w], lds[wib], lane);
}

// The dense top block: its K <= 128 columns wait for each other and for nothing else (the rows of a column of the block are in
// the block), mostly as one chain, so ONE wavefront takes them in ascending order with Sigma_TT in LDS: a dense symmetric K x K
// matrix that starts as zero and receives the entries of the pattern as they are made, so that a pair outside the pattern reads
// as 0 (the zero-fill rule without a match record).  toprows[j][e] is the index inside the block of entry e's row (the column
// itself: j).  The only trips to memory are a column's own R values and row indices, requested one column ahead; the sums
// run over LDS in the order of the level kernel.  The entries also go to S and vars, where the columns outside the block read them.
constexpr int kSiTopLd = kSelinvTopMax + 1;
constexpr size_t kSiTopSmem = ((size_t)kSelinvTopMax * kSiTopLd + 64) * sizeof(double) + 64 * sizeof(int) + kSelinvTopMax * sizeof(int4);
__global__ void __launch_bounds__(64) gpv_selinv_top_kernel(const SelinvArgs A, const int K, const uint8_t *toprows)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sitop_smem[];
    double *Sig = reinterpret_cast<double *>(sitop_smem);      // [row][column], rows kSiTopLd apart
    double *rl = Sig + (size_t)kSelinvTopMax * kSiTopLd;       // [64] R_.c of the column at hand
    int4 *recs = reinterpret_cast<int4 *>(rl + 64);            // [K] the block's column records
    int *ri = reinterpret_cast<int *>(recs + kSelinvTopMax);   // [64] block indices of the column's rows
    const int lane = threadIdx.x;
    for (int i = lane; i < kSelinvTopMax * kSiTopLd; i += 64) Sig[i] = 0.0;
    for (int i = lane; i < K; i += 64) recs[i] = A.rec[i];
    __syncthreads();
    double rv_next = 0.0;
    int row_next = 0;
    {
        const int4 r0 = recs[0];
        if (lane < r0.z) { rv_next = A.C[(size_t)r0.y + 1 + lane].y; row_next = (int)toprows[lane]; }
    }
    for (int j = 0; j < K; ++j) {
        const int4 rec = recs[j];
        const int m = rec.z - 1;
        const double rv = rv_next;
        const int row = row_next;
        if (j + 1 < K) {                                       // the next column's operands leave now
            const int4 rn = recs[j + 1];
            rv_next = 0.0;
            row_next = 0;
            if (lane < rn.z) { rv_next = A.C[(size_t)rn.y + 1 + lane].y; row_next = (int)toprows[(size_t)(j + 1) * 64 + lane]; }
        }
        rl[lane] = rv;
        ri[lane] = row;
        __syncthreads();
        const double rcc = rl[m];
        double s = 0.0;
        if (lane < m)
            for (int f = 0; f < m; ++f) s = __builtin_fma(Sig[row * kSiTopLd + ri[f]], rl[f], s);
        const double sig = -s / rcc;
        double dot = lane < m ? sig * rv : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dot += si_shfl(dot, lane ^ off);
        const double scc = (1.0 / rcc - dot) / rcc;
        __syncthreads();                                       // every lane has read the tile before it changes
        if (lane < m) {
            Sig[row * kSiTopLd + j] = sig;
            Sig[j * kSiTopLd + row] = sig;
            A.S[(size_t)rec.y + 1 + lane] = sig;
        }
        if (lane == m) {
            Sig[j * kSiTopLd + j] = scc;
            A.S[(size_t)rec.y + 1 + m] = scc;
            A.vars[rec.x] = scc;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) gpv_selinv_out_kernel(const double *vars, int64_t n, int64_t skip_front, double *out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[k] = k < skip_front ? 0.0 : vars[k];
}

int selinv_tile(int max_entries) { return max_entries <= 16 ? 16 : max_entries <= 32 ? 32 : max_entries <= 64 ? 64 : 0; }

hipError_t launch_selinv_top(const SelinvArgs &a, int K, const uint8_t *toprows, hipStream_t s)
{
    if (K <= 0) return hipSuccess;
    if (K > kSelinvTopMax || !toprows) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> done{0ull};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_relaxed) & bit)) {
        hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(&gpv_selinv_top_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSiTopSmem);
        if (e1 != hipSuccess) return e1;
        done.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(gpv_selinv_top_kernel, dim3(1), dim3(64), kSiTopSmem, s, a, K, toprows);
    return hipGetLastError();
}

hipError_t launch_selinv_level(const SelinvArgs &a, int first, int count, int tile, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    if (first < 0) return hipErrorInvalidValue;
    if (tile == 16) hipLaunchKernelGGL((gpv_selinv_level_kernel<16, 4>), dim3((count + 3) / 4), dim3(256), 0, s, a, first, count);
    else if (tile == 32) hipLaunchKernelGGL((gpv_selinv_level_kernel<32, 4>), dim3((count + 3) / 4), dim3(256), 0, s, a, first, count);
    else if (tile == 64) hipLaunchKernelGGL((gpv_selinv_level_kernel<64, 1>), dim3(count), dim3(64), 0, s, a, first, count);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_selinv_out(const double *vars, int64_t n, int64_t skip_front, double *out, hipStream_t s)
{
    if (n <= 0 || (n + 255) / 256 > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_selinv_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, vars, n, skip_front, out);
    return hipGetLastError();
}

}  // namespace gpv
