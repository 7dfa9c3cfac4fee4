// gpv_unwhiten.hip — the colouring operator of an evaluation, the exact inverse of the whitening operator of gpv_whiten.hip,
// applied to a block of columns (gfx950).
//
// For row k of a cond.yz = 'z' plan with stored U entries L_kj (j in J_k), own entry d_k and nugget tau_k,
//     b_k = sqrt(tau_k + 1/d_k^2) e_k - (sum_j L_kj b_j) / d_k,        k = 0, 1, .. in the plan's ordered row sequence:
// a forward substitution over the ordered neighbour graph.  Row k needs the FINISHED values of its neighbours, so the rows are
// processed level by level (level(k) = 0 without neighbours, else 1 + max_j level(j); the schedule is built on the host by
// gpv_api.hip): all rows of one level are independent.  A wide level is one launch; a run of consecutive narrow levels is one
// launch of one workgroup with a workgroup barrier between the levels.  Kernel boundaries and workgroup barriers are the only
// synchronisation: no flags, nothing spins, no workgroup waits for another.
//
// Visibility inside a narrow run.  A level's values are written to B in global memory with plain stores and read by the
// next level with plain loads, by wavefronts of the SAME workgroup.  __syncthreads() between them is a workgroup-scope release
// fence, the barrier and a workgroup-scope acquire fence, which is what HIP guarantees to order them.  On gfx950 the wavefronts
// of one workgroup run on one compute unit (the library is never built for threadgroup-split mode) and their vector memory
// accesses go in issue order through that unit's one write-through L1, so the fences cost no cache operation and no wait for
// the stores: the compiler emits the bare barrier.  B is one non-const, non-restrict pointer for the loads and the stores, so
// the compiler neither keeps a value across the barrier nor treats the loads as invariant.
//
// Layout and arithmetic: those of the whitening pass.  16 lanes per set = (16 / CP neighbour slots) x (CP columns); slot sl
// adds its neighbours t = sl, sl + NS, .. in ascending order, the slots meet in a fixed xor tree: the same bits every call,
// with or without a captured graph, and a column's bits depend on CP alone, never on the other columns.
#include "gpv_unwhiten.h"
#include "gpv_philox.hpp"

namespace gpv {
namespace {

__global__ void __launch_bounds__(256) gpv_unwhiten_pack_kernel(const double *__restrict__ in, int64_t n, int ncols, int cp,
                                                                double *__restrict__ E)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * cp) return;
    const int64_t k = t / cp;
    const int c = (int)(t - k * cp);
    E[t] = c < ncols ? in[(int64_t)c * n + k] : 0.0;
}

__global__ void __launch_bounds__(256) gpv_unwhiten_unpack_kernel(const double *__restrict__ B, const int32_t *__restrict__ newpos,
                                                                  int64_t n, int ncols, int cp, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * ncols) return;
    const int64_t c = t / n, i = t - c * n;
    out[t] = B[(int64_t)newpos[i] * cp + c];
}

// one thread per (ordered location, draw pair): a Box-Muller pair is two adjacent columns, one 16-byte store
__global__ void __launch_bounds__(256) gpv_unwhiten_normals_kernel(double *E, int64_t n, uint64_t seed, int64_t draw0)
{
    constexpr int PAIRS = kUnwhitenMaxCols / 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t k = t / PAIRS;
    const int p = (int)(t % PAIRS);
    if (k >= n) return;
    double2 v;
    draws_normal_pair(seed, (uint64_t)k, (uint64_t)(draw0 / 2 + p), v.x, v.y);
    *reinterpret_cast<double2 *>(E + k * kUnwhitenMaxCols + 2 * p) = v;
}

// Stored set s by the 16 lanes of one group (lig = lane in the group); every lane of the group takes the same path.  `on`:
// the group holds a set of its own (the others repeat the slice's last set and write nothing, so that all 64 lanes of a
// wavefront reach the cross-lane sums).
template <int CP>
__device__ __forceinline__ void unwhiten_set(const UnwhitenArgs &A, const int32_t s, const bool on, const int lig)
{
    constexpr int NS = kUnwhitenLanes / CP;            // neighbour slots of a set's 16 lanes
    const int c = lig & (CP - 1), sl = lig / CP;
    const int P = A.P;
    const int32_t *const nr = A.nn + (int64_t)s * P;
    const int32_t own = nr[P - 1];
    const bool have = own >= 0;
    const int64_t kout = A.rowid[s];
    const double ek = A.E[kout * CP + c];
    const double tau = have ? (A.nuggets != nullptr ? A.nuggets[own] : A.nug_scalar) : 0.0;
    int miss = 0;                                      // missing entries stand in front
    for (int q = lig; q < P; q += kUnwhitenLanes) miss += nr[q] < 0 ? 1 : 0;
#pragma unroll
    for (int off = 1; off < kUnwhitenLanes; off <<= 1) miss += __shfl_xor(miss, off, kUnwhitenLanes);
    const int n0 = P - miss;
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
    for (int off = CP; off < kUnwhitenLanes; off <<= 1) acc += __shfl_xor(acc, off, kUnwhitenLanes);
    const double d = have ? lr[n0 - 1] : 0.0;          // (own >= 0: n0 >= 1)
    const bool fail = !(d > 0.0);                      // a block that was not positive definite left its row of U at zero
    const double sv = tau + 1.0 / (d * d);
    const double b = fail ? __builtin_nan("") : sqrt(sv) * ek - acc / d;
    if (on && have && sl == 0) A.B[(int64_t)own * CP + c] = b;
    if (on && fail && lig == 0) atomicAdd(A.nfail, 1u);
}

template <int CP>
__global__ void __launch_bounds__(kUnwhitenWideThreads) gpv_unwhiten_wide_kernel(const UnwhitenArgs A, const int64_t lo,
                                                                                 const int64_t hi)
{
    const int grp = threadIdx.x >> 4, lig = threadIdx.x & 15;
    const int64_t i = lo + (int64_t)blockIdx.x * kUnwhitenWideSets + grp;      // (the grid covers [lo, hi): blockIdx.x * 16 < hi - lo)
    const bool on = i < hi;
    unwhiten_set<CP>(A, A.order[on ? i : hi - 1], on, lig);
}

template <int CP>
__global__ void __launch_bounds__(kUnwhitenNarrowThreads) gpv_unwhiten_narrow_kernel(const UnwhitenArgs A, const int lev0,
                                                                                     const int lev1)
{
    const int grp = threadIdx.x >> 4, lig = threadIdx.x & 15;
    for (int lev = lev0; lev < lev1; ++lev) {          // every bound below is the same for the whole workgroup
        const int32_t lo = A.levptr[lev], hi = A.levptr[lev + 1];
        for (int32_t i0 = lo; i0 < hi; i0 += kUnwhitenNarrowSets) {
            const bool on = i0 + grp < hi;
            unwhiten_set<CP>(A, A.order[on ? i0 + grp : hi - 1], on, lig);
        }
        __syncthreads();                               // this level's stores to B are visible to the workgroup's next loads
    }
}

bool unwhiten_cp_ok(int cp) { return cp >= 1 && cp <= kUnwhitenMaxCols && (cp & (cp - 1)) == 0; }

}  // namespace

hipError_t launch_unwhiten_pack(const double *in, int64_t n, int ncols, int cp, double *E, hipStream_t s)
{
    if (n < 1 || ncols < 1 || ncols > cp || !unwhiten_cp_ok(cp)) return hipErrorInvalidValue;
    const int64_t blocks = (n * cp + 255) / 256;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_unwhiten_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, n, ncols, cp, E);
    return hipGetLastError();
}

hipError_t launch_unwhiten_unpack(const double *B, const int32_t *newpos, int64_t n, int ncols, int cp, double *out, hipStream_t s)
{
    if (n < 1 || ncols < 1 || ncols > cp || !unwhiten_cp_ok(cp)) return hipErrorInvalidValue;
    const int64_t blocks = (n * ncols + 255) / 256;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_unwhiten_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, B, newpos, n, ncols, cp, out);
    return hipGetLastError();
}

hipError_t launch_unwhiten_normals(double *E, int64_t n, uint64_t seed, int64_t draw0, hipStream_t s)
{
    const int64_t blocks = (n * (kUnwhitenMaxCols / 2) + 255) / 256;
    if (n < 1 || draw0 < 0 || (draw0 % kUnwhitenMaxCols) != 0 || blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpv_unwhiten_normals_kernel, dim3((unsigned)blocks), dim3(256), 0, s, E, n, seed, draw0);
    return hipGetLastError();
}

hipError_t launch_unwhiten_wide(const UnwhitenArgs &a, int cp, int64_t lo, int64_t hi, hipStream_t s)
{
    if (lo < 0 || hi <= lo || a.P < 1) return hipErrorInvalidValue;
    const int64_t blocks = (hi - lo + kUnwhitenWideSets - 1) / kUnwhitenWideSets;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    const dim3 g((unsigned)blocks), b(kUnwhitenWideThreads);
    switch (cp) {
        case 1: hipLaunchKernelGGL(gpv_unwhiten_wide_kernel<1>, g, b, 0, s, a, lo, hi); break;
        case 2: hipLaunchKernelGGL(gpv_unwhiten_wide_kernel<2>, g, b, 0, s, a, lo, hi); break;
        case 4: hipLaunchKernelGGL(gpv_unwhiten_wide_kernel<4>, g, b, 0, s, a, lo, hi); break;
        case 8: hipLaunchKernelGGL(gpv_unwhiten_wide_kernel<8>, g, b, 0, s, a, lo, hi); break;
        case 16: hipLaunchKernelGGL(gpv_unwhiten_wide_kernel<16>, g, b, 0, s, a, lo, hi); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_unwhiten_narrow(const UnwhitenArgs &a, int cp, int lev0, int lev1, hipStream_t s)
{
    if (lev0 < 0 || lev1 <= lev0 || a.P < 1 || !a.levptr) return hipErrorInvalidValue;
    const dim3 g(1), b(kUnwhitenNarrowThreads);
    switch (cp) {
        case 1: hipLaunchKernelGGL(gpv_unwhiten_narrow_kernel<1>, g, b, 0, s, a, lev0, lev1); break;
        case 2: hipLaunchKernelGGL(gpv_unwhiten_narrow_kernel<2>, g, b, 0, s, a, lev0, lev1); break;
        case 4: hipLaunchKernelGGL(gpv_unwhiten_narrow_kernel<4>, g, b, 0, s, a, lev0, lev1); break;
        case 8: hipLaunchKernelGGL(gpv_unwhiten_narrow_kernel<8>, g, b, 0, s, a, lev0, lev1); break;
        case 16: hipLaunchKernelGGL(gpv_unwhiten_narrow_kernel<16>, g, b, 0, s, a, lev0, lev1); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gpv
