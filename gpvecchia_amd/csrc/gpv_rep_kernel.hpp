// gpv_rep_kernel.hpp — value, gradient and expected Fisher information of the cond.yz='z' Vecchia log-likelihood SUMMED OVER R
// REPLICATES of the data over the same locations (gpv_plan_loglik_rep), gfx950, FP64.  Included by gpv_grad.hip inside its
// per-bucket half behind gpv_fisher_kernel.hpp: helpers, geometry (one wavefront per conditioning set, lane i owns row i, rows
// padded in front with rows of tau I) and the reduction are those of that kernel.
//
// Nothing of the factorisation depends on the data.  Per set, in the notation of gpv_fisher_kernel.hpp (u = S'^-1 e_last,
// t_p = D_p u with t_NPAR = u for the nugget, a_p = u't_p, y_p = S'^-1 t_p), the data enter a replicate's row terms only through
//     q_r = u'z_r       and       b_{p,r} = w_r't_p = z_r'S'^-1 t_p = z_r'y_p          (S' is symmetric),
// so the sweep carries the one right-hand side e_last, the replay gives y_p as it does for the information, and replicate r then
// costs NPAR + 2 dot products of length PB with the data-free vectors {u, y_0 .. y_NPAR}.  Summed over the replicates:
//     sum_r l_{k,r}             = R (1/2 log u_last - 1/2 log 2 pi) - 1/2 Q2 / u_last                    Q2   = sum_r q_r^2
//     sum_r dl_{k,r}/dtheta_p   = -1/2 R a_p / u_last + QB_p / u_last - 1/2 Q2 a_p / u_last^2            QB_p = sum_r q_r b_{p,r}
//     information               = R F_k                                            (it does not depend on the data)
//
// Replicate loop: lane i reads kRepChunk values of its neighbour at a time from Z[pos][RP] (contiguous, RP a multiple of
// kRepChunk, zeros behind column R) and forms the kRepChunk products with one of the NPAR + 2 vectors.  They are summed over the
// lanes by a reduce-scatter: the steps at lane distance 32, 16, 8 each HALVE the number of values a lane holds (a lane keeps the
// replicates of its half and hands over the others), 4 + 2 + 1 shuffles, and the steps at distance 4, 2, 1 finish the one value
// left, so a dot product costs 10 / 8 shuffles instead of 6.  Lane l then holds replicate (l >> 3) of the chunk, for every
// vector alike, squares and multiplies there, and accumulates over the chunks; one lane of each group of 8 enters the final sums.
// The order of every addition is fixed by the lane numbers: bitwise reproducible.
//
// Builtins only, no inline assembly.
#pragma once

// sum over the 64 lanes of each of the kRepChunk values x[c]; lane l returns the sum of x[l >> 3]
__device__ __forceinline__ double rep_reduce_scatter(const double (&x)[kRepChunk], const int lane)
{
    static_assert(kRepChunk == 8, "three halving steps");
    const bool h32 = lane & 32, h16 = lane & 16, h8 = lane & 8;
    double s4[4], s2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) s4[i] = (h32 ? x[4 + i] : x[i]) + __shfl_xor(h32 ? x[i] : x[4 + i], 32, 64);
#pragma unroll
    for (int i = 0; i < 2; ++i) s2[i] = (h16 ? s4[2 + i] : s4[i]) + __shfl_xor(h16 ? s4[i] : s4[2 + i], 16, 64);
    double s = (h8 ? s2[1] : s2[0]) + __shfl_xor(h8 ? s2[0] : s2[1], 8, 64);
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

template <int PB, int COV>
__global__ void __launch_bounds__(64 * kGradWavesPerBlock, (PB == 16 ? 3 : (PB == 32 ? 2 : 1)))
    gpv_rep_kernel(const RepArgs B)
{
    constexpr int NPAR = CovTraits<COV>::NPAR, NP1 = NPAR + 1;
    const GradArgs &A = B.g;
    __shared__ double s_part[kGradWavesPerBlock][kFisherNV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool packed = A.dim <= 3;
    const int64_t nwaves = (int64_t)gridDim.x * kGradWavesPerBlock;
    const double Rd = (double)B.R;
    double acc[kFisherNV];
#pragma unroll
    for (int t = 0; t < kFisherNV; ++t) acc[t] = 0.0;

    for (int64_t k = (int64_t)blockIdx.x * kGradWavesPerBlock + wave; k < A.rows; k += nwaves) {
        // ---- gather, as gpv_fisher_kernel (no datum)
        const int e = A.P - PB + lane;
        const int v = (lane < PB && e >= 0) ? A.nn[k * A.P + e] : -1;
        const bool valid = v >= 0;
        const unsigned long long vmask = __ballot(valid);
        const bool own_ok = (vmask >> (PB - 1)) & 1ull;
        double xc[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) xc[t] = (packed && valid && t < A.dim) ? A.rec[(int64_t)v * 4 + t] : 0.0;
        double a[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) a[j] = 0.0;
        for (int t = 0; t < A.dim; ++t) {
            const double x = valid ? (packed ? A.rec[(int64_t)v * 4 + t] : A.locs[(int64_t)v * A.locs_ld + t]) : 0.0;
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                const double df = x - readlane_d(x, j);
                a[j] = __builtin_fma(df, df, a[j]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const int vhi = __double2hiint(valid ? 1.0 : 0.0);
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double vj = __hiloint2double(__builtin_amdgcn_readlane(vhi, j), 0);
            a[j] = grad_cov<COV>(gen_r2<COV>(a[j], valid && vj != 0.0), A) * (valid ? vj : 0.0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- Gauss-Jordan with the right-hand side e_last; a[j] <- the multiplier of step j
        double r1 = (lane == PB - 1) ? 1.0 : 0.0, dg = 1.0;
        bool fail = !own_ok;
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double d = readlane_d(a[j], j) + A.nug;
            fail |= !(d > 0.0);
            const bool pivot = lane == j;
            const double inv = 1.0 / d;
            const double f = pivot ? 0.0 : a[j] * inv;
            dg = pivot ? inv : dg;
#pragma unroll
            for (int c = j + 1; c < PB; ++c) {
                a[c] = __builtin_fma(-f, readlane_d(a[c], j), a[c]);
            }
            r1 = __builtin_fma(-f, readlane_d(r1, j), r1);
            a[j] = f;
            __builtin_amdgcn_sched_barrier(0);
        }
        const double u = r1 * dg;                                     // exact zeros on the padded rows
        // ---- pair pass: tt_p = sum_j D_p(lane, j) u_j, zero on the padded rows; tt_NPAR = u
        double tt[NP1];
#pragma unroll
        for (int p = 0; p < NP1; ++p) tt[p] = 0.0;
        const int j0 = vmask ? __ffsll((long long)vmask) - 1 : 0;
#pragma unroll 1
        for (int j = j0; j < PB; ++j) {
            double q2 = 0.0;
            if (packed) {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const double df = xc[t] - readlane_d(xc[t], j);
                    q2 = __builtin_fma(df, df, q2);
                }
            } else {
                for (int t = 0; t < A.dim; ++t) {
                    const double x = valid ? A.locs[(int64_t)v * A.locs_ld + t] : 0.0;
                    const double df = x - readlane_d(x, j);
                    q2 = __builtin_fma(df, df, q2);
                }
            }
            double d[NPAR];
            grad_dcov<COV>(gen_r2<COV>(q2, valid), A, d);
            const double uj = readlane_d(u, j);
#pragma unroll
            for (int p = 0; p < NPAR; ++p) tt[p] = __builtin_fma(d[p], uj, tt[p]);
        }
#pragma unroll
        for (int p = 0; p < NPAR; ++p) tt[p] = valid ? tt[p] : 0.0;
        tt[NPAR] = u;
        // ---- y_p = S'^-1 tt_p: the sweep again, on the kept multipliers
        double y[NP1];
#pragma unroll
        for (int p = 0; p < NP1; ++p) y[p] = tt[p];
#pragma unroll
        for (int j = 0; j < PB; ++j) {
#pragma unroll
            for (int p = 0; p < NP1; ++p) y[p] = __builtin_fma(-a[j], readlane_d(y[p], j), y[p]);
        }
#pragma unroll
        for (int p = 0; p < NP1; ++p) y[p] *= dg;
        // ---- replicate loop: lane l accumulates q_r^2 and q_r b_{p,r} of the replicates r = chunk + (l >> 3)
        double q2l = 0.0, qbl[NP1];
#pragma unroll
        for (int p = 0; p < NP1; ++p) qbl[p] = 0.0;
        const double2 *zrow = reinterpret_cast<const double2 *>(B.Z + (int64_t)(valid ? v : 0) * B.RP);
#pragma unroll 1
        for (int c0 = 0; c0 < B.RP; c0 += kRepChunk) {
            double z[kRepChunk], x[kRepChunk];
#pragma unroll
            for (int i = 0; i < kRepChunk / 2; ++i) {
                const double2 two = zrow[(c0 >> 1) + i];
                z[2 * i] = valid ? two.x : 0.0;
                z[2 * i + 1] = valid ? two.y : 0.0;
            }
#pragma unroll
            for (int i = 0; i < kRepChunk; ++i) x[i] = u * z[i];
            const double qr = rep_reduce_scatter(x, lane);
            q2l = __builtin_fma(qr, qr, q2l);
#pragma unroll
            for (int p = 0; p < NP1; ++p) {
#pragma unroll
                for (int i = 0; i < kRepChunk; ++i) x[i] = y[p] * z[i];
                qbl[p] = __builtin_fma(qr, rep_reduce_scatter(x, lane), qbl[p]);
            }
        }
        const bool mine8 = (lane & 7) == 0;                           // the 8 lanes of a group hold the same sums
        const double Q2 = wave_sum(mine8 ? q2l : 0.0);
        // ---- row terms, summed over the replicates (every lane ends with the same values)
        const double ul = readlane_d(u, PB - 1);
        double val[kFisherRowLd], ai[NP1];
        val[0] = Rd * (0.5 * log(ul) - 0.91893853320467274178) - 0.5 * Q2 / ul;   // 1/2 log 2 pi
#pragma unroll
        for (int p = 0; p < NP1; ++p) {
            ai[p] = wave_sum(u * tt[p]);
            const double QB = wave_sum(mine8 ? qbl[p] : 0.0);
            val[1 + p] = -0.5 * Rd * ai[p] / ul + QB / ul - 0.5 * Q2 * ai[p] / (ul * ul);
        }
#pragma unroll
        for (int p = NP1 + 1; p < kFisherRowLd; ++p) val[p] = 0.0;
        {
            int at = kGradRowLd;                                      // upper triangle, row-major, kernel-parameter order
#pragma unroll
            for (int i = 0; i < NP1; ++i) {
#pragma unroll
                for (int j = i; j < NP1; ++j)
                    val[at++] = Rd * (wave_sum(tt[i] * y[j]) / ul - 0.5 * ai[i] * ai[j] / (ul * ul));
            }
        }
        acc[7] += 1.0;
        if (fail) {
            acc[6] += 1.0;
        } else {
#pragma unroll
            for (int p = 0; p < kGradRowLd; ++p) acc[p] += val[p];
#pragma unroll
            for (int p = kGradRowLd; p < kFisherRowLd; ++p) acc[p + 2] += val[p];
        }
        if (A.row_terms != nullptr && lane < kFisherRowLd) {
            double mine = 0.0;
#pragma unroll
            for (int p = 0; p < kFisherRowLd; ++p) mine = (lane == p) ? val[p] : mine;
            A.row_terms[(int64_t)A.rowid[k] * kFisherRowLd + lane] = fail ? __builtin_nan("") : mine;
        }
    }
    // ---- per-workgroup partials, waves added in wave order
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < kFisherNV; ++t) s_part[wave][t] = acc[t];
    }
    __syncthreads();
    if (threadIdx.x < kFisherNV) {
        double s = 0.0;
        for (int wv = 0; wv < kGradWavesPerBlock; ++wv) s += s_part[wv][threadIdx.x];
        A.block_part[(int64_t)blockIdx.x * kFisherNV + threadIdx.x] = s;
    }
}
