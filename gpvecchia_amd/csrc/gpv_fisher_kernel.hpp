// gpv_fisher_kernel.hpp — value, gradient and expected Fisher information of the cond.yz='z' Vecchia log-likelihood
// (gpv_plan_loglik_fisher), gfx950, FP64.  Included by gpv_grad.hip inside its per-bucket half: the helpers readlane_d, wave_sum,
// CovTraits, grad_cov and grad_dcov are those of that file, and so are the geometry (one wavefront per conditioning set, lane i
// owns row i, rows padded in front with rows of tau I) and the reduction.
//
// Per set, in the notation of gpv_grad.hip, with t_i = D_i u (t = u for the nugget), a_i = u't_i and y_j = S'^-1 t_j:
//     F_k[i, j] = t_i'y_j / u_last - 1/2 a_i a_j / u_last^2
// which is 1/2 tr(S'^-1 D_i S'^-1 D_j) of the block minus the same trace of its leading block without the set's own point: with
// L L' = S' only the last row of L^-1 D_i L^-T differs between the two, and that row is (L^-1 D_i v)' with v = u / sqrt(u_last).
// It is the expectation of -d2 l_k / dtheta_i dtheta_j under the exact process.
//
// The solves y_j REPLAY the elimination instead of repeating it: after step j of the Gauss-Jordan sweep column j of the block is
// dead, so the step's multiplier is kept there (and 1 / pivot in dg, as before); a further right-hand side then costs PB fused
// multiply-adds and read-lanes, (NPAR + 1) PB per set beside the PB^2 / 2 of the sweep.  The pair pass that forms t_i therefore
// may not use a[] as its scratch the way the gradient kernel's does: it recomputes each pair's squared distance inside its loop
// over the columns, from coordinates held in registers (dimension <= 3) or loaded per (column, coordinate) (dimension > 3),
// summing over the coordinates in the order of the first pass, so the distances are the same bits.  That loop indexes no
// register array and is not unrolled over the whole row.
//
// Builtins only, no inline assembly.
#pragma once

template <int PB, int COV>
__global__ void __launch_bounds__(64 * kGradWavesPerBlock, (PB == 16 ? 3 : (PB == 32 ? 2 : 1)))
    gpv_fisher_kernel(const GradArgs A)
{
    constexpr int NPAR = CovTraits<COV>::NPAR, NP1 = NPAR + 1;
    __shared__ double s_part[kGradWavesPerBlock][kFisherNV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool packed = A.dim <= 3;
    const int64_t nwaves = (int64_t)gridDim.x * kGradWavesPerBlock;
    double acc[kFisherNV];
#pragma unroll
    for (int t = 0; t < kFisherNV; ++t) acc[t] = 0.0;

    for (int64_t k = (int64_t)blockIdx.x * kGradWavesPerBlock + wave; k < A.rows; k += nwaves) {
        // ---- gather, as gpv_grad_kernel
        const int e = A.P - PB + lane;
        const int v = (lane < PB && e >= 0) ? A.nn[k * A.P + e] : -1;
        const bool valid = v >= 0;
        const unsigned long long vmask = __ballot(valid);
        const bool own_ok = (vmask >> (PB - 1)) & 1ull;
        const double zi = valid ? (packed ? A.rec[(int64_t)v * 4 + 3] : (A.z ? A.z[v] : 0.0)) : 0.0;
        // coordinates the pair pass keeps (dimension <= 3; the ones past the dimension are zeros and add exact zeros)
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
        // ---- Gauss-Jordan with the right-hand sides e_last and z_J; a[j] <- the multiplier of step j
        double r1 = (lane == PB - 1) ? 1.0 : 0.0, r2 = zi, dg = 1.0;
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
            r2 = __builtin_fma(-f, readlane_d(r2, j), r2);
            a[j] = f;
            __builtin_amdgcn_sched_barrier(0);
        }
        const double u = r1 * dg, w = r2 * dg;                        // exact zeros on the padded rows
        // ---- pair pass: tt_p = sum_j D_p(lane, j) u_j, zero on the padded rows (they are right-hand sides below); tt_NPAR = u
        double tt[NP1];
#pragma unroll
        for (int p = 0; p < NP1; ++p) tt[p] = 0.0;
        const int j0 = vmask ? __ffsll((long long)vmask) - 1 : 0;     // the columns in front of the first valid one hold u_j = 0
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
            grad_dcov<COV>(gen_r2<COV>(q2, valid), A, d);                 // (the columns from j0 on are valid)
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
        // ---- row terms (every lane ends with the same values)
        const double ul = readlane_d(u, PB - 1);
        const double q = wave_sum(u * zi);
        double val[kFisherRowLd], ai[NP1];
        val[0] = 0.5 * log(ul) - 0.5 * q * q / ul - 0.91893853320467274178;   // 1/2 log 2 pi
#pragma unroll
        for (int p = 0; p < NP1; ++p) {
            ai[p] = wave_sum(u * tt[p]);
            const double bi = wave_sum(w * tt[p]);
            val[1 + p] = -0.5 * ai[p] / ul + q * bi / ul - 0.5 * q * q * ai[p] / (ul * ul);
        }
#pragma unroll
        for (int p = NP1 + 1; p < kFisherRowLd; ++p) val[p] = 0.0;
        {
            int at = kGradRowLd;                                      // upper triangle, row-major, kernel-parameter order
#pragma unroll
            for (int i = 0; i < NP1; ++i) {
#pragma unroll
                for (int j = i; j < NP1; ++j) val[at++] = wave_sum(tt[i] * y[j]) / ul - 0.5 * ai[i] * ai[j] / (ul * ul);
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
