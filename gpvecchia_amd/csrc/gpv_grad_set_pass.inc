// gpv_grad_set_pass.inc -- the body of gpv_grad_kernel, gpv_fisher_kernel and gpv_rep_kernel (gpv_grad.hip), included once into
// each of them: every phase of a conditioning set stands here once, as text.  The includer provides KIND (kSetsGrad / kSetsFisher
// / kSetsRep), A (the GradArgs) and repZ, repR, repRP (the replicates; nullptr, 0, 0 unless kSetsRep).  Why text and not a
// template that the kernels call, and not one kernel template either: see the comment above the kernels.
    constexpr bool INFO = KIND != kSetsGrad, REP = KIND == kSetsRep;
    constexpr int NPAR = CovTraits<COV>::NPAR, NP1 = NPAR + 1;
    constexpr bool SCALED = CovTraits<COV>::SCALED;                   // matern_scaledim: the pair passes need the differences per coordinate
    constexpr int NROW = INFO ? kFisherRowLd : kGradRowLd, NV = INFO ? kFisherNV : kGradNV;
    __shared__ double s_part[kGradWavesPerBlock][NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool packed = A.dim <= 3;
    const int64_t nwaves = (int64_t)gridDim.x * kGradWavesPerBlock;
    double Rd = 1.0;                                                  // the replicate count (kSetsRep)
    if constexpr (REP) Rd = (double)repR;
    double acc[NV];
#pragma unroll
    for (int t = 0; t < NV; ++t) acc[t] = 0.0;

    for (int64_t k = (int64_t)blockIdx.x * kGradWavesPerBlock + wave; k < A.rows; k += nwaves) {
        // ---- gather: lane i of the bucket takes entry P - PB + i of the stored row (the valid entries are its LAST n0)
        const int e = A.P - PB + lane;
        const int v = (lane < PB && e >= 0) ? A.nn[k * A.P + e] : -1;
        const bool valid = v >= 0;
        const unsigned long long vmask = __ballot(valid);
        const bool own_ok = (vmask >> (PB - 1)) & 1ull;
        double zi = 0.0;                                              // the datum (the replicates are read in their own loop)
        if constexpr (!REP) zi = valid ? (packed ? A.rec[(int64_t)v * 4 + 3] : (A.z ? A.z[v] : 0.0)) : 0.0;
        double xc[3];                                                 // INFO, SCALED: the coordinates the pair pass keeps (dimension <= 3)
        if constexpr (INFO || SCALED) {
#pragma unroll
            for (int t = 0; t < 3; ++t) xc[t] = (packed && valid && t < A.dim) ? A.rec[(int64_t)v * 4 + t] : 0.0;
        }
        double a[PB];
        // kSetsGrad fills twice, as a call, as gpv_grad_kernel always did.  The closure is declared here because both of its uses,
        // below and in the gradient branch, must see it; in the other modes it is dead and leaves no trace in the code object
        auto distances = [&]() { GPV_FILL_DISTANCES };
        if constexpr (INFO) {
            GPV_FILL_DISTANCES
        } else {
            distances();
        }
        // ---- C on the valid rows and columns, zero elsewhere (a product with the 0 / 1 flags of both entries: no per-column
        // lane masks to keep); tau joins the diagonal where the pivot is read, so a padded row is tau times an identity row
        const int vhi = __double2hiint(valid ? 1.0 : 0.0);
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double vj = __hiloint2double(__builtin_amdgcn_readlane(vhi, j), 0);
            a[j] = grad_cov<COV>(gen_r2<COV>(a[j], valid && vj != 0.0), A) * (valid ? vj : 0.0);
            __builtin_amdgcn_sched_barrier(0);                        // one exp at a time: PB interleaved ones spill
        }
        // ---- Gauss-Jordan with the right-hand sides e_last [and z_J]; INFO: a[j] <- the multiplier of step j, for the replay
        double r1 = (lane == PB - 1) ? 1.0 : 0.0, r2 = zi, dg = 1.0;   // dg: 1 / pivot of the lane's own row
        bool fail = !own_ok;
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double d = readlane_d(a[j], j) + A.nug;
            fail |= !(d > 0.0);                                      // (uniform: every lane holds the same pivot)
            const bool pivot = lane == j;
            const double inv = 1.0 / d;                               // (needed on both sides of the select: stays branch-free)
            const double f = pivot ? 0.0 : a[j] * inv;
            dg = pivot ? inv : dg;
#pragma unroll
            for (int c = j + 1; c < PB; ++c) {
                a[c] = __builtin_fma(-f, readlane_d(a[c], j), a[c]);
            }
            r1 = __builtin_fma(-f, readlane_d(r1, j), r1);
            if constexpr (!REP) r2 = __builtin_fma(-f, readlane_d(r2, j), r2);
            if constexpr (INFO) a[j] = f;
            __builtin_amdgcn_sched_barrier(0);
        }
        const double u = r1 * dg, w = r2 * dg;                 // exact zeros on the padded rows (w: unused by kSetsRep)
        double val[NROW];                                             // the row's terms: every lane ends with the same values
        if constexpr (!INFO) {
            // ---- second pair pass: t_p = sum_j D_p(lane, j) u_j
            distances();
            double tp[NPAR];
#pragma unroll
            for (int p = 0; p < NPAR; ++p) tp[p] = 0.0;
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                double d[NPAR];
                if constexpr (SCALED) {                               // a[] holds the distances: the differences again, by read-lanes
                    double dq[3];
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        const double df = xc[t] - readlane_d(xc[t], j);
                        dq[t] = df * df;
                    }
                    grad_dcov_scaled<COV>(a[j], dq, A, d);
                } else {
                    grad_dcov<COV>(gen_r2<COV>(a[j], valid && ((vmask >> j) & 1ull)), A, d);
                }
                const double uj = readlane_d(u, j);
#pragma unroll
                for (int p = 0; p < NPAR; ++p) tp[p] = __builtin_fma(d[p], uj, tp[p]);
                __builtin_amdgcn_sched_barrier(0);
            }
            const double ul = readlane_d(u, PB - 1);
            const double q = wave_sum(u * zi);
            val[0] = 0.5 * log(ul) - 0.5 * q * q / ul - 0.91893853320467274178;   // 1/2 log 2 pi
#pragma unroll
            for (int p = 0; p <= NPAR; ++p) {
                const double ai = wave_sum(p < NPAR ? u * tp[p] : u * u);          // the nugget's block is the identity
                const double bi = wave_sum(p < NPAR ? w * tp[p] : w * u);
                val[1 + p] = -0.5 * ai / ul + q * bi / ul - 0.5 * q * q * ai / (ul * ul);
            }
#pragma unroll
            for (int p = NPAR + 2; p < kGradRowLd; ++p) val[p] = 0.0;
        } else {
            // ---- pair pass: tt_p = sum_j D_p(lane, j) u_j, zero on the padded rows (they are right-hand sides below); tt_NPAR = u
            double tt[NP1];
#pragma unroll
            for (int p = 0; p < NP1; ++p) tt[p] = 0.0;
            const int j0 = vmask ? __ffsll((long long)vmask) - 1 : 0;    // the columns in front of the first valid one hold u_j = 0
#pragma unroll 1
            for (int j = j0; j < PB; ++j) {
                double q2 = 0.0, dq[3] = {0.0, 0.0, 0.0};                // dq: SCALED only
                if (packed) {
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        const double df = xc[t] - readlane_d(xc[t], j);
                        if constexpr (SCALED) dq[t] = df * df;
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
                if constexpr (SCALED) grad_dcov_scaled<COV>(q2, dq, A, d);
                else grad_dcov<COV>(gen_r2<COV>(q2, valid), A, d);        // (the columns from j0 on are valid)
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
            // ---- row terms: of the one column, or summed over the replicates (gpv_rep_kernel.hpp)
            double ai[NP1], q2l = 0.0, qbl[NP1], Q2 = 0.0;            // q2l, qbl, Q2: the replicate mode's sums
            if constexpr (REP) {
                // lane l accumulates q_r^2 and q_r b_{p,r} of the replicates r = chunk + (l >> 3)
#pragma unroll
                for (int p = 0; p < NP1; ++p) qbl[p] = 0.0;
                const double2 *zrow = reinterpret_cast<const double2 *>(repZ + (int64_t)(valid ? v : 0) * repRP);
#pragma unroll 1
                for (int c0 = 0; c0 < repRP; c0 += kRepChunk) {
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
            }
            const bool mine8 = (lane & 7) == 0;                       // (kSetsRep: the 8 lanes of a group hold the same sums)
            if constexpr (REP) Q2 = wave_sum(mine8 ? q2l : 0.0);
            const double ul = readlane_d(u, PB - 1);                  // (read once: a second read moves the replicate kernels)
            if constexpr (REP) {
                val[0] = Rd * (0.5 * log(ul) - 0.91893853320467274178) - 0.5 * Q2 / ul;   // 1/2 log 2 pi
#pragma unroll
                for (int p = 0; p < NP1; ++p) {
                    ai[p] = wave_sum(u * tt[p]);
                    const double QB = wave_sum(mine8 ? qbl[p] : 0.0);
                    val[1 + p] = -0.5 * Rd * ai[p] / ul + QB / ul - 0.5 * Q2 * ai[p] / (ul * ul);
                }
            } else {
                const double q = wave_sum(u * zi);
                val[0] = 0.5 * log(ul) - 0.5 * q * q / ul - 0.91893853320467274178;
#pragma unroll
                for (int p = 0; p < NP1; ++p) {
                    ai[p] = wave_sum(u * tt[p]);
                    const double bi = wave_sum(w * tt[p]);
                    val[1 + p] = -0.5 * ai[p] / ul + q * bi / ul - 0.5 * q * q * ai[p] / (ul * ul);
                }
            }
#pragma unroll
            for (int p = NP1 + 1; p < NROW; ++p) val[p] = 0.0;
            int at = kGradRowLd;                                      // upper triangle, row-major, kernel-parameter order
#pragma unroll
            for (int i = 0; i < NP1; ++i) {
#pragma unroll
                for (int j = i; j < NP1; ++j) {
                    const double f = wave_sum(tt[i] * y[j]) / ul - 0.5 * ai[i] * ai[j] / (ul * ul);
                    val[at++] = REP ? Rd * f : f;                     // (the information of R columns is R F_k)
                }
            }
        }
        // ---- the set joins the wavefront's sums (behind the kGradRowLd values of the gradient come `failed` and `rows`, then the
        // triangle) unless it failed, and its terms go to its output row, one lane per value, NaN on failure
        acc[7] += 1.0;
        if (fail) {
            acc[6] += 1.0;
        } else {
#pragma unroll
            for (int p = 0; p < kGradRowLd; ++p) acc[p] += val[p];
#pragma unroll
            for (int p = kGradRowLd; p < NROW; ++p) acc[p + 2] += val[p];   // (INFO: the triangle, behind `failed` and `rows`)
        }
        if (A.row_terms != nullptr && lane < NROW) {
            double mine = 0.0;
#pragma unroll
            for (int p = 0; p < NROW; ++p) mine = (lane == p) ? val[p] : mine;
            A.row_terms[(int64_t)A.rowid[k] * NROW + lane] = fail ? __builtin_nan("") : mine;
        }
    }
    // ---- per-workgroup partials, waves added in wave order
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < NV; ++t) s_part[wave][t] = acc[t];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = 0.0;
        for (int wv = 0; wv < kGradWavesPerBlock; ++wv) s += s_part[wv][threadIdx.x];
        A.block_part[(int64_t)blockIdx.x * NV + threadIdx.x] = s;
    }
