// tests/sanitize/csim_summary_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_cond_sim_summary
// (include/gpvecchia.h) under AddressSanitizer + UBSan, linked like tests/sanitize/csim_driver.cpp against
// tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  Kernels do not run, so this checks the statuses, the refusals
// before the device is touched (nothing written, nothing launched), the launch counts against the schedule (the factor pass by
// its chunks; one sweep for the means and one per batch of 16 that [col0, col0 + ndraws) touches, a sweep = a packing or normals
// launch + one launch per wide level and per run of narrow ones; one launch that prepares mu and the live mask; per batch the
// accumulation, the fold over the chunks when there is a chunk and the join when a region has none or several; one finish), the
// shape of what is written (heap blocks of exactly the stated length: a byte beyond them is the sanitizer's finding), that the
// plan's evaluation stays what it was, that gpv_plan_cond_sim launches what it launched before the two shared their operator,
// and that nothing is left allocated — never numbers.
//
//   build: tests/_host_driver_build.py; run by tests/test_csim_summary_driver.py and tools/sanitize_host.sh.
#include "../../include/gpvecchia.h"

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

extern "C" long mockhip_launches(void);
extern "C" long mockhip_live_allocations(void);
extern "C" int gpv_plan_debug_csim_chunk(gpv_plan *pl, int64_t chunk);
extern "C" int gpv_plan_debug_csim_summary_ms(gpv_plan *pl, double *ms);

static int g_fail = 0;
#define EXPECT(cond)                                                                           \
    do {                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)
#define EXPECT_ST(call, want)                                                                  \
    do {                                                                                       \
        const int st_ = (call);                                                                \
        if (st_ != (want)) { std::fprintf(stderr, "%s:%d: %s -> %d (%s), wanted %d\n", __FILE__, __LINE__, #call, st_, gpv_status_string(st_), (int)(want)); ++g_fail; } \
    } while (0)

static void make_rows(int64_t n, int p, bool latent, std::vector<int> &revNN, std::vector<int> &revCond)
{
    revNN.assign((size_t)n * p, 0);
    revCond.assign((size_t)n * p, INT_MIN);
    for (int64_t k = 0; k < n; ++k)
        for (int j = 0; j < p; ++j) {
            const int64_t v = k - (p - 1 - j);
            if (v < 0) continue;
            revNN[(size_t)(k + (int64_t)j * n)] = (int)v + 1;
            revCond[(size_t)(k + (int64_t)j * n)] = (j == p - 1 || latent) ? 1 : 0;
        }
}

static constexpr double kGuard = -7.0;
struct Block {                                          // a heap block of exactly n doubles
    std::unique_ptr<double[]> p;
    int64_t n = 0;
    void make(int64_t n_) { n = n_; p.reset(new double[(size_t)n_]); std::fill_n(p.get(), n_, kGuard); }
    bool all(bool guard) const
    {
        bool a = true;
        for (int64_t i = 0; i < n; ++i) a = a && ((p[(size_t)i] == kGuard) == guard);
        return a;
    }
};

// every argument of one call, with defaults that are served; the outputs as heap blocks of exactly the stated length
struct Call {
    gpv_plan *pl;
    const char *cov = "matern";
    const double *par, *nug, *Z = nullptr, *q, *scale = nullptr, *offset = nullptr, *thr = nullptr, *regw = nullptr;
    int npar = 3, ncols = 1, m, link = 0, nthr = 0;
    int64_t nnug = 1, nq, col0 = 0, ndraws = 20, nreg = 0;
    const int *nn;
    const unsigned char *elig = nullptr;
    const int64_t *regptr = nullptr;
    const int32_t *regidx = nullptr;
    Block mean, sd, mcm, mcv, ex, rt, rx, rn, ra, rw;
    std::unique_ptr<int64_t[]> rc;
    int64_t nlev = -1, nlaunch = -1, nf = -1;
    bool null_mean = false, null_ex = false, null_rt = false, null_ra = false, null_rw = false, null_rc = false, null_nf = false;
    void alloc()
    {
        const int64_t nd = ndraws > 0 ? ndraws : 0, nr = nreg > 0 ? nreg : 0, nt = nthr > 0 ? nthr : 0, n = nq > 0 ? nq : 0;
        mean.make(n); sd.make(n); mcm.make(n); mcv.make(n); ex.make(n * nt);
        rt.make(nr * nd); rx.make(nr * nd); rn.make(nr * nd); ra.make(nr * nd * nt); rw.make(nr);
        rc.reset(new int64_t[(size_t)nr]);
        std::fill_n(rc.get(), nr, (int64_t)-7);
        nlev = nlaunch = nf = -1;
    }
    int run()
    {
        alloc();
        return gpv_plan_cond_sim_summary(pl, cov, par, npar, nug, nnug, Z, ncols, q, nq, m, nn, scale, elig, 5, col0, ndraws, offset, link, nthr,
                                         thr, nreg, regptr, regidx, regw, null_mean ? nullptr : mean.p.get(), sd.p.get(), mcm.p.get(),
                                         mcv.p.get(), null_ex ? nullptr : ex.p.get(), null_rt ? nullptr : rt.p.get(), rx.p.get(), rn.p.get(),
                                         null_ra ? nullptr : ra.p.get(), null_rw ? nullptr : rw.p.get(), null_rc ? nullptr : rc.get(), &nlev,
                                         &nlaunch, null_nf ? nullptr : &nf);
    }
    bool counts(bool guard) const
    {
        bool a = true;
        for (int64_t r = 0; r < (nreg > 0 ? nreg : 0); ++r) a = a && ((rc[(size_t)r] == -7) == guard);
        return a;
    }
    bool untouched() const
    {
        return nlev == -1 && nlaunch == -1 && nf == -1 && mean.all(true) && sd.all(true) && mcm.all(true) && mcv.all(true) && ex.all(true) &&
               rt.all(true) && rx.all(true) && rn.all(true) && ra.all(true) && rw.all(true) && counts(true);
    }
    bool written() const
    {
        return nlev >= 0 && nf >= 0 && mean.all(false) && sd.all(false) && mcm.all(false) && mcv.all(false) && ex.all(false) && rt.all(false) &&
               rx.all(false) && rn.all(false) && ra.all(false) && rw.all(false) && counts(false);
    }
};

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);
    const int64_t n = 3000;
    const int dim = 2, p = 11, m = 10;
    std::mt19937_64 rng(9);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> locs((size_t)n * dim), z((size_t)n), Zc((size_t)n, 0.5);
    for (auto &v : locs) v = U(rng);
    for (auto &v : z) v = U(rng) - 0.5;
    std::vector<int> revNN, revCond;
    make_rows(n, p, false, revNN, revCond);
    const double cp[3] = {1.0, 0.1, 1.5}, tau = 0.1;
    // the lists of tests/sanitize/csim_driver.cpp: 52 levels, two wide ones and ONE run of narrow ones
    const int64_t nq = 700, want_levels = 52, L = 3;
    std::vector<int> NN((size_t)nq * m, 0);
    for (int64_t i = 0; i < nq; ++i) {
        for (int s = 0; s < 8; ++s) NN[(size_t)(i + (int64_t)s * nq)] = (int)((i * 7 + s) % n) + 1;
        if (i >= 300 && i < 600) NN[(size_t)(i + 8 * nq)] = (int)(n + 1 + (i - 300));
        if (i >= 600 && i < 650) NN[(size_t)(i + 9 * nq)] = (int)(n + i);
    }
    std::vector<double> ql((size_t)nq * dim), off((size_t)nq, 0.25);
    for (auto &v : ql) v = 1.4 * U(rng) - 0.2;
    const double thr8[8] = {-1, -0.5, 0, 0.1, 0.2, 0.5, 1, 2};
    // regions: all 700 rows (6 chunks of 128: joined), rows 0 .. 9 (one chunk: finished by the fold), none (written by the join),
    // 129 rows (two chunks)
    std::vector<int64_t> regptr = {0, 700, 710, 710, 839};
    std::vector<int32_t> regidx;
    for (int i = 0; i < 700; ++i) regidx.push_back(i);
    for (int i = 0; i < 10; ++i) regidx.push_back(i);
    for (int i = 0; i < 129; ++i) regidx.push_back(699 - 3 * i);
    std::vector<double> regw(regidx.size());
    for (size_t e = 0; e < regw.size(); ++e) regw[e] = (e % 5 == 0) ? -0.5 : 1.0 + 0.001 * (double)e;
    const int64_t one_ptr[2] = {0, 10}, empty_ptr[2] = {0, 0};

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    const auto base = [&] {
        Call c;
        c.pl = pl; c.par = cp; c.nug = &tau; c.Z = Zc.data(); c.q = ql.data(); c.m = m; c.nq = nq; c.nn = NN.data();
        c.nthr = 3; c.thr = thr8; c.nreg = 4; c.regptr = regptr.data(); c.regidx = regidx.data(); c.regw = regw.data();
        return c;
    };
    // ---- arguments, before the state is looked at and before the device is touched
    const long l0 = mockhip_launches();
#define REFUSED(want, ...)                                             \
    do {                                                               \
        Call c = base();                                               \
        __VA_ARGS__;                                                   \
        EXPECT_ST(c.run(), want);                                      \
        EXPECT(c.untouched());                                         \
    } while (0)
    REFUSED(GPV_ERR_BAD_ARG, c.pl = nullptr);
    REFUSED(GPV_ERR_BAD_ARG, c.cov = nullptr);
    REFUSED(GPV_ERR_BAD_ARG, c.par = nullptr);
    REFUSED(GPV_ERR_BAD_ARG, c.npar = 4);
    REFUSED(GPV_ERR_COVTYPE, c.cov = "gauss");
    REFUSED(GPV_ERR_BAD_ARG, c.m = 0);
    REFUSED(GPV_ERR_UNSUPPORTED_M, c.m = 64; c.nn = nullptr);
    REFUSED(GPV_ERR_BAD_ARG, c.nug = nullptr);
    REFUSED(GPV_ERR_BAD_ARG, c.nnug = 2);
    REFUSED(GPV_ERR_BAD_ARG, c.ncols = 2);                                    // one data column only
    REFUSED(GPV_ERR_BAD_ARG, c.ncols = 0);
    REFUSED(GPV_ERR_BAD_ARG, c.q = nullptr);
    REFUSED(GPV_ERR_BAD_ARG, c.nq = -1);
    REFUSED(GPV_ERR_BAD_ARG, c.ndraws = 1);
    REFUSED(GPV_ERR_BAD_ARG, c.ndraws = 0);
    REFUSED(GPV_ERR_BAD_ARG, c.ndraws = -4);
    REFUSED(GPV_ERR_BAD_ARG, c.col0 = -1);
    REFUSED(GPV_ERR_BAD_ARG, c.col0 = INT64_MAX - 3);                         // col0 + ndraws overflows
    REFUSED(GPV_ERR_BAD_ARG, c.link = -1);
    REFUSED(GPV_ERR_BAD_ARG, c.link = 3);
    REFUSED(GPV_ERR_BAD_ARG, c.nthr = -1);
    REFUSED(GPV_ERR_BAD_ARG, c.nthr = 9);
    REFUSED(GPV_ERR_BAD_ARG, c.thr = nullptr);
    REFUSED(GPV_ERR_BAD_ARG, c.null_mean = true);
    REFUSED(GPV_ERR_BAD_ARG, c.null_ex = true);
    REFUSED(GPV_ERR_BAD_ARG, c.null_rt = true);
    REFUSED(GPV_ERR_BAD_ARG, c.null_ra = true);
    REFUSED(GPV_ERR_BAD_ARG, c.null_rw = true);
    REFUSED(GPV_ERR_BAD_ARG, c.null_rc = true);
    REFUSED(GPV_ERR_BAD_ARG, c.null_nf = true);
    REFUSED(GPV_ERR_BAD_ARG, c.nreg = -1);
    REFUSED(GPV_ERR_BAD_ARG, c.regptr = nullptr);
    REFUSED(GPV_ERR_BAD_ARG, c.regidx = nullptr);
    {
        std::vector<int64_t> rp(regptr);
        rp[0] = 1;
        REFUSED(GPV_ERR_BAD_ARG, c.regptr = rp.data());                       // not from 0
        rp[0] = 0; rp[2] = 699;
        REFUSED(GPV_ERR_BAD_ARG, c.regptr = rp.data());                       // decreasing
        std::vector<double> rw(regw);
        rw[705] = INFINITY;
        REFUSED(GPV_ERR_BAD_ARG, c.regw = rw.data());
        rw[705] = NAN;
        REFUSED(GPV_ERR_BAD_ARG, c.regw = rw.data());
        std::vector<int32_t> ri(regidx);
        ri[703] = (int32_t)nq;
        REFUSED(GPV_ERR_INDEX, c.regidx = ri.data());
        ri[703] = -1;
        REFUSED(GPV_ERR_INDEX, c.regidx = ri.data());
        std::vector<int> bad(NN);
        bad[(size_t)(5 + 9 * nq)] = (int)(n + 5 + 1);                          // its own row
        REFUSED(GPV_ERR_INDEX, c.nn = bad.data());
        const double neg = -0.1, cpn[3] = {1.0, 0.1, 61.0}, scbad[2] = {0.1, 0.0};
        REFUSED(GPV_ERR_BAD_ARG, c.nug = &neg);
        REFUSED(GPV_ERR_UNSUPPORTED_NU, c.par = cpn);
        REFUSED(GPV_ERR_BAD_ARG, c.scale = scbad; c.nn = nullptr);
    }
    REFUSED(GPV_ERR_STATE, c.Z = nullptr);                                    // the plan's data, and none set
    EXPECT(mockhip_launches() == l0);
    // ---- no location: every region is empty, nothing launched
    {
        Call c = base();
        c.nq = 0; c.q = nullptr; c.nn = nullptr; c.regptr = empty_ptr; c.nreg = 1; c.regidx = nullptr; c.regw = nullptr;
        EXPECT_ST(c.run(), GPV_OK);
        EXPECT(c.written() && c.nlev == 0 && c.nlaunch == 0 && c.nf == 0 && mockhip_launches() == l0);
        EXPECT(c.rt.p[0] == 0.0 && std::isnan(c.rx.p[0]) && std::isnan(c.rn.p[0]) && c.ra.p[0] == 0.0 && c.rw.p[0] == 0.0 && c.rc[0] == 0);
        c.regptr = one_ptr; c.regidx = regidx.data();                         // a member, and no row to name
        EXPECT_ST(c.run(), GPV_ERR_INDEX);
        EXPECT(c.untouched());
    }
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    // ---- launches against the schedule
    {
        const long sweep = L + 1;                                             // (packing or normals) + the levels
        struct { int64_t chunk, col0, ndraws; bool given_Z; int regs, nthr; long launches; } cases[] = {
            // regs 0: none; 1: the four regions (fold + join); 2: one region of one chunk (fold); 3: one empty region (join)
            {0, 0, 2, false, 1, 3, 1 + sweep + 1 + 1 * (sweep + 3) + 1},
            {0, 0, 16, false, 1, 0, 1 + sweep + 1 + 1 * (sweep + 3) + 1},
            {0, 0, 17, true, 1, 8, 1 + 1 + sweep + 1 + 2 * (sweep + 3) + 1},        // one launch packs the given column
            {0, 15, 2, false, 2, 3, 1 + sweep + 1 + 2 * (sweep + 2) + 1},          // draws 15 and 16: two batches
            {0, 17, 33, false, 3, 3, 1 + sweep + 1 + 3 * (sweep + 2) + 1},         // batches 1, 2 and 3
            {0, 32, 16, false, 0, 3, 1 + sweep + 1 + 1 * (sweep + 1) + 1},
            {100, 0, 2, false, 0, 0, 7 + sweep + 1 + 1 * (sweep + 1) + 1},         // 700 rows in chunks of 100
            {299, 0, 2, true, 1, 1, 1 + 3 + sweep + 1 + 1 * (sweep + 3) + 1}};
        for (auto &k : cases) {
            Call c = base();
            c.Z = k.given_Z ? Zc.data() : nullptr;
            c.col0 = k.col0; c.ndraws = k.ndraws; c.nthr = k.nthr; c.offset = (k.regs & 1) ? off.data() : nullptr;
            if (k.regs == 0) { c.nreg = 0; c.regptr = nullptr; c.regidx = nullptr; c.regw = nullptr; }
            if (k.regs == 2) { c.nreg = 1; c.regptr = one_ptr; c.regidx = regidx.data() + 700; c.regw = nullptr; }
            if (k.regs == 3) { c.nreg = 1; c.regptr = empty_ptr; c.regidx = nullptr; c.regw = nullptr; }
            EXPECT_ST(gpv_plan_debug_csim_chunk(pl, k.chunk), GPV_OK);
            const long b = mockhip_launches();
            EXPECT_ST(c.run(), GPV_OK);
            if (mockhip_launches() - b != k.launches)
                std::fprintf(stderr, "chunk %lld col0 %lld ndraws %lld regs %d: %ld launches, wanted %ld\n", (long long)k.chunk, (long long)k.col0,
                             (long long)k.ndraws, k.regs, mockhip_launches() - b, k.launches);
            EXPECT(mockhip_launches() - b == k.launches && c.nf == 0 && c.nlev == want_levels && c.nlaunch == L);
            EXPECT(c.written());
            std::unique_ptr<double[]> ms(new double[4]);
            std::fill_n(ms.get(), 4, -1.0);
            EXPECT_ST(gpv_plan_debug_csim_summary_ms(pl, ms.get()), GPV_OK);
            EXPECT(ms[0] >= 0.0 && ms[1] >= 0.0 && ms[2] >= 0.0 && ms[3] >= 0.0);
        }
        EXPECT_ST(gpv_plan_debug_csim_chunk(pl, 0), GPV_OK);
        // gpv_plan_cond_sim launches what it did: the factor pass + (1 + batches) x (packing or normals, the levels, unpacking)
        struct { int64_t chunk, col0, nsim; long launches; } old[] = {
            {0, 0, 0, 1 + (L + 2)}, {0, 0, 16, 1 + 2 * (L + 2)}, {0, 15, 2, 1 + 3 * (L + 2)}, {100, 0, 1, 7 + 2 * (L + 2)}};
        for (auto &k : old) {
            const int64_t nd = k.nsim;
            std::unique_ptr<double[]> mean(new double[(size_t)nq]), dev(new double[(size_t)(nq * (nd ? nd : 1))]), sd(new double[(size_t)nq]);
            int64_t nlev = -1, nlaunch = -1, nf = -1;
            EXPECT_ST(gpv_plan_debug_csim_chunk(pl, k.chunk), GPV_OK);
            const long b = mockhip_launches();
            EXPECT_ST(gpv_plan_cond_sim(pl, "matern", cp, 3, &tau, 1, nullptr, 0, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5,
                                        k.col0, k.nsim, mean.get(), nq, dev.get(), nq, sd.get(), &nlev, &nlaunch, &nf), GPV_OK);
            EXPECT(mockhip_launches() - b == k.launches && nlev == want_levels && nlaunch == L);
        }
        EXPECT_ST(gpv_plan_debug_csim_chunk(pl, 0), GPV_OK);
    }
    // ---- the library's search (the mock's device memory holds zeros: every list comes back empty, one level); links
    {
        std::vector<unsigned char> el((size_t)n, 1);
        for (int64_t i = 0; i < n; i += 3) el[(size_t)i] = 0;
        const double sc2[2] = {0.1, 0.3}, cps[4] = {1.0, 0.1, 0.3, 2.5};
        Call c = base();
        c.nn = nullptr; c.elig = el.data(); c.link = 1;
        EXPECT_ST(c.run(), GPV_OK);
        EXPECT(c.written() && c.nlev == 1 && c.nlaunch == 1);
        c.cov = "matern_scaledim"; c.par = cps; c.npar = 4; c.scale = sc2; c.link = 2;
        EXPECT_ST(c.run(), GPV_OK);
        EXPECT(c.written());
    }
    // ---- an evaluation stays what it was
    {
        double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
        int64_t st0 = -1, st1 = -2;
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
        EXPECT_ST(gpv_plan_factor_stamp(pl, &st0), GPV_OK);
        Call c = base();
        EXPECT_ST(c.run(), GPV_OK);
        EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
        EXPECT_ST(gpv_plan_factor_stamp(pl, &st1), GPV_OK);
        for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
        EXPECT(st0 == st1);
        std::vector<double> Lent((size_t)n * p);
        EXPECT_ST(gpv_plan_get_Lentries(pl, Lent.data()), GPV_OK);
    }
    // ---- state: unobserved locations, a row shard, neighbours conditioned on as latent y
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    REFUSED(GPV_ERR_STATE, (void)0);
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        REFUSED(GPV_ERR_STATE, (void)0);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        REFUSED(GPV_ERR_STATE, (void)0);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("csim_summary_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail, mockhip_launches());
    return g_fail ? 1 : 0;
}
