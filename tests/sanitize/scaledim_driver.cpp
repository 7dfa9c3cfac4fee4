// tests/sanitize/scaledim_driver.cpp — TEST INFRASTRUCTURE: the HOST code of covType "matern_scaledim" (one range per coordinate,
// include/gpvecchia.h) under AddressSanitizer + UBSan, a stand-alone program linked like tests/sanitize/loglik_rep_driver.cpp
// against tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  Kernels do not run, so this checks the argument checks
// and refusals of the family at the C ABI with a plan in hand (wrong count, a range <= 0 or infinite, a smoothness no entry
// takes, more than three coordinates into the gradient-type entries, more than eight into an evaluation), that a refused call
// writes and launches nothing, that an evaluation of this family enqueues exactly one launch more than 'matern' (the scaled
// copy) at EVERY evaluation, the shape of what the gradient-type entries write in 1, 2 and 3 dimensions (NaN exactly in the
// smoothness slots, guard entries behind grad, fisher and row_terms untouched), and that nothing is left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_scaledim_driver.py and tools/sanitize_host.sh.
#include "../../include/gpvecchia.h"

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

extern "C" long mockhip_launches(void);
extern "C" long mockhip_live_allocations(void);

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

static const char *FAM = "matern_scaledim";

// rows of the m previous points, conditioned on as observations; own point last
static void make_rows(int64_t n, int p, std::vector<int> &revNN, std::vector<int> &revCond)
{
    revNN.assign((size_t)n * p, 0);
    revCond.assign((size_t)n * p, INT_MIN);
    for (int64_t k = 0; k < n; ++k)
        for (int j = 0; j < p; ++j) {
            const int64_t v = k - (p - 1 - j);
            if (v < 0) continue;
            revNN[(size_t)(k + (int64_t)j * n)] = (int)v + 1;
            revCond[(size_t)(k + (int64_t)j * n)] = (j == p - 1) ? 1 : 0;
        }
}

struct Case {
    gpv_plan *pl = nullptr;
    std::vector<double> locs, z, Z;
};

static void make_plan(Case &c, int64_t n, int dim, int p, int R)
{
    std::mt19937_64 rng(9 + dim);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    c.locs.resize((size_t)n * dim);
    c.z.resize((size_t)n);
    c.Z.resize((size_t)n * R);
    for (auto &v : c.locs) v = U(rng);
    for (auto &v : c.z) v = U(rng) - 0.5;
    for (auto &v : c.Z) v = U(rng) - 0.5;
    std::vector<int> revNN, revCond;
    make_rows(n, p, revNN, revCond);
    EXPECT_ST(gpv_plan_create(&c.pl, 0, n, dim, p, c.locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!c.pl) std::exit(1);
    EXPECT_ST(gpv_plan_set_data(c.pl, c.z.data()), GPV_OK);
    EXPECT_ST(gpv_plan_set_replicates(c.pl, c.Z.data(), n, R), GPV_OK);
}

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);      // developer build: wait for the (mock) stream, not for a number no kernel will write
    const int64_t n = 200;
    const int p = 11, R = 3;
    const double tau = 0.1, guard = -7.0, inf = std::numeric_limits<double>::infinity();
    const double cpm[3] = {1.0, 0.1, 1.5};
    double ll = guard;
    int64_t nf = -1;

    // ---- evaluation, two coordinates
    Case c2;
    make_plan(c2, n, 2, p, R);
    gpv_plan *pl = c2.pl;
    const double cp2[4] = {1.0, 0.1, 0.4, 1.5}, cp2b[4] = {0.7, 0.3, 0.05, 0.8};
    long l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_eval(pl, "matern", cpm, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    const long per_matern = mockhip_launches() - l0;
    for (int rep = 0; rep < 3; ++rep) {                                // the copy is written at EVERY evaluation
        l0 = mockhip_launches();
        EXPECT_ST(gpv_plan_eval(pl, FAM, rep == 1 ? cp2b : cp2, 4, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
        EXPECT(mockhip_launches() - l0 == per_matern + (rep == 1 ? 1 : 0) + 1);   // (a general smoothness also fits its table)
    }
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_eval(pl, "matern", cpm, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    EXPECT(mockhip_launches() - l0 == per_matern);                     // 'matern' enqueues what it enqueued
    double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
    EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
    // refusals of the family itself, from an evaluating entry: nothing is launched
    l0 = mockhip_launches();
    const double bad0[4] = {1.0, 0.1, 0.0, 1.5}, badn[4] = {1.0, -0.1, 0.4, 1.5}, badi[4] = {1.0, 0.1, inf, 1.5},
                 badnu[4] = {1.0, 0.1, 0.4, 0.0}, cp3x[5] = {1.0, 0.1, 0.4, 0.2, 1.5};
    EXPECT_ST(gpv_plan_eval(pl, FAM, cpm, 3, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_eval(pl, FAM, cp3x, 5, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_eval(pl, FAM, bad0, 4, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_eval(pl, FAM, badn, 4, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_eval(pl, FAM, badi, 4, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_eval(pl, FAM, badnu, 4, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_ERR_UNSUPPORTED_NU);
    EXPECT_ST(gpv_plan_eval(pl, "matern_scaled", cp2, 4, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_ERR_COVTYPE);
    EXPECT(mockhip_launches() == l0);

    // ---- the gradient-type entries, two coordinates: np = 5 outputs, T = 15
    {
        const int np = 5, T = 15, ld_g = np + 1, ld_f = np + 1 + T;
        std::vector<double> grad(np + 2, guard), fi(np * np + 2, guard), rows((size_t)n * ld_f + 4, guard);
        double *g = grad.data(), *f = fi.data();
        l0 = mockhip_launches();
        EXPECT_ST(gpv_plan_loglik_grad(pl, FAM, cp2b, 4, tau, &ll, g, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(gpv_plan_loglik_grad_nu(pl, FAM, cp2b, 4, tau, &ll, g, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);   // not differentiated
        EXPECT_ST(gpv_plan_loglik_fisher(pl, FAM, cp2b, 4, tau, &ll, g, f, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(gpv_plan_loglik_fisher_nu(pl, FAM, cp2b, 4, tau, &ll, g, f, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(gpv_plan_loglik_rep(pl, FAM, cp2b, 4, tau, &ll, g, f, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(gpv_plan_loglik_rep_nu(pl, FAM, cp2b, 4, tau, &ll, g, f, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(gpv_plan_loglik_grad(pl, FAM, cpm, 3, tau, &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_plan_loglik_fisher(pl, FAM, cp3x, 5, tau, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_plan_loglik_rep(pl, FAM, bad0, 4, tau, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_plan_loglik_grad(pl, FAM, badi, 4, tau, &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_plan_loglik_grad(pl, FAM, cp2, 4, 0.0, &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
        EXPECT(mockhip_launches() == l0 && ll == guard && nf == -1 && grad[0] == guard && fi[0] == guard);
        EXPECT_ST(gpv_plan_loglik_grad(pl, FAM, cp2, 4, tau, &ll, g, &nf, rows.data()), GPV_OK);
        EXPECT(mockhip_launches() - l0 == 3);                         // the scaled copy, the set pass, the fixed-order sum
        EXPECT(std::isnan(grad[3]) && !std::isnan(grad[0]) && !std::isnan(grad[1]) && !std::isnan(grad[2]) && !std::isnan(grad[4]));
        EXPECT(grad[np] == guard && rows[(size_t)n * ld_g] == guard);
        for (int64_t k = 0; k < n; ++k) EXPECT(std::isnan(rows[(size_t)(k * ld_g + 4)]) && !std::isnan(rows[(size_t)(k * ld_g + 5)]));
        EXPECT_ST(gpv_plan_loglik_fisher(pl, FAM, cp2, 4, tau, &ll, g, f, &nf, rows.data()), GPV_OK);
        EXPECT_ST(gpv_plan_loglik_rep(pl, FAM, cp2, 4, tau, &ll, g, f, &nf, rows.data()), GPV_OK);
        EXPECT_ST(gpv_plan_loglik_rep_nu(pl, FAM, cp2, 4, tau, &ll, g, nullptr, &nf, nullptr), GPV_OK);
        for (int i = 0; i < np; ++i)
            for (int j = 0; j < np; ++j) {                             // NaN in the row and column of the smoothness, symmetric
                EXPECT(std::isnan(fi[i * np + j]) == (i == 3 || j == 3));
                if (i != 3 && j != 3) EXPECT(fi[i * np + j] == fi[j * np + i]);
            }
        EXPECT(fi[np * np] == guard && grad[np] == guard && rows[(size_t)n * ld_f] == guard);
        EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);               // the last evaluation stays what it was
        for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t] || (std::isnan(sums0[t]) && std::isnan(sums1[t])));
    }
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);

    // ---- one and three coordinates: np = 4 and 6 (the information of three coordinates has 21 triangle entries)
    for (int dim : {1, 3}) {
        Case c;
        make_plan(c, n, dim, p, R);
        const int ncov = dim + 2, np = dim + 3, T = np * (np + 1) / 2, ld_f = np + 1 + T;
        // covparms on the heap, exactly ncov doubles: a read of covparms[ncov] (one dimension: covparms[3]) is a sanitizer report
        const std::vector<double> cpv = dim == 1 ? std::vector<double>{1.0, 0.1, 2.5} : std::vector<double>{1.0, 0.1, 0.4, 0.2, 2.5};
        const double *cp = cpv.data();
        EXPECT((int)cpv.size() == ncov);
        std::vector<double> grad(np + 2, guard), fi(np * np + 2, guard), rows((size_t)n * ld_f + 4, guard);
        EXPECT_ST(gpv_plan_eval(c.pl, FAM, cp, ncov, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_loglik_grad(c.pl, FAM, cp, ncov, tau, &ll, grad.data(), &nf, rows.data()), GPV_OK);
        EXPECT(std::isnan(grad[dim + 1]) && grad[np] == guard && rows[(size_t)n * (np + 1)] == guard);
        EXPECT_ST(gpv_plan_loglik_fisher(c.pl, FAM, cp, ncov, tau, &ll, grad.data(), fi.data(), &nf, rows.data()), GPV_OK);
        EXPECT_ST(gpv_plan_loglik_rep(c.pl, FAM, cp, ncov, tau, &ll, grad.data(), fi.data(), &nf, rows.data()), GPV_OK);
        int nans = 0;
        for (int t = 0; t < np * np; ++t) nans += std::isnan(fi[(size_t)t]) ? 1 : 0;
        EXPECT(nans == 2 * np - 1 && fi[(size_t)(np * np)] == guard && rows[(size_t)n * ld_f] == guard);
        for (int64_t k = 0; k < n; ++k) {
            int rn = 0;
            for (int t = 0; t < ld_f; ++t) rn += std::isnan(rows[(size_t)(k * ld_f + t)]) ? 1 : 0;
            EXPECT(rn == 1 + np);                                     // the smoothness: its derivative and its np triangle entries
        }
        EXPECT_ST(gpv_plan_destroy(c.pl), GPV_OK);
    }

    // ---- five coordinates: evaluation only (the coordinate array); nine: more inverse ranges than a launch carries
    {
        Case c;
        make_plan(c, n, 5, p, R);
        const double cp5[7] = {1.0, 0.1, 0.4, 0.2, 0.3, 0.5, 1.5};
        std::vector<double> grad(10, guard), fi(70, guard);
        l0 = mockhip_launches();
        EXPECT_ST(gpv_plan_loglik_grad(c.pl, FAM, cp5, 7, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_loglik_fisher(c.pl, FAM, cp5, 7, tau, &ll, grad.data(), fi.data(), &nf, nullptr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_loglik_rep(c.pl, FAM, cp5, 7, tau, &ll, grad.data(), fi.data(), &nf, nullptr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_loglik_grad_nu(c.pl, FAM, cp5, 7, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);
        EXPECT(mockhip_launches() == l0 && grad[0] == guard && fi[0] == guard);
        EXPECT_ST(gpv_plan_eval(c.pl, FAM, cp5, 7, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_eval(c.pl, FAM, cp5, 6, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_plan_destroy(c.pl), GPV_OK);
        Case c9;
        make_plan(c9, n, 9, p, R);
        std::vector<double> cp9(11, 0.3);
        cp9[10] = 1.5;
        EXPECT_ST(gpv_plan_eval(c9.pl, FAM, cp9.data(), 11, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_plan_destroy(c9.pl), GPV_OK);
    }
    EXPECT_ST(gpv_plan_cache_clear(), GPV_OK);
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("scaledim_driver: %d failed expectation(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
