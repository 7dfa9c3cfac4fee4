// tests/sanitize/loglik_grad_nu_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_loglik_grad_nu, gpv_plan_loglik_fisher_nu
// and gpv_matern_derivs_host (include/gpvecchia.h) under AddressSanitizer + UBSan, a stand-alone program linked like
// tests/sanitize/loglik_fisher_driver.cpp against tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  Kernels do not
// run, so this checks the argument checks and state refusals, that a refused call writes and launches nothing, the shape of what
// is written at a general smoothness (nothing NaN-masked, guard entries behind grad, fisher and row_terms untouched, fisher
// symmetric), the launches of a call (table fit, set pass, fixed-order sum), that the old entries keep refusing, that the plan's
// last evaluation is left alone and that nothing is left allocated.  The pair functions run on the host: their values at the ends
// of the argument range are checked for what they must be exactly.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_loglik_grad_nu_driver.py and tools/sanitize_host.sh.
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

// rows of the m previous points, the own point last (tests/sanitize/loglik_fisher_driver.cpp)
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

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);      // developer build: wait for the (mock) stream, not for a number no kernel will write
    const int64_t n = 200;
    const int dim = 2, p = 11;
    std::mt19937_64 rng(9);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> locs((size_t)n * dim), z((size_t)n);
    for (auto &v : locs) v = U(rng);
    for (auto &v : z) v = U(rng) - 0.5;
    std::vector<int> revNN, revCond;
    make_rows(n, p, false, revNN, revCond);
    const double cp[3] = {1.0, 0.1, 1.5}, cp08[3] = {1.0, 0.1, 0.8}, cp61[3] = {1.0, 0.1, 61.0}, ce[4] = {0.8, 0.1, 0.5, 0.2};
    const double tau = 0.1, guard = -7.0, inf = std::numeric_limits<double>::infinity();
    const int ldm = 5 + 10;                                           // row_terms of the information entry: ncovparms + 2 + T
    double ll = guard;
    int64_t nf = -1;
    std::vector<double> grad(6, guard), fi(26, guard), rows((size_t)n * ldm + 4, guard);
    double *g = grad.data(), *f = fi.data();

    // ---- the pair functions on the host
    {
        const double s[6] = {0.0, 1e-10, 1.0, 800.0, 5e3, 1e-30};
        double out[18];
        const double nus[4] = {0.3, 0.8, 2.2, 30.0};
        for (double nu : nus) {
            for (double &v : out) v = guard;
            EXPECT_ST(gpv_matern_derivs_host(nu, 0.5, s, 6, out), GPV_OK);
            EXPECT(out[0] == 1.0 && out[1] == 0.0 && out[2] == 0.0);                           // r = 0
            for (int t = 9; t < 15; ++t) EXPECT(out[t] == 0.0);                                // e^-s underflows
            for (double v : out) EXPECT(std::isfinite(v));
            EXPECT(out[6] > 0.0 && out[6] < 1.0 && out[7] > 0.0);
        }
        EXPECT_ST(gpv_matern_derivs_host(0.8, 0.5, nullptr, 6, out), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_matern_derivs_host(0.8, 0.5, s, 6, nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_matern_derivs_host(0.8, 0.5, s, -1, out), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_matern_derivs_host(0.8, 0.0, s, 6, out), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_matern_derivs_host(0.8, inf, s, 6, out), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_matern_derivs_host(0.0, 0.5, s, 6, out), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(gpv_matern_derivs_host(61.0, 0.5, s, 6, out), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(gpv_matern_derivs_host(std::nan(""), 0.5, s, 6, out), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(gpv_matern_derivs_host(0.8, 0.5, nullptr, 0, nullptr), GPV_OK);
    }

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    // ---- arguments, before the state is looked at
    EXPECT_ST(gpv_plan_loglik_grad_nu(nullptr, "matern", cp08, 3, tau, &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, nullptr, cp08, 3, tau, &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", nullptr, 3, tau, &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, nullptr, g, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, &ll, nullptr, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, &ll, g, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_fisher_nu(pl, "matern", cp08, 3, tau, &ll, g, nullptr, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 2, tau, &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 4, tau, &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_fisher_nu(pl, "esqe", ce, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, 0.0, &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_fisher_nu(pl, "matern", cp08, 3, inf, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, std::nan(""), &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "gauss", cp08, 3, tau, &ll, g, &nf, nullptr), GPV_ERR_COVTYPE);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp61, 3, tau, &ll, g, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
    EXPECT_ST(gpv_plan_loglik_fisher_nu(pl, "matern", cp61, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
    // ---- state
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, &ll, g, &nf, rows.data()), GPV_ERR_STATE);      // no data
    EXPECT_ST(gpv_plan_loglik_fisher_nu(pl, "matern", cp08, 3, tau, &ll, g, f, &nf, rows.data()), GPV_ERR_STATE);
    EXPECT(ll == guard && nf == -1 && grad[0] == guard && fi[0] == guard && rows[0] == guard);  // a refused call writes nothing
    EXPECT(mockhip_launches() == 0);                                                           // ... and launches nothing
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp08, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
    int64_t stamp0 = -1, stamp1 = -1;
    EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    long l0 = mockhip_launches();
    // the old entries keep refusing a general smoothness
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp08, 3, tau, &ll, g, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
    EXPECT_ST(gpv_plan_loglik_fisher(pl, "matern", cp08, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, -1.0, &ll, g, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT(mockhip_launches() == l0 && ll == guard && grad[0] == guard);
    // ---- a general smoothness: the table fit, the set pass, the fixed-order sum
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, &ll, g, &nf, nullptr), GPV_OK);
    EXPECT(mockhip_launches() - l0 == 3);
    EXPECT(nf == 0 && grad[4] == guard);
    for (int t = 0; t < 4; ++t) EXPECT(!std::isnan(grad[t]) && grad[t] != guard);             // all four written, none masked
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_loglik_fisher_nu(pl, "matern", cp08, 3, tau, &ll, g, f, &nf, rows.data()), GPV_OK);
    EXPECT(mockhip_launches() - l0 == 3);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) EXPECT(!std::isnan(fi[i * 4 + j]) && fi[i * 4 + j] != guard && fi[i * 4 + j] == fi[j * 4 + i]);
    for (size_t t = 16; t < fi.size(); ++t) EXPECT(fi[t] == guard);
    for (size_t t = 0; t < (size_t)n * ldm; ++t) EXPECT(!std::isnan(rows[t]) && rows[t] != guard);
    for (size_t t = (size_t)n * ldm; t < rows.size(); ++t) EXPECT(rows[t] == guard);
    for (auto &v : rows) v = guard;
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, &ll, g, &nf, rows.data()), GPV_OK);
    for (size_t t = 0; t < (size_t)n * 5; ++t) EXPECT(!std::isnan(rows[t]) && rows[t] != guard);
    for (size_t t = (size_t)n * 5; t < rows.size(); ++t) EXPECT(rows[t] == guard);
    // without the tables (the switch is read at every call): one launch fewer
    setenv("GPV_NO_MATERN_TABLE", "1", 1);
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, &ll, g, &nf, nullptr), GPV_OK);
    EXPECT(mockhip_launches() - l0 == 2);
    unsetenv("GPV_NO_MATERN_TABLE");
    // ---- a closed form and esqe through the new entries: what the old entries write
    for (auto &v : grad) v = guard;
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp, 3, tau, &ll, g, &nf, nullptr), GPV_OK);
    EXPECT(mockhip_launches() - l0 == 2);                                                      // no table
    EXPECT(std::isnan(grad[2]) && !std::isnan(grad[3]) && grad[4] == guard);
    EXPECT_ST(gpv_plan_loglik_fisher_nu(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_OK);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) EXPECT(std::isnan(fi[i * 4 + j]) == (i == 2 || j == 2));
    EXPECT_ST(gpv_plan_loglik_fisher_nu(pl, "esqe", ce, 4, tau, &ll, g, f, &nf, nullptr), GPV_OK);
    for (int t = 0; t < 25; ++t) EXPECT(!std::isnan(fi[t]) && fi[t] != guard);
    EXPECT(grad[5] == guard && fi[25] == guard);
    // ---- the plan's last evaluation
    EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
    EXPECT(stamp0 == stamp1);
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, &ll, g, &nf, nullptr), GPV_ERR_STATE);          // unobserved locations
    EXPECT(mockhip_launches() == l0);
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, &ll, g, &nf, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    // a row shard
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
        l0 = mockhip_launches();
        EXPECT_ST(gpv_plan_loglik_fisher_nu(pl, "matern", cp08, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_STATE);
        EXPECT(mockhip_launches() == l0);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // neighbours conditioned on as latent y
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
        l0 = mockhip_launches();
        EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, &ll, g, &nf, nullptr), GPV_ERR_STATE);
        EXPECT(mockhip_launches() == l0);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // m + 1 = 65
    std::vector<int> nnW, cdW;
    make_rows(n, 65, false, nnW, cdW);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, 65, locs.data(), nnW.data(), cdW.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
        l0 = mockhip_launches();
        EXPECT_ST(gpv_plan_loglik_grad_nu(pl, "matern", cp08, 3, tau, &ll, g, &nf, nullptr), GPV_ERR_UNSUPPORTED_M);
        EXPECT(mockhip_launches() == l0);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("loglik_grad_nu_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail,
                mockhip_launches());
    return g_fail ? 1 : 0;
}
