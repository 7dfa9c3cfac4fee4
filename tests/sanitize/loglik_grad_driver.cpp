// tests/sanitize/loglik_grad_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_loglik_grad (include/gpvecchia.h)
// under AddressSanitizer + UBSan, linked like tests/sanitize/host_driver.cpp against tests/sanitize/mock_hip_runtime.cpp instead
// of the HIP runtime.  Kernels do not run, so this checks the argument checks, the state errors, the shape of what is written
// (guard entries behind grad and row_terms stay untouched), that the plan's last evaluation is left alone and that nothing is
// left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_host_drivers.py and tools/sanitize_host.sh.
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

// rows of the m previous points (not the nearest: the structure is all the host code looks at); latent: the neighbours are
// conditioned on as latent y (a cond.yz = 'y' plan), else as observations (cond.yz = 'z'); the own point comes last
static void make_rows(int64_t n, int p, bool latent, std::vector<int> &revNN, std::vector<int> &revCond)
{
    revNN.assign((size_t)n * p, 0);
    revCond.assign((size_t)n * p, INT_MIN);
    for (int64_t k = 0; k < n; ++k)
        for (int j = 0; j < p; ++j) {
            const int64_t v = k - (p - 1 - j);                       // column p - 1: the point itself
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
    const double cp[3] = {1.0, 0.1, 1.5}, cp08[3] = {1.0, 0.1, 0.8}, ce[4] = {0.8, 0.1, 0.5, 0.2};
    const double tau = 0.1, guard = -7.0;
    double ll = guard;
    int64_t nf = -1;
    std::vector<double> grad(6, guard), rows((size_t)n * 6 + 4, guard);

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    // ---- arguments, before the state is looked at
    EXPECT_ST(gpv_plan_loglik_grad(nullptr, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, nullptr, cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", nullptr, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, nullptr, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, nullptr, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, grad.data(), nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 2, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 4, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "esqe", ce, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, 0.0, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, -1.0, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, std::numeric_limits<double>::infinity(), &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, std::nan(""), &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "gauss", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_COVTYPE);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp08, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
    // ---- state
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);     // no data
    EXPECT(ll == guard && nf == -1 && grad[0] == guard);                                       // a refused call writes nothing
    EXPECT(mockhip_launches() == 0);                                                           // ... and launches nothing
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
    int64_t stamp0 = -1, stamp1 = -1;
    EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    const long l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_OK);
    EXPECT(mockhip_launches() - l0 == 2);                                                      // the set pass and the fixed-order sum
    EXPECT(nf == 0 && std::isnan(grad[2]) && grad[4] == guard);                                // ncovparms + 1 entries, nu not differentiated
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, rows.data()), GPV_OK);
    for (int64_t k = 0; k < n; ++k) EXPECT(std::isnan(rows[(size_t)(k * 5 + 3)]));             // Nlocs x (ncovparms + 2), row-major
    for (size_t t = (size_t)n * 5; t < rows.size(); ++t) EXPECT(rows[t] == guard);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "esqe", ce, 4, tau, &ll, grad.data(), &nf, rows.data()), GPV_OK);
    EXPECT(grad[5] == guard);
    for (size_t t = (size_t)n * 6; t < rows.size(); ++t) EXPECT(rows[t] == guard);
    EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
    EXPECT(stamp0 == stamp1);
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);     // unobserved locations
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    // a row shard
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
        EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // neighbours conditioned on as latent y
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
        EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // m + 1 = 65
    std::vector<int> nnW, cdW;
    make_rows(n, 65, false, nnW, cdW);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, 65, locs.data(), nnW.data(), cdW.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
        EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_UNSUPPORTED_M);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("loglik_grad_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail,
                mockhip_launches());
    return g_fail ? 1 : 0;
}
