// tests/sanitize/loglik_rep_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_set_replicates, gpv_plan_replicates,
// gpv_plan_loglik_rep and gpv_plan_loglik_rep_nu (include/gpvecchia.h) under AddressSanitizer + UBSan, a stand-alone program
// linked like tests/sanitize/loglik_fisher_driver.cpp against tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.
// Kernels do not run, so this checks every argument check and state refusal, that a refused call writes and launches nothing,
// that the upload reads exactly Nlocs rows of each column (the columns sit at the end of a heap block: one row more is a
// sanitizer report), the shape of what is written (guard entries behind grad, fisher and row_terms stay untouched, fisher may be
// NULL), that the plan's data column and last evaluation are left alone and that nothing is left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_loglik_rep_driver.py and tools/sanitize_host.sh.
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

// rows of the m previous points; latent: the neighbours are conditioned on as latent y, else as observations; own point last
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
    const int64_t n = 200, ldz = n + 5;
    const int dim = 2, p = 11, R = 17;
    std::mt19937_64 rng(9);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> locs((size_t)n * dim), z((size_t)n);
    for (auto &v : locs) v = U(rng);
    for (auto &v : z) v = U(rng) - 0.5;
    // R columns ldz apart, the last one exactly n long: the block ends with the last row that may be read
    std::vector<double> Z((size_t)ldz * (R - 1) + n);
    for (auto &v : Z) v = U(rng) - 0.5;
    std::vector<int> revNN, revCond;
    make_rows(n, p, false, revNN, revCond);
    const double cp[3] = {1.0, 0.1, 1.5}, cp08[3] = {1.0, 0.1, 0.8}, ce[4] = {0.8, 0.1, 0.5, 0.2};
    const double tau = 0.1, guard = -7.0, inf = std::numeric_limits<double>::infinity();
    const int ldm = 5 + 10, lde = 6 + 15;                             // row_terms: ncovparms + 2 + T doubles per row
    double ll = guard;
    int64_t nf = -1;
    int r = -1;
    std::vector<double> grad(6, guard), fi(26, guard), rows((size_t)n * lde + 4, guard);
    double *g = grad.data(), *f = fi.data();

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    // ---- gpv_plan_set_replicates / gpv_plan_replicates: arguments
    long l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_set_replicates(nullptr, Z.data(), ldz, R), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_set_replicates(pl, nullptr, ldz, R), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_set_replicates(pl, Z.data(), ldz, -1), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_set_replicates(pl, Z.data(), n - 1, R), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_replicates(nullptr, &r), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_replicates(pl, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_replicates(pl, &r), GPV_OK);
    EXPECT(r == 0 && mockhip_launches() == l0);
    // ---- gpv_plan_loglik_rep: arguments, before the state is looked at
    EXPECT_ST(gpv_plan_loglik_rep(nullptr, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, nullptr, cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", nullptr, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, nullptr, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, nullptr, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 2, tau, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "esqe", ce, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, 0.0, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, inf, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, std::nan(""), &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "gauss", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_COVTYPE);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp08, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
    EXPECT_ST(gpv_plan_loglik_rep_nu(nullptr, "matern", cp08, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);
    // ---- state: no replicates (a data column does not stand in for them)
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, rows.data()), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, rows.data()), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_loglik_rep_nu(pl, "matern", cp08, 3, tau, &ll, g, f, &nf, rows.data()), GPV_ERR_STATE);
    EXPECT(ll == guard && nf == -1 && grad[0] == guard && fi[0] == guard && rows[0] == guard);  // a refused call writes nothing
    EXPECT(mockhip_launches() == l0);                                                           // ... and launches nothing
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
    int64_t stamp0 = -1, stamp1 = -1;
    EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    // ---- upload: one packing launch; exactly n rows of each column are read
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_set_replicates(pl, Z.data(), ldz, R), GPV_OK);
    EXPECT(mockhip_launches() - l0 == 1);
    EXPECT_ST(gpv_plan_replicates(pl, &r), GPV_OK);
    EXPECT(r == R);
    const long live_R = mockhip_live_allocations();
    EXPECT_ST(gpv_plan_set_replicates(pl, Z.data(), ldz, 3), GPV_OK);                           // a second upload replaces the first
    EXPECT_ST(gpv_plan_replicates(pl, &r), GPV_OK);
    EXPECT(r == 3 && mockhip_live_allocations() == live_R);                                     // (the staging buffer is gone again)
    EXPECT_ST(gpv_plan_set_replicates(pl, Z.data(), n - 1, 3), GPV_ERR_BAD_ARG);                // a refused upload keeps the old one
    EXPECT_ST(gpv_plan_replicates(pl, &r), GPV_OK);
    EXPECT(r == 3);
    EXPECT_ST(gpv_plan_set_replicates(pl, Z.data(), ldz, R), GPV_OK);
    // ---- the call
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, -1.0, &ll, g, f, &nf, nullptr), GPV_ERR_BAD_ARG);         // refused with replicates set
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp08, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
    EXPECT(mockhip_launches() == l0 && ll == guard && fi[0] == guard);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, nullptr, &nf, nullptr), GPV_OK);             // fisher may be NULL
    EXPECT(mockhip_launches() - l0 == 2);                                                      // the set pass and the fixed-order sum
    EXPECT(nf == 0 && std::isnan(grad[2]) && grad[4] == guard && fi[0] == guard);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_OK);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {                                                          // NaN in the row and column of nu, symmetric
            EXPECT(std::isnan(fi[i * 4 + j]) == (i == 2 || j == 2));
            if (i != 2 && j != 2) EXPECT(fi[i * 4 + j] == fi[j * 4 + i]);
        }
    for (size_t t = 16; t < fi.size(); ++t) EXPECT(fi[t] == guard);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, rows.data()), GPV_OK);
    const int nan_at[5] = {3, 5 + 2, 5 + 5, 5 + 7, 5 + 8};
    for (int64_t k = 0; k < n; ++k) {
        int nans = 0;
        for (int t = 0; t < ldm; ++t) nans += std::isnan(rows[(size_t)(k * ldm + t)]) ? 1 : 0;
        EXPECT(nans == 5);
        for (int t : nan_at) EXPECT(std::isnan(rows[(size_t)(k * ldm + t)]));
    }
    for (size_t t = (size_t)n * ldm; t < rows.size(); ++t) EXPECT(rows[t] == guard);
    EXPECT_ST(gpv_plan_loglik_rep_nu(pl, "matern", cp08, 3, tau, &ll, g, f, &nf, nullptr), GPV_OK);              // a general smoothness
    for (int t = 0; t < 16; ++t) EXPECT(!std::isnan(fi[t]));
    EXPECT_ST(gpv_plan_loglik_rep(pl, "esqe", ce, 4, tau, &ll, g, f, &nf, rows.data()), GPV_OK);
    EXPECT(grad[5] == guard && fi[25] == guard);
    for (int t = 0; t < 25; ++t) EXPECT(!std::isnan(fi[t]) && fi[t] != guard);
    for (size_t t = 0; t < (size_t)n * lde; ++t) EXPECT(rows[t] != guard);
    for (size_t t = (size_t)n * lde; t < rows.size(); ++t) EXPECT(rows[t] == guard);
    // the one-column entries beside it, and the plan's last evaluation
    EXPECT_ST(gpv_plan_loglik_grad(pl, "matern", cp, 3, tau, &ll, g, &nf, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_fisher(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
    EXPECT(stamp0 == stamp1);
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_STATE);            // unobserved locations
    EXPECT(mockhip_launches() == l0);
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_OK);
    // R = 0 releases the buffer (Z_ord is not read): no replicates again, the data column still serves its own entries
    const long live = mockhip_live_allocations();
    EXPECT_ST(gpv_plan_set_replicates(pl, nullptr, 0, 0), GPV_OK);
    EXPECT(mockhip_live_allocations() == live - 1);
    EXPECT_ST(gpv_plan_replicates(pl, &r), GPV_OK);
    EXPECT(r == 0);
    EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_loglik_fisher(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_set_replicates(pl, Z.data(), ldz, R), GPV_OK);                           // destroyed with the plan
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    // a row shard: the upload is accepted, the call refused
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_set_replicates(pl, Z.data(), ldz, R), GPV_OK);
        l0 = mockhip_launches();
        EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_STATE);
        EXPECT(mockhip_launches() == l0);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // neighbours conditioned on as latent y
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_set_replicates(pl, Z.data(), ldz, R), GPV_OK);
        l0 = mockhip_launches();
        EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_STATE);
        EXPECT(mockhip_launches() == l0);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // m + 1 = 65
    std::vector<int> nnW, cdW;
    make_rows(n, 65, false, nnW, cdW);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, 65, locs.data(), nnW.data(), cdW.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_set_replicates(pl, Z.data(), ldz, R), GPV_OK);
        l0 = mockhip_launches();
        EXPECT_ST(gpv_plan_loglik_rep(pl, "matern", cp, 3, tau, &ll, g, f, &nf, nullptr), GPV_ERR_UNSUPPORTED_M);
        EXPECT(mockhip_launches() == l0);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("loglik_rep_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail,
                mockhip_launches());
    return g_fail ? 1 : 0;
}
