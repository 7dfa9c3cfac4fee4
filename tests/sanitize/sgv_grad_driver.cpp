// tests/sanitize/sgv_grad_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_loglik_grad_sgv (include/gpvecchia.h) under
// AddressSanitizer + UBSan, linked like tests/sanitize/selinv_driver.cpp against tests/sanitize/mock_hip_runtime.cpp instead of
// the HIP runtime.  Kernels do not run, so this checks the statuses, with and without a plan in hand, the index records built
// at first use from the arrays the plan keeps on the "device" (their bounds under ASan), the shape of what is written (guard
// entries stay), the evaluation the call makes (factor stamp), a repeat after gpv_plan_build_posterior, and that nothing is
// left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_sgv_grad_driver.py and tools/sanitize_host.sh.
#include "../../include/gpvecchia.h"

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

// every row conditions on the points k - off[t] and on itself (row length p = off.size() + 1, offsets descending): as latent y
// where off[t] <= latent_upto, as observed z beyond
static void make_rows(int64_t n, const std::vector<int> &off, int latent_upto, std::vector<int> &revNN, std::vector<int> &revCond)
{
    const int p = (int)off.size() + 1;
    revNN.assign((size_t)n * p, 0);
    revCond.assign((size_t)n * p, INT_MIN);
    for (int64_t k = 0; k < n; ++k)
        for (int j = 0; j < p; ++j) {
            const int64_t v = j == p - 1 ? k : k - off[(size_t)j];
            if (v < 0) continue;
            revNN[(size_t)(k + (int64_t)j * n)] = (int)v + 1;
            revCond[(size_t)(k + (int64_t)j * n)] = (j == p - 1 || off[(size_t)j] <= latent_upto) ? 1 : 0;
        }
}

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);      // developer build: wait for the (mock) stream, not for a number no kernel will write
    const int64_t n = 400;
    const int dim = 2;
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> locs((size_t)n * dim), z((size_t)n);
    for (auto &v : locs) v = U(rng);
    for (auto &v : z) v = U(rng) - 0.5;
    const double cp[3] = {1.0, 0.1, 1.5}, cp_nu[3] = {1.0, 0.1, 0.8}, cp_sc[4] = {1.0, 0.1, 0.1, 1.5}, cp_e[4] = {0.8, 0.1, 0.5, 0.08};
    const double tau = 0.1, guard = -7.0;
    double ll = guard;
    std::vector<double> grad(4 + 2, guard), cols((size_t)n * 5 + 4, guard);
    int64_t nf = -1, stamp0 = 0, stamp1 = 0;

    // ---- a band of the 10 previous points, the nearest 5 conditioned on as latent y: the latent members of a set are
    // neighbours of each other, the selected inverse drops nothing
    std::vector<int> band;
    for (int t = 10; t >= 1; --t) band.push_back(t);
    std::vector<int> revNN, revCond;
    make_rows(n, band, 5, revNN, revCond);
    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, (int)band.size() + 1, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    // arguments, before the state is looked at
    EXPECT_ST(gpv_plan_loglik_grad_sgv(nullptr, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, nullptr, cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", nullptr, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, nullptr, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, nullptr, &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 2, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, 0.0, &ll, grad.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "gauss", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_COVTYPE);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp_nu, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern_scaledim", cp_sc, 4, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_UNSUPPORTED_NU);
    // state
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);      // no data
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);      // no structure
    EXPECT(ll == guard && nf == -1 && grad[0] == guard);                                     // a refused call writes nothing
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    EXPECT(stamp0 == 0);
    // the first call builds the index records and allocates; the next ones do not
    const long l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, cols.data()), GPV_OK);
    EXPECT(mockhip_launches() > l0);
    EXPECT(grad[3] != guard && grad[4] == guard && grad[5] == guard);                        // ncovparms + 1 values and no more
    for (size_t t = (size_t)n * 4; t < cols.size(); ++t) EXPECT(cols[t] == guard);           // Nlocs x (ncovparms + 1) and no more
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    EXPECT(stamp0 != 0);                                                                     // the call evaluated the plan
    const long a1 = mockhip_live_allocations();
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, cols.data()), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_OK);
    EXPECT(mockhip_live_allocations() == a1);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    EXPECT(stamp1 == stamp0 + 2);                                                            // one evaluation per call
    {   // what such an evaluation leaves can be read back, and the selected inverse follows it
        std::vector<double> sums(GPV_NSUMS), mu((size_t)n), vars((size_t)n);
        int64_t nd = -1;
        EXPECT_ST(gpv_plan_get_sums(pl, sums.data()), GPV_OK);
        EXPECT_ST(gpv_plan_get_posterior_mean(pl, mu.data()), GPV_OK);
        EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_OK);
        EXPECT(nd == 0);
    }
    // esqe: five outputs per column
    std::fill(cols.begin(), cols.end(), guard);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "esqe", cp_e, 4, tau, &ll, grad.data(), &nf, cols.data()), GPV_OK);
    EXPECT(grad[4] != guard && grad[5] == guard && cols[(size_t)n * 5 - 1] != guard && cols[(size_t)n * 5] == guard);
    // a rebuilt structure: the records are built again
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, cols.data()), GPV_OK);
    // the filled structure of the same rows is refused, and so is the plan once it has unobserved locations
    double ratio = 0.0;
    EXPECT_ST(gpv_plan_build_posterior_fill(pl, revNN.data(), revCond.data(), 8.0, &ratio), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_OK);
    {
        std::vector<int> obs((size_t)n, 1);
        obs[5] = 0;
        EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
        EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_OK);
    }
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    EXPECT(mockhip_live_allocations() == 0);

    // ---- a row shard: refused
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, (int)band.size() + 1, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
        EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // ---- rows that condition on k - 7, k - 3 and k - 1 as latent y: the selected inverse of that structure drops terms
    {
        std::vector<int> nn2, cd2;
        make_rows(n, {7, 3, 1}, 7, nn2, cd2);
        pl = nullptr;
        EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, 4, locs.data(), nn2.data(), cd2.data(), 0, n), GPV_OK);
        if (pl) {
            EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
            EXPECT_ST(gpv_plan_build_posterior(pl, nn2.data(), cd2.data()), GPV_OK);
            EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
            EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, nullptr), GPV_ERR_STATE);
            EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
            EXPECT(stamp1 == stamp0);                                                        // refused before any evaluation
            EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
        }
    }
    // ---- no latent neighbour at all (cond.yz = 'z' with a structure) and no neighbours at all (m = 0): diagonal W, accepted
    for (int m0 : {10, 0}) {
        std::vector<int> off, nn3, cd3;
        for (int t = m0; t >= 1; --t) off.push_back(t);
        make_rows(n, off, 0, nn3, cd3);
        pl = nullptr;
        EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, m0 + 1, locs.data(), nn3.data(), cd3.data(), 0, n), GPV_OK);
        if (pl) {
            EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
            EXPECT_ST(gpv_plan_build_posterior(pl, nn3.data(), cd3.data()), GPV_OK);
            EXPECT_ST(gpv_plan_loglik_grad_sgv(pl, "matern", cp, 3, tau, &ll, grad.data(), &nf, cols.data()), GPV_OK);
            EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
        }
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("sgv_grad_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail,
                mockhip_launches());
    return g_fail ? 1 : 0;
}
