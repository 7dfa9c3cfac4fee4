// tests/sanitize/solve_t_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_solve_t (include/gpvecchia.h) under
// AddressSanitizer + UBSan, linked like tests/sanitize/host_driver.cpp against tests/sanitize/mock_hip_runtime.cpp instead of
// the HIP runtime.  Kernels do not run, so this checks statuses, the strided copies of E and X (guard columns stay
// untouched), batching, in-place use, graph lifetime across a rebuild, and that nothing is left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_host_drivers.py and tools/sanitize_host.sh.
#include "../../include/gpvecchia.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

extern "C" long mockhip_launches(void);
extern "C" long mockhip_graph_launches(void);
extern "C" long mockhip_live_allocations(void);
extern "C" int gpv_plan_debug_solve_t_ms(gpv_plan *pl, int reps, double *ms);      // developer aid, not in the public header

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

int main()
{
    const int64_t n = 300;
    const int dim = 2, m = 10, p = m + 1;
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> raw((size_t)n * dim), locs((size_t)n * dim);
    for (auto &v : raw) v = U(rng);
    std::vector<int> ord((size_t)n);
    EXPECT_ST(gpv_order_maxmin_exact(raw.data(), n, dim, ord.data()), GPV_OK);
    for (int64_t k = 0; k < n; ++k)
        for (int t = 0; t < dim; ++t) locs[k + t * n] = raw[(size_t)(ord[(size_t)k] - 1) + (size_t)t * n];
    // nearest previous neighbours by brute force: self first, ascending distance, 1-based, 0 = none
    std::vector<int> NN((size_t)n * p, 0), Cond((size_t)n * p, 0), revNN((size_t)n * p), revCond((size_t)n * p);
    std::vector<std::pair<double, int>> d;
    for (int64_t k = 0; k < n; ++k) {
        d.clear();
        for (int64_t j = 0; j <= k; ++j) {
            double s = 0;
            for (int t = 0; t < dim; ++t) { const double df = locs[k + t * n] - locs[j + t * n]; s += df * df; }
            d.emplace_back(std::sqrt(s), (int)j);
        }
        std::stable_sort(d.begin(), d.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        const int cnt = (int)std::min<size_t>(d.size(), (size_t)p);
        for (int q = 0; q < cnt; ++q) NN[k + (int64_t)q * n] = d[(size_t)q].second + 1;
    }
    EXPECT_ST(gpv_whichCondOnLatent(NN.data(), n, p, n + 1, Cond.data()), GPV_OK);
    for (int64_t k = 0; k < n; ++k)
        for (int j = 0; j < p; ++j) {
            const int v = NN[k + (int64_t)(p - 1 - j) * n];
            revNN[k + (int64_t)j * n] = v;
            revCond[k + (int64_t)j * n] = v ? Cond[k + (int64_t)(p - 1 - j) * n] : INT_MIN;
        }
    std::vector<double> z((size_t)n), tau((size_t)n);
    for (auto &v : z) v = U(rng) - 0.5;
    for (auto &v : tau) v = 0.05 + 0.2 * U(rng);

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    const int NB = gpv_lincomb_batch();
    const int64_t ncols = 2 * NB + 5, ld = n + 3;                          // two full batches and a short one; guard columns
    std::vector<double> E((size_t)ncols * ld, 0.25), X((size_t)ncols * ld, -7.0);
    EXPECT_ST(gpv_plan_solve_t(nullptr, 1, E.data(), ld, X.data(), ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_solve_t(pl, 1, E.data(), ld, X.data(), ld), GPV_ERR_STATE);           // no posterior structure
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(gpv_plan_solve_t(pl, 1, E.data(), ld, X.data(), ld), GPV_ERR_STATE);           // no factor yet
    const double cp[3] = {1.0, 0.1, 1.5};
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_DENOM | GPV_WANT_MEAN, nullptr, nullptr), GPV_OK);
    int64_t stamp0 = 0, stamp1 = 0;
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    EXPECT_ST(gpv_plan_solve_t(pl, -1, E.data(), ld, X.data(), ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_solve_t(pl, 1, nullptr, ld, X.data(), ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_solve_t(pl, 1, E.data(), ld, nullptr, ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_solve_t(pl, 1, E.data(), n - 1, X.data(), ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_solve_t(pl, 1, E.data(), ld, X.data(), n - 1), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_solve_t(pl, 0, E.data(), ld, X.data(), ld), GPV_OK);
    // the timed repetitions: arguments, then the state (a factor, but no batch left by a call yet)
    double ms[3] = {-7.0, -7.0, -7.0};
    EXPECT_ST(gpv_plan_debug_solve_t_ms(nullptr, 2, ms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_solve_t_ms(pl, 0, ms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_solve_t_ms(pl, 2, nullptr), GPV_ERR_BAD_ARG);
    long l1 = mockhip_launches(), g1 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_debug_solve_t_ms(pl, 2, ms), GPV_ERR_STATE);
    EXPECT(mockhip_launches() == l1 && mockhip_graph_launches() == g1 && ms[0] == -7.0);
    const long g0 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_solve_t(pl, ncols, E.data(), ld, X.data(), ld), GPV_OK);
    EXPECT(mockhip_graph_launches() - g0 == 3);                            // one replay per batch
    for (int64_t j = 0; j < ncols; ++j)
        for (int64_t k = n; k < ld; ++k) EXPECT(X[(size_t)(j * ld + k)] == -7.0);            // the guard columns are not written
    EXPECT_ST(gpv_plan_solve_t(pl, ncols, E.data(), ld, E.data(), ld), GPV_OK);              // in place
    l1 = mockhip_launches(), g1 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_solve_t(pl, 1, E.data(), n, X.data(), n), GPV_OK);                    // tight strides, one column
    // ... on what that call left: the untimed pack and the sweep (as the call replays or enqueues it), no unpacking, no copies
    const long rep_l = mockhip_launches() - l1 - 1, rep_g = mockhip_graph_launches() - g1;
    EXPECT(rep_l >= 1 && rep_l - 1 + rep_g >= 1);
    l1 = mockhip_launches(), g1 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_debug_solve_t_ms(pl, 2, ms), GPV_OK);
    EXPECT(mockhip_launches() - l1 == 2 * rep_l && mockhip_graph_launches() - g1 == 2 * rep_g);
    EXPECT(ms[0] == 0.125 && ms[1] == 0.125 && ms[2] == -7.0);             // the mock's elapsed time, reps values
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    EXPECT(stamp0 != 0 && stamp1 == stamp0);                               // the factor is only read
    // a rebuild destroys the captured sweep with the structure it names; the next solve needs a new evaluation first
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(gpv_plan_solve_t(pl, 1, E.data(), ld, X.data(), ld), GPV_ERR_STATE);
    l1 = mockhip_launches(), g1 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_debug_solve_t_ms(pl, 2, ms), GPV_ERR_STATE);                          // ... and so do the timed repetitions
    EXPECT(mockhip_launches() == l1 && mockhip_graph_launches() == g1);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_DENOM, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_solve_t(pl, NB + 1, E.data(), ld, X.data(), ld), GPV_OK);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("solve_t_driver: %d failed expectation(s); %ld kernel launches and %ld graph replays swallowed by the mock runtime\n",
                g_fail, mockhip_launches(), mockhip_graph_launches());
    return g_fail ? 1 : 0;
}
