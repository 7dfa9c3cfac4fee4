// tests/sanitize/draws_summary_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_draws_normals_host,
// gpv_plan_draws_normals and gpv_plan_draws_summary (include/gpvecchia.h) under AddressSanitizer + UBSan, linked like
// tests/sanitize/solve_t_driver.cpp against tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  Kernels do not
// run, so this checks the argument validation of the three entries (every GPV_ERR_BAD_ARG / GPV_ERR_STATE case, before and
// after a factor exists), the strided writes of the host generator (guard entries stay untouched), batching, the growth of the
// per-draw buffers, graph lifetime across a rebuild, and that nothing is left allocated — never device numbers.
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
    const uint64_t seed = 0x8000000000000005ull;
    // the host generator: strided columns, guard entries, the same bits whatever the request
    {
        const int64_t nk = 37, lde = nk + 2, nc = 2 * NB + 5;
        std::vector<double> G((size_t)nc * lde, -7.0), one(1, 0.0);
        EXPECT_ST(gpv_draws_normals_host(seed, 0, nk, 0, nc, nullptr, lde), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_draws_normals_host(seed, -1, nk, 0, nc, G.data(), lde), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_draws_normals_host(seed, 0, -1, 0, nc, G.data(), lde), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_draws_normals_host(seed, 0, nk, -1, nc, G.data(), lde), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_draws_normals_host(seed, 0, nk, 0, -1, G.data(), lde), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_draws_normals_host(seed, 0, nk, 0, nc, G.data(), nk - 1), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_draws_normals_host(seed, 0, 0, 0, nc, G.data(), lde), GPV_OK);
        EXPECT_ST(gpv_draws_normals_host(seed, 0, nk, 0, 0, G.data(), lde), GPV_OK);
        EXPECT(G[0] == -7.0);
        EXPECT_ST(gpv_draws_normals_host(seed, 0, nk, 0, nc, G.data(), lde), GPV_OK);
        for (int64_t j = 0; j < nc; ++j) {
            for (int64_t k = 0; k < nk; ++k) EXPECT(std::isfinite(G[(size_t)(j * lde + k)]) && std::fabs(G[(size_t)(j * lde + k)]) < 8.5);
            for (int64_t k = nk; k < lde; ++k) EXPECT(G[(size_t)(j * lde + k)] == -7.0);
        }
        EXPECT_ST(gpv_draws_normals_host(seed, 36, 1, 33, 1, one.data(), 1), GPV_OK);          // odd first draw, one entry
        EXPECT(one[0] == G[(size_t)(33 * lde + 36)]);
        EXPECT_ST(gpv_draws_normals_host(seed, ((int64_t)1 << 32) + 1, 1, ((int64_t)1 << 33) + 1, 1, one.data(), 1), GPV_OK);
        EXPECT(std::isfinite(one[0]));
    }
    const int64_t nd = 2 * NB + 11, ld = n + 3;                                // two full batches and a short, odd one
    std::vector<double> E((size_t)nd * ld, -7.0), mu((size_t)n, 0.5), mean((size_t)n), var((size_t)n), exceed((size_t)8 * n);
    std::vector<double> dmax((size_t)nd + 40), dmean((size_t)nd + 40);
    std::vector<uint8_t> mask((size_t)n, 0), none((size_t)n, 0);
    for (int64_t k = 0; k < n; k += 3) mask[(size_t)k] = 1;
    const double thr[8] = {-1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0};
#define SUMMARY(nd_, skip_, link_, nthr_, thr_, mask_, mean_, var_, ex_, dmax_, dmean_) \
    gpv_plan_draws_summary(pl, nd_, seed, skip_, mu.data(), link_, nthr_, thr_, mask_, mean_, var_, ex_, dmax_, dmean_)
    // no plan, no structure, no factor
    EXPECT_ST(gpv_plan_draws_summary(nullptr, nd, seed, 0, mu.data(), 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr),
              GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_draws_normals(nullptr, seed, 0, 0, 1, E.data(), ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, 0, 0, 1, E.data(), ld), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(SUMMARY(nd, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, 0, 0, 1, E.data(), ld), GPV_ERR_STATE);
    // bad arguments win over the state: they are checked first
    EXPECT_ST(SUMMARY(1, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    const double cp[3] = {1.0, 0.1, 1.5};
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_DENOM | GPV_WANT_MEAN, nullptr, nullptr), GPV_OK);
    int64_t stamp0 = 0, stamp1 = 0;
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    const long live0 = mockhip_live_allocations();
    // every GPV_ERR_BAD_ARG case of the summary
    EXPECT_ST(SUMMARY(1, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(0, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(-4, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, 0, -1, thr, nullptr, mean.data(), var.data(), exceed.data(), nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, 0, 9, thr, nullptr, mean.data(), var.data(), exceed.data(), nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, -1, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, 3, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, -1, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, n, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, 0, 0, nullptr, none.data(), mean.data(), var.data(), nullptr, dmax.data(), dmean.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 1, 0, 0, nullptr, mask.data(), mean.data(), var.data(), nullptr, dmax.data(), dmean.data()), GPV_OK);
    {   // a mask whose only location lies in front of skip_front selects nothing
        std::vector<uint8_t> first((size_t)n, 0);
        first[0] = 1;
        EXPECT_ST(SUMMARY(nd, 1, 0, 0, nullptr, first.data(), mean.data(), var.data(), nullptr, dmax.data(), dmean.data()), GPV_ERR_BAD_ARG);
    }
    EXPECT_ST(SUMMARY(nd, 0, 0, 0, nullptr, nullptr, nullptr, var.data(), nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, 0, 0, nullptr, nullptr, mean.data(), nullptr, nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, 0, 2, nullptr, nullptr, mean.data(), var.data(), exceed.data(), nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, 0, 2, thr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, dmax.data(), nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(SUMMARY(nd, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, dmean.data()), GPV_ERR_BAD_ARG);
    // ... and of the read-back of the device normals
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, 0, 0, 1, nullptr, ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, 0, 0, -1, E.data(), ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, 0, -1, 1, E.data(), ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, 0, 0, 1, E.data(), n - 1), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, -1, 0, 1, E.data(), ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, n, 0, 1, E.data(), ld), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, 0, 0, 0, E.data(), ld), GPV_OK);
    // valid calls: batches, guard columns, buffers that grow with the number of draws
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, 2, 0, nd, E.data(), ld), GPV_OK);
    for (int64_t j = 0; j < nd; ++j)
        for (int64_t k = n; k < ld; ++k) EXPECT(E[(size_t)(j * ld + k)] == -7.0);
    EXPECT_ST(gpv_plan_draws_normals(pl, seed, 0, NB + 3, NB, E.data(), n), GPV_OK);           // across a batch border, tight stride
    const long g0 = mockhip_graph_launches();
    EXPECT_ST(SUMMARY(nd, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_OK);
    EXPECT(mockhip_graph_launches() - g0 == 3);                            // one replay of the captured sweep per batch
    EXPECT_ST(SUMMARY(2, 0, 1, 8, thr, nullptr, mean.data(), var.data(), exceed.data(), dmax.data(), dmean.data()), GPV_OK);
    EXPECT_ST(SUMMARY(nd + 40, 5, 2, 3, thr, mask.data(), mean.data(), var.data(), exceed.data(), dmax.data(), dmean.data()), GPV_OK);
    EXPECT_ST(gpv_plan_draws_summary(pl, nd, seed, 0, nullptr, 0, 1, thr, nullptr, mean.data(), var.data(), exceed.data(), nullptr, nullptr),
              GPV_OK);                                                         // mu NULL: zeros
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    EXPECT(stamp0 != 0 && stamp1 == stamp0);                               // the factor is only read
    EXPECT(mockhip_live_allocations() > live0);                            // the buffers stay with the plan ...
    // the plan's other entries are unaffected, and a rebuild asks for a new evaluation first
    EXPECT_ST(gpv_plan_solve_t(pl, 1, E.data(), ld, E.data(), ld), GPV_OK);
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(SUMMARY(nd, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, nullptr, nullptr), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_DENOM, nullptr, nullptr), GPV_OK);
    EXPECT_ST(SUMMARY(NB + 1, 0, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, dmax.data(), dmean.data()), GPV_OK);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    EXPECT(mockhip_live_allocations() == 0);                               // ... and go with it
    std::printf("draws_summary_driver: %d failed expectation(s); %ld kernel launches and %ld graph replays swallowed by the mock runtime\n",
                g_fail, mockhip_launches(), mockhip_graph_launches());
    return g_fail ? 1 : 0;
}
