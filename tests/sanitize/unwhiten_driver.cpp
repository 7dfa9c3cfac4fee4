// tests/sanitize/unwhiten_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_unwhiten_levels / gpv_plan_unwhiten /
// gpv_plan_simulate (include/gpvecchia.h) under AddressSanitizer + UBSan, linked like tests/sanitize/whiten_driver.cpp against
// tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  Kernels do not run, so this checks the argument checks, the
// state errors with a plan in hand, the level schedule (built on the host from the index arrays the plan keeps on the "device":
// n_levels and n_launches against a loop over the rows here), the shape of what is written (guard entries and the padding of
// the leading dimensions stay untouched), buffer growth across column counts, and that nothing is left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_unwhiten_driver.py and tools/sanitize_host.sh.
#include "../../include/gpvecchia.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

extern "C" long mockhip_launches(void);
extern "C" long mockhip_graph_launches(void);
extern "C" long mockhip_live_allocations(void);
extern "C" int gpv_plan_debug_unwhiten_ms(gpv_plan *pl, int reps, double *ms);     // developer aid, not in the public header

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

// rows of the m previous points; latent: the neighbours are conditioned on as latent y, else as observations (cond.yz = 'z')
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

// one neighbour per row (p = 2): a chain over the first 40 rows, then blocks of 300 rows that hang on the block before them
static void make_blocks(int64_t n, std::vector<int> &revNN, std::vector<int> &revCond)
{
    revNN.assign((size_t)n * 2, 0);
    revCond.assign((size_t)n * 2, INT_MIN);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t v = k == 0 ? -1 : (k < 40 ? k - 1 : (k - 300 >= 40 ? k - 300 : 39));
        if (v >= 0) { revNN[(size_t)k] = (int)v + 1; revCond[(size_t)k] = 0; }
        revNN[(size_t)(k + n)] = (int)k + 1;
        revCond[(size_t)(k + n)] = 1;
    }
}

// the schedule's two counts by the definition: level(k) = 0 without neighbours, else 1 + max level(j); a launch per wide level
// and per maximal run of consecutive narrow ones
static void count_levels(int64_t n, int p, const std::vector<int> &revNN, int narrow, int64_t &n_levels, int64_t &n_launches)
{
    std::vector<int> lev((size_t)n, 0);
    int top = 0;
    for (int64_t k = 0; k < n; ++k) {
        int lv = 0;
        for (int j = 0; j < p - 1; ++j) {
            const int v = revNN[(size_t)(k + (int64_t)j * n)];
            if (v >= 1) lv = std::max(lv, lev[(size_t)v - 1] + 1);
        }
        lev[(size_t)k] = lv;
        top = std::max(top, lv);
    }
    std::vector<int64_t> width((size_t)top + 1, 0);
    for (int64_t k = 0; k < n; ++k) width[(size_t)lev[(size_t)k]]++;
    n_levels = top + 1;
    n_launches = 0;
    bool in_run = false;
    for (int64_t w : width) {
        if (w <= narrow) { if (!in_run) ++n_launches; in_run = true; }
        else { ++n_launches; in_run = false; }
    }
}

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);      // developer build: wait for the (mock) stream, not for a number no kernel will write
    const int64_t n = 200, lde = n + 3, ldb = n + 5;
    const int dim = 2, p = 11, nc = 16;
    std::mt19937_64 rng(9);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> locs((size_t)n * dim), z((size_t)n), nugv((size_t)n, 0.2);
    for (auto &v : locs) v = U(rng);
    for (auto &v : z) v = U(rng) - 0.5;
    std::vector<int> revNN, revCond;
    make_rows(n, p, false, revNN, revCond);
    const double cp[3] = {1.0, 0.1, 1.5};
    const double tau = 0.1, guard = -7.0;
    std::vector<double> E((size_t)lde * nc, 0.5), B((size_t)ldb * nc + 4, guard), Z((size_t)ldb * 40 + 4, guard);
    int64_t nf = -1, nl = -1, nk = -1;
    const int narrow = gpv_unwhiten_narrow();
    EXPECT(narrow >= 1 && narrow <= 1024);

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    // ---- arguments, before the state is looked at
    EXPECT_ST(gpv_plan_unwhiten(nullptr, E.data(), lde, 3, B.data(), ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten(pl, nullptr, lde, 3, B.data(), ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 3, nullptr, ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 3, B.data(), ldb, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 0, B.data(), ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, -2, B.data(), ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 17, B.data(), ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), n - 1, 3, B.data(), ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 3, B.data(), n - 1, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_simulate(nullptr, 1, 0, 3, Z.data(), ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_simulate(pl, 1, 0, 3, nullptr, ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_simulate(pl, 1, 0, 3, Z.data(), ldb, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_simulate(pl, 1, -1, 3, Z.data(), ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_simulate(pl, 1, 0, 0, Z.data(), ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_simulate(pl, 1, INT64_MAX - 1, 3, Z.data(), ldb, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_simulate(pl, 1, 0, 3, Z.data(), n - 1, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten_levels(nullptr, &nl, &nk), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten_levels(pl, nullptr, &nk), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_unwhiten_levels(pl, &nl, nullptr), GPV_ERR_BAD_ARG);
    double ms[3] = {guard, guard, guard};
    EXPECT_ST(gpv_plan_debug_unwhiten_ms(nullptr, 2, ms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_unwhiten_ms(pl, 0, ms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_unwhiten_ms(pl, 2, nullptr), GPV_ERR_BAD_ARG);
    // ---- state: which evaluation the resident factor belongs to
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 3, B.data(), ldb, &nf), GPV_ERR_STATE);                       // no evaluation
    EXPECT_ST(gpv_plan_simulate(pl, 1, 0, 3, Z.data(), ldb, &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_debug_unwhiten_ms(pl, 2, ms), GPV_ERR_STATE);
    EXPECT(nf == -1 && B[0] == guard && Z[0] == guard);                                        // a refused call writes nothing
    EXPECT(mockhip_launches() == 0);                                                           // ... and launches nothing
    // the schedule needs no evaluation: a chain, one row per level, all narrow: one launch
    int64_t want_l = 0, want_k = 0;
    count_levels(n, p, revNN, narrow, want_l, want_k);
    EXPECT_ST(gpv_plan_unwhiten_levels(pl, &nl, &nk), GPV_OK);
    EXPECT(nl == want_l && nk == want_k && nl == n && nk == 1);
    EXPECT(mockhip_launches() == 0);
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 3, B.data(), ldb, &nf), GPV_ERR_STATE);                       // no GPV_WANT_U
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
    int64_t stamp0 = -1, stamp1 = -1;
    EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    long l0 = mockhip_launches(), g0 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_debug_unwhiten_ms(pl, 2, ms), GPV_ERR_STATE);                           // a factor, but no columns left by a call yet
    EXPECT(mockhip_launches() == l0 && mockhip_graph_launches() == g0 && ms[0] == guard);
    // ---- buffer growth across column counts, shapes
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 3, B.data(), ldb, &nf), GPV_OK);
    EXPECT(nf == 0 && B[0] != guard && B[(size_t)2 * ldb + n - 1] != guard && B[(size_t)3 * ldb] == guard);      // 3 columns and no more
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, nc, B.data(), ldb, &nf), GPV_OK);                             // a wider call: buffers grow
    for (int j = 0; j < nc; ++j) {
        EXPECT(B[(size_t)j * ldb] != guard && B[(size_t)j * ldb + n - 1] != guard);            // Nlocs rows per column
        for (int64_t k = n; k < ldb; ++k) EXPECT(B[(size_t)j * ldb + k] == guard);             // the padding of ldb stays
    }
    for (size_t t = (size_t)ldb * nc; t < B.size(); ++t) EXPECT(B[t] == guard);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 5, B.data(), ldb, &nf), GPV_OK);                              // narrower again
    // the timed repetitions on what that call left: the sweep alone (as the call replays or enqueues it), no packing, no copies
    l0 = mockhip_launches(), g0 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 5, B.data(), ldb, &nf), GPV_OK);
    const long sweep_l = mockhip_launches() - l0 - 2, sweep_g = mockhip_graph_launches() - g0;      // (less packing and unpacking)
    EXPECT(sweep_l >= 0 && sweep_l + sweep_g >= 1);
    l0 = mockhip_launches(), g0 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_debug_unwhiten_ms(pl, 2, ms), GPV_OK);
    EXPECT(mockhip_launches() - l0 == 2 * sweep_l && mockhip_graph_launches() - g0 == 2 * sweep_g);
    EXPECT(ms[0] == 0.125 && ms[1] == 0.125 && ms[2] == guard);                                // the mock's elapsed time, reps values
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 2, E.data(), lde, &nf), GPV_OK);                              // in place
    EXPECT_ST(gpv_plan_simulate(pl, 5, 13, 22, Z.data(), ldb, &nf), GPV_OK);                                     // draws 13 .. 34: three batches
    for (int j = 0; j < 22; ++j) {
        EXPECT(Z[(size_t)j * ldb] != guard && Z[(size_t)j * ldb + n - 1] != guard);
        for (int64_t k = n; k < ldb; ++k) EXPECT(Z[(size_t)j * ldb + k] == guard);
    }
    EXPECT(Z[(size_t)22 * ldb] == guard);
    EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
    EXPECT(stamp0 == stamp1);
    // whitening beside it: buffers of its own
    {
        std::vector<double> G((size_t)nc * nc);
        double ld = 0.0;
        EXPECT_ST(gpv_plan_whiten(pl, E.data(), lde, 4, nullptr, 0, G.data(), &ld, &nf), GPV_OK);
        EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 4, B.data(), ldb, &nf), GPV_OK);
    }
    // a vector of nuggets: another evaluation, the sweep is captured again
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, nugv.data(), n, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 2, B.data(), ldb, &nf), GPV_OK);
    EXPECT_ST(gpv_plan_simulate(pl, 5, 0, 1, Z.data(), ldb, &nf), GPV_OK);
    // the next evaluation leaves U alone: the resident one is stale
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 2, B.data(), ldb, &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_simulate(pl, 5, 0, 1, Z.data(), ldb, &nf), GPV_ERR_STATE);
    l0 = mockhip_launches(), g0 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_debug_unwhiten_ms(pl, 2, ms), GPV_ERR_STATE);                           // ... for the timed repetitions too
    EXPECT(mockhip_launches() == l0 && mockhip_graph_launches() == g0);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    // unobserved locations
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 2, B.data(), ldb, &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_simulate(pl, 5, 0, 1, Z.data(), ldb, &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 2, B.data(), ldb, &nf), GPV_OK);
    // a rebuilt posterior structure
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 2, B.data(), ldb, &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 2, B.data(), ldb, &nf), GPV_OK);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    // ---- a second schedule: a chain of 40 rows, three blocks of 300 rows, a tail of 60
    {
        const int64_t n2 = 1000;
        std::vector<double> locs2((size_t)n2 * dim);
        for (auto &v : locs2) v = U(rng);
        std::vector<int> nnB, cdB;
        make_blocks(n2, nnB, cdB);
        count_levels(n2, 2, nnB, narrow, want_l, want_k);
        pl = nullptr;
        EXPECT_ST(gpv_plan_create(&pl, 0, n2, dim, 2, locs2.data(), nnB.data(), cdB.data(), 0, n2), GPV_OK);
        if (pl) {
            EXPECT_ST(gpv_plan_unwhiten_levels(pl, &nl, &nk), GPV_OK);
            EXPECT(nl == want_l && nk == want_k && nl == 44);
            if (narrow >= 60 && narrow < 300) EXPECT(nk == 5);             // the chain, three wide levels, the tail
            EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
            std::vector<double> E2((size_t)n2 * 3, 0.25), B2((size_t)n2 * 3 + 2, guard);
            EXPECT_ST(gpv_plan_unwhiten(pl, E2.data(), n2, 3, B2.data(), n2, &nf), GPV_OK);
            EXPECT(B2[(size_t)n2 * 3] == guard && B2[(size_t)n2 * 3 - 1] != guard);
            EXPECT_ST(gpv_plan_unwhiten_levels(pl, &nl, &nk), GPV_OK);     // reported again, not rebuilt
            EXPECT(nl == want_l && nk == want_k);
            EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
        }
    }
    // a row shard
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 2, B.data(), ldb, &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_simulate(pl, 5, 0, 1, Z.data(), ldb, &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_unwhiten_levels(pl, &nl, &nk), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // neighbours conditioned on as latent y
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 2, B.data(), ldb, &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_simulate(pl, 5, 0, 1, Z.data(), ldb, &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_unwhiten_levels(pl, &nl, &nk), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // a long row (m + 1 = 100, the generic set kernel): one loop takes any row length
    std::vector<int> nnW, cdW;
    make_rows(n, 100, false, nnW, cdW);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, 100, locs.data(), nnW.data(), cdW.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_unwhiten(pl, E.data(), lde, 2, B.data(), ldb, &nf), GPV_OK);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("unwhiten_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail,
                mockhip_launches());
    return g_fail ? 1 : 0;
}
