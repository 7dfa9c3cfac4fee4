// tests/sanitize/selinv_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_selinv (include/gpvecchia.h) under
// AddressSanitizer + UBSan, linked like tests/sanitize/unwhiten_driver.cpp against tests/sanitize/mock_hip_runtime.cpp instead of
// the HIP runtime.  Kernels do not run, so this checks the argument checks, the state errors with a plan in hand, the records
// built at first use from the structure the plan keeps on the "device" (their bounds under ASan, the dropped count against a
// loop over the pattern here), the shape of what is written (guard entries stay), the rebuild after a new structure, one graph
// replay per call, and that nothing is left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_selinv_driver.py and tools/sanitize_host.sh.
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
extern "C" int gpv_plan_debug_selinv_ms(gpv_plan *pl, int reps, double *ms);       // developer aid, not in the public header

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

// every row conditions on the points k - off[t] as latent y and on itself (row length p = off.size() + 1, offsets descending)
static void make_rows(int64_t n, const std::vector<int> &off, std::vector<int> &revNN, std::vector<int> &revCond)
{
    const int p = (int)off.size() + 1;
    revNN.assign((size_t)n * p, 0);
    revCond.assign((size_t)n * p, INT_MIN);
    for (int64_t k = 0; k < n; ++k)
        for (int j = 0; j < p; ++j) {
            const int64_t v = j == p - 1 ? k : k - off[(size_t)j];
            if (v < 0) continue;
            revNN[(size_t)(k + (int64_t)j * n)] = (int)v + 1;
            revCond[(size_t)(k + (int64_t)j * n)] = 1;
        }
}

// pairs i < k of a column's rows with i no row of column k, over all columns
static int64_t count_dropped(int64_t n, const std::vector<int> &off)
{
    int64_t d = 0;
    for (int64_t c = 0; c < n; ++c)
        for (size_t a = 0; a < off.size(); ++a)
            for (size_t b = a + 1; b < off.size(); ++b) {
                const int64_t i = c - off[a], k = c - off[b];                // i < k (offsets descend)
                if (i < 0) continue;
                d += std::find(off.begin(), off.end(), (int)(k - i)) == off.end();
            }
    return d;
}

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);      // developer build: wait for the (mock) stream, not for a number no kernel will write
    const int64_t n = 400;
    const int dim = 2;
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> locs((size_t)n * dim), z((size_t)n), tau((size_t)n);
    for (auto &v : locs) v = U(rng);
    for (auto &v : z) v = U(rng) - 0.5;
    for (auto &v : tau) v = 0.05 + 0.2 * U(rng);
    const double cp[3] = {1.0, 0.1, 1.5}, guard = -7.0;
    std::vector<double> vars((size_t)n + 4, guard);
    int64_t nd = -1, stamp0 = 0, stamp1 = 0;

    // ---- a band of the 10 previous points: every two rows of a column are neighbours, nothing is dropped
    std::vector<int> band;
    for (int t = 10; t >= 1; --t) band.push_back(t);
    std::vector<int> revNN, revCond;
    make_rows(n, band, revNN, revCond);
    EXPECT(count_dropped(n, band) == 0);
    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, (int)band.size() + 1, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    // arguments, before the state is looked at
    EXPECT_ST(gpv_plan_selinv(nullptr, 0, vars.data(), &nd), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_selinv(pl, 0, nullptr, &nd), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_selinv(pl, -1, vars.data(), &nd), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_selinv(pl, n, vars.data(), &nd), GPV_ERR_BAD_ARG);
    double ms[3] = {guard, guard, guard};
    EXPECT_ST(gpv_plan_debug_selinv_ms(nullptr, 2, ms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_selinv_ms(pl, 0, ms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_selinv_ms(pl, 2, nullptr), GPV_ERR_BAD_ARG);
    // state
    EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_ERR_STATE);                      // no posterior structure
    EXPECT_ST(gpv_plan_debug_selinv_ms(pl, 2, ms), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_ERR_STATE);                      // no factor yet
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_ERR_STATE);                      // an evaluation without a posterior pass
    EXPECT(nd == -1 && vars[0] == guard);                                                    // a refused call writes nothing
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_DENOM | GPV_WANT_MEAN, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    // the first call builds the records and allocates; the next ones do not
    const long l0 = mockhip_launches(), g0 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_debug_selinv_ms(pl, 2, ms), GPV_ERR_STATE);                           // a factor, but no records built by a call yet
    EXPECT(mockhip_launches() == l0 && mockhip_graph_launches() == g0 && ms[0] == guard);
    EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_OK);
    EXPECT(nd == 0);
    EXPECT(vars[0] != guard && vars[(size_t)n - 1] != guard);
    for (size_t t = (size_t)n; t < vars.size(); ++t) EXPECT(vars[t] == guard);               // Nlocs values and no more
    EXPECT(mockhip_launches() > l0 && mockhip_graph_launches() - g0 == 1);                   // one replay per call
    const long a1 = mockhip_live_allocations();
    EXPECT_ST(gpv_plan_selinv(pl, n - 1, vars.data(), &nd), GPV_OK);
    EXPECT_ST(gpv_plan_selinv(pl, 7, vars.data(), &nd), GPV_OK);
    EXPECT(mockhip_live_allocations() == a1 && mockhip_graph_launches() - g0 == 3);
    // the timed repetitions: the pass alone (as the call replays or enqueues it), without the launch that writes the call's output
    long l1 = mockhip_launches(), g1 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_selinv(pl, 7, vars.data(), &nd), GPV_OK);
    const long rep_l = mockhip_launches() - l1 - 1, rep_g = mockhip_graph_launches() - g1;
    EXPECT(rep_l >= 0 && rep_l + rep_g >= 1);
    l1 = mockhip_launches(), g1 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_debug_selinv_ms(pl, 2, ms), GPV_OK);
    EXPECT(mockhip_launches() - l1 == 2 * rep_l && mockhip_graph_launches() - g1 == 2 * rep_g);
    EXPECT(ms[0] == 0.125 && ms[1] == 0.125 && ms[2] == guard);                              // the mock's elapsed time, reps values
    EXPECT(mockhip_live_allocations() == a1);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    EXPECT(stamp0 != 0 && stamp1 == stamp0);                                                 // the factor is only read
    // the other sweeps of the plan beside it: buffers and graphs of their own
    {
        const int64_t hptr[2] = {0, 1};
        const int32_t hidx[1] = {5};
        const double hval[1] = {1.0};
        double v1 = 0.0;
        std::vector<double> E((size_t)n, 0.25);
        EXPECT_ST(gpv_plan_lincomb(pl, 1, hptr, hidx, hval, &v1, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_solve_t(pl, 1, E.data(), n, E.data(), n), GPV_OK);
        EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_OK);
    }
    // another evaluation: the same records, the new factor
    const long a2 = mockhip_live_allocations();
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_DENOM, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_OK);
    EXPECT(mockhip_live_allocations() == a2);
    // a rebuilt structure: refused until it holds a factor, then the records are built again
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_ERR_STATE);
    l1 = mockhip_launches(), g1 = mockhip_graph_launches();
    EXPECT_ST(gpv_plan_debug_selinv_ms(pl, 2, ms), GPV_ERR_STATE);                           // ... and so are the timed repetitions
    EXPECT(mockhip_launches() == l1 && mockhip_graph_launches() == g1);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_MEAN, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_OK);
    EXPECT(nd == 0);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    EXPECT(mockhip_live_allocations() == 0);

    // ---- rows that condition on k - 7, k - 3 and k - 1: the pairs of a column are no neighbours of each other
    {
        const std::vector<int> off = {7, 3, 1};
        const int64_t want = count_dropped(n, off);
        EXPECT(want > 0);
        std::vector<int> nn2, cd2;
        make_rows(n, off, nn2, cd2);
        pl = nullptr;
        EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, (int)off.size() + 1, locs.data(), nn2.data(), cd2.data(), 0, n), GPV_OK);
        if (pl) {
            EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
            EXPECT_ST(gpv_plan_build_posterior(pl, nn2.data(), cd2.data()), GPV_OK);
            EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_MEAN, nullptr, nullptr), GPV_OK);
            EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_OK);
            EXPECT(nd == want);
            // the same rows on the filled pattern: closed, nothing is dropped
            double ratio = 0.0;
            EXPECT_ST(gpv_plan_build_posterior_fill(pl, nn2.data(), cd2.data(), 8.0, &ratio), GPV_OK);
            EXPECT(ratio > 1.0);
            EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_MEAN, nullptr, nullptr), GPV_OK);
            EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_OK);
            EXPECT(nd == 0);
            EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
        }
    }
    // ---- no neighbours at all (m = 0): a diagonal factor, one level
    {
        std::vector<int> nn3, cd3;
        make_rows(n, {}, nn3, cd3);
        pl = nullptr;
        EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, 1, locs.data(), nn3.data(), cd3.data(), 0, n), GPV_OK);
        if (pl) {
            EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
            EXPECT_ST(gpv_plan_build_posterior(pl, nn3.data(), cd3.data()), GPV_OK);
            EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, tau.data(), n, GPV_WANT_MEAN, nullptr, nullptr), GPV_OK);
            EXPECT_ST(gpv_plan_selinv(pl, 0, vars.data(), &nd), GPV_OK);
            EXPECT(nd == 0);
            EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
        }
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("selinv_driver: %d failed expectation(s); %ld kernel launches and %ld graph replays swallowed by the mock runtime\n",
                g_fail, mockhip_launches(), mockhip_graph_launches());
    return g_fail ? 1 : 0;
}
