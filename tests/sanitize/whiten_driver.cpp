// tests/sanitize/whiten_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_whiten (include/gpvecchia.h) under
// AddressSanitizer + UBSan, linked like tests/sanitize/host_driver.cpp against tests/sanitize/mock_hip_runtime.cpp instead of the
// HIP runtime.  Kernels do not run, so this checks the argument checks, the state errors (which evaluation the resident factor
// belongs to, through every route that rewrites it), the shape of what is written (guard entries behind gram and E stay
// untouched, leading dimensions are honoured), that the plan's last evaluation is left alone and that nothing is left
// allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_whiten_driver.py and tools/sanitize_host.sh.
#include "../../include/gpvecchia.h"

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

extern "C" long mockhip_launches(void);
extern "C" long mockhip_live_allocations(void);
extern "C" int gpv_plan_debug_whiten_ms(gpv_plan *pl, int reps, double *ms);       // developer aid, not in the public header

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

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);      // developer build: wait for the (mock) stream, not for a number no kernel will write
    const int64_t n = 200, ldb = n + 3, lde = n + 5;
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
    std::vector<double> B((size_t)ldb * nc, 0.5), E((size_t)lde * nc + 4, guard), G((size_t)nc * nc + 4, guard);
    double ld = guard;
    int64_t nf = -1;

    EXPECT(gpv_whiten_max_cols() == 16);
    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    // ---- arguments, before the state is looked at
    EXPECT_ST(gpv_plan_whiten(nullptr, B.data(), ldb, 3, E.data(), lde, G.data(), &ld, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten(pl, nullptr, ldb, 3, E.data(), lde, G.data(), &ld, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 3, E.data(), lde, nullptr, &ld, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 3, E.data(), lde, G.data(), nullptr, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 3, E.data(), lde, G.data(), &ld, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 0, E.data(), lde, G.data(), &ld, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, -2, E.data(), lde, G.data(), &ld, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 17, E.data(), lde, G.data(), &ld, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), n - 1, 3, E.data(), lde, G.data(), &ld, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 3, E.data(), n - 1, G.data(), &ld, &nf), GPV_ERR_BAD_ARG);
    double ms[3] = {guard, guard, guard};
    EXPECT_ST(gpv_plan_debug_whiten_ms(nullptr, 2, ms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_whiten_ms(pl, 0, ms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_whiten_ms(pl, 2, nullptr), GPV_ERR_BAD_ARG);
    // ---- state: which evaluation the resident factor belongs to
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 3, E.data(), lde, G.data(), &ld, &nf), GPV_ERR_STATE);          // no evaluation
    EXPECT_ST(gpv_plan_debug_whiten_ms(pl, 2, ms), GPV_ERR_STATE);
    EXPECT(ld == guard && nf == -1 && G[0] == guard && E[0] == guard);                         // a refused call writes nothing
    EXPECT(mockhip_launches() == 0);                                                           // ... and launches nothing
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 3, E.data(), lde, G.data(), &ld, &nf), GPV_ERR_STATE);          // no GPV_WANT_U
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
    int64_t stamp0 = -1, stamp1 = -1;
    EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    long l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_debug_whiten_ms(pl, 2, ms), GPV_ERR_STATE);                             // a factor, but no columns left by a call yet
    EXPECT(mockhip_launches() == l0 && ms[0] == guard);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 3, nullptr, 0, G.data(), &ld, &nf), GPV_OK);                    // no E: lde unused
    EXPECT(mockhip_launches() - l0 == 4);                          // packing, the whitening pass, the Gram pass and its sum
    EXPECT(nf == 0 && G[8] == 0.0 && G[9] == guard && E[0] == guard);                          // 3 x 3 and no more
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, nc, E.data(), lde, G.data(), &ld, &nf), GPV_OK);                // a wider call: buffers grow
    EXPECT(mockhip_launches() - l0 == 5);                          // ... and the unpacking of E
    for (int j = 0; j < nc; ++j) {
        EXPECT(E[(size_t)j * lde] != guard && E[(size_t)j * lde + n - 1] != guard);            // Nlocs rows per column
        for (int64_t k = n; k < lde; ++k) EXPECT(E[(size_t)j * lde + k] == guard);             // the padding of lde stays
    }
    for (size_t t = (size_t)lde * nc; t < E.size(); ++t) EXPECT(E[t] == guard);
    for (size_t t = (size_t)nc * nc; t < G.size(); ++t) EXPECT(G[t] == guard);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 5, E.data(), lde, G.data(), &ld, &nf), GPV_OK);                 // narrower again
    // the timed repetitions on what that call left: the two passes and the sum per repetition, no packing, no copies
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_debug_whiten_ms(pl, 2, ms), GPV_OK);
    EXPECT(mockhip_launches() - l0 == 2 * 3);
    EXPECT(ms[0] == 0.125 && ms[1] == 0.125 && ms[2] == guard);                                // the mock's elapsed time, reps values
    EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
    EXPECT(stamp0 == stamp1);
    // a vector of nuggets
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, nugv.data(), n, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_OK);
    // the next evaluation leaves U alone: the resident one is stale
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_ERR_STATE);
    l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_debug_whiten_ms(pl, 2, ms), GPV_ERR_STATE);                             // ... for the timed repetitions too
    EXPECT(mockhip_launches() == l0);
    // an evaluation that is refused (bad nugget count) after one with U: nothing is trusted
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, nugv.data(), n - 1, GPV_WANT_U, nullptr, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    // unobserved locations
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_OK);
    // the posterior routes: a rebuilt structure, the pass (fused: U is not materialised), a Vecchia-Laplace step
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_OK);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_DENOM, nullptr, nullptr), GPV_OK);
    {
        double *dL = nullptr;
        int64_t ldL = 0;
        const bool haveU = gpv_plan_Lentries_device(pl, &dL, &ldL) == GPV_OK;                   // (an unfused pass materialises U)
        EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), haveU ? GPV_OK : GPV_ERR_STATE);
    }
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_vl_begin(pl, 2, nullptr, z.data(), nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_OK);                    // nothing rewritten yet
    {
        double dmax = 0.0;
        int fl = 0;
        EXPECT_ST(gpv_plan_vl_step(pl, "matern", cp, 3, &dmax, &fl), GPV_OK);
        double *dL = nullptr;
        int64_t ldL = 0;
        const bool haveU = gpv_plan_Lentries_device(pl, &dL, &ldL) == GPV_OK;
        EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), haveU ? GPV_OK : GPV_ERR_STATE);
    }
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    // a row shard
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // neighbours conditioned on as latent y
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // a long row (m + 1 = 100, the generic set kernel): one loop takes any row length
    std::vector<int> nnW, cdW;
    make_rows(n, 100, false, nnW, cdW);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, 100, locs.data(), nnW.data(), cdW.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_whiten(pl, B.data(), ldb, 2, nullptr, 0, G.data(), &ld, &nf), GPV_OK);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("whiten_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail,
                mockhip_launches());
    return g_fail ? 1 : 0;
}
