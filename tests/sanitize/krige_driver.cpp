// tests/sanitize/krige_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_krige / gpv_find_query_nn
// (include/gpvecchia.h) under AddressSanitizer + UBSan, linked like tests/sanitize/blockcv_driver.cpp against
// tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  Kernels do not run, so this checks the argument checks and
// the refusals before the device is touched (nothing written, nothing launched), the state errors with a plan in hand, the
// chunk arithmetic by the launches it makes (nq = 0, 1, chunk, chunk + 1), the shape of what is written (guard entries and the
// padding of the leading dimension stay untouched), the search index built on the host from the plan's resident coordinates
// (grid and brute route, an eligibility mask, non-finite coordinates), that the plan's evaluation stays what it was, and
// that nothing is left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_krige_driver.py and tools/sanitize_host.sh.
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
    const int64_t n = 3000, nq = 130, ldm = nq + 3;     // n: above the grid threshold of the search
    const int dim = 2, p = 11, m = 10, nc = 16;
    std::mt19937_64 rng(9);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> locs((size_t)n * dim), z((size_t)n), nugv((size_t)n, 0.2), Z((size_t)(n + 2) * nc, 0.5), ql((size_t)nq * dim);
    for (auto &v : locs) v = U(rng);
    for (auto &v : z) v = U(rng) - 0.5;
    for (auto &v : ql) v = 1.4 * U(rng) - 0.2;          // some outside the box
    std::vector<int> revNN, revCond;
    make_rows(n, p, false, revNN, revCond);
    const double cp[3] = {1.0, 0.1, 1.5}, cpg[3] = {1.0, 0.1, 0.8}, cpe[4] = {1.0, 0.1, 0.5, 0.2}, cps[4] = {1.0, 0.1, 0.3, 2.5};
    const double tau = 0.1, guard = -7.0, sc2[2] = {0.1, 0.3};
    std::vector<double> M((size_t)ldm * nc + 4, guard), V((size_t)nq + 2, guard);
    std::vector<int> NNq((size_t)nq * m);
    for (int64_t i = 0; i < nq; ++i)
        for (int s = 0; s < m; ++s) NNq[(size_t)(i + (int64_t)s * nq)] = (s < 8) ? (int)((i * 7 + s) % n) + 1 : 0;
    std::vector<unsigned char> el((size_t)n, 1);
    for (int64_t i = 0; i < n; i += 3) el[(size_t)i] = 0;
    int64_t nf = -1;
    EXPECT(gpv_krige_max_cols() == 16);

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
#define KRIGE(plan, cov, par, npar, nug, nnug, Zp, ldz, ncols, q, nq_, m_, nn, scale, elig, chunk, mean, ldm_, var) \
    gpv_plan_krige(plan, cov, par, npar, nug, nnug, Zp, ldz, ncols, q, nq_, m_, nn, scale, elig, chunk, mean, ldm_, var, &nf)
    // ---- arguments, before the state is looked at and before the device is touched
    const long l0 = mockhip_launches();
    EXPECT_ST(KRIGE(nullptr, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(KRIGE(pl, nullptr, cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(KRIGE(pl, "matern", nullptr, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, nullptr, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, nullptr, nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, nullptr, ldm, V.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_krige(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data(), nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 2, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);      // n_nuggets
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 0, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);      // ncols
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 17, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, nullptr, n, 2, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);       // the plan's data: one column
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n - 1, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);  // ldz
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), nq - 1, V.data()), GPV_ERR_BAD_ARG);   // ldm
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), -1, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, 0, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);      // m
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, -1, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);     // chunk
    EXPECT_ST(KRIGE(pl, "matern", cp, 4, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);      // ncovparms
    EXPECT_ST(KRIGE(pl, "matern_scaledim", cps, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(KRIGE(pl, "gauss", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_COVTYPE);
    {
        const double neg = -0.1, inf = INFINITY, cpn[3] = {1.0, 0.1, 61.0}, scbad[2] = {0.1, 0.0};
        EXPECT_ST(KRIGE(pl, "matern", cp, 3, &neg, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
        EXPECT_ST(KRIGE(pl, "matern", cp, 3, &inf, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
        EXPECT_ST(KRIGE(pl, "matern", cpn, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, scbad, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_BAD_ARG);
        std::vector<int> bad(NNq);
        bad[5] = (int)n + 1;
        EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, bad.data(), nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_INDEX);
        bad[5] = -1;
        EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, bad.data(), nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_INDEX);
    }
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, 64, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_UNSUPPORTED_M);
    // the plan's data, and none set
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, nullptr, 0, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_STATE);
    EXPECT(nf == -1 && M[0] == guard && V[0] == guard && mockhip_launches() == l0);             // a refused call writes and launches nothing
    // ---- chunk arithmetic: a search and a pass per chunk, no evaluation needed
    const int64_t chunk = 64;
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), 0, m, nullptr, nullptr, nullptr, chunk, M.data(), ldm, V.data()), GPV_OK);
    EXPECT(nf == 0 && M[0] == guard && V[0] == guard && mockhip_launches() == l0);              // nq = 0: nothing to do
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, nullptr, 0, 1, nullptr, 0, m, nullptr, nullptr, nullptr, chunk, nullptr, 0, nullptr), GPV_OK);
    struct { int64_t nq; long launches; } cases[] = {{1, 2}, {chunk, 2}, {chunk + 1, 4}, {nq, 6}};
    for (auto &c : cases) {
        std::fill(M.begin(), M.end(), guard);
        std::fill(V.begin(), V.end(), guard);
        const long b = mockhip_launches();
        EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, nullptr, 0, 1, ql.data(), c.nq, m, nullptr, nullptr, nullptr, chunk, M.data(), ldm, V.data()), GPV_OK);
        EXPECT(mockhip_launches() - b == c.launches && nf == 0);
        EXPECT(M[0] != guard && M[(size_t)c.nq - 1] != guard && M[(size_t)c.nq] == guard);
        EXPECT(V[0] != guard && V[(size_t)c.nq - 1] != guard && V[(size_t)c.nq] == guard);
    }
    // ---- columns: ldz and ldm wider than the data, every column written and nothing else; one more launch (the pack)
    std::fill(M.begin(), M.end(), guard);
    {
        const long b = mockhip_launches();
        EXPECT_ST(KRIGE(pl, "matern", cp, 3, nugv.data(), n, Z.data(), n + 2, nc, ql.data(), nq, m, nullptr, nullptr, el.data(), 0, M.data(), ldm, V.data()), GPV_OK);
        EXPECT(mockhip_launches() - b == 3);
    }
    for (int j = 0; j < nc; ++j) {
        EXPECT(M[(size_t)j * ldm] != guard && M[(size_t)j * ldm + nq - 1] != guard);
        for (int64_t k = nq; k < ldm; ++k) EXPECT(M[(size_t)j * ldm + k] == guard);             // the padding of the leading dimension stays
    }
    for (size_t t = (size_t)ldm * nc; t < M.size(); ++t) EXPECT(M[t] == guard);
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 5, ql.data(), nq, m, NNq.data(), nullptr, nullptr, 50, M.data(), ldm, V.data()), GPV_OK);   // given neighbours
    // every family; the search on scaled coordinates; the brute-force route; non-finite coordinates of a query
    EXPECT_ST(KRIGE(pl, "matern", cpg, 3, &tau, 1, Z.data(), n, 3, ql.data(), nq, 63, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_OK);
    EXPECT_ST(KRIGE(pl, "esqe", cpe, 4, &tau, 1, Z.data(), n, 3, ql.data(), nq, 15, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_OK);
    EXPECT_ST(KRIGE(pl, "matern_scaledim", cps, 4, &tau, 1, Z.data(), n, 3, ql.data(), nq, 16, nullptr, sc2, el.data(), 33, M.data(), ldm, V.data()), GPV_OK);
    setenv("GPV_NN_BRUTE", "1", 1);
    ql[3] = NAN;
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_OK);
    unsetenv("GPV_NN_BRUTE");
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_OK);
    ql[3] = 0.5;
    // ---- an evaluation stays what it was
    {
        double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
        EXPECT_ST(KRIGE(pl, "matern", cp, 3, nugv.data(), n, Z.data(), n, 2, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_OK);
        EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
        for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
        std::vector<double> Lent((size_t)n * p);
        EXPECT_ST(gpv_plan_get_Lentries(pl, Lent.data()), GPV_OK);                              // U is still that evaluation's
    }
    // unobserved locations
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    nf = -1;
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_STATE);
    EXPECT(nf == -1);
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_OK);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    // a row shard
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // neighbours conditioned on as latent y
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(KRIGE(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, nullptr, nullptr, 0, M.data(), ldm, V.data()), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // ---- the search entry on host arrays: five dimensions (brute force), fewer points than m, refusals
    {
        const int64_t n5 = 40, q5 = 70;
        std::vector<double> x((size_t)n5 * 5), y((size_t)q5 * 5);
        for (auto &v : x) v = U(rng);
        for (auto &v : y) v = U(rng);
        x[3] = NAN;
        std::vector<int> NN((size_t)q5 * 50 + 2, -9);
        EXPECT_ST(gpv_find_query_nn(0, x.data(), n5, 5, nullptr, y.data(), q5, 50, NN.data()), GPV_OK);
        EXPECT(NN[(size_t)q5 * 50 - 1] != -9 && NN[(size_t)q5 * 50] == -9);
        std::vector<int> NN2((size_t)nq * 15 + 1, -9);                                          // the grid route, with a mask
        EXPECT_ST(gpv_find_query_nn(0, locs.data(), n, 2, el.data(), ql.data(), nq, 15, NN2.data()), GPV_OK);
        EXPECT(NN2[(size_t)nq * 15 - 1] != -9 && NN2[(size_t)nq * 15] == -9);
        std::fill(NN.begin(), NN.end(), -9);
        EXPECT_ST(gpv_find_query_nn(0, x.data(), n5, 5, nullptr, y.data(), 0, 50, nullptr), GPV_OK);
        EXPECT_ST(gpv_find_query_nn(0, nullptr, n5, 5, nullptr, y.data(), q5, 50, NN.data()), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_find_query_nn(0, x.data(), n5, 5, nullptr, nullptr, q5, 50, NN.data()), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_find_query_nn(0, x.data(), n5, 5, nullptr, y.data(), q5, 50, nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_find_query_nn(0, x.data(), 0, 5, nullptr, y.data(), q5, 50, NN.data()), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_find_query_nn(0, x.data(), n5, 9, nullptr, y.data(), q5, 50, NN.data()), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_find_query_nn(0, x.data(), n5, 5, nullptr, y.data(), q5, 0, NN.data()), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_find_query_nn(0, x.data(), n5, 5, nullptr, y.data(), q5, gpv_nn_max_m() + 1, NN.data()), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_find_query_nn(0, x.data(), n5, 5, nullptr, y.data(), -1, 50, NN.data()), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_find_query_nn(3, x.data(), n5, 5, nullptr, y.data(), q5, 50, NN.data()), GPV_ERR_NO_DEVICE);
        EXPECT(NN[0] == -9);
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("krige_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail, mockhip_launches());
    return g_fail ? 1 : 0;
}
