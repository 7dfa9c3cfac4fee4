// tests/sanitize/loo_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_whiten_t / gpv_plan_precision / gpv_plan_loo /
// gpv_plan_loo_index / gpv_loo_index_host (include/gpvecchia.h) under AddressSanitizer + UBSan, linked like
// tests/sanitize/unwhiten_driver.cpp against tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  Kernels do not run,
// so this checks the argument checks, the state errors with a plan in hand, the transposed index (built on the host from the
// index arrays the plan keeps on the "device": its counts against a loop over the rows here, a star plan, empty columns, the
// 32-bit guard, buffers of exactly the documented sizes), the shape of what is written (guard entries and the padding of the
// leading dimensions stay untouched), buffer growth across column counts, and that nothing is left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_loo_driver.py and tools/sanitize_host.sh.
#include "../../include/gpvecchia.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

extern "C" long mockhip_launches(void);
extern "C" long mockhip_live_allocations(void);
extern "C" int gpv_plan_debug_loo_ms(gpv_plan *pl, int reps, double *ms);          // developer aid, not in the public header

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

// every row k > 0 conditions on row 0 alone (p = 2)
static void make_star(int64_t n, std::vector<int> &revNN, std::vector<int> &revCond)
{
    revNN.assign((size_t)n * 2, 0);
    revCond.assign((size_t)n * 2, INT_MIN);
    for (int64_t k = 0; k < n; ++k) {
        if (k > 0) { revNN[(size_t)k] = 1; revCond[(size_t)k] = 0; }
        revNN[(size_t)(k + n)] = (int)k + 1;
        revCond[(size_t)(k + n)] = 1;
    }
}

// the index's three counts by the definition: in-degree of every location over the neighbour entries
static void count_index(int64_t n, int p, const std::vector<int> &revNN, int64_t &nnz, int64_t &longest, int64_t &empty)
{
    std::vector<int64_t> deg((size_t)n, 0);
    for (int64_t k = 0; k < n; ++k)
        for (int j = 0; j < p - 1; ++j) {
            const int v = revNN[(size_t)(k + (int64_t)j * n)];
            if (v >= 1) deg[(size_t)v - 1]++;
        }
    nnz = longest = empty = 0;
    for (int64_t d : deg) { nnz += d; longest = std::max(longest, d); empty += d == 0; }
}

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);      // developer build: wait for the (mock) stream, not for a number no kernel will write
    const int64_t n = 200, lda = n + 3, ldo = n + 5;
    const int dim = 2, p = 11, nc = 16, ns = GPV_LOO_NSCORES;
    std::mt19937_64 rng(9);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> locs((size_t)n * dim), z((size_t)n), nugv((size_t)n, 0.2);
    for (auto &v : locs) v = U(rng);
    for (auto &v : z) v = U(rng) - 0.5;
    std::vector<int> revNN, revCond;
    make_rows(n, p, false, revNN, revCond);
    const double cp[3] = {1.0, 0.1, 1.5};
    const double tau = 0.1, guard = -7.0;
    std::vector<double> A((size_t)lda * nc, 0.5), O((size_t)ldo * nc + 4, guard), q((size_t)n + 2, guard), sc((size_t)nc * ns + 2, guard);
    int64_t nf = -1, e0 = -1, e1 = -1, e2 = -1;
    EXPECT(gpv_loo_nscores() == GPV_LOO_NSCORES);

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    // ---- arguments, before the state is looked at
    EXPECT_ST(gpv_plan_whiten_t(nullptr, A.data(), lda, 3, O.data(), ldo, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten_t(pl, nullptr, lda, 3, O.data(), ldo, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 3, nullptr, ldo, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 3, O.data(), ldo, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 0, O.data(), ldo, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 17, O.data(), ldo, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), n - 1, 3, O.data(), ldo, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 3, O.data(), n - 1, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_precision(nullptr, A.data(), lda, 3, O.data(), ldo, q.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_precision(pl, nullptr, lda, 3, O.data(), ldo, q.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, 3, nullptr, ldo, q.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, 3, O.data(), ldo, q.data(), nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, -2, O.data(), ldo, q.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, 17, O.data(), ldo, q.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_precision(pl, A.data(), n - 1, 3, O.data(), ldo, q.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, 3, O.data(), n - 1, q.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo(nullptr, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo(pl, nullptr, lda, 3, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 3, O.data(), ldo, q.data(), nullptr, &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 0, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 17, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), n - 1, 3, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 3, O.data(), n - 1, q.data(), sc.data(), &nf), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo_index(nullptr, &e0, &e1, &e2), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo_index(pl, nullptr, &e1, &e2), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo_index(pl, &e0, nullptr, &e2), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_loo_index(pl, &e0, &e1, nullptr), GPV_ERR_BAD_ARG);
    double ms[3] = {guard, guard, guard};
    EXPECT_ST(gpv_plan_debug_loo_ms(nullptr, 2, ms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_loo_ms(pl, 0, ms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_loo_ms(pl, 2, nullptr), GPV_ERR_BAD_ARG);
    // ---- state: which evaluation the resident factor belongs to
    EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 3, O.data(), ldo, &nf), GPV_ERR_STATE);                       // no evaluation
    EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, 3, O.data(), ldo, q.data(), &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_debug_loo_ms(pl, 2, ms), GPV_ERR_STATE);
    EXPECT(nf == -1 && O[0] == guard && q[0] == guard && sc[0] == guard);                      // a refused call writes nothing
    EXPECT(mockhip_launches() == 0);                                                           // ... and launches nothing
    // the index needs no evaluation: every location k is a neighbour of the rows k + 1 .. k + 10
    int64_t w0 = 0, w1 = 0, w2 = 0;
    count_index(n, p, revNN, w0, w1, w2);
    EXPECT_ST(gpv_plan_loo_index(pl, &e0, &e1, &e2), GPV_OK);
    EXPECT(e0 == w0 && e1 == w1 && e2 == w2 && e1 == p - 1 && e2 == 1);
    EXPECT(mockhip_launches() == 0);
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_STATE);       // no GPV_WANT_U
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
    int64_t stamp0 = -1, stamp1 = -1;
    EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    const long l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_debug_loo_ms(pl, 2, ms), GPV_ERR_STATE);                                // a factor, but no columns left by a call yet
    EXPECT(mockhip_launches() == l0 && ms[0] == guard);
    // ---- buffer growth across column counts, shapes
    EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 3, O.data(), ldo, &nf), GPV_OK);
    EXPECT(nf == 0 && O[0] != guard && O[(size_t)2 * ldo + n - 1] != guard && O[(size_t)3 * ldo] == guard);      // 3 columns and no more
    EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, nc, O.data(), ldo, q.data(), &nf), GPV_OK);                  // a wider call: buffers grow
    for (int j = 0; j < nc; ++j) {
        EXPECT(O[(size_t)j * ldo] != guard && O[(size_t)j * ldo + n - 1] != guard);            // Nlocs rows per column
        for (int64_t k = n; k < ldo; ++k) EXPECT(O[(size_t)j * ldo + k] == guard);             // the padding of the leading dimension stays
    }
    for (size_t t = (size_t)ldo * nc; t < O.size(); ++t) EXPECT(O[t] == guard);
    EXPECT(q[0] != guard && q[(size_t)n - 1] != guard && q[(size_t)n] == guard);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 5, O.data(), ldo, q.data(), sc.data(), &nf), GPV_OK);              // narrower again
    EXPECT(sc[0] != guard && sc[(size_t)5 * ns - 1] != guard && sc[(size_t)5 * ns] == guard && q[(size_t)n] == guard);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, nc, nullptr, 0, nullptr, sc.data(), &nf), GPV_OK);                 // optional outputs left out
    EXPECT(sc[(size_t)nc * ns - 1] != guard && sc[(size_t)nc * ns] == guard);
    EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, 2, O.data(), ldo, nullptr, &nf), GPV_OK);
    EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 2, A.data(), lda, &nf), GPV_OK);                              // in place
    EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, 2, A.data(), lda, q.data(), &nf), GPV_OK);
    EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
    EXPECT(stamp0 == stamp1);
    // whitening and colouring beside it: buffers of their own
    {
        std::vector<double> G((size_t)nc * nc);
        double ld = 0.0;
        EXPECT_ST(gpv_plan_whiten(pl, A.data(), lda, 4, nullptr, 0, G.data(), &ld, &nf), GPV_OK);
        EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 4, O.data(), ldo, q.data(), sc.data(), &nf), GPV_OK);
    }
    // a vector of nuggets: another evaluation, the scale pre-pass runs again
    const long before = mockhip_launches();
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf), GPV_OK);
    const long per_call = mockhip_launches() - before;
    // the timed repetitions on what that call left: its device passes (the scale is the evaluation's, made once), no copies
    EXPECT_ST(gpv_plan_debug_loo_ms(pl, 2, ms), GPV_OK);
    EXPECT(mockhip_launches() - before == per_call + 2 * per_call);
    EXPECT(ms[0] == 0.125 && ms[1] == 0.125 && ms[2] == guard);                                // the mock's elapsed time, reps values
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, nugv.data(), n, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    const long before2 = mockhip_launches();
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf), GPV_OK);
    EXPECT(mockhip_launches() - before2 == per_call + 1);
    // the next evaluation leaves U alone: the resident one is stale
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 2, O.data(), ldo, &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, 2, O.data(), ldo, q.data(), &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_STATE);
    const long l1 = mockhip_launches();
    EXPECT_ST(gpv_plan_debug_loo_ms(pl, 2, ms), GPV_ERR_STATE);                                // ... for the timed repetitions too
    EXPECT(mockhip_launches() == l1);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    // unobserved locations
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf), GPV_OK);
    // a rebuilt posterior structure
    EXPECT_ST(gpv_plan_build_posterior(pl, revNN.data(), revCond.data()), GPV_OK);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf), GPV_OK);
    EXPECT_ST(gpv_plan_loo_index(pl, &e0, &e1, &e2), GPV_OK);                                  // reported again, not rebuilt
    EXPECT(e0 == w0 && e1 == w1 && e2 == w2);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    // ---- a star plan: one column of n2 - 1 entries, n2 - 1 empty ones
    {
        const int64_t n2 = 3000;
        std::vector<double> locs2((size_t)n2 * dim);
        for (auto &v : locs2) v = U(rng);
        std::vector<int> nnS, cdS;
        make_star(n2, nnS, cdS);
        pl = nullptr;
        EXPECT_ST(gpv_plan_create(&pl, 0, n2, dim, 2, locs2.data(), nnS.data(), cdS.data(), 0, n2), GPV_OK);
        if (pl) {
            EXPECT_ST(gpv_plan_loo_index(pl, &e0, &e1, &e2), GPV_OK);
            EXPECT(e0 == n2 - 1 && e1 == n2 - 1 && e2 == n2 - 1);
            EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
            std::vector<double> Z2((size_t)n2 * 3, 0.25), M2((size_t)n2 * 3 + 2, guard), v2((size_t)n2), s2((size_t)3 * ns);
            EXPECT_ST(gpv_plan_loo(pl, Z2.data(), n2, 3, M2.data(), n2, v2.data(), s2.data(), &nf), GPV_OK);
            EXPECT(M2[(size_t)n2 * 3] == guard && M2[(size_t)n2 * 3 - 1] != guard);
            EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
        }
    }
    // ---- the builder on host arrays, buffers of exactly the documented sizes
    {
        // four locations, P = 3: position 3 is nobody's neighbour, position 1 ends two sets
        const int32_t nn[4 * 3] = {-1, -1, 0,   -1, 0, 1,   0, 1, 2,   0, 2, 1};
        const int32_t rowid[4] = {0, 1, 3, 2};
        std::vector<int32_t> colptr(5, -9), owner(4, -9), col;
        int64_t nnz = -1;
        EXPECT_ST(gpv_loo_index_host(nn, rowid, 4, 4, 3, colptr.data(), owner.data(), nullptr, 0, &nnz), GPV_OK);     // the size first
        EXPECT(nnz == 6 && colptr[0] == 0 && colptr[4] == 6);
        col.assign((size_t)nnz, -9);
        EXPECT_ST(gpv_loo_index_host(nn, rowid, 4, 4, 3, colptr.data(), owner.data(), col.data(), nnz - 1, &nnz), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_loo_index_host(nn, rowid, 4, 4, 3, colptr.data(), owner.data(), col.data(), nnz, &nnz), GPV_OK);
        EXPECT(owner[0] == 0 && owner[1] == 1 * 3 + 1 && owner[2] == 3 * 3 + 2 && owner[3] == -1);
        EXPECT(colptr[1] == 3 && colptr[2] == 5 && colptr[3] == 6);
        EXPECT(col[0] == 1 * 3 + 0 && col[1] == 3 * 3 + 0 && col[2] == 2 * 3 + 0);             // position 0: sets 1, 2, 3 in that order
        EXPECT(col[3] == 3 * 3 + 1 && col[4] == 2 * 3 + 2);                                    // position 1: set 2, then set 3's OWN entry
        EXPECT(col[5] == 2 * 3 + 1);                                                           // position 2: set 3
        for (int32_t c : col) EXPECT(c >= 0 && c < 4 * 3);
        EXPECT_ST(gpv_loo_index_host(nn, rowid, 4, 4, 3, colptr.data(), owner.data(), col.data(), nnz, nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_loo_index_host(nullptr, rowid, 4, 4, 3, colptr.data(), owner.data(), col.data(), nnz, &nnz), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_loo_index_host(nn, rowid, 4, 2, 3, colptr.data(), owner.data(), col.data(), nnz, &nnz), GPV_ERR_BAD_ARG);   // index 2 >= Nlocs
        // rows x P >= 2^31: refused before any array is read
        nnz = -1;
        EXPECT_ST(gpv_loo_index_host(nullptr, nullptr, (int64_t)1 << 27, (int64_t)1 << 27, 16, nullptr, nullptr, nullptr, 0, &nnz), GPV_ERR_INDEX);
        EXPECT_ST(gpv_loo_index_host(nullptr, nullptr, 11184811, 11184811, 192, nullptr, nullptr, nullptr, 0, &nnz), GPV_ERR_INDEX);
        EXPECT(nnz == -1);
    }
    // a row shard
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 2, O.data(), ldo, &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_precision(pl, A.data(), lda, 2, O.data(), ldo, q.data(), &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_loo_index(pl, &e0, &e1, &e2), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // neighbours conditioned on as latent y
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_whiten_t(pl, A.data(), lda, 2, O.data(), ldo, &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_loo_index(pl, &e0, &e1, &e2), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // a long row (m + 1 = 100, the generic set kernel): one loop takes any row length
    std::vector<int> nnW, cdW;
    make_rows(n, 100, false, nnW, cdW);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, 100, locs.data(), nnW.data(), cdW.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf), GPV_OK);
        count_index(n, 100, nnW, w0, w1, w2);
        EXPECT_ST(gpv_plan_loo_index(pl, &e0, &e1, &e2), GPV_OK);
        EXPECT(e0 == w0 && e1 == w1 && e2 == w2 && e1 == 99);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("loo_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail, mockhip_launches());
    return g_fail ? 1 : 0;
}
