// tests/sanitize/krige_groups_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_krige_groups (include/gpvecchia.h)
// under AddressSanitizer + UBSan, linked like tests/sanitize/krige_driver.cpp against tests/sanitize/mock_hip_runtime.cpp
// instead of the HIP runtime.  Kernels do not run, so this checks the argument checks and the refusals before the device is
// touched (nothing written, nothing launched), the state errors with a plan in hand, the chunk arithmetic by the launches it
// makes (one search and one pass per row bucket present in a chunk), the shape of what is written (heap blocks of exactly the
// stated length for every output, the packed covariances included: a byte beyond them is the sanitizer's finding), that
// the plan's evaluation stays what it was, and that nothing is left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_krige_groups_driver.py and tools/sanitize_host.sh.
#include "../../include/gpvecchia.h"

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
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

// the outputs of one call as heap blocks of exactly the stated length, filled with a guard value
struct Out {
    int64_t nq, ng, ldm, ldg, ncov;
    int nc;
    std::unique_ptr<double[]> mean, var, gmean, gvar, cov;
    int64_t nf = -1;
    static constexpr double guard = -7.0;
    Out(int64_t nq_, int64_t ng_, int nc_, int64_t ncov_, int64_t padm = 0, int64_t padg = 0)
        : nq(nq_), ng(ng_), ldm(nq_ + padm), ldg(ng_ + padg), ncov(ncov_), nc(nc_)
    {
        // (the last column needs no padding behind it: ld * (nc - 1) + rows)
        mean.reset(new double[(size_t)(ldm * (nc - 1) + nq)]);
        var.reset(new double[(size_t)nq]);
        gmean.reset(new double[(size_t)(ldg * (nc - 1) + ng)]);
        gvar.reset(new double[(size_t)ng]);
        cov.reset(new double[(size_t)ncov]);
        fill();
    }
    void fill()
    {
        std::fill_n(mean.get(), ldm * (nc - 1) + nq, guard);
        std::fill_n(var.get(), nq, guard);
        std::fill_n(gmean.get(), ldg * (nc - 1) + ng, guard);
        std::fill_n(gvar.get(), ng, guard);
        std::fill_n(cov.get(), ncov, guard);
        nf = -1;
    }
    bool untouched() const
    {
        bool u = nf == -1;
        for (int64_t i = 0; i < ldm * (nc - 1) + nq; ++i) u = u && mean[(size_t)i] == guard;
        for (int64_t i = 0; i < nq; ++i) u = u && var[(size_t)i] == guard;
        for (int64_t i = 0; i < ldg * (nc - 1) + ng; ++i) u = u && gmean[(size_t)i] == guard;
        for (int64_t i = 0; i < ng; ++i) u = u && gvar[(size_t)i] == guard;
        for (int64_t i = 0; i < ncov; ++i) u = u && cov[(size_t)i] == guard;
        return u;
    }
    // every entry of the stated shape written, the padding of the leading dimensions not
    bool written() const
    {
        bool w = true;
        for (int j = 0; j < nc; ++j) {
            for (int64_t i = 0; i < nq; ++i) w = w && mean[(size_t)(j * ldm + i)] != guard;
            for (int64_t i = nq; i < ldm && j < nc - 1; ++i) w = w && mean[(size_t)(j * ldm + i)] == guard;
            for (int64_t i = 0; i < ng; ++i) w = w && gmean[(size_t)(j * ldg + i)] != guard;
            for (int64_t i = ng; i < ldg && j < nc - 1; ++i) w = w && gmean[(size_t)(j * ldg + i)] == guard;
        }
        for (int64_t i = 0; i < nq; ++i) w = w && var[(size_t)i] != guard;
        for (int64_t i = 0; i < ng; ++i) w = w && gvar[(size_t)i] != guard;
        for (int64_t i = 0; i < ncov; ++i) w = w && cov[(size_t)i] != guard;
        return w;
    }
};

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);      // developer build: wait for the (mock) stream, not for a number no kernel will write
    const int64_t n = 3000;                    // above the grid threshold of the search
    const int dim = 2, p = 11, m = 10, nc = 16;
    std::mt19937_64 rng(9);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> locs((size_t)n * dim), z((size_t)n), nugv((size_t)n, 0.2), Z((size_t)(n + 2) * nc, 0.5);
    for (auto &v : locs) v = U(rng);
    for (auto &v : z) v = U(rng) - 0.5;
    std::vector<int> revNN, revCond;
    make_rows(n, p, false, revNN, revCond);
    const double cp[3] = {1.0, 0.1, 1.5}, cpg[3] = {1.0, 0.1, 0.8}, cpe[4] = {1.0, 0.1, 0.5, 0.2}, cps[4] = {1.0, 0.1, 0.3, 2.5};
    const double tau = 0.1, sc2[2] = {0.1, 0.3};
    // groups of every bucket at m = 10: sizes 1 .. 54 (m + g = 11 .. 64), cycling
    const int sizes[] = {1, 6, 7, 22, 23, 54, 3, 2, 30, 1};
    const int64_t ng = 40;
    std::vector<int64_t> gptr((size_t)ng + 1, 0);
    int64_t ncov = 0;
    for (int64_t k = 0; k < ng; ++k) {
        const int g = sizes[k % 10];
        gptr[(size_t)k + 1] = gptr[(size_t)k] + g;
        ncov += (int64_t)g * (g + 1) / 2;
    }
    const int64_t nq = gptr[(size_t)ng];
    std::vector<double> ql((size_t)nq * dim), w((size_t)nq);
    for (auto &v : ql) v = 1.4 * U(rng) - 0.2;          // some outside the box
    for (auto &v : w) v = U(rng) - 0.5;
    std::vector<int> NNg((size_t)ng * m);
    for (int64_t k = 0; k < ng; ++k)
        for (int s = 0; s < m; ++s) NNg[(size_t)(k + (int64_t)s * ng)] = (s < 8) ? (int)((k * 7 + s) % n) + 1 : 0;
    std::vector<unsigned char> el((size_t)n, 1);
    for (int64_t i = 0; i < n; i += 3) el[(size_t)i] = 0;
    EXPECT(gpv_krige_groups_max_rows() == 64);

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    Out o(nq, ng, 1, ncov);
#define GROUPS(plan, cov_, par, npar, nug, nnug, Zp, ldz, ncols, q, nq_, gp, ng_, wt, m_, nn, scale, elig, chunk, O, covp) \
    gpv_plan_krige_groups(plan, cov_, par, npar, nug, nnug, Zp, ldz, ncols, q, nq_, gp, ng_, wt, m_, nn, scale, elig, chunk, \
                          (O).mean.get(), (O).ldm, (O).var.get(), (O).gmean.get(), (O).ldg, (O).gvar.get(), covp, &(O).nf)
#define PLAIN(plan, cov_, par, npar, gp, wt, m_, nn) \
    GROUPS(plan, cov_, par, npar, &tau, 1, Z.data(), n, 1, ql.data(), nq, gp, ng, wt, m_, nn, nullptr, nullptr, 0, o, o.cov.get())
    // ---- arguments, before the state is looked at and before the device is touched
    const long l0 = mockhip_launches();
    EXPECT_ST(PLAIN(nullptr, "matern", cp, 3, gptr.data(), nullptr, m, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(PLAIN(pl, nullptr, cp, 3, gptr.data(), nullptr, m, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(PLAIN(pl, "matern", nullptr, 3, gptr.data(), nullptr, m, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(PLAIN(pl, "matern", cp, 3, nullptr, nullptr, m, nullptr), GPV_ERR_BAD_ARG);                 // gptr
    EXPECT_ST(PLAIN(pl, "matern", cp, 4, gptr.data(), nullptr, m, nullptr), GPV_ERR_BAD_ARG);             // ncovparms
    EXPECT_ST(PLAIN(pl, "gauss", cp, 3, gptr.data(), nullptr, m, nullptr), GPV_ERR_COVTYPE);
    EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), nullptr, 0, nullptr), GPV_ERR_BAD_ARG);             // m
    EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), nullptr, 11, nullptr), GPV_ERR_UNSUPPORTED_M);      // 11 + 54 = 65
    EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), nullptr, 64, nullptr), GPV_ERR_UNSUPPORTED_M);
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, nullptr, 1, Z.data(), n, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 2, Z.data(), n, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);   // n_nuggets
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 0, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);   // ncols
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 17, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, nullptr, n, 2, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n - 1, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);  // ldz
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, nullptr, nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);        // qlocs
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, -1, o, nullptr), GPV_ERR_BAD_ARG);     // chunk
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq + 1, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);  // gptr[ng] != nq (and ldm < nq)
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, gptr.data(), -1, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, gptr.data(), 0, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);      // no group, nq > 0
    EXPECT_ST(gpv_plan_krige_groups(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o.mean.get(),
                                    nq - 1, o.var.get(), o.gmean.get(), ng, o.gvar.get(), nullptr, &o.nf), GPV_ERR_BAD_ARG);                                          // ldm
    EXPECT_ST(gpv_plan_krige_groups(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o.mean.get(),
                                    nq, o.var.get(), o.gmean.get(), ng - 1, o.gvar.get(), nullptr, &o.nf), GPV_ERR_BAD_ARG);                                          // ldg
    EXPECT_ST(gpv_plan_krige_groups(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o.mean.get(),
                                    nq, o.var.get(), nullptr, ng, o.gvar.get(), nullptr, &o.nf), GPV_ERR_BAD_ARG);                                                   // gmean
    EXPECT_ST(gpv_plan_krige_groups(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o.mean.get(),
                                    nq, o.var.get(), o.gmean.get(), ng, o.gvar.get(), nullptr, nullptr), GPV_ERR_BAD_ARG);                                           // n_failed
    {
        const double neg = -0.1, cpn[3] = {1.0, 0.1, 61.0}, scbad[2] = {0.1, 0.0};
        EXPECT_ST(GROUPS(pl, "matern", cp, 3, &neg, 1, Z.data(), n, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(PLAIN(pl, "matern", cpn, 3, gptr.data(), nullptr, m, nullptr), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, scbad, nullptr, 0, o, nullptr), GPV_ERR_BAD_ARG);
        std::vector<int64_t> gp(gptr);
        gp[5] = gp[4];                                                                          // an empty group
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gp.data(), nullptr, m, nullptr), GPV_ERR_BAD_ARG);
        gp[5] = gp[4] - 1;                                                                      // decreasing
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gp.data(), nullptr, m, nullptr), GPV_ERR_BAD_ARG);
        gp = gptr;
        gp[0] = 1;
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gp.data(), nullptr, m, nullptr), GPV_ERR_BAD_ARG);
        gp = gptr;
        gp[3] = nq + 5;                                                                         // beyond nq in the middle
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gp.data(), nullptr, m, nullptr), GPV_ERR_BAD_ARG);
        std::vector<double> wb(w);
        wb[7] = NAN;
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), wb.data(), m, nullptr), GPV_ERR_BAD_ARG);
        wb[7] = -INFINITY;
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), wb.data(), m, nullptr), GPV_ERR_BAD_ARG);
        std::vector<int> bad(NNg);
        bad[5] = (int)n + 1;
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), nullptr, m, bad.data()), GPV_ERR_INDEX);
        bad[5] = -1;
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), nullptr, m, bad.data()), GPV_ERR_INDEX);
    }
    // the plan's data, and none set
    EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, nullptr, 0, 1, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, o, nullptr), GPV_ERR_STATE);
    EXPECT(o.untouched() && mockhip_launches() == l0);                                          // a refused call writes and launches nothing
    // ---- no group: nothing to do, nothing needed
    {
        const int64_t g0 = 0;
        EXPECT_ST(gpv_plan_krige_groups(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, nullptr, 0, &g0, 0, nullptr, m, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr,
                                        nullptr, 0, nullptr, nullptr, &o.nf), GPV_OK);
        EXPECT(o.nf == 0 && mockhip_launches() == l0);
        EXPECT_ST(gpv_plan_krige_groups(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, nullptr, 0, nullptr, 0, nullptr, m, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr,
                                        nullptr, 0, nullptr, nullptr, &o.nf), GPV_OK);
        o.fill();
    }
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    // ---- chunk arithmetic: per chunk one search and one pass per row bucket present; one more launch packs given columns.
    // Sizes cycle {1, 6 | 7, 22 | 23, 54 | 3, 2 | 30, 1}: rows 11, 16 (bucket 16), 17, 32 (bucket 32), 33, 64 (bucket 64), 13, 12, 40, 11
    {
        struct { int64_t ng, chunk; long launches; } cases[] = {
            {1, 0, 2}, {2, 0, 2}, {3, 0, 3}, {5, 0, 4}, {ng, 0, 4}, {ng, 2, 20 * 2 + 0 /* searches */ + 0}, {ng, 10, 4 * 4}, {ng, ng + 5, 4}};
        // chunk = 2: the pairs (1, 6), (7, 22), (23, 54), (3, 2), (30, 1): one bucket each but the last (64 and 16): 4 * (4 * 2 + 3)
        cases[5].launches = 4 * (4 * 2 + 3);
        for (auto &c : cases) {
            const int64_t cq = gptr[(size_t)c.ng];
            int64_t cc = 0;
            for (int64_t k = 0; k < c.ng; ++k) cc += (gptr[(size_t)k + 1] - gptr[(size_t)k]) * (gptr[(size_t)k + 1] - gptr[(size_t)k] + 1) / 2;
            Out oc(cq, c.ng, 1, cc);
            std::vector<double> qc((size_t)cq * dim);                // the first cq rows of the column-major nq x dim array
            for (int t = 0; t < dim; ++t)
                for (int64_t i = 0; i < cq; ++i) qc[(size_t)(i + t * cq)] = ql[(size_t)(i + t * nq)];
            const long b = mockhip_launches();
            EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, nullptr, 0, 1, qc.data(), cq, gptr.data(), c.ng, nullptr, m, nullptr, nullptr, nullptr, c.chunk, oc,
                             oc.cov.get()), GPV_OK);
            if (mockhip_launches() - b != c.launches)
                std::fprintf(stderr, "ng %lld chunk %lld: %ld launches, wanted %ld\n", (long long)c.ng, (long long)c.chunk, mockhip_launches() - b, c.launches);
            EXPECT(mockhip_launches() - b == c.launches && oc.nf == 0);
            EXPECT(oc.written());
        }
    }
    // ---- columns: ldz, ldm and ldg wider than the data, every column written and nothing else; weights; no cov buffer
    {
        Out oc(nq, ng, nc, 1, 3, 2);
        const long b = mockhip_launches();
        EXPECT_ST(GROUPS(pl, "matern", cp, 3, nugv.data(), n, Z.data(), n + 2, nc, ql.data(), nq, gptr.data(), ng, w.data(), m, nullptr, nullptr, el.data(), 0, oc,
                         nullptr), GPV_OK);
        EXPECT(mockhip_launches() - b == 5);                         // the pack, the search, three buckets
        EXPECT(oc.cov[0] == Out::guard);
        oc.cov[0] = 0.0;
        EXPECT(oc.written());
        // given neighbours: no search
        Out og(nq, ng, 5, ncov);
        const long b2 = mockhip_launches();
        EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 5, ql.data(), nq, gptr.data(), ng, nullptr, m, NNg.data(), nullptr, nullptr, 7, og, og.cov.get()), GPV_OK);
        EXPECT(mockhip_launches() - b2 > 6 && og.written());
    }
    // every family; the search on scaled coordinates; the brute-force route; non-finite coordinates of a member
    {
        Out of(nq, ng, 3, ncov);
        EXPECT_ST(GROUPS(pl, "matern", cpg, 3, &tau, 1, Z.data(), n, 3, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, of, of.cov.get()), GPV_OK);
        EXPECT_ST(GROUPS(pl, "esqe", cpe, 4, &tau, 1, Z.data(), n, 3, ql.data(), nq, gptr.data(), ng, nullptr, 1, nullptr, nullptr, nullptr, 0, of, of.cov.get()), GPV_OK);
        EXPECT_ST(GROUPS(pl, "matern_scaledim", cps, 4, &tau, 1, Z.data(), n, 3, ql.data(), nq, gptr.data(), ng, w.data(), m, nullptr, sc2, el.data(), 33, of, of.cov.get()), GPV_OK);
        setenv("GPV_NN_BRUTE", "1", 1);
        ql[3] = NAN;
        EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 3, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, of, of.cov.get()), GPV_OK);
        unsetenv("GPV_NN_BRUTE");
        EXPECT_ST(GROUPS(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 3, ql.data(), nq, gptr.data(), ng, nullptr, m, nullptr, nullptr, nullptr, 0, of, of.cov.get()), GPV_OK);
        ql[3] = 0.5;
    }
    // ---- an evaluation stays what it was
    {
        double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), nullptr, m, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
        for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
        std::vector<double> Lent((size_t)n * p);
        EXPECT_ST(gpv_plan_get_Lentries(pl, Lent.data()), GPV_OK);                              // U is still that evaluation's
    }
    // unobserved locations
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    o.fill();
    EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), nullptr, m, nullptr), GPV_ERR_STATE);
    EXPECT(o.untouched());
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), nullptr, m, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    // a row shard
    pl = nullptr;
    o.fill();
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), nullptr, m, nullptr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // neighbours conditioned on as latent y
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, gptr.data(), nullptr, m, nullptr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    EXPECT(o.untouched());
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("krige_groups_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail, mockhip_launches());
    return g_fail ? 1 : 0;
}
