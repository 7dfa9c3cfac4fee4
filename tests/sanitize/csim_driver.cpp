// tests/sanitize/csim_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_cond_sim and gpv_csim_levels_host
// (include/gpvecchia.h) under AddressSanitizer + UBSan, linked like tests/sanitize/krige_driver.cpp against
// tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  Kernels do not run, so this checks the argument checks and
// the refusals before the device is touched (nothing written, nothing launched), the state errors with a plan in hand, the
// launch counts against the level schedule (the factor pass by its chunks; a sweep = one launch per wide level and one per run
// of narrow ones, between a packing or normals launch and an unpacking one; one sweep for the means and one per batch of 16
// draws), the shape of what is written (heap blocks of exactly the stated length for every output and for the caller's normals:
// a byte beyond them is the sanitizer's finding), that the plan's evaluation stays what it was, and that nothing is left
// allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_csim_driver.py and tools/sanitize_host.sh.
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
extern "C" int gpv_plan_debug_csim_chunk(gpv_plan *pl, int64_t chunk);      // developer aid: rows per launch of the factor pass

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
    int64_t nq, nsim, ldm, ldd;
    int nc;
    std::unique_ptr<double[]> mean, dev, sd;
    int64_t nlev = -1, nlaunch = -1, nf = -1;
    static constexpr double guard = -7.0;
    Out(int64_t nq_, int nc_, int64_t nsim_, int64_t padm = 0, int64_t padd = 0) : nq(nq_), nsim(nsim_), ldm(nq_ + padm), ldd(nq_ + padd), nc(nc_)
    {
        mean.reset(new double[(size_t)nmean()]);
        dev.reset(new double[(size_t)ndev()]);
        sd.reset(new double[(size_t)nq]);
        fill();
    }
    int64_t nmean() const { return ldm * (nc - 1) + nq; }            // (the last column needs no padding behind it)
    int64_t ndev() const { return nsim > 0 ? ldd * (nsim - 1) + nq : 0; }
    void fill()
    {
        std::fill_n(mean.get(), nmean(), guard);
        std::fill_n(dev.get(), ndev(), guard);
        std::fill_n(sd.get(), nq, guard);
        nlev = nlaunch = nf = -1;
    }
    bool untouched() const
    {
        bool u = nlev == -1 && nlaunch == -1 && nf == -1;
        for (int64_t i = 0; i < nmean(); ++i) u = u && mean[(size_t)i] == guard;
        for (int64_t i = 0; i < ndev(); ++i) u = u && dev[(size_t)i] == guard;
        for (int64_t i = 0; i < nq; ++i) u = u && sd[(size_t)i] == guard;
        return u;
    }
    // every entry of the stated shape written, the padding of the leading dimensions not
    bool written() const
    {
        bool w = true;
        for (int j = 0; j < nc; ++j) {
            for (int64_t i = 0; i < nq; ++i) w = w && mean[(size_t)(j * ldm + i)] != guard;
            for (int64_t i = nq; i < ldm && j < nc - 1; ++i) w = w && mean[(size_t)(j * ldm + i)] == guard;
        }
        for (int64_t j = 0; j < nsim; ++j) {
            for (int64_t i = 0; i < nq; ++i) w = w && dev[(size_t)(j * ldd + i)] != guard;
            for (int64_t i = nq; i < ldd && j < nsim - 1; ++i) w = w && dev[(size_t)(j * ldd + i)] == guard;
        }
        for (int64_t i = 0; i < nq; ++i) w = w && sd[(size_t)i] != guard;
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
    // The lists: rows 0 .. 299 and 650 .. 699 hold observations only (level 0: 350 rows, wide); row 300 + i names row i (level 1:
    // 300 rows, wide); rows 600 .. 649 name the row before them (levels 2 .. 51, one row each: ONE run of narrow levels).
    const int64_t nq = 700;
    const int64_t want_levels = 52, want_launches = 3;
    std::vector<int> NN((size_t)nq * m, 0);
    for (int64_t i = 0; i < nq; ++i) {
        for (int s = 0; s < 8; ++s) NN[(size_t)(i + (int64_t)s * nq)] = (int)((i * 7 + s) % n) + 1;
        if (i >= 300 && i < 600) NN[(size_t)(i + 8 * nq)] = (int)(n + 1 + (i - 300));
        if (i >= 600 && i < 650) NN[(size_t)(i + 9 * nq)] = (int)(n + i);                  // (the largest legal id of row i)
    }
    std::vector<double> ql((size_t)nq * dim);
    for (auto &v : ql) v = 1.4 * U(rng) - 0.2;          // some outside the box
    std::vector<unsigned char> el((size_t)n, 1);
    for (int64_t i = 0; i < n; i += 3) el[(size_t)i] = 0;

    // ---- the schedule on the host, no plan and no device
    {
        std::unique_ptr<int32_t[]> level(new int32_t[(size_t)nq]), order(new int32_t[(size_t)nq]);
        std::unique_ptr<int64_t[]> levptr(new int64_t[(size_t)nq + 1]);
        int64_t nlev = -1;
        const long l0 = mockhip_launches();
        EXPECT_ST(gpv_csim_levels_host(NN.data(), nq, m, n, level.get(), order.get(), levptr.get(), &nlev), GPV_OK);
        EXPECT(nlev == want_levels && levptr[0] == 0 && levptr[1] == 350 && levptr[2] == 650 && levptr[(size_t)nlev] == nq);
        EXPECT(level[0] == 0 && level[300] == 1 && level[600] == 2 && level[649] == 51 && level[650] == 0 && order[300] == 650);
        int64_t launches = 0;
        bool run = false;
        for (int64_t l = 0; l < nlev; ++l) {
            const bool narrow = levptr[(size_t)l + 1] - levptr[(size_t)l] <= 256;
            launches += narrow ? (run ? 0 : 1) : 1;
            run = narrow;
        }
        EXPECT(launches == want_launches);
        std::vector<int> bad(NN);
        bad[(size_t)(5 + 9 * nq)] = (int)(n + 5 + 1);                                         // its own row
        EXPECT_ST(gpv_csim_levels_host(bad.data(), nq, m, n, level.get(), order.get(), levptr.get(), &nlev), GPV_ERR_INDEX);
        bad[(size_t)(5 + 9 * nq)] = -1;
        EXPECT_ST(gpv_csim_levels_host(bad.data(), nq, m, n, level.get(), order.get(), levptr.get(), &nlev), GPV_ERR_INDEX);
        EXPECT_ST(gpv_csim_levels_host(nullptr, nq, m, n, level.get(), order.get(), levptr.get(), &nlev), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_csim_levels_host(NN.data(), nq, 0, n, level.get(), order.get(), levptr.get(), &nlev), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_csim_levels_host(NN.data(), nq, m, n, level.get(), order.get(), levptr.get(), nullptr), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_csim_levels_host(NN.data(), nq, m, ((int64_t)1 << 31), level.get(), order.get(), levptr.get(), &nlev), GPV_ERR_INDEX);
        EXPECT_ST(gpv_csim_levels_host(nullptr, 0, m, n, nullptr, nullptr, levptr.get(), &nlev), GPV_OK);
        EXPECT(nlev == 0 && levptr[0] == 0 && mockhip_launches() == l0);
    }

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    const int64_t nsim = 20;
    std::unique_ptr<double[]> E(new double[(size_t)((nq + 1) * (nsim - 1) + nq)]);                // lde = nq + 1, exactly
    std::fill_n(E.get(), (nq + 1) * (nsim - 1) + nq, 0.25);
    Out o(nq, 1, nsim);
#define CSIM(plan, cov_, par, npar, nug, nnug, Zp, ldz, ncols, q, nq_, m_, nn, scale, elig, Ep, lde, seed, col0, nsim_, O)        \
    gpv_plan_cond_sim(plan, cov_, par, npar, nug, nnug, Zp, ldz, ncols, q, nq_, m_, nn, scale, elig, Ep, lde, seed, col0, nsim_, \
                      (O).mean.get(), (O).ldm, (O).dev.get(), (O).ldd, (O).sd.get(), &(O).nlev, &(O).nlaunch, &(O).nf)
#define PLAIN(plan, cov_, par, npar, m_, nn) \
    CSIM(plan, cov_, par, npar, &tau, 1, Z.data(), n, 1, ql.data(), nq, m_, nn, nullptr, nullptr, nullptr, 0, 5, 0, nsim, o)
    // ---- arguments, before the state is looked at and before the device is touched
    const long l0 = mockhip_launches();
    EXPECT_ST(PLAIN(nullptr, "matern", cp, 3, m, NN.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(PLAIN(pl, nullptr, cp, 3, m, NN.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(PLAIN(pl, "matern", nullptr, 3, m, NN.data()), GPV_ERR_BAD_ARG);
    EXPECT_ST(PLAIN(pl, "matern", cp, 4, m, NN.data()), GPV_ERR_BAD_ARG);                       // ncovparms
    EXPECT_ST(PLAIN(pl, "gauss", cp, 3, m, NN.data()), GPV_ERR_COVTYPE);
    EXPECT_ST(PLAIN(pl, "matern", cp, 3, 0, NN.data()), GPV_ERR_BAD_ARG);                       // m
    EXPECT_ST(PLAIN(pl, "matern", cp, 3, 64, nullptr), GPV_ERR_UNSUPPORTED_M);
    EXPECT_ST(CSIM(pl, "matern", cp, 3, nullptr, 1, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_BAD_ARG);
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 2, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_BAD_ARG);   // n_nuggets
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 0, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_BAD_ARG);   // ncols
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 17, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_BAD_ARG);
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, nullptr, n, 2, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_BAD_ARG);
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n - 1, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_BAD_ARG);  // ldz
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, nullptr, nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_BAD_ARG);        // qlocs
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), -1, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_BAD_ARG);       // nq
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, -1, o), GPV_ERR_BAD_ARG);         // nsim
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, -1, nsim, o), GPV_ERR_BAD_ARG);      // col0
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, E.get(), nq - 1, 5, 0, nsim, o), GPV_ERR_BAD_ARG); // lde
    EXPECT_ST(gpv_plan_cond_sim(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o.mean.get(),
                                nq - 1, o.dev.get(), nq, o.sd.get(), &o.nlev, &o.nlaunch, &o.nf), GPV_ERR_BAD_ARG);                                        // ldm
    EXPECT_ST(gpv_plan_cond_sim(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o.mean.get(),
                                nq, o.dev.get(), nq - 1, o.sd.get(), &o.nlev, &o.nlaunch, &o.nf), GPV_ERR_BAD_ARG);                                        // ldd
    EXPECT_ST(gpv_plan_cond_sim(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o.mean.get(),
                                nq, nullptr, nq, o.sd.get(), &o.nlev, &o.nlaunch, &o.nf), GPV_ERR_BAD_ARG);                                                // dev
    EXPECT_ST(gpv_plan_cond_sim(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o.mean.get(),
                                nq, o.dev.get(), nq, nullptr, &o.nlev, &o.nlaunch, &o.nf), GPV_ERR_BAD_ARG);                                               // sd
    EXPECT_ST(gpv_plan_cond_sim(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o.mean.get(),
                                nq, o.dev.get(), nq, o.sd.get(), &o.nlev, &o.nlaunch, nullptr), GPV_ERR_BAD_ARG);                                          // n_failed
    {
        const double neg = -0.1, cpn[3] = {1.0, 0.1, 61.0}, scbad[2] = {0.1, 0.0};
        EXPECT_ST(CSIM(pl, "matern", cp, 3, &neg, 1, Z.data(), n, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_BAD_ARG);
        EXPECT_ST(PLAIN(pl, "matern", cpn, 3, m, NN.data()), GPV_ERR_UNSUPPORTED_NU);
        EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, ql.data(), nq, m, nullptr, scbad, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_BAD_ARG);
        std::vector<int> bad(NN);
        bad[(size_t)(5 + 9 * nq)] = (int)(n + 5 + 1);                                           // a forward id: the row itself
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, m, bad.data()), GPV_ERR_INDEX);
        bad[(size_t)(5 + 9 * nq)] = (int)(n + nq);                                              // the last row, from row 5
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, m, bad.data()), GPV_ERR_INDEX);
        bad[(size_t)(5 + 9 * nq)] = -1;
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, m, bad.data()), GPV_ERR_INDEX);
    }
    // the plan's data, and none set
    EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, nullptr, 0, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, nsim, o), GPV_ERR_STATE);
    EXPECT(o.untouched() && mockhip_launches() == l0);                                          // a refused call writes and launches nothing
    // ---- no location: nothing to do, nothing needed
    EXPECT_ST(gpv_plan_cond_sim(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 1, nullptr, 0, m, nullptr, nullptr, nullptr, nullptr, 0, 5, 0, nsim, nullptr, 0, nullptr,
                                0, nullptr, &o.nlev, &o.nlaunch, &o.nf), GPV_OK);
    EXPECT(o.nf == 0 && o.nlev == 0 && o.nlaunch == 0 && mockhip_launches() == l0);
    o.fill();
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    // ---- launches against the schedule.  One call = the factor pass in its chunks + (1 + batches) sweeps of
    // (packing or normals) + want_launches + unpacking, and one launch more that packs given data columns
    {
        const int64_t sweep = want_launches + 2;
        struct { int64_t chunk, col0, nsim; bool given_E, given_Z; long launches; } cases[] = {
            {0, 0, 0, false, false, (long)(1 + sweep)},                          // means only, the plan's data
            {0, 0, 0, false, true, (long)(1 + 1 + sweep)},
            {0, 0, 20, true, false, (long)(1 + 3 * sweep)},                      // the caller's normals: 16 + 4
            {0, 0, 16, false, false, (long)(1 + 2 * sweep)},                     // one batch of the generator's
            {0, 15, 2, false, false, (long)(1 + 3 * sweep)},                     // draws 15 and 16: two batches
            {0, 17, 1, false, false, (long)(1 + 2 * sweep)},
            {100, 0, 1, false, false, (long)(7 + 2 * sweep)},                    // 700 rows in chunks of 100
            {299, 0, 1, true, true, (long)(1 + 3 + 2 * sweep)},
            {nq + 5, 0, 1, false, false, (long)(1 + 2 * sweep)}};
        for (auto &c : cases) {
            Out oc(nq, 1, c.nsim, 2, 1);
            EXPECT_ST(gpv_plan_debug_csim_chunk(pl, c.chunk), GPV_OK);
            const long b = mockhip_launches();
            EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, c.given_Z ? Z.data() : nullptr, c.given_Z ? n : 0, 1, ql.data(), nq, m, NN.data(), nullptr, nullptr,
                           c.given_E ? E.get() : nullptr, nq + 1, 5, c.col0, c.nsim, oc), GPV_OK);
            if (mockhip_launches() - b != c.launches)
                std::fprintf(stderr, "chunk %lld col0 %lld nsim %lld: %ld launches, wanted %ld\n", (long long)c.chunk, (long long)c.col0, (long long)c.nsim,
                             mockhip_launches() - b, c.launches);
            EXPECT(mockhip_launches() - b == c.launches && oc.nf == 0 && oc.nlev == want_levels && oc.nlaunch == want_launches);
            EXPECT(oc.written());
        }
        EXPECT_ST(gpv_plan_debug_csim_chunk(pl, -1), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_plan_debug_csim_chunk(pl, 0), GPV_OK);
    }
    // ---- columns: ldz, ldm and ldd wider than the data, every column written and nothing else; a vector of nuggets; the search
    {
        Out oc(nq, nc, 3, 3, 2);
        EXPECT_ST(CSIM(pl, "matern", cp, 3, nugv.data(), n, Z.data(), n + 2, nc, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, 3, oc), GPV_OK);
        EXPECT(oc.written() && oc.nlev == want_levels);
        // the library's search (the mock's device memory holds zeros: every list comes back empty, one level)
        Out os(nq, 3, 2);
        const long b = mockhip_launches();
        EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 3, ql.data(), nq, m, nullptr, nullptr, el.data(), nullptr, 0, 5, 0, 2, os), GPV_OK);
        EXPECT(mockhip_launches() - b >= 1 + 1 + 1 + 2 * 3 && os.written() && os.nlev == 1 && os.nlaunch == 1);
    }
    // every family; the search on scaled coordinates; the brute-force route; non-finite coordinates of a location
    {
        Out of(nq, 3, 2);
        EXPECT_ST(CSIM(pl, "matern", cpg, 3, &tau, 1, Z.data(), n, 3, ql.data(), nq, m, NN.data(), nullptr, nullptr, nullptr, 0, 5, 0, 2, of), GPV_OK);
        EXPECT_ST(CSIM(pl, "esqe", cpe, 4, &tau, 1, Z.data(), n, 3, ql.data(), nq, 1, nullptr, nullptr, nullptr, nullptr, 0, 5, 0, 2, of), GPV_OK);
        EXPECT_ST(CSIM(pl, "matern_scaledim", cps, 4, &tau, 1, Z.data(), n, 3, ql.data(), nq, m, nullptr, sc2, el.data(), nullptr, 0, 5, 0, 2, of), GPV_OK);
        EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 3, ql.data(), nq, 63, nullptr, nullptr, nullptr, nullptr, 0, 5, 0, 2, of), GPV_OK);
        setenv("GPV_NN_BRUTE", "1", 1);
        ql[3] = NAN;
        EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 3, ql.data(), nq, m, nullptr, nullptr, nullptr, nullptr, 0, 5, 0, 2, of), GPV_OK);
        unsetenv("GPV_NN_BRUTE");
        EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 3, ql.data(), nq, m, nullptr, nullptr, nullptr, nullptr, 0, 5, 0, 2, of), GPV_OK);
        ql[3] = 0.5;
        // no observation eligible: the lists hold prediction locations alone
        std::vector<unsigned char> none((size_t)n, 0);
        EXPECT_ST(CSIM(pl, "matern", cp, 3, &tau, 1, Z.data(), n, 3, ql.data(), nq, m, nullptr, nullptr, none.data(), nullptr, 0, 5, 0, 2, of), GPV_OK);
    }
    // ---- an evaluation stays what it was
    {
        double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
        int64_t st0 = -1, st1 = -2;
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
        EXPECT_ST(gpv_plan_factor_stamp(pl, &st0), GPV_OK);
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, m, NN.data()), GPV_OK);
        EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
        EXPECT_ST(gpv_plan_factor_stamp(pl, &st1), GPV_OK);
        for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
        EXPECT(st0 == st1);
        std::vector<double> Lent((size_t)n * p);
        EXPECT_ST(gpv_plan_get_Lentries(pl, Lent.data()), GPV_OK);                              // U is still that evaluation's
    }
    // unobserved locations
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    o.fill();
    EXPECT_ST(PLAIN(pl, "matern", cp, 3, m, NN.data()), GPV_ERR_STATE);
    EXPECT(o.untouched());
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(PLAIN(pl, "matern", cp, 3, m, NN.data()), GPV_OK);
    EXPECT(o.written());
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    // a row shard
    pl = nullptr;
    o.fill();
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, m, NN.data()), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // neighbours conditioned on as latent y
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(PLAIN(pl, "matern", cp, 3, m, NN.data()), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    EXPECT(o.untouched());
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("csim_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail, mockhip_launches());
    return g_fail ? 1 : 0;
}
