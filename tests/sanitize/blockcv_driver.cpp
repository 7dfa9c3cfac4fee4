// tests/sanitize/blockcv_driver.cpp — TEST INFRASTRUCTURE: the HOST code of gpv_plan_set_blocks / gpv_plan_block_cv /
// gpv_blocks_index_host (include/gpvecchia.h) under AddressSanitizer + UBSan, linked like tests/sanitize/loo_driver.cpp against
// tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  Kernels do not run, so this checks the argument checks, the
// state errors with a plan in hand, the block index (built on the host from the index arrays the plan keeps on the "device":
// its counts against a count made here, its entries on a small example, the refusals of bad labels and that a refused call
// keeps the blocks before it, the 32-bit guard, buffers of exactly the documented sizes), the shape of what is written (guard
// entries and the padding of the leading dimensions stay untouched), buffer growth across column counts, replaced blocks, and
// that nothing is left allocated — never numbers.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_blockcv_driver.py and tools/sanitize_host.sh.
#include "../../include/gpvecchia.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

extern "C" long mockhip_launches(void);
extern "C" long mockhip_live_allocations(void);
extern "C" int gpv_plan_debug_blockcv_ms(gpv_plan *pl, int reps, int parts, double *ms);   // developer aid, not in the public header

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

// the length of the set lists by the definition: for every block the rows that hold at least one member (make_rows: row k holds
// the ordered rows k - p + 1 .. k)
static int64_t count_refs(int64_t n, int p, const std::vector<int32_t> &lab)
{
    int64_t refs = 0;
    std::vector<int32_t> ids(lab);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    for (int32_t b : ids) {
        if (b < 0) continue;
        for (int64_t k = 0; k < n; ++k) {
            bool hit = false;
            for (int64_t v = std::max<int64_t>(0, k - p + 1); v <= k && !hit; ++v) hit = lab[(size_t)v] == b;
            refs += hit;
        }
    }
    return refs;
}

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);      // developer build: wait for the (mock) stream, not for a number no kernel will write
    const int64_t n = 200, lda = n + 3, ldo = n + 5;
    const int dim = 2, p = 11, nc = 16, ns = GPV_BLOCKCV_NSCORES;
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
    int64_t nf = -1, nbad = -1, nb = -1, nh = -1, nr = -1;
    int ms = -1;
    EXPECT(gpv_blockcv_nscores() == GPV_BLOCKCV_NSCORES && GPV_BLOCKCV_NSCORES == 8 && gpv_blockcv_max_block() == 64);
    std::vector<int32_t> tens((size_t)n), some((size_t)n, -1);
    for (int64_t k = 0; k < n; ++k) tens[(size_t)k] = (int32_t)(k / 10);                       // 20 blocks of 10 consecutive rows
    for (int64_t k = 0; k < n; k += 3) some[(size_t)k] = (int32_t)(150 + (k % 7));             // scattered, most locations kept

    gpv_plan *pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n), GPV_OK);
    if (!pl) return 1;
    // ---- arguments, before the state is looked at
    EXPECT_ST(gpv_plan_set_blocks(nullptr, tens.data(), &nb, &nh, &ms, &nr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_set_blocks(pl, nullptr, &nb, &nh, &ms, &nr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_set_blocks(pl, tens.data(), nullptr, &nh, &ms, &nr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_set_blocks(pl, tens.data(), &nb, nullptr, &ms, &nr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_set_blocks(pl, tens.data(), &nb, &nh, nullptr, &nr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_set_blocks(pl, tens.data(), &nb, &nh, &ms, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_block_cv(nullptr, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_block_cv(pl, nullptr, lda, 3, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 3, O.data(), ldo, q.data(), nullptr, &nf, &nbad), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), nullptr, &nbad), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), &nf, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 0, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 17, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), n - 1, 3, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 3, O.data(), n - 1, q.data(), sc.data(), &nf, &nbad), GPV_ERR_BAD_ARG);
    double tms[3] = {guard, guard, guard};
    EXPECT_ST(gpv_plan_debug_blockcv_ms(nullptr, 2, 7, tms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 0, 7, tms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 2, 7, nullptr), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 2, 0, tms), GPV_ERR_BAD_ARG);
    EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 2, 8, tms), GPV_ERR_BAD_ARG);
    // ---- state: no evaluation and no blocks
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 2, 7, tms), GPV_ERR_STATE);
    EXPECT(nf == -1 && nbad == -1 && O[0] == guard && q[0] == guard && sc[0] == guard);        // a refused call writes nothing
    // labels are refused before the device is touched, and nothing is reported
    {
        std::vector<int32_t> bad(tens);
        bad[7] = (int32_t)n;
        EXPECT_ST(gpv_plan_set_blocks(pl, bad.data(), &nb, &nh, &ms, &nr), GPV_ERR_BAD_ARG);    // a label >= Nlocs
        bad[7] = -2;
        EXPECT_ST(gpv_plan_set_blocks(pl, bad.data(), &nb, &nh, &ms, &nr), GPV_ERR_BAD_ARG);    // a label < -1
        std::fill(bad.begin(), bad.end(), -1);
        EXPECT_ST(gpv_plan_set_blocks(pl, bad.data(), &nb, &nh, &ms, &nr), GPV_ERR_BAD_ARG);    // no block at all
        for (int64_t k = 0; k < 65; ++k) bad[(size_t)k] = 4;
        EXPECT_ST(gpv_plan_set_blocks(pl, bad.data(), &nb, &nh, &ms, &nr), GPV_ERR_BAD_ARG);    // a block of 65
        EXPECT(nb == -1 && nh == -1 && ms == -1 && nr == -1);
        bad[64] = -1;
        EXPECT_ST(gpv_plan_set_blocks(pl, bad.data(), &nb, &nh, &ms, &nr), GPV_OK);             // 64 is the limit
        EXPECT(nb == 1 && nh == 64 && ms == 64 && nr == count_refs(n, p, bad));
    }
    // the index needs no evaluation
    EXPECT_ST(gpv_plan_set_blocks(pl, tens.data(), &nb, &nh, &ms, &nr), GPV_OK);
    EXPECT(nb == 20 && nh == n && ms == 10 && nr == count_refs(n, p, tens) && nr == 19 * 20 + 10);
    EXPECT(mockhip_launches() == 0);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_STATE);   // blocks, no evaluation
    EXPECT_ST(gpv_plan_set_data(pl, z.data()), GPV_OK);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_STATE);   // no GPV_WANT_U
    EXPECT(nf == -1 && nbad == -1 && O[0] == guard);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U | GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    double sums0[GPV_NSUMS], sums1[GPV_NSUMS];
    int64_t stamp0 = -1, stamp1 = -1;
    EXPECT_ST(gpv_plan_get_sums(pl, sums0), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp0), GPV_OK);
    const long l0 = mockhip_launches();
    EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 2, 7, tms), GPV_ERR_STATE);                        // a factor and blocks, but no columns left by a call yet
    EXPECT(mockhip_launches() == l0 && tms[0] == guard);
    // ---- buffer growth across column counts, shapes
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 3, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_OK);
    EXPECT(nf == 0 && nbad == 0);                                                              // (no kernel ran: the counters were cleared)
    EXPECT(O[0] != guard && O[(size_t)2 * ldo + n - 1] != guard && O[(size_t)3 * ldo] == guard);                 // 3 columns and no more
    EXPECT(sc[0] != guard && sc[(size_t)3 * ns - 1] != guard && sc[(size_t)3 * ns] == guard);
    EXPECT(q[0] != guard && q[(size_t)n - 1] != guard && q[(size_t)n] == guard);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, nc, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_OK); // a wider call: buffers grow
    for (int j = 0; j < nc; ++j) {
        EXPECT(O[(size_t)j * ldo] != guard && O[(size_t)j * ldo + n - 1] != guard);            // Nlocs rows per column
        for (int64_t k = n; k < ldo; ++k) EXPECT(O[(size_t)j * ldo + k] == guard);             // the padding of the leading dimension stays
    }
    for (size_t t = (size_t)ldo * nc; t < O.size(); ++t) EXPECT(O[t] == guard);
    EXPECT(sc[(size_t)nc * ns - 1] != guard && sc[(size_t)nc * ns] == guard);
    std::fill(sc.begin(), sc.end(), guard);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 5, nullptr, 0, nullptr, sc.data(), &nf, &nbad), GPV_OK);      // narrower, optional outputs left out
    EXPECT(sc[(size_t)5 * ns - 1] != guard && sc[(size_t)5 * ns] == guard);
    // gpv_plan_loo beside it: buffers of its own; the evaluation stays what it was
    {
        std::vector<double> s6((size_t)nc * GPV_LOO_NSCORES);
        EXPECT_ST(gpv_plan_loo(pl, A.data(), lda, 4, O.data(), ldo, q.data(), s6.data(), &nf), GPV_OK);
        EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 4, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_OK);
    }
    EXPECT_ST(gpv_plan_get_sums(pl, sums1), GPV_OK);
    EXPECT_ST(gpv_plan_factor_stamp(pl, &stamp1), GPV_OK);
    for (int t = 0; t < GPV_NSUMS; ++t) EXPECT(sums0[t] == sums1[t]);
    EXPECT(stamp0 == stamp1);
    // ---- the blocks are replaced; a refused replacement keeps them
    EXPECT_ST(gpv_plan_set_blocks(pl, some.data(), &nb, &nh, &ms, &nr), GPV_OK);
    EXPECT(nb == 7 && nh == (n + 2) / 3 && ms <= 64 && nr == count_refs(n, p, some));
    {
        std::vector<int32_t> none((size_t)n, -1);
        int64_t a = -1, b = -1, d = -1;
        int c = -1;
        EXPECT_ST(gpv_plan_set_blocks(pl, none.data(), &a, &b, &c, &d), GPV_ERR_BAD_ARG);
        EXPECT(a == -1 && b == -1 && c == -1 && d == -1);
    }
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_OK);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 2, A.data(), lda, q.data(), sc.data(), &nf, &nbad), GPV_OK);  // in place
    // a vector of nuggets: another evaluation, the scale pre-pass runs again
    const long before = mockhip_launches();
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_OK);
    const long per_call = mockhip_launches() - before;
    // the timed repetitions on what that call left: its device passes (the scale is the evaluation's, made once), no copies
    EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 2, 7, tms), GPV_OK);
    EXPECT(mockhip_launches() - before == per_call + 2 * per_call);
    EXPECT(tms[0] == 0.125 && tms[1] == 0.125 && tms[2] == guard);                             // the mock's elapsed time, reps values
    {                                                                                          // the three parts make up the whole
        const long b1 = mockhip_launches();
        EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 1, 1, tms), GPV_OK);
        EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 1, 2, tms), GPV_OK);
        EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 1, 4, tms), GPV_OK);
        EXPECT(mockhip_launches() - b1 == per_call);
    }
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, nugv.data(), n, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    const long before2 = mockhip_launches();
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_OK);  // the blocks outlive evaluations
    EXPECT(mockhip_launches() - before2 == per_call + 1);
    // the next evaluation leaves U alone: the resident one is stale
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_STATE);
    const long l1 = mockhip_launches();
    EXPECT_ST(gpv_plan_debug_blockcv_ms(pl, 2, 7, tms), GPV_ERR_STATE);                        // ... for the timed repetitions too
    EXPECT(mockhip_launches() == l1);
    EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
    // unobserved locations
    std::vector<int> obs((size_t)n, 1);
    obs[5] = 0;
    EXPECT_ST(gpv_plan_set_observed(pl, obs.data()), GPV_OK);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_STATE);
    EXPECT_ST(gpv_plan_set_observed(pl, nullptr), GPV_OK);
    EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_OK);
    EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    // ---- the builder on host arrays, buffers of exactly the documented sizes
    {
        // four locations, P = 3: position 3 is nobody's neighbour, position 1 ends two sets (stored sets 2 and 3)
        const int32_t nn[4 * 3] = {-1, -1, 0,   -1, 0, 1,   0, 1, 2,   0, 2, 1};
        const int32_t rowid[4] = {0, 1, 3, 2};
        const int32_t newpos[4] = {2, 0, 3, 1};                      // ordered row -> internal position
        const int32_t lab[4] = {3, 1, -1, 1};                        // label 1: ordered rows 1, 3 = positions 0, 1; label 3: row 0 = position 2
        std::vector<int32_t> memptr(3, -9), members(3, -9), setptr(3, -9), sets, blkloc(8, -9);
        EXPECT_ST(gpv_blocks_index_host(nn, rowid, 4, 4, 3, newpos, lab, &nb, &nh, &ms, &nr, nullptr, nullptr, nullptr, nullptr, 0, nullptr),
                  GPV_OK);                                           // the sizes first
        EXPECT(nb == 2 && nh == 3 && ms == 2 && nr == 6);
        sets.assign((size_t)nr, -9);
        EXPECT_ST(gpv_blocks_index_host(nn, rowid, 4, 4, 3, newpos, lab, &nb, &nh, &ms, &nr, memptr.data(), members.data(), setptr.data(),
                                        sets.data(), nr - 1, blkloc.data()), GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_blocks_index_host(nn, rowid, 4, 4, 3, newpos, lab, &nb, &nh, &ms, &nr, memptr.data(), members.data(), setptr.data(),
                                        sets.data(), nr, blkloc.data()), GPV_OK);
        EXPECT(memptr[0] == 0 && memptr[1] == 2 && memptr[2] == 3);
        EXPECT(members[0] == 0 && members[1] == 1 && members[2] == 2);
        EXPECT(setptr[0] == 0 && setptr[1] == 4 && setptr[2] == 6);
        EXPECT(sets[0] == 0 && sets[1] == 1 && sets[2] == 2 && sets[3] == 3);                  // positions 0 or 1: every set, each once
        EXPECT(sets[4] == 2 && sets[5] == 3);                                                  // position 2: sets 2 and 3
        const int32_t want_bl[8] = {0, 0, 0, 1, 1, 0, -1, -1};
        for (int t = 0; t < 8; ++t) EXPECT(blkloc[(size_t)t] == want_bl[t]);
        const int32_t twice[4] = {2, 0, 3, 0};
        EXPECT_ST(gpv_blocks_index_host(nn, rowid, 4, 4, 3, twice, lab, &nb, &nh, &ms, &nr, nullptr, nullptr, nullptr, nullptr, 0, nullptr),
                  GPV_ERR_BAD_ARG);                                  // newpos is no permutation
        EXPECT_ST(gpv_blocks_index_host(nn, rowid, 4, 4, 3, nullptr, nullptr, &nb, &nh, &ms, &nr, nullptr, nullptr, nullptr, nullptr, 0, nullptr),
                  GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_blocks_index_host(nn, rowid, 4, 4, 3, nullptr, lab, nullptr, &nh, &ms, &nr, nullptr, nullptr, nullptr, nullptr, 0, nullptr),
                  GPV_ERR_BAD_ARG);
        EXPECT_ST(gpv_blocks_index_host(nn, rowid, 4, 2, 3, nullptr, lab, &nb, &nh, &ms, &nr, nullptr, nullptr, nullptr, nullptr, 0, nullptr),
                  GPV_ERR_BAD_ARG);                                  // (labels and indices >= Nlocs)
        // rows x P >= 2^31: refused before any array is read
        nb = -1;
        EXPECT_ST(gpv_blocks_index_host(nullptr, nullptr, (int64_t)1 << 27, (int64_t)1 << 27, 16, nullptr, nullptr, &nb, &nh, &ms, &nr, nullptr,
                                        nullptr, nullptr, nullptr, 0, nullptr), GPV_ERR_INDEX);
        EXPECT(nb == -1);
    }
    // a row shard
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), revNN.data(), revCond.data(), 0, n / 2), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_set_blocks(pl, tens.data(), &nb, &nh, &ms, &nr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // neighbours conditioned on as latent y
    std::vector<int> nnY, cdY;
    make_rows(n, p, true, nnY, cdY);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, p, locs.data(), nnY.data(), cdY.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_set_blocks(pl, tens.data(), &nb, &nh, &ms, &nr), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_ERR_STATE);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    // a long row (m + 1 = 100, the generic set kernel): the slot loop takes any row length
    std::vector<int> nnW, cdW;
    make_rows(n, 100, false, nnW, cdW);
    pl = nullptr;
    EXPECT_ST(gpv_plan_create(&pl, 0, n, dim, 100, locs.data(), nnW.data(), cdW.data(), 0, n), GPV_OK);
    if (pl) {
        EXPECT_ST(gpv_plan_eval(pl, "matern", cp, 3, &tau, 1, GPV_WANT_U, nullptr, nullptr), GPV_OK);
        EXPECT_ST(gpv_plan_set_blocks(pl, tens.data(), &nb, &nh, &ms, &nr), GPV_OK);
        EXPECT(nb == 20 && nr == count_refs(n, 100, tens));
        EXPECT_ST(gpv_plan_block_cv(pl, A.data(), lda, 2, O.data(), ldo, q.data(), sc.data(), &nf, &nbad), GPV_OK);
        EXPECT_ST(gpv_plan_destroy(pl), GPV_OK);
    }
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("blockcv_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail, mockhip_launches());
    return g_fail ? 1 : 0;
}
