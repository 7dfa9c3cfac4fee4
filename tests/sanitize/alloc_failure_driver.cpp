// tests/sanitize/alloc_failure_driver.cpp — TEST INFRASTRUCTURE (tests/test_host_drivers.py): every device or pinned allocation
// of one pass through the C ABI (include/gpvecchia.h) is made to fail once, under AddressSanitizer + UBSan, against
// tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  The pass runs once undisturbed, which counts its A
// allocations and records its outputs; then for every k < A the k-th allocation returns hipErrorOutOfMemory and the failed call
// must come back as GPV_ERR_HIP naming hipMalloc / hipHostMalloc, succeed when repeated on the same plan, the rest of the
// pass must give the outputs of the undisturbed one, and nothing may stay allocated.  Kernels do not run: the outputs are
// whatever zero-filled "device" memory produces, so equal outputs say that the same calls read the same buffers, not more.
#include "../../include/gpvecchia.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

extern "C" long mockhip_live_allocations(void);
extern "C" long mockhip_allocs(void);
extern "C" void mockhip_fail_alloc_at(long k);

static int g_fail = 0;
#define EXPECT(cond)                                                                           \
    do {                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

struct Data {
    int64_t n = 300;
    int dim = 2, p = 21;                                                   // m = 20
    std::vector<double> locs, z, tau, dist;
    std::vector<int> revNN, revCond, revCondZ;                             // SGV conditioning, and cond.yz = 'z'
};

static Data make_data()
{
    Data c;
    const int64_t n = c.n;
    const int dim = c.dim, p = c.p;
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> raw((size_t)n * dim);
    for (auto &v : raw) v = U(rng);
    std::vector<int> ord((size_t)n);
    EXPECT(gpv_order_maxmin_exact(raw.data(), n, dim, ord.data()) == GPV_OK);
    c.locs.resize((size_t)n * dim);
    for (int64_t k = 0; k < n; ++k)
        for (int t = 0; t < dim; ++t) c.locs[k + t * n] = raw[(size_t)(ord[(size_t)k] - 1) + (size_t)t * n];
    std::vector<int> NN((size_t)n * p, 0), Cond((size_t)n * p, 0);
    std::vector<std::pair<double, int>> d;
    for (int64_t k = 0; k < n; ++k) {                                      // nearest previous neighbours, self first, 1-based
        d.clear();
        for (int64_t j = 0; j <= k; ++j) {
            double s = 0;
            for (int t = 0; t < dim; ++t) { const double df = c.locs[k + t * n] - c.locs[j + t * n]; s += df * df; }
            d.emplace_back(std::sqrt(s), (int)j);
        }
        std::stable_sort(d.begin(), d.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        const int cnt = (int)std::min<size_t>(d.size(), (size_t)p);
        for (int q = 0; q < cnt; ++q) NN[k + (int64_t)q * n] = d[(size_t)q].second + 1;
    }
    EXPECT(gpv_whichCondOnLatent(NN.data(), n, p, n + 1, Cond.data()) == GPV_OK);
    c.revNN.resize((size_t)n * p);
    c.revCond.resize((size_t)n * p);
    c.revCondZ.resize((size_t)n * p);
    for (int64_t k = 0; k < n; ++k)
        for (int j = 0; j < p; ++j) {
            const int v = NN[k + (int64_t)(p - 1 - j) * n];
            c.revNN[k + (int64_t)j * n] = v;
            c.revCond[k + (int64_t)j * n] = v ? Cond[k + (int64_t)(p - 1 - j) * n] : INT_MIN;
            c.revCondZ[k + (int64_t)j * n] = v ? (j == p - 1 ? 1 : 0) : INT_MIN;   // only the point itself is latent
        }
    c.z.resize((size_t)n);
    c.tau.resize((size_t)n);
    for (auto &v : c.z) v = U(rng) - 0.5;
    for (auto &v : c.tau) v = 0.05 + 0.2 * U(rng);
    c.dist.resize(500);
    for (size_t i = 0; i < c.dist.size(); ++i) c.dist[i] = 0.002 * (double)i;
    return c;
}

// One pass: the steps in order, each of them a call (or a few) that can be repeated after it failed.  Returns how many steps
// failed once; `out` collects every number the calls hand back.
static int run_pass(const Data &c, std::vector<double> &out)
{
    const int64_t n = c.n;
    const int p = c.p, nint = (int)n, one = 1, three = 3;
    gpv_plan *pl = nullptr, *plz = nullptr;
    const double cp[3] = {1.0, 0.1, 1.5}, cpg[3] = {1.0, 0.1, 1.1}, tau1 = 0.1;
    double sums[GPV_NSUMS];
    std::vector<double> v((size_t)n), w((size_t)n * p), gram(32 * 32);
    auto keep = [&](const double *x, size_t cnt) { out.insert(out.end(), x, x + cnt); };
    auto eval_post = [&]() {
        int st = gpv_plan_eval(pl, "matern", cp, 3, c.tau.data(), n, GPV_WANT_DENOM | GPV_WANT_MEAN, nullptr, nullptr);
        if (st == GPV_OK) st = gpv_plan_get_sums(pl, sums);
        if (st == GPV_OK) st = gpv_plan_get_posterior_mean(pl, v.data());
        if (st == GPV_OK) { keep(sums, GPV_NSUMS); keep(v.data(), v.size()); }
        return st;
    };
    auto draws = [&](int64_t nd) {
        std::vector<double> mean((size_t)n), var((size_t)n), dmax((size_t)nd), dmean((size_t)nd);
        const int st = gpv_plan_draws_summary(pl, nd, 7, 0, nullptr, 0, 0, nullptr, nullptr, mean.data(), var.data(), nullptr, dmax.data(),
                                              dmean.data());
        if (st == GPV_OK) { keep(mean.data(), mean.size()); keep(var.data(), var.size()); keep(dmax.data(), dmax.size()); }
        return st;
    };
    const std::vector<std::function<int()>> steps = {
        [&] { return gpv_plan_create(&pl, 0, n, c.dim, p, c.locs.data(), c.revNN.data(), c.revCond.data(), 0, n); },
        [&] { return gpv_plan_set_data(pl, c.z.data()); },
        [&] {
            int st = gpv_plan_eval(pl, "matern", cp, 3, &tau1, 1, GPV_WANT_LOGLIK_Z, nullptr, nullptr);
            if (st == GPV_OK) st = gpv_plan_get_sums(pl, sums);
            if (st == GPV_OK) keep(sums, GPV_NSUMS);
            return st;
        },
        [&] { return gpv_plan_build_posterior(pl, c.revNN.data(), c.revCond.data()); },
        eval_post,
        [&] {   // variances of 40 unit rows (two batches), then the Gram matrix of the first 32 (the most one call takes)
            std::vector<int64_t> hptr(41);
            std::vector<int32_t> hidx(40);
            std::vector<double> hval(40, 1.0), vars(40);
            for (int r = 0; r <= 40; ++r) hptr[(size_t)r] = r;
            for (int r = 0; r < 40; ++r) hidx[(size_t)r] = (int32_t)(n - 1 - 3 * r);
            int st = gpv_plan_lincomb(pl, 40, hptr.data(), hidx.data(), hval.data(), vars.data(), nullptr);
            if (st == GPV_OK) st = gpv_plan_lincomb(pl, 32, hptr.data(), hidx.data(), hval.data(), vars.data(), gram.data());
            if (st == GPV_OK) { keep(vars.data(), vars.size()); keep(gram.data(), gram.size()); }
            return st;
        },
        [&] {
            std::vector<double> E((size_t)33 * n, 0.25), X((size_t)33 * n);
            const int st = gpv_plan_solve_t(pl, 33, E.data(), n, X.data(), n);
            if (st == GPV_OK) keep(X.data(), X.size());
            return st;
        },
        [&] { return draws(32); },
        [&] { return draws(96); },
        [&] { return gpv_plan_build_posterior(pl, c.revNN.data(), c.revCond.data()); },
        eval_post,
        [&] {
            int st = gpv_plan_eval(pl, "matern", cp, 3, c.tau.data(), n, GPV_WANT_U | GPV_WANT_NUMERATOR, nullptr, nullptr);
            if (st == GPV_OK) st = gpv_plan_get_Lentries(pl, w.data());
            if (st == GPV_OK) keep(w.data(), w.size());
            return st;
        },
        [&] {
            std::vector<double> Z((size_t)2 * n);
            const int st = gpv_plan_get_Zentries(pl, Z.data());
            if (st == GPV_OK) keep(Z.data(), Z.size());
            return st;
        },
        [&] {   // general nu, three times: both copies of the table are set up and the first is come back to
            int st = GPV_OK;
            for (int rep = 0; rep < 3 && st == GPV_OK; ++rep) {
                st = gpv_plan_eval(pl, "matern", cpg, 3, c.tau.data(), n, GPV_WANT_NUMERATOR, nullptr, nullptr);
                if (st == GPV_OK) st = gpv_plan_get_sums(pl, sums);
            }
            if (st == GPV_OK) keep(sums, GPV_NSUMS);
            return st;
        },
        [&] {
            const double lik[3] = {2.0, 0.3, 0.0};
            std::vector<double> zc((size_t)n), pm((size_t)n, 0.0);
            for (int64_t k = 0; k < n; ++k) zc[(size_t)k] = (double)(k % 4);
            return gpv_plan_vl_begin(pl, 2 /* poisson */, lik, zc.data(), pm.data(), nullptr);
        },
        [&] {
            double dmax = 0;
            int fl = 0;
            const int st = gpv_plan_vl_step(pl, "matern", cp, 3, &dmax, &fl);
            if (st == GPV_OK) keep(&dmax, 1);
            return st;
        },
        [&] { return gpv_plan_create(&plz, 0, n, c.dim, p, c.locs.data(), c.revNN.data(), c.revCondZ.data(), 0, n); },
        [&] { return gpv_plan_set_data(plz, c.z.data()); },
        [&] {
            double ll = 0, grad[4];
            int64_t nf = 0;
            std::vector<double> rows((size_t)n * 5);
            const int st = gpv_plan_loglik_grad(plz, "matern", cp, 3, tau1, &ll, grad, &nf, rows.data());
            if (st == GPV_OK) { keep(&ll, 1); keep(grad, 2); keep(rows.data(), rows.size()); }   // (grad[2], the smoothness, is NaN)
            return st;
        },
        [&] {
            const char *ct = "matern";
            int nf = 0, st = -1;
            std::vector<double> Z((size_t)2 * n);
            gpv_U_NZentries(&one, &nint, &nint, &c.dim, &p, c.locs.data(), c.revNN.data(), c.revCond.data(), c.tau.data(), c.tau.data(), &ct,
                            cp, &three, w.data(), Z.data(), &nf, &st);
            if (st == GPV_OK) { keep(w.data(), w.size()); keep(Z.data(), Z.size()); }
            return st;
        },
        [&] {
            int nf = 0, st = -1;
            std::vector<double> K((size_t)n * n, 0.0), Z((size_t)2 * n);
            for (int64_t i = 0; i < n; ++i) K[(size_t)(i * n + i)] = 1.0;
            gpv_U_NZentries_mat(&one, &nint, &nint, &p, c.revNN.data(), c.tau.data(), K.data(), w.data(), Z.data(), &nf, &st);
            if (st == GPV_OK) { keep(w.data(), w.size()); keep(Z.data(), Z.size()); }
            return st;
        },
        [&] {
            int st = -1;
            const int ne = (int)c.dist.size();
            std::vector<double> cv(c.dist.size());
            gpv_MaternFun(c.dist.data(), &ne, cp, cv.data(), &st);
            if (st == GPV_OK) keep(cv.data(), cv.size());
            return st;
        },
        [&] { return gpv_plan_cache_clear(); },
    };
    int failed = 0;
    for (size_t i = 0; i < steps.size(); ++i) {
        const size_t mark = out.size();
        int st = steps[i]();
        if (st != GPV_OK) {                                                // the armed allocation: once, and it says so
            ++failed;
            char txt[256] = "";
            const int code = gpv_last_hip_error(txt, (int)sizeof(txt));
            const bool named = std::strstr(txt, "hipMalloc") || std::strstr(txt, "hipHostMalloc");
            if (st != GPV_ERR_HIP || code == 0 || !named || !std::strstr(txt, "gpv_api.hip:")) {
                std::fprintf(stderr, "step %zu: status %d (%s), last error %d \"%s\"\n", i, st, gpv_status_string(st), code, txt);
                ++g_fail;
            }
            out.resize(mark);
            st = steps[i]();                                               // the same call on the same plan, undisturbed
            if (st != GPV_OK) {
                std::fprintf(stderr, "step %zu: the repeated call returned %d (%s)\n", i, st, gpv_status_string(st));
                ++g_fail;
                break;
            }
        }
    }
    EXPECT(gpv_plan_destroy(pl) == GPV_OK);
    EXPECT(gpv_plan_destroy(plz) == GPV_OK);
    EXPECT(gpv_plan_cache_clear() == GPV_OK);
    mockhip_fail_alloc_at(-1);
    return failed;
}

int main()
{
    setenv("GPV_NO_SEQ_HANDOFF", "1", 1);      // developer build: wait for the (mock) stream, not for a number no kernel will write
    const Data c = make_data();
    std::vector<double> want, got;
    const long a0 = mockhip_allocs();
    EXPECT(run_pass(c, want) == 0);
    const long A = mockhip_allocs() - a0;
    EXPECT(A > 60 && mockhip_live_allocations() == 0);
    std::vector<long> bad;
    for (long k = 0; k < A; ++k) {
        const int before = g_fail;
        got.clear();
        mockhip_fail_alloc_at(k);
        const int failed = run_pass(c, got);
        EXPECT(failed == 1);                                               // every k meets its allocation
        EXPECT(got.size() == want.size() && (got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(double)) == 0));
        EXPECT(mockhip_live_allocations() == 0);
        if (g_fail != before) { bad.push_back(k); std::fprintf(stderr, "allocation %ld of %ld: see above\n", k, A); }
    }
    std::printf("alloc_failure_driver: %ld allocations in the pass, %zu of them not survived (k =", A, bad.size());
    for (long k : bad) std::printf(" %ld", k);
    std::printf("); %d failed expectation(s); %ld allocation(s) still alive\n", g_fail, mockhip_live_allocations());
    return g_fail ? 1 : 0;
}
