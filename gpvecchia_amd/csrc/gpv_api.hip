// gpv_api.hip — the C ABI of libgpvecchia_hip.so (include/gpvecchia.h): plan
// management, host-side re-layout of the R objects into the device plan, and
// the literal .C()-style drop-ins for the reference's native entry points.
// There is no CPU compute path in here: without a GPU every entry fails loudly.
#include "../../include/gpvecchia.h"
#include "gpv_internal.h"
#include "gpv_laplace.h"
#include "gpv_generic.h"
#include "gpv_posterior_ext.h"
#include "gpv_philox.hpp"
#include "gpv_grad.h"
#include "gpv_whiten.h"
#include "gpv_unwhiten.h"
#include "gpv_loo.h"
#include "gpv_blockcv.h"
#include "gpv_krige.h"
#include "gpv_krige_groups.h"
#include "gpv_csim.h"
#include "gpv_csim_summary.h"
#include "gpv_selinv.h"
#include "gpv_grad_sgv.h"
#include "gpv_hip_raii.hpp"

#include <dlfcn.h>

#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <limits>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>

using namespace gpv;

// RCCL is bound at run time (dlopen), never at link time: the library must load in an R session on a one-GPU machine that has
// no RCCL at all.  Only five entry points are used; their C ABI (rccl.h: 128-byte ncclUniqueId by value, ncclDouble = 8,
// ncclSum = 0) has been stable since NCCL 2.0.
namespace {
struct RcclId { char internal[128]; };
struct RcclApi {
    void *handle = nullptr;
    int (*GetUniqueId)(RcclId *) = nullptr;
    int (*CommInitRank)(void **, int, RcclId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int *) = nullptr;
    int version = 0;                               // ncclGetVersion's code (2.x.y: >= 2000); 0 = not bound
};
thread_local char g_rccl_text[200] = "";
const RcclApi *rccl_api()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        // a process that already holds RCCL (PyTorch loads its own copy) is given THAT copy: dlopen matches the soname
        const char *names[] = {getenv("GPV_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *nm : names) {
            if (!nm || !*nm) continue;
            if ((api.handle = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
        }
        if (!api.handle) return;
        api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.handle, "ncclGetUniqueId");
        api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.handle, "ncclCommInitRank");
        api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.handle, "ncclCommDestroy");
        api.AllReduce = (decltype(api.AllReduce))dlsym(api.handle, "ncclAllReduce");
        api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.handle, "ncclGetErrorString");
        api.GetVersion = (decltype(api.GetVersion))dlsym(api.handle, "ncclGetVersion");
        // the hand-declared prototypes above are those of NCCL >= 2.0 (ncclUniqueId by value, ncclDouble = 8, ncclSum = 0):
        // refuse anything that cannot say it is that; gpv_comm_create then PROVES the ABI with one tiny all-reduce
        int v = 0;
        if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce || !api.GetVersion ||
            api.GetVersion(&v) != 0 || v < 2000) { dlclose(api.handle); api = RcclApi{}; return; }
        api.version = v;
    });
    return api.handle ? &api : nullptr;
}
inline int note_rccl(int r, const char *what)
{
    const RcclApi *A = rccl_api();
    g_hip_code = r;
    std::snprintf(g_hip_text, sizeof(g_hip_text), "RCCL: %s [%s]", (A && A->GetErrorString) ? A->GetErrorString(r) : "?", what);
    return GPV_ERR_HIP;
}
}  // namespace

struct gpv_comm {
    void *comm = nullptr;
    int device = 0, rank = 0, world = 1;
};

namespace {

struct CovSetup {
    int cov;
    double sig0, sA, cA, sB, cB;
    // "matern_scaledim": the kernels run the isotropic family at range 1 on a copy of the coordinates multiplied by inv[t] =
    // 1 / range_t (launch_scale_locs); nscale = the dimension, 0 for every other family.  inv_min / inv_max: the smallest and
    // largest of them (1 and 1 otherwise), by which the plan's distance bounds are stretched
    int nscale = 0;
    double inv[kMaxDimGeneric] = {0, 0, 0, 0, 0, 0, 0, 0};
    double inv_min = 1.0, inv_max = 1.0;
};

// the constants of the Matern branches at (sigma^2, range, nu): src/Matern.cpp:24
static int matern_setup(double sigma2, double range, double nu, CovSetup &c)
{
    c.sig0 = sigma2;
    c.sA = sigma2;
    if (nu == 0.5) {                   // branch chosen by exact == like the reference
        c.cov = COV_MATERN05;
        c.cA = 1.0 / range;
    } else if (nu == 1.5) {
        c.cov = COV_MATERN15;
        c.cA = std::sqrt(3.0) / range;
    } else if (nu == 2.5) {
        c.cov = COV_MATERN25;
        c.cA = std::sqrt(5.0) / range;
    } else if (nu > 0.0 && nu <= 60.0 && std::isfinite(nu)) {
        // general smoothness: Bessel branch, src/Matern.cpp:72-84.  NOTE the reference applies no sqrt(2 nu)
        // scaling there, so the covariance is discontinuous in nu at 0.5, 1.5, 2.5 (reproduced, not fixed).
        c.cov = COV_MATERN_GEN;
        c.sA = sigma2 / (std::pow(2.0, nu - 1.0) * std::tgamma(nu));   // normcon, :73
        c.cA = 1.0 / range;
        c.sB = nu;
    } else {
        return GPV_ERR_UNSUPPORTED_NU;
    }
    return GPV_OK;
}

// covType / covparms -> kernel constants.  matern: covparms = (sigma^2, range, nu)
// (src/Matern.cpp:24), esqe: (sigma1^2, r1, sigma2^2, r2) (src/Esqe.cpp:17), matern_scaledim: (sigma^2, range_1 .. range_dim,
// nu), which needs the dimension of the locations (`dim`; the other two ignore it).  No device is touched.
int cov_setup(const char *covType, const double *cp, int ncov, int dim, CovSetup &c)
{
    if (covType == nullptr || cp == nullptr) return GPV_ERR_BAD_ARG;
    c = CovSetup{};                                                   // (zeros; nscale = 0, inv_min = inv_max = 1)
    if (std::strcmp(covType, "matern") == 0) {
        if (ncov < 3) return GPV_ERR_BAD_ARG;
        const int rc = matern_setup(cp[0], cp[1], cp[2], c);
        if (rc != GPV_OK) return rc;
        // a NaN variance or range makes every covariance NaN in the reference, every block fails and the rows stay zero
        // (src/U_NZentries.cpp:64-66).  The kernels clamp the exponent's argument with v_min_f64, which drops a NaN, so the
        // NaN is planted where nothing can drop it: on the diagonal of every block.
        if (!(cp[0] == cp[0]) || !(cp[1] == cp[1])) c.sig0 = NAN;
        return GPV_OK;
    }
    if (std::strcmp(covType, "matern_scaledim") == 0) {
        // the Matern above at range 1 and distance sqrt(sum_t ((x_t - x'_t) / range_t)^2); the inverse ranges are parameters of
        // the kernel that writes the scaled copy, hence at most kMaxDimGeneric of them
        if (dim < 1 || dim > kMaxDimGeneric || ncov != dim + 2) return GPV_ERR_BAD_ARG;
        bool nan = !(cp[0] == cp[0]);
        for (int t = 0; t < dim; ++t) {
            const double r = cp[1 + t];
            if (r == r && (!(r > 0.0) || std::isinf(r))) return GPV_ERR_BAD_ARG;
            nan = nan || !(r == r);
        }
        const int rc = matern_setup(cp[0], 1.0, cp[dim + 1], c);
        if (rc != GPV_OK) return rc;
        c.nscale = dim;
        c.inv_min = INFINITY; c.inv_max = 0.0;
        for (int t = 0; t < dim; ++t) {
            c.inv[t] = 1.0 / cp[1 + t];
            if (c.inv[t] < c.inv_min) c.inv_min = c.inv[t];
            if (c.inv[t] > c.inv_max) c.inv_max = c.inv[t];
        }
        if (nan) { c.sig0 = NAN; c.inv_min = c.inv_max = 1.0; }           // as for matern: the diagonal of every block
        return GPV_OK;
    }
    if (std::strcmp(covType, "esqe") == 0) {
        if (ncov < 4) return GPV_ERR_BAD_ARG;
        c.cov = COV_ESQE;
        c.sig0 = cp[0] + cp[2];
        c.sA = cp[0];
        c.cA = 1.0 / cp[1];
        c.sB = cp[2];
        c.cB = 1.0 / (cp[3] * cp[3]);
        if (!(cp[1] == cp[1]) || !(cp[3] == cp[3])) c.sig0 = NAN;     // as above (sigma1^2 / sigma2^2 NaN: sig0 is NaN already)
        return GPV_OK;
    }
    return GPV_ERR_COVTYPE;
}

template <class F>
void parallel_for(int64_t n, F f, int max_threads = 32)
{
    unsigned hw = std::thread::hardware_concurrency();
    int64_t nt = hw ? hw : 4;
    if (nt > max_threads) nt = max_threads;
    if (n < 65536) nt = 1;
    if (nt <= 1) {
        f(0, n);
        return;
    }
    std::vector<std::thread> th;
    const int64_t chunk = (n + nt - 1) / nt;
    for (int64_t t = 0; t < nt; ++t) {
        const int64_t b = t * chunk, e = (b + chunk < n) ? b + chunk : n;
        if (b >= e) break;
        th.emplace_back([=] { f(b, e); });
    }
    for (auto &t : th) t.join();
}

inline bool is_missing(int v) { return v == 0 || v == INT_MIN; }

// order[r] = index of the r-th smallest key, ties by ascending index (what std::stable_sort over an iota gives):
// LSD radix sort of (key, index) pairs, 11 bits per pass, histograms and scatters split over threads.
// 1e6 keys: ~15 ms instead of ~105 ms for the comparison sort.
void sort_order_by_key(const uint64_t *key, int64_t n, int32_t *order)
{
    if (n <= 0) return;
    uint64_t kmax = 0;
    for (int64_t i = 0; i < n; ++i) kmax = key[i] > kmax ? key[i] : kmax;
    int bits = 0;
    while (bits < 64 && (kmax >> bits) != 0) ++bits;
    constexpr int RB = 11, NB = 1 << RB;
    struct KV { uint64_t k; int32_t i; };
    std::vector<KV> a((size_t)n), b((size_t)n);
    for (int64_t i = 0; i < n; ++i) a[(size_t)i] = KV{key[i], (int32_t)i};
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)(hw ? (hw > 16 ? 16 : hw) : 4);
    if (n < 262144) nt = 1;
    const int64_t chunk = (n + nt - 1) / nt;
    std::vector<int64_t> hist((size_t)nt * NB);
    KV *src = a.data(), *dst = b.data();
    for (int shift = 0; shift < bits; shift += RB) {
        std::fill(hist.begin(), hist.end(), 0);
        auto run = [&](auto fn) {
            if (nt == 1) { fn(0); return; }
            std::vector<std::thread> th;
            for (int t = 0; t < nt; ++t) th.emplace_back([=] { fn(t); });
            for (auto &x : th) x.join();
        };
        run([&](int t) {
            int64_t *h = &hist[(size_t)t * NB];
            const int64_t lo = t * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
            for (int64_t i = lo; i < hi; ++i) ++h[(src[i].k >> shift) & (NB - 1)];
        });
        int64_t run_sum = 0;                               // bucket-major, thread-minor: keeps the pass stable
        for (int d = 0; d < NB; ++d)
            for (int t = 0; t < nt; ++t) {
                const int64_t c = hist[(size_t)t * NB + d];
                hist[(size_t)t * NB + d] = run_sum;
                run_sum += c;
            }
        run([&](int t) {
            int64_t *h = &hist[(size_t)t * NB];
            const int64_t lo = t * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
            for (int64_t i = lo; i < hi; ++i) dst[h[(src[i].k >> shift) & (NB - 1)]++] = src[i];
        });
        std::swap(src, dst);
    }
    for (int64_t i = 0; i < n; ++i) order[i] = src[i].i;
}

// 128-bit content hash of a host buffer.  The buffer is cut into a FIXED number of chunks (the result does not depend on
// how many threads share them), every chunk runs eight independent multiply-rotate lanes over 64-byte blocks (every step
// is a bijection of its lane for a given word, so a change of any single word changes the result), the chunks are
// combined in chunk order.  Not cryptographic: it keys the plan cache of the literal drop-in, where a false hit needs a
// collision between two different index arrays of the same shape.
struct Hash128 {
    uint64_t a = 0, b = 0;
    bool operator==(const Hash128 &o) const { return a == o.a && b == o.b; }
};
inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
Hash128 hash_bytes(const void *ptr, size_t bytes, uint64_t seed, unsigned max_threads = 32)
{
    const unsigned char *p = static_cast<const unsigned char *>(ptr);
    const size_t words = bytes / 8;
    constexpr uint64_t K1 = 0xC2B2AE3D27D4EB4Full, K2 = 0x9E3779B97F4A7C15ull, K3 = 0x165667B19E3779F9ull, K4 = 0xD6E8FEB86659FD93ull;
    const size_t nchunk = (bytes < ((size_t)1 << 22)) ? 1 : 64;
    const size_t chunk = ((words + nchunk - 1) / nchunk + 7) / 8 * 8;    // words per chunk, whole 64-byte blocks
    std::vector<Hash128> part(nchunk);
    auto work = [&](size_t t) {
        const size_t lo = t * chunk < words ? t * chunk : words, hi = (lo + chunk < words) ? lo + chunk : words;
        uint64_t acc[8];
        for (int l = 0; l < 8; ++l) acc[l] = (seed + (uint64_t)l) * K3 ^ rotl64(K4, 7 * l + 1);
        size_t i = lo;
        for (; i + 8 <= hi; i += 8) {
            uint64_t v[8];
            std::memcpy(v, p + 8 * i, 64);
            for (int l = 0; l < 8; ++l) acc[l] = rotl64(acc[l] + v[l] * K1, 31) * K2;
        }
        for (int l = 0; i < hi; ++i, ++l) {
            uint64_t v0;
            std::memcpy(&v0, p + 8 * i, 8);
            acc[l] = rotl64(acc[l] + v0 * K1, 31) * K2;
        }
        uint64_t a = seed ^ K4, b = ~seed * K3;
        for (int l = 0; l < 8; ++l) {
            a = rotl64(a ^ acc[l], 27) * K2 + (uint64_t)l;
            b = rotl64(b + (acc[l] ^ rotl64(acc[l], 32)), 41) * K1 ^ (uint64_t)l;
        }
        part[t].a = a;
        part[t].b = b;
    };
    unsigned hw = std::thread::hardware_concurrency();
    size_t nt = hw ? (hw > max_threads ? max_threads : hw) : 4;
    if (nt > nchunk) nt = nchunk;
    if (nt <= 1) {
        for (size_t t = 0; t < nchunk; ++t) work(t);
    } else {
        std::atomic<size_t> next{0};
        auto loop = [&]() {
            for (size_t t = next.fetch_add(1); t < nchunk; t = next.fetch_add(1)) work(t);
        };
        std::vector<std::thread> th;
        for (size_t t = 0; t + 1 < nt; ++t) th.emplace_back(loop);
        loop();
        for (auto &x : th) x.join();
    }
    Hash128 r;
    r.a = seed ^ (uint64_t)bytes;
    r.b = ~seed + (uint64_t)bytes;
    for (size_t t = 0; t < nchunk; ++t) {
        r.a = rotl64(r.a ^ part[t].a, 25) * K2 + t;
        r.b = rotl64(r.b + part[t].b, 37) * K1 ^ t;
    }
    uint64_t tail = 0;                                        // the last bytes % 8 bytes
    std::memcpy(&tail, p + 8 * words, bytes - 8 * words);
    r.a ^= tail * K4;
    r.b += rotl64(tail, 13);
    return r;
}

}  // namespace

struct gpv_plan {
    // Every device resource is a member that releases itself (gpv_hip_raii.hpp); gpv_plan_destroy holds no list of them.
    // Members are destroyed in REVERSE order of declaration and the release order is graphs, buffers, events, stream: so the
    // stream comes first here, then the events, the buffers follow, and the graphs stand at the very end.
    Stream stream;
    Event ev0, ev1;
    Event stage_ev[2], mt_ev[2];                     // guards of h_stage / of the general-nu table copies (h_mt2, d_mt2)
    int device = 0, cus = 0;
    int64_t Nlocs = 0, row_begin = 0, row_end = 0, rows = 0;
    int dim = 0, p = 0, P = 0, locs_ld = 0, grid = 1;
    // d_locs: dim <= 3: packed records [Nlocs][4] = {c0,c1,c2,data} in the plan's INTERNAL (Morton) order;
    //         dim  > 3: coordinates [Nlocs][dim] in internal order, data in d_z
    // d_nuggets: internal order (gathered by the kernel); d_nug_user: caller's ordered layout (Zentries)
    // d_locs_sc: matern_scaledim's copy of d_locs with the coordinates divided by the ranges, rewritten by every evaluation of
    //         that family (eval_scaled_locs) and by its gradient-type calls; allocated on first use
    DevBuf<double> d_locs_sc;
    DevBuf<double> d_locs, d_nuggets, d_nug_user, d_z, d_L, d_block, d_sums, d_Z, d_tmp, d_covvals, d_stage;
    DevBuf<int32_t> d_nn, d_newpos, d_rowid;
    DevBuf<unsigned> d_ticket;                       // arrival counter of the set kernel's workgroups (gpv_reduce_tail.hpp)
    bool ticket_dirty = false;                       // an evaluation failed after its launch may have started: reset before the next
    // pinned host mirror of the totals: when the caller names no device mirror, the kernels write the totals straight into
    // host memory and gpv_plan_get_sums needs no copy command, only the stream's completion
    PinnedBuf<char> h_stage[2];                      // pinned staging of gpv_plan_get_Lentries (32 MB each, on first use)
    PinnedBuf<double> h_sums;
    double *h_sums_dev = nullptr;                    // the device's address of h_sums
    bool sums_on_host = false;
    // hand-off of the totals by memory: h_sums holds 8 totals and, behind them, 8 sequence numbers the producing kernel
    // stores after the totals (gpv_reduce_tail.hpp, publish_seq); gpv_plan_get_sums spins on them
    unsigned long long seq = 0;                      // sequence number of the latest evaluation
    bool sums_by_seq = false;                        // the latest evaluation publishes its totals that way
    gpv_comm *comm = nullptr;                        // attached communicator: every evaluation all-reduces its 8 sums (gpv_plan_set_comm)
    // posterior ("U2V") pass, built on request (gpv_plan_build_posterior)
    bool have_post = false;
    DevBuf<int32_t> d_colptr, d_crow, d_ccol;
    DevBuf<int4> d_colrec, d_rowrec;
    DevBuf<int4> d_rr0;                              // first-round row-list records in schedule order (PostArgs::rr0)
    std::vector<int64_t> lev_rr0;                    // [level] where its records start in d_rr0
    int64_t top_rr0 = 0;                             // the dense top block's
    DevBuf<uint8_t> d_tp;
    DevBuf<double2> d_C;
    DevBuf<int32_t> d_cboff, d_cdel;                 // block offsets in d_C (Morton order of the locations), and cboff - colptr
    int64_t post_nnz = 0;
    bool post_fused = false;                         // the set kernel writes the compact blocks itself (block positions in d_cond)
    int post_ld = 0;                                 // bound of the entries per column of the posterior structure (>= P; more with fill)
    DevBuf<uint8_t> d_cslot;
    DevBuf<double> d_avec_base;                      // allocation of d_avec: 64 bytes of header, then the n values
    double *d_avec = nullptr;                        // = d_avec_base + 8
    DevBuf<double> d_tvec, d_rdiag, d_post_part, d_zuser;
    DevBuf<uint8_t> d_obs;                           // [Nlocs] ordered layout: 1 = the location carries an observation; nullptr: all do
    DevBuf<double> d_nug_masked;                     // [Nlocs] the evaluation's nuggets with +Inf where d_obs == 0 (PostArgs::nuggets)
    std::vector<int32_t> levptr, levptr2;
    std::vector<int> lev_lpc;                        // lanes per column of every level's kernel (16 / 32 / 64), from its row lists
    DevBuf<double> d_nug_post;                       // ONE double: the constant nugget of the evaluation (PostArgs::nug_cell)
    // general-nu Matern: range of pair distances of the plan (parameter independent) and the per-evaluation table
    double coord_maxabs = 0.0;                       // largest finite |coordinate| (guards the kernel's pre-scaled coordinates)
    double dist_min = 0.0, dist_max = 0.0;
    // distances of ALL pairs inside a sample of the conditioning sets, by quarter octave (index = floor(4 log2 d) + 4400):
    // where the set kernel's LDS window of the general-nu table goes
    std::vector<int64_t> dist_hist;
    PinnedBuf<double> h_mt2[2];                      // pinned staging / device copies, used alternately
    DevBuf<double> d_mt2[2];
    int mt_slot = 0, mt_pending = -1;
    DevBuf<int32_t> d_order2, d_levptr2;
    DevBuf<int4> d_meanrec;                          // mean sweep: one record per column in schedule order
    DevBuf<double> d_toppart;                        // [top_K][66] partial sums of the top block's columns
    DevBuf<int2> d_topinfo;                          // [top_K] {column, offset of its block in C}
    DevBuf<uint8_t> d_toprows;                       // [top_K][64] index inside the block of each entry's row
    int top_K = 0;                                   // columns 0 .. top_K-1 are kept out of the schedule (gpv_posterior_ext.h)
    int mean_head_levels = 0;                        // leading levels of the mean sweep run by one workgroup
    DevBuf<double> d_u, d_mu;
    bool have_mean = false;
    // linear combinations (gpv_plan_lincomb): everything is allocated on first use
    bool have_factor = false;                        // C holds the factor of an evaluation with a posterior pass
    int64_t factor_stamp = 0;                        // counts those evaluations
    DevBuf<int2> d_lc_rec;                           // LincombArgs::lrec, rebuilt after gpv_plan_build_posterior
    bool lc_ready = false;
    DevBuf<double> d_lc_X, d_lc_part, d_lc_vars, d_lc_gpart, d_lc_gram;
    DevBuf<double> d_st_E;                           // gpv_plan_solve_t: one batch of dense columns, [kLincombNB][Nlocs]
    // gpv_plan_selinv (gpv_selinv.hip), built and allocated on first use after gpv_plan_build_posterior: the column records in
    // the order of the pass (top block, then the ascending schedule), the pair records by entry of crow, Sigma on the pattern
    // of C, its diagonal by column and as the caller gets it; the tile of every level's kernel; the dropped terms of the pattern
    DevBuf<int4> d_sel_rec;
    DevBuf<int2> d_sel_pair;
    DevBuf<double> d_sel_S, d_sel_vars, d_sel_out;
    std::vector<int> sel_lev_tile;
    int64_t sel_dropped = 0;
    bool sel_ready = false;
    // gpv_plan_loglik_grad_sgv (gpv_grad_sgv.hip), built and allocated on first use after gpv_plan_build_posterior: by stored
    // set, the position of every entry in the set's posterior column and the column's record (SgvGradArgs::cpos, setrec);
    // per-workgroup partials, their totals, per-row terms
    DevBuf<uint8_t> d_sgv_cpos;
    DevBuf<int4> d_sgv_rec;
    DevBuf<double> d_sgv_part, d_sgv_tot, d_sgv_rows;
    int sgv_grid = 0;
    bool sgv_ready = false;
    bool post_filled = false;                        // the structure is a filled one (gpv_plan_build_posterior_fill)
    // gpv_plan_draws_summary: mu, S1, S2, mean, var [Nlocs] each, exceed [8][Nlocs], the accumulation's block partials; counts
    // [8][Nlocs]; mask [Nlocs]; draw_max, draw_mean [ds_draw_cap] each.  Allocated on first use.
    DevBuf<double> d_ds, d_ds_draw;
    DevBuf<uint32_t> d_ds_cnt;
    DevBuf<uint8_t> d_ds_mask;
    int64_t ds_draw_cap = 0;
    double nug_scalar = 0.0;
    bool nug_is_scalar = true;
    // Facts the lean likelihood-only kernel relies on (gpv_sets_kernel.hpp, k_lean), fixed when the plan is built ...
    bool coords_finite = false;    // no NaN / Inf among the location coordinates
    double bbox_diam = INFINITY;   // diagonal of the locations' bounding box: no pair of the plan is farther apart
    bool idx32 = false;            // rows * P < 2^31: 32-bit products address nn / cond
    DevBuf<uint8_t> d_task_pad;    // [tasks, padded to a multiple of 4] SetArgs::task_pad (instantiations with a lean kernel)
    // ... or when the nugget vector is uploaded (a scalar nugget is tested per call)
    bool nug_vec_ok = false;       // d_nuggets holds finite values <= 2^990 only
    int last_set_kernel = 0;       // kSetKernel* of the latest evaluation (gpv_plan_last_set_kernel)
    DevBuf<uint8_t> d_cond;
    std::vector<int32_t> h_newpos;  // host copy of d_newpos (shared with the sibling plans of a gpv_mplan)
    bool generic = false;          // row length > 64 or dimension > 8: workgroup-per-set kernel (gpv_sets_generic.hip)
    bool latent_nb = false;        // some NEIGHBOUR (not a row's own point) is conditioned on as latent y: not a cond.yz='z' plan
    // gpv_plan_loglik_grad (gpv_grad.hip), allocated on first use: per-workgroup partials, their totals, per-row terms
    DevBuf<double> d_gr_part, d_gr_tot, d_gr_rows;
    int gr_grid = 0;
    // the same for gpv_plan_loglik_fisher (the kSetsFisher mode of gpv_grad.hip)
    DevBuf<double> d_fi_part, d_fi_tot, d_fi_rows;
    int fi_grid = 0;
    // gpv_plan_loglik_grad_nu / _fisher_nu at a general smoothness: the call's tables (gpv_bessel.hpp, MaternDTab)
    DevBuf<double> d_gmt;
    // gpv_plan_set_replicates / gpv_plan_loglik_rep (gpv_rep_kernel.hpp): the replicates by internal position [Nlocs][rep_RP],
    // zeros behind column rep_R; rep_R = 0: none set.  The calls are blocking and their partials, totals and rows have the
    // layout of gpv_plan_loglik_fisher's, so they use d_fi_part / d_fi_tot / d_fi_rows.
    DevBuf<double> d_rep_Z;
    int rep_R = 0, rep_RP = 0;
    // gpv_plan_whiten (gpv_whiten.hip), allocated on first use and grown with the padded column count: the caller's columns as
    // they arrive / E on its way back [cp][Nlocs], the columns by internal position [Nlocs][cp], E [Nlocs][cp], the partials of
    // both passes and the totals
    DevBuf<double> d_wh_in, d_wh_B, d_wh_E, d_wh_wpart, d_wh_gpart, d_wh_tot;
    int wh_cp_cap = 0, wh_cp_last = 0, wh_wgrid = 0, wh_ggrid = 0;
    // gpv_plan_unwhiten / gpv_plan_simulate (gpv_unwhiten.hip).  The level schedule is built from d_nn / d_rowid at first use
    // (unwhiten_schedule) and never changes: the stored sets level by level (d_uw_order), where the levels start in that list
    // (uw_levptr, d_uw_levptr) and the launches of one sweep.  The column buffers are allocated on first use and grown with the
    // padded column count: the caller's columns as they arrive / B on its way back [cp][Nlocs], E by ordered row [Nlocs][cp],
    // B by internal position [Nlocs][cp]; d_uw_nfail: the sweep's counter of failed rows.
    struct UwLaunch { int lev0, lev1; bool narrow; };    // levels lev0 .. lev1 - 1: one run of narrow levels, or one wide level
    bool uw_sched = false, uw_holes = false;
    std::vector<int32_t> uw_levptr;
    std::vector<UwLaunch> uw_launches;
    DevBuf<int32_t> d_uw_order, d_uw_levptr;
    DevBuf<double> d_uw_in, d_uw_E, d_uw_B;
    DevBuf<unsigned> d_uw_nfail;
    int uw_cp_cap = 0, uw_cp_last = 0;
    int64_t uw_graph_eval[5] = {0, 0, 0, 0, 0};      // the evaluation whose addresses and nugget uw_graph[log2 cp] holds
    // gpv_plan_whiten_t / gpv_plan_precision / gpv_plan_loo (gpv_loo.hip).  The transposed index is built from d_nn / d_rowid at
    // first use (loo_index) and never changes: column starts, owners, flat offsets (LooArgs).  d_loo_g belongs to evaluation
    // loo_g_eval (the scale pre-pass runs once per evaluation; loo_nfail is its count of failed rows).  The column buffers are
    // allocated on first use and grown with the padded column count: the caller's columns as they arrive and the result on its
    // way back [cp][Nlocs], B and R by internal position [Nlocs][cp], E by ordered row [Nlocs][cp]; q by internal position and
    // in the ordered numbering, the variances, the score partials [16][loo_sgrid][6] and the scores [16][6].
    bool loo_have_index = false;
    int64_t loo_nnz = 0, loo_maxcol = 0, loo_empty = 0;
    DevBuf<int32_t> d_loo_colptr, d_loo_owner, d_loo_col;
    DevBuf<double> d_loo_g, d_loo_in, d_loo_out, d_loo_B, d_loo_E, d_loo_R, d_loo_q, d_loo_qord, d_loo_var, d_loo_part, d_loo_scores;
    DevBuf<unsigned> d_loo_nfail;
    int loo_cp_cap = 0, loo_grid = 0, loo_sgrid = 0;
    int loo_last_mode = -1, loo_last_ncols = 0;      // what gpv_plan_debug_loo_ms repeats
    int64_t loo_g_eval = 0;
    unsigned loo_nfail = 0;
    // gpv_plan_set_blocks / gpv_plan_block_cv (gpv_blockcv.hip).  The block index (BlockIndex) stays until the labels are
    // replaced.  The calls use the transposed index and d_loo_g above and column buffers of their OWN, so what gpv_plan_loo left
    // on the device stays: the caller's columns and the means on their way back [cp][Nlocs], B, R, delta and y^2 by internal
    // position [Nlocs][cp], E by ordered row, q, the variances and the -log pivots by internal position and ordered, the score
    // partials [16][bcv_sgrid][8] and the scores [16][8]; d_bcv_nbad: the call's counter of bad blocks.
    bool bcv_have = false;
    int64_t bcv_nblocks = 0, bcv_nheld = 0, bcv_nrefs = 0;
    int bcv_maxsize = 0;
    DevBuf<int32_t> d_bcv_memptr, d_bcv_members, d_bcv_setptr, d_bcv_sets, d_bcv_blkloc;
    DevBuf<double> d_bcv_in, d_bcv_out, d_bcv_B, d_bcv_E, d_bcv_R, d_bcv_q, d_bcv_D, d_bcv_Y2, d_bcv_y2ord, d_bcv_var, d_bcv_nlp,
        d_bcv_varord, d_bcv_nlpord, d_bcv_part, d_bcv_scores;
    DevBuf<unsigned> d_bcv_nbad;
    int bcv_cp_cap = 0, bcv_grid = 0, bcv_sgrid = 0, bcv_last_ncols = 0;
    // gpv_plan_krige (gpv_krige.hip): device time of the latest call's searches and passes, summed over its chunks
    // (gpv_plan_debug_krige_ms).  Its buffers live for the call.
    double kr_search_ms = 0.0, kr_pass_ms = 0.0;
    // gpv_plan_cond_sim (gpv_csim.hip): the rows per launch of its factor pass (0: the default; gpv_plan_debug_csim_chunk) and
    // the latest call's times (gpv_plan_debug_csim_ms): the search by the host's clock, then device time of the factor pass,
    // of all sweeps and of the last sweep.  Its buffers live for the call.
    int64_t cs_chunk = 0;
    double cs_search_ms = 0.0, cs_factor_ms = 0.0, cs_sweep_ms = 0.0, cs_last_sweep_ms = 0.0;
    // gpv_plan_cond_sim_summary (gpv_csim_summary.hip): device time of the latest call's folds, all batches and the last one
    // (gpv_plan_debug_csim_summary_ms); the other times of such a call are those above
    double cs_fold_ms = 0.0, cs_last_fold_ms = 0.0, cs_copy_ms = 0.0, cs_last_copy_ms = 0.0;
    // d_L and the nuggets on the device (d_nuggets / nug_scalar) belong to evaluation L_of_eval of the plan (evaluations are
    // counted from 1; 0: to none).  Set at the end of an evaluation that materialised U, cleared before anything of the two is
    // rewritten: an evaluation that starts, a Vecchia-Laplace step that writes its pseudo-nuggets, a rebuilt posterior structure.
    int64_t eval_count = 0, L_of_eval = 0;
    // Vecchia-Laplace state (gpv_plan_vl_begin): data z, prior mean, two latent-mean buffers (current / next), flags + max
    DevBuf<double> d_vl_z, d_vl_pm, d_vl_y[2], d_vl_out;
    DevBuf<double> d_vl_y0;                          // the start value, kept so that a restart needs no upload
    DevBuf<double> d_vl_part;                        // scratch of the missing-data and likelihood-term reductions
    DevBuf<int32_t> d_user_ord;                      // ord.z (1-based): caller's layout <-> ordered layout on the device
    DevBuf<int> d_vl_flags;
    int vl_model = -1, vl_cur = 0;
    bool vl_missing = false;                         // some z is NaN: the substitutes of removeNAs are computed every step
    PinnedBuf<double> h_vl;                          // pinned: {max|dy|, flags (as a double)} of the step, written by the kernels
    double *h_vl_dev = nullptr;                      // the device's address of h_vl
    double vl_alpha = 2.0, vl_sigma = 0.0, vl_beta = 0.5;
    bool has_z = false, evaluated = false, have_U = false;
    bool timing = true, timed = false;               // hipEvent pair around the set kernel (gpv_plan_set_kernel_timing)
    hipStream_t last_stream = nullptr;               // not owned: the plan's stream or the caller's
    // the posterior pass as a captured HIP graph (one per {denominator, denominator + mean}): ~140 (280) launches of a few
    // microseconds each, which the host cannot enqueue as fast as the device retires them in the narrow tail levels
    struct PostGraph { GraphExec exec; double *sums_out = nullptr; };
    PostGraph pgraph[8];                             // index = want_mean + 2 * (nuggets are a vector) + 4 * (mean from B: 'zy')
    GraphExec lc_graph;                              // gpv_plan_lincomb's sweep (levels, top block, column sums)
    GraphExec st_graph;                              // the transposed sweep (top block, levels)
    GraphExec sel_graph;                             // the selected inverse (top block, levels)
    GraphExec uw_graph[5];                           // the colouring sweep at cp = 1, 2, 4, 8, 16 (see uw_graph_eval)
    void drop_graphs()                               // they hold addresses and a schedule that are about to change
    {
        for (auto &g : pgraph) g.exec.reset();
        lc_graph.reset();
        st_graph.reset();
        sel_graph.reset();
        for (auto &g : uw_graph) g.reset();
    }
};

// ---- what the operators on a resident factor share: every entry below is made of these, none keeps a copy ------------------
// An entry's first step on the device: the plan's device, then a wait for the stream of the plan's latest evaluation (the
// plan's own or a caller's), which may still be writing what the entry reads.  enter() leaves the plan's own stream alone: what
// the entry enqueues there is ordered behind the evaluation anyway.  enter_final() waits for it as well: the factor must be
// final, since the entry reads the structure back with blocking copies or makes the plan's stream the latest one.
static int enter(gpv_plan *pl)
{
    GPV_HIP(hipSetDevice(pl->device));
    if (pl->last_stream && pl->last_stream != pl->stream) GPV_HIP(hipStreamSynchronize(pl->last_stream));
    return GPV_OK;
}
static int enter_final(gpv_plan *pl)
{
    GPV_HIP(hipSetDevice(pl->device));
    if (pl->last_stream) GPV_HIP(hipStreamSynchronize(pl->last_stream));
    return GPV_OK;
}

// How an entry leaves after a failure past its first enqueue: nothing in flight on `st` still reads the caller's arrays or the
// buffers that live for the call when they go.
static int drain_fail(hipStream_t st, int rc)
{
    (void)hipStreamSynchronize(st);
    return rc;
}

// `ncols` columns of `n` doubles between a host array of leading dimension `ld` and a device buffer that holds them back to
// back, one copy per column on `st`; a failed copy is recorded here, under its own name.  cols_fill_nan(): what a caller gets in
// place of columns that a failed row has reached.
static int cols_to_device(double *dev, const double *host, int64_t ld, int64_t n, int64_t ncols, hipStream_t st)
{
    for (int64_t j = 0; j < ncols; ++j)
        GPV_HIP(hipMemcpyAsync(dev + (size_t)j * n, host + j * ld, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    return GPV_OK;
}
static int cols_to_host(double *host, int64_t ld, const double *dev, int64_t n, int64_t ncols, hipStream_t st)
{
    for (int64_t j = 0; j < ncols; ++j)
        GPV_HIP(hipMemcpyAsync(host + j * ld, dev + (size_t)j * n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    return GPV_OK;
}
static void cols_fill_nan(double *host, int64_t ld, int64_t n, int64_t ncols)
{
    for (int64_t j = 0; j < ncols; ++j) std::fill_n(host + j * ld, (size_t)n, (double)NAN);
}

// The factor of the plan's latest evaluation as the operators' kernels see it (WhitenArgs, UnwhitenArgs, LooArgs): the U
// entries, the index arrays, and the nuggets as a vector or as one value.
template <class Args>
static void factor_view(const gpv_plan *pl, Args &a)
{
    a.L = pl->d_L; a.nn = pl->d_nn; a.rowid = pl->d_rowid;
    a.nuggets = pl->nug_is_scalar ? nullptr : pl->d_nuggets.get();
    a.nug_scalar = pl->nug_scalar;
}

// d_L and the nuggets on the device are those of the plan's latest evaluation
static bool factor_current(const gpv_plan *pl) { return !(pl->L_of_eval == 0 || pl->L_of_eval != pl->eval_count || !pl->d_L); }
// What the plan's structure must be for a level schedule or a transposed index to mean anything, evaluation or not: every row
// on this device and no neighbour conditioned on as latent.  (plan_fill uploads both index arrays of every plan.)
static int z_structure(const gpv_plan *pl)
{
    if (pl->rows != pl->Nlocs || pl->Nlocs < 1 || pl->latent_nb || !pl->d_nn || !pl->d_rowid) return GPV_ERR_STATE;
    return GPV_OK;
}
// What every operator on the resident factor asks: the latest evaluation left its factor, and this is a plain 'z' plan (no row
// shard, no unobserved location).
static int factor_state(const gpv_plan *pl)
{
    if (!factor_current(pl) || pl->comm || pl->d_obs) return GPV_ERR_STATE;
    return z_structure(pl);
}

// What every entry that sweeps with the posterior factor asks of the plan (gpv_plan_solve_t, gpv_plan_selinv, the draws): a
// structure, a factor of its own (no row shard), and columns no longer than the sweeps' tiles (no structure is built with longer).
static int posterior_factor_state(const gpv_plan *pl)
{
    if (!pl->have_post || !pl->have_factor || pl->comm) return GPV_ERR_STATE;
    if (pl->post_ld > 64 || !pl->d_meanrec) return GPV_ERR_STATE;
    return GPV_OK;
}

// The body of the gpv_plan_debug_*_ms entries, which have checked their arguments and their state: the plan's device (and,
// with wait_eval, enter()'s wait), then `reps` runs of `body` on the plan's stream, each between a pair of events and waited
// for: ms[r] = the device time of run r.  `before` is enqueued ahead of each run's first event, untimed.
static hipError_t nothing_before() { return hipSuccess; }
template <class Body, class Before = hipError_t (*)()>
static int timed_reps(gpv_plan *pl, bool wait_eval, int reps, double *ms, Body body, Before before = nothing_before)
{
    if (wait_eval) {
        if (const int rc = enter(pl)) return rc;
    } else {
        GPV_HIP(hipSetDevice(pl->device));
    }
    hipStream_t st = pl->stream;
    Event a, b;
    GPV_HIP(hipEventCreate(a.put()));
    GPV_HIP(hipEventCreate(b.put()));
    int rc = GPV_OK;
    for (int r = 0; r < reps && rc == GPV_OK; ++r) {
        float t = 0.f;
        if (GPV_HIP_FAILED(before()) || GPV_HIP_FAILED(hipEventRecord(a, st)) || GPV_HIP_FAILED(body()) ||
            GPV_HIP_FAILED(hipEventRecord(b, st)) || GPV_HIP_FAILED(hipStreamSynchronize(st)) ||
            GPV_HIP_FAILED(hipEventElapsedTime(&t, a, b)))
            rc = GPV_ERR_HIP;
        ms[r] = (double)t;
    }
    (void)hipStreamSynchronize(st);
    return rc;
}

extern "C" {

const char *gpv_status_string(int status)
{
    switch (status) {
        case GPV_OK: return "ok";
        case GPV_ERR_NO_DEVICE: return "no usable HIP device (libgpvecchia_hip has no CPU fallback)";
        case GPV_ERR_BAD_ARG: return "bad argument";
        case GPV_ERR_COVTYPE: return "covariance is not implemented (covType must be \"matern\", \"matern_scaledim\" or \"esqe\")";
        case GPV_ERR_UNSUPPORTED_NU: return "Matern smoothness must be finite, > 0 and <= 60";
        case GPV_ERR_UNSUPPORTED_M: return "m+1 exceeds 192 (or 64 for the device posterior pass)";
        case GPV_ERR_HIP: return "HIP runtime error";
        case GPV_ERR_STATE: return "call order error (no evaluation yet / no data set)";
        case GPV_ERR_INDEX: return "neighbour index out of range";
        default: return "unknown status";
    }
}

int gpv_version(void) { return 101; }

int gpv_last_hip_error(char *text, int text_len)
{
    if (text && text_len > 0) {
        std::strncpy(text, g_hip_text, (size_t)text_len - 1);
        text[text_len - 1] = 0;
    }
    return g_hip_code;
}

int gpv_device_count(int *count)
{
    if (!count) return GPV_ERR_BAD_ARG;
    int c = 0;
    if (GPV_HIP_FAILED(hipGetDeviceCount(&c))) {
        *count = 0;
        return GPV_ERR_NO_DEVICE;
    }
    *count = c;
    return c > 0 ? GPV_OK : GPV_ERR_NO_DEVICE;
}

int gpv_max_p(void) { return generic_max_P(); }

int gpv_plan_destroy(gpv_plan *pl)
{
    if (!pl) return GPV_OK;
    (void)hipSetDevice(pl->device);
    if (pl->stream) (void)hipStreamSynchronize(pl->stream);
    delete pl;                        // every resource goes with its member (an attached communicator is its creator's)
    return GPV_OK;
}

// GPV_TIMING=1: host-side phase times of plan construction and of the literal drop-in on stderr (developer aid)
struct PhaseTimer {
    bool on;
    std::chrono::steady_clock::time_point t0;
    PhaseTimer() : on(getenv("GPV_TIMING") != nullptr), t0(std::chrono::steady_clock::now()) {}
    void lap(const char *what)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[gpv timing] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// shared_newpos: the internal (Morton) position of every location as computed by an earlier plan of the same locations
// (gpv_mplan_create builds one plan per device; the order depends on the locations only), or nullptr
static int plan_create_impl(gpv_plan **out, int device, int64_t Nlocs, int dim, int ncolNN, const double *locs,
                            const int *revNN, const int *revCond, int64_t row_begin, int64_t row_end,
                            const int32_t *shared_newpos);

int gpv_plan_create(gpv_plan **out, int device, int64_t Nlocs, int dim, int ncolNN, const double *locs,
                    const int *revNN, const int *revCond, int64_t row_begin, int64_t row_end)
{
    return plan_create_impl(out, device, Nlocs, dim, ncolNN, locs, revNN, revCond, row_begin, row_end, nullptr);
}

static int plan_fill(gpv_plan *pl, int device, int64_t Nlocs, int dim, int ncolNN, const double *locs, const int *revNN,
                     const int *revCond, int64_t row_begin, int64_t row_end, const int32_t *shared_newpos);

static int plan_create_impl(gpv_plan **out, int device, int64_t Nlocs, int dim, int ncolNN, const double *locs,
                            const int *revNN, const int *revCond, int64_t row_begin, int64_t row_end,
                            const int32_t *shared_newpos)
{
    if (!out) return GPV_ERR_BAD_ARG;
    *out = nullptr;
    if (Nlocs <= 0 || Nlocs >= ((int64_t)1 << 31) || dim < 1 || dim > 4096 || ncolNN < 1 || !revNN)
        return GPV_ERR_BAD_ARG;
    if (row_begin < 0 || row_end > Nlocs || row_begin > row_end) return GPV_ERR_BAD_ARG;
    int ndev = 0;
    if (gpv_device_count(&ndev) != GPV_OK) return GPV_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return GPV_ERR_NO_DEVICE;
    gpv_plan *pl = new gpv_plan();
    const int rc = plan_fill(pl, device, Nlocs, dim, ncolNN, locs, revNN, revCond, row_begin, row_end, shared_newpos);
    if (rc != GPV_OK) {                                   // the one failure path: whatever the plan holds so far goes with it
        gpv_plan_destroy(pl);
        return rc;
    }
    *out = pl;
    return GPV_OK;
}

static int plan_fill(gpv_plan *pl, int device, int64_t Nlocs, int dim, int ncolNN, const double *locs, const int *revNN,
                     const int *revCond, int64_t row_begin, int64_t row_end, const int32_t *shared_newpos)
{
    PhaseTimer tm;
    int P = pick_P(ncolNN);
    bool generic = false;
    if (P == 0 || dim > kMaxDimGeneric) {          // shapes without an unrolled instantiation: the slow generic kernel
        if (ncolNN > generic_max_P()) return GPV_ERR_UNSUPPORTED_M;
        P = ncolNN;
        generic = true;
    }
    if (GPV_HIP_FAILED(hipSetDevice(device))) return GPV_ERR_NO_DEVICE;
    pl->device = device;
    pl->Nlocs = Nlocs;
    pl->row_begin = row_begin;
    pl->row_end = row_end;
    pl->rows = row_end - row_begin;
    pl->dim = dim;
    pl->p = ncolNN;
    pl->P = P;
    pl->generic = generic;
    pl->locs_ld = (dim <= 3) ? 4 : dim;
    hipDeviceProp_t prop;
    if (GPV_HIP_FAILED(hipGetDeviceProperties(&prop, device))) return GPV_ERR_NO_DEVICE;
    pl->cus = prop.multiProcessorCount;
    pl->grid = 1;

    // ---- internal location order: Morton (Z-curve) sort of the coordinates.  Invisible at the ABI: only the
    // device copies of locations / data / nuggets are permuted and the neighbour indices remapped.  The m
    // neighbours of a point are spatially close, so their 32-byte records then share cache lines instead of
    // costing one fabric request each (profiles/: FETCH_SIZE per launch).
    std::vector<int32_t> newpos((size_t)Nlocs);
    if (shared_newpos) {
        std::memcpy(newpos.data(), shared_newpos, sizeof(int32_t) * (size_t)Nlocs);
    } else {
        std::vector<uint64_t> key((size_t)Nlocs, 0);
        if (locs) {
            const int kd = dim < 3 ? dim : 3;
            double lo[3] = {0, 0, 0}, sc[3] = {0, 0, 0};
            for (int t = 0; t < kd; ++t) {
                double mn = INFINITY, mx = -INFINITY;
                for (int64_t i = 0; i < Nlocs; ++i) {
                    const double v = locs[i + (int64_t)t * Nlocs];
                    if (v == v) { mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
                }
                lo[t] = mn;
                sc[t] = (mx > mn) ? 2097151.0 / (mx - mn) : 0.0;       // 21 bits per dimension
            }
            parallel_for(Nlocs, [&, kd](int64_t b, int64_t e) {
                for (int64_t i = b; i < e; ++i) {
                    uint64_t k = 0;
                    uint32_t q[3] = {0, 0, 0};
                    for (int t = 0; t < kd; ++t) {
                        const double v = (locs[i + (int64_t)t * Nlocs] - lo[t]) * sc[t];
                        q[t] = (v == v && v > 0) ? (uint32_t)(v < 2097151.0 ? v : 2097151.0) : 0u;
                    }
                    for (int bit = 20; bit >= 0; --bit)
                        for (int t = 0; t < kd; ++t) k = (k << 1) | ((q[t] >> bit) & 1u);
                    key[(size_t)i] = k;
                }
            });
        }
        std::vector<int32_t> order((size_t)Nlocs);
        sort_order_by_key(key.data(), Nlocs, order.data());                // all keys 0 without locs: identity
        for (int64_t r = 0; r < Nlocs; ++r) newpos[(size_t)order[(size_t)r]] = (int32_t)r;
    }
    const int32_t *np_ = newpos.data();
    tm.lap("plan: morton order");

    // ---- host re-layout: column-major 1-based R matrices -> row-major, 0-based, right-aligned rows
    const int64_t rows = pl->rows;
    std::vector<int32_t> nn((size_t)(rows > 0 ? rows : 1) * P, -1);
    std::vector<uint8_t> cd((size_t)(rows > 0 ? rows : 1) * P, 1);
    std::vector<int> err_flag(1, GPV_OK);
    int *errp = err_flag.data();
    std::atomic<int> latent_nb{0};                     // a neighbour conditioned on as latent y (gpv_plan_loglik_grad refuses)
    std::atomic<int> *latp = &latent_nb;
    // stored set s <- conditioning set (row) rowsrc[s]: rows sorted by the Morton position of the point they belong
    // to (the last entry of the row, R/U_sparsity.R:32), so that sets processed together share neighbours in L2
    std::vector<int32_t> rowsrc((size_t)(rows > 0 ? rows : 1), 0);
    {
        std::vector<uint64_t> selfpos((size_t)(rows > 0 ? rows : 1), 0);
        for (int64_t r = 0; r < rows; ++r) {
            const int v = revNN[(row_begin + r) + (int64_t)(ncolNN - 1) * Nlocs];
            selfpos[(size_t)r] = (!is_missing(v) && v >= 1 && (int64_t)v <= Nlocs) ? (uint64_t)np_[v - 1] : 0;
        }
        sort_order_by_key(selfpos.data(), rows, rowsrc.data());
    }
    const int32_t *rs_ = rowsrc.data();
    tm.lap("plan: set order");
    parallel_for(rows, [=, &nn, &cd](int64_t b, int64_t e) {   // (np_, rs_ captured by value)
        std::vector<int32_t> tmp(ncolNN);
        for (int64_t r = b; r < e; ++r) {
            const int64_t k = row_begin + rs_[r];
            int n0 = 0;
            for (int j = 0; j < ncolNN; ++j) {            // src/U_NZentries.cpp:44: non-zero entries, compacted, -1
                const int v = revNN[k + (int64_t)j * Nlocs];
                if (is_missing(v)) continue;
                if (v < 1 || (int64_t)v > Nlocs) { *errp = GPV_ERR_INDEX; continue; }
                tmp[n0++] = np_[v - 1];
            }
            int32_t *nr = &nn[(size_t)r * P];
            uint8_t *cr = &cd[(size_t)r * P];
            for (int t = 0; t < n0; ++t) {
                nr[P - n0 + t] = tmp[t];
                // :47 pairs the compacted indices with the LAST n0 entries of the cond row
                int c = 1;
                if (revCond) {
                    c = revCond[k + (int64_t)(ncolNN - n0 + t) * Nlocs];
                    if (c == INT_MIN) { *errp = GPV_ERR_BAD_ARG; c = 1; }
                }
                cr[P - n0 + t] = (uint8_t)(c != 0);
                if (c != 0 && t < n0 - 1) latp->store(1, std::memory_order_relaxed);
            }
        }
    });
    if (err_flag[0] != GPV_OK) return err_flag[0];
    pl->latent_nb = latent_nb.load() != 0;
    tm.lap("plan: index re-layout");
    std::vector<double> lr((size_t)Nlocs * pl->locs_ld, 0.0);
    if (locs) {
        const int ld = pl->locs_ld;
        // one pass over the coordinates: the largest finite |coordinate|, and for the lean kernel whether all of them are
        // finite and how far apart two locations can be at most (the bounding box's diagonal)
        double mabs = 0.0, diam2 = 0.0;
        bool fin = true;
        for (int t = 0; t < dim; ++t) {
            double mn = INFINITY, mx = -INFINITY;
            const double *c = locs + (int64_t)t * Nlocs;
            for (int64_t i = 0; i < Nlocs; ++i) {
                const double v = std::fabs(c[i]);
                if (v > mabs && v <= 1.79e308) mabs = v;
                fin = fin && std::isfinite(v);
                mn = c[i] < mn ? c[i] : mn;
                mx = c[i] > mx ? c[i] : mx;
            }
            diam2 += (mx - mn) * (mx - mn);
        }
        pl->coord_maxabs = mabs;
        pl->coords_finite = fin;
        pl->bbox_diam = fin ? std::sqrt(diam2) : INFINITY;
        parallel_for(Nlocs, [=, &lr](int64_t b, int64_t e) {
            for (int64_t i = b; i < e; ++i)
                for (int t = 0; t < dim; ++t) lr[(size_t)np_[i] * ld + t] = locs[i + (int64_t)t * Nlocs];
        });
    }

    // range of the pair distances inside conditioning sets (for the general-nu table): the closest pair overall is some
    // point and its nearest earlier neighbour; no pair of a set is farther apart than twice its farthest neighbour
    if (locs) {
        std::mutex mu_;
        double gmin = INFINITY, gmax = 0.0;
        constexpr int kHist = 8800;
        pl->dist_hist.assign(kHist, 0);
        const int64_t stride = Nlocs > 8192 ? Nlocs / 4096 : 1;          // the pairs of ~4096 sets: ~2e6 distances
        parallel_for(Nlocs, [&](int64_t b, int64_t e) {
            double lmin = INFINITY, lmax = 0.0;
            std::vector<int64_t> lh(kHist, 0);
            std::vector<int> members((size_t)ncolNN);
            auto dist_of = [&](int a1, int b1) {
                double r2 = 0.0;
                for (int t = 0; t < dim; ++t) {
                    const double df = locs[(a1 - 1) + (int64_t)t * Nlocs] - locs[(b1 - 1) + (int64_t)t * Nlocs];
                    r2 += df * df;
                }
                return std::sqrt(r2);
            };
            for (int64_t k = b; k < e; ++k) {
                const int self = revNN[k + (int64_t)(ncolNN - 1) * Nlocs];
                if (is_missing(self) || self < 1 || (int64_t)self > Nlocs) continue;
                int nm = 0;
                for (int j = 0; j < ncolNN - 1; ++j) {
                    const int v = revNN[k + (int64_t)j * Nlocs];
                    if (is_missing(v) || v < 1 || (int64_t)v > Nlocs) continue;
                    members[(size_t)nm++] = v;
                    const double dd = dist_of(self, v);
                    if (dd > lmax) lmax = dd;                    // first valid entry is the farthest, but rows need not be sorted
                    if (dd > 0.0 && dd < lmin) lmin = dd;
                }
                if (k % stride != 0) continue;
                members[(size_t)nm++] = self;
                for (int a1 = 1; a1 < nm; ++a1)
                    for (int b1 = 0; b1 < a1; ++b1) {
                        const double dd = dist_of(members[(size_t)a1], members[(size_t)b1]);
                        if (dd > 0.0 && std::isfinite(dd)) {
                            const int ex = (int)std::floor(4.0 * std::log2(dd)) + kHist / 2;
                            lh[(size_t)(ex < 0 ? 0 : (ex > kHist - 1 ? kHist - 1 : ex))]++;
                        }
                    }
            }
            std::lock_guard<std::mutex> g(mu_);
            if (lmin < gmin) gmin = lmin;
            if (lmax > gmax) gmax = lmax;
            for (size_t t = 0; t < lh.size(); ++t) pl->dist_hist[t] += lh[t];
        });
        pl->dist_min = std::isfinite(gmin) ? gmin : 0.0;
        pl->dist_max = gmax;
    }
    tm.lap("plan: location records");
    GPV_HIP(hipStreamCreateWithFlags(pl->stream.put(), hipStreamNonBlocking));
    GPV_HIP(hipEventCreate(pl->ev0.put()));
    GPV_HIP(hipEventCreate(pl->ev1.put()));
    GPV_BUF(pl->d_nn, upload(nn.data(), nn.size()));
    GPV_BUF(pl->d_cond, upload(cd.data(), cd.size()));
    GPV_BUF(pl->d_locs, upload(lr.data(), lr.size()));
    GPV_BUF(pl->d_nuggets, resize((size_t)Nlocs));
    GPV_BUF(pl->d_block, resize(kNSums * (size_t)kMaxGrid));
    GPV_BUF(pl->d_sums, resize(kNSums));
    GPV_BUF(pl->d_ticket, resize(16));
    GPV_HIP(hipMemset(pl->d_ticket, 0, 64));
    GPV_BUF(pl->h_sums, resize(2 * kNSums));
    GPV_HIP(hipHostGetDevicePointer((void **)&pl->h_sums_dev, pl->h_sums, 0));
    std::memset(pl->h_sums, 0, sizeof(double) * 2 * kNSums);
    GPV_BUF(pl->d_rowid, upload(rowsrc.data(), rowsrc.size()));
    GPV_BUF(pl->d_newpos, upload(newpos.data(), (size_t)Nlocs));
    GPV_BUF(pl->d_stage, resize((size_t)Nlocs));
    // lean kernel: one byte per task of SPW sets (internal set order): does the task hold a missing neighbour or a set beyond
    // `rows`.  This plan's rows are fixed (a shard is a plan of its own), so the bytes are too.
    pl->idx32 = rows * (int64_t)P < ((int64_t)1 << 31);
    const int spw = generic ? 0 : sets_per_task(P);
    if (spw > 0 && rows > 0) {
        const int64_t ntasks = (rows + spw - 1) / spw;
        std::vector<uint8_t> pad((size_t)((ntasks + 3) & ~(int64_t)3) + 4, 1);
        const int32_t *nnp = nn.data();
        parallel_for(ntasks, [=, &pad](int64_t b, int64_t e) {
            for (int64_t t = b; t < e; ++t) {
                bool any = (t + 1) * spw > rows;
                for (int64_t sset = t * spw; sset < (t + 1) * spw && !any; ++sset)
                    for (int j = 0; j < P; ++j) any = any || nnp[sset * P + j] < 0;
                pad[(size_t)t] = any ? 1 : 0;
            }
        });
        GPV_BUF(pl->d_task_pad, upload(pad.data(), pad.size()));
    }
    tm.lap("plan: alloc + H2D");
    pl->h_newpos.swap(newpos);
    return GPV_OK;
}

int gpv_plan_set_data(gpv_plan *pl, const double *z_ord)
{
    if (!pl || !z_ord) return GPV_ERR_BAD_ARG;
    // an evaluation enqueued earlier on a caller stream may still be reading the records / d_zuser this call rewrites
    if (const int rc = enter(pl)) return rc;
    GPV_HIP(hipMemcpyAsync(pl->d_stage, z_ord, sizeof(double) * (size_t)pl->Nlocs, hipMemcpyHostToDevice, pl->stream));
    if (pl->dim <= 3) {
        GPV_HIP(launch_scatter(pl->d_stage, pl->d_newpos, pl->Nlocs, pl->d_locs, 4, 3, pl->stream));   // rec[.][3] = datum
    } else {
        GPV_BUF(pl->d_z, ensure((size_t)pl->Nlocs));
        GPV_HIP(launch_scatter(pl->d_stage, pl->d_newpos, pl->Nlocs, pl->d_z, 1, 0, pl->stream));
    }
    GPV_BUF(pl->d_zuser, ensure((size_t)pl->Nlocs));
    GPV_HIP(hipMemcpyAsync(pl->d_zuser, pl->d_stage, sizeof(double) * (size_t)pl->Nlocs, hipMemcpyDeviceToDevice, pl->stream));
    GPV_HIP(hipStreamSynchronize(pl->stream));
    pl->has_z = true;
    return GPV_OK;
}

int gpv_plan_set_observed(gpv_plan *pl, const int *obs_ord)
{
    if (!pl) return GPV_ERR_BAD_ARG;
    if (const int rc = enter_final(pl)) return rc;
    for (auto &g : pl->pgraph) g.exec.reset();        // the captured passes hold the address of the nuggets they read
    std::vector<uint8_t> h((size_t)pl->Nlocs);
    bool all = true;
    for (int64_t i = 0; obs_ord && i < pl->Nlocs; ++i) { h[(size_t)i] = obs_ord[i] != 0 ? 1 : 0; all = all && h[(size_t)i]; }
    if (all) {                                        // (or no list at all: back to "every location is observed")
        GPV_HIP(pl->d_obs.reset());
        return GPV_OK;
    }
    GPV_BUF(pl->d_obs, ensure((size_t)pl->Nlocs));
    GPV_HIP(hipMemcpy(pl->d_obs, h.data(), (size_t)pl->Nlocs, hipMemcpyHostToDevice));
    return GPV_OK;
}

// ---- one evaluation of a plan, phase by phase (plan_eval_impl below is their sequence) ----------------------------------------
constexpr int kPostFlags = GPV_WANT_DENOM | GPV_WANT_MEAN_B;          // the evaluation runs a posterior pass

// the evaluation's nuggets: a constant, the caller's vector (inspected for the lean kernel, uploaded, scattered into the internal
// order) or what a Vecchia-Laplace step left in HBM; with unobserved locations also the masked copy the posterior pass reads
static int eval_nuggets(gpv_plan *pl, const double *nuggets, int64_t n_nuggets, int flags, hipStream_t st)
{
    if (!nuggets && n_nuggets != -1) return GPV_ERR_BAD_ARG;
    if (n_nuggets == 1) {
        pl->nug_is_scalar = true;                                         // R/createU.R:74
        pl->nug_scalar = nuggets[0];
    } else if (n_nuggets == -1 && pl->d_nug_user) {
        pl->nug_is_scalar = false;                                        // per-location nuggets already in HBM (VL step)
        pl->nug_vec_ok = false;                                           // (written on the device: not inspected)
    } else if (n_nuggets == pl->Nlocs) {
        pl->nug_is_scalar = false;
        std::atomic<int> okv{1};
        std::atomic<int> *okp = &okv;
        parallel_for(pl->Nlocs, [=](int64_t b, int64_t e) {
            bool ok = true;
            for (int64_t i = b; i < e; ++i) ok = ok && std::isfinite(nuggets[i]) && nuggets[i] <= 0x1p990;
            if (!ok) okp->store(0, std::memory_order_relaxed);
        });
        pl->nug_vec_ok = okv.load() != 0;
        GPV_BUF(pl->d_nug_user, ensure((size_t)pl->Nlocs));
        GPV_HIP(hipMemcpyAsync(pl->d_nug_user, nuggets, sizeof(double) * (size_t)pl->Nlocs, hipMemcpyHostToDevice, st));
        GPV_HIP(launch_scatter(pl->d_nug_user, pl->d_newpos, pl->Nlocs, pl->d_nuggets, 1, 0, st));
    } else {
        return GPV_ERR_BAD_ARG;
    }
    // locations without an observation (prediction locations): the set kernel keeps the caller's value (0 in the
    // reference's nuggets.all.ord, R/createU.R:75-77; such a location is only ever conditioned on as latent, where the
    // nugget drops out), the posterior pass reads +Inf there: no 1/tau on the diagonal of W = U_y U_y^T, no z/tau in z2.
    // The masked values go to a buffer of their own that only the pass reads: Zentries, D_ord and the Vecchia-Laplace
    // step keep seeing the caller's nuggets, and evaluations without a pass do not touch it.
    if (pl->d_obs && !pl->nug_is_scalar && (flags & kPostFlags)) {
        GPV_BUF(pl->d_nug_masked, ensure((size_t)pl->Nlocs));
        GPV_HIP(launch_mask_unobserved(pl->d_nug_user, pl->d_nug_masked, pl->d_obs, pl->Nlocs, st));
    }
    // with unobserved locations the posterior pass needs the per-location form (a constant cannot say "none here")
    if (pl->d_obs && (flags & kPostFlags) && pl->nug_is_scalar) return GPV_ERR_BAD_ARG;
    return GPV_OK;
}

// the hand-off of the totals by memory: the 8 sequence numbers behind the 8 totals of h_sums (gpv_reduce_tail.hpp, publish_seq)
static unsigned long long *seq_cells_of(gpv_plan *pl) { return reinterpret_cast<unsigned long long *>(pl->h_sums_dev + kNSums); }

// the launch arguments that do not depend on the covariance family's extras, and where this evaluation's totals go
static int eval_set_args(gpv_plan *pl, const CovSetup &cs, int flags, hipStream_t st, double *d_sums_out, SetArgs &a)
{
    a.rec = pl->d_locs;
    a.locs = pl->d_locs;
    a.nn = pl->d_nn;
    a.cond = pl->d_cond;
    a.rowid = pl->d_rowid;
    a.nuggets = pl->nug_is_scalar ? nullptr : pl->d_nuggets;
    a.nug_scalar = pl->nug_scalar;
    a.z = (flags & (GPV_WANT_LOGLIK_Z | GPV_WANT_NUMERATOR)) ? pl->d_z : nullptr;
    a.covvals = pl->d_covvals;
    a.Lentries = (flags & GPV_WANT_U) ? pl->d_L : nullptr;
    a.aout = (flags & kPostFlags) ? pl->d_avec : nullptr;
    const bool fused = (flags & kPostFlags) && pl->post_fused;
    a.block_sums = pl->d_block;
    a.sums = pl->d_sums;
    // with a communicator attached the totals of THIS rank stay in d_sums, RCCL sums them over the ranks in place on the
    // same stream, and one 64-byte copy command hands them to the host (or to the caller's device buffer)
    gpv_comm *const cm = pl->comm;
    if (cm && (flags & kPostFlags)) return GPV_ERR_STATE;         // the posterior pass does not shard
    pl->sums_on_host = (d_sums_out == nullptr);
    a.sums_copy = cm ? nullptr : (d_sums_out ? d_sums_out : pl->h_sums_dev);
    a.ticket = pl->d_ticket;
    // the set kernel's totals are final (no posterior pass adds to them) and go to the plan's own host buffer: the kernel
    // appends the sequence number of this evaluation and gpv_plan_get_sums spins on it instead of waiting for the stream
    static const bool no_seq = dev_getenv("GPV_NO_SEQ_HANDOFF") != nullptr;
    // inside somebody's stream capture the sequence number would be frozen into the graph (every replay would publish the
    // same one, and gpv_plan_get_sums would accept the previous replay's totals without waiting): wait for the stream there
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    const bool final_here = !(flags & kPostFlags) && d_sums_out == nullptr && !no_seq && cap == hipStreamCaptureStatusNone;
    if (pl->ticket_dirty) {                        // the previous evaluation of this plan ended in an error: the arrival counter
        GPV_HIP(hipMemsetAsync(pl->d_ticket, 0, 64, st));   // of its kernel may be non-zero (no workgroup would ever be "last")
        pl->ticket_dirty = false;
    }
    pl->sums_by_seq = final_here;
    if (final_here) ++pl->seq;
    a.seq_cells = (final_here && !cm) ? seq_cells_of(pl) : nullptr;
    a.seq = pl->seq;
    a.nug_cell = (flags & GPV_WANT_DENOM) ? pl->d_nug_post.get() : nullptr;
    a.rows = pl->rows;
    a.nlocs = pl->Nlocs;
    a.locs_ld = pl->locs_ld;
    a.dim = pl->dim;
    a.cov = cs.cov;
    a.flags = flags | (fused ? kFlagFused : 0) | ((fused && (flags & GPV_WANT_MEAN_B)) ? kFlagBoth : 0);
    a.sig0 = cs.sig0; a.sA = cs.sA; a.cA = cs.cA; a.sB = cs.sB; a.cB = cs.cB;
    // The Matern kernels multiply the coordinates by cA = sqrt(2 nu)/range once per row instead of the distance once per
    // pair.  Where c * |x| would overflow (range below 1e-300 of the coordinates' magnitude) the reference's own dist/range
    // is Inf for every pair of distinct points and its covariance NaN (Inf * 0, src/Matern.cpp:52,68,80): all blocks fail.
    // Same outcome here, through the diagonal.  (nu = 0.5 gives exact zeros there instead, an independent model: not mirrored.)
    // (matern_scaledim: the same of the scaled copy, whose coordinates are at most inv_max times the plan's)
    if (cs.cov != COV_DENSE && cs.cov != COV_ESQE && !(std::fabs(cs.cA) * cs.inv_max * pl->coord_maxabs < 1e300)) a.sig0 = NAN;
    a.mt = nullptr; a.mt_base = 0; a.mt_nseg = 0; a.mt_full = 0; a.mt_win = 0;
    return GPV_OK;
}

// matern_scaledim: the set kernel reads a copy of the records (dim <= 3; the coordinate array otherwise) whose coordinates are
// multiplied by 1 / range_t and whose datum slot is the plan's, written on the evaluation's stream in front of the kernel at
// EVERY evaluation: gpv_plan_set_data and the Vecchia-Laplace steps rewrite the datum slot of d_locs between evaluations.  The
// inverse ranges are arguments of that launch, which is no part of a captured graph (the posterior pass reads no coordinate).
static int eval_scaled_locs(gpv_plan *pl, const CovSetup &cs, hipStream_t st, const double *&rec, const double *&locs)
{
    const size_t cnt = (size_t)pl->Nlocs * (size_t)pl->locs_ld;
    GPV_BUF(pl->d_locs_sc, ensure(cnt));
    GPV_HIP(launch_scale_locs(pl->d_locs, pl->d_locs_sc, pl->Nlocs, pl->locs_ld, pl->dim, cs.inv, st));
    rec = pl->d_locs_sc;
    locs = pl->d_locs_sc;
    return GPV_OK;
}

// The lean likelihood-only kernel leaves out what these facts make a no-op (the launcher checks family, dimension and
// row length, sets_args_lean):
//   coordinates finite, nuggets finite and <= 2^990, sigma^2 finite and small against 2^990: no NaN to inject into a
//     diagonal, none above the 2^990 clamp;
//   t_bounded: parameters finite and cA * (bounding-box diagonal) <= 500: no pair's scaled distance reaches the clamp at
//     1000 (500 leaves the rounding of this product and of the kernel's own sum of squares a wide margin);
//   idx32; flags exactly GPV_WANT_LOGLIK_Z.
// GPV_NO_LEAN=1: always the general likelihood-only kernel (tests and A/B runs).
static void lean_facts(const gpv_plan *pl, const CovSetup &cs, SetArgs &a)
{
    static const bool no_lean = getenv("GPV_NO_LEAN") != nullptr;
    const bool nug_ok = pl->nug_is_scalar ? (std::isfinite(pl->nug_scalar) && pl->nug_scalar <= 0x1p990) : pl->nug_vec_ok;
    const bool parms_ok = std::isfinite(a.sig0) && std::fabs(a.sig0) <= 0x1p930 && std::isfinite(a.sA) && std::isfinite(a.cA);
    // (matern_scaledim: no pair of the scaled copy is farther apart than inv_max times the bounding box's diagonal, and the
    // copy is finite where the coordinates are, by the test of eval_set_args; inv_max is 1 for the other families)
    const bool t_bounded = parms_ok && std::fabs(a.cA) * cs.inv_max * pl->bbox_diam <= 500.0;
    const bool only_z = a.flags == GPV_WANT_LOGLIK_Z;
    a.task_pad = pl->d_task_pad;
    a.lean_ok = (!no_lean && pl->d_task_pad && pl->coords_finite && nug_ok && pl->idx32 && t_bounded && only_z) ? 1 : 0;
}

// LDS window of the kernel (gpv_sets_kernel.hpp, mt_window_rows): of the table's `noct` octaves of s = dist/range, the first
// of those `win_oct` consecutive ones that hold most of the pair distances inside the plan's conditioning sets.  dist_hist counts
// distances by quarter octave, e_lo is the binary exponent of the table's first segment, sh = log2 |cA|.
static int matern_window_octave(const std::vector<int64_t> &dist_hist, int e_lo, int noct, int win_oct, double sh)
{
    const int kHist = (int)dist_hist.size();
    std::vector<double> H((size_t)noct, 0.0);
    for (int ex = 0; ex < kHist; ++ex) {
        if (!dist_hist[(size_t)ex]) continue;
        const int o = (int)std::floor(((double)(ex - kHist / 2) + 0.5) * 0.25 + sh) - e_lo;   // the bin's centre
        if (o >= 0 && o < noct) H[(size_t)o] += (double)dist_hist[(size_t)ex];
    }
    double best = -1.0;
    int bo = 0;
    for (int o = 0; o + win_oct <= noct || o == 0; ++o) {
        double mw = 0.0;
        for (int t = 0; t < win_oct && o + t < noct; ++t) mw += H[(size_t)(o + t)];
        if (mw > best) { best = mw; bo = o; }
        if (o + win_oct > noct) break;
    }
    return bo;
}

// general nu: the evaluation's table of normcon s^nu K_nu(s) e^s over the plan's range of pair distances, fitted on the
// evaluation's stream in front of the set kernel.  GPV_NO_MATERN_TABLE=1: the kernel evaluates the Bessel function per pair.
static int matern_table_prepare(gpv_plan *pl, const CovSetup &cs, hipStream_t st, SetArgs &a)
{
    static const bool no_tab = getenv("GPV_NO_MATERN_TABLE") != nullptr;
    if (no_tab || !(pl->dist_min > 0.0) || !(pl->dist_max >= pl->dist_min)) return GPV_OK;
    constexpr int kMaxSeg = 80 * MaternTab::SPO;                   // 80 octaves
    // two device copies of the table used alternately (and, for the host fit GPV_MATERN_TABLE_HOST=1 only, two pinned
    // staging buffers guarded by an event each, so that filling one never waits for the stream: the previous
    // evaluation may still be reading the other copy)
    const size_t tabn = (size_t)kMaxSeg * MaternTab::ROW;
    const int sl = pl->mt_slot ^= 1;
    GPV_BUF(pl->h_mt2[sl], ensure(tabn));
    GPV_BUF(pl->d_mt2[sl], ensure(tabn));
    if (!pl->mt_ev[sl]) GPV_HIP(hipEventCreateWithFlags(pl->mt_ev[sl].put(), hipEventDisableTiming));
    else GPV_HIP(hipEventSynchronize(pl->mt_ev[sl]));             // two evaluations ago: long done in steady state
    int full = 0, e_lo = 0;
    static const bool host_fit = getenv("GPV_MATERN_TABLE_HOST") != nullptr;    // cross-check of the device fit
    // (matern_scaledim: a pair at distance d has the scaled distance between inv_min d and inv_max d; both are 1 otherwise)
    const double s_lo = 0.5 * pl->dist_min * cs.cA * cs.inv_min, s_hi = 4.0 * pl->dist_max * cs.cA * cs.inv_max;
    if (host_fit) matern_tab_build(cs.sB, s_lo, s_hi, cs.sA, pl->h_mt2[sl], &a.mt_base, &a.mt_nseg, kMaxSeg, &full);
    else (void)matern_tab_range(s_lo, s_hi, kMaxSeg, &e_lo, &a.mt_base, &a.mt_nseg, &full);
    a.mt_full = (a.mt_nseg > 0 && full) ? 1 : 0;
    const int win_oct = sets_mt_window_rows(pl->P, pl->dim) / MaternTab::SPO;   // as many octaves as the instantiation has room for
    if (a.mt_nseg > 0 && win_oct > 0 && !pl->dist_hist.empty())
        a.mt_win = MaternTab::SPO * matern_window_octave(pl->dist_hist, (a.mt_base >> MaternTab::LSPO) - 1023,
                                                         a.mt_nseg / MaternTab::SPO, win_oct,
                                                         std::log2(std::fabs(cs.cA) * std::sqrt(cs.inv_min * cs.inv_max)));
    if (a.mt_nseg > 0) {
        // the fit runs on the evaluation's stream in front of the set kernel (~10 us; on the host it was 0.3 ms in
        // series with every optimiser step); the stream orders it behind the previous evaluation's reads
        if (host_fit)
            GPV_HIP(hipMemcpyAsync(pl->d_mt2[sl], pl->h_mt2[sl], sizeof(double) * (size_t)a.mt_nseg * MaternTab::ROW,
                                   hipMemcpyHostToDevice, st));
        else
            GPV_HIP(launch_matern_tab(cs.sB, e_lo, a.mt_nseg, cs.sA, pl->d_mt2[sl], st));
        a.mt = pl->d_mt2[sl];
    }
    pl->mt_pending = sl;
    return GPV_OK;
}

// the conditioning-set kernel between the timing events; the partial sums are totalled by its last workgroup (no reduction launch)
static int eval_launch_sets(gpv_plan *pl, const SetArgs &a, hipStream_t st)
{
    if (pl->timing) GPV_HIP(hipEventRecord(pl->ev0, st));
    pl->last_set_kernel = pl->generic ? 0 : sets_kernel_kind(pl->P, a);
    if (pl->generic) GPV_HIP(launch_sets_generic(pl->P, a, pl->cus, &pl->grid, st));
    else GPV_HIP(launch_sets(pl->P, a, pl->cus, &pl->grid, st));
    if (pl->timing) GPV_HIP(hipEventRecord(pl->ev1, st));   // ev0..ev1 brackets the conditioning-set kernel alone
    pl->timed = pl->timing;
    if (pl->mt_pending >= 0) {                     // the kernel that reads this evaluation's Matern table has been enqueued
        GPV_HIP(hipEventRecord(pl->mt_ev[pl->mt_pending], st));
        pl->mt_pending = -1;
    }
    return GPV_OK;
}

// with a communicator: this rank's totals summed over the ranks in place, then handed to the host or the caller's buffer
static int eval_allreduce(gpv_plan *pl, hipStream_t st, double *d_sums_out)
{
    const RcclApi *R = rccl_api();
    if (!R) return GPV_ERR_STATE;
    const int rr = R->AllReduce(pl->d_sums, pl->d_sums, (size_t)kNSums, /*ncclDouble*/ 8, /*ncclSum*/ 0, pl->comm->comm, st);
    if (rr != 0) return note_rccl(rr, "ncclAllReduce");
    // to the host by a 64-thread kernel that stores into pinned memory, not by a copy command: an event behind a 64-byte
    // hipMemcpyAsync took ~100 us longer to turn ready under hipEventQuery (measured, tools/comm_diag.py)
    if (d_sums_out) GPV_HIP(hipMemcpyAsync(d_sums_out, pl->d_sums, sizeof(double) * kNSums, hipMemcpyDeviceToDevice, st));
    else if (pl->sums_by_seq) GPV_HIP(launch_publish_sums(pl->d_sums, pl->h_sums_dev, seq_cells_of(pl), pl->seq, st));
    else GPV_HIP(hipMemcpyAsync(pl->h_sums, pl->d_sums, sizeof(double) * kNSums, hipMemcpyDeviceToHost, st));
    return GPV_OK;
}

// the mean sweep R^T u = t, mu = -u: the dense top block, the head levels in one workgroup, then one launch per level
static hipError_t mean_sweep_enqueue(gpv_plan *pl, const PostArgs &pa, hipStream_t st)
{
    hipError_t e = hipSuccess;
    if (pl->top_K > 0) e = launch_mean_top(pa, pl->d_u, pl->top_K, pl->d_topinfo, pl->d_toprows, st);
    if (e == hipSuccess) e = launch_mean_head(pa, pl->d_order2, pl->d_u, pl->d_levptr2, pl->mean_head_levels, st);
    for (size_t lv = (size_t)pl->mean_head_levels; e == hipSuccess && lv + 1 < pl->levptr2.size(); ++lv)
        e = launch_mean_level(pa, pl->d_order2, pl->d_u, pl->levptr2[lv], pl->levptr2[lv + 1] - pl->levptr2[lv], st);
    if (e == hipSuccess) e = launch_negate(pl->d_u, pl->d_mu, pl->Nlocs, st);
    return e;
}

// the posterior pass behind the set kernel: compaction (unless fused), the factor's levels and top block, the two sums into
// `mirror` and the mean sweep; replayed from the plan's captured graph of that combination
static int posterior_pass_enqueue(gpv_plan *pl, int flags, double *mirror, hipStream_t st)
{
    const bool want_mean = (flags & GPV_WANT_MEAN) != 0, mean_b = (flags & GPV_WANT_MEAN_B) != 0, fused = pl->post_fused;
    pl->have_factor = false;                                         // C is being rewritten: true again once the pass is enqueued
    // (constant nugget: the set kernel above left it in d_nug_post[0]; vector: d_nug_user, a fixed address as well)
    PostArgs pa;
    pa.colptr = pl->d_colptr; pa.crow = pl->d_crow;
    pa.colrec = pl->d_colrec; pa.rowrec = pl->d_rowrec; pa.tp = pl->d_tp;
    pa.C = pl->d_C; pa.cboff = pl->d_cboff; pa.z = pl->d_zuser;
    pa.nuggets = pl->nug_is_scalar ? nullptr : (pl->d_obs ? pl->d_nug_masked : pl->d_nug_user);
    pa.nug_cell = pl->d_nug_post;
    pa.tvec = pl->d_tvec; pa.rdiag = pl->d_rdiag; pa.ld = pl->post_ld;
    pa.meanrec = pl->d_meanrec;
    pa.rr0 = pl->d_rr0;
    // cond.yz = 'zy' (R/vecchia_prediction.R:68-70,118-126): V.ord is the reversed latent block B of U itself, no
    // factorisation.  After createU's removal of the dummy latent variables (R/createU.R:166-171) no latent row has an
    // entry in an observed column, so z2 = U[latent,] z1 = B a with a = z1[latent columns] = the a_k the set kernel
    // already produces, and mu = -B^-T B^-1 z2 = -B^-T a: ONE lower-triangular solve, the level-scheduled mean sweep
    // with R := B (the compaction writes B into both halves) and t := a.
    if (mean_b) pa.tvec = pl->d_avec;
    auto enqueue = [&]() -> hipError_t {
        hipError_t e = fused ? hipSuccess
                             : launch_posterior_compact(pl->d_L, pl->P, pl->d_avec, pl->d_colptr, pl->d_ccol, pl->d_cslot,
                                                        pl->d_cdel, pl->Nlocs, pl->post_nnz, pl->d_C, mean_b, st);
        if (mean_b) return e == hipSuccess ? mean_sweep_enqueue(pl, pa, st) : e;
        for (size_t lv = 0; e == hipSuccess && lv + 1 < pl->levptr.size(); ++lv)
            e = launch_posterior_level(pa, pl->levptr[lv], pl->levptr[lv + 1] - pl->levptr[lv], lv == 0,
                                       lv < pl->lev_lpc.size() ? pl->lev_lpc[lv] : 64, pl->lev_rr0[lv], st);
        if (e == hipSuccess && pl->top_K > 0)
            e = launch_posterior_top(pa, (int)(pl->Nlocs - pl->top_K), pl->top_K, pl->d_toppart, pl->d_topinfo, pl->d_toprows,
                                     pl->top_rr0, st);
        if (e == hipSuccess)
            e = launch_sum_pair(pl->d_rdiag, pl->d_tvec, pl->Nlocs, pl->d_post_part, pl->d_sums, mirror, st);
        if (e == hipSuccess && want_mean) e = mean_sweep_enqueue(pl, pa, st);
        return e;
    };
    static const bool post_skip = dev_getenv("GPV_POST_SKIP") != nullptr;   // developer aid (timing only, results are WRONG): the set
    if (post_skip) return GPV_OK;                                           // kernel of mode S without its pass
    gpv_plan::PostGraph &g = pl->pgraph[(want_mean ? 1 : 0) + (pl->nug_is_scalar ? 0 : 2) + (mean_b ? 4 : 0)];
    bool captured = false;
    GPV_HIP(graph_replay(g.exec, st, enqueue, /*stale: another mirror address*/ g.sums_out != mirror, &captured));
    if (captured) g.sums_out = mirror;
    pl->have_factor = true;                                          // (gpv_plan_lincomb reads C as this pass leaves it)
    ++pl->factor_stamp;
    if (want_mean || mean_b) pl->have_mean = true;
    return GPV_OK;
}

static int plan_eval_impl(gpv_plan *pl, const CovSetup &cs, const double *nuggets, int64_t n_nuggets, int flags,
                          void *stream_v, double *d_sums_out)
{
    flags &= 63;                                                  // (the bits above are the kernels' own)
    if (flags & GPV_WANT_MEAN) flags |= GPV_WANT_DENOM;
    if ((flags & GPV_WANT_MEAN_B) && (flags & GPV_WANT_DENOM)) return GPV_ERR_BAD_ARG;      // one posterior pass per evaluation
    if (flags & kPostFlags) {
        if (!pl->have_post) return GPV_ERR_STATE;
        flags |= GPV_WANT_NUMERATOR;
        if (!pl->post_fused) flags |= GPV_WANT_U;                 // (fused: the set kernel fills the compact blocks itself)
    }
    if ((flags & (GPV_WANT_LOGLIK_Z | GPV_WANT_NUMERATOR)) && !pl->has_z) return GPV_ERR_STATE;
    GPV_HIP(hipSetDevice(pl->device));
    hipStream_t st = stream_v ? (hipStream_t)stream_v : (hipStream_t)pl->stream;
    // the plan's buffers (nuggets, partial sums, U entries, posterior blocks) are reused by every evaluation: one that
    // moves to ANOTHER stream first waits for the previous stream, evaluations on one stream are ordered by it
    // (not while `st` is being captured into a graph: a host wait is illegal there, and the caller who captures owns the
    // ordering against the plan's earlier evaluations)
    hipStreamCaptureStatus cap0 = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap0) != hipSuccess) { (void)hipGetLastError(); cap0 = hipStreamCaptureStatusNone; }
    if (pl->last_stream && pl->last_stream != st && cap0 == hipStreamCaptureStatusNone) GPV_HIP(hipStreamSynchronize(pl->last_stream));
    pl->L_of_eval = 0;                                            // (nuggets and, with GPV_WANT_U, d_L are about to change)
    if (flags & GPV_WANT_U) GPV_BUF(pl->d_L, ensure((size_t)(pl->rows > 0 ? pl->rows : 1) * pl->P));
    int rc = cs.cov != COV_DENSE ? eval_nuggets(pl, nuggets, n_nuggets, flags, st) : GPV_OK;
    SetArgs a;
    if (rc == GPV_OK) rc = eval_set_args(pl, cs, flags, st, d_sums_out, a);
    if (rc != GPV_OK) return rc;
    lean_facts(pl, cs, a);
    if (cs.nscale > 0 && (rc = eval_scaled_locs(pl, cs, st, a.rec, a.locs)) != GPV_OK) return rc;
    if (cs.cov == COV_MATERN_GEN && (rc = matern_table_prepare(pl, cs, st, a)) != GPV_OK) return rc;
    if ((rc = eval_launch_sets(pl, a, st)) != GPV_OK) return rc;
    if (pl->comm && (rc = eval_allreduce(pl, st, d_sums_out)) != GPV_OK) return rc;
    if ((flags & kPostFlags) && (rc = posterior_pass_enqueue(pl, flags, a.sums_copy, st)) != GPV_OK) return rc;
    pl->evaluated = true;
    pl->have_U = (flags & GPV_WANT_U) != 0;
    ++pl->eval_count;
    // (a dense covariance matrix carries no nugget: U_NZentries_mat, src/U_NZentries.cpp:144)
    if (pl->have_U && cs.cov != COV_DENSE) pl->L_of_eval = pl->eval_count;
    pl->last_stream = st;
    return GPV_OK;
}

// every caller's way into plan_eval_impl: an evaluation that failed after its launch may have started leaves the arrival
// counter of the fused reduction mid-count; the next evaluation of the plan resets it first
static int plan_eval_checked(gpv_plan *pl, const CovSetup &cs, const double *nuggets, int64_t n_nuggets, int flags,
                             void *stream, double *d_sums_out)
{
    const int rc = plan_eval_impl(pl, cs, nuggets, n_nuggets, flags, stream, d_sums_out);
    if (rc != GPV_OK && rc != GPV_ERR_BAD_ARG) pl->ticket_dirty = true;
    return rc;
}

int gpv_plan_eval(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, const double *nuggets,
                  int64_t n_nuggets, int flags, void *stream, double *d_sums_out)
{
    if (!pl) return GPV_ERR_BAD_ARG;
    CovSetup cs;
    const int st = cov_setup(covType, covparms, ncovparms, pl->dim, cs);
    if (st != GPV_OK) return st;
    return plan_eval_checked(pl, cs, nuggets, n_nuggets, flags, stream, d_sums_out);
}

int gpv_rccl_version(void)
{
    const RcclApi *R = rccl_api();
    return R ? R->version : 0;
}

int gpv_comm_unique_id(void *id128)
{
    if (!id128) return GPV_ERR_BAD_ARG;
    const RcclApi *R = rccl_api();
    if (!R) return GPV_ERR_STATE;
    RcclId id;
    const int rr = R->GetUniqueId(&id);
    if (rr != 0) return note_rccl(rr, "ncclGetUniqueId");
    std::memcpy(id128, &id, sizeof(id));
    return GPV_OK;
}

int gpv_comm_create(gpv_comm **out, int device, int rank, int world, const void *id128)
{
    if (!out || !id128 || world < 1 || rank < 0 || rank >= world) return GPV_ERR_BAD_ARG;
    *out = nullptr;
    const RcclApi *R = rccl_api();
    if (!R) return GPV_ERR_STATE;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GPV_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return GPV_ERR_BAD_ARG;
    GPV_HIP(hipSetDevice(device));                 // RCCL binds the communicator to the CURRENT device
    RcclId id;
    std::memcpy(&id, id128, sizeof(id));
    void *c = nullptr;
    const int rr = R->CommInitRank(&c, world, id, rank);   // collective: returns when every rank has joined
    if (rr != 0 || !c) return note_rccl(rr, "ncclCommInitRank");
    // prove the communicator (and the hand-declared enum values) before any evaluation depends on it: all-reduce
    // (1, rank + 1) as doubles with "sum"; every rank must read (world, world (world + 1) / 2)
    {
        double h[2] = {1.0, (double)(rank + 1)};
        DevBuf<double> d;
        Stream ps;
        int bad = 0;
        if (d.upload(h, 2) != hipSuccess || hipStreamCreateWithFlags(ps.put(), hipStreamNonBlocking) != hipSuccess) bad = 1;
        int ar = 0;
        if (!bad) ar = R->AllReduce(d, d, 2, /*ncclDouble*/ 8, /*ncclSum*/ 0, c, ps);
        if (!bad && ar == 0 && (hipStreamSynchronize(ps) != hipSuccess || hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess))
            bad = 1;
        ps.reset();
        (void)d.reset();
        const double want0 = (double)world, want1 = 0.5 * (double)world * (double)(world + 1);
        if (bad || ar != 0 || h[0] != want0 || h[1] != want1) {
            (void)R->CommDestroy(c);
            if (ar != 0) return note_rccl(ar, "ncclAllReduce (probe)");
            g_hip_code = 0;
            std::snprintf(g_hip_text, sizeof(g_hip_text), "RCCL probe all-reduce over %d ranks returned (%g, %g), expected (%g, %g)",
                          world, h[0], h[1], want0, want1);
            return GPV_ERR_STATE;
        }
    }
    gpv_comm *cm = new gpv_comm;
    cm->comm = c; cm->device = device; cm->rank = rank; cm->world = world;
    *out = cm;
    return GPV_OK;
}

int gpv_comm_destroy(gpv_comm *cm)
{
    if (!cm) return GPV_OK;
    const RcclApi *R = rccl_api();
    if (R && cm->comm) {
        (void)hipSetDevice(cm->device);
        (void)R->CommDestroy(cm->comm);
    }
    delete cm;
    return GPV_OK;
}

int gpv_plan_set_comm(gpv_plan *pl, gpv_comm *cm)
{
    if (!pl) return GPV_ERR_BAD_ARG;
    if (cm && cm->device != pl->device) return GPV_ERR_BAD_ARG;
    if (pl->last_stream) { GPV_HIP(hipSetDevice(pl->device)); GPV_HIP(hipStreamSynchronize(pl->last_stream)); }
    pl->comm = cm;
    return GPV_OK;
}

static int build_posterior_impl(gpv_plan *pl, const int *revNN, const int *revCond, bool with_fill, double max_fill,
                                double *fill_ratio);

int gpv_plan_build_posterior(gpv_plan *pl, const int *revNN, const int *revCond)
{
    return build_posterior_impl(pl, revNN, revCond, false, 0.0, nullptr);
}

int gpv_plan_build_posterior_fill(gpv_plan *pl, const int *revNN, const int *revCond, double max_fill, double *fill_ratio)
{
    return build_posterior_impl(pl, revNN, revCond, true, max_fill, fill_ratio);
}

static int build_posterior_impl(gpv_plan *pl, const int *revNN, const int *revCond, bool with_fill, double max_fill,
                                double *fill_ratio)
{
    // symbolic structure of the latent block B of U (R/U_sparsity.R:36-56 restricted to latent rows) as column
    // lists, row lists and a level schedule; parameter independent, built once.
    if (fill_ratio) *fill_ratio = 1.0;
    if (!pl || !revNN || !revCond) return GPV_ERR_BAD_ARG;
    // a rebuild that fails half way must not leave the old schedule's graphs and flag over new tables: the plan has no
    // posterior structure from here until the last line of this function
    pl->have_post = false;
    pl->have_factor = false;
    pl->lc_ready = false;
    pl->sel_ready = false;
    pl->sgv_ready = false;
    if (pl->last_stream) { GPV_HIP(hipSetDevice(pl->device)); GPV_HIP(hipStreamSynchronize(pl->last_stream)); }
    pl->drop_graphs();
    if (pl->row_begin != 0 || pl->row_end != pl->Nlocs) return GPV_ERR_BAD_ARG;   // not shardable
    if (pl->Nlocs >= (int64_t)1 << 31) return GPV_ERR_BAD_ARG;
    const int64_t n = pl->Nlocs;
    const int p = pl->p;
    std::vector<int32_t> colptr((size_t)n + 1, 0), rowcnt((size_t)n + 1, 0);
    std::vector<int32_t> crow;
    std::vector<uint8_t> cslot;
    crow.reserve((size_t)n * 12);
    cslot.reserve((size_t)n * 12);
    std::vector<int32_t> tmp(p);
    for (int64_t k = 0; k < n; ++k) {
        int n0 = 0;
        for (int j = 0; j < p; ++j) {
            const int v = revNN[k + (int64_t)j * n];
            if (is_missing(v)) continue;
            if (v < 1 || (int64_t)v > n) return GPV_ERR_INDEX;
            tmp[n0++] = v - 1;
        }
        if (n0 == 0 || tmp[n0 - 1] != (int32_t)k) return GPV_ERR_BAD_ARG;        // last entry must be the point itself
        for (int t = 0; t < n0; ++t) {
            const int c = revCond[k + (int64_t)(p - n0 + t) * n];
            const bool latent = (c != 0 && c != INT_MIN);
            if (t == n0 - 1 && !latent) return GPV_ERR_BAD_ARG;
            if (latent) {
                if (tmp[t] > (int32_t)k) return GPV_ERR_BAD_ARG;                  // neighbours precede the point
                crow.push_back(tmp[t]);
                cslot.push_back((uint8_t)t);
            }
        }
        colptr[(size_t)k + 1] = (int32_t)crow.size();
        {   // ascending rows within the column (insertion sort, <= 64 entries); self = k is the maximum, stays last
            const size_t b0 = (size_t)colptr[(size_t)k], e0 = crow.size();
            for (size_t a = b0 + 1; a < e0; ++a) {
                const int32_t rv = crow[a];
                const uint8_t sv = cslot[a];
                size_t b = a;
                while (b > b0 && crow[b - 1] > rv) { crow[b] = crow[b - 1]; cslot[b] = cslot[b - 1]; --b; }
                crow[b] = rv; cslot[b] = sv;
            }
        }
    }
    // the level kernels own one lane per row of a column: at most 64 LATENT entries per conditioning set (the row length
    // m + 1 itself may be larger: under SGV about a third of a set is conditioned on as latent)
    int maxlat = 0;
    for (int64_t k = 0; k < n; ++k) maxlat = std::max(maxlat, (int)(colptr[(size_t)k + 1] - colptr[(size_t)k]));
    if (maxlat > 64) return GPV_ERR_UNSUPPORTED_M;
    int maxcnt = p <= 64 ? p : maxlat;
    if (with_fill) {
        // cond.yz = 'y' (R/vecchia_prediction.R:72-83): W = B B^T + D^-1 couples every two rows of a column, and the UL factor
        // R (= what t(chol(rev(W))) holds, reversed) fills in beyond the pattern of B.  Symbolic factorisation, last column
        // first: struct(R_.k) = {rows i <= k of W_.k} u U over the columns c whose parent is k of (struct(R_.c) minus c), parent(c) =
        // the largest row below c in struct(R_.c) (the elimination tree of the reversed matrix).  On the FILLED pattern, with
        // zeros where B has no entry, the fixed-pattern factorisation of the level kernels drops nothing: it is exact.
        // Bounded: refused when the filled pattern exceeds max_fill times nnz(B) or a column outgrows the 64 lanes of a
        // wavefront (the caller then factorises on the host, like the reference's CHOLMOD).
        const size_t nnzB = crow.size();
        std::vector<int32_t> rp((size_t)n + 1, 0);                       // row lists of B: columns c >= k that contain row k
        for (size_t e = 0; e < nnzB; ++e) rp[(size_t)crow[e] + 1]++;
        for (int64_t i = 0; i < n; ++i) rp[(size_t)i + 1] += rp[(size_t)i];
        std::vector<int32_t> rl(nnzB), fillpos(rp.begin(), rp.end() - 1);
        for (int64_t k = 0; k < n; ++k)
            for (int32_t e = colptr[(size_t)k]; e < colptr[(size_t)k + 1]; ++e) rl[(size_t)fillpos[(size_t)crow[(size_t)e]]++] = (int32_t)k;
        std::vector<std::vector<int32_t>> st((size_t)n);                 // struct(R_.k), ascending, k last
        std::vector<std::vector<int32_t>> child((size_t)n);
        std::vector<int32_t> mark((size_t)n, -1), buf;
        size_t total = 0;
        const size_t budget = (size_t)(max_fill > 0.0 ? max_fill * (double)nnzB : 4.0 * (double)nnzB) + (size_t)n;
        for (int64_t k = n - 1; k >= 0; --k) {
            buf.clear();
            auto add = [&](int32_t i) {
                if (i <= (int32_t)k && mark[(size_t)i] != (int32_t)k) { mark[(size_t)i] = (int32_t)k; buf.push_back(i); }
            };
            for (int32_t q = rp[(size_t)k]; q < rp[(size_t)k + 1]; ++q) {   // W_.k: rows of every column of B that holds row k
                const int32_t c = rl[(size_t)q];
                for (int32_t e = colptr[(size_t)c]; e < colptr[(size_t)c + 1]; ++e) add(crow[(size_t)e]);
            }
            for (int32_t c : child[(size_t)k])
                for (int32_t i : st[(size_t)c]) if (i != c) add(i);
            std::sort(buf.begin(), buf.end());
            if (buf.empty() || buf.back() != (int32_t)k) return GPV_ERR_BAD_ARG;
            total += buf.size();
            if (buf.size() > 64 || total > budget) {
                // (the ratio over the columns processed so far: the fill grows towards the early columns, so this is a lower bound)
                const size_t seen = nnzB - (size_t)colptr[(size_t)k];
                if (fill_ratio) *fill_ratio = (double)total / (double)(seen ? seen : 1);
                return GPV_ERR_UNSUPPORTED_M;
            }
            if (buf.size() >= 2) child[(size_t)buf[buf.size() - 2]].push_back((int32_t)k);   // parent = largest row below k
            st[(size_t)k] = buf;
        }
        if (fill_ratio) *fill_ratio = (double)total / (double)(nnzB ? nnzB : 1);
        // the filled columns replace B's: an entry B has carries its Lentries slot, a fill entry 0xFF (the compaction writes 0)
        std::vector<int32_t> colptr2((size_t)n + 1, 0), crow2;
        std::vector<uint8_t> cslot2;
        crow2.reserve(total);
        cslot2.reserve(total);
        for (int64_t k = 0; k < n; ++k) {
            int32_t e = colptr[(size_t)k];
            const int32_t e1 = colptr[(size_t)k + 1];
            for (int32_t i : st[(size_t)k]) {
                while (e < e1 && crow[(size_t)e] < i) ++e;
                crow2.push_back(i);
                cslot2.push_back((e < e1 && crow[(size_t)e] == i) ? cslot[(size_t)e] : (uint8_t)0xFF);
            }
            colptr2[(size_t)k + 1] = (int32_t)crow2.size();
            if ((int)st[(size_t)k].size() > maxcnt) maxcnt = (int)st[(size_t)k].size();
        }
        colptr.swap(colptr2);
        crow.swap(crow2);
        cslot.swap(cslot2);
    }
    pl->post_ld = (pl->P <= 64 && maxcnt < pl->P) ? pl->P : maxcnt;     // bound of the entries per column (LDS tiles are sized by it)
    const size_t nnz = crow.size();
    for (size_t e = 0; e < nnz; ++e) rowcnt[(size_t)crow[e] + 1]++;
    std::vector<int32_t> rowptr((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) rowptr[(size_t)i + 1] = rowptr[(size_t)i] + rowcnt[(size_t)i + 1];
    std::vector<int32_t> fill(rowptr.begin(), rowptr.end() - 1), rcol(nnz), qof(nnz);
    std::vector<uint8_t> rslot(nnz);
    for (int64_t k = 0; k < n; ++k)                        // ascending k => every row list ascends
        for (int32_t e = colptr[(size_t)k]; e < colptr[(size_t)k + 1]; ++e) {
            const int32_t i = crow[(size_t)e];
            rcol[(size_t)fill[(size_t)i]] = (int32_t)k;
            rslot[(size_t)fill[(size_t)i]] = cslot[(size_t)e];
            qof[(size_t)e] = fill[(size_t)i];              // row-list position of the pair (row i, column k)
            fill[(size_t)i]++;
        }
    // match lists: for the pair q = (row k, column c > k) every entry e of column c with row r_e <= k is a row of
    // column k as well (the latent conditioning sets of SGV are cliques; for other patterns the entry is dropped, which is
    // the zero-fill rule); store the position of r_e in column k (the entries of a column are kept in ascending row
    // order in the compact blocks, so e itself addresses the value)
    std::vector<int32_t> tptr(nnz + 1, 0);
    for (int64_t c = 0; c < n; ++c) {
        const int32_t b0 = colptr[(size_t)c], cn = colptr[(size_t)c + 1] - b0;
        for (int32_t ek = 0; ek + 1 < cn; ++ek) tptr[(size_t)qof[(size_t)(b0 + ek)] + 1] = ek + 1;   // entries 0..ek (k itself included)
    }
    if ((int64_t)nnz + n >= ((int64_t)1 << 31)) return GPV_ERR_BAD_ARG;       // 32-bit offsets into the compact blocks
    {
        int64_t total = 0;
        for (size_t q = 0; q < nnz; ++q) total += tptr[q + 1];
        if (total >= ((int64_t)1 << 31)) return GPV_ERR_BAD_ARG;              // 32-bit offsets into the match records
    }
    for (size_t q = 0; q < nnz; ++q) tptr[q + 1] += tptr[q];
    std::vector<uint8_t> tp((size_t)tptr[nnz] + 16);          // padded: the kernels read one (masked) byte at a record's start even when it is empty
    {
        const int32_t *cp_ = colptr.data(), *cr_ = crow.data(), *qo_ = qof.data(), *tq_ = tptr.data();
        uint8_t *tp_ = tp.data();
        parallel_for(n, [=](int64_t cb2, int64_t ce2) {
            for (int64_t c = cb2; c < ce2; ++c) {
                const int32_t b0 = cp_[c], cn = cp_[c + 1] - b0;
                for (int32_t ek = 0; ek + 1 < cn; ++ek) {
                    const int32_t k = cr_[b0 + ek];
                    const int32_t kb = cp_[k], kn = cp_[k + 1] - kb;
                    uint8_t *dst = tp_ + tq_[qo_[b0 + ek]];
                    int32_t w = 0;
                    for (int32_t e = 0; e <= ek; ++e) {
                        const int32_t r = cr_[b0 + e];
                        int32_t lo = 0, hi = kn;                    // position of r in column k (ascending rows)
                        while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (cr_[kb + mid] < r) lo = mid + 1; else hi = mid; }
                        if (lo < kn && cr_[kb + lo] == r) dst[w++] = (uint8_t)lo;
                        else dst[w++] = (uint8_t)0xFF;              // not a row of column k: dropped (never under SGV)
                    }
                }
            }
        });
    }
    // the dense top block (gpv_posterior_ext.h): the first columns of the ordering stay out of the schedule
    // (GPV_POST_TOP=0: all columns are scheduled; GPV_POST_TOP=64: the one-block form only)
    static const int top_env = getenv("GPV_POST_TOP") != nullptr ? atoi(getenv("GPV_POST_TOP")) : kTopMax;
    const bool no_top = top_env <= 0;
    const int64_t K0 = no_top ? 0 : std::min<int64_t>(n, kTopBlock);
    // level of column k >= K0 = 1 + max level of the columns c > k that contain row k
    std::vector<int32_t> lev((size_t)n, 0);
    int32_t maxlev = -1;
    for (int64_t k = n - 1; k >= K0; --k) {
        int32_t l = 0;
        for (int32_t q = rowptr[(size_t)k]; q < rowptr[(size_t)k + 1]; ++q) {
            const int32_t c = rcol[(size_t)q];
            if (c > (int32_t)k && lev[(size_t)c] + 1 > l) l = lev[(size_t)c] + 1;
        }
        lev[(size_t)k] = l;
        if (l > maxlev) maxlev = l;
    }
    // two-block form: the highest levels, a few columns each and one launch apiece, join the block while it has room.  A row
    // i of a column k waits for k (level(i) > level(k)), so with a column all its rows are taken, and nothing below waits for them.
    std::vector<int32_t> topcols;
    std::vector<uint8_t> in_top((size_t)n, 0);
    for (int64_t k = 0; k < K0; ++k) { topcols.push_back((int32_t)k); in_top[(size_t)k] = 1; }
    if (!no_top && top_env > kTopBlock && maxlev >= 0) {
        std::vector<int64_t> width((size_t)maxlev + 1, 0);
        for (int64_t k = K0; k < n; ++k) width[(size_t)lev[(size_t)k]]++;
        int64_t room = kTopMax - K0;
        int32_t L = maxlev + 1;
        while (L > 0 && width[(size_t)L - 1] <= room) { room -= width[(size_t)L - 1]; --L; }
        if (L <= maxlev) {
            for (int64_t k = K0; k < n; ++k)
                if (lev[(size_t)k] >= L) { topcols.push_back((int32_t)k); in_top[(size_t)k] = 1; }
            maxlev = L - 1;
        }
    }
    const int64_t K = (int64_t)topcols.size();
    pl->top_K = (int)K;
    pl->levptr.assign((size_t)(maxlev + 2), 0);
    for (int64_t k = K0; k < n; ++k)
        if (!in_top[(size_t)k]) pl->levptr[(size_t)lev[(size_t)k] + 1]++;
    for (int32_t l = 0; l <= maxlev; ++l) pl->levptr[(size_t)l + 1] += pl->levptr[(size_t)l];
    std::vector<int32_t> pos(pl->levptr.begin(), pl->levptr.end() - 1), order((size_t)n);
    for (int64_t k = n - 1; k >= K0; --k)
        if (!in_top[(size_t)k]) order[(size_t)pos[(size_t)lev[(size_t)k]]++] = (int32_t)k;
    for (int64_t j = 0; j < K; ++j) order[(size_t)(n - K + j)] = topcols[(size_t)j];   // the top block's records: after the schedule
    // The compact blocks are laid out in the Morton order of the locations (the internal order of the plan's location
    // records): a column gathers from the columns of the points that condition on it, its spatial neighbours, whose blocks
    // then share cache lines and L2 sets instead of being scattered by a maxmin ordering.
    std::vector<int32_t> cboff((size_t)n), cdel((size_t)n);
    int64_t c_entries = 0;
    {
        std::vector<int32_t> inv((size_t)n);
        const bool have_pos = pl->h_newpos.size() == (size_t)n;
        for (int64_t k = 0; k < n; ++k) inv[(size_t)(have_pos ? pl->h_newpos[(size_t)k] : (int32_t)k)] = (int32_t)k;
        // blocks start on 64-byte boundaries (4 entries): --mode S 433.5-433.8 -> 435.0-435.4 evaluations/s at n = 1e6, m = 30
        // (128 bytes: the same), for <= 5 % more memory.  GPV_POST_ALIGN (developer A/B): entries per boundary
        static const int al = dev_getenv("GPV_POST_ALIGN") ? std::max(1, atoi(dev_getenv("GPV_POST_ALIGN"))) : 4;
        int64_t off = 0;
        for (int64_t r = 0; r < n; ++r) {
            const int32_t k = inv[(size_t)r];
            off = (off + al - 1) / al * al;
            cboff[(size_t)k] = (int32_t)off;
            cdel[(size_t)k] = (int32_t)(off - colptr[(size_t)k]);
            off += colptr[(size_t)k + 1] - colptr[(size_t)k] + 1;
            if (off >= ((int64_t)1 << 31)) return GPV_ERR_BAD_ARG;
        }
        c_entries = off;
    }
    // inside a level: wide levels in Morton order too (concurrent wavefronts then work in the same neighbourhood), narrow
    // ones longest row lists first (they bound the level's duration)
    for (int32_t l = 0; l <= maxlev; ++l) {
        const auto b0 = order.begin() + pl->levptr[(size_t)l], e0 = order.begin() + pl->levptr[(size_t)l + 1];
        if (e0 - b0 > 2048 && pl->h_newpos.size() == (size_t)n)
            std::sort(b0, e0, [&](int32_t a, int32_t b) { return pl->h_newpos[(size_t)a] < pl->h_newpos[(size_t)b]; });
        else
            std::stable_sort(b0, e0, [&](int32_t a, int32_t b) {
                return rowptr[(size_t)a + 1] - rowptr[(size_t)a] > rowptr[(size_t)b + 1] - rowptr[(size_t)b];
            });
    }
    // lanes per column of a level: by the mean length of its row lists (the column itself included): rounds of 4 / 8 / 16
    // columns.  GPV_POST_LPC=64 (or 16, 32) in the environment forces one form (developer A/B).
    {
        const char *force = dev_getenv("GPV_POST_LPC");
        pl->lev_lpc.assign((size_t)(maxlev + 1), 64);
        for (int32_t l = 0; l <= maxlev; ++l) {
            const int32_t b0 = pl->levptr[(size_t)l], e0 = pl->levptr[(size_t)l + 1];
            if (e0 <= b0) continue;
            double tot = 0.0;
            for (int32_t i = b0; i < e0; ++i) tot += rowptr[(size_t)order[(size_t)i] + 1] - rowptr[(size_t)order[(size_t)i]];
            const double mean = tot / (e0 - b0);
            static const double t16 = dev_getenv("GPV_POST_T16") ? atof(dev_getenv("GPV_POST_T16")) : 4.5;
            static const double t32 = dev_getenv("GPV_POST_T32") ? atof(dev_getenv("GPV_POST_T32")) : 10.0;
            int lpc = mean <= t16 ? 16 : (mean <= t32 ? 32 : 64);
            if (force) lpc = atoi(force);
            pl->lev_lpc[(size_t)l] = (lpc == 16 || lpc == 32) ? lpc : 64;
            static const bool dbg = dev_getenv("GPV_POST_DEBUG") != nullptr;       // developer: the schedule's shape, level by level
            if (dbg) std::fprintf(stderr, "[gpv post] level %d: %d columns, mean row list %.1f, lanes/column %d\n", (int)l,
                                  (int)(e0 - b0), mean, pl->lev_lpc[(size_t)l]);
        }
    }
    std::vector<int4> colrec(2 * (size_t)n), rowrec(nnz);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t k = order[(size_t)i];
        const int32_t b0 = colptr[(size_t)k], cn = colptr[(size_t)k + 1] - b0;
        colrec[2 * (size_t)i] = make_int4(k, cboff[(size_t)k], cn, rowptr[(size_t)k]);
        colrec[2 * (size_t)i + 1] = make_int4(rowptr[(size_t)k + 1], 0, 0, 0);
    }
    std::vector<int32_t> ccol(nnz);
    for (int64_t c = 0; c < n; ++c) {
        const int32_t b0 = colptr[(size_t)c], cn = colptr[(size_t)c + 1] - b0;
        for (int32_t e = 0; e < cn; ++e) {
            const size_t q = (size_t)qof[(size_t)(b0 + e)];               // the pair (row crow[b0+e], column c)
            rowrec[q] = make_int4(cboff[(size_t)c], tptr[q], e | ((e + 1 < cn ? e + 1 : 0) << 8), (int)in_top[(size_t)c]);   // .w: column c is in the top block
            ccol[(size_t)(b0 + e)] = (int32_t)c;
        }
    }

    // PostArgs::rr0: the first round of every scheduled column's row list in schedule order, at the stride of its level's kernel
    std::vector<int4> rr0;
    {
        pl->lev_rr0.assign((size_t)(maxlev + 1), 0);
        int64_t tot = 0;
        std::vector<int> stride((size_t)(maxlev + 1), 0);
        for (int32_t l = 0; l <= maxlev; ++l) {
            const int cntl = pl->levptr[(size_t)l + 1] - pl->levptr[(size_t)l];
            stride[(size_t)l] = posterior_level_form(cntl, l == 0, pl->lev_lpc[(size_t)l], pl->post_ld).rr0_stride;
            pl->lev_rr0[(size_t)l] = tot;
            tot += (int64_t)cntl * stride[(size_t)l];
        }
        pl->top_rr0 = tot;
        tot += K * kTopRr0Stride;
        rr0.resize((size_t)tot + 1);
        auto fill_col = [&](int4 *dst, int32_t k, int st) {
            const int32_t qb = rowptr[(size_t)k], qe = rowptr[(size_t)k + 1];
            for (int s2 = 0; s2 < st; ++s2) dst[s2] = rowrec[(size_t)(qb + s2 < qe ? qb + s2 : qb)];
        };
        for (int32_t l = 0; l <= maxlev; ++l)
            for (int32_t i = pl->levptr[(size_t)l]; i < pl->levptr[(size_t)l + 1] && stride[(size_t)l] > 0; ++i)
                fill_col(rr0.data() + pl->lev_rr0[(size_t)l] + (int64_t)(i - pl->levptr[(size_t)l]) * stride[(size_t)l],
                         order[(size_t)i], stride[(size_t)l]);
        for (int64_t j = 0; j < K; ++j)
            fill_col(rr0.data() + pl->top_rr0 + j * kTopRr0Stride, topcols[(size_t)j], kTopRr0Stride);
    }

    // the top block's own tables: where each of its columns lives, and the index inside the block of each entry's row
    std::vector<int2> topinfo((size_t)K);
    std::vector<uint8_t> toprows((size_t)K * kTopBlock, (uint8_t)0xFF);
    for (int64_t j = 0; j < K; ++j) {
        const int32_t k = topcols[(size_t)j];
        topinfo[(size_t)j] = make_int2(k, cboff[(size_t)k]);
        const int32_t b0 = colptr[(size_t)k], cn = colptr[(size_t)k + 1] - b0;
        if (cn > kTopBlock) return GPV_ERR_UNSUPPORTED_M;
        for (int32_t e = 0; e < cn; ++e) {
            const auto it = std::lower_bound(topcols.begin(), topcols.end(), crow[(size_t)(b0 + e)]);
            if (it == topcols.end() || *it != crow[(size_t)(b0 + e)]) return GPV_ERR_STATE;     // (cannot happen: see above)
            toprows[(size_t)j * kTopBlock + (size_t)e] = (uint8_t)(it - topcols.begin());
        }
    }
    // second schedule for the posterior mean (R^T u = t): column k waits for the rows i < k it contains
    // (the columns of the top block are solved first, by one dense substitution: launch_mean_top; they wait for nothing outside)
    std::vector<int32_t> lev2((size_t)n, 0);
    int32_t maxlev2 = 0;
    for (int64_t k = 0; k < n; ++k) {
        if (in_top[(size_t)k]) { lev2[(size_t)k] = -1; continue; }
        int32_t l = 0;
        for (int32_t e = colptr[(size_t)k]; e < colptr[(size_t)k + 1]; ++e) {
            const int32_t i = crow[(size_t)e];
            if (i < (int32_t)k && lev2[(size_t)i] + 1 > l) l = lev2[(size_t)i] + 1;
        }
        lev2[(size_t)k] = l;
        if (l > maxlev2) maxlev2 = l;
    }
    pl->levptr2.assign((size_t)maxlev2 + 2, 0);
    for (int64_t k = 0; k < n; ++k)
        if (!in_top[(size_t)k]) pl->levptr2[(size_t)lev2[(size_t)k] + 1]++;
    for (int32_t l = 0; l <= maxlev2; ++l) pl->levptr2[(size_t)l + 1] += pl->levptr2[(size_t)l];
    std::vector<int32_t> pos2(pl->levptr2.begin(), pl->levptr2.end() - 1), order2((size_t)(n - K));
    for (int64_t k = 0; k < n; ++k)
        if (!in_top[(size_t)k]) order2[(size_t)pos2[(size_t)lev2[(size_t)k]]++] = (int32_t)k;

    GPV_HIP(hipSetDevice(pl->device));
    {
        // Fused compaction: every latent entry of a conditioning set learns its position in the set's column block (bits 1..7
        // of its cond byte: 1 + position), so that the set kernel deposits (B, 0) straight into the compact blocks and the
        // posterior pass needs neither the Lentries round trip (248 MB written, 248 MB read at n = 1e6, m = 30) nor the
        // compaction launch.  Not with fill (cond.yz = 'y'): the filled pattern has entries B lacks, zeroed by the compaction.
        const int64_t rows = pl->rows;
        const int P = pl->P;
        std::vector<uint8_t> cdh((size_t)rows * P);
        std::vector<int32_t> rid((size_t)rows);
        GPV_HIP(hipMemcpy(cdh.data(), pl->d_cond, cdh.size(), hipMemcpyDeviceToHost));
        GPV_HIP(hipMemcpy(rid.data(), pl->d_rowid, rid.size() * 4, hipMemcpyDeviceToHost));
        const bool fuse = !with_fill && !pl->generic && dev_getenv("GPV_POST_NO_FUSE") == nullptr;
        const int32_t *cp_ = colptr.data();
        const uint8_t *cs_ = cslot.data();
        uint8_t *cd_ = cdh.data();
        const int32_t *rid_ = rid.data();
        parallel_for(rows, [=](int64_t b, int64_t e) {
            for (int64_t r = b; r < e; ++r) {
                const int64_t k = rid_[r];
                int n0 = 0;
                for (int j = 0; j < p; ++j) n0 += !is_missing(revNN[k + (int64_t)j * n]);
                uint8_t *row = cd_ + (size_t)r * P;
                for (int t = 0; t < P; ++t) row[t] &= 1u;                     // (a rebuild starts from the flags alone)
                if (!fuse) continue;
                for (int32_t q = cp_[k]; q < cp_[k + 1]; ++q) {
                    const unsigned t = cs_[q];
                    if (t != 0xFFu) row[P - n0 + (int)t] |= (uint8_t)((q - cp_[k] + 1) << 1);
                }
            }
        });
        GPV_HIP(hipMemcpy(pl->d_cond, cdh.data(), cdh.size(), hipMemcpyHostToDevice));
        pl->post_fused = fuse;
    }
    GPV_BUF(pl->d_colptr, upload(colptr.data(), colptr.size()));
    GPV_BUF(pl->d_crow, upload(crow.data(), nnz));
    GPV_BUF(pl->d_cslot, upload(cslot.data(), nnz));
    GPV_BUF(pl->d_colrec, upload(colrec.data(), colrec.size()));
    GPV_BUF(pl->d_rowrec, upload(rowrec.data(), rowrec.size()));
    GPV_BUF(pl->d_rr0, upload(rr0.data(), rr0.size()));
    GPV_BUF(pl->d_tp, upload(tp.data(), tp.size()));
    GPV_BUF(pl->d_ccol, upload(ccol.data(), nnz));
    GPV_BUF(pl->d_cboff, upload(cboff.data(), cboff.size()));
    GPV_BUF(pl->d_cdel, upload(cdel.data(), cdel.size()));
    GPV_BUF(pl->d_C, resize((size_t)c_entries));
    pl->post_nnz = (int64_t)nnz;
    GPV_BUF(pl->d_order2, upload(order2.data(), order2.size()));
    {
        std::vector<int4> meanrec(order2.size());
        for (size_t i = 0; i < order2.size(); ++i) {
            const int32_t k = order2[i];
            meanrec[(size_t)i] = make_int4(k, cboff[(size_t)k], colptr[(size_t)k + 1] - colptr[(size_t)k], colptr[(size_t)k]);
        }
        GPV_BUF(pl->d_meanrec, upload(meanrec.data(), meanrec.size()));
    }
    GPV_BUF(pl->d_levptr2, upload(pl->levptr2.data(), pl->levptr2.size()));
    GPV_HIP(pl->d_toppart.reset());
    if (pl->top_K > 0) GPV_BUF(pl->d_toppart, resize(66 * (size_t)pl->top_K));
    GPV_BUF(pl->d_topinfo, upload(topinfo.data(), topinfo.size()));
    GPV_BUF(pl->d_toprows, upload(toprows.data(), toprows.size()));
    pl->mean_head_levels = 0;
    static const bool no_head = dev_getenv("GPV_NO_MEAN_HEAD") != nullptr;
    while (!no_head && (size_t)pl->mean_head_levels + 1 < pl->levptr2.size() &&
           pl->levptr2[(size_t)pl->mean_head_levels + 1] - pl->levptr2[(size_t)pl->mean_head_levels] <= kMeanHeadMax)
        ++pl->mean_head_levels;
    if (pl->mean_head_levels < 4) pl->mean_head_levels = 0;            // not worth a launch of its own
    GPV_BUF(pl->d_avec_base, ensure((size_t)n + 8));
    pl->d_avec = pl->d_avec_base + 8;                                  // 64 bytes of header in front (SetArgs::aout)
    {
        const unsigned long long hdr[4] = {(unsigned long long)(uintptr_t)pl->d_C.get(), (unsigned long long)(uintptr_t)pl->d_cboff.get(), 0ull, 0ull};
        GPV_HIP(hipMemcpy(pl->d_avec - 4, hdr, sizeof(hdr), hipMemcpyHostToDevice));
    }
    GPV_BUF(pl->d_nug_post, ensure(8));
    GPV_BUF(pl->d_tvec, ensure((size_t)n));
    GPV_BUF(pl->d_rdiag, ensure((size_t)n));
    GPV_BUF(pl->d_u, ensure((size_t)n));
    GPV_BUF(pl->d_mu, ensure((size_t)n));
    GPV_BUF(pl->d_post_part, ensure(2048));                            // launch_sum_pair: 2 x 1024
    if (!pl->post_fused) GPV_BUF(pl->d_L, ensure((size_t)n * pl->P));  // (fused: only when the caller wants U)
    pl->L_of_eval = 0;                                                 // (evaluations from here on may leave d_L alone: fused)
    pl->post_filled = with_fill;
    pl->have_post = true;
    return GPV_OK;
}

int gpv_plan_get_posterior_mean(gpv_plan *pl, double *mu_ord)
{
    if (!pl || !mu_ord) return GPV_ERR_BAD_ARG;
    if (!pl->evaluated || !pl->have_mean) return GPV_ERR_STATE;
    GPV_HIP(hipSetDevice(pl->device));
    GPV_HIP(hipMemcpyAsync(mu_ord, pl->d_mu, sizeof(double) * (size_t)pl->Nlocs, hipMemcpyDeviceToHost, pl->last_stream));
    GPV_HIP(hipStreamSynchronize(pl->last_stream));
    return GPV_OK;
}

// ---- Vecchia-Laplace Newton-Raphson on the device (R/vecchia_laplace_NR.R:31-155) -------------------------------
static int vl_begin_impl(gpv_plan *pl, int model, const double *likparms, const double *z, const double *prior_mean,
                         const double *y_init, bool user_layout)
{
    if (!pl || !z) return GPV_ERR_BAD_ARG;
    if (model < 0 || model > 5) return GPV_ERR_BAD_ARG;
    if (!pl->have_post) return GPV_ERR_STATE;                       // every step is a posterior-mean evaluation
    if (user_layout && !pl->d_user_ord) return GPV_ERR_STATE;
    if (const int rc = enter(pl)) return rc;
    const size_t nb = sizeof(double) * (size_t)pl->Nlocs;
    DevBuf<double> *bufs[] = {&pl->d_vl_z, &pl->d_vl_pm, &pl->d_vl_y[0], &pl->d_vl_y[1], &pl->d_vl_y0, &pl->d_nug_user, &pl->d_zuser};
    for (DevBuf<double> *b : bufs) GPV_BUF(*b, ensure((size_t)pl->Nlocs));
    if (pl->dim > 3) GPV_BUF(pl->d_z, ensure((size_t)pl->Nlocs));
    GPV_BUF(pl->d_vl_out, ensure(4));
    GPV_BUF(pl->d_vl_flags, ensure(1));
    GPV_BUF(pl->d_vl_part, ensure(2048));
    if (!pl->h_vl) {
        GPV_BUF(pl->h_vl, resize(8));
        GPV_HIP(hipHostGetDevicePointer((void **)&pl->h_vl_dev, pl->h_vl, 0));
    }
    {
        bool miss = false;
        for (int64_t i = 0; i < pl->Nlocs && !miss; ++i) miss = (z[i] != z[i]);
        pl->vl_missing = miss;
    }
    hipStream_t st = pl->stream;
    // caller's layout: the vector travels as it is and is gathered into the ordering on the device (x_ord[i] = x[ord[i]-1])
    auto put = [&](const double *src, double *dst) -> int {
        if (!user_layout) {
            GPV_HIP(hipMemcpyAsync(dst, src, nb, hipMemcpyHostToDevice, st));
        } else {
            GPV_HIP(hipMemcpyAsync(pl->d_stage, src, nb, hipMemcpyHostToDevice, st));
            GPV_HIP(launch_reorder(pl->d_stage, pl->d_user_ord, pl->Nlocs, dst, true, nullptr, st));
        }
        return GPV_OK;
    };
    int rc = put(z, pl->d_vl_z);
    if (rc != GPV_OK) return rc;
    if (prior_mean) { if ((rc = put(prior_mean, pl->d_vl_pm)) != GPV_OK) return rc; }
    else GPV_HIP(hipMemsetAsync(pl->d_vl_pm, 0, nb, st));
    // y_init NA -> prior mean (R/vecchia_laplace_NR.R:81-82)
    if (y_init) { if ((rc = put(y_init, pl->d_vl_y0)) != GPV_OK) return rc; }
    else GPV_HIP(hipMemcpyAsync(pl->d_vl_y0, pl->d_vl_pm, nb, hipMemcpyDeviceToDevice, st));
    GPV_HIP(hipMemcpyAsync(pl->d_vl_y[0], pl->d_vl_y0, nb, hipMemcpyDeviceToDevice, st));
    GPV_HIP(hipStreamSynchronize(st));
    pl->vl_model = model;
    pl->vl_alpha = likparms ? likparms[0] : 2.0;
    pl->vl_sigma = likparms ? likparms[1] : std::sqrt(0.1);
    pl->vl_beta = (likparms && model == 4) ? likparms[2] : 0.5;
    pl->vl_cur = 0;
    pl->has_z = true;                                               // the pseudo-data of every step is the plan's data
    return GPV_OK;
}

int gpv_plan_vl_begin(gpv_plan *pl, int model, const double *likparms, const double *z_ord, const double *prior_mean_ord,
                      const double *y_init_ord)
{
    return vl_begin_impl(pl, model, likparms, z_ord, prior_mean_ord, y_init_ord, false);
}

int gpv_plan_set_user_order(gpv_plan *pl, const int *ord_z)
{
    if (!pl || !ord_z) return GPV_ERR_BAD_ARG;
    for (int64_t i = 0; i < pl->Nlocs; ++i)
        if (ord_z[i] < 1 || (int64_t)ord_z[i] > pl->Nlocs) return GPV_ERR_INDEX;
    GPV_HIP(hipSetDevice(pl->device));
    GPV_BUF(pl->d_user_ord, ensure((size_t)pl->Nlocs));
    GPV_HIP(hipMemcpy(pl->d_user_ord, ord_z, sizeof(int32_t) * (size_t)pl->Nlocs, hipMemcpyHostToDevice));
    return GPV_OK;
}

int gpv_plan_vl_begin_user(gpv_plan *pl, int model, const double *likparms, const double *z, const double *prior_mean,
                           const double *y_init)
{
    return vl_begin_impl(pl, model, likparms, z, prior_mean, y_init, true);
}

int gpv_plan_vl_restart(gpv_plan *pl, const double *likparms)
{
    // the same data, prior mean and start value as the last gpv_plan_vl_begin*: nothing crosses PCIe
    if (!pl) return GPV_ERR_BAD_ARG;
    if (pl->vl_model < 0 || !pl->d_vl_y0) return GPV_ERR_STATE;
    if (const int rc = enter(pl)) return rc;
    GPV_HIP(hipMemcpyAsync(pl->d_vl_y[0], pl->d_vl_y0, sizeof(double) * (size_t)pl->Nlocs, hipMemcpyDeviceToDevice, pl->stream));
    if (likparms) {
        pl->vl_alpha = likparms[0];
        pl->vl_sigma = likparms[1];
        if (pl->vl_model == 4) pl->vl_beta = likparms[2];
    }
    pl->vl_cur = 0;
    pl->has_z = true;
    return GPV_OK;
}

// one Newton step in two halves, so that several plans (replicas on several GPUs) can have theirs in flight together
static int vl_step_enqueue(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms);
static int vl_step_finish(gpv_plan *pl, double *dmax, int *flags);

int gpv_plan_vl_step(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, double *dmax, int *flags)
{
    if (!pl || !dmax || !flags) return GPV_ERR_BAD_ARG;
    const int rc = vl_step_enqueue(pl, covType, covparms, ncovparms);
    return rc != GPV_OK ? rc : vl_step_finish(pl, dmax, flags);
}

static int vl_step_enqueue(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms)
{
    if (!pl) return GPV_ERR_BAD_ARG;
    if (pl->vl_model < 0) return GPV_ERR_STATE;
    CovSetup cs;
    const int st0 = cov_setup(covType, covparms, ncovparms, pl->dim, cs);
    if (st0 != GPV_OK) return st0;
    GPV_HIP(hipSetDevice(pl->device));
    hipStream_t st = pl->stream;
    const double *y = pl->d_vl_y[pl->vl_cur];
    double *ynew = pl->d_vl_y[pl->vl_cur ^ 1];
    GPV_HIP(hipMemsetAsync(pl->d_vl_flags, 0, sizeof(int), st));
    pl->L_of_eval = 0;                              // the pseudo-nuggets overwrite the nuggets d_L was computed with
    // pseudo-data and pseudo-nuggets of this step (:93-109) straight into the plan's data / nugget arrays
    double *data_int = pl->dim <= 3 ? pl->d_locs : pl->d_z;
    const int dstr = pl->dim <= 3 ? 4 : 1, doff = pl->dim <= 3 ? 3 : 0;
    GPV_HIP(launch_vl_prepare(pl->vl_model, pl->vl_alpha, pl->vl_sigma, pl->vl_beta, y, pl->d_vl_z, pl->d_vl_pm, pl->Nlocs,
                              pl->d_newpos, data_int, dstr, doff, pl->d_zuser, pl->d_nuggets, pl->d_nug_user, pl->d_vl_flags, st));
    // missing observations (seen when the data were uploaded): what removeNAs of vecchia_prediction puts in their place
    if (pl->vl_missing)
        GPV_HIP(launch_vl_fill_missing(pl->d_vl_z, pl->Nlocs, pl->d_newpos, data_int, dstr, doff, pl->d_zuser, pl->d_nuggets,
                                       pl->d_nug_user, pl->d_vl_part, st));
    // vecchia_prediction(pseudo.data, nuggets = D, return.values = 'meanmat') (:112-113)
    const int rc = plan_eval_checked(pl, cs, nullptr, -1, GPV_WANT_MEAN, st, nullptr);
    if (rc != GPV_OK) return rc;
    // :115-117; the step's two scalars (max |dy| and the flag word) land in pinned host memory: no copy command
    GPV_HIP(launch_vl_update(pl->d_mu, pl->d_vl_pm, y, pl->d_vl_z, ynew, pl->Nlocs, pl->d_post_part, pl->d_vl_out, pl->d_vl_flags,
                             pl->h_vl_dev, st));
    return GPV_OK;
}

static int vl_step_finish(gpv_plan *pl, double *dmax, int *flags)
{
    GPV_HIP(hipSetDevice(pl->device));
    hipStream_t st = pl->stream;
    GPV_HIP(hipStreamSynchronize(st));
    const double h_out = pl->h_vl[0];
    const int h_flags = (int)pl->h_vl[1];
    *dmax = h_out;
    *flags = h_flags;
    if (h_out == h_out) pl->vl_cur ^= 1;          // NaN: the reference keeps y_prev (:117-122)
    return GPV_OK;
}

int gpv_plan_vl_get(gpv_plan *pl, double *mean_ord, double *t_ord, double *D_ord)
{
    // after >= 1 step: preds$mu.obs + prior_mean, pseudo.data + prior_mean and D of the LAST step, ordered layout (:141-144)
    if (!pl) return GPV_ERR_BAD_ARG;
    if (pl->vl_model < 0 || !pl->have_mean) return GPV_ERR_STATE;
    GPV_HIP(hipSetDevice(pl->device));
    const int64_t n = pl->Nlocs;
    const size_t nb = sizeof(double) * (size_t)n;
    std::vector<double> pm;
    if (mean_ord || t_ord) {
        pm.resize((size_t)n);
        GPV_HIP(hipMemcpy(pm.data(), pl->d_vl_pm, nb, hipMemcpyDeviceToHost));
    }
    if (mean_ord) {
        GPV_HIP(hipMemcpy(mean_ord, pl->d_mu, nb, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) mean_ord[i] += pm[(size_t)i];
    }
    if (t_ord) {
        GPV_HIP(hipMemcpy(t_ord, pl->d_zuser, nb, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) t_ord[i] += pm[(size_t)i];
    }
    if (D_ord) GPV_HIP(hipMemcpy(D_ord, pl->d_nug_user, nb, hipMemcpyDeviceToHost));
    return GPV_OK;
}

int gpv_plan_vl_get_user(gpv_plan *pl, double *mean, double *t, double *D)
{
    // the same three vectors in the CALLER's layout (x[ord[i]-1] = x_ord[i], scattered on the device); a missing
    // observation has t = NaN like the reference's pseudo.data (:103-105); D is returned for every location
    if (!pl) return GPV_ERR_BAD_ARG;
    if (pl->vl_model < 0 || !pl->have_mean || !pl->d_user_ord) return GPV_ERR_STATE;
    GPV_HIP(hipSetDevice(pl->device));
    hipStream_t st = pl->stream;
    const size_t nb = sizeof(double) * (size_t)pl->Nlocs;
    double *scratch = pl->d_stage;                                   // [Nlocs]
    if (mean) {
        GPV_HIP(launch_reorder(pl->d_mu, pl->d_user_ord, pl->Nlocs, scratch, false, pl->d_vl_pm, st));
        GPV_HIP(hipMemcpyAsync(mean, scratch, nb, hipMemcpyDeviceToHost, st));
        GPV_HIP(hipStreamSynchronize(st));
    }
    if (t) {
        GPV_HIP(launch_reorder(pl->d_zuser, pl->d_user_ord, pl->Nlocs, scratch, false, pl->d_vl_pm, st));
        GPV_HIP(hipMemcpyAsync(t, scratch, nb, hipMemcpyDeviceToHost, st));
        GPV_HIP(hipStreamSynchronize(st));
    }
    if (D) {
        GPV_HIP(launch_reorder(pl->d_nug_user, pl->d_user_ord, pl->Nlocs, scratch, false, nullptr, st));
        GPV_HIP(hipMemcpyAsync(D, scratch, nb, hipMemcpyDeviceToHost, st));
        GPV_HIP(hipStreamSynchronize(st));
    }
    return GPV_OK;
}

int gpv_plan_vl_loglik(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, double *terms)
{
    // vecchia_laplace_likelihood_from_posterior (R/vecchia_laplace_NR.R:376-409) on the state the last Newton step left in
    // HBM: terms[0] = the pseudo-marginal vecchia_likelihood of the pseudo-data with the pseudo-nuggets (:396-397: one
    // more evaluation of the plan with the posterior pass; for missing observations the resident values are exactly what
    // removeNAs substitutes there), terms[1] = model_llh(mean, z) (:402), terms[2] = the pseudo-conditional term (:405).
    // loglik = terms[0] - terms[2] + terms[1] (:408-409).  Three scalars cross PCIe.
    if (!pl || !terms) return GPV_ERR_BAD_ARG;
    if (pl->vl_model < 0 || !pl->have_mean) return GPV_ERR_STATE;
    CovSetup cs;
    const int st0 = cov_setup(covType, covparms, ncovparms, pl->dim, cs);
    if (st0 != GPV_OK) return st0;
    GPV_HIP(hipSetDevice(pl->device));
    hipStream_t st = pl->stream;
    GPV_HIP(launch_vl_terms(pl->vl_model, pl->vl_alpha, pl->vl_sigma, pl->vl_beta, pl->d_vl_y[pl->vl_cur], pl->d_vl_z, pl->d_vl_pm,
                            pl->d_zuser, pl->d_nug_user, pl->Nlocs, pl->d_vl_part, pl->d_vl_out + 2, st));
    const int rc = plan_eval_checked(pl, cs, nullptr, -1, GPV_WANT_DENOM, st, nullptr);
    if (rc != GPV_OK) return rc;
    double sums[GPV_NSUMS], two[2];
    GPV_HIP(hipMemcpyAsync(two, pl->d_vl_out + 2, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
    const int rc2 = gpv_plan_get_sums(pl, sums);                     // synchronises the stream
    if (rc2 != GPV_OK) return rc2;
    double ll = 0.0;
    gpv_loglik_from_sums(sums, pl->Nlocs, &ll);
    terms[0] = ll;
    terms[1] = two[0];
    terms[2] = two[1];
    return GPV_OK;
}

int gpv_plan_posterior_levels(gpv_plan *pl, int *n_levels)
{
    if (!pl || !n_levels) return GPV_ERR_BAD_ARG;
    if (!pl->have_post) return GPV_ERR_STATE;
    *n_levels = (int)pl->levptr.size() - 1;
    return GPV_OK;
}

int gpv_lincomb_batch(void) { return kLincombNB; }

int gpv_plan_factor_stamp(gpv_plan *pl, int64_t *stamp)
{
    if (!pl || !stamp) return GPV_ERR_BAD_ARG;
    *stamp = (pl->have_post && pl->have_factor) ? pl->factor_stamp : 0;
    return GPV_OK;
}

// psi(x) = d ln Gamma(x) / dx for x > 0 (the C++ library has none): the recurrence psi(x) = psi(x + 1) - 1/x up to x >= 10, then
// seven terms (k = 1..7) of the asymptotic series ln x - 1/(2x) - sum_k B_2k / (2k x^2k).  The truncation error is below the
// first omitted term, |B_16| / 16 / x^16 = 0.4433 / x^16: at most 4.5e-17 for x >= 10 (at x = 6 it would be 1.6e-13, hence 10).
static double gpv_digamma(double x)
{
    double acc = 0.0;
    while (x < 10.0) {
        acc -= 1.0 / x;
        x += 1.0;
    }
    const double r = 1.0 / x, r2 = r * r;
    // B_2k / 2k: 1/12, -1/120, 1/252, -1/240, 1/132, -691/32760, 1/12
    const double ser = r2 * (1.0 / 12.0 - r2 * (1.0 / 120.0 - r2 * (1.0 / 252.0 - r2 * (1.0 / 240.0 - r2 * (1.0 / 132.0
                       - r2 * (691.0 / 32760.0 - r2 * (1.0 / 12.0)))))));
    return acc + std::log(x) - 0.5 * r - ser;
}

static MaternDerivConst matern_deriv_const(double nu)
{
    MaternDerivConst k;
    k.nu = nu;
    k.lnc = (1.0 - nu) * 0.69314718055994530942 - std::lgamma(nu);
    k.lpsi = 0.69314718055994530942 + gpv_digamma(nu);
    return k;
}

// {C / sigma^2, dC/drho / sigma^2, dC/dnu / sigma^2} of the general-nu Matern at s[i] = distance / range, on the host: the
// functions the _nu entries tabulate and fall back to (gpv_bessel.hpp, matern_general_derivs)
int gpv_matern_derivs_host(double nu, double range, const double *s, int64_t n, double *out)
{
    if (n < 0 || (n > 0 && (!s || !out))) return GPV_ERR_BAD_ARG;
    if (!(range > 0.0) || !std::isfinite(range)) return GPV_ERR_BAD_ARG;
    if (!(nu > 0.0 && nu <= 60.0)) return GPV_ERR_UNSUPPORTED_NU;
    const MaternDerivConst k = matern_deriv_const(nu);
    for (int64_t i = 0; i < n; ++i) {
        double f[3];
        matern_general_derivs(s[i], k, 0, f);
        out[3 * i] = f[0];
        out[3 * i + 1] = f[1] / range;
        out[3 * i + 2] = f[2];
    }
    return GPV_OK;
}

// Argument and state checks shared by gpv_plan_loglik_grad and gpv_plan_loglik_fisher (and their _nu forms, with_nu: a general
// smoothness is accepted and differentiated), before the device is touched; on GPV_OK `a` holds everything but the output
// buffers and the tables of a general smoothness, and `cs` the parsed family (matern_scaledim: its inverse ranges, for the scaled
// copy).  rep: the data are the plan's replicates (gpv_plan_set_replicates), not its column.
static int grad_args_checked(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, double nugget, bool with_nu,
                             bool &matern, GradArgs &a, CovSetup &cs, bool rep = false, bool sgv = false)
{
    matern = std::strcmp(covType, "matern") == 0;
    const bool scaled = std::strcmp(covType, "matern_scaledim") == 0;
    if (!matern && !scaled && std::strcmp(covType, "esqe") != 0) return GPV_ERR_COVTYPE;
    // matern_scaledim: variance, up to three ranges and the nugget fill the five parameter slots of the kernels
    if (scaled && pl->dim > 3) return GPV_ERR_STATE;
    if (ncovparms != (matern ? 3 : (scaled ? pl->dim + 2 : 4))) return GPV_ERR_BAD_ARG;
    if (!(nugget > 0.0) || !std::isfinite(nugget)) return GPV_ERR_BAD_ARG;
    const int rc = cov_setup(covType, covparms, ncovparms, pl->dim, cs);
    if (rc != GPV_OK) return rc;
    // (the reference's Matern is discontinuous in nu at the closed forms, and analytic in it everywhere else; the smoothness of
    // matern_scaledim is not differentiated, with_nu or not)
    if (cs.cov == COV_MATERN_GEN && (!with_nu || scaled)) return GPV_ERR_UNSUPPORTED_NU;
    if (pl->p > kGradMaxP) return GPV_ERR_UNSUPPORTED_M;
    if (!(rep ? pl->rep_R > 0 && pl->d_rep_Z : pl->has_z) || pl->comm || pl->rows != pl->Nlocs || pl->d_obs ||
        (pl->latent_nb && !sgv))                                     // (sgv: gpv_plan_loglik_grad_sgv, which is for such plans)
        return GPV_ERR_STATE;
    a.rec = pl->d_locs; a.locs = pl->d_locs; a.z = pl->d_z;
    a.nn = pl->d_nn; a.rowid = pl->d_rowid;
    a.row_terms = nullptr; a.block_part = nullptr; a.totals = nullptr;
    a.rows = pl->rows; a.P = pl->P; a.dim = pl->dim; a.locs_ld = pl->locs_ld; a.cov = cs.cov;
    // irA, irB per family: covparms holds ncovparms entries, 3 for matern_scaledim in one dimension (no covparms[3] there)
    a.sA = cs.sA; a.cA = cs.cA; a.irA = scaled ? cs.inv[0] : 1.0 / covparms[1];
    a.sB = cs.sB; a.cB = cs.cB; a.irB = (matern || scaled) ? 0.0 : 1.0 / covparms[3];
    a.nug = nugget;
    a.gen = MaternDerivConst{0.0, 0.0, 0.0};
    a.gmt = nullptr; a.gmt_base = 0; a.gmt_nseg = 0;
    if (cs.cov == COV_MATERN_GEN) {
        a.sA = covparms[0];                                          // (cov_setup's is the normalised constant of the value path)
        a.gen = matern_deriv_const(covparms[2]);
    }
    if (scaled) {
        // the kernels read the scaled copy, which the entry writes itself (grad_scaled_copy): they pass through no evaluation
        a.cov = cs.cov + kCovScaled05;                               // COV_MATERN05 / 15 / 25 are 0, 1, 2
        a.irB = pl->dim > 1 ? cs.inv[1] : 0.0;                       // irA, irB, sB: 1 / range_1, _2, _3 (0: no such coordinate)
        a.sB = pl->dim > 2 ? cs.inv[2] : 0.0;
        a.cB = 0.0;
    }
    return GPV_OK;
}

// matern_scaledim: the copy of the records with the coordinates divided by the ranges, on `st` in front of the pair passes.  It
// shares d_locs_sc with the evaluations, which rewrite the copy in front of their own kernel; `st` is the plan's stream, so an
// evaluation enqueued earlier on a caller's stream is waited for first.
static int grad_scaled_copy(gpv_plan *pl, const CovSetup &cs, GradArgs &a, hipStream_t st)
{
    if (cs.nscale == 0) return GPV_OK;
    if (pl->last_stream && pl->last_stream != st) GPV_HIP(hipStreamSynchronize(pl->last_stream));
    return eval_scaled_locs(pl, cs, st, a.rec, a.locs);
}

// general smoothness: fit the call's tables over the plan's range of pair distances on `st`, in front of the pair passes (the
// range of matern_table_prepare).  GPV_NO_MATERN_TABLE set, or a plan without distances: no table, every pair takes the
// quadrature.  The calls are blocking, so one buffer serves.
static int grad_gen_table(gpv_plan *pl, GradArgs &a, hipStream_t st)
{
    if (a.cov != COV_MATERN_GEN) return GPV_OK;
    if (getenv("GPV_NO_MATERN_TABLE") != nullptr || !(pl->dist_min > 0.0) || !(pl->dist_max >= pl->dist_min)) return GPV_OK;
    int e_lo = 0, base = 0, nseg = 0;
    if (!matern_dtab_range(0.5 * pl->dist_min * a.cA, 4.0 * pl->dist_max * a.cA, &e_lo, &base, &nseg)) return GPV_OK;
    GPV_BUF(pl->d_gmt, ensure((size_t)MaternDTab::MAX_SEG * MaternDTab::ROW));
    GPV_HIP(launch_matern_dtab(a.gen, e_lo, nseg, pl->d_gmt, st));
    a.gmt = pl->d_gmt; a.gmt_base = base; a.gmt_nseg = nseg;
    return GPV_OK;
}

// Value and gradient of the cond.yz='z' log-likelihood (gpv_grad.hip), with the expected Fisher information of the same
// likelihood (GK_FISHER, the kSetsFisher mode) or the same sums over the plan's replicates (GK_REP, gpv_rep_kernel.hpp; fisher
// may be NULL): the one implementation behind the six entries.  Reads the plan's records and index arrays only and writes
// buffers of its own, so the sums, the U entries and the factor of the plan's last evaluation stay what they were.
enum GradKind { GK_GRAD, GK_FISHER, GK_REP };
static int loglik_family_impl(gpv_plan *pl, GradKind kind, const char *covType, const double *covparms, int ncovparms, double nugget,
                              bool with_nu, double *loglik, double *grad, double *fisher, int64_t *n_failed, double *row_terms)
{
    if (!pl || !covType || !covparms || !loglik || !grad || (kind == GK_FISHER && !fisher) || !n_failed) return GPV_ERR_BAD_ARG;
    bool matern;
    RepArgs ra;
    GradArgs &a = ra.g;
    CovSetup cs;
    int rc = grad_args_checked(pl, covType, covparms, ncovparms, nugget, with_nu, matern, a, cs, kind == GK_REP);
    if (rc != GPV_OK) return rc;
    GPV_HIP(hipSetDevice(pl->device));
    // partials, totals and rows: the gradient's, or the wider ones the information and the replicates share
    const bool info = kind != GK_GRAD;
    const int nv = info ? kFisherNV : kGradNV, ld = info ? kFisherRowLd : kGradRowLd;
    DevBuf<double> &d_part = info ? pl->d_fi_part : pl->d_gr_part, &d_tot = info ? pl->d_fi_tot : pl->d_gr_tot,
                   &d_rows = info ? pl->d_fi_rows : pl->d_gr_rows;
    int &part_grid = info ? pl->fi_grid : pl->gr_grid;
    const int grid = grad_grid(pl->rows, pl->cus);
    if (!d_part || part_grid < grid) {
        GPV_BUF(d_part, resize(nv * (size_t)grid));
        part_grid = grid;
    }
    GPV_BUF(d_tot, ensure(nv));
    if (row_terms) GPV_BUF(d_rows, ensure(ld * (size_t)pl->rows));
    a.row_terms = row_terms ? d_rows.get() : nullptr;
    a.block_part = d_part; a.totals = d_tot;
    hipStream_t st = pl->stream;
    if ((rc = grad_gen_table(pl, a, st)) != GPV_OK) return rc;
    if ((rc = grad_scaled_copy(pl, cs, a, st)) != GPV_OK) return rc;
    ra.Z = pl->d_rep_Z; ra.R = pl->rep_R; ra.RP = pl->rep_RP;
    double tot[kFisherNV];
    GPV_HIP(kind == GK_GRAD ? launch_grad(pl->p, a, grid, st)
                            : (kind == GK_FISHER ? launch_fisher(pl->p, a, grid, st) : launch_rep(pl->p, ra, grid, st)));
    GPV_HIP(hipMemcpyAsync(tot, d_tot, sizeof(double) * nv, hipMemcpyDeviceToHost, st));
    GPV_HIP(hipStreamSynchronize(st));
    // kernel parameters -> covparms: matern {variance, range, -, nugget}, esqe {variance 1, range 1, variance 2, range 2, nugget},
    // matern at a general smoothness {variance, range, smoothness, nugget}; the triangle of the nk kernel parameters -> that of
    // the np = ncovparms + 1 outputs
    // matern_scaledim {variance, range_1 .. range_dim, -, nugget} from the kernels' {variance, three ranges, nugget}: the slots of
    // the coordinates the plan does not have (exact zeros) are dropped (at = -1)
    const bool gen = a.cov == COV_MATERN_GEN, scaled = a.cov >= kCovScaled05;
    const int nk = scaled ? 5 : (gen ? 4 : (matern ? 3 : 5)), np = ncovparms + 1, ntri = np * (np + 1) / 2;
    int at[5] = {0, 1, (matern && !gen) ? 3 : 2, 3, 4};              // output position of kernel parameter t
    if (scaled) {
        for (int t = 0; t < 3; ++t) at[1 + t] = t < pl->dim ? 1 + t : -1;
        at[4] = pl->dim + 2;
    }
    auto spread = [&](const double *src, double *dst) {              // src: {derivatives}, dst: np
        for (int t = 0; t < np; ++t) dst[t] = NAN;
        for (int t = 0; t < nk; ++t)
            if (at[t] >= 0) dst[at[t]] = src[t];
    };
    auto spread_tri = [&](const double *src, double *dst) {          // dst: ntri, row-major with i <= j
        for (int t = 0; t < ntri; ++t) dst[t] = NAN;
        for (int i = 0, s = 0; i < nk; ++i)
            for (int j = i; j < nk; ++j, ++s)
                if (at[i] >= 0 && at[j] >= 0) dst[at[i] * np - at[i] * (at[i] - 1) / 2 + (at[j] - at[i])] = src[s];
    };
    *n_failed = (int64_t)tot[6];
    if (tot[6] > 0.0) {
        *loglik = -INFINITY;
        for (int t = 0; t < np; ++t) grad[t] = NAN;
        for (int t = 0; fisher && t < np * np; ++t) fisher[t] = NAN;
    } else {
        *loglik = tot[0];
        spread(tot + 1, grad);
        if (fisher) {
            double tri[kFisherTri + 6];                              // (np <= 6: matern_scaledim in three dimensions, NaN smoothness row)
            spread_tri(tot + kGradNV, tri);
            for (int i = 0, s = 0; i < np; ++i)                      // mirrored here: exactly symmetric
                for (int j = i; j < np; ++j, ++s) fisher[i * np + j] = fisher[j * np + i] = tri[s];
        }
    }
    if (row_terms) {
        std::vector<double> h((size_t)pl->rows * ld);
        GPV_HIP(hipMemcpy(h.data(), d_rows, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
        const int64_t out_ld = np + 1 + (info ? ntri : 0);
        for (int64_t k = 0; k < pl->rows; ++k) {
            const double *src = &h[(size_t)k * ld];
            row_terms[k * out_ld] = src[0];
            spread(src + 1, row_terms + k * out_ld + 1);
            if (info) spread_tri(src + kGradRowLd, row_terms + k * out_ld + 1 + np);
        }
    }
    return GPV_OK;
}

int gpv_plan_loglik_grad(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, double nugget, double *loglik,
                         double *grad, int64_t *n_failed, double *row_terms)
{
    return loglik_family_impl(pl, GK_GRAD, covType, covparms, ncovparms, nugget, false, loglik, grad, nullptr, n_failed, row_terms);
}

// the same, with the smoothness of "matern" differentiated wherever the function is differentiable in it
int gpv_plan_loglik_grad_nu(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, double nugget, double *loglik,
                            double *grad, int64_t *n_failed, double *row_terms)
{
    return loglik_family_impl(pl, GK_GRAD, covType, covparms, ncovparms, nugget, true, loglik, grad, nullptr, n_failed, row_terms);
}

int gpv_plan_loglik_fisher(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, double nugget, double *loglik,
                           double *grad, double *fisher, int64_t *n_failed, double *row_terms)
{
    return loglik_family_impl(pl, GK_FISHER, covType, covparms, ncovparms, nugget, false, loglik, grad, fisher, n_failed, row_terms);
}

int gpv_plan_loglik_fisher_nu(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, double nugget, double *loglik,
                              double *grad, double *fisher, int64_t *n_failed, double *row_terms)
{
    return loglik_family_impl(pl, GK_FISHER, covType, covparms, ncovparms, nugget, true, loglik, grad, fisher, n_failed, row_terms);
}

// ---- replicated data: R realisations over the plan's locations, one pass for their summed value, gradient and information ---
// Uploads the columns (the staging buffer lives for the call only) and packs them by internal position.  Touches nothing of the
// plan but d_rep_Z: the data column, the last evaluation and the factor stamp stay what they were.
int gpv_plan_set_replicates(gpv_plan *pl, const double *Z_ord, int64_t ldz, int R)
{
    if (!pl || R < 0 || (R > 0 && (!Z_ord || ldz < pl->Nlocs))) return GPV_ERR_BAD_ARG;
    const int64_t n = pl->Nlocs;
    if (R > 0 && (n < 1 || !pl->d_newpos)) return GPV_ERR_STATE;
    GPV_HIP(hipSetDevice(pl->device));
    hipStream_t st = pl->stream;
    pl->rep_R = pl->rep_RP = 0;
    if (R == 0) {
        GPV_BUF(pl->d_rep_Z, reset());
        return GPV_OK;
    }
    const int rp = rep_rp(R);
    DevBuf<double> d_in;
    GPV_BUF(d_in, resize((size_t)n * R));
    GPV_BUF(pl->d_rep_Z, resize((size_t)n * rp));
    if (cols_to_device(d_in, Z_ord, ldz, n, R, st)) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(launch_rep_pack(d_in, pl->d_newpos, n, R, rp, pl->d_rep_Z, st))) return drain_fail(st, GPV_ERR_HIP);
    GPV_HIP(hipStreamSynchronize(st));
    pl->rep_R = R; pl->rep_RP = rp;
    return GPV_OK;
}

int gpv_plan_replicates(gpv_plan *pl, int *R)
{
    if (!pl || !R) return GPV_ERR_BAD_ARG;
    *R = pl->rep_R;
    return GPV_OK;
}

int gpv_plan_loglik_rep(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, double nugget, double *loglik,
                        double *grad, double *fisher, int64_t *n_failed, double *row_terms)
{
    return loglik_family_impl(pl, GK_REP, covType, covparms, ncovparms, nugget, false, loglik, grad, fisher, n_failed, row_terms);
}

int gpv_plan_loglik_rep_nu(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, double nugget, double *loglik,
                           double *grad, double *fisher, int64_t *n_failed, double *row_terms)
{
    return loglik_family_impl(pl, GK_REP, covType, covparms, ncovparms, nugget, true, loglik, grad, fisher, n_failed, row_terms);
}

// ---- the whitening operator of the plan's latest evaluation applied to a block of columns (gpv_whiten.hip) -----------------
int gpv_whiten_max_cols(void) { return kWhitenMaxCols; }

// the two passes on what is resident: d_wh_B -> d_wh_E, partials, totals
static hipError_t whiten_enqueue(gpv_plan *pl, int cp, hipStream_t st)
{
    WhitenArgs a;
    factor_view(pl, a);
    a.B = pl->d_wh_B; a.E = pl->d_wh_E; a.part = pl->d_wh_wpart;
    a.rows = pl->rows; a.P = pl->P;
    const hipError_t e = launch_whiten(a, cp, pl->wh_wgrid, st);
    if (e != hipSuccess) return e;
    return launch_whiten_gram(pl->d_wh_E, pl->rows, cp, pl->wh_ggrid, pl->d_wh_gpart, pl->d_wh_wpart, pl->wh_wgrid, pl->d_wh_tot, st);
}

// Reads d_L, the index arrays and the nuggets of the plan's latest evaluation and writes buffers of its own, so the sums, the U
// entries, the posterior state and the factor stamp stay what they were.
int gpv_plan_whiten(gpv_plan *pl, const double *B_ord, int64_t ldb, int ncols, double *E_ord, int64_t lde, double *gram,
                    double *logdet, int64_t *n_failed)
{
    if (!pl || !B_ord || !gram || !logdet || !n_failed) return GPV_ERR_BAD_ARG;
    if (ncols < 1 || ncols > kWhitenMaxCols) return GPV_ERR_BAD_ARG;
    const int64_t n = pl->Nlocs;
    if (ldb < n || (E_ord && lde < n)) return GPV_ERR_BAD_ARG;
    if (const int rc = factor_state(pl)) return rc;
    if (const int rc = enter(pl)) return rc;
    hipStream_t st = pl->stream;
    const int cp = whiten_cp(ncols);
    if (cp > pl->wh_cp_cap) {
        pl->wh_cp_cap = 0;
        GPV_BUF(pl->d_wh_in, resize((size_t)n * cp));
        GPV_BUF(pl->d_wh_B, resize((size_t)n * cp));
        GPV_BUF(pl->d_wh_E, resize((size_t)n * cp));
        pl->wh_cp_cap = cp;
    }
    if (!pl->d_wh_tot) {
        pl->wh_wgrid = whiten_grid(pl->rows, pl->cus);
        pl->wh_ggrid = whiten_gram_grid(pl->rows, pl->cus);
        GPV_BUF(pl->d_wh_wpart, resize((size_t)pl->wh_wgrid * kWhitenNV));
        GPV_BUF(pl->d_wh_gpart, resize((size_t)pl->wh_ggrid * kGramTile));
        GPV_BUF(pl->d_wh_tot, resize(kWhitenTotals));
    }
    if (cols_to_device(pl->d_wh_in, B_ord, ldb, n, ncols, st)) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(launch_whiten_pack(pl->d_wh_in, pl->d_newpos, n, ncols, cp, pl->d_wh_B, st))) return drain_fail(st, GPV_ERR_HIP);
    pl->wh_cp_last = cp;
    if (GPV_HIP_FAILED(whiten_enqueue(pl, cp, st))) return drain_fail(st, GPV_ERR_HIP);
    double tot[kWhitenTotals];
    if (GPV_HIP_FAILED(hipMemcpyAsync(tot, pl->d_wh_tot, sizeof(tot), hipMemcpyDeviceToHost, st))) return drain_fail(st, GPV_ERR_HIP);
    if (E_ord) {
        if (GPV_HIP_FAILED(launch_whiten_unpack(pl->d_wh_E, n, ncols, cp, pl->d_wh_in, st))) return drain_fail(st, GPV_ERR_HIP);
        if (cols_to_host(E_ord, lde, pl->d_wh_in, n, ncols, st)) return drain_fail(st, GPV_ERR_HIP);
    }
    GPV_HIP(hipStreamSynchronize(st));
    const bool bad = tot[kGramTile + 1] > 0.0;
    *n_failed = (int64_t)tot[kGramTile + 1];
    *logdet = bad ? NAN : tot[kGramTile];
    for (int i = 0; i < ncols; ++i)
        for (int j = 0; j < ncols; ++j) gram[i * ncols + j] = bad ? NAN : tot[i * kWhitenMaxCols + j];
    return GPV_OK;
}

// developer aid (tools/whiten_timing.py; not part of the public header): device time of `reps` runs of the two passes (whitening,
// Gram with its sum) over the columns the latest gpv_plan_whiten left on the device, by a pair of events around them alone: no
// copies, no packing
extern "C" int gpv_plan_debug_whiten_ms(gpv_plan *pl, int reps, double *ms)
{
    if (!pl || reps <= 0 || !ms) return GPV_ERR_BAD_ARG;
    if (!factor_current(pl) || pl->wh_cp_last == 0 || !pl->d_wh_tot) return GPV_ERR_STATE;   // (d_L lives as long as the plan)
    return timed_reps(pl, true, reps, ms, [&] { return whiten_enqueue(pl, pl->wh_cp_last, pl->stream); });
}

// ---- the colouring operator, the inverse of the whitening operator: simulation from the Vecchia model (gpv_unwhiten.hip) ----
int gpv_unwhiten_narrow(void) { return kUnwhitenNarrow; }

// The level schedule from the plan's own index arrays, read back once: level(k) = 0 for a row without neighbours, else
// 1 + max_j level(j), taken in the ordered row sequence (every neighbour precedes its row); the stored sets sorted by level,
// ascending (the plan's Morton order) inside a level; maximal runs of consecutive narrow levels become one launch each.
static int unwhiten_schedule(gpv_plan *pl)
{
    if (pl->uw_sched) return GPV_OK;
    const int64_t rows = pl->rows, n = pl->Nlocs;
    const int P = pl->P;
    std::vector<int32_t> nn((size_t)rows * P), rowid((size_t)rows);
    GPV_HIP(hipMemcpy(nn.data(), pl->d_nn, nn.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(rowid.data(), pl->d_rowid, rowid.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    // lev_pos: level of the row that wrote a position last (-1: none yet); touch: highest level of a row that has read or
    // written it.  In a plan whose rows end in distinct points that their neighbours' rows precede, touch of a row's own point
    // is still -1 when the row comes, and the level is the definition's.  Rows that share their last entry (the ordered
    // nearest-neighbour search can name a coincident earlier point as a row's last entry) are kept in the ordered row
    // sequence: such a row goes to a later level than every row that has read or written the point before it.
    std::vector<int32_t> set_of_row((size_t)rows, -1), lev_pos((size_t)n, -1), touch((size_t)n, -1), lev_set((size_t)rows, 0);
    for (int64_t s = 0; s < rows; ++s) {
        if (rowid[(size_t)s] < 0 || rowid[(size_t)s] >= rows) return GPV_ERR_STATE;
        set_of_row[(size_t)rowid[(size_t)s]] = (int32_t)s;
    }
    int32_t top = 0;
    for (int64_t k = 0; k < rows; ++k) {
        const int32_t s = set_of_row[(size_t)k];
        if (s < 0) return GPV_ERR_STATE;
        const int32_t *nr = &nn[(size_t)s * P];
        const int32_t own = nr[P - 1];
        if (own >= n) return GPV_ERR_STATE;
        int32_t lv = own >= 0 ? touch[(size_t)own] + 1 : 0;
        for (int q = 0; q < P - 1; ++q) {
            if (nr[q] < 0) continue;
            if (nr[q] >= n) return GPV_ERR_STATE;
            const int32_t l = lev_pos[(size_t)nr[q]] + 1;          // (a position no earlier row owns counts as level -1)
            lv = l > lv ? l : lv;
        }
        for (int q = 0; q < P - 1; ++q)
            if (nr[q] >= 0 && touch[(size_t)nr[q]] < lv) touch[(size_t)nr[q]] = lv;
        lev_set[(size_t)s] = lv;
        if (own >= 0) lev_pos[(size_t)own] = touch[(size_t)own] = lv;
        top = lv > top ? lv : top;
    }
    pl->uw_holes = false;                                          // positions that no row owns: kept at zero (unwhiten_sweep)
    for (int64_t i = 0; i < n; ++i) pl->uw_holes = pl->uw_holes || lev_pos[(size_t)i] < 0;
    const int nlev = top + 1;
    std::vector<int32_t> levptr((size_t)nlev + 1, 0), order((size_t)rows);
    for (int64_t s = 0; s < rows; ++s) levptr[(size_t)lev_set[(size_t)s] + 1]++;
    for (int l = 0; l < nlev; ++l) levptr[(size_t)l + 1] += levptr[(size_t)l];
    {
        std::vector<int32_t> fill(levptr.begin(), levptr.end() - 1);
        for (int64_t s = 0; s < rows; ++s) order[(size_t)fill[(size_t)lev_set[(size_t)s]]++] = (int32_t)s;
    }
    std::vector<gpv_plan::UwLaunch> launches;
    for (int l = 0; l < nlev; ++l) {
        const bool narrow = levptr[(size_t)l + 1] - levptr[(size_t)l] <= kUnwhitenNarrow;
        if (narrow && !launches.empty() && launches.back().narrow) launches.back().lev1 = l + 1;
        else launches.push_back(gpv_plan::UwLaunch{l, l + 1, narrow});
    }
    GPV_BUF(pl->d_uw_order, upload(order.data(), order.size()));
    GPV_BUF(pl->d_uw_levptr, upload(levptr.data(), levptr.size()));
    GPV_BUF(pl->d_uw_nfail, resize(2));
    pl->uw_levptr.swap(levptr);
    pl->uw_launches.swap(launches);
    pl->uw_sched = true;
    return GPV_OK;
}

int gpv_plan_unwhiten_levels(gpv_plan *pl, int64_t *n_levels, int64_t *n_launches)
{
    if (!pl || !n_levels || !n_launches) return GPV_ERR_BAD_ARG;
    if (const int rc = z_structure(pl)) return rc;             // (the schedule needs no evaluation)
    GPV_HIP(hipSetDevice(pl->device));
    if (const int rc = unwhiten_schedule(pl)) return rc;
    *n_levels = (int64_t)pl->uw_levptr.size() - 1;
    *n_launches = (int64_t)pl->uw_launches.size();
    return GPV_OK;
}

// the sweep on what is resident: d_uw_E -> d_uw_B, level by level
static hipError_t unwhiten_enqueue(gpv_plan *pl, int cp, hipStream_t st)
{
    UnwhitenArgs a;
    factor_view(pl, a);
    a.E = pl->d_uw_E; a.B = pl->d_uw_B; a.order = pl->d_uw_order; a.levptr = pl->d_uw_levptr; a.nfail = pl->d_uw_nfail;
    a.P = pl->P;
    for (const gpv_plan::UwLaunch &u : pl->uw_launches) {
        const hipError_t e = u.narrow ? launch_unwhiten_narrow(a, cp, u.lev0, u.lev1, st)
                                      : launch_unwhiten_wide(a, cp, pl->uw_levptr[(size_t)u.lev0], pl->uw_levptr[(size_t)u.lev1], st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the counter cleared, then the sweep: replayed from one captured linear graph per padded column count, captured again when
// another evaluation has left its factor (the launches carry d_L, the nuggets' address and the constant nugget by value)
static hipError_t unwhiten_sweep(gpv_plan *pl, int cp, hipStream_t st)
{
    int gi = 0;
    while ((1 << gi) < cp) ++gi;
    hipError_t e = hipMemsetAsync(pl->d_uw_nfail, 0, sizeof(unsigned), st);
    if (e != hipSuccess) return e;
    if (pl->uw_holes) {                                // some position belongs to no row: what a row reads there is zero, every call
        e = hipMemsetAsync(pl->d_uw_B, 0, sizeof(double) * (size_t)pl->Nlocs * cp, st);
        if (e != hipSuccess) return e;
    }
    const bool stale = pl->uw_graph_eval[gi] != pl->eval_count;
    pl->uw_graph_eval[gi] = pl->eval_count;
    return graph_replay(pl->uw_graph[gi], st, [&] { return unwhiten_enqueue(pl, cp, st); }, stale);
}

// device, schedule and the column buffers at the padded column count cp
static int unwhiten_prepare(gpv_plan *pl, int cp)
{
    if (const int rc = enter(pl)) return rc;
    if (const int rc = unwhiten_schedule(pl)) return rc;
    if (cp > pl->uw_cp_cap) {
        const size_t cnt = (size_t)pl->Nlocs * cp;
        pl->uw_cp_cap = 0;
        for (auto &g : pl->uw_graph) g.reset();                   // they hold the buffers' addresses
        GPV_BUF(pl->d_uw_in, resize(cnt));
        GPV_BUF(pl->d_uw_E, resize(cnt));
        GPV_BUF(pl->d_uw_B, resize(cnt));
        pl->uw_cp_cap = cp;
    }
    return GPV_OK;
}

// Reads d_L, the index arrays and the nuggets of the plan's latest evaluation and writes buffers of its own, so the sums, the U
// entries, the posterior state, the factor stamp and what gpv_plan_whiten left on the device stay what they were.
int gpv_plan_unwhiten(gpv_plan *pl, const double *E_ord, int64_t lde, int ncols, double *B_ord, int64_t ldb, int64_t *n_failed)
{
    if (!pl || !E_ord || !B_ord || !n_failed) return GPV_ERR_BAD_ARG;
    if (ncols < 1 || ncols > kUnwhitenMaxCols) return GPV_ERR_BAD_ARG;
    const int64_t n = pl->Nlocs;
    if (lde < n || ldb < n) return GPV_ERR_BAD_ARG;
    if (const int rc = factor_state(pl)) return rc;
    const int cp = whiten_cp(ncols);
    if (const int rc = unwhiten_prepare(pl, cp)) return rc;
    hipStream_t st = pl->stream;
    if (cols_to_device(pl->d_uw_in, E_ord, lde, n, ncols, st)) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(launch_unwhiten_pack(pl->d_uw_in, n, ncols, cp, pl->d_uw_E, st))) return drain_fail(st, GPV_ERR_HIP);
    pl->uw_cp_last = cp;
    if (GPV_HIP_FAILED(unwhiten_sweep(pl, cp, st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(launch_unwhiten_unpack(pl->d_uw_B, pl->d_newpos, n, ncols, cp, pl->d_uw_in, st))) return drain_fail(st, GPV_ERR_HIP);
    unsigned nf = 0;
    if (GPV_HIP_FAILED(hipMemcpyAsync(&nf, pl->d_uw_nfail, sizeof(nf), hipMemcpyDeviceToHost, st))) return drain_fail(st, GPV_ERR_HIP);
    if (cols_to_host(B_ord, ldb, pl->d_uw_in, n, ncols, st)) return drain_fail(st, GPV_ERR_HIP);   // (B_ord may be E_ord: read before)
    GPV_HIP(hipStreamSynchronize(st));
    *n_failed = (int64_t)nf;
    if (nf > 0) cols_fill_nan(B_ord, ldb, n, ncols);                              // the recursion hands a failed row's NaN on: no entry is trusted
    return GPV_OK;
}

// Draw j is always made in the batch of the 16 draws [16 floor(j / 16), + 16) at the padded column count 16, whatever col0 and
// ncols are: a column's bits depend on (seed, j) and the evaluation alone.
int gpv_plan_simulate(gpv_plan *pl, uint64_t seed, int64_t col0, int64_t ncols, double *Z_ord, int64_t ldz, int64_t *n_failed)
{
    constexpr int NB = kUnwhitenMaxCols;
    if (!pl || !Z_ord || !n_failed || col0 < 0 || ncols < 1) return GPV_ERR_BAD_ARG;
    const int64_t n = pl->Nlocs;
    if (ldz < n || col0 > INT64_MAX - ncols) return GPV_ERR_BAD_ARG;
    if (const int rc = factor_state(pl)) return rc;
    if (const int rc = unwhiten_prepare(pl, NB)) return rc;
    hipStream_t st = pl->stream;
    const int64_t end = col0 + ncols;
    unsigned nf = 0;
    pl->uw_cp_last = NB;
    for (int64_t b = col0 / NB; b * NB < end; ++b) {
        const int64_t base = b * NB;
        if (GPV_HIP_FAILED(launch_unwhiten_normals(pl->d_uw_E, n, seed, base, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(unwhiten_sweep(pl, NB, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(launch_unwhiten_unpack(pl->d_uw_B, pl->d_newpos, n, NB, NB, pl->d_uw_in, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipMemcpyAsync(&nf, pl->d_uw_nfail, sizeof(nf), hipMemcpyDeviceToHost, st))) return drain_fail(st, GPV_ERR_HIP);
        const int64_t j0 = std::max(base, col0), j1 = std::min(base + NB, end);        // the batch's share of the call's columns
        if (cols_to_host(Z_ord + (j0 - col0) * ldz, ldz, pl->d_uw_in + (size_t)(j0 - base) * n, n, j1 - j0, st))
            return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
    }
    *n_failed = (int64_t)nf;
    if (nf > 0) cols_fill_nan(Z_ord, ldz, n, ncols);
    return GPV_OK;
}

// developer aid (tools/unwhiten_timing.py; not part of the public header): device time of `reps` sweeps over the columns the
// latest gpv_plan_unwhiten / gpv_plan_simulate left on the device, by a pair of events around the sweep alone: no copies, no
// packing
extern "C" int gpv_plan_debug_unwhiten_ms(gpv_plan *pl, int reps, double *ms)
{
    if (!pl || reps <= 0 || !ms) return GPV_ERR_BAD_ARG;
    if (const int rc = factor_state(pl)) return rc;
    if (pl->uw_cp_last == 0 || !pl->uw_sched) return GPV_ERR_STATE;
    return timed_reps(pl, true, reps, ms, [&] { return unwhiten_sweep(pl, pl->uw_cp_last, pl->stream); });
}

// ---- the transposed whitening operator: precision products and leave-one-out cross-validation (gpv_loo.hip) ----------------
int gpv_loo_nscores(void) { return kLooNScores; }

int gpv_loo_index_host(const int32_t *nn, const int32_t *rowid, int64_t rows, int64_t Nlocs, int P, int32_t *colptr, int32_t *owner,
                       int32_t *col, int64_t col_cap, int64_t *nnz)
{
    if (!nnz || rows < 0 || Nlocs < 0 || P < 1) return GPV_ERR_BAD_ARG;
    if (rows * (int64_t)P >= ((int64_t)1 << 31) || Nlocs >= ((int64_t)1 << 31) - 1) return GPV_ERR_INDEX;      // before any array is read
    if (!nn || !rowid || !colptr || !owner) return GPV_ERR_BAD_ARG;
    std::vector<int32_t> cptr, own, cl;
    const int rc = loo_build_index(nn, rowid, rows, Nlocs, P, cptr, own, cl);
    if (rc != 0) return rc == 1 ? GPV_ERR_INDEX : GPV_ERR_BAD_ARG;
    *nnz = (int64_t)cl.size();
    std::copy(cptr.begin(), cptr.end(), colptr);
    std::copy(own.begin(), own.end(), owner);
    if (col) {
        if (col_cap < *nnz) return GPV_ERR_BAD_ARG;
        std::copy(cl.begin(), cl.end(), col);
    }
    return GPV_OK;
}

// z_structure() and the index's own limit / factor_state() and that limit, after every state error
static int loo_structure(const gpv_plan *pl)
{
    if (const int rc = z_structure(pl)) return rc;
    if ((int64_t)pl->rows * pl->P >= ((int64_t)1 << 31)) return GPV_ERR_INDEX;     // the flat offsets of the index are int32
    return GPV_OK;
}
static int loo_state(const gpv_plan *pl)
{
    if (const int rc = factor_state(pl)) return rc;
    return loo_structure(pl);
}

// The transposed index from the plan's own index arrays, read back once (the structure does not depend on the parameters).
static int loo_index(gpv_plan *pl)
{
    if (pl->loo_have_index) return GPV_OK;
    const int64_t rows = pl->rows, n = pl->Nlocs;
    const int P = pl->P;
    std::vector<int32_t> nn((size_t)rows * P), rowid((size_t)rows), colptr, owner, col;
    GPV_HIP(hipMemcpy(nn.data(), pl->d_nn, nn.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(rowid.data(), pl->d_rowid, rowid.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int rc = loo_build_index(nn.data(), rowid.data(), rows, n, P, colptr, owner, col);
    if (rc != 0) return rc == 1 ? GPV_ERR_INDEX : GPV_ERR_STATE;
    int64_t maxcol = 0, empty = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = colptr[(size_t)i + 1] - colptr[(size_t)i];
        maxcol = std::max(maxcol, len);
        empty += len == 0;
    }
    GPV_BUF(pl->d_loo_colptr, upload(colptr.data(), colptr.size()));
    GPV_BUF(pl->d_loo_owner, upload(owner.data(), owner.size()));
    GPV_BUF(pl->d_loo_col, upload(col.data(), col.size()));
    GPV_BUF(pl->d_loo_g, resize((size_t)rows));
    GPV_BUF(pl->d_loo_nfail, resize(2));
    GPV_BUF(pl->d_loo_q, resize((size_t)n));
    GPV_BUF(pl->d_loo_qord, resize((size_t)n));
    GPV_BUF(pl->d_loo_var, resize((size_t)n));
    pl->loo_grid = loo_grid(rows, pl->cus);
    pl->loo_sgrid = loo_score_grid(n, pl->cus);
    GPV_BUF(pl->d_loo_part, resize((size_t)kLooMaxCols * pl->loo_sgrid * kLooNScores));
    GPV_BUF(pl->d_loo_scores, resize((size_t)kLooMaxCols * kLooNScores));
    pl->loo_nnz = (int64_t)col.size();
    pl->loo_maxcol = maxcol;
    pl->loo_empty = empty;
    pl->loo_g_eval = 0;
    pl->loo_have_index = true;
    return GPV_OK;
}

int gpv_plan_loo_index(gpv_plan *pl, int64_t *n_entries, int64_t *max_column, int64_t *n_empty)
{
    if (!pl || !n_entries || !max_column || !n_empty) return GPV_ERR_BAD_ARG;
    if (const int rc = loo_structure(pl)) return rc;
    GPV_HIP(hipSetDevice(pl->device));
    if (const int rc = loo_index(pl)) return rc;
    *n_entries = pl->loo_nnz;
    *max_column = pl->loo_maxcol;
    *n_empty = pl->loo_empty;
    return GPV_OK;
}

enum { kLooModeT = 0, kLooModeQ = 1, kLooModeCV = 2 };

static LooArgs loo_args(gpv_plan *pl)
{
    LooArgs a;
    factor_view(pl, a);
    a.colptr = pl->d_loo_colptr; a.owner = pl->d_loo_owner; a.col = pl->d_loo_col;
    a.g = pl->d_loo_g; a.nfail = pl->d_loo_nfail;
    a.B = pl->d_loo_B; a.E = pl->d_loo_E; a.R = pl->d_loo_R; a.q = pl->d_loo_q;
    a.rows = pl->rows; a.n = pl->Nlocs; a.P = pl->P;
    a.pmagic = loo_pmagic(pl->P);
    return a;
}

// the device passes of one call on what is resident: d_loo_in -> d_loo_out (and d_loo_qord, d_loo_var, d_loo_scores)
static hipError_t loo_enqueue(gpv_plan *pl, int mode, int ncols, bool want_q, hipStream_t st)
{
    const int cp = whiten_cp(ncols);
    const int64_t n = pl->Nlocs;
    const LooArgs a = loo_args(pl);
    hipError_t e;
    if (mode == kLooModeT) {
        if ((e = launch_loo_pack(pl->d_loo_in, nullptr, n, ncols, cp, pl->d_loo_E, st)) != hipSuccess) return e;
    } else {
        if ((e = launch_loo_pack(pl->d_loo_in, pl->d_newpos, n, ncols, cp, pl->d_loo_B, st)) != hipSuccess) return e;
        if ((e = launch_loo_forward(a, cp, pl->loo_grid, st)) != hipSuccess) return e;
    }
    if ((e = launch_loo_transposed(a, cp, pl->loo_grid, st)) != hipSuccess) return e;
    if ((e = launch_loo_unpack(pl->d_loo_R, pl->d_newpos, n, ncols, cp, pl->d_loo_out, st)) != hipSuccess) return e;
    if (want_q || mode == kLooModeCV)
        if ((e = launch_loo_unpack(pl->d_loo_q, pl->d_newpos, n, 1, 1, pl->d_loo_qord, st)) != hipSuccess) return e;
    if (mode == kLooModeCV)
        return launch_loo_scores(pl->d_loo_in, pl->d_loo_out, pl->d_loo_qord, pl->d_loo_var, n, ncols, pl->loo_sgrid, pl->d_loo_part,
                                 pl->d_loo_scores, st);
    return hipSuccess;
}

// the scale pre-pass: once per evaluation (needs loo_index)
static int loo_scale_once(gpv_plan *pl, hipStream_t st)
{
    if (pl->loo_g_eval == pl->eval_count) return GPV_OK;
    pl->loo_g_eval = 0;
    if (GPV_HIP_FAILED(hipMemsetAsync(pl->d_loo_nfail, 0, sizeof(unsigned), st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(launch_loo_scale(loo_args(pl), pl->loo_grid, st))) return drain_fail(st, GPV_ERR_HIP);
    unsigned nf = 0;
    if (GPV_HIP_FAILED(hipMemcpyAsync(&nf, pl->d_loo_nfail, sizeof(nf), hipMemcpyDeviceToHost, st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return GPV_ERR_HIP;
    pl->loo_nfail = nf;
    pl->loo_g_eval = pl->eval_count;
    return GPV_OK;
}

// Reads d_L, the index arrays and the nuggets of the plan's latest evaluation and writes buffers of its own, so the sums, the U
// entries, the posterior state, the factor stamp and what gpv_plan_whiten left on the device stay what they were.
//   in / out: ncols columns; vec: qdiag (kLooModeQ) or var (kLooModeCV), NULL = not wanted; out may be NULL in kLooModeCV
static int loo_run(gpv_plan *pl, int mode, const double *in, int64_t ldin, int ncols, double *out, int64_t ldout, double *vec,
                   double *scores, int64_t *n_failed)
{
    if (const int rc = loo_state(pl)) return rc;
    const int64_t n = pl->Nlocs;
    if (const int rc = enter(pl)) return rc;
    hipStream_t st = pl->stream;
    if (const int rc = loo_index(pl)) return rc;
    const int cp = whiten_cp(ncols);
    if (cp > pl->loo_cp_cap) {
        const size_t cnt = (size_t)n * cp;
        pl->loo_cp_cap = 0;
        GPV_BUF(pl->d_loo_in, resize(cnt));
        GPV_BUF(pl->d_loo_out, resize(cnt));
        GPV_BUF(pl->d_loo_B, resize(cnt));
        GPV_BUF(pl->d_loo_E, resize(cnt));
        GPV_BUF(pl->d_loo_R, resize(cnt));
        pl->loo_cp_cap = cp;
    }
    if (const int rc = loo_scale_once(pl, st)) return rc;
    if (cols_to_device(pl->d_loo_in, in, ldin, n, ncols, st)) return drain_fail(st, GPV_ERR_HIP);
    pl->loo_last_mode = mode;
    pl->loo_last_ncols = ncols;
    if (GPV_HIP_FAILED(loo_enqueue(pl, mode, ncols, vec != nullptr, st))) return drain_fail(st, GPV_ERR_HIP);
    double sc[kLooMaxCols * kLooNScores];
    if (mode == kLooModeCV &&
        GPV_HIP_FAILED(hipMemcpyAsync(sc, pl->d_loo_scores, sizeof(double) * (size_t)ncols * kLooNScores, hipMemcpyDeviceToHost, st)))
        return drain_fail(st, GPV_ERR_HIP);
    if (out && cols_to_host(out, ldout, pl->d_loo_out, n, ncols, st)) return drain_fail(st, GPV_ERR_HIP);   // (out may be in: read before)
    if (vec && GPV_HIP_FAILED(hipMemcpyAsync(vec, mode == kLooModeCV ? pl->d_loo_var.get() : pl->d_loo_qord.get(),
                                             sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st)))
        return drain_fail(st, GPV_ERR_HIP);
    GPV_HIP(hipStreamSynchronize(st));
    const bool bad = pl->loo_nfail > 0;
    *n_failed = (int64_t)pl->loo_nfail;
    if (scores)
        for (int t = 0; t < ncols * kLooNScores; ++t) scores[t] = bad ? (double)NAN : sc[t];
    if (bad) {                                         // a failed row's NaN reaches every location that names it: no entry is trusted
        if (out) cols_fill_nan(out, ldout, n, ncols);
        if (vec) std::fill_n(vec, (size_t)n, (double)NAN);
    }
    return GPV_OK;
}

int gpv_plan_whiten_t(gpv_plan *pl, const double *E_ord, int64_t lde, int ncols, double *B_ord, int64_t ldb, int64_t *n_failed)
{
    if (!pl || !E_ord || !B_ord || !n_failed) return GPV_ERR_BAD_ARG;
    if (ncols < 1 || ncols > kLooMaxCols) return GPV_ERR_BAD_ARG;
    if (lde < pl->Nlocs || ldb < pl->Nlocs) return GPV_ERR_BAD_ARG;
    return loo_run(pl, kLooModeT, E_ord, lde, ncols, B_ord, ldb, nullptr, nullptr, n_failed);
}

int gpv_plan_precision(gpv_plan *pl, const double *B_ord, int64_t ldb, int ncols, double *R_ord, int64_t ldr, double *qdiag,
                       int64_t *n_failed)
{
    if (!pl || !B_ord || !R_ord || !n_failed) return GPV_ERR_BAD_ARG;
    if (ncols < 1 || ncols > kLooMaxCols) return GPV_ERR_BAD_ARG;
    if (ldb < pl->Nlocs || ldr < pl->Nlocs) return GPV_ERR_BAD_ARG;
    return loo_run(pl, kLooModeQ, B_ord, ldb, ncols, R_ord, ldr, qdiag, nullptr, n_failed);
}

int gpv_plan_loo(gpv_plan *pl, const double *Z_ord, int64_t ldz, int ncols, double *mean, int64_t ldm, double *var, double *scores,
                 int64_t *n_failed)
{
    if (!pl || !Z_ord || !scores || !n_failed) return GPV_ERR_BAD_ARG;
    if (ncols < 1 || ncols > kLooMaxCols) return GPV_ERR_BAD_ARG;
    if (ldz < pl->Nlocs || (mean && ldm < pl->Nlocs)) return GPV_ERR_BAD_ARG;
    return loo_run(pl, kLooModeCV, Z_ord, ldz, ncols, mean, ldm, var, scores, n_failed);
}

// developer aid (tools/loo_timing.py; not part of the public header): device time of `reps` runs of the device passes of the
// latest gpv_plan_whiten_t / gpv_plan_precision / gpv_plan_loo over the columns it left on the device, by a pair of events
// around them alone: no copies to or from the host
extern "C" int gpv_plan_debug_loo_ms(gpv_plan *pl, int reps, double *ms)
{
    if (!pl || reps <= 0 || !ms) return GPV_ERR_BAD_ARG;
    if (const int rc = loo_state(pl)) return rc;
    if (pl->loo_last_mode < 0 || !pl->loo_have_index || pl->loo_g_eval != pl->eval_count) return GPV_ERR_STATE;
    return timed_reps(pl, true, reps, ms, [&] { return loo_enqueue(pl, pl->loo_last_mode, pl->loo_last_ncols, true, pl->stream); });
}

// ---- leave-block-out cross-validation: per-block precision solves (gpv_blockcv.hip) ----------------------------------------
int gpv_blockcv_nscores(void) { return kBcvNScores; }
int gpv_blockcv_max_block(void) { return kBcvMaxBlock; }

static int blockcv_status(int rc) { return rc == 0 ? GPV_OK : rc == 1 ? GPV_ERR_INDEX : GPV_ERR_BAD_ARG; }

int gpv_blocks_index_host(const int32_t *nn, const int32_t *rowid, int64_t rows, int64_t Nlocs, int P, const int32_t *newpos,
                          const int32_t *block_of_ord, int64_t *n_blocks, int64_t *n_heldout, int *max_size, int64_t *n_set_refs,
                          int32_t *memptr, int32_t *members, int32_t *setptr, int32_t *sets, int64_t sets_cap, int32_t *blkloc)
{
    if (!n_blocks || !n_heldout || !max_size || !n_set_refs || rows < 0 || Nlocs < 0 || P < 1) return GPV_ERR_BAD_ARG;
    if (rows * (int64_t)P >= ((int64_t)1 << 31) || Nlocs >= ((int64_t)1 << 31) - 1) return GPV_ERR_INDEX;      // before any array is read
    if (!nn || !rowid || !block_of_ord) return GPV_ERR_BAD_ARG;
    BlockIndex ix;
    if (const int rc = blockcv_build_index(nn, rowid, rows, Nlocs, P, newpos, block_of_ord, ix)) return blockcv_status(rc);
    *n_blocks = ix.n_blocks;
    *n_heldout = ix.n_heldout;
    *max_size = ix.max_size;
    *n_set_refs = ix.n_set_refs;
    if (memptr) std::copy(ix.memptr.begin(), ix.memptr.end(), memptr);
    if (members) std::copy(ix.members.begin(), ix.members.end(), members);
    if (setptr) std::copy(ix.setptr.begin(), ix.setptr.end(), setptr);
    if (blkloc) std::copy(ix.blkloc.begin(), ix.blkloc.end(), blkloc);
    if (sets) {
        if (sets_cap < ix.n_set_refs) return GPV_ERR_BAD_ARG;
        std::copy(ix.sets.begin(), ix.sets.end(), sets);
    }
    return GPV_OK;
}

int gpv_plan_set_blocks(gpv_plan *pl, const int32_t *block_of_ord, int64_t *n_blocks, int64_t *n_heldout, int *max_size,
                        int64_t *n_set_refs)
{
    if (!pl || !block_of_ord || !n_blocks || !n_heldout || !max_size || !n_set_refs) return GPV_ERR_BAD_ARG;
    if (const int rc = loo_structure(pl)) return rc;
    const int64_t rows = pl->rows, n = pl->Nlocs;
    const int P = pl->P;
    if (pl->h_newpos.size() != (size_t)n) return GPV_ERR_STATE;
    {                                                  // the labels by themselves, before the device is touched
        std::vector<int32_t> ids, sizes;
        if (blockcv_check_labels(block_of_ord, n, ids, sizes) != 0) return GPV_ERR_BAD_ARG;
    }
    GPV_HIP(hipSetDevice(pl->device));
    std::vector<int32_t> nn((size_t)rows * P), rowid((size_t)rows);
    GPV_HIP(hipMemcpy(nn.data(), pl->d_nn, nn.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(rowid.data(), pl->d_rowid, rowid.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    BlockIndex ix;
    if (const int rc = blockcv_build_index(nn.data(), rowid.data(), rows, n, P, pl->h_newpos.data(), block_of_ord, ix))
        return rc == 2 ? GPV_ERR_STATE : blockcv_status(rc);
    // the new index goes to buffers of its own first: a failure leaves the plan's current blocks as they were
    DevBuf<int32_t> memptr, members, setptr, sets, blkloc;
    GPV_BUF(memptr, upload(ix.memptr.data(), ix.memptr.size()));
    GPV_BUF(members, upload(ix.members.data(), ix.members.size()));
    GPV_BUF(setptr, upload(ix.setptr.data(), ix.setptr.size()));
    GPV_BUF(sets, upload(ix.sets.data(), ix.sets.size()));
    GPV_BUF(blkloc, upload(ix.blkloc.data(), ix.blkloc.size()));
    GPV_HIP(hipStreamSynchronize(pl->stream));         // nothing of an earlier call still reads the index that is about to go
    pl->d_bcv_memptr = std::move(memptr);
    pl->d_bcv_members = std::move(members);
    pl->d_bcv_setptr = std::move(setptr);
    pl->d_bcv_sets = std::move(sets);
    pl->d_bcv_blkloc = std::move(blkloc);
    pl->bcv_nblocks = *n_blocks = ix.n_blocks;
    pl->bcv_nheld = *n_heldout = ix.n_heldout;
    pl->bcv_maxsize = *max_size = ix.max_size;
    pl->bcv_nrefs = *n_set_refs = ix.n_set_refs;
    pl->bcv_grid = blockcv_grid(ix.n_blocks, pl->cus);
    pl->bcv_last_ncols = 0;
    pl->bcv_have = true;
    return GPV_OK;
}

// back to the ordered numbering, column-major, and the scores
static hipError_t bcv_epilogue(gpv_plan *pl, int ncols, int cp, hipStream_t st)
{
    const int64_t n = pl->Nlocs;
    hipError_t e;
    if ((e = launch_loo_unpack(pl->d_bcv_D, pl->d_newpos, n, ncols, cp, pl->d_bcv_out, st)) != hipSuccess) return e;
    if ((e = launch_loo_unpack(pl->d_bcv_Y2, pl->d_newpos, n, ncols, cp, pl->d_bcv_y2ord, st)) != hipSuccess) return e;
    if ((e = launch_loo_unpack(pl->d_bcv_var, pl->d_newpos, n, 1, 1, pl->d_bcv_varord, st)) != hipSuccess) return e;
    if ((e = launch_loo_unpack(pl->d_bcv_nlp, pl->d_newpos, n, 1, 1, pl->d_bcv_nlpord, st)) != hipSuccess) return e;
    return launch_blockcv_scores(pl->d_bcv_in, pl->d_bcv_out, pl->d_bcv_y2ord, pl->d_bcv_varord, pl->d_bcv_nlpord, n, ncols,
                                 pl->bcv_sgrid, pl->d_bcv_part, pl->d_bcv_scores, st);
}

// the device passes of one call on what is resident: d_bcv_in -> d_bcv_out, d_bcv_varord, d_bcv_scores, d_bcv_nbad.
// parts (gpv_plan_debug_blockcv_ms): 1 = r = Q z (pack, forward, transposed), 2 = the fills and the block pass, 4 = unpack and scores
static hipError_t bcv_enqueue(gpv_plan *pl, int ncols, hipStream_t st, int parts = 7)
{
    const int cp = whiten_cp(ncols);
    const int64_t n = pl->Nlocs;
    LooArgs a = loo_args(pl);
    a.B = pl->d_bcv_B; a.E = pl->d_bcv_E; a.R = pl->d_bcv_R; a.q = pl->d_bcv_q;
    hipError_t e;
    if (parts & 1) {
        if ((e = launch_loo_pack(pl->d_bcv_in, pl->d_newpos, n, ncols, cp, pl->d_bcv_B, st)) != hipSuccess) return e;
        if ((e = launch_loo_forward(a, cp, pl->loo_grid, st)) != hipSuccess) return e;
        if ((e = launch_loo_transposed(a, cp, pl->loo_grid, st)) != hipSuccess) return e;
    }
    if (!(parts & 2)) return parts & 4 ? bcv_epilogue(pl, ncols, cp, st) : hipSuccess;
    // every byte 0xFF is a NaN: what a kept location and a bad block return
    const size_t colbytes = sizeof(double) * (size_t)n * cp, vecbytes = sizeof(double) * (size_t)n;
    if ((e = hipMemsetAsync(pl->d_bcv_D, 0xFF, colbytes, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(pl->d_bcv_Y2, 0xFF, colbytes, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(pl->d_bcv_var, 0xFF, vecbytes, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(pl->d_bcv_nlp, 0xFF, vecbytes, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(pl->d_bcv_nbad, 0, sizeof(unsigned), st)) != hipSuccess) return e;
    BlockCvArgs b;
    b.L = a.L; b.nn = a.nn; b.rowid = a.rowid; b.g = a.g;     // the factor's view and the scale, as the two passes above had them
    b.memptr = pl->d_bcv_memptr; b.members = pl->d_bcv_members; b.setptr = pl->d_bcv_setptr; b.sets = pl->d_bcv_sets;
    b.blkloc = reinterpret_cast<const int2 *>(pl->d_bcv_blkloc.get());
    b.B = pl->d_bcv_B; b.R = pl->d_bcv_R; b.D = pl->d_bcv_D; b.Y2 = pl->d_bcv_Y2; b.var = pl->d_bcv_var; b.nlp = pl->d_bcv_nlp;
    b.nbad = pl->d_bcv_nbad;
    b.n_blocks = pl->bcv_nblocks; b.P = pl->P;
    if ((e = launch_blockcv_blocks(b, cp, pl->bcv_grid, st)) != hipSuccess) return e;
    return parts & 4 ? bcv_epilogue(pl, ncols, cp, st) : hipSuccess;
}

// Reads what gpv_plan_loo reads (d_L, the index arrays, the nuggets, the transposed index, the scale of the evaluation) and
// writes buffers of its own: the plan's last evaluation and what gpv_plan_whiten and gpv_plan_loo left on the device stay.
int gpv_plan_block_cv(gpv_plan *pl, const double *Z_ord, int64_t ldz, int ncols, double *mean, int64_t ldm, double *var, double *scores,
                      int64_t *n_failed, int64_t *n_bad_blocks)
{
    if (!pl || !Z_ord || !scores || !n_failed || !n_bad_blocks) return GPV_ERR_BAD_ARG;
    if (ncols < 1 || ncols > kBcvMaxCols) return GPV_ERR_BAD_ARG;
    if (ldz < pl->Nlocs || (mean && ldm < pl->Nlocs)) return GPV_ERR_BAD_ARG;
    if (const int rc = loo_state(pl)) return rc;
    if (!pl->bcv_have) return GPV_ERR_STATE;
    const int64_t n = pl->Nlocs;
    if (const int rc = enter(pl)) return rc;
    hipStream_t st = pl->stream;
    if (const int rc = loo_index(pl)) return rc;
    const int cp = whiten_cp(ncols);
    if (cp > pl->bcv_cp_cap) {
        const size_t cnt = (size_t)n * cp;
        pl->bcv_cp_cap = 0;
        GPV_BUF(pl->d_bcv_in, resize(cnt));
        GPV_BUF(pl->d_bcv_out, resize(cnt));
        GPV_BUF(pl->d_bcv_B, resize(cnt));
        GPV_BUF(pl->d_bcv_E, resize(cnt));
        GPV_BUF(pl->d_bcv_R, resize(cnt));
        GPV_BUF(pl->d_bcv_D, resize(cnt));
        GPV_BUF(pl->d_bcv_Y2, resize(cnt));
        GPV_BUF(pl->d_bcv_y2ord, resize(cnt));
        GPV_BUF(pl->d_bcv_q, ensure((size_t)n));
        GPV_BUF(pl->d_bcv_var, ensure((size_t)n));
        GPV_BUF(pl->d_bcv_nlp, ensure((size_t)n));
        GPV_BUF(pl->d_bcv_varord, ensure((size_t)n));
        GPV_BUF(pl->d_bcv_nlpord, ensure((size_t)n));
        GPV_BUF(pl->d_bcv_nbad, ensure(2));
        pl->bcv_sgrid = blockcv_score_grid(n, pl->cus);
        GPV_BUF(pl->d_bcv_part, ensure((size_t)kBcvMaxCols * pl->bcv_sgrid * kBcvNScores));
        GPV_BUF(pl->d_bcv_scores, ensure((size_t)kBcvMaxCols * kBcvNScores));
        pl->bcv_cp_cap = cp;
    }
    if (const int rc = loo_scale_once(pl, st)) return rc;
    if (cols_to_device(pl->d_bcv_in, Z_ord, ldz, n, ncols, st)) return drain_fail(st, GPV_ERR_HIP);
    pl->bcv_last_ncols = ncols;
    if (GPV_HIP_FAILED(bcv_enqueue(pl, ncols, st))) return drain_fail(st, GPV_ERR_HIP);
    double sc[kBcvMaxCols * kBcvNScores];
    unsigned nbad = 0;
    if (GPV_HIP_FAILED(hipMemcpyAsync(sc, pl->d_bcv_scores, sizeof(double) * (size_t)ncols * kBcvNScores, hipMemcpyDeviceToHost, st)))
        return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipMemcpyAsync(&nbad, pl->d_bcv_nbad, sizeof(nbad), hipMemcpyDeviceToHost, st))) return drain_fail(st, GPV_ERR_HIP);
    if (mean && cols_to_host(mean, ldm, pl->d_bcv_out, n, ncols, st)) return drain_fail(st, GPV_ERR_HIP);   // (mean may be Z_ord: read before)
    if (var && GPV_HIP_FAILED(hipMemcpyAsync(var, pl->d_bcv_varord, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st)))
        return drain_fail(st, GPV_ERR_HIP);
    GPV_HIP(hipStreamSynchronize(st));
    const bool bad = pl->loo_nfail > 0;
    *n_failed = (int64_t)pl->loo_nfail;
    *n_bad_blocks = (int64_t)nbad;
    for (int t = 0; t < ncols * kBcvNScores; ++t) scores[t] = bad ? (double)NAN : sc[t];
    if (bad) {                                         // a failed row's NaN reaches every block that names it: no entry is trusted
        if (mean) cols_fill_nan(mean, ldm, n, ncols);
        if (var) std::fill_n(var, (size_t)n, (double)NAN);
    }
    return GPV_OK;
}

// developer aid (tools/blockcv_timing.py; not part of the public header): device time of `reps` runs of the device passes of
// the latest gpv_plan_block_cv over the columns it left on the device, by a pair of events around them alone; parts: 7 = all,
// or 1 / 2 / 4 = one part of bcv_enqueue on what the other parts left
extern "C" int gpv_plan_debug_blockcv_ms(gpv_plan *pl, int reps, int parts, double *ms)
{
    if (!pl || reps <= 0 || !ms || parts < 1 || parts > 7) return GPV_ERR_BAD_ARG;
    if (const int rc = loo_state(pl)) return rc;
    if (!pl->bcv_have || pl->bcv_last_ncols < 1 || !pl->loo_have_index || pl->loo_g_eval != pl->eval_count) return GPV_ERR_STATE;
    return timed_reps(pl, true, reps, ms, [&] { return bcv_enqueue(pl, pl->bcv_last_ncols, pl->stream, parts); });
}

// ---- local kriging of a cond.yz='z' plan at new locations (gpv_krige.hip; the search: gpv_nn.hip) --------------------------
int gpv_krige_max_cols(void) { return kKrigeMaxCols; }

// ---- what gpv_plan_krige and gpv_plan_krige_groups share ----
// the buffers that live for one call and the search index over the plan's locations
namespace {
struct KrigeCall {
    CovSetup cs;
    DevBuf<double> d_nug, d_in, d_Z;
    QnnIndex ix;
    KrigeCall() = default;
    KrigeCall(const KrigeCall &) = delete;
    KrigeCall &operator=(const KrigeCall &) = delete;
    ~KrigeCall() { qnn_free(ix); }
};
}  // namespace

// the arguments both entries take: the nuggets, the columns, the family and its parameters, the scale of the search
static int krige_check_args(const gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, const double *nuggets,
                            int64_t n_nuggets, const double *Z_ord, int64_t ldz, int ncols, const double *scale, CovSetup &cs)
{
    const int64_t n = pl->Nlocs;
    if ((n_nuggets != 1 && n_nuggets != n) || ncols < 1 || ncols > kKrigeMaxCols) return GPV_ERR_BAD_ARG;
    if (Z_ord ? ldz < n : ncols != 1) return GPV_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_nuggets; ++i)
        if (!(nuggets[i] >= 0.0) || !std::isfinite(nuggets[i])) return GPV_ERR_BAD_ARG;
    const bool matern = std::strcmp(covType, "matern") == 0, scaled = std::strcmp(covType, "matern_scaledim") == 0;
    if (!matern && !scaled && std::strcmp(covType, "esqe") != 0) return GPV_ERR_COVTYPE;
    if (ncovparms != (matern ? 3 : (scaled ? pl->dim + 2 : 4))) return GPV_ERR_BAD_ARG;
    if (const int rc = cov_setup(covType, covparms, ncovparms, pl->dim, cs)) return rc;
    if (scale)
        for (int t = 0; t < pl->dim; ++t)
            if (!(scale[t] > 0.0) || !std::isfinite(scale[t])) return GPV_ERR_BAD_ARG;
    return GPV_OK;
}

// the plan both entries take; NN: nn given ids (or nullptr), each in [0, Nlocs]
static int krige_check_state(const gpv_plan *pl, bool plan_data, const int *NN, int64_t nn)
{
    const int64_t n = pl->Nlocs;
    if (pl->dim > kMaxDimGeneric || !pl->d_locs || !pl->d_newpos) return GPV_ERR_STATE;
    // a row shard, unobserved locations, a neighbour conditioned on as latent (not a 'z' plan), no data to predict from
    if (pl->comm || pl->rows != n || pl->d_obs || pl->latent_nb || (plan_data && !pl->has_z) || (int64_t)pl->h_newpos.size() != n)
        return GPV_ERR_STATE;
    if (NN)
        for (int64_t i = 0; i < nn; ++i)
            if (NN[i] < 0 || NN[i] > n) return GPV_ERR_INDEX;
    return GPV_OK;
}

// what a pass reads of the plan and of the call, but the chunks: the records, the covariance (the table of a general
// smoothness included), the call's nuggets and columns on the device
static int krige_resident(gpv_plan *pl, const double *covparms, int ncovparms, const double *nuggets, int64_t n_nuggets,
                          const double *Z_ord, int64_t ldz, int ncols, int m, KrigeCall &kc, KrigeArgs &a, hipStream_t st)
{
    const CovSetup &cs = kc.cs;
    const int64_t n = pl->Nlocs;
    const int dim = pl->dim;
    a.rec = pl->d_locs; a.z = pl->d_z; a.newpos = pl->d_newpos;
    a.m = m; a.dim = dim; a.locs_ld = pl->locs_ld; a.ncols = ncols;
    a.cov = cs.cov; a.nscale = cs.nscale;
    a.sA = cs.sA; a.cA = cs.cA; a.sB = cs.sB; a.cB = cs.cB; a.nug = nuggets[0];
    for (int t = 0; t < 8; ++t) a.inv[t] = (cs.nscale && t < dim) ? cs.inv[t] : 1.0;
    a.gen = MaternDerivConst{0.0, 0.0, 0.0};
    if (cs.cov == COV_MATERN_GEN) {
        // (cov_setup's sA is the normalised constant of the set kernel's value path: the tables hold C / sigma^2)
        a.sA = covparms[0];
        a.gen = matern_deriv_const(covparms[ncovparms - 1]);
        int e_lo = 0, base = 0, nseg = 0;
        const double lo = cs.nscale ? cs.inv_min : a.cA, hi = cs.nscale ? cs.inv_max : a.cA;
        if (getenv("GPV_NO_MATERN_TABLE") == nullptr && pl->dist_min > 0.0 && pl->dist_max >= pl->dist_min &&
            matern_dtab_range(0.5 * pl->dist_min * lo, 4.0 * pl->dist_max * hi, &e_lo, &base, &nseg)) {
            GPV_BUF(pl->d_gmt, ensure((size_t)MaternDTab::MAX_SEG * MaternDTab::ROW));
            GPV_HIP(launch_matern_dtab(a.gen, e_lo, nseg, pl->d_gmt, st));
            a.gmt = pl->d_gmt; a.gmt_base = base; a.gmt_nseg = nseg;
        }
    }
    // the call's nuggets and columns
    if (n_nuggets > 1) {
        GPV_BUF(kc.d_nug, upload(nuggets, (size_t)n));
        a.nuggets = kc.d_nug;
    }
    if (Z_ord) {
        a.zld = (ncols + 3) / 4 * 4;
        GPV_BUF(kc.d_in, resize((size_t)n * ncols));
        GPV_BUF(kc.d_Z, resize((size_t)n * a.zld));
        if (cols_to_device(kc.d_in, Z_ord, ldz, n, ncols, st)) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(launch_rep_pack(kc.d_in, pl->d_newpos, n, ncols, a.zld, kc.d_Z, st))) return drain_fail(st, GPV_ERR_HIP);
        a.Z = kc.d_Z;
    }
    return GPV_OK;
}

// the search index over the plan's locations in the ORDERED numbering, on the coordinates divided by `scale`
static int krige_index(gpv_plan *pl, const double *scale, const unsigned char *eligible_ord, KrigeCall &kc, hipStream_t st)
{
    const int64_t n = pl->Nlocs;
    const int dim = pl->dim;
    const int ld = dim <= 3 ? 4 : pl->locs_ld;
    std::vector<double> rec((size_t)n * ld), lc((size_t)n * dim);
    if (GPV_HIP_FAILED(hipMemcpyAsync(rec.data(), pl->d_locs, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, st)) ||
        GPV_HIP_FAILED(hipStreamSynchronize(st)))
        return drain_fail(st, GPV_ERR_HIP);
    for (int t = 0; t < dim; ++t)
        for (int64_t i = 0; i < n; ++i) {
            const double x = rec[(size_t)pl->h_newpos[(size_t)i] * ld + t];
            lc[(size_t)i + (size_t)t * n] = scale ? x / scale[t] : x;
        }
    if (GPV_HIP_FAILED(qnn_build(lc.data(), n, dim, eligible_ord, kc.ix))) return drain_fail(st, GPV_ERR_HIP);
    return GPV_OK;
}

// Reads the plan's records, its data and newpos, and writes buffers that live for the call only (and d_gmt, the table of a
// general smoothness, which the blocking gradient calls share): no evaluation is needed and none is disturbed.  Every refusal
// comes before the device is touched and before anything is written.
int gpv_plan_krige(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, const double *nuggets, int64_t n_nuggets,
                   const double *Z_ord, int64_t ldz, int ncols, const double *qlocs, int64_t nq, int m, const int *NNq,
                   const double *scale, const unsigned char *eligible_ord, int64_t chunk, double *mean, int64_t ldm, double *var,
                   int64_t *n_failed)
{
    if (!pl || !covType || !covparms || !nuggets || !n_failed || nq < 0 || chunk < 0 || m < 1) return GPV_ERR_BAD_ARG;
    if (nq > 0 && (!qlocs || !mean || !var)) return GPV_ERR_BAD_ARG;
    if (ldm < nq) return GPV_ERR_BAD_ARG;
    KrigeCall kc;
    if (const int rc = krige_check_args(pl, covType, covparms, ncovparms, nuggets, n_nuggets, Z_ord, ldz, ncols, scale, kc.cs)) return rc;
    if (m + 1 > kKrigeMaxP) return GPV_ERR_UNSUPPORTED_M;
    if (const int rc = krige_check_state(pl, !Z_ord, NNq, nq * m)) return rc;
    *n_failed = 0;
    if (nq == 0) return GPV_OK;

    if (const int rc = enter(pl)) return rc;
    hipStream_t st = pl->stream;
    const int dim = pl->dim;
    KrigeArgs a{};
    if (const int rc = krige_resident(pl, covparms, ncovparms, nuggets, n_nuggets, Z_ord, ldz, ncols, m, kc, a, st)) return rc;
    if (!NNq)
        if (const int rc = krige_index(pl, scale, eligible_ord, kc, st)) return rc;
    // the chunks: queries up, search or neighbours up, the pass, results back
    const int64_t cap = std::min<int64_t>(chunk > 0 ? chunk : kKrigeChunk, nq);
    DevBuf<double> d_q, d_qs, d_mean, d_var;
    DevBuf<int32_t> d_nn;
    DevBuf<unsigned> d_nfail;
    GPV_BUF(d_q, resize((size_t)cap * dim));
    if (!NNq && scale) GPV_BUF(d_qs, resize((size_t)cap * dim));
    GPV_BUF(d_mean, resize((size_t)cap * ncols));
    GPV_BUF(d_var, resize((size_t)cap));
    GPV_BUF(d_nn, resize((size_t)cap * m));
    GPV_BUF(d_nfail, resize(2));
    if (GPV_HIP_FAILED(hipMemsetAsync(d_nfail, 0, sizeof(unsigned), st))) return drain_fail(st, GPV_ERR_HIP);
    a.nnq = d_nn; a.q = d_q; a.mean = d_mean; a.var = d_var; a.nfail = d_nfail;
    Event ev[3];                                           // around the search and the pass of a chunk
    for (auto &e : ev) GPV_HIP(hipEventCreate(e.put()));
    pl->kr_search_ms = pl->kr_pass_ms = 0.0;
    std::vector<double> hq((size_t)cap * dim), hqs(d_qs ? (size_t)cap * dim : 0);
    std::vector<int32_t> hnn(NNq ? (size_t)cap * m : 0);
    for (int64_t c0 = 0; c0 < nq; c0 += cap) {
        const int64_t cn = std::min(cap, nq - c0);
        for (int t = 0; t < dim; ++t)
            for (int64_t i = 0; i < cn; ++i) {
                const double x = qlocs[c0 + i + (int64_t)t * nq];
                hq[(size_t)i * dim + t] = x;
                if (d_qs) hqs[(size_t)i * dim + t] = x / scale[t];
            }
        if (GPV_HIP_FAILED(hipMemcpyAsync(d_q, hq.data(), sizeof(double) * (size_t)cn * dim, hipMemcpyHostToDevice, st)))
            return drain_fail(st, GPV_ERR_HIP);
        if (NNq) {
            for (int s = 0; s < m; ++s)
                for (int64_t i = 0; i < cn; ++i) hnn[(size_t)i * m + s] = NNq[c0 + i + (int64_t)s * nq];
            if (GPV_HIP_FAILED(hipMemcpyAsync(d_nn, hnn.data(), sizeof(int32_t) * (size_t)cn * m, hipMemcpyHostToDevice, st)))
                return drain_fail(st, GPV_ERR_HIP);
        } else {
            if (d_qs && GPV_HIP_FAILED(hipMemcpyAsync(d_qs, hqs.data(), sizeof(double) * (size_t)cn * dim, hipMemcpyHostToDevice, st)))
                return drain_fail(st, GPV_ERR_HIP);
            if (GPV_HIP_FAILED(hipEventRecord(ev[0], st))) return drain_fail(st, GPV_ERR_HIP);
            if (GPV_HIP_FAILED(qnn_search(kc.ix, d_qs ? d_qs.get() : d_q.get(), cn, m, d_nn, st))) return drain_fail(st, GPV_ERR_HIP);
        }
        a.nq = cn;
        if (GPV_HIP_FAILED(hipEventRecord(ev[1], st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(launch_krige(a, krige_grid(cn, pl->cus), st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipEventRecord(ev[2], st))) return drain_fail(st, GPV_ERR_HIP);
        if (cols_to_host(mean + c0, ldm, d_mean, cn, ncols, st)) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipMemcpyAsync(var + c0, d_var, sizeof(double) * (size_t)cn, hipMemcpyDeviceToHost, st)))
            return drain_fail(st, GPV_ERR_HIP);
        GPV_HIP(hipStreamSynchronize(st));                 // (the staging vectors and the chunk buffers are reused)
        float t = 0.f;
        if (!NNq && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) pl->kr_search_ms += (double)t;
        if (hipEventElapsedTime(&t, ev[1], ev[2]) == hipSuccess) pl->kr_pass_ms += (double)t;
    }
    unsigned nbad = 0;
    GPV_HIP(hipMemcpy(&nbad, d_nfail, sizeof(nbad), hipMemcpyDeviceToHost));
    *n_failed = (int64_t)nbad;
    return GPV_OK;
}

// ---- grouped local kriging (gpv_krige_groups.hip): joint predictions of groups of locations that share a conditioning set ----
int gpv_krige_groups_max_rows(void) { return kKrigeGroupMaxRows; }

// The contract of gpv_plan_krige: buffers that live for the call, no evaluation needed and none disturbed, every refusal before
// the device is touched and before anything is written.  The groups are streamed `chunk` at a time; the groups of a chunk are
// binned by their row bucket (a function of m + g alone) and each bucket is one launch, so a group's bits depend neither on the
// chunking nor on the other groups.
int gpv_plan_krige_groups(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, const double *nuggets,
                          int64_t n_nuggets, const double *Z_ord, int64_t ldz, int ncols, const double *qlocs, int64_t nq,
                          const int64_t *gptr, int64_t ngroups, const double *weights, int m, const int *NNg, const double *scale,
                          const unsigned char *eligible_ord, int64_t chunk, double *mean, int64_t ldm, double *var, double *gmean,
                          int64_t ldg, double *gvar, double *cov, int64_t *n_failed)
{
    if (!pl || !covType || !covparms || !nuggets || !n_failed || nq < 0 || ngroups < 0 || chunk < 0 || m < 1) return GPV_ERR_BAD_ARG;
    if (ngroups > 0 && (!gptr || !qlocs || !mean || !var || !gmean || !gvar)) return GPV_ERR_BAD_ARG;
    if (ldm < nq || ldg < ngroups) return GPV_ERR_BAD_ARG;
    KrigeCall kc;
    if (const int rc = krige_check_args(pl, covType, covparms, ncovparms, nuggets, n_nuggets, Z_ord, ldz, ncols, scale, kc.cs)) return rc;
    // the groups: gptr non-decreasing from 0 to nq, no group empty
    if (ngroups == 0 ? nq != 0 : (gptr[0] != 0 || gptr[ngroups] != nq)) return GPV_ERR_BAD_ARG;
    int64_t gmax = 0;
    for (int64_t k = 0; k < ngroups; ++k) {
        if (gptr[k + 1] <= gptr[k] || gptr[k + 1] > nq) return GPV_ERR_BAD_ARG;
        gmax = std::max(gmax, gptr[k + 1] - gptr[k]);
    }
    if (weights)
        for (int64_t i = 0; i < nq; ++i)
            if (!std::isfinite(weights[i])) return GPV_ERR_BAD_ARG;
    if (m + 1 > kKrigeGroupMaxRows || m + gmax > kKrigeGroupMaxRows) return GPV_ERR_UNSUPPORTED_M;
    if (const int rc = krige_check_state(pl, !Z_ord, NNg, ngroups * m)) return rc;
    *n_failed = 0;
    if (ngroups == 0) return GPV_OK;

    if (const int rc = enter(pl)) return rc;
    hipStream_t st = pl->stream;
    const int dim = pl->dim;
    KrigeGroupArgs a{};
    if (const int rc = krige_resident(pl, covparms, ncovparms, nuggets, n_nuggets, Z_ord, ldz, ncols, m, kc, a.k, st)) return rc;
    if (!NNg)
        if (const int rc = krige_index(pl, scale, eligible_ord, kc, st)) return rc;
    // the chunks, by groups; what the largest of them holds
    const int64_t cap = std::min<int64_t>(std::min<int64_t>(chunk > 0 ? chunk : kKrigeGroupChunk, ngroups), (int64_t)1 << 24);
    int64_t maxq = 0, maxc = 0;
    const auto tri = [](int64_t g) { return g * (g + 1) / 2; };
    for (int64_t k0 = 0; k0 < ngroups; k0 += cap) {
        const int64_t k1 = std::min(k0 + cap, ngroups);
        int64_t c = 0;
        for (int64_t k = k0; k < k1; ++k) c += tri(gptr[k + 1] - gptr[k]);
        maxq = std::max(maxq, gptr[k1] - gptr[k0]);
        maxc = std::max(maxc, c);
    }
    DevBuf<double> d_q, d_anc, d_w, d_mean, d_var, d_gmean, d_gvar, d_cov;
    DevBuf<int32_t> d_nn, d_gptr, d_list;
    DevBuf<int64_t> d_coff;
    DevBuf<unsigned> d_nfail;
    GPV_BUF(d_q, resize((size_t)maxq * dim));
    if (!NNg) GPV_BUF(d_anc, resize((size_t)cap * dim));
    GPV_BUF(d_w, resize((size_t)maxq));
    GPV_BUF(d_mean, resize((size_t)maxq * ncols));
    GPV_BUF(d_var, resize((size_t)maxq));
    GPV_BUF(d_gmean, resize((size_t)cap * ncols));
    GPV_BUF(d_gvar, resize((size_t)cap));
    if (cov) {
        GPV_BUF(d_cov, resize((size_t)maxc));
        GPV_BUF(d_coff, resize((size_t)cap));
    }
    GPV_BUF(d_nn, resize((size_t)cap * m));
    GPV_BUF(d_gptr, resize((size_t)cap + 1));
    GPV_BUF(d_list, resize((size_t)cap));
    GPV_BUF(d_nfail, resize(2));
    if (GPV_HIP_FAILED(hipMemsetAsync(d_nfail, 0, sizeof(unsigned), st))) return drain_fail(st, GPV_ERR_HIP);
    a.k.nnq = d_nn; a.k.q = d_q; a.k.mean = d_mean; a.k.var = d_var; a.k.nfail = d_nfail;
    a.gptr = d_gptr; a.w = d_w; a.coff = d_coff; a.gmean = d_gmean; a.gvar = d_gvar; a.cov = cov ? d_cov.get() : nullptr;
    Event ev[3];                                           // around the search and the passes of a chunk
    for (auto &e : ev) GPV_HIP(hipEventCreate(e.put()));
    pl->kr_search_ms = pl->kr_pass_ms = 0.0;
    std::vector<double> hq((size_t)maxq * dim), hanc(NNg ? 0 : (size_t)cap * dim), hw((size_t)maxq);
    std::vector<int32_t> hnn(NNg ? (size_t)cap * m : 0), hgptr((size_t)cap + 1), hlist((size_t)cap);
    std::vector<int64_t> hcoff(cov ? (size_t)cap : 0);
    int64_t cov0 = 0;                                      // where the chunk's triangles start in `cov`
    for (int64_t k0 = 0; k0 < ngroups; k0 += cap) {
        const int64_t cg = std::min(cap, ngroups - k0), q0 = gptr[k0], cn = gptr[k0 + cg] - q0;
        int64_t nb[kKrigeGroupBuckets] = {0, 0, 0}, at[kKrigeGroupBuckets], clen = 0;
        for (int64_t k = 0; k < cg; ++k) {
            const int64_t g0 = gptr[k0 + k] - q0, g = gptr[k0 + k + 1] - gptr[k0 + k];
            hgptr[(size_t)k] = (int32_t)g0;
            ++nb[krige_group_bucket(m + (int)g)];
            if (cov) hcoff[(size_t)k] = clen;
            clen += tri(g);
            for (int64_t i = 0; i < g; ++i) hw[(size_t)(g0 + i)] = weights ? weights[q0 + g0 + i] : 1.0 / (double)g;
            if (!NNg)                                      // the anchor: the members' mean, summed in member order, then the scale
                for (int t = 0; t < dim; ++t) {
                    double s = qlocs[q0 + g0 + (int64_t)t * nq];
                    for (int64_t i = 1; i < g; ++i) s += qlocs[q0 + g0 + i + (int64_t)t * nq];
                    const double anchor = s / (double)g;
                    hanc[(size_t)k * dim + t] = scale ? anchor / scale[t] : anchor;
                }
        }
        hgptr[(size_t)cg] = (int32_t)cn;
        at[0] = 0; at[1] = nb[0]; at[2] = nb[0] + nb[1];
        {
            int64_t fill[kKrigeGroupBuckets] = {at[0], at[1], at[2]};
            for (int64_t k = 0; k < cg; ++k) hlist[(size_t)fill[krige_group_bucket(m + (int)(gptr[k0 + k + 1] - gptr[k0 + k]))]++] = (int32_t)k;
        }
        for (int t = 0; t < dim; ++t)
            for (int64_t i = 0; i < cn; ++i) hq[(size_t)i * dim + t] = qlocs[q0 + i + (int64_t)t * nq];
        if (GPV_HIP_FAILED(hipMemcpyAsync(d_q, hq.data(), sizeof(double) * (size_t)cn * dim, hipMemcpyHostToDevice, st)) ||
            GPV_HIP_FAILED(hipMemcpyAsync(d_w, hw.data(), sizeof(double) * (size_t)cn, hipMemcpyHostToDevice, st)) ||
            GPV_HIP_FAILED(hipMemcpyAsync(d_gptr, hgptr.data(), sizeof(int32_t) * (size_t)(cg + 1), hipMemcpyHostToDevice, st)) ||
            GPV_HIP_FAILED(hipMemcpyAsync(d_list, hlist.data(), sizeof(int32_t) * (size_t)cg, hipMemcpyHostToDevice, st)))
            return drain_fail(st, GPV_ERR_HIP);
        if (cov && GPV_HIP_FAILED(hipMemcpyAsync(d_coff, hcoff.data(), sizeof(int64_t) * (size_t)cg, hipMemcpyHostToDevice, st)))
            return drain_fail(st, GPV_ERR_HIP);
        if (NNg) {
            for (int s = 0; s < m; ++s)
                for (int64_t k = 0; k < cg; ++k) hnn[(size_t)k * m + s] = NNg[k0 + k + (int64_t)s * ngroups];
            if (GPV_HIP_FAILED(hipMemcpyAsync(d_nn, hnn.data(), sizeof(int32_t) * (size_t)cg * m, hipMemcpyHostToDevice, st)))
                return drain_fail(st, GPV_ERR_HIP);
        } else {
            if (GPV_HIP_FAILED(hipMemcpyAsync(d_anc, hanc.data(), sizeof(double) * (size_t)cg * dim, hipMemcpyHostToDevice, st)))
                return drain_fail(st, GPV_ERR_HIP);
            if (GPV_HIP_FAILED(hipEventRecord(ev[0], st))) return drain_fail(st, GPV_ERR_HIP);
            if (GPV_HIP_FAILED(qnn_search(kc.ix, d_anc, cg, m, d_nn, st))) return drain_fail(st, GPV_ERR_HIP);
        }
        a.k.nq = cn; a.ng = cg;
        if (GPV_HIP_FAILED(hipEventRecord(ev[1], st))) return drain_fail(st, GPV_ERR_HIP);
        for (int b = 0; b < kKrigeGroupBuckets; ++b) {
            if (nb[b] == 0) continue;
            a.list = d_list.get() + at[b]; a.nlist = nb[b];
            if (GPV_HIP_FAILED(launch_krige_groups(a, b, krige_grid(nb[b], pl->cus), st))) return drain_fail(st, GPV_ERR_HIP);
        }
        if (GPV_HIP_FAILED(hipEventRecord(ev[2], st))) return drain_fail(st, GPV_ERR_HIP);
        if (cols_to_host(mean + q0, ldm, d_mean, cn, ncols, st)) return drain_fail(st, GPV_ERR_HIP);
        if (cols_to_host(gmean + k0, ldg, d_gmean, cg, ncols, st)) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipMemcpyAsync(var + q0, d_var, sizeof(double) * (size_t)cn, hipMemcpyDeviceToHost, st)) ||
            GPV_HIP_FAILED(hipMemcpyAsync(gvar + k0, d_gvar, sizeof(double) * (size_t)cg, hipMemcpyDeviceToHost, st)))
            return drain_fail(st, GPV_ERR_HIP);
        if (cov && GPV_HIP_FAILED(hipMemcpyAsync(cov + cov0, d_cov, sizeof(double) * (size_t)clen, hipMemcpyDeviceToHost, st)))
            return drain_fail(st, GPV_ERR_HIP);
        cov0 += clen;
        GPV_HIP(hipStreamSynchronize(st));                 // (the staging vectors and the chunk buffers are reused)
        float t = 0.f;
        if (!NNg && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) pl->kr_search_ms += (double)t;
        if (hipEventElapsedTime(&t, ev[1], ev[2]) == hipSuccess) pl->kr_pass_ms += (double)t;
    }
    unsigned nbad = 0;
    GPV_HIP(hipMemcpy(&nbad, d_nfail, sizeof(nbad), hipMemcpyDeviceToHost));
    *n_failed = (int64_t)nbad;
    return GPV_OK;
}

// developer aid (tools/krige_timing.py, tools/krige_groups_timing.py; not part of the public header): device time of the
// searches and of the passes of the latest gpv_plan_krige or gpv_plan_krige_groups, each summed over the call's chunks, by
// event pairs around them alone
extern "C" int gpv_plan_debug_krige_ms(gpv_plan *pl, double *ms)
{
    if (!pl || !ms) return GPV_ERR_BAD_ARG;
    ms[0] = pl->kr_search_ms;
    ms[1] = pl->kr_pass_ms;
    return GPV_OK;
}

// ---- conditional simulation of a map (gpv_csim.hip): the sequential kriging sweep over the prediction locations -------------
namespace {
struct CsimLaunch { int lev0, lev1; bool narrow; };
}  // namespace

// The level schedule of a mixed neighbour list: entry (i, s) at NN[i * rs + s * cs]; an id in (Nlocs, Nlocs + i] names sweep row
// id - Nlocs - 1.  level(i) = 0 without such an id, else 1 + the largest level among them; the rows counting-sorted by level,
// ascending inside a level.  (The schedule of gpv_plan_unwhiten is built from the plan's index arrays, where rows may share
// their last entry and positions may have no owner: it keeps its own loop and its bits.)  Returns GPV_ERR_INDEX for an id
// outside [0, Nlocs + own row].
static int csim_levels_core(const int32_t *NN, int64_t rs, int64_t cs, int64_t nq, int m, int64_t Nlocs, std::vector<int32_t> &level,
                            std::vector<int32_t> &order, std::vector<int64_t> &levptr)
{
    level.assign((size_t)nq, 0);
    int32_t top = 0;
    for (int64_t i = 0; i < nq; ++i) {
        int32_t lv = 0;
        for (int s = 0; s < m; ++s) {
            const int64_t id = NN[i * rs + (int64_t)s * cs];
            if (id < 0 || id > Nlocs + i) return GPV_ERR_INDEX;
            if (id > Nlocs) lv = std::max(lv, level[(size_t)(id - Nlocs - 1)] + 1);
        }
        level[(size_t)i] = lv;
        top = std::max(top, lv);
    }
    const int64_t nlev = nq > 0 ? (int64_t)top + 1 : 0;
    levptr.assign((size_t)nlev + 1, 0);
    order.assign((size_t)nq, 0);
    for (int64_t i = 0; i < nq; ++i) levptr[(size_t)level[(size_t)i] + 1]++;
    for (int64_t l = 0; l < nlev; ++l) levptr[(size_t)l + 1] += levptr[(size_t)l];
    std::vector<int64_t> fill(levptr.begin(), levptr.end() - 1);
    for (int64_t i = 0; i < nq; ++i) order[(size_t)fill[(size_t)level[(size_t)i]]++] = (int32_t)i;
    return GPV_OK;
}

int gpv_csim_levels_host(const int32_t *NN, int64_t nq, int m, int64_t Nlocs, int32_t *level, int32_t *order, int64_t *levptr,
                         int64_t *n_levels)
{
    if (!n_levels || nq < 0 || m < 1 || Nlocs < 0) return GPV_ERR_BAD_ARG;
    if (Nlocs + nq >= ((int64_t)1 << 31) - 1) return GPV_ERR_INDEX;                      // before any array is read
    if (nq > 0 && (!NN || !level || !order)) return GPV_ERR_BAD_ARG;
    if (!levptr) return GPV_ERR_BAD_ARG;
    std::vector<int32_t> lv, ord;
    std::vector<int64_t> lp;
    if (const int rc = csim_levels_core(NN, 1, nq, nq, m, Nlocs, lv, ord, lp)) return rc;
    std::copy(lv.begin(), lv.end(), level);
    std::copy(ord.begin(), ord.end(), order);
    std::copy(lp.begin(), lp.end(), levptr);
    *n_levels = (int64_t)lp.size() - 1;
    return GPV_OK;
}

// The neighbour lists of the sweep rows by the library's ordered search (gpv_nn.hip) on [the eligible ORDERED observations ;
// the prediction locations], each coordinate divided by `scale` when given: row Nlocs' + i of that search lists the m + 1
// closest among its predecessors and itself; the row's own entry is dropped (a row that does not list itself, being one of
// more than m + 1 coincident points, loses its last entry) and the ids go back to the call's numbering.  hnn: [nq][m] row-major.
static int csim_search(gpv_plan *pl, const double *qlocs, int64_t nq, int m, const double *scale, const unsigned char *eligible_ord,
                       std::vector<int32_t> &hnn, hipStream_t st)
{
    const int64_t n = pl->Nlocs;
    const int dim = pl->dim;
    const int ld = dim <= 3 ? 4 : pl->locs_ld;
    std::vector<double> rec((size_t)n * ld);
    if (GPV_HIP_FAILED(hipMemcpyAsync(rec.data(), pl->d_locs, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, st)) ||
        GPV_HIP_FAILED(hipStreamSynchronize(st)))
        return drain_fail(st, GPV_ERR_HIP);
    std::vector<int32_t> back;                              // compact index -> ORDERED id - 1
    back.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        if (!eligible_ord || eligible_ord[i]) back.push_back((int32_t)i);
    const int64_t ne = (int64_t)back.size(), nt = ne + nq;
    std::vector<double> lc((size_t)nt * dim);
    for (int t = 0; t < dim; ++t) {
        const double sc = scale ? scale[t] : 1.0;
        for (int64_t i = 0; i < ne; ++i) {
            const double x = rec[(size_t)pl->h_newpos[(size_t)back[(size_t)i]] * ld + t];
            lc[(size_t)i + (size_t)t * nt] = scale ? x / sc : x;
        }
        for (int64_t i = 0; i < nq; ++i) {
            const double x = qlocs[i + (int64_t)t * nq];
            lc[(size_t)(ne + i) + (size_t)t * nt] = scale ? x / sc : x;
        }
    }
    std::vector<int> found((size_t)nq * (m + 1));
    if (const int rc = ordered_nn_rows(pl->device, lc.data(), nt, dim, m, ne, nt, found.data(), nq)) return rc;
    hnn.assign((size_t)nq * m, 0);
    for (int64_t i = 0; i < nq; ++i) {
        const int64_t self = ne + i + 1;
        int w = 0;
        for (int s = 0; s <= m && w < m; ++s) {
            const int64_t id = found[(size_t)(i + (int64_t)s * nq)];
            if (id <= 0 || id == self) continue;
            if (id > self) return GPV_ERR_STATE;
            hnn[(size_t)i * m + w++] = id <= ne ? back[(size_t)(id - 1)] + 1 : (int32_t)(n + (id - ne));
        }
    }
    return GPV_OK;
}

// the caller's lists (or none): GPV_ERR_INDEX for an id outside [0, Nlocs + own row], and for more rows than 32-bit ids name
static int csim_check_lists(const int *NNq, int64_t nq, int m, int64_t n)
{
    if (n + nq >= ((int64_t)1 << 31) - 1) return GPV_ERR_INDEX;
    if (NNq)
        for (int64_t i = 0; i < nq; ++i)
            for (int s = 0; s < m; ++s) {
                const int64_t id = NNq[i + (int64_t)s * nq];
                if (id < 0 || id > n + i) return GPV_ERR_INDEX;
            }
    return GPV_OK;
}

// The operator (I - B)^-1 of one call, shared by gpv_plan_cond_sim and gpv_plan_cond_sim_summary: open() takes a validated call
// from the plan's resident records through the search, the level schedule, the uploads and the chunked factor pass (sd goes to
// the caller there); mean_sweep() leaves the means in d_X at cpm columns; draw_sweep() leaves one batch of 16 seeded deviation
// fields in d_X; sweep() is the level-scheduled pass over whatever d_X holds.  Its buffers live as long as the object.
namespace {
struct CsimOp {
    gpv_plan *pl = nullptr;
    hipStream_t st = nullptr;
    int64_t nq = 0, n = 0;
    int m = 0, ncols = 1, cpm = 1, nlev = 0;
    KrigeCall kc;
    CsimFactorArgs f{};
    CsimSweepArgs w{};
    std::vector<int64_t> levptr;
    std::vector<CsimLaunch> launches;
    DevBuf<double> d_q, d_coef, d_sd, d_a, d_X, d_io;
    DevBuf<int32_t> d_nn, d_order, d_levptr;
    DevBuf<unsigned> d_nfail;
    Event ev[2];

    // cpx: the columns of d_X at most; io_cols: the columns of the staging copy d_io (0: none)
    int open(gpv_plan *plan, const double *covparms, int ncovparms, const double *nuggets, int64_t n_nuggets, const double *Z_ord,
             int64_t ldz, int ncols_, const double *qlocs, int64_t nq_, int m_, const int *NNq, const double *scale,
             const unsigned char *eligible_ord, int cpx, int io_cols, double *sd)
    {
        pl = plan; nq = nq_; m = m_; ncols = ncols_; n = pl->Nlocs;
        if (const int rc = enter(pl)) return rc;
        st = pl->stream;
        const int dim = pl->dim;
        if (const int rc = krige_resident(pl, covparms, ncovparms, nuggets, n_nuggets, Z_ord, ldz, ncols, m, kc, f.k, st)) return rc;
        pl->cs_search_ms = pl->cs_factor_ms = pl->cs_sweep_ms = pl->cs_last_sweep_ms = 0.0;
        // the lists, row-major, and the schedule
        std::vector<int32_t> hnn;
        if (NNq) {
            hnn.resize((size_t)nq * m);
            for (int s = 0; s < m; ++s)
                for (int64_t i = 0; i < nq; ++i) hnn[(size_t)i * m + s] = NNq[i + (int64_t)s * nq];
        } else {
            const auto t0 = std::chrono::steady_clock::now();
            if (const int rc = csim_search(pl, qlocs, nq, m, scale, eligible_ord, hnn, st)) return rc;
            pl->cs_search_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        std::vector<int32_t> level, order;
        if (csim_levels_core(hnn.data(), m, 1, nq, m, n, level, order, levptr)) return GPV_ERR_STATE;   // (given lists were checked by the entry)
        nlev = (int)levptr.size() - 1;
        std::vector<int32_t> levptr32(levptr.begin(), levptr.end());
        for (int l = 0; l < nlev; ++l) {
            const bool narrow = levptr[(size_t)l + 1] - levptr[(size_t)l] <= kCsimNarrow;
            if (narrow && !launches.empty() && launches.back().narrow) launches.back().lev1 = l + 1;
            else launches.push_back(CsimLaunch{l, l + 1, narrow});
        }
        // what stays resident for the call
        cpm = whiten_cp(ncols);
        {
            std::vector<double> hq((size_t)nq * dim);
            for (int t = 0; t < dim; ++t)
                for (int64_t i = 0; i < nq; ++i) hq[(size_t)i * dim + t] = qlocs[i + (int64_t)t * nq];
            GPV_BUF(d_q, upload(hq.data(), hq.size()));
        }
        GPV_BUF(d_nn, upload(hnn.data(), hnn.size()));
        GPV_BUF(d_order, upload(order.data(), order.size()));
        GPV_BUF(d_levptr, upload(levptr32.data(), levptr32.size()));
        GPV_BUF(d_coef, resize((size_t)nq * m));
        GPV_BUF(d_sd, resize((size_t)nq));
        GPV_BUF(d_a, resize((size_t)nq * ncols));
        GPV_BUF(d_X, resize((size_t)nq * cpx));
        if (io_cols > 0) GPV_BUF(d_io, resize((size_t)nq * io_cols));
        GPV_BUF(d_nfail, resize(2));
        if (GPV_HIP_FAILED(hipMemsetAsync(d_nfail, 0, sizeof(unsigned), st))) return drain_fail(st, GPV_ERR_HIP);
        for (auto &e : ev) GPV_HIP(hipEventCreate(e.put()));
        // ---- the factor pass
        f.k.nnq = d_nn; f.k.nfail = d_nfail;
        f.qall = d_q; f.nrows = nq; f.Nlocs = n; f.coef = d_coef; f.sd = d_sd; f.a = d_a;
        const int64_t cap = std::min<int64_t>(pl->cs_chunk > 0 ? pl->cs_chunk : kCsimChunk, nq);
        if (GPV_HIP_FAILED(hipEventRecord(ev[0], st))) return drain_fail(st, GPV_ERR_HIP);
        for (int64_t c0 = 0; c0 < nq; c0 += cap) {
            f.row0 = c0;
            f.k.nq = std::min(cap, nq - c0);
            if (GPV_HIP_FAILED(launch_csim_factor(f, krige_grid(f.k.nq, pl->cus), st))) return drain_fail(st, GPV_ERR_HIP);
        }
        if (GPV_HIP_FAILED(hipEventRecord(ev[1], st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipMemcpyAsync(sd, d_sd, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
        {
            float t = 0.f;
            if (hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) pl->cs_factor_ms = (double)t;
        }
        // ---- the sweeps: d_X holds the right-hand sides, then the solution
        w.coef = d_coef; w.nn = d_nn; w.X = d_X; w.order = d_order; w.levptr = d_levptr; w.Nlocs = n; w.m = m;
        return GPV_OK;
    }
    // the level-scheduled pass over d_X at cp columns, between the call's event pair; the caller drains the stream on failure
    int sweep(int cp)
    {
        if (GPV_HIP_FAILED(hipEventRecord(ev[0], st))) return GPV_ERR_HIP;
        for (const CsimLaunch &u : launches)
            if (GPV_HIP_FAILED(u.narrow ? launch_csim_narrow(w, cp, u.lev0, u.lev1, st)
                                        : launch_csim_wide(w, cp, levptr[(size_t)u.lev0], levptr[(size_t)u.lev1], st)))
                return GPV_ERR_HIP;
        if (GPV_HIP_FAILED(hipEventRecord(ev[1], st))) return GPV_ERR_HIP;
        return GPV_OK;
    }
    // after the stream was waited for: the device time of the latest sweep()
    void sweep_time()
    {
        float t = 0.f;
        if (hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) {
            pl->cs_sweep_ms += (double)t;
            pl->cs_last_sweep_ms = (double)t;
        }
    }
    // the means: (I - B)^-1 A, left in d_X[nq][cpm]
    int mean_sweep()
    {
        if (GPV_HIP_FAILED(launch_csim_pack(d_a, nq, nullptr, nq, ncols, cpm, d_X, st))) return GPV_ERR_HIP;
        return sweep(cpm);
    }
    // the deviation fields of the draws base .. base + 15 of the library's generator, left in d_X[nq][16].  Draw j is always made
    // in the batch [16 floor(j / 16), + 16) at CP = 16: its bits depend on (seed, j) alone; the normals of sweep row i are those of
    // the id Nlocs + i, apart from what gpv_plan_simulate draws for the observations
    int draw_sweep(uint64_t seed, int64_t base)
    {
        if (GPV_HIP_FAILED(launch_csim_normals(d_X, d_sd, nq, seed, n, base, st))) return GPV_ERR_HIP;
        return sweep(kCsimMaxCols);
    }
    int failed(int64_t *n_failed)
    {
        unsigned nbad = 0;
        GPV_HIP(hipMemcpy(&nbad, d_nfail, sizeof(nbad), hipMemcpyDeviceToHost));
        *n_failed = (int64_t)nbad;
        return GPV_OK;
    }
};
}  // namespace

// The contract of gpv_plan_krige: buffers that live for the call, no evaluation needed and none disturbed, every refusal before
// the device is touched and before anything is written.  The factor pass may be chunked over the rows (the locations stay
// resident: a row reads those of its list); the sweeps run on what it left.
int gpv_plan_cond_sim(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, const double *nuggets, int64_t n_nuggets,
                      const double *Z_ord, int64_t ldz, int ncols, const double *qlocs, int64_t nq, int m, const int *NNq,
                      const double *scale, const unsigned char *eligible_ord, const double *E, int64_t lde, uint64_t seed, int64_t col0,
                      int64_t nsim, double *mean, int64_t ldm, double *dev, int64_t ldd, double *sd, int64_t *n_levels,
                      int64_t *n_launches, int64_t *n_failed)
{
    constexpr int NB = kCsimMaxCols;
    if (!pl || !covType || !covparms || !nuggets || !n_levels || !n_launches || !n_failed || nq < 0 || m < 1) return GPV_ERR_BAD_ARG;
    if (nsim < 0 || col0 < 0 || col0 > INT64_MAX - nsim) return GPV_ERR_BAD_ARG;
    if (nq > 0 && (!qlocs || !mean || !sd || (nsim > 0 && !dev))) return GPV_ERR_BAD_ARG;
    if (ldm < nq || (nsim > 0 && (ldd < nq || (E && lde < nq)))) return GPV_ERR_BAD_ARG;
    CsimOp op;
    if (const int rc = krige_check_args(pl, covType, covparms, ncovparms, nuggets, n_nuggets, Z_ord, ldz, ncols, scale, op.kc.cs)) return rc;
    if (m + 1 > kKrigeMaxP) return GPV_ERR_UNSUPPORTED_M;
    if (const int rc = krige_check_state(pl, !Z_ord, nullptr, 0)) return rc;
    if (const int rc = csim_check_lists(NNq, nq, m, pl->Nlocs)) return rc;
    *n_failed = 0;
    *n_levels = 0;
    *n_launches = 0;
    if (nq == 0) return GPV_OK;

    const int cpm = whiten_cp(ncols);
    const int cpx = nsim > 0 ? (E ? std::max(cpm, whiten_cp((int)std::min<int64_t>(nsim, NB))) : NB) : cpm;
    if (const int rc = op.open(pl, covparms, ncovparms, nuggets, n_nuggets, Z_ord, ldz, ncols, qlocs, nq, m, NNq, scale, eligible_ord, cpx,
                               std::max(cpx, ncols), sd))
        return rc;
    hipStream_t st = op.st;
    double *const d_X = op.d_X, *const d_io = op.d_io;
    // the means
    if (op.mean_sweep()) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(launch_csim_unpack(d_X, nq, ncols, cpm, d_io, st))) return drain_fail(st, GPV_ERR_HIP);
    if (cols_to_host(mean, ldm, d_io, nq, ncols, st)) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
    op.sweep_time();
    // the deviation fields: (I - B)^-1 D E, sixteen columns at a time
    if (nsim > 0 && E) {
        for (int64_t b0 = 0; b0 < nsim; b0 += NB) {
            const int nb = (int)std::min<int64_t>(NB, nsim - b0), cp = whiten_cp(nb);
            if (cols_to_device(d_io, E + b0 * lde, lde, nq, nb, st)) return drain_fail(st, GPV_ERR_HIP);
            if (GPV_HIP_FAILED(launch_csim_pack(d_io, nq, op.d_sd, nq, nb, cp, d_X, st))) return drain_fail(st, GPV_ERR_HIP);
            if (op.sweep(cp)) return drain_fail(st, GPV_ERR_HIP);
            if (GPV_HIP_FAILED(launch_csim_unpack(d_X, nq, nb, cp, d_io, st))) return drain_fail(st, GPV_ERR_HIP);
            if (cols_to_host(dev + b0 * ldd, ldd, d_io, nq, nb, st)) return drain_fail(st, GPV_ERR_HIP);
            if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
            op.sweep_time();
        }
    } else if (nsim > 0) {
        const int64_t end = col0 + nsim;
        for (int64_t b = col0 / NB; b * NB < end; ++b) {
            const int64_t base = b * NB;
            if (op.draw_sweep(seed, base)) return drain_fail(st, GPV_ERR_HIP);
            if (GPV_HIP_FAILED(launch_csim_unpack(d_X, nq, NB, NB, d_io, st))) return drain_fail(st, GPV_ERR_HIP);
            const int64_t j0 = std::max(base, col0), j1 = std::min(base + NB, end);
            if (cols_to_host(dev + (j0 - col0) * ldd, ldd, d_io + (size_t)(j0 - base) * nq, nq, j1 - j0, st)) return drain_fail(st, GPV_ERR_HIP);
            if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
            op.sweep_time();
        }
    }
    if (const int rc = op.failed(n_failed)) return rc;
    *n_levels = op.nlev;
    *n_launches = (int64_t)op.launches.size();
    return GPV_OK;
}

// ---- summaries of conditional draws, folded on the device (gpv_csim_summary.hip) --------------------------------------------
// The operator of gpv_plan_cond_sim, built once; each batch of 16 seeded draws is swept as there and folded while it is in
// d_X: no unpacking and no copy of nq numbers per batch.  What leaves the device: per batch the region block of the requested
// columns, at the end the per-location moments.
int gpv_plan_cond_sim_summary(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, const double *nuggets,
                              int64_t n_nuggets, const double *Z_ord, int ncols, const double *qlocs, int64_t nq, int m, const int *NNq,
                              const double *scale, const unsigned char *eligible_ord, uint64_t seed, int64_t col0, int64_t ndraws,
                              const double *offset, int link, int nthr, const double *thr, int64_t nreg, const int64_t *regptr,
                              const int32_t *regidx, const double *regw, double *mean, double *sd, double *mc_mean, double *mc_var,
                              double *exceed, double *reg_total, double *reg_max, double *reg_min, double *reg_area, double *reg_weight,
                              int64_t *reg_count, int64_t *n_levels, int64_t *n_launches, int64_t *n_failed)
{
    constexpr int NB = kCsimMaxCols;
    static_assert(kCsumCols == kCsimMaxCols, "the folds read the sweep's rows");
    if (!pl || !covType || !covparms || !nuggets || !n_levels || !n_launches || !n_failed || nq < 0 || m < 1) return GPV_ERR_BAD_ARG;
    if (ncols != 1 || ndraws < 2 || col0 < 0 || col0 > INT64_MAX - ndraws) return GPV_ERR_BAD_ARG;
    if (link < 0 || link > 2 || nthr < 0 || nthr > kCsumMaxThr || (nthr > 0 && !thr)) return GPV_ERR_BAD_ARG;
    if (nq > 0 && (!qlocs || !mean || !sd || !mc_mean || !mc_var || (nthr > 0 && !exceed))) return GPV_ERR_BAD_ARG;
    if (nreg < 0 || nreg >= ((int64_t)1 << 31) - 1) return GPV_ERR_BAD_ARG;
    if (nreg > 0 && (!regptr || !reg_total || !reg_max || !reg_min || (nthr > 0 && !reg_area) || !reg_weight || !reg_count)) return GPV_ERR_BAD_ARG;
    int64_t nnz = 0;
    if (nreg > 0) {
        if (regptr[0] != 0) return GPV_ERR_BAD_ARG;
        for (int64_t r = 0; r < nreg; ++r)
            if (regptr[r + 1] < regptr[r]) return GPV_ERR_BAD_ARG;
        nnz = regptr[nreg];
        if (nnz > 0 && !regidx) return GPV_ERR_BAD_ARG;
        if (regw)
            for (int64_t e = 0; e < nnz; ++e)
                if (!std::isfinite(regw[e])) return GPV_ERR_BAD_ARG;
    }
    CsimOp op;
    if (const int rc = krige_check_args(pl, covType, covparms, ncovparms, nuggets, n_nuggets, Z_ord, pl->Nlocs, ncols, scale, op.kc.cs)) return rc;
    if (m + 1 > kKrigeMaxP) return GPV_ERR_UNSUPPORTED_M;
    if (const int rc = krige_check_state(pl, !Z_ord, nullptr, 0)) return rc;
    if (const int rc = csim_check_lists(NNq, nq, m, pl->Nlocs)) return rc;
    for (int64_t e = 0; e < nnz; ++e)
        if (regidx[e] < 0 || regidx[e] >= nq) return GPV_ERR_INDEX;
    // the chunks of the regions' lists and the regions whose chunks a second launch joins (none, or several)
    std::vector<CsumChunk> chunks;
    std::vector<CsumJoin> joins;
    int64_t nslots = 0;
    for (int64_t r = 0; r < nreg; ++r) {
        const int64_t b = regptr[r], len = regptr[r + 1] - b, nc = (len + kCsumChunkRows - 1) / kCsumChunkRows;
        if (nc > INT32_MAX) return GPV_ERR_INDEX;
        if (nc != 1) joins.push_back(CsumJoin{nslots, (int32_t)nc, (int32_t)r});
        for (int64_t k = 0; k < nc; ++k)
            chunks.push_back(CsumChunk{b + k * kCsumChunkRows, nc == 1 ? -1 : nslots + k,
                                       (int32_t)std::min<int64_t>(kCsumChunkRows, len - k * kCsumChunkRows), (int32_t)r});
        if (nc != 1) nslots += nc;
    }
    *n_failed = 0;
    *n_levels = 0;
    *n_launches = 0;
    pl->cs_fold_ms = pl->cs_last_fold_ms = pl->cs_copy_ms = pl->cs_last_copy_ms = 0.0;
    const int64_t end = col0 + ndraws;
    const double nan = (double)NAN;
    if (nq == 0) {                                      // every region is empty
        std::fill_n(reg_total, (size_t)(nreg * ndraws), 0.0);
        std::fill_n(reg_max, (size_t)(nreg * ndraws), nan);
        std::fill_n(reg_min, (size_t)(nreg * ndraws), nan);
        if (nthr > 0) std::fill_n(reg_area, (size_t)(nreg * ndraws * nthr), 0.0);
        std::fill_n(reg_weight, (size_t)nreg, 0.0);
        std::fill_n(reg_count, (size_t)nreg, (int64_t)0);
        return GPV_OK;
    }

    if (const int rc = op.open(pl, covparms, ncovparms, nuggets, n_nuggets, Z_ord, pl->Nlocs, ncols, qlocs, nq, m, NNq, scale, eligible_ord, NB,
                               0, sd))
        return rc;
    hipStream_t st = op.st;
    const int V = 3 + nthr;
    DevBuf<double> d_mu, d_S, d_off, d_regw, d_part, d_res;
    DevBuf<uint8_t> d_live;
    DevBuf<uint32_t> d_cnt;
    DevBuf<int32_t> d_regidx;
    DevBuf<CsumChunk> d_chunk;
    DevBuf<CsumJoin> d_join;
    GPV_BUF(d_mu, resize((size_t)nq));
    GPV_BUF(d_live, resize((size_t)nq));
    GPV_BUF(d_S, resize((size_t)nq * 2));
    GPV_BUF(d_cnt, resize((size_t)nq * nthr));
    if (offset) GPV_BUF(d_off, upload(offset, (size_t)nq));
    if (nreg > 0) {
        if (nnz > 0) GPV_BUF(d_regidx, upload(regidx, (size_t)nnz));
        if (nnz > 0 && regw) GPV_BUF(d_regw, upload(regw, (size_t)nnz));
        if (!chunks.empty()) GPV_BUF(d_chunk, upload(chunks.data(), chunks.size()));
        if (!joins.empty()) GPV_BUF(d_join, upload(joins.data(), joins.size()));
        GPV_BUF(d_part, resize((size_t)nslots * V * NB));
        GPV_BUF(d_res, resize((size_t)nreg * V * NB));
    }
    Event evf[3];                                       // around the folds of a batch, and behind the copies of its region block
    for (auto &e : evf) GPV_HIP(hipEventCreate(e.put()));
    CsumArgs a{};
    a.X = op.d_X; a.mu = d_mu; a.live = d_live; a.nq = nq; a.nthr = nthr;
    for (int t = 0; t < nthr; ++t) a.thr[t] = thr[t];
    a.S1 = d_S; a.S2 = d_S + nq; a.cnt = d_cnt;
    a.nreg = nreg; a.regidx = d_regidx; a.regw = d_regw; a.chunk = d_chunk; a.nchunks = (int64_t)chunks.size();
    a.join = d_join; a.njoin = (int64_t)joins.size(); a.part = d_part;
    a.rtot = d_res; a.rmax = d_res + (size_t)nreg * NB; a.rmin = d_res + (size_t)nreg * NB * 2; a.rarea = d_res + (size_t)nreg * NB * 3;
    // ---- the means (one column: d_X[nq][1]), mu and the live mask
    if (op.mean_sweep()) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(launch_csum_prepare(op.d_X, d_off, nq, d_mu, d_live, st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipMemsetAsync(d_S, 0, sizeof(double) * (size_t)nq * 2, st))) return drain_fail(st, GPV_ERR_HIP);
    if (nthr > 0 && GPV_HIP_FAILED(hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * (size_t)nq * nthr, st))) return drain_fail(st, GPV_ERR_HIP);
    std::vector<uint8_t> live((size_t)nq);
    if (GPV_HIP_FAILED(hipMemcpyAsync(live.data(), d_live, (size_t)nq, hipMemcpyDeviceToHost, st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
    op.sweep_time();
    for (int64_t r = 0; r < nreg; ++r) {                // once per region, in the order of its list
        double wsum = 0.0;
        int64_t cnt = 0;
        for (int64_t e = regptr[r]; e < regptr[r + 1]; ++e)
            if (live[(size_t)regidx[e]]) {
                wsum += regw ? regw[e] : 1.0;
                ++cnt;
            }
        reg_weight[r] = wsum;
        reg_count[r] = cnt;
    }
    // ---- the batches: normals, sweep, folds, and the region block of the requested columns
    for (int64_t b = col0 / NB; b * NB < end; ++b) {
        const int64_t base = b * NB;
        const int64_t j0 = std::max(base, col0), j1 = std::min(base + NB, end);
        const unsigned colmask = (unsigned)(((1ull << (j1 - base)) - 1ull) & ~((1ull << (j0 - base)) - 1ull));
        if (op.draw_sweep(seed, base)) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipEventRecord(evf[0], st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(launch_csum_accum(a, link, colmask, st))) return drain_fail(st, GPV_ERR_HIP);
        if (nreg > 0 && GPV_HIP_FAILED(launch_csum_fold(a, link, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipEventRecord(evf[1], st))) return drain_fail(st, GPV_ERR_HIP);
        if (nreg > 0) {
            const size_t cols = (size_t)(j1 - j0) * (size_t)nreg, src = (size_t)(j0 - base) * (size_t)nreg, dst = (size_t)(j0 - col0) * (size_t)nreg;
            if (GPV_HIP_FAILED(hipMemcpyAsync(reg_total + dst, a.rtot + src, sizeof(double) * cols, hipMemcpyDeviceToHost, st)) ||
                GPV_HIP_FAILED(hipMemcpyAsync(reg_max + dst, a.rmax + src, sizeof(double) * cols, hipMemcpyDeviceToHost, st)) ||
                GPV_HIP_FAILED(hipMemcpyAsync(reg_min + dst, a.rmin + src, sizeof(double) * cols, hipMemcpyDeviceToHost, st)) ||
                (nthr > 0 && GPV_HIP_FAILED(hipMemcpyAsync(reg_area + dst * nthr, a.rarea + src * nthr, sizeof(double) * cols * nthr,
                                                           hipMemcpyDeviceToHost, st))))
                return drain_fail(st, GPV_ERR_HIP);
        }
        if (GPV_HIP_FAILED(hipEventRecord(evf[2], st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
        op.sweep_time();
        float t = 0.f;
        if (hipEventElapsedTime(&t, evf[0], evf[1]) == hipSuccess) {
            pl->cs_fold_ms += (double)t;
            pl->cs_last_fold_ms = (double)t;
        }
        if (hipEventElapsedTime(&t, evf[1], evf[2]) == hipSuccess) {
            pl->cs_copy_ms += (double)t;
            pl->cs_last_copy_ms = (double)t;
        }
    }
    // ---- the per-location results, staged in d_X: the last batch is folded
    double *const d_out = op.d_X;
    if (GPV_HIP_FAILED(launch_csum_finish(a, link, ndraws, d_out, st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipMemcpyAsync(mean, d_out, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, st)) ||
        GPV_HIP_FAILED(hipMemcpyAsync(mc_mean, d_out + nq, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, st)) ||
        GPV_HIP_FAILED(hipMemcpyAsync(mc_var, d_out + 2 * nq, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, st)) ||
        (nthr > 0 && GPV_HIP_FAILED(hipMemcpyAsync(exceed, d_out + 3 * nq, sizeof(double) * (size_t)nq * nthr, hipMemcpyDeviceToHost, st))))
        return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
    if (const int rc = op.failed(n_failed)) return rc;
    *n_levels = op.nlev;
    *n_launches = (int64_t)op.launches.size();
    return GPV_OK;
}

// developer aids (tools/cond_sim_timing.py and the tests; not part of the public header): the rows per launch of the factor
// pass of the plan's following gpv_plan_cond_sim calls (0: the default), which changes no bit of a result; and the times of the
// latest call: {search (host clock), factor pass, all sweeps, the last sweep} in milliseconds, the last three device time by
// event pairs
extern "C" int gpv_plan_debug_csim_chunk(gpv_plan *pl, int64_t chunk)
{
    if (!pl || chunk < 0) return GPV_ERR_BAD_ARG;
    pl->cs_chunk = chunk;
    return GPV_OK;
}

extern "C" int gpv_plan_debug_csim_ms(gpv_plan *pl, double *ms)
{
    if (!pl || !ms) return GPV_ERR_BAD_ARG;
    ms[0] = pl->cs_search_ms;
    ms[1] = pl->cs_factor_ms;
    ms[2] = pl->cs_sweep_ms;
    ms[3] = pl->cs_last_sweep_ms;
    return GPV_OK;
}

// the folds of the latest gpv_plan_cond_sim_summary: {folds of all batches, of the last batch, the copies of the region blocks of
// all batches, of the last batch} in milliseconds, device time by event pairs around the accumulation and the region fold
// alone, and from there to behind the copies (the sweeps of that call: gpv_plan_debug_csim_ms)
extern "C" int gpv_plan_debug_csim_summary_ms(gpv_plan *pl, double *ms)
{
    if (!pl || !ms) return GPV_ERR_BAD_ARG;
    ms[0] = pl->cs_fold_ms;
    ms[1] = pl->cs_last_fold_ms;
    ms[2] = pl->cs_copy_ms;
    ms[3] = pl->cs_last_copy_ms;
    return GPV_OK;
}

// LincombArgs::lrec from the plan's structure as it lives on the device (built on the first gpv_plan_lincomb after a
// gpv_plan_build_posterior: plans that never ask for variances pay nothing).  The row lists are rebuilt exactly as
// build_posterior_impl lays them out (columns ascending, the column itself first), so that the positions the column records
// name are these.
static int lincomb_prepare(gpv_plan *pl)
{
    const int64_t n = pl->Nlocs;
    const size_t nnz = (size_t)pl->post_nnz;
    std::vector<int32_t> colptr((size_t)n + 1), crow(nnz), cboff((size_t)n);
    std::vector<int2> topinfo((size_t)pl->top_K);
    GPV_HIP(hipMemcpy(colptr.data(), pl->d_colptr, colptr.size() * 4, hipMemcpyDeviceToHost));
    if (nnz) GPV_HIP(hipMemcpy(crow.data(), pl->d_crow, nnz * 4, hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(cboff.data(), pl->d_cboff, cboff.size() * 4, hipMemcpyDeviceToHost));
    if (pl->top_K > 0) GPV_HIP(hipMemcpy(topinfo.data(), pl->d_topinfo, topinfo.size() * sizeof(int2), hipMemcpyDeviceToHost));
    if ((size_t)colptr[(size_t)n] != nnz) return GPV_ERR_STATE;
    std::vector<uint8_t> in_top((size_t)n, 0);
    for (const int2 &t : topinfo) {
        if (t.x < 0 || t.x >= n) return GPV_ERR_STATE;
        in_top[(size_t)t.x] = 1;
    }
    std::vector<int32_t> fill((size_t)n + 1, 0);
    for (size_t e = 0; e < nnz; ++e) {
        if (crow[e] < 0 || crow[e] >= n) return GPV_ERR_STATE;
        fill[(size_t)crow[e] + 1]++;
    }
    for (int64_t i = 0; i < n; ++i) fill[(size_t)i + 1] += fill[(size_t)i];
    std::vector<int2> lrec(nnz ? nnz : 1);
    for (int64_t c = 0; c < n; ++c)
        for (int32_t e = colptr[(size_t)c]; e < colptr[(size_t)c + 1]; ++e) {
            const int32_t i = crow[(size_t)e];
            lrec[(size_t)fill[(size_t)i]++] = make_int2(in_top[(size_t)c] ? ~(int32_t)c : (int32_t)c,
                                                        cboff[(size_t)c] + 1 + (e - colptr[(size_t)c]));
        }
    GPV_BUF(pl->d_lc_rec, upload(lrec.data(), lrec.size()));
    GPV_BUF(pl->d_lc_X, ensure((size_t)n * kLincombNB));
    GPV_BUF(pl->d_lc_part, ensure((size_t)kLincombBlocks * kLincombNB));
    GPV_BUF(pl->d_lc_vars, ensure(kLincombNB));
    pl->lc_ready = true;
    return GPV_OK;
}

int gpv_plan_lincomb(gpv_plan *pl, int64_t nrows, const int64_t *hptr, const int32_t *hidx, const double *hval, double *vars,
                     double *cov)
{
    constexpr int NB = kLincombNB;
    if (!pl || nrows < 0 || !hptr || !vars) return GPV_ERR_BAD_ARG;
    if (cov && nrows > NB) return GPV_ERR_BAD_ARG;
    if (hptr[0] < 0) return GPV_ERR_BAD_ARG;
    for (int64_t r = 0; r < nrows; ++r)
        if (hptr[r + 1] < hptr[r]) return GPV_ERR_BAD_ARG;
    const int64_t h0 = hptr[0], hnnz = hptr[nrows] - h0;
    if (hnnz > 0 && (!hidx || !hval)) return GPV_ERR_BAD_ARG;
    // per batch: the longest row, and whether some row repeats an index (rows that ascend strictly cannot)
    const int64_t nbatch = (nrows + NB - 1) / NB;
    std::vector<int64_t> bmax((size_t)nbatch, 0);
    std::vector<uint8_t> bserial((size_t)nbatch, 0);
    for (int64_t r = 0; r < nrows; ++r) {
        bool ascending = true;
        for (int64_t q = hptr[r]; q < hptr[r + 1]; ++q) {
            if (hidx[q] < 0 || (int64_t)hidx[q] >= pl->Nlocs) return GPV_ERR_INDEX;
            if (q > hptr[r] && hidx[q] <= hidx[q - 1]) ascending = false;
        }
        if (!ascending) {                                    // no repeat after all?  (sorted copy of the row)
            std::vector<int32_t> tmp(hidx + hptr[r], hidx + hptr[r + 1]);
            std::sort(tmp.begin(), tmp.end());
            if (std::adjacent_find(tmp.begin(), tmp.end()) != tmp.end()) bserial[(size_t)(r / NB)] = 1;
        }
        bmax[(size_t)(r / NB)] = std::max(bmax[(size_t)(r / NB)], hptr[r + 1] - hptr[r]);
    }
    if (!pl->have_post || !pl->have_factor || pl->comm) return GPV_ERR_STATE;
    if (nrows == 0) return GPV_OK;
    if (const int rc = enter_final(pl)) return rc;
    if (!pl->lc_ready) {
        const int rc = lincomb_prepare(pl);
        if (rc != GPV_OK) return rc;
    }
    hipStream_t st = pl->stream;
    DevBuf<int64_t> d_hptr;                                                   // this call's rows (freed when it returns)
    DevBuf<int32_t> d_hidx;
    DevBuf<double> d_hval;
    std::vector<int64_t> hp((size_t)nrows + 1);
    for (int64_t r = 0; r <= nrows; ++r) hp[(size_t)r] = hptr[r] - h0;        // offsets into the uploaded slice
    if (GPV_BUF_FAILED(d_hptr, upload(hp.data(), hp.size())) || GPV_BUF_FAILED(d_hidx, upload(hnnz ? hidx + h0 : nullptr, (size_t)hnnz)) ||
        GPV_BUF_FAILED(d_hval, upload(hnnz ? hval + h0 : nullptr, (size_t)hnnz)))
        return drain_fail(st, GPV_ERR_HIP);
    if (cov && (GPV_BUF_FAILED(pl->d_lc_gpart, ensure((size_t)kLincombBlocks * NB * NB)) || GPV_BUF_FAILED(pl->d_lc_gram, ensure(NB * NB))))
        return drain_fail(st, GPV_ERR_HIP);
    LincombArgs la;
    la.colrec = pl->d_colrec; la.lrec = pl->d_lc_rec; la.C = pl->d_C; la.X = pl->d_lc_X;
    // the sweep: the factor pass's levels, leaves first, then the dense top block, then the column sums
    auto enqueue = [&]() -> hipError_t {
        hipError_t e = hipSuccess;
        for (size_t lv = 0; e == hipSuccess && lv + 1 < pl->levptr.size(); ++lv)
            e = launch_lincomb_level(la, pl->levptr[lv], pl->levptr[lv + 1] - pl->levptr[lv], lv == 0, st);
        if (e == hipSuccess && pl->top_K > 0)
            e = launch_lincomb_top(la, (int)(pl->Nlocs - pl->top_K), pl->top_K, pl->d_topinfo, pl->d_toprows, st);
        if (e == hipSuccess) e = launch_lincomb_vars(pl->d_lc_X, pl->Nlocs, pl->d_lc_part, pl->d_lc_vars, st);
        return e;
    };
    std::vector<double> vb((size_t)NB), gb(cov ? (size_t)NB * NB : 0);
    for (int64_t b = 0; b < nbatch; ++b) {
        const int64_t row0 = b * NB;
        const int nb = (int)std::min<int64_t>(NB, nrows - row0);
        if (GPV_HIP_FAILED(launch_lincomb_init(pl->d_lc_X, pl->Nlocs, d_hptr, d_hidx, d_hval, row0, nb, bmax[(size_t)b],
                                               bserial[(size_t)b] != 0, st)))
            return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(graph_replay(pl->lc_graph, st, enqueue))) return drain_fail(st, GPV_ERR_HIP);
        if (cov && GPV_HIP_FAILED(launch_lincomb_gram(pl->d_lc_X, pl->Nlocs, pl->d_lc_gpart, pl->d_lc_gram, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipMemcpyAsync(vb.data(), pl->d_lc_vars, sizeof(double) * NB, hipMemcpyDeviceToHost, st))) return drain_fail(st, GPV_ERR_HIP);
        if (cov && GPV_HIP_FAILED(hipMemcpyAsync(gb.data(), pl->d_lc_gram, sizeof(double) * NB * NB, hipMemcpyDeviceToHost, st)))
            return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
        for (int j = 0; j < nb; ++j) vars[row0 + j] = vb[(size_t)j];
        if (cov)
            for (int i = 0; i < nb; ++i)
                for (int j = 0; j < nb; ++j) cov[(int64_t)i * nrows + j] = gb[(size_t)i * NB + j];
    }
    pl->last_stream = st;
    return GPV_OK;
}

// the transposed sweep on d_lc_X: the dense top block, then the mean sweep's levels in ascending order, one launch each
static hipError_t solvet_enqueue(gpv_plan *pl, hipStream_t st)
{
    SolveTArgs sa;
    sa.meanrec = pl->d_meanrec; sa.crow = pl->d_crow; sa.C = pl->d_C; sa.X = pl->d_lc_X;
    hipError_t e = hipSuccess;
    if (pl->top_K > 0) e = launch_solvet_top(sa, pl->top_K, pl->d_topinfo, pl->d_toprows, st);
    for (size_t lv = 0; e == hipSuccess && lv + 1 < pl->levptr2.size(); ++lv)
        e = launch_solvet_level(sa, pl->levptr2[lv], pl->levptr2[lv + 1] - pl->levptr2[lv], st);
    return e;
}
// ... as the plan's captured graph
static hipError_t solvet_sweep(gpv_plan *pl, hipStream_t st)
{
    return graph_replay(pl->st_graph, st, [&] { return solvet_enqueue(pl, st); });
}

int gpv_plan_solve_t(gpv_plan *pl, int64_t ncols, const double *E, int64_t lde, double *X, int64_t ldx)
{
    constexpr int NB = kLincombNB;
    if (!pl || ncols < 0 || !E || !X) return GPV_ERR_BAD_ARG;
    const int64_t n = pl->Nlocs;
    if (lde < n || ldx < n) return GPV_ERR_BAD_ARG;
    if (const int rc = posterior_factor_state(pl)) return rc;
    if (ncols == 0) return GPV_OK;
    if (const int rc = enter_final(pl)) return rc;
    GPV_BUF(pl->d_lc_X, ensure((size_t)n * NB));
    GPV_BUF(pl->d_st_E, ensure((size_t)n * NB));
    hipStream_t st = pl->stream;
    const int64_t nbatch = (ncols + NB - 1) / NB;
    for (int64_t b = 0; b < nbatch; ++b) {
        const int64_t col0 = b * NB;
        const int nb = (int)std::min<int64_t>(NB, ncols - col0);
        if (cols_to_device(pl->d_st_E, E + col0 * lde, lde, n, nb, st)) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(launch_solvet_pack(pl->d_lc_X, pl->d_st_E, n, n, nb, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(solvet_sweep(pl, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(launch_solvet_unpack(pl->d_lc_X, pl->d_st_E, n, n, nb, st))) return drain_fail(st, GPV_ERR_HIP);
        if (cols_to_host(X + col0 * ldx, ldx, pl->d_st_E, n, nb, st)) return drain_fail(st, GPV_ERR_HIP);   // (X may be E: the batch was read before)
        if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
    }
    pl->last_stream = st;
    return GPV_OK;
}

// developer aid (tools/lincomb_timing.py; not part of the public header): device time of `reps` transposed sweeps over a full
// batch, each on a fresh copy of what the latest gpv_plan_solve_t left in the staging buffer (the time does not depend on the
// values), by a pair of events around the sweep alone: no packing, no copies
extern "C" int gpv_plan_debug_solve_t_ms(gpv_plan *pl, int reps, double *ms)
{
    if (!pl || reps <= 0 || !ms) return GPV_ERR_BAD_ARG;
    if (!pl->have_post || !pl->have_factor || pl->comm || !pl->d_lc_X || !pl->d_st_E) return GPV_ERR_STATE;
    // (the one timed entry that does not wait for the stream of the latest evaluation; the pack ahead of each run is untimed)
    return timed_reps(pl, false, reps, ms, [&] { return solvet_sweep(pl, pl->stream); },
                      [&] { return launch_solvet_pack(pl->d_lc_X, pl->d_st_E, pl->Nlocs, pl->Nlocs, kLincombNB, pl->stream); });
}

// ---- the selected inverse of the factor: every posterior variance in one pass (gpv_selinv.hip) -------------------------------
// The records of the pass from the plan's structure as it lives on the device (built on the first gpv_plan_selinv after a
// gpv_plan_build_posterior: plans that never ask pay nothing): the row lists are rebuilt as build_posterior_impl lays them
// out, which gives every entry of a column the row-list position of its pair and with it the pair's match records; the terms
// the pattern drops are counted here, once: they depend on the structure alone.
static int selinv_prepare(gpv_plan *pl)
{
    const int64_t n = pl->Nlocs;
    const size_t nnz = (size_t)pl->post_nnz, K = (size_t)pl->top_K;
    if (nnz < (size_t)n || K > (size_t)kSelinvTopMax || K > (size_t)n) return GPV_ERR_STATE;
    std::vector<int32_t> colptr((size_t)n + 1), crow(nnz), cboff((size_t)n);
    std::vector<int2> topinfo(K);
    std::vector<int4> rowrec(nnz), rec((size_t)n);
    GPV_HIP(hipMemcpy(colptr.data(), pl->d_colptr, colptr.size() * 4, hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(crow.data(), pl->d_crow, nnz * 4, hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(cboff.data(), pl->d_cboff, cboff.size() * 4, hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(rowrec.data(), pl->d_rowrec, nnz * sizeof(int4), hipMemcpyDeviceToHost));
    if (K > 0) GPV_HIP(hipMemcpy(topinfo.data(), pl->d_topinfo, K * sizeof(int2), hipMemcpyDeviceToHost));
    if ((size_t)n > K) GPV_HIP(hipMemcpy(rec.data() + K, pl->d_meanrec, ((size_t)n - K) * sizeof(int4), hipMemcpyDeviceToHost));
    if (colptr[0] != 0 || (size_t)colptr[(size_t)n] != nnz) return GPV_ERR_STATE;
    int64_t c_entries = 0;
    for (int64_t c = 0; c < n; ++c) {
        const int32_t cn = colptr[(size_t)c + 1] - colptr[(size_t)c];
        if (cn < 1 || cn > 64 || cboff[(size_t)c] < 0 || crow[(size_t)colptr[(size_t)c + 1] - 1] != (int32_t)c) return GPV_ERR_STATE;
        c_entries = std::max<int64_t>(c_entries, (int64_t)cboff[(size_t)c] + cn + 1);
    }
    for (size_t j = 0; j < K; ++j) {                          // the top block: ascending, before the schedule
        const int32_t k = topinfo[j].x;
        if (k < 0 || k >= n || (j > 0 && k <= topinfo[j - 1].x)) return GPV_ERR_STATE;
        rec[j] = make_int4(k, cboff[(size_t)k], colptr[(size_t)k + 1] - colptr[(size_t)k], colptr[(size_t)k]);
    }
    for (size_t i = K; i < (size_t)n; ++i) {                  // (the schedule's records name the same columns' own numbers)
        const int4 r = rec[i];
        if (r.x < 0 || r.x >= n || r.y != cboff[(size_t)r.x] || r.w != colptr[(size_t)r.x] ||
            r.z != colptr[(size_t)r.x + 1] - colptr[(size_t)r.x])
            return GPV_ERR_STATE;
    }
    std::vector<int32_t> fill((size_t)n + 1, 0);
    for (size_t e = 0; e < nnz; ++e) {
        if (crow[e] < 0 || crow[e] >= n) return GPV_ERR_STATE;
        fill[(size_t)crow[e] + 1]++;
    }
    for (int64_t i = 0; i < n; ++i) fill[(size_t)i + 1] += fill[(size_t)i];
    std::vector<int2> pair(nnz);
    int64_t tp_size = 0;
    for (int64_t c = 0; c < n; ++c) {
        const int32_t b0 = colptr[(size_t)c], cn = colptr[(size_t)c + 1] - b0;
        for (int32_t e = 0; e < cn; ++e) {
            const int32_t i = crow[(size_t)(b0 + e)];
            const int4 rr = rowrec[(size_t)fill[(size_t)i]++];                       // the pair (row i, column c)
            if (rr.x != cboff[(size_t)c] || (rr.z & 0xFF) != e || rr.y < 0) return GPV_ERR_STATE;
            pair[(size_t)(b0 + e)] = make_int2(cboff[(size_t)i], e + 1 < cn ? rr.y : 0);
            if (e + 1 < cn) tp_size = std::max<int64_t>(tp_size, (int64_t)rr.y + e + 1);
        }
    }
    // the match records: a position must lie inside the column it names (the kernels index Sigma with it); 0xFF = a dropped term
    std::vector<uint8_t> tp((size_t)tp_size);
    if (tp_size > 0) GPV_HIP(hipMemcpy(tp.data(), pl->d_tp, (size_t)tp_size, hipMemcpyDeviceToHost));
    int64_t dropped = 0;
    for (int64_t c = 0; c < n; ++c) {
        const int32_t b0 = colptr[(size_t)c], cn = colptr[(size_t)c + 1] - b0;
        for (int32_t ek = 0; ek + 1 < cn; ++ek) {
            const int32_t i = crow[(size_t)(b0 + ek)], in = colptr[(size_t)i + 1] - colptr[(size_t)i];
            const uint8_t *t = tp.data() + pair[(size_t)(b0 + ek)].y;
            for (int32_t e = 0; e <= ek; ++e) {
                if (t[e] == 0xFF) ++dropped;
                else if ((int32_t)t[e] >= in) return GPV_ERR_STATE;
            }
            if ((int32_t)t[ek] != in - 1) return GPV_ERR_STATE;                      // (row i of column i: its diagonal, last)
        }
    }
    const size_t nlev = pl->levptr2.size() > 0 ? pl->levptr2.size() - 1 : 0;
    if (nlev > 0 && (size_t)pl->levptr2[nlev] != (size_t)n - K) return GPV_ERR_STATE;
    pl->sel_lev_tile.assign(nlev, 16);
    for (size_t lv = 0; lv < nlev; ++lv) {
        int mx = 1;
        for (int32_t i = pl->levptr2[lv]; i < pl->levptr2[lv + 1]; ++i) mx = std::max(mx, rec[K + (size_t)i].z);
        pl->sel_lev_tile[lv] = selinv_tile(mx);
    }
    pl->sel_graph.reset();
    GPV_BUF(pl->d_sel_rec, upload(rec.data(), rec.size()));
    GPV_BUF(pl->d_sel_pair, upload(pair.data(), pair.size()));
    GPV_BUF(pl->d_sel_S, resize((size_t)c_entries));
    GPV_BUF(pl->d_sel_vars, resize((size_t)n));
    GPV_BUF(pl->d_sel_out, resize((size_t)n));
    GPV_HIP(hipMemset(pl->d_sel_S, 0, sizeof(double) * (size_t)c_entries));
    pl->sel_dropped = dropped;
    pl->sel_ready = true;
    return GPV_OK;
}

// the pass: the dense top block, then the mean sweep's levels in ascending order, one launch each
static hipError_t selinv_enqueue(gpv_plan *pl, hipStream_t st)
{
    SelinvArgs a;
    a.rec = pl->d_sel_rec; a.pair = pl->d_sel_pair; a.tp = pl->d_tp; a.C = pl->d_C; a.S = pl->d_sel_S; a.vars = pl->d_sel_vars;
    hipError_t e = launch_selinv_top(a, pl->top_K, pl->d_toprows, st);
    for (size_t lv = 0; e == hipSuccess && lv < pl->sel_lev_tile.size(); ++lv)
        e = launch_selinv_level(a, pl->top_K + pl->levptr2[lv], pl->levptr2[lv + 1] - pl->levptr2[lv], pl->sel_lev_tile[lv], st);
    return e;
}
// ... as the plan's captured graph
static hipError_t selinv_sweep(gpv_plan *pl, hipStream_t st)
{
    return graph_replay(pl->sel_graph, st, [&] { return selinv_enqueue(pl, st); });
}

// Reads C and the structure and writes buffers of its own: the factor, its stamp and every later result of the plan stay what
// they were.
int gpv_plan_selinv(gpv_plan *pl, int64_t skip_front, double *vars_ord, int64_t *n_dropped)
{
    if (!pl || !vars_ord || !n_dropped) return GPV_ERR_BAD_ARG;
    if (skip_front < 0 || skip_front >= pl->Nlocs) return GPV_ERR_BAD_ARG;
    if (const int rc = posterior_factor_state(pl)) return rc;
    if (const int rc = enter_final(pl)) return rc;
    if (!pl->sel_ready)
        if (const int rc = selinv_prepare(pl)) return rc;
    hipStream_t st = pl->stream;
    if (GPV_HIP_FAILED(selinv_sweep(pl, st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(launch_selinv_out(pl->d_sel_vars, pl->Nlocs, skip_front, pl->d_sel_out, st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipMemcpyAsync(vars_ord, pl->d_sel_out, sizeof(double) * (size_t)pl->Nlocs, hipMemcpyDeviceToHost, st)))
        return drain_fail(st, GPV_ERR_HIP);
    GPV_HIP(hipStreamSynchronize(st));
    *n_dropped = pl->sel_dropped;
    pl->last_stream = st;
    return GPV_OK;
}

// developer aid (tools/selinv_timing.py; not part of the public header): device time of `reps` passes on the factor the latest
// gpv_plan_selinv read, by a pair of events around the pass alone: no copies
extern "C" int gpv_plan_debug_selinv_ms(gpv_plan *pl, int reps, double *ms)
{
    if (!pl || reps <= 0 || !ms) return GPV_ERR_BAD_ARG;
    if (const int rc = posterior_factor_state(pl)) return rc;
    if (!pl->sel_ready) return GPV_ERR_STATE;
    return timed_reps(pl, true, reps, ms, [&] { return selinv_sweep(pl, pl->stream); });
}

// ---- value and analytic gradient of the cond.yz='SGV' log-likelihood (gpv_grad_sgv.hip) ---------------------------------------
// The index data of the pass from the plan's arrays as they live on the device (built on the first call after a
// gpv_plan_build_posterior): for every stored set the record of its posterior column, and for every entry of the set the
// position of its point among the column's entries.  Every position is found in the column itself and checked against it:
// the latent entries of a set must be the entries of its column, one each, the set's own point last; the kernel indexes its
// tile of Sigma and the match records with them.
static int sgv_prepare(gpv_plan *pl)
{
    const int64_t n = pl->Nlocs, rows = pl->rows;
    const int P = pl->P;
    const size_t nnz = (size_t)pl->post_nnz;
    if (rows != n || pl->h_newpos.size() != (size_t)n || nnz < (size_t)n) return GPV_ERR_STATE;
    std::vector<int32_t> nn((size_t)rows * P), rid((size_t)rows), colptr((size_t)n + 1), crow(nnz), cboff((size_t)n), inv((size_t)n, -1);
    std::vector<uint8_t> cd((size_t)rows * P);
    GPV_HIP(hipMemcpy(nn.data(), pl->d_nn, nn.size() * 4, hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(cd.data(), pl->d_cond, cd.size(), hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(rid.data(), pl->d_rowid, rid.size() * 4, hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(colptr.data(), pl->d_colptr, colptr.size() * 4, hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(crow.data(), pl->d_crow, nnz * 4, hipMemcpyDeviceToHost));
    GPV_HIP(hipMemcpy(cboff.data(), pl->d_cboff, cboff.size() * 4, hipMemcpyDeviceToHost));
    if (colptr[0] != 0 || (size_t)colptr[(size_t)n] != nnz) return GPV_ERR_STATE;
    for (int64_t i = 0; i < n; ++i) {                         // ordered index of every internal position
        const int32_t r = pl->h_newpos[(size_t)i];
        if (r < 0 || r >= n || inv[(size_t)r] != -1) return GPV_ERR_STATE;
        inv[(size_t)r] = (int32_t)i;
    }
    std::vector<uint8_t> cpos((size_t)rows * P, (uint8_t)0xFF);
    std::vector<int4> rec((size_t)rows);
    for (int64_t r = 0; r < rows; ++r) {
        const int32_t k = rid[(size_t)r];
        if (k < 0 || k >= n) return GPV_ERR_STATE;
        const int32_t b0 = colptr[(size_t)k], cn = colptr[(size_t)k + 1] - b0;
        if (cn < 1 || cn > kGradMaxP || b0 < 0 || (size_t)b0 + (size_t)cn > nnz || cboff[(size_t)k] < 0) return GPV_ERR_STATE;
        const int32_t *col = crow.data() + b0;
        unsigned long long seen = 0ull;
        for (int t = 0; t < P; ++t) {
            const int32_t v = nn[(size_t)r * P + t];
            if (v < 0 || !(cd[(size_t)r * P + t] & 1u)) continue;
            if (v >= n) return GPV_ERR_STATE;
            const int32_t *at = std::lower_bound(col, col + cn, inv[(size_t)v]);
            if (at == col + cn || *at != inv[(size_t)v]) return GPV_ERR_STATE;      // a latent entry outside the column
            const int pos = (int)(at - col);
            const int stored = cd[(size_t)r * P + t] >> 1;                           // (the set kernel's own record, where it has one)
            if ((seen >> pos) & 1ull || (stored != 0 && stored != pos + 1)) return GPV_ERR_STATE;
            seen |= 1ull << pos;
            cpos[(size_t)r * P + t] = (uint8_t)pos;
        }
        if (seen != (cn == 64 ? ~0ull : (1ull << cn) - 1ull)) return GPV_ERR_STATE;  // every entry of the column, once
        if (cpos[(size_t)r * P + P - 1] != (uint8_t)(cn - 1) || col[cn - 1] != k) return GPV_ERR_STATE;   // the own point: last
        rec[(size_t)r] = make_int4(cboff[(size_t)k], b0, cn, k);
    }
    GPV_BUF(pl->d_sgv_cpos, upload(cpos.data(), cpos.size()));
    GPV_BUF(pl->d_sgv_rec, upload(rec.data(), rec.size()));
    pl->sgv_ready = true;
    return GPV_OK;
}

// Unlike the 'z' entries this one EVALUATES the plan: an evaluation with GPV_WANT_MEAN at these parameters, the selected
// inverse of its factor, then the per-set pass; the plan's last evaluation afterwards is that evaluation.
int gpv_plan_loglik_grad_sgv(gpv_plan *pl, const char *covType, const double *covparms, int ncovparms, double nugget, double *loglik,
                             double *grad, int64_t *n_failed, double *col_terms)
{
    if (!pl || !covType || !covparms || !loglik || !grad || !n_failed) return GPV_ERR_BAD_ARG;
    if (std::strcmp(covType, "matern_scaledim") == 0) return GPV_ERR_UNSUPPORTED_NU;
    bool matern;
    SgvGradArgs sa;
    GradArgs &a = sa.g;
    CovSetup cs;
    int rc = grad_args_checked(pl, covType, covparms, ncovparms, nugget, false, matern, a, cs, false, true);
    if (rc != GPV_OK) return rc;
    if (!pl->have_post || pl->post_filled || pl->post_ld > 64 || !pl->d_meanrec || pl->row_begin != 0) return GPV_ERR_STATE;
    // the structure's own facts, established once: the terms its selected inverse drops (none for SGV) and the index data.
    // They read the plan's arrays and write buffers of their own; a refusal here leaves every result of the plan as it was.
    if ((rc = enter_final(pl)) != GPV_OK) return rc;
    if (!pl->sel_ready && (rc = selinv_prepare(pl)) != GPV_OK) return rc;
    if (pl->sel_dropped > 0) return GPV_ERR_STATE;
    if (!pl->sgv_ready && (rc = sgv_prepare(pl)) != GPV_OK) return rc;
    const int grid = grad_sgv_grid(pl->p, pl->rows, pl->cus);
    if (!pl->d_sgv_part || pl->sgv_grid < grid) {
        GPV_BUF(pl->d_sgv_part, resize(kSgvNV * (size_t)grid));
        pl->sgv_grid = grid;
    }
    GPV_BUF(pl->d_sgv_tot, ensure(kSgvNV));
    if (col_terms) GPV_BUF(pl->d_sgv_rows, ensure(kSgvRowLd * (size_t)pl->rows));
    // the evaluation, on the plan's stream; its sums, mean, U entries and factor stamp are what the caller finds afterwards
    if ((rc = plan_eval_checked(pl, cs, &nugget, 1, GPV_WANT_MEAN, nullptr, nullptr)) != GPV_OK) return rc;
    hipStream_t st = pl->stream;
    if (GPV_HIP_FAILED(selinv_sweep(pl, st))) return drain_fail(st, GPV_ERR_HIP);
    a.row_terms = col_terms ? pl->d_sgv_rows.get() : nullptr;
    a.block_part = pl->d_sgv_part; a.totals = pl->d_sgv_tot;
    sa.cpos = pl->d_sgv_cpos; sa.setrec = pl->d_sgv_rec; sa.crow = pl->d_crow;
    sa.pair = pl->d_sel_pair; sa.tp = pl->d_tp; sa.S = pl->d_sel_S; sa.vars = pl->d_sel_vars; sa.mu = pl->d_u;
    double tot[kSgvNV];
    if (GPV_HIP_FAILED(launch_grad_sgv(pl->p, sa, grid, st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipMemcpyAsync(tot, pl->d_sgv_tot, sizeof(tot), hipMemcpyDeviceToHost, st))) return drain_fail(st, GPV_ERR_HIP);
    GPV_HIP(hipStreamSynchronize(st));
    double sums[kNSums];
    if ((rc = gpv_plan_get_sums(pl, sums)) != GPV_OK) return rc;
    // kernel parameters -> covparms: matern {variance, range, - (NaN), nugget}, esqe {variance 1, range 1, variance 2, range 2, nugget}
    const int nk = matern ? 3 : 5, np = ncovparms + 1;
    const int at[5] = {0, 1, matern ? 3 : 2, 3, 4};
    auto spread = [&](const double *src, double *dst) {
        for (int t = 0; t < np; ++t) dst[t] = NAN;
        for (int t = 0; t < nk; ++t) dst[at[t]] = src[t];
    };
    *n_failed = (int64_t)tot[6];
    if (tot[6] > 0.0) {
        *loglik = -INFINITY;
        for (int t = 0; t < np; ++t) grad[t] = NAN;
    } else {
        if ((rc = gpv_loglik_from_sums(sums, pl->Nlocs, loglik)) != GPV_OK) return rc;
        spread(tot, grad);
    }
    if (col_terms) {
        std::vector<double> h((size_t)pl->rows * kSgvRowLd);
        GPV_HIP(hipMemcpy(h.data(), pl->d_sgv_rows, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < pl->rows; ++k) spread(&h[(size_t)k * kSgvRowLd], col_terms + k * np);
    }
    return GPV_OK;
}

// ---- Monte-Carlo summaries of posterior draws: normals made on the device, the transposed sweep, fused sums ------------------
int gpv_draws_normals_host(uint64_t seed, int64_t k0, int64_t nk, int64_t col0, int64_t ncols, double *E, int64_t lde)
{
    if (!E || k0 < 0 || nk < 0 || col0 < 0 || ncols < 0 || lde < nk) return GPV_ERR_BAD_ARG;
    if (nk == 0 || ncols == 0) return GPV_OK;
    const int64_t q0 = col0 / 2, q1 = (col0 + ncols - 1) / 2;
    for (int64_t q = q0; q <= q1; ++q)
        for (int64_t k = 0; k < nk; ++k) {
            double z[2];
            draws_normal_pair(seed, (uint64_t)(k0 + k), (uint64_t)q, z[0], z[1]);
            for (int h = 0; h < 2; ++h) {
                const int64_t j = 2 * q + h - col0;
                if (j >= 0 && j < ncols) E[j * lde + k] = z[h];
            }
        }
    return GPV_OK;
}

int gpv_plan_draws_normals(gpv_plan *pl, uint64_t seed, int64_t skip_front, int64_t col0, int64_t ncols, double *E, int64_t lde)
{
    constexpr int NB = kLincombNB;
    if (!pl || !E || ncols < 0 || col0 < 0) return GPV_ERR_BAD_ARG;
    const int64_t n = pl->Nlocs;
    if (lde < n || skip_front < 0 || skip_front >= n) return GPV_ERR_BAD_ARG;
    if (const int rc = posterior_factor_state(pl)) return rc;
    if (ncols == 0) return GPV_OK;
    if (const int rc = enter_final(pl)) return rc;
    GPV_BUF(pl->d_lc_X, ensure((size_t)n * NB));
    GPV_BUF(pl->d_st_E, ensure((size_t)n * NB));
    hipStream_t st = pl->stream;
    const int64_t end = col0 + ncols;
    for (int64_t b = col0 / NB; b * NB < end; ++b) {                       // the batches of gpv_plan_draws_summary that hold them
        const int64_t base = b * NB;
        const int nb = (int)std::min<int64_t>(NB, end - base);
        if (GPV_HIP_FAILED(launch_draws_fill(pl->d_lc_X, n, seed, skip_front, base, nb, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(launch_solvet_unpack(pl->d_lc_X, pl->d_st_E, n, n, nb, st))) return drain_fail(st, GPV_ERR_HIP);
        const int64_t j0 = std::max(base, col0);                           // the batch's share of the call's columns
        if (cols_to_host(E + (j0 - col0) * lde, lde, pl->d_st_E + (size_t)(j0 - base) * n, n, base + nb - j0, st))
            return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
    }
    pl->last_stream = st;
    return GPV_OK;
}

// the device buffers of the summaries, by their offsets in d_ds (doubles)
struct DrawsBuf {
    double *mu, *S1, *S2, *mean, *var, *exceed, *part;
};
static DrawsBuf draws_buf(const gpv_plan *pl)
{
    const size_t n = (size_t)pl->Nlocs;
    double *b = pl->d_ds;
    return DrawsBuf{b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, b + 5 * n, b + (5 + kDrawsMaxThr) * n};
}
static int draws_alloc(gpv_plan *pl, int64_t ndraws)
{
    constexpr int NB = kLincombNB;
    const size_t n = (size_t)pl->Nlocs;
    GPV_BUF(pl->d_lc_X, ensure(n * NB));
    GPV_BUF(pl->d_ds, ensure((5 + kDrawsMaxThr) * n + (size_t)kDrawsBlocks * 2 * NB));
    GPV_BUF(pl->d_ds_cnt, ensure(kDrawsMaxThr * n));
    GPV_BUF(pl->d_ds_mask, ensure(n));
    if (pl->ds_draw_cap < ndraws) {
        pl->ds_draw_cap = 0;
        GPV_BUF(pl->d_ds_draw, resize(2 * (size_t)ndraws));
        pl->ds_draw_cap = ndraws;
    }
    return GPV_OK;
}

int gpv_plan_draws_summary(gpv_plan *pl, int64_t ndraws, uint64_t seed, int64_t skip_front, const double *mu_ord, int link, int nthr,
                           const double *thr, const uint8_t *mask, double *mean, double *var, double *exceed, double *draw_max,
                           double *draw_mean)
{
    constexpr int NB = kLincombNB;
    if (!pl || !mean || !var || ndraws < 2 || nthr < 0 || nthr > kDrawsMaxThr || link < 0 || link > 2) return GPV_ERR_BAD_ARG;
    if (nthr > 0 && (!thr || !exceed)) return GPV_ERR_BAD_ARG;
    if ((draw_max == nullptr) != (draw_mean == nullptr)) return GPV_ERR_BAD_ARG;
    const int64_t n = pl->Nlocs;
    if (skip_front < 0 || skip_front >= n) return GPV_ERR_BAD_ARG;
    const bool want_draw = draw_max != nullptr;
    int64_t nsel = n - skip_front;
    if (mask) {
        nsel = 0;
        for (int64_t k = skip_front; k < n; ++k) nsel += mask[k] != 0;
        if (nsel == 0) return GPV_ERR_BAD_ARG;
    }
    if (const int rc = posterior_factor_state(pl)) return rc;
    if (const int rc = enter_final(pl)) return rc;
    if (const int rc = draws_alloc(pl, ndraws)) return rc;
    hipStream_t st = pl->stream;
    const DrawsBuf B = draws_buf(pl);
    DrawsArgs a{};
    a.X = pl->d_lc_X; a.mu = B.mu; a.mask = (mask && want_draw) ? pl->d_ds_mask : nullptr;
    a.S1 = B.S1; a.S2 = B.S2; a.cnt = pl->d_ds_cnt; a.part = B.part;
    a.n = n; a.skip_front = skip_front; a.nthr = nthr; a.want_draw = want_draw ? 1 : 0;
    for (int t = 0; t < nthr; ++t) a.thr[t] = thr[t];
    const size_t nbytes = sizeof(double) * (size_t)n;
    if (mu_ord ? GPV_HIP_FAILED(hipMemcpyAsync(B.mu, mu_ord, nbytes, hipMemcpyHostToDevice, st))
               : GPV_HIP_FAILED(hipMemsetAsync(B.mu, 0, nbytes, st)))
        return drain_fail(st, GPV_ERR_HIP);
    if (a.mask && GPV_HIP_FAILED(hipMemcpyAsync(pl->d_ds_mask, mask, (size_t)n, hipMemcpyHostToDevice, st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipMemsetAsync(B.S1, 0, 2 * nbytes, st))) return drain_fail(st, GPV_ERR_HIP);                  // S1 and S2
    if (nthr > 0 && GPV_HIP_FAILED(hipMemsetAsync(pl->d_ds_cnt, 0, sizeof(uint32_t) * (size_t)nthr * (size_t)n, st)))
        return drain_fail(st, GPV_ERR_HIP);
    double *d_max = pl->d_ds_draw, *d_mean = pl->d_ds_draw + ndraws;
    for (int64_t draw0 = 0; draw0 < ndraws; draw0 += NB) {
        const int nb = (int)std::min<int64_t>(NB, ndraws - draw0);
        if (GPV_HIP_FAILED(launch_draws_fill(pl->d_lc_X, n, seed, skip_front, draw0, nb, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(solvet_sweep(pl, st))) return drain_fail(st, GPV_ERR_HIP);
        if (GPV_HIP_FAILED(launch_draws_accum(a, link, nb, draw0, (double)nsel, want_draw ? d_max : nullptr,
                                              want_draw ? d_mean : nullptr, st)))
            return drain_fail(st, GPV_ERR_HIP);
    }
    if (GPV_HIP_FAILED(launch_draws_finish(a, link, ndraws, B.mean, B.var, B.exceed, st))) return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipMemcpyAsync(mean, B.mean, nbytes, hipMemcpyDeviceToHost, st)) ||
        GPV_HIP_FAILED(hipMemcpyAsync(var, B.var, nbytes, hipMemcpyDeviceToHost, st)))
        return drain_fail(st, GPV_ERR_HIP);
    if (nthr > 0 && GPV_HIP_FAILED(hipMemcpyAsync(exceed, B.exceed, nbytes * (size_t)nthr, hipMemcpyDeviceToHost, st)))
        return drain_fail(st, GPV_ERR_HIP);
    if (want_draw && (GPV_HIP_FAILED(hipMemcpyAsync(draw_max, d_max, sizeof(double) * (size_t)ndraws, hipMemcpyDeviceToHost, st)) ||
                      GPV_HIP_FAILED(hipMemcpyAsync(draw_mean, d_mean, sizeof(double) * (size_t)ndraws, hipMemcpyDeviceToHost, st))))
        return drain_fail(st, GPV_ERR_HIP);
    if (GPV_HIP_FAILED(hipStreamSynchronize(st))) return drain_fail(st, GPV_ERR_HIP);
    pl->last_stream = st;
    return GPV_OK;
}

// developer aid (tools/lincomb_timing.py --summary; not part of the public header): device times of ONE full batch of
// gpv_plan_draws_summary by events between its three parts, ms[0..3) = fill, sweep, accumulation (link 0, no thresholds, the
// per-draw functionals over every location).  The sums it leaves in the plan's buffers belong to no call.
extern "C" int gpv_plan_debug_draws_ms(gpv_plan *pl, uint64_t seed, double *ms)
{
    if (!pl || !ms) return GPV_ERR_BAD_ARG;
    if (const int rc = posterior_factor_state(pl)) return rc;
    if (!pl->d_lc_X || !pl->d_ds || pl->ds_draw_cap < kLincombNB) return GPV_ERR_STATE;   // (after a gpv_plan_draws_summary)
    if (const int rc = enter_final(pl)) return rc;
    hipStream_t st = pl->stream;
    const DrawsBuf B = draws_buf(pl);
    DrawsArgs a{};
    a.X = pl->d_lc_X; a.mu = B.mu; a.S1 = B.S1; a.S2 = B.S2; a.cnt = pl->d_ds_cnt; a.part = B.part;
    a.n = pl->Nlocs; a.want_draw = 1;
    Event ev[4];
    int rc = GPV_OK;
    for (auto &e : ev)
        if (rc == GPV_OK && GPV_HIP_FAILED(hipEventCreate(e.put()))) rc = GPV_ERR_HIP;
    if (rc == GPV_OK &&
        (GPV_HIP_FAILED(hipEventRecord(ev[0], st)) || GPV_HIP_FAILED(launch_draws_fill(pl->d_lc_X, a.n, seed, 0, 0, kLincombNB, st)) ||
         GPV_HIP_FAILED(hipEventRecord(ev[1], st)) || GPV_HIP_FAILED(solvet_sweep(pl, st)) ||
         GPV_HIP_FAILED(hipEventRecord(ev[2], st)) ||
         GPV_HIP_FAILED(launch_draws_accum(a, 0, kLincombNB, 0, (double)a.n, pl->d_ds_draw, pl->d_ds_draw + pl->ds_draw_cap, st)) ||
         GPV_HIP_FAILED(hipEventRecord(ev[3], st)) || GPV_HIP_FAILED(hipStreamSynchronize(st))))
        rc = GPV_ERR_HIP;
    for (int i = 0; i < 3 && rc == GPV_OK; ++i) {
        float t = 0.f;
        if (GPV_HIP_FAILED(hipEventElapsedTime(&t, ev[i], ev[i + 1]))) rc = GPV_ERR_HIP;
        ms[i] = (double)t;
    }
    (void)hipStreamSynchronize(st);
    pl->last_stream = st;
    return rc;
}

int gpv_plan_get_sums(gpv_plan *pl, double *sums)
{
    if (!pl || !sums) return GPV_ERR_BAD_ARG;
    if (!pl->evaluated) return GPV_ERR_STATE;
    GPV_HIP(hipSetDevice(pl->device));
    if (pl->sums_on_host) {                        // the kernels wrote the totals into pinned host memory
        if (pl->sums_by_seq) {
            // spin on the sequence numbers the producing kernel stores behind the totals: no stream wait, no wake-up by
            // interrupt (the evaluation is a fraction of a millisecond for one rank of a sharded job).  Every 64 Ki spins the
            // stream is asked whether it has failed or finished without the numbers turning up (then the ordinary wait decides).
            const volatile unsigned long long *c = reinterpret_cast<const volatile unsigned long long *>(pl->h_sums + kNSums);
            bool seen = false;
            for (unsigned spin = 1; !seen; ++spin) {
                seen = true;
                for (int t = 0; t < kNSums; ++t) seen = seen && (c[t] == pl->seq);
                if (seen) break;
                __builtin_ia32_pause();                  // be a polite spinner: the sibling hardware thread may be the runtime's
                if ((spin & 0xFFFFu) == 0 && hipStreamQuery(pl->last_stream) != hipErrorNotReady) break;
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            if (!seen) {
                // the stream ended (or failed) without the numbers turning up: the ordinary wait decides, and totals that
                // still do not carry this evaluation's number are NOT handed out as if they were its result
                pl->ticket_dirty = true;
                GPV_HIP(hipStreamSynchronize(pl->last_stream));
                std::atomic_thread_fence(std::memory_order_acquire);
                for (int t = 0; t < kNSums; ++t)
                    if (c[t] != pl->seq) return GPV_ERR_STATE;
                pl->ticket_dirty = false;
            }
        } else {
            GPV_HIP(hipStreamSynchronize(pl->last_stream));
        }
        std::memcpy(sums, pl->h_sums, sizeof(double) * kNSums);
        return GPV_OK;
    }
    GPV_HIP(hipMemcpyAsync(sums, pl->d_sums, sizeof(double) * kNSums, hipMemcpyDeviceToHost, pl->last_stream));
    GPV_HIP(hipStreamSynchronize(pl->last_stream));
    return GPV_OK;
}

// developer aid (tools/wave_timeline.py, builds with -DGPV_TRACE_TIMES): `count` doubles of the per-workgroup partial-sum buffer
// from `offset` on; not part of the public header
extern "C" int gpv_plan_debug_block_sums(gpv_plan *pl, int64_t offset, int64_t count, double *out, int *grid)
{
    if (!pl || !out || offset < 0 || count < 0 || offset + count > (int64_t)kMaxGrid * kNSums) return GPV_ERR_BAD_ARG;
    if (const int rc = enter_final(pl)) return rc;
    GPV_HIP(hipMemcpy(out, pl->d_block + offset, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    if (grid) *grid = pl->grid;
    return GPV_OK;
}

int gpv_plan_get_Lentries(gpv_plan *pl, double *Lentries)
{
    if (!pl || !Lentries) return GPV_ERR_BAD_ARG;
    if (!pl->evaluated || !pl->have_U) return GPV_ERR_STATE;
    if (pl->rows == 0) return GPV_OK;
    GPV_HIP(hipSetDevice(pl->device));
    const size_t bytes = sizeof(double) * (size_t)pl->rows * pl->p;
    GPV_BUF(pl->d_tmp, ensure((size_t)pl->rows * pl->p));
    hipStream_t st = pl->last_stream;
    GPV_HIP(launch_rows_to_colmajor(pl->d_L, pl->P, pl->rows, pl->p, pl->d_tmp, st));
    static const bool no_stage = dev_getenv("GPV_NO_D2H_STAGING") != nullptr;
    constexpr size_t kChunk = (size_t)32 << 20;
    if (no_stage || bytes < 2 * kChunk) {
        GPV_HIP(hipMemcpyAsync(Lentries, pl->d_tmp, bytes, hipMemcpyDeviceToHost, st));
        GPV_HIP(hipStreamSynchronize(st));
        return GPV_OK;
    }
    // The caller's buffer is pageable (R allocates a fresh vector per .C() call): a plain hipMemcpy of 248 MB moves at
    // ~27 GB/s through HIP's own staging.  Two pinned 32 MB buffers instead: chunk c travels by DMA while host threads
    // copy chunk c - 1 out of the other buffer into the caller's memory.
    for (int b = 0; b < 2; ++b) {
        GPV_BUF(pl->h_stage[b], ensure(kChunk));
        if (!pl->stage_ev[b]) GPV_HIP(hipEventCreateWithFlags(pl->stage_ev[b].put(), hipEventDisableTiming));
    }
    const size_t nchunk = (bytes + kChunk - 1) / kChunk;
    const char *src = reinterpret_cast<const char *>(pl->d_tmp.get());
    char *dst = reinterpret_cast<char *>(Lentries);
    auto issue = [&](size_t c) -> hipError_t {
        const size_t off = c * kChunk, len = (off + kChunk <= bytes) ? kChunk : bytes - off;
        hipError_t e = hipMemcpyAsync(pl->h_stage[c & 1], src + off, len, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(pl->stage_ev[c & 1], st);
        return e;
    };
    GPV_HIP(issue(0));
    if (nchunk > 1) GPV_HIP(issue(1));
    for (size_t c = 0; c < nchunk; ++c) {
        GPV_HIP(hipEventSynchronize(pl->stage_ev[c & 1]));
        const size_t off = c * kChunk, len = (off + kChunk <= bytes) ? kChunk : bytes - off;
        const char *hs = pl->h_stage[c & 1];
        parallel_for((int64_t)len, [=](int64_t b0, int64_t e0) { std::memcpy(dst + off + b0, hs + b0, (size_t)(e0 - b0)); }, 8);
        if (c + 2 < nchunk) GPV_HIP(issue(c + 2));
    }
    return GPV_OK;
}

int gpv_plan_get_Zentries(gpv_plan *pl, double *Z)
{
    if (!pl || !Z) return GPV_ERR_BAD_ARG;
    if (!pl->evaluated) return GPV_ERR_STATE;
    if (pl->rows == 0) return GPV_OK;
    GPV_HIP(hipSetDevice(pl->device));
    GPV_BUF(pl->d_Z, ensure(2 * (size_t)pl->rows));
    if (pl->nug_is_scalar) {
        GPV_HIP(launch_fill(pl->d_stage, pl->nug_scalar, pl->rows, pl->last_stream));
        GPV_HIP(launch_zentries(pl->d_stage, pl->rows, pl->d_Z, pl->last_stream));
    } else {
        GPV_HIP(launch_zentries(pl->d_nug_user + pl->row_begin, pl->rows, pl->d_Z, pl->last_stream));
    }
    GPV_HIP(hipMemcpyAsync(Z, pl->d_Z, sizeof(double) * 2 * (size_t)pl->rows, hipMemcpyDeviceToHost, pl->last_stream));
    GPV_HIP(hipStreamSynchronize(pl->last_stream));
    return GPV_OK;
}

int gpv_plan_Lentries_device(gpv_plan *pl, double **d_ptr, int64_t *ld)
{
    if (!pl || !d_ptr || !ld) return GPV_ERR_BAD_ARG;
    if (!pl->evaluated || !pl->have_U) return GPV_ERR_STATE;
    *d_ptr = pl->d_L;
    *ld = pl->P;
    return GPV_OK;
}

int gpv_plan_rows(gpv_plan *pl, int64_t *row_begin, int64_t *row_end)
{
    if (!pl || !row_begin || !row_end) return GPV_ERR_BAD_ARG;
    *row_begin = pl->row_begin;
    *row_end = pl->row_end;
    return GPV_OK;
}

int gpv_plan_dims(gpv_plan *pl, int64_t *Nlocs, int *dim, int *ncolNN)
{
    if (!pl) return GPV_ERR_BAD_ARG;
    if (Nlocs) *Nlocs = pl->Nlocs;
    if (dim) *dim = pl->dim;
    if (ncolNN) *ncolNN = pl->p;
    return GPV_OK;
}

int gpv_plan_last_kernel_ms(gpv_plan *pl, double *ms)
{
    if (!pl || !ms) return GPV_ERR_BAD_ARG;
    if (!pl->evaluated || !pl->timed) return GPV_ERR_STATE;
    GPV_HIP(hipSetDevice(pl->device));
    GPV_HIP(hipEventSynchronize(pl->ev1));
    float f = 0.f;
    GPV_HIP(hipEventElapsedTime(&f, pl->ev0, pl->ev1));
    *ms = (double)f;
    return GPV_OK;
}

int gpv_plan_last_set_kernel(gpv_plan *pl)
{
    return (pl && pl->evaluated) ? pl->last_set_kernel : 0;
}

int gpv_plan_set_kernel_timing(gpv_plan *pl, int on)
{
    if (!pl) return GPV_ERR_BAD_ARG;
    pl->timing = on != 0;
    return GPV_OK;
}

int gpv_loglik_z_from_sums(const double *s, int64_t n, double *loglik)
{
    if (!s || !loglik) return GPV_ERR_BAD_ARG;
    // -1/2 [ sum log(tau+v) + sum (z-mu)^2/(tau+v) + n log 2pi ]  == R/vecchia_likelihood.R:95-96 for cond.yz='z'
    if (s[6] > 0.0) {
        // a failed block leaves its Lentries row at zero (src/U_NZentries.cpp:64-66) => diag(U) = 0 => logdet.num = +Inf
        // (R/vecchia_likelihood.R:76) => loglik = -Inf (:95-96); an optimiser comparing likelihoods sees "worst", not NaN
        *loglik = -INFINITY;
        return GPV_OK;
    }
    *loglik = -0.5 * (s[2] + s[3] + (double)n * std::log(2.0 * M_PI));
    return GPV_OK;
}

int gpv_loglik_from_sums(const double *s, int64_t n, double *loglik)
{
    // R/vecchia_likelihood.R:95-96 with logdet.num = -2 s0 + s5, quadform.num = s1 + s4 (numerator sums) and, from the
    // posterior pass (GPV_WANT_DENOM), logdet.denom = -s2 (s2 = log det W), quadform.denom = s3
    if (!s || !loglik) return GPV_ERR_BAD_ARG;
    if (s[6] > 0.0) { *loglik = -INFINITY; return GPV_OK; }      // as above: log(0) in logdet.num
    const double neg2 = (-2.0 * s[0] + s[5]) + s[2] + (s[1] + s[4]) - s[3] + (double)n * std::log(2.0 * M_PI);
    *loglik = -0.5 * neg2;
    return GPV_OK;
}

int gpv_numerator_from_sums(const double *s, double *logdet_num, double *quadform_num)
{
    if (!s || !logdet_num || !quadform_num) return GPV_ERR_BAD_ARG;
    *logdet_num = -2.0 * s[0] + s[5];     // -2 sum log diag(U): latent columns d_k, observed columns 1/sqrt(tau_k)
    *quadform_num = s[1] + s[4];          // sum z1^2
    return GPV_OK;
}

// ---------------------------------------------------------------------------------------
// literal drop-ins
// ---------------------------------------------------------------------------------------
// Plan cache of the literal drop-in.  An unmodified R createU (R/createU.R:152-154) hands the same locsord / revNNarray /
// revCondOnLatent to U_NZentries at every optimiser step (vecchia_estimate: up to 300 calls, R/vecchia_wrappers.R:87-93);
// the device plan built from them (Morton order, index re-layout, uploads: ~100 ms at n = 1e6) is kept and reused while
// shape and a 128-bit content hash of the three arrays match.  One entry; GPV_NO_PLAN_CACHE=1 disables it;
// gpv_plan_cache_clear() frees the device memory it holds.
namespace {
struct PlanCache {
    std::mutex mu;
    gpv_plan *pl = nullptr;
    int64_t Nlocs = 0;
    int dim = 0, ncol = 0;
    Hash128 h_locs, h_nn, h_cond;
    int64_t hits = 0, misses = 0;
};
PlanCache g_cache;
}  // namespace

int gpv_hash_bytes(const void *ptr, int64_t bytes, uint64_t seed, uint64_t *out2)
{
    if ((!ptr && bytes > 0) || bytes < 0 || !out2) return GPV_ERR_BAD_ARG;
    static const unsigned char none = 0;
    const Hash128 h = hash_bytes(bytes > 0 ? ptr : &none, (size_t)bytes, seed);
    out2[0] = h.a;
    out2[1] = h.b;
    return GPV_OK;
}

int gpv_plan_cache_clear(void)
{
    std::lock_guard<std::mutex> g(g_cache.mu);
    if (g_cache.pl) gpv_plan_destroy(g_cache.pl);
    g_cache.pl = nullptr;
    return GPV_OK;
}

int gpv_plan_cache_stats(int64_t *hits, int64_t *misses)
{
    std::lock_guard<std::mutex> g(g_cache.mu);
    if (hits) *hits = g_cache.hits;
    if (misses) *misses = g_cache.misses;
    return GPV_OK;
}

static int zentries_host(gpv_plan *pl, const double *nuggets_obsord, int64_t n, double *Zentries)
{
    if (n <= 0) return GPV_OK;
    if (n <= pl->Nlocs && n <= pl->rows) {
        // the plan's own buffers: no allocation on the (cached) hot path of the drop-in
        GPV_BUF(pl->d_Z, ensure(2 * (size_t)pl->rows));
        GPV_HIP(hipMemcpyAsync(pl->d_stage, nuggets_obsord, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, pl->stream));
        GPV_HIP(launch_zentries(pl->d_stage, n, pl->d_Z, pl->stream));
        GPV_HIP(hipMemcpyAsync(Zentries, pl->d_Z, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, pl->stream));
        GPV_HIP(hipStreamSynchronize(pl->stream));
        return GPV_OK;
    }
    DevBuf<double> d_n, d_Z;
    GPV_BUF(d_n, resize((size_t)n));
    GPV_BUF(d_Z, resize(2 * (size_t)n));
    GPV_HIP(hipMemcpyAsync(d_n, nuggets_obsord, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, pl->stream));
    GPV_HIP(launch_zentries(d_n, n, d_Z, pl->stream));
    GPV_HIP(hipMemcpyAsync(Zentries, d_Z, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, pl->stream));
    GPV_HIP(hipStreamSynchronize(pl->stream));
    return GPV_OK;
}

void gpv_U_NZentries(const int *Ncores, const int *n, const int *Nlocs, const int *dim, const int *ncolNN,
                     const double *locs, const int *revNNarray, const int *revCondOnLatent, const double *nuggets,
                     const double *nuggets_obsord, const char **covType, const double *covparms, const int *ncovparms,
                     double *Lentries, double *Zentries, int *n_failed, int *status)
{
    (void)Ncores;
    int dummy = 0;
    if (!status) status = &dummy;
    if (!n || !Nlocs || !dim || !ncolNN || !locs || !revNNarray || !revCondOnLatent || !nuggets || !nuggets_obsord ||
        !covType || !covparms || !ncovparms || !Lentries || !Zentries) {
        *status = GPV_ERR_BAD_ARG;
        return;
    }
    CovSetup cs;
    int rc = cov_setup(*covType, covparms, *ncovparms, *dim, cs);   // checked first: src/U_NZentries.cpp:27-29
    if (rc != GPV_OK) { *status = rc; return; }
    gpv_plan *pl = nullptr;
    PhaseTimer tm;
    static const bool no_cache = getenv("GPV_NO_PLAN_CACHE") != nullptr;
    std::unique_lock<std::mutex> cache_lock(g_cache.mu, std::defer_lock);
    bool cached = false, evaluated = false;
    // The speculative evaluation copies the CACHED plan's U entries into the caller's Lentries before the content hash has said
    // whose plan that is.  If the hash then does not match and the rebuild or its evaluation fails, those values must not stay
    // there looking like results: every exit with an error behind a speculative write fills Lentries with NaN.
    bool spec_wrote = false;
    auto fail = [&](int code) {
        if (spec_wrote) {
            const size_t cnt = (size_t)*Nlocs * (size_t)*ncolNN;
            const double nanv = std::numeric_limits<double>::quiet_NaN();
            for (size_t e = 0; e < cnt; ++e) Lentries[e] = nanv;
        }
        *status = code;
    };
    if (!no_cache && *Nlocs > 0 && *dim > 0 && *ncolNN > 0) {
        cache_lock.lock();                                   // the cached plan is in use until this call returns
        const size_t nl = (size_t)*Nlocs;
        Hash128 hl, hn, hc;
        // (threads: 32 when nothing else runs; 12 beside the evaluation, whose copy to the caller keeps 8 host threads and the
        //  DMA engine busy on the same memory)
        auto hash_all = [&](unsigned threads) {
            hl = hash_bytes(locs, nl * (size_t)*dim * sizeof(double), 1, threads);
            hn = hash_bytes(revNNarray, nl * (size_t)*ncolNN * sizeof(int), 2, threads);
            hc = hash_bytes(revCondOnLatent, nl * (size_t)*ncolNN * sizeof(int), 3, threads);
        };
        // The hash of the three arrays (264 MB at n = 1e6, m = 30: ~3.6 ms on 32 threads) is what proves the cached plan
        // is the plan of THIS call.  When a plan of the right shape is cached -- every call of an optimiser run but the first
        // -- the evaluation is started on it at once and the arrays are hashed while the kernel, the transposition and the
        // copy of the U entries to the caller run; the outputs count only once the hash has matched, otherwise the plan is
        // rebuilt and everything is computed again over them.
        int rc_spec = GPV_OK;
        const bool spec = g_cache.pl && g_cache.Nlocs == *Nlocs && g_cache.dim == *dim && g_cache.ncol == *ncolNN;
        spec_wrote = spec;
        if (spec) {
            std::thread hasher(hash_all, 12u);
            rc_spec = plan_eval_checked(g_cache.pl, cs, nuggets, *Nlocs, GPV_WANT_U, nullptr, nullptr);
            if (rc_spec == GPV_OK) rc_spec = gpv_plan_get_Lentries(g_cache.pl, Lentries);
            hasher.join();
            tm.lap("drop-in: content hash over nuggets H2D + kernel + transpose + D2H");
        } else {
            hash_all(32u);
            tm.lap("drop-in: content hash");
        }
        if (spec && g_cache.h_locs == hl && g_cache.h_nn == hn && g_cache.h_cond == hc) {
            pl = g_cache.pl;
            cached = true;
            evaluated = true;
            rc = rc_spec;
            ++g_cache.hits;
        } else {
            if (g_cache.pl) gpv_plan_destroy(g_cache.pl);
            g_cache.pl = nullptr;
            ++g_cache.misses;
            rc = gpv_plan_create(&pl, 0, *Nlocs, *dim, *ncolNN, locs, revNNarray, revCondOnLatent, 0, *Nlocs);
            if (rc != GPV_OK) { fail(rc); return; }
            g_cache.pl = pl;
            g_cache.Nlocs = *Nlocs; g_cache.dim = *dim; g_cache.ncol = *ncolNN;
            g_cache.h_locs = hl; g_cache.h_nn = hn; g_cache.h_cond = hc;
            cached = true;                                   // owned by the cache from here on
        }
    } else {
        rc = gpv_plan_create(&pl, 0, *Nlocs, *dim, *ncolNN, locs, revNNarray, revCondOnLatent, 0, *Nlocs);
        if (rc != GPV_OK) { *status = rc; return; }
    }
    tm.lap("drop-in: plan");
    if (!evaluated) {
        rc = plan_eval_checked(pl, cs, nuggets, *Nlocs, GPV_WANT_U, nullptr, nullptr);
        if (rc == GPV_OK && tm.on) (void)hipStreamSynchronize(pl->stream);
        tm.lap("drop-in: nuggets H2D + kernel");
        if (rc == GPV_OK) rc = gpv_plan_get_Lentries(pl, Lentries);
        tm.lap("drop-in: transpose + D2H");
    }
    double sums[GPV_NSUMS];
    if (rc == GPV_OK) rc = gpv_plan_get_sums(pl, sums);
    if (rc == GPV_OK) rc = zentries_host(pl, nuggets_obsord, *n, Zentries);
    if (rc == GPV_OK && n_failed) *n_failed = (int)sums[6];
    tm.lap("drop-in: Zentries");
    if (!cached) {
        gpv_plan_destroy(pl);
    } else if (rc != GPV_OK) {                               // do not keep a plan whose evaluation failed
        gpv_plan_destroy(pl);
        g_cache.pl = nullptr;
    }
    tm.lap("drop-in: destroy");
    if (rc != GPV_OK) fail(rc);
    else *status = rc;
}

void gpv_U_NZentries_mat(const int *Ncores, const int *n, const int *Nlocs, const int *ncolNN, const int *revNNarray,
                         const double *nuggets_obsord, const double *covVals, double *Lentries, double *Zentries,
                         int *n_failed, int *status)
{
    (void)Ncores;
    int dummy = 0;
    if (!status) status = &dummy;
    if (!n || !Nlocs || !ncolNN || !revNNarray || !nuggets_obsord || !covVals || !Lentries || !Zentries) {
        *status = GPV_ERR_BAD_ARG;
        return;
    }
    gpv_plan *pl = nullptr;
    int rc = gpv_plan_create(&pl, 0, *Nlocs, 1, *ncolNN, nullptr, revNNarray, nullptr, 0, *Nlocs);
    if (rc != GPV_OK) { *status = rc; return; }
    if (GPV_BUF_FAILED(pl->d_covvals, upload(covVals, (size_t)(*Nlocs) * (size_t)(*Nlocs)))) {
        gpv_plan_destroy(pl);
        *status = GPV_ERR_HIP;
        return;
    }
    CovSetup cs{};
    cs.cov = COV_DENSE;
    rc = plan_eval_impl(pl, cs, nullptr, 0, GPV_WANT_U, nullptr, nullptr);
    if (rc == GPV_OK) rc = gpv_plan_get_Lentries(pl, Lentries);
    double sums[GPV_NSUMS];
    if (rc == GPV_OK) rc = gpv_plan_get_sums(pl, sums);
    if (rc == GPV_OK) rc = zentries_host(pl, nuggets_obsord, *n, Zentries);
    if (rc == GPV_OK && n_failed) *n_failed = (int)sums[6];
    gpv_plan_destroy(pl);
    *status = rc;
}

static void covfun_host(const double *distmat, const int *nelem, const CovSetup &cs, double *covmat, int *status)
{
    int ndev = 0;
    if (gpv_device_count(&ndev) != GPV_OK) { *status = GPV_ERR_NO_DEVICE; return; }
    const int64_t n = *nelem;
    if (n <= 0) { *status = GPV_OK; return; }
    DevBuf<double> d_in, d_out;
    *status = GPV_ERR_HIP;
    if (GPV_HIP_FAILED(hipSetDevice(0)) || GPV_BUF_FAILED(d_in, upload(distmat, (size_t)n)) || GPV_BUF_FAILED(d_out, resize((size_t)n)) ||
        GPV_HIP_FAILED(launch_covfun(d_in, n, cs.cov, cs.sig0, cs.sA, cs.cA, cs.sB, cs.cB, d_out, nullptr)) ||
        GPV_HIP_FAILED(hipMemcpy(covmat, d_out, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost)))
        return;
    *status = GPV_OK;
}

void gpv_MaternFun(const double *distmat, const int *nelem, const double *covparms, double *covmat, int *status)
{
    int dummy = 0;
    if (!status) status = &dummy;
    if (!distmat || !nelem || !covparms || !covmat) { *status = GPV_ERR_BAD_ARG; return; }
    CovSetup cs;
    const int rc = cov_setup("matern", covparms, 3, 0, cs);
    if (rc != GPV_OK) { *status = rc; return; }
    covfun_host(distmat, nelem, cs, covmat, status);
}

void gpv_EsqeFun(const double *distmat, const int *nelem, const double *covparms, double *covmat, int *status)
{
    int dummy = 0;
    if (!status) status = &dummy;
    if (!distmat || !nelem || !covparms || !covmat) { *status = GPV_ERR_BAD_ARG; return; }
    CovSetup cs;
    const int rc = cov_setup("esqe", covparms, 4, 0, cs);
    if (rc != GPV_OK) { *status = rc; return; }
    covfun_host(distmat, nelem, cs, covmat, status);
}

// ---------------------------------------------------------------------------------------
// several GPUs from ONE host process (what an R session would use): one plan per device, contiguous row shards,
// replicated locations / data, the 8-double partial sums added on the host in device order (deterministic).
// The one-process-per-GPU route (torchrun + RCCL all-reduce) uses gpv_plan_* directly, see bench.py.
// ---------------------------------------------------------------------------------------
struct gpv_mplan {
    std::vector<gpv_plan *> plans;
    int64_t Nlocs = 0;
    int p = 0;
    bool replicas = false;        // every plan owns ALL rows (gpv_mplan_create_replicas); else contiguous row shards
};

int gpv_mplan_create(gpv_mplan **out, const int *devices, int ndev, int64_t Nlocs, int dim, int ncolNN,
                     const double *locs, const int *revNN, const int *revCond)
{
    if (!out || !devices || ndev < 1) return GPV_ERR_BAD_ARG;
    *out = nullptr;
    gpv_mplan *mp = new gpv_mplan();
    mp->Nlocs = Nlocs;
    mp->p = ncolNN;
    for (int g = 0; g < ndev; ++g) {
        gpv_plan *pl = nullptr;
        const int64_t a = (Nlocs * g) / ndev, b = (Nlocs * (g + 1)) / ndev;     // rows beyond the first m cost the same
        const int rc = plan_create_impl(&pl, devices[g], Nlocs, dim, ncolNN, locs, revNN, revCond, a, b,
                                        mp->plans.empty() ? nullptr : mp->plans[0]->h_newpos.data());   // Morton order: once
        if (rc != GPV_OK) {
            for (gpv_plan *q : mp->plans) gpv_plan_destroy(q);
            delete mp;
            return rc;
        }
        mp->plans.push_back(pl);
    }
    *out = mp;
    return GPV_OK;
}

// Replicas: what "8 GPUs" means for the parts of the path that do not shard (the posterior pass of cond.yz='SGV', hence
// every Vecchia-Laplace Newton step, BASELINE.json configs[4]): one COMPLETE plan per device, each evaluating its own
// parameter vector (the vertices of a simplex, a grid, restarts) or its own data set, all of them in flight together.
int gpv_mplan_create_replicas(gpv_mplan **out, const int *devices, int ndev, int64_t Nlocs, int dim, int ncolNN,
                              const double *locs, const int *revNN, const int *revCond)
{
    if (!out || !devices || ndev < 1) return GPV_ERR_BAD_ARG;
    *out = nullptr;
    gpv_mplan *mp = new gpv_mplan();
    mp->Nlocs = Nlocs;
    mp->p = ncolNN;
    mp->replicas = true;
    for (int g = 0; g < ndev; ++g) {
        gpv_plan *pl = nullptr;
        const int rc = plan_create_impl(&pl, devices[g], Nlocs, dim, ncolNN, locs, revNN, revCond, 0, Nlocs,
                                        mp->plans.empty() ? nullptr : mp->plans[0]->h_newpos.data());
        if (rc != GPV_OK) {
            for (gpv_plan *q : mp->plans) gpv_plan_destroy(q);
            delete mp;
            return rc;
        }
        mp->plans.push_back(pl);
    }
    *out = mp;
    return GPV_OK;
}

int gpv_mplan_count(gpv_mplan *mp, int *n)
{
    if (!mp || !n) return GPV_ERR_BAD_ARG;
    *n = (int)mp->plans.size();
    return GPV_OK;
}

int gpv_mplan_build_posterior(gpv_mplan *mp, const int *revNN, const int *revCond)
{
    if (!mp || !mp->replicas) return GPV_ERR_BAD_ARG;               // row shards cannot run the posterior pass
    for (gpv_plan *q : mp->plans) {
        const int rc = gpv_plan_build_posterior(q, revNN, revCond);
        if (rc != GPV_OK) return rc;
    }
    return GPV_OK;
}

int gpv_mplan_set_data_one(gpv_mplan *mp, int replica, const double *z_ord)
{
    if (!mp || !mp->replicas || replica < 0 || replica >= (int)mp->plans.size()) return GPV_ERR_BAD_ARG;
    return gpv_plan_set_data(mp->plans[(size_t)replica], z_ord);
}

int gpv_mplan_eval_each(gpv_mplan *mp, const char *covType, const double *covparms, int ncovparms, const double *nuggets,
                        int flags, double *sums)
{
    if (!mp || !mp->replicas || !covparms || !nuggets || !sums || ncovparms < 1) return GPV_ERR_BAD_ARG;
    const size_t R = mp->plans.size();
    for (size_t r = 0; r < R; ++r) {                                // every replica is enqueued before any is awaited
        const int rc = gpv_plan_eval(mp->plans[r], covType, covparms + r * (size_t)ncovparms, ncovparms, nuggets + r, 1, flags,
                                     nullptr, nullptr);
        if (rc != GPV_OK) return rc;
    }
    for (size_t r = 0; r < R; ++r) {
        const int rc = gpv_plan_get_sums(mp->plans[r], sums + r * GPV_NSUMS);
        if (rc != GPV_OK) return rc;
    }
    return GPV_OK;
}

int gpv_mplan_vl_begin_one(gpv_mplan *mp, int replica, int model, const double *likparms, const double *z_ord,
                           const double *prior_mean_ord, const double *y_init_ord)
{
    if (!mp || !mp->replicas || replica < 0 || replica >= (int)mp->plans.size()) return GPV_ERR_BAD_ARG;
    return gpv_plan_vl_begin(mp->plans[(size_t)replica], model, likparms, z_ord, prior_mean_ord, y_init_ord);
}

int gpv_mplan_vl_step_each(gpv_mplan *mp, const char *covType, const double *covparms, int ncovparms, const int *active,
                           double *dmax, int *flags)
{
    if (!mp || !mp->replicas || !covparms || !dmax || !flags || ncovparms < 1) return GPV_ERR_BAD_ARG;
    const size_t R = mp->plans.size();
    for (size_t r = 0; r < R; ++r) {
        if (active && !active[r]) continue;
        const int rc = vl_step_enqueue(mp->plans[r], covType, covparms + r * (size_t)ncovparms, ncovparms);
        if (rc != GPV_OK) return rc;
    }
    for (size_t r = 0; r < R; ++r) {
        if (active && !active[r]) continue;
        const int rc = vl_step_finish(mp->plans[r], dmax + r, flags + r);
        if (rc != GPV_OK) return rc;
    }
    return GPV_OK;
}

int gpv_mplan_vl_get_one(gpv_mplan *mp, int replica, double *mean_ord, double *t_ord, double *D_ord)
{
    if (!mp || !mp->replicas || replica < 0 || replica >= (int)mp->plans.size()) return GPV_ERR_BAD_ARG;
    return gpv_plan_vl_get(mp->plans[(size_t)replica], mean_ord, t_ord, D_ord);
}

int gpv_mplan_destroy(gpv_mplan *mp)
{
    if (!mp) return GPV_OK;
    for (gpv_plan *q : mp->plans) gpv_plan_destroy(q);
    delete mp;
    return GPV_OK;
}

int gpv_mplan_set_data(gpv_mplan *mp, const double *z_ord)
{
    if (!mp) return GPV_ERR_BAD_ARG;
    for (gpv_plan *q : mp->plans) {
        const int rc = gpv_plan_set_data(q, z_ord);
        if (rc != GPV_OK) return rc;
    }
    return GPV_OK;
}

int gpv_mplan_eval(gpv_mplan *mp, const char *covType, const double *covparms, int ncovparms, const double *nuggets,
                   int64_t n_nuggets, int flags, double *sums)
{
    if (!mp || !sums || mp->replicas) return GPV_ERR_BAD_ARG;
    if (flags & (GPV_WANT_DENOM | GPV_WANT_MEAN)) return GPV_ERR_BAD_ARG;       // the posterior pass does not shard
    for (gpv_plan *q : mp->plans) {                                              // all devices start before any is awaited
        const int rc = gpv_plan_eval(q, covType, covparms, ncovparms, nuggets, n_nuggets, flags, nullptr, nullptr);
        if (rc != GPV_OK) return rc;
    }
    for (int s = 0; s < GPV_NSUMS; ++s) sums[s] = 0.0;
    for (gpv_plan *q : mp->plans) {
        double part[GPV_NSUMS];
        const int rc = gpv_plan_get_sums(q, part);
        if (rc != GPV_OK) return rc;
        for (int s = 0; s < GPV_NSUMS; ++s) sums[s] += part[s];
    }
    return GPV_OK;
}

int gpv_mplan_get_Lentries(gpv_mplan *mp, double *Lentries)
{
    // column-major Nlocs x ncolNN: every device's shard lands in its rows
    if (!mp || !Lentries || mp->replicas) return GPV_ERR_BAD_ARG;
    for (gpv_plan *q : mp->plans) {
        const int64_t rows = q->rows;
        if (rows == 0) continue;
        std::vector<double> tmp((size_t)rows * mp->p);
        const int rc = gpv_plan_get_Lentries(q, tmp.data());
        if (rc != GPV_OK) return rc;
        for (int c = 0; c < mp->p; ++c)
            std::memcpy(Lentries + (size_t)c * mp->Nlocs + q->row_begin, tmp.data() + (size_t)c * rows, sizeof(double) * (size_t)rows);
    }
    return GPV_OK;
}

// ---------------------------------------------------------------------------------------
// host-side setup helper (parameter-independent, runs once per data set; "next" row §8f-3)
// ---------------------------------------------------------------------------------------
int gpv_whichCondOnLatent(const int *NNarray, int64_t n, int ncolNN, int64_t firstind_pred, int *Cond)
{
    // R/whichCondOnLatent.R:2-26, literal semantics (is.element(NA, x) is TRUE when x holds an NA; first maximum).
    // O(n p^2) with a stamp array instead of R's O(n p^3) nested is.element calls.  The loop is bound by the random
    // row reads (under maxmin ordering the neighbours of a point are scattered over the whole array), so every finished
    // row is kept as a compact list of its latent-conditioned neighbours (one cache line instead of two full rows) and
    // the lists point k+2 will look at are prefetched.
    if (!NNarray || !Cond || n <= 0 || ncolNN < 1 || n >= ((int64_t)1 << 31)) return GPV_ERR_BAD_ARG;
    const int p = ncolNN;
    std::vector<int32_t> nnr((size_t)n * p);               // row-major working copy (the R layout has stride n)
    for (int c = 0; c < p; ++c)
        for (int64_t r = 0; r < n; ++r) {
            const int v = NNarray[r + (int64_t)c * n];
            const int w = is_missing(v) ? 0 : v;
            if (w < 0 || (int64_t)w > n) return GPV_ERR_INDEX;
            nnr[(size_t)r * p + c] = w;
        }
    auto NN = [&](int64_t r, int c) -> int32_t { return nnr[(size_t)r * p + c]; };
    const int LS = p + 1;                                   // lat row: [count, entries...]
    std::vector<int32_t> lat((size_t)n * LS, 0);
    std::vector<int32_t> stamp((size_t)n + 1, -1);
    std::vector<char> has_na((size_t)n, 0);
    std::vector<int> latents(p), cdrow(p);
    for (int c = 0; c < p; ++c) Cond[(int64_t)c * n] = INT_MIN;
    Cond[0] = 1;                                                         // :10
    for (int c = 0; c < p; ++c) has_na[0] |= (NN(0, c) == 0);
    if (NN(0, 0) != 0) { lat[0] = 1; lat[1] = NN(0, 0); }
    for (int64_t k = 1; k < n; ++k) {                                    // :12
        if (k + 2 < n) {
            for (int c = 1; c < p; ++c) {
                const int32_t l = NN(k + 2, c);
                if (l != 0) {
                    const char *a = reinterpret_cast<const char *>(&lat[(size_t)(l - 1) * LS]);
                    __builtin_prefetch(a);
                    __builtin_prefetch(a + 64);
                }
            }
        }
        int n_na = 0;
        for (int c = 0; c < p; ++c) {
            const int32_t v = NN(k, c);
            if (v == 0) ++n_na; else stamp[v] = (int32_t)k;
        }
        has_na[k] = n_na > 0;
        latents[0] = 0;
        for (int ind = 1; ind < p; ++ind) {                              // :14-18
            latents[ind] = 0;
            const int32_t l = NN(k, ind);
            if (l != 0 && l < firstind_pred) {
                const int32_t *lr = &lat[(size_t)(l - 1) * LS];
                int cnt = 0;
                for (int t = 1; t <= lr[0]; ++t) cnt += (stamp[lr[t]] == (int32_t)k);
                if (has_na[l - 1]) cnt += n_na;
                latents[ind] = cnt;
            }
        }
        int best = 0;
        for (int ind = 1; ind < p; ++ind)
            if (latents[ind] > latents[best]) best = ind;                // which(latents == max)[1]
        const int32_t ref = NN(k, best);                                 // :19
        // :20 -- table = NNarray[ref,] * CondOnLatent[ref,]; for ref == k that row is still all NA
        const int32_t *tab = nullptr;
        int ntab = 0;
        if (ref != 0 && ref - 1 != k) {
            tab = &lat[(size_t)(ref - 1) * LS + 1];
            ntab = lat[(size_t)(ref - 1) * LS];
        }
        for (int c = 0; c < p; ++c) {
            const int32_t v = NN(k, c);
            cdrow[c] = INT_MIN;
            if (v == 0) continue;                                        // stays NA (:23)
            int val = 0;
            for (int t = 0; t < ntab; ++t) val |= (tab[t] == v);
            if (v >= firstind_pred) val = 1;                             // :21
            cdrow[c] = val;
        }
        if (NN(k, 0) != 0) cdrow[0] = 1;                                 // :22
        int32_t *lw = &lat[(size_t)k * LS];
        int w = 0;
        for (int c = 0; c < p; ++c) {
            Cond[k + (int64_t)c * n] = cdrow[c];
            if (cdrow[c] == 1) lw[++w] = NN(k, c);
        }
        lw[0] = w;
    }
    return GPV_OK;
}

}  // extern "C"
