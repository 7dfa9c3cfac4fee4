// tests/sanitize/nn_driver.cpp — TEST INFRASTRUCTURE: the HOST half of gpv_find_ordered_nn (csrc/gpv_nn.hip) under
// AddressSanitizer + UBSan, linked against tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime.  That half is the
// argument check, the transposition into the padded row-major buffer, the extent scan, the choice of the cell edge, the clamp
// to 4096 cells per dimension, the counting sort into cells, seven allocations and the scatter of the shard into the caller's
// column-major array.  Kernels do not run ("device" memory is zero-filled host memory), so this checks statuses, bounds,
// lifetimes and leaks, never indices: after a good call the rows of the shard hold 0 and every other entry of the caller's
// array still holds the sentinel it was filled with.
//
//   build: tests/_host_driver_build.py (every unit of gpvecchia_amd/build.py units() --offload-host-only with the sanitizers, the
//          mock runtime, this file as the program); run by tests/test_nn_driver.py and tools/sanitize_host.sh.
#include "../../include/gpvecchia.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

extern "C" long mockhip_launches(void);
extern "C" long mockhip_live_allocations(void);
extern "C" long mockhip_allocs(void);
extern "C" void mockhip_fail_alloc_at(long k);

static int g_fail = 0;
#define EXPECT(cond)                                                                           \
    do {                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static const int kSentinel = -77;

struct Result { int status; long launches, allocs; bool inside_zero, outside_kept; };

// one call on a sentinel-filled array; what was written where
static Result call(const std::vector<double> &locs, int64_t n, int dim, int m, int64_t rb, int64_t re)
{
    const int p = m < 0 ? 1 : m + 1;
    std::vector<int> nn((size_t)n * p, kSentinel);
    const long l0 = mockhip_launches(), a0 = mockhip_allocs();
    Result r;
    r.status = gpv_find_ordered_nn(0, locs.data(), n, dim, m, rb, re, nn.data());
    r.launches = mockhip_launches() - l0;
    r.allocs = mockhip_allocs() - a0;
    r.inside_zero = r.outside_kept = true;
    for (int s = 0; s < p; ++s)
        for (int64_t k = 0; k < n; ++k) {
            const int v = nn[(size_t)(k + (int64_t)s * n)];
            if (r.status == GPV_OK && k >= rb && k < re) r.inside_zero = r.inside_zero && v == 0;
            else r.outside_kept = r.outside_kept && v == kSentinel;
        }
    EXPECT(mockhip_live_allocations() == 0);
    return r;
}

// a good call: the shard written, nothing else; launches as expected
static void good(const char *what, const std::vector<double> &locs, int64_t n, int dim, int m, int64_t rb, int64_t re, long launches)
{
    const Result r = call(locs, n, dim, m, rb, re);
    if (r.status != GPV_OK || !r.inside_zero || !r.outside_kept || r.launches != launches) {
        std::fprintf(stderr, "%s: status %d, shard written %d, rest kept %d, %ld launches (wanted %ld)\n", what, r.status,
                     (int)r.inside_zero, (int)r.outside_kept, r.launches, launches);
        ++g_fail;
    }
}

static void refused(const char *what, const double *locs, int64_t n, int dim, int m, int64_t rb, int64_t re, bool null_out = false)
{
    std::vector<int> nn(4096, kSentinel);                      // (refused before anything is sized from the arguments)
    const long l0 = mockhip_launches(), a0 = mockhip_allocs();
    const int st = gpv_find_ordered_nn(0, locs, n, dim, m, rb, re, null_out ? nullptr : nn.data());
    bool kept = true;
    for (int v : nn) kept = kept && v == kSentinel;
    if (st != GPV_ERR_BAD_ARG || !kept || mockhip_launches() != l0 || mockhip_allocs() != a0) {
        std::fprintf(stderr, "%s: status %d (wanted %d), array kept %d, %ld launches, %ld allocations\n", what, st,
                     (int)GPV_ERR_BAD_ARG, (int)kept, mockhip_launches() - l0, mockhip_allocs() - a0);
        ++g_fail;
    }
}

// every allocation of the call failing in turn: GPV_ERR_HIP, nothing written, nothing left; then one more: all succeed
static void alloc_failures(const char *what, const std::vector<double> &locs, int64_t n, int dim, int m, long nalloc)
{
    for (long k = 0; k <= nalloc; ++k) {
        mockhip_fail_alloc_at(k);
        const Result r = call(locs, n, dim, m, 0, n);
        mockhip_fail_alloc_at(-1);
        const int want = k < nalloc ? GPV_ERR_HIP : GPV_OK;
        if (r.status != want || !r.outside_kept || !r.inside_zero || (k < nalloc && r.allocs != k + 1) || (k == nalloc && r.allocs != nalloc)) {
            std::fprintf(stderr, "%s: allocation %ld of %ld failing -> status %d (wanted %d), %ld allocation calls, array ok %d\n", what,
                         k, nalloc, r.status, want, r.allocs, (int)(r.outside_kept && r.inside_zero));
            ++g_fail;
        }
    }
}

static std::vector<double> uniform(int64_t n, int dim, uint64_t seed)
{
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> x((size_t)n * dim);
    for (auto &v : x) v = U(rng);
    return x;
}

int main()
{
    const int m = 10, mmax = gpv_nn_max_m();
    EXPECT(mmax == 212);                       // 768 (m + 1) bytes of LDS <= 160 KB; gpv_max_p() - 1 = 191 is inside
    // ---- the grid: n = 8193 (the first size that takes it) and n = 20000, one to three dimensions
    for (int dim = 1; dim <= 3; ++dim)
        for (int64_t n : {(int64_t)8193, (int64_t)20000}) {
            const std::vector<double> x = uniform(n, dim, 10 * dim + (n > 10000));           // (1-D, n = 20000: 6666 cells wanted, 4096 given)
            good("grid, all rows", x, n, dim, m, 0, n, 2);
            good("grid, shard (4096, 4096)", x, n, dim, m, 4096, 4096, 0);
            good("grid, shard (4095, 4097)", x, n, dim, m, 4095, 4097, 2);
            good("grid, shard (0, 4096): brute force only", x, n, dim, m, 0, 4096, 1);
            good("grid, shard (4096, n): grid only", x, n, dim, m, 4096, n, 1);
            good("grid, last row", x, n, dim, m, n - 1, n, 1);
        }
    good("n = 8192: no grid", uniform(8192, 2, 5), 8192, 2, m, 0, 8192, 1);
    good("the longest list", uniform(300, 2, 6), 300, 2, mmax, 0, 300, 1);
    good("the longest list through the grid", uniform(8200, 3, 7), 8200, 3, mmax, 0, 8200, 2);
    good("n = 1", uniform(1, 2, 8), 1, 2, 5, 0, 1, 1);
    {
        const int64_t n = 9000;
        std::vector<double> x = uniform(n, 3, 21);
        for (int64_t i = 0; i < n; ++i) x[(size_t)(i + 2 * n)] *= 1e-9;                      // a thin third dimension: one cell across it
        good("thin third dimension", x, n, 3, m, 0, n, 2);
        for (int64_t i = 0; i < n; ++i) x[(size_t)(i + n)] *= 1e-9;                          // two thin ones
        good("two thin dimensions", x, n, 3, m, 0, n, 2);
        x = uniform(n, 2, 22);
        for (int64_t i = 0; i < n; ++i) x[(size_t)(i + n)] = 0.25;                           // a dimension without extent
        good("flat dimension", x, n, 2, m, 0, n, 2);
        for (int64_t i = 0; i < n; ++i) x[(size_t)i] = -3.5;                                 // all points identical: no grid
        good("identical points", x, n, 2, m, 0, n, 1);
        x = uniform(n, 2, 23);
        x[150] = std::numeric_limits<double>::quiet_NaN();
        good("a NaN coordinate", x, n, 2, m, 0, n, 1);
        x[150] = 0.5;
        x[(size_t)(n + 200)] = std::numeric_limits<double>::infinity();
        good("an Inf coordinate", x, n, 2, m, 0, n, 1);
        x[(size_t)(n + 200)] = -std::numeric_limits<double>::infinity();
        x[0] = std::numeric_limits<double>::quiet_NaN();                                     // (the scan starts from this one)
        good("NaN first and -Inf", x, n, 2, m, 0, n, 1);
        x = uniform(n, 2, 24);
        for (auto &v : x) v = (v - 0.5) * 2.0 * 1.7e308;                                            // finite points, an extent that is not
        good("overflowing extent", x, n, 2, m, 0, n, 1);
        x = uniform(n, 3, 25);
        for (auto &v : x) v = 1e6 + v * 1e-6;                                                // a tiny cloud far from the origin
        good("shifted, tiny extent", x, n, 3, m, 0, n, 2);
        x = uniform(n, 5, 26);
        good("five dimensions: no grid", x, n, 5, m, 0, n, 1);
        good("eight dimensions", uniform(n, 8, 27), n, 8, m, 4095, 4097, 1);
    }
    // ---- refusals: before the device is touched
    {
        const std::vector<double> x = uniform(100, 8, 30);
        refused("dim = 0", x.data(), 100, 0, m, 0, 100);
        refused("dim = 9", x.data(), 88, 9, m, 0, 88);
        refused("m = -1", x.data(), 100, 2, -1, 0, 100);
        refused("m beyond the limit", x.data(), 100, 2, mmax + 1, 0, 100);
        refused("m = 255", x.data(), 100, 2, 255, 0, 100);
        refused("row_begin > row_end", x.data(), 100, 2, m, 51, 50);
        refused("row_end > n", x.data(), 100, 2, m, 0, 101);
        refused("row_begin < 0", x.data(), 100, 2, m, -1, 100);
        refused("n = 0", x.data(), 0, 2, m, 0, 0);
        refused("n = 2^31", x.data(), (int64_t)1 << 31, 2, m, 0, 1);
        refused("NULL locs", nullptr, 100, 2, m, 0, 100);
        refused("NULL NNarray", x.data(), 100, 2, m, 0, 100, true);
        std::vector<int> nn(100 * (m + 1), kSentinel);
        EXPECT(gpv_find_ordered_nn(1, x.data(), 100, 2, m, 0, 100, nn.data()) == GPV_ERR_NO_DEVICE);   // (the mock has one device)
        EXPECT(gpv_find_ordered_nn(-1, x.data(), 100, 2, m, 0, 100, nn.data()) == GPV_ERR_NO_DEVICE);
        EXPECT(nn[0] == kSentinel && mockhip_live_allocations() == 0);
    }
    // ---- every allocation failing in turn: coordinates, output, and the four arrays of the grid
    alloc_failures("brute force", uniform(500, 2, 40), 500, 2, m, 2);
    alloc_failures("five dimensions", uniform(8300, 5, 41), 8300, 5, m, 2);
    for (int dim = 1; dim <= 3; ++dim) alloc_failures("grid", uniform(8300, dim, 42 + dim), 8300, dim, m, 6);
    EXPECT(mockhip_live_allocations() == 0);
    std::printf("nn_driver: %d failed expectation(s); %ld kernel launches swallowed by the mock runtime\n", g_fail, mockhip_launches());
    return g_fail ? 1 : 0;
}
