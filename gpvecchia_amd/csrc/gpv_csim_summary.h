// gpv_csim_summary.h — launchers of the folds of gpv_plan_cond_sim_summary (gpv_csim_summary.hip): what is taken from a batch of
// 16 swept draws X[nq][16] (gpv_csim.hip) while it is still on the device.  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gpv {

constexpr int kCsumCols = 16;                      // = kCsimMaxCols: the columns of a batch; a row of X is one 128-byte line
constexpr int kCsumMaxThr = 8;                     // thresholds at most (= kDrawsMaxThr)
constexpr int kCsumThreads = 256;                  // every kernel: 16 groups of 16 lanes, lane c of a group = column c
constexpr int kCsumGroups = kCsumThreads / kCsumCols;
constexpr int kCsumChunkRows = 128;                // members of a region that ONE group folds, in ascending order: a chunk
constexpr int kCsumStepRows = 4;                   // members of a chunk whose loads are in flight together

// One chunk of a region's member list: the entries beg .. beg + len - 1 of regidx / regw, len in [1, kCsumChunkRows].  The
// chunks of a region are cut from the start of its list, so they depend on the list alone.  slot >= 0: the chunk's partials go
// to part[slot]; slot < 0: the region has this chunk alone and its result is written at once.
struct CsumChunk {
    int64_t beg;
    int64_t slot;
    int32_t len;
    int32_t reg;
};
// A region with no chunk (empty) or with several: its partials part[slot0 .. slot0 + nslots) meet in ascending order.
struct CsumJoin {
    int64_t slot0;
    int32_t nslots;
    int32_t reg;
};

struct CsumArgs {
    const double *X;         // [nq][16] the deviation fields of the batch, as the sweep left them
    const double *mu;        // [nq] mean + offset
    const uint8_t *live;     // [nq] the mean is not NaN
    int64_t nq;
    int nthr;
    double thr[kCsumMaxThr];
    // per location
    double *S1, *S2;         // [nq] running sums of d and d^2, d = g(y) - g(mu)
    uint32_t *cnt;           // [nthr][nq] running counts of y > thr
    // regions, CSR over sweep rows
    int64_t nreg;
    const int32_t *regidx;
    const double *regw;      // nullptr: weights 1
    const CsumChunk *chunk;
    int64_t nchunks;
    const CsumJoin *join;
    int64_t njoin;
    double *part;            // [slots][3 + nthr][16]: total, max, min, areas
    // the batch's result block: column c of region r at [c * nreg + r], the areas at [(c * nthr + t) * nreg + r]
    double *rtot, *rmax, *rmin, *rarea;
};

// mu = mean + offset (offset nullptr: mean), live = the mean is not NaN; mean: [nq] the swept mean column
hipError_t launch_csum_prepare(const double *mean, const double *offset, int64_t nq, double *mu, uint8_t *live, hipStream_t s);
// the per-location sums of one batch; bit c of colmask: column c is one of the requested draws
hipError_t launch_csum_accum(const CsumArgs &a, int link, unsigned colmask, hipStream_t s);
// the region functionals of one batch, all 16 columns: one launch over the chunks, one over the regions that join several or none
hipError_t launch_csum_fold(const CsumArgs &a, int link, hipStream_t s);
// out: [3 + nthr][nq] = mean, mc_mean, mc_var, exceed; NaN where a location is not live.  out may be X.
hipError_t launch_csum_finish(const CsumArgs &a, int link, int64_t ndraws, double *out, hipStream_t s);

}  // namespace gpv
