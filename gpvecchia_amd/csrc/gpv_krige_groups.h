// gpv_krige_groups.h — grouped local kriging of a cond.yz='z' plan (gpv_plan_krige_groups): the launcher of the joint predict
// pass (gpv_krige_groups.hip).  A group of g prediction locations shares one conditioning set of m observations and is one
// (m + g)-row solve in one wavefront.  Not installed.
#pragma once
#include "gpv_krige.h"

namespace gpv {

constexpr int kKrigeGroupMaxRows = 64;            // m + g: the neighbours and the members, one lane each
constexpr int64_t kKrigeGroupChunk = 1 << 16;     // groups per chunk by default (at most 63 members each)
constexpr int kKrigeGroupBuckets = 3;             // row buckets 16, 32, 64

struct KrigeGroupArgs {
    KrigeArgs k;             // the plan's records, the nuggets, the columns and the covariance, as the per-location pass reads them;
                             // k.q: [nq][dim] the chunk's members, k.nnq: [ng][m] per GROUP, k.mean: [ncols][nq], k.var: [nq], k.nq: members
    const int32_t *gptr;     // [ng + 1] first member of each group of the chunk
    const double *w;         // [nq] weights of the members
    const int32_t *list;     // [nlist] the groups of the chunk this launch solves (those of one row bucket)
    const int64_t *coff;     // [ng] offset of each group's packed lower triangle in cov (read when cov != nullptr)
    double *gmean;           // [ncols][ng] out
    double *gvar;            // [ng] out
    double *cov;             // out, or nullptr
    int64_t ng;              // groups of the chunk
    int64_t nlist;
};

// the row bucket of a group is a function of m + g alone: 16, 32 or 64
inline int krige_group_bucket(int rows) { return rows <= 16 ? 0 : (rows <= 32 ? 1 : 2); }
// launches over a.list with the kernel of `bucket` (0, 1, 2: 16, 32, 64 rows); every group of the list has m + g in that bucket
hipError_t launch_krige_groups(const KrigeGroupArgs &a, int bucket, int grid, hipStream_t s);

}  // namespace gpv
