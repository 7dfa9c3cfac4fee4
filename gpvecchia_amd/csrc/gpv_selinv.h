// gpv_selinv.h — launchers of the selected inverse of the posterior factor behind gpv_plan_selinv (gpv_selinv.hip).  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpv {

// Sigma = W^-1 on the pattern of the factor R (W = R R^T, gpv_posterior.hip), one double per entry of the compact blocks C and
// at the same index: S[cb + 1 + e] = Sigma_{row e of column c, c}, the diagonal last (S[cb] is not used).
struct SelinvArgs {
    // one record per column {k, offset of its block in C, entries, first entry in crow}: the columns of the dense top block
    // first, ascending, then the ascending schedule of the mean sweep (PostArgs::meanrec)
    const int4 *rec;
    // [nnz] by entry of crow, for the pair (row i = crow[e], column c): {offset in C of column i's block, first match record of
    // the pair in tp}.  The match records tp[first + l], l = 0 .. position of i in c, hold where row l of column c sits in
    // column i (0xFF: nowhere, the term is dropped: the zero-fill rule of the factor pass).
    const int2 *pair;
    const uint8_t *tp;
    const double2 *C;        // the factor: R_ec = C[cb + 1 + e].y (read only)
    double *S;
    double *vars;            // [Nlocs] Sigma_cc by column
};

constexpr int kSelinvTopMax = 128;     // columns the top kernel takes at most (kTopMax of gpv_posterior_ext.h)

// the tile a level's kernel keeps per column: the smallest of 16, 32, 64 that holds max_entries entries (0: none does)
int selinv_tile(int max_entries);
// the records [0, K) (the dense top block, closed: the rows of its columns are among its columns), one after the other in ONE
// workgroup; toprows[j][e], 64 per column: the index inside the block of the row of entry e of column j
hipError_t launch_selinv_top(const SelinvArgs &a, int K, const uint8_t *toprows, hipStream_t s);
// the records [first, first + count): one level of the schedule, every column at most `tile` entries long
hipError_t launch_selinv_level(const SelinvArgs &a, int first, int count, int tile, hipStream_t s);
// out[k] = k < skip_front ? 0 : vars[k]
hipError_t launch_selinv_out(const double *vars, int64_t n, int64_t skip_front, double *out, hipStream_t s);

}  // namespace gpv
