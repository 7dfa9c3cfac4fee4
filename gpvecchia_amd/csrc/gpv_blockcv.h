// gpv_blockcv.h — launchers of the leave-block-out cross-validation behind gpv_plan_set_blocks / gpv_plan_block_cv
// (gpv_blockcv.hip), and the host builder of the block index.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace gpv {

// Geometry.  ONE wavefront per held-out block and one lane per member: a workgroup is one wavefront of 64 lanes, so the
// barriers between the phases of a block are those of a single wavefront and a block's arithmetic is nobody else's.  LDS per
// workgroup: the lower triangle of Q_BB packed by rows, 64 x 65 / 2 doubles = 16 640 B, and the set's entries by local index,
// 64 doubles = 512 B: 17 152 B, nine workgroups to a CU's 160 KB.  The right-hand sides stay in registers (CP per lane).
constexpr int kBcvMaxBlock = 64;                   // gpv_blockcv_max_block()
constexpr int kBcvThreads = 64;
constexpr int kBcvTri = kBcvMaxBlock * (kBcvMaxBlock + 1) / 2;
constexpr int kBcvBlocksPerCU = 8;                 // grid cap of the block pass (LDS admits nine workgroups to a CU)
constexpr int kBcvMaxCols = 16;                    // = kLooMaxCols
constexpr int kBcvNScores = 8;                     // gpv_blockcv_nscores(), GPV_BLOCKCV_NSCORES
constexpr int kBcvScoreThreads = 256;
constexpr int kBcvScoreBlocksPerCU = 2;            // grid cap (per column) of the score pass

// The block index of a labelling (host; structure only, never the parameters).  Blocks are numbered 0 .. n_blocks - 1 in
// ascending label, empty labels skipped; the members of a block in ascending ORDERED row.
struct BlockIndex {
    int64_t n_blocks = 0, n_heldout = 0, n_set_refs = 0;
    int max_size = 0;
    std::vector<int32_t> memptr;     // [n_blocks + 1] where the members of each block start in members
    std::vector<int32_t> members;    // [n_heldout] internal positions
    std::vector<int32_t> setptr;     // [n_blocks + 1] where the set list of each block starts in sets
    std::vector<int32_t> sets;       // [n_set_refs] stored sets with at least one member (the own entry counts) in the block,
                                     // ascending in stored-set order
    std::vector<int32_t> blkloc;     // [Nlocs][2] by internal position: {block, local index in the block}, {-1, -1}: kept
};

struct BlockCvArgs {
    const double *L;         // [rows][P] U entries by OUTPUT row, left-aligned, the own entry last (LooArgs::L)
    const int32_t *nn;       // [rows][P] internal positions, valid entries right-aligned, -1 = missing
    const int32_t *rowid;    // [rows] output row of each stored set
    const double *g;         // [rows] by OUTPUT row: the scale of the row (LooArgs::g)
    const int32_t *memptr, *members, *setptr, *sets;     // BlockIndex, on the device
    const int2 *blkloc;
    const double *B;         // [Nlocs][CP] the data columns by internal position
    const double *R;         // [Nlocs][CP] Q z by internal position (launch_loo_transposed)
    double *D;               // [Nlocs][CP] out: delta = Q_BB^-1 r_B at the members (the rest is the caller's fill)
    double *Y2;              // [Nlocs][CP] out: y_a^2, R y = r_B: their sum over a block is r_B' Q_BB^-1 r_B
    double *var;             // [Nlocs] out: diag(Q_BB^-1)
    double *nlp;             // [Nlocs] out: -log(pivot_a) of the factor: their sum over a block is -log det Q_BB
    unsigned *nbad;          // ONE counter: blocks with a pivot that is not > 0 (an integer count: order-free)
    int64_t n_blocks;
    int P;
};

int blockcv_grid(int64_t n_blocks, int cus);
int blockcv_score_grid(int64_t n, int cus);
// The labels alone (nothing of the plan is read): 0, or 3 (a label < -1 or >= n, a block of more than kBcvMaxBlock members,
// no block at all).  ids: [n] the block number of each ORDERED location (-1: kept); sizes: [n_blocks].
int blockcv_check_labels(const int32_t *block_of_ord, int64_t n, std::vector<int32_t> &ids,
                                             std::vector<int32_t> &sizes);
// The index.  newpos: [n] internal position of each ordered location, nullptr = the identity.  Returns 0, 1 (rows x P >= 2^31),
// 2 (an index out of range, a missing entry behind a valid one, newpos not a permutation) or 3 (blockcv_check_labels).
int blockcv_build_index(const int32_t *nn, const int32_t *rowid, int64_t rows, int64_t n, int P,
                                            const int32_t *newpos, const int32_t *block_of_ord, BlockIndex &out);
// assembly of Q_BB, factor, solves, variances: cp = 1, 2, 4, 8, 16 columns
hipError_t launch_blockcv_blocks(const BlockCvArgs &a, int cp, int grid, hipStream_t s);
// the epilogue on ORDERED column-major data: Z, DM, Y2 [ncols][n], var, nlp [n].  DM holds delta on entry and the predictive
// mean z - delta on return; a location whose var is not > 0 (kept, or of a bad block) enters no sum.
// part: [ncols][grid][kBcvNScores]; scores: [ncols][kBcvNScores]
hipError_t launch_blockcv_scores(const double *Z, double *DM, const double *Y2, const double *var, const double *nlp,
                                                     int64_t n, int ncols, int grid, double *part, double *scores, hipStream_t s);

}  // namespace gpv
