/*
 * gpvecchia.h — C ABI of libgpvecchia_hip.so, the MI355X (gfx950) engine for the
 * GPvecchia U_NZentries hot path and the log-likelihood reductions fed by it.
 *
 * Plain C: pointers and sizes only, no R / torch / C++ types.  Every entry
 * point names the reference interface it replaces (paths relative to the
 * GPvecchia source tree, v0.1.8).
 *
 * Conventions
 *   - Matrices crossing this boundary are COLUMN-MAJOR (R / Armadillo layout,
 *     src/RcppExports.cpp:57-63) unless a comment says otherwise.
 *   - Index arrays are 1-based with 0 (or NA_INTEGER = INT_MIN) for "missing",
 *     exactly what R/createU.R:146-147 hands to the reference.
 *   - All functions are blocking host calls unless they take a stream.
 *   - Status codes: 0 = ok, > 0 = error (gpv_status_string()).  A non-positive-
 *     definite block is NOT an error (reference: message on Rcerr, zero row,
 *     src/U_NZentries.cpp:64-66); it is reported through n_failed.
 *   - Threading: every call blocks the calling host thread (or is asynchronous on the given stream); a plan may be
 *     used from one thread at a time; different plans may be used concurrently from different threads.  The library
 *     keeps no global state besides what HIP keeps.
 *   - The library never falls back to a CPU path: without a usable GPU every
 *     compute entry returns GPV_ERR_NO_DEVICE.
 */
#ifndef GPVECCHIA_H
#define GPVECCHIA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    GPV_OK = 0,
    GPV_ERR_NO_DEVICE = 1,      /* no HIP device / HIP runtime error at init        */
    GPV_ERR_BAD_ARG = 2,        /* null pointer, negative size, bad shard range      */
    GPV_ERR_COVTYPE = 3,        /* covType not "matern"/"matern_scaledim"/"esqe" (src/U_NZentries.cpp:27-29) */
    GPV_ERR_UNSUPPORTED_NU = 4, /* Matern smoothness not in (0, 60] or not finite                */
    GPV_ERR_UNSUPPORTED_M = 5,  /* m+1 > 192 (m+1 <= 64: unrolled register kernels; up to 192 and any dimension: a slow
                                   workgroup-per-set kernel); m+1 > 64 for gpv_plan_build_posterior and for
                                   gpv_plan_loglik_grad and gpv_plan_loglik_fisher */
    GPV_ERR_HIP = 6,            /* HIP runtime failure (alloc, copy, launch)         */
    GPV_ERR_STATE = 7,          /* call order: result requested before an eval, no data set */
    GPV_ERR_INDEX = 8           /* neighbour index outside [0, Nlocs]                */
};

/* gpv_plan_eval flags */
enum {
    GPV_WANT_U = 1,        /* materialise Lentries (the U factor entries) in HBM              */
    GPV_WANT_LOGLIK_Z = 2, /* fused cond.yz='z' log-likelihood sums (needs gpv_plan_set_data) */
    GPV_WANT_NUMERATOR = 4,/* numerator sums of R/vecchia_likelihood.R:74-76 for any cond.yz  */
    GPV_WANT_DENOM = 8,    /* + posterior pass (U2V) on the GPU for cond.yz='SGV': sums[2] = log det W, sums[3] = quadform.denom
                              (R/vecchia_likelihood.R:85-90); needs gpv_plan_build_posterior; implies WANT_NUMERATOR.  The U
                              entries are materialised (gpv_plan_get_Lentries) only when GPV_WANT_U is asked for as well: the
                              kernel hands the latent entries to the posterior pass directly.
                              Nuggets must be > 0 (+Inf = unobserved is fine): a zero nugget makes W infinite and the sums NaN;
                              the reference removes such rows on the host first (R/createU.R:173-193) */
    GPV_WANT_MEAN = 16,    /* + posterior mean of the latent field in ORDERED layout, mu.ord of R/vecchia_prediction.R:118-126
                              (two triangular solves with the posterior factor); implies GPV_WANT_DENOM */
    GPV_WANT_MEAN_B = 32   /* posterior mean for cond.yz='zy' (the reference's default with prediction locations in >= 2-D,
                              R/vecchia_specify.R:92-96): V.ord is the reversed latent block of U itself, no factorisation
                              (R/vecchia_prediction.R:68-70); mu.ord = -B^-T a by one level-scheduled triangular solve.  The
                              plan holds the rows of the 'zy' revNNarray (n dummy rows, n latent-at-observed rows, prediction
                              rows); data: z_ord for the first n rows, anything (0) for the others; the mean comes back for
                              every row (the first n, the dummies of R/createU.R:166-171, are to be dropped).  Needs
                              gpv_plan_build_posterior; not together with GPV_WANT_DENOM / GPV_WANT_MEAN */
};

/* layout of the 8-double partial-sum vector produced by an eval (summed over the
 * plan's row shard; one all-reduce(sum) over ranks completes it):
 *   [0] sum_k log d_k              d_k = diag(U) of the latent column k (= Lentries[k, n0-1])
 *   [1] sum_k a_k^2                a_k = sum over observed-conditioned neighbours of M_j * z_j   (z1 of :74, latent columns)
 *   [2] sum_k log(tau_k + v_k)     v_k = 1/d_k^2 conditional variance            (cond.yz='z' only)
 *   [3] sum_k (z_k - mu_k)^2/(tau_k+v_k), mu_k = -a_k/d_k                       (cond.yz='z' only)
 *   [4] sum_k z_k^2 / tau_k        (observed columns of z1, :74-75)
 *   [5] sum_k log tau_k
 *   with GPV_WANT_DENOM slots [2],[3] hold instead  log det W  and  z2' W^{-1} z2  (W = U_y U_y^T)
 *   [6] number of rows whose block was not positive definite
 *   [7] number of rows processed
 */
#define GPV_NSUMS 8

typedef struct gpv_plan gpv_plan;

const char *gpv_status_string(int status);
/* GPV_ERR_HIP collapses every HIP runtime failure (out of memory, invalid stream, failed launch ...).  This returns the
 * hipError_t of the last such failure seen by the CALLING host thread (0 = none so far) and, when text != NULL, copies
 * "<hipError name>: <HIP's description> [<failing call>, file:line]" into text (NUL-terminated, at most text_len bytes).
 * The reference reports native failures as R errors carrying the C++ exception text (src/RcppExports.cpp:52,66). */
int gpv_last_hip_error(char *text, int text_len);
int gpv_version(void);                 /* 100*major + minor */
int gpv_device_count(int *count);      /* number of visible HIP devices */
int gpv_max_p(void);                   /* widest supported row length m+1 (192) */

/* -------------------------------------------------------------------------
 * Literal drop-ins for the reference's native entry points.  Signature shape:
 * R's .C() convention (every argument a pointer, outputs caller-allocated), so
 * that an R wrapper needs no compiled glue.
 *
 * Replaces: _GPvecchia_U_NZentries  (src/RcppExports.cpp:51-67, arity 9 at :159)
 *           R stub U_NZentries()    (R/RcppExports.R:22-24), called at R/createU.R:152-154
 *           body                    src/U_NZentries.cpp:25-118
 *   Ncores          accepted for signature parity, unused on the GPU
 *   n               number of observed locations (length of nuggets_obsord)
 *   Nlocs, dim      rows / cols of locs
 *   ncolNN          m+1 = columns of revNNarray / revCondOnLatent
 *   locs            Nlocs x dim double
 *   revNNarray      Nlocs x ncolNN int, 1-based, 0 or NA_INTEGER = missing
 *   revCondOnLatent Nlocs x ncolNN int (R logical: 1 TRUE latent, 0 FALSE observed, NA_INTEGER ignored)
 *   nuggets         Nlocs double (R/createU.R:77), nuggets_obsord n double (R/createU.R:78)
 *   covType         pointer to a C string, "matern", "matern_scaledim" or "esqe"
 *   covparms        ncovparms doubles (3 for matern, 4 for esqe, dim + 2 for matern_scaledim)
 *                   "matern_scaledim": the Matern with one range per coordinate, covparms = (variance, range_1 .. range_dim,
 *                   smoothness).  With h = sqrt(sum_t ((x_t - x'_t) / range_t)^2), summed in coordinate order, it is "matern"
 *                   at distance h and range 1 (the closed forms at smoothness 0.5, 1.5, 2.5, the general branch otherwise;
 *                   h == 0 gives the variance exactly).  Every entry that takes a covType and evaluates accepts it
 *                   (this one, gpv_plan_eval, gpv_mplan_eval*, the Vecchia-Laplace steps), for dim <= 8: each evaluation
 *                   first writes a plan-owned copy of the locations with the coordinates multiplied by 1 / range_t, on its
 *                   own stream, and the set kernel of "matern" runs on that copy.  Checked before the device is touched:
 *                   ncovparms != dim + 2, dim > 8, a range <= 0 or infinite are GPV_ERR_BAD_ARG; a NaN range or variance
 *                   fails every block, like "matern".
 *   Lentries        out, Nlocs x ncolNN double, rows left-aligned and zero padded
 *   Zentries        out, 2n double  (src/U_NZentries.cpp:111-115)
 *   n_failed        out, rows left all-zero because the block was not PD
 *   status          out, GPV_OK or an error code (outputs untouched on error)
 */
void gpv_U_NZentries(const int *Ncores, const int *n, const int *Nlocs, const int *dim, const int *ncolNN,
                     const double *locs, const int *revNNarray, const int *revCondOnLatent,
                     const double *nuggets, const double *nuggets_obsord, const char **covType,
                     const double *covparms, const int *ncovparms, double *Lentries, double *Zentries,
                     int *n_failed, int *status);

/* gpv_U_NZentries keeps the device plan it builds from (locs, revNNarray, revCondOnLatent) and reuses it while the next
 * call passes arrays of the same shape and content (128-bit hash): an unmodified createU (R/createU.R:152-154) called
 * once per optimiser step by vecchia_estimate (R/vecchia_wrappers.R:72-93) pays the re-layout once.  The cached plan
 * holds device memory (about 0.5 GB at Nlocs = 1e6, m = 30) until the next different call or gpv_plan_cache_clear();
 * the environment variable GPV_NO_PLAN_CACHE=1 disables the cache.  Calls are serialised on the cache. */
int gpv_plan_cache_clear(void);
int gpv_plan_cache_stats(int64_t *hits, int64_t *misses);   /* counters since load (either pointer may be NULL) */
/* The 128-bit content hash the plan cache keys on (multi-threaded, result independent of the thread count; not
 * cryptographic), for host code that wants to key a cache of its own on the same arrays: out2[0..1] = hash of `bytes` bytes
 * at ptr under `seed`.  bytes == 0 is valid (ptr may be NULL then). */
int gpv_hash_bytes(const void *ptr, int64_t bytes, uint64_t seed, uint64_t *out2);

/* Replaces: _GPvecchia_U_NZentries_mat (src/RcppExports.cpp:70-86), R/RcppExports.R:26-28,
 * body src/U_NZentries.cpp:126-197, call site R/createU.R:149-151.
 * covVals is the dense Nlocs x Nlocs covariance (column-major); no nugget is added (:144);
 * locs / revCondOnLatent / nuggets / covparms of the reference signature are unused there
 * and therefore not part of this ABI. */
void gpv_U_NZentries_mat(const int *Ncores, const int *n, const int *Nlocs, const int *ncolNN,
                         const int *revNNarray, const double *nuggets_obsord, const double *covVals,
                         double *Lentries, double *Zentries, int *n_failed, int *status);

/* Replaces: _GPvecchia_MaternFun / _GPvecchia_EsqeFun (src/RcppExports.cpp, R-visible through
 * NAMESPACE:3; bodies src/Matern.cpp:24-86, src/Esqe.cpp:17-39).  Elementwise on nelem distances. */
void gpv_MaternFun(const double *distmat, const int *nelem, const double *covparms, double *covmat, int *status);
void gpv_EsqeFun(const double *distmat, const int *nelem, const double *covparms, double *covmat, int *status);

/* -------------------------------------------------------------------------
 * Plan API — the fast path.  A plan is the device-resident image of the
 * parameter-independent vecchia.approx object (R/vecchia_specify.R:234-235,
 * U.prep of R/U_sparsity.R:78-79): uploaded and re-laid-out once, evaluated once
 * per optimiser step (R/vecchia_wrappers.R:72-78 calls vecchia_likelihood each step).
 *
 * A plan owns the rows [row_begin, row_end) of the Nlocs conditioning sets
 * (0-based, half open); locations / nuggets / data are replicated on every
 * plan.  One plan per GPU; rows shard with no data exchange.
 */
int gpv_plan_create(gpv_plan **plan, int device, int64_t Nlocs, int dim, int ncolNN,
                    const double *locs,            /* Nlocs x dim col-major */
                    const int *revNNarray,         /* Nlocs x ncolNN col-major, 1-based, 0/NA missing */
                    const int *revCondOnLatent,    /* Nlocs x ncolNN col-major, R logical */
                    int64_t row_begin, int64_t row_end);
int gpv_plan_destroy(gpv_plan *plan);

/* z in ORDERED observation order (zord of R/vecchia_likelihood.R:68), length Nlocs.
 * Log-likelihood sums assume every location is observed (obs all TRUE, no 'zy').
 * Blocking; it first waits for the stream of the plan's last evaluation, so an eval still in flight on a caller
 * stream never sees half-written data. */
int gpv_plan_set_data(gpv_plan *plan, const double *z_ord);

/* One evaluation = what createU()+vecchia_likelihood_U() trigger per parameter
 * value (R/vecchia_likelihood.R:23-26).  nuggets: n_nuggets == 1 (constant,
 * R/createU.R:74) or == Nlocs (ordered, nuggets.all.ord of R/createU.R:77).
 * Asynchronous on `stream` (a hipStream_t; NULL selects the plan's own non-blocking stream, NOT the HIP
 * null stream: pass the stream your consumer of d_sums_out runs on); results are valid after that stream
 * is synchronised or after a blocking getter.  With a general Matern smoothness (nu not in {0.5, 1.5, 2.5}) the call
 * spends ~1 ms on the host fitting the table of s^nu K_nu(s) for this nu before it enqueues; it does not wait for the
 * stream (the table is double buffered).
 * Evaluations of one plan are ordered by the stream they are enqueued on; an evaluation enqueued on a different stream
 * than the previous one first waits (on the host) for that previous stream, because the plan's buffers are reused.
 * If d_sums_out != NULL the GPV_NSUMS partial sums are ALSO written to that
 * device address (caller-owned, e.g. the buffer an RCCL all-reduce works on). */
int gpv_plan_eval(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms,
                  const double *nuggets, int64_t n_nuggets, int flags, void *stream, double *d_sums_out);

/* Posterior ("U2V") structure for cond.yz='SGV' (R/vecchia_prediction.R:62-83): column/row lists of the latent
 * block of U and a level schedule, from the same revNNarray / revCondOnLatent handed to gpv_plan_create.
 * Requires a plan that owns all rows.  For SGV the factor has no fill, so the fixed-pattern factorisation is
 * exact; for other conditioning patterns it is the zero-fill incomplete factor (the reference's ic0=TRUE). */
int gpv_plan_build_posterior(gpv_plan *plan, const int *revNNarray, const int *revCondOnLatent);
/* The same for patterns that are not cliques -- cond.yz='y' (latent conditioning throughout, R/vecchia_specify.R:186-187), whose
 * factor fills in (R/vecchia_prediction.R:72-83; the reference calls CHOLMOD): the structure is built on the FILLED pattern
 * (symbolic factorisation on the host, once), on which the fixed-pattern factorisation is exact.  Bounded: returns
 * GPV_ERR_UNSUPPORTED_M -- the caller then factorises on the host -- when the filled pattern exceeds max_fill (<= 0: 4) times
 * the entries of the latent block or a column of the factor outgrows 64 rows.  *fill_ratio (may be NULL): filled entries /
 * entries of the latent block (when refused: over the columns processed up to the refusal, a lower bound). */
int gpv_plan_build_posterior_fill(gpv_plan *plan, const int *revNNarray, const int *revCondOnLatent, double max_fill,
                                  double *fill_ratio);
/* Plans whose locsord holds locations WITHOUT an observation (prediction locations, R/vecchia_specify.R:119-149), cond.yz in
 * {SGV, SGVT, y}: obs_ord[k] != 0 iff ordered location k is observed (vecchia.approx$obs); NULL = all observed (the default).
 * The posterior pass then leaves 1/tau_k out of W_kk and z_k/tau_k out of z2 at unobserved k, which is U2V + vecchia_mean of
 * R/vecchia_prediction.R:62-126 for BOTH orderings of prediction plans: with ordering.pred = 'obspred' the reference's third
 * branch (:84-107, prediction columns of U_y unchanged, Cholesky of the observed block only) is what the one factorisation
 * W = R R^T yields by itself (R = B on the prediction columns).  Evaluate with per-location nuggets (n_nuggets == Nlocs, any value
 * at the unobserved locations: 0 in the reference, R/createU.R:75-77) and data 0 there; gpv_plan_get_posterior_mean returns
 * mu.ord over ALL locations (mu.obs and mu.pred after :135-139).  The likelihood sums are not defined for such plans. */
int gpv_plan_set_observed(gpv_plan *plan, const int *obs_ord);
int gpv_plan_posterior_levels(gpv_plan *plan, int *n_levels);
/* blocking: mu.ord (length Nlocs, ordered layout) after an eval with GPV_WANT_MEAN */
int gpv_plan_get_posterior_mean(gpv_plan *plan, double *mu_ord);

/* Var(H y | z) for nrows linear combinations of the latent field (R/vecchia_prediction.R:164-178, vecchia_lincomb), after an
 * eval of this plan with GPV_WANT_DENOM, GPV_WANT_MEAN or GPV_WANT_MEAN_B (the factor of THAT evaluation is used; it is only
 * read, nothing is factorised again).  With W = R R^T the variance of row h is |x|^2, R x = h: one level-scheduled triangular
 * solve for gpv_lincomb_batch() rows at a time.  H in CSR over the plan's ORDERED latent index (hptr: nrows + 1 offsets, hidx
 * in [0, Nlocs), repeated indices within a row add in the order given).  Unit rows give the exact posterior variances
 * (the var.exact path of vecchia_var, :223-244; for a fill-closed factor also the diagonal SelInv returns).
 * vars: nrows out.  cov: NULL, or nrows x nrows (row-major) out -- only for nrows <= gpv_lincomb_batch(), else GPV_ERR_BAD_ARG;
 * its diagonal equals vars bit for bit.  Blocking.  Results are bitwise reproducible from call to call.
 * GPV_ERR_STATE: no posterior structure / no such evaluation yet / a communicator is attached; GPV_ERR_INDEX: an index
 * outside [0, Nlocs).  Arguments are validated before the device is touched. */
int gpv_plan_lincomb(gpv_plan *plan, int64_t nrows, const int64_t *hptr, const int32_t *hidx, const double *hval,
                     double *vars, double *cov);
/* The batched transposed solve R^T x_j = e_j, j < ncols, with the same factor (W = R R^T; for GPV_WANT_MEAN_B, R = B).  For
 * e ~ N(0, I), x = R^-T e has covariance W^-1: mu.ord + x is a draw from the Vecchia posterior of the latent field at every
 * location of the plan.  Column j of E is E + j * lde, length Nlocs, in the plan's ORDERED latent layout; X likewise with ldx,
 * and X may be E itself (then with ldx == lde).  gpv_lincomb_batch() columns share one level-scheduled sweep (the schedule of
 * the posterior mean's R^T u = t); a short last batch is padded with zeros.  The factor is only read and
 * gpv_plan_factor_stamp does not change.  Blocking.  Results are bitwise reproducible from call to call and do not depend on
 * a column's position among the ncols.  For cond.yz = 'zy' plans the n dummy rows in front are outside the contract: pass
 * zeros there, as in H for gpv_plan_lincomb (x is then zero there as well).
 * GPV_ERR_BAD_ARG: a null pointer, ncols < 0, lde or ldx < Nlocs; GPV_ERR_STATE: as for gpv_plan_lincomb; ncols == 0 is GPV_OK.
 * Arguments are validated before the device is touched. */
int gpv_plan_solve_t(gpv_plan *plan, int64_t ncols, const double *E, int64_t lde, double *X, int64_t ldx);
/* Monte-Carlo summaries of posterior draws, reduced on the device.  The standard normal of (ordered location k, draw j) is a
 * function of (seed, k, j) alone: Philox4x32-10 with key (seed low, seed high) and counter (k low, k high, q low, q high),
 * q = j / 2; its four words give two uniforms with 52 random bits in (0, 1), and Box-Muller in FP64 gives draw 2q (cosine) and
 * draw 2q + 1 (sine).  It does not depend on Nlocs, on the batch or on how many draws are asked for.
 *
 * gpv_draws_normals_host: host only, no device needed: the normals of the locations [k0, k0 + nk) and the draws
 * [col0, col0 + ncols); column j at E + j * lde (lde >= nk).  The device's values differ by a few ulp of log / sqrt / sincos.
 * gpv_plan_draws_normals: what the device writes for the draws [col0, col0 + ncols) of a summary with this seed and skip_front,
 * read back: column j at E + j * lde in the plan's ORDERED latent layout (lde >= Nlocs), zeros in the rows k < skip_front.
 *
 * gpv_plan_draws_summary: ndraws draws y = mu_ord + R^-T e (the draws of gpv_plan_solve_t with those normals),
 * gpv_lincomb_batch() per sweep, folded after every sweep; only the results leave the device.  With g the link (0: identity,
 * 1: exp, 2: logistic 1 / (1 + exp(-y))) and d = g(y) - g(mu):
 *   mean[k] = g(mu_k) + sum d / ndraws,  var[k] = (sum d^2 - (sum d)^2 / ndraws) / (ndraws - 1), clamped at 0;
 *   exceed[t * Nlocs + k] = #{draws: y_k > thr[t]} / ndraws, thresholds on the LATENT scale, nthr <= 8;
 *   draw_max[j], draw_mean[j]: maximum and mean of g(y) over the locations k >= skip_front with mask[k] != 0 (mask NULL: all
 *   of them) in draw j; pass both or neither.
 * skip_front: the rows in front that carry no latent variable (the n dummy rows of cond.yz = 'zy'): their normals are zero and
 * their results are zeros.  mu_ord NULL stands for zeros; exceed may be NULL when nthr == 0.
 * State, stream handling and blocking as gpv_plan_solve_t; the factor is only read and gpv_plan_factor_stamp does not change.
 * Results are bitwise reproducible from call to call.  GPV_ERR_BAD_ARG: ndraws < 2, nthr outside [0, 8], link outside {0, 1, 2},
 * skip_front outside [0, Nlocs), a mask that selects nothing, a required pointer NULL, one of draw_max / draw_mean NULL.
 * Arguments are validated before the device is touched. */
int gpv_draws_normals_host(uint64_t seed, int64_t k0, int64_t nk, int64_t col0, int64_t ncols, double *E, int64_t lde);
int gpv_plan_draws_normals(gpv_plan *plan, uint64_t seed, int64_t skip_front, int64_t col0, int64_t ncols, double *E, int64_t lde);
int gpv_plan_draws_summary(gpv_plan *plan, int64_t ndraws, uint64_t seed, int64_t skip_front, const double *mu_ord, int link,
                           int nthr, const double *thr, const uint8_t *mask, double *mean, double *var, double *exceed,
                           double *draw_max, double *draw_mean);
int gpv_lincomb_batch(void);   /* right-hand sides per sweep (32) */
/* The selected inverse of the factor: Sigma = W^-1 on the pattern of R (W = R R^T; for GPV_WANT_MEAN_B, R = B) by the Takahashi
 * recursion, the SelInv branch of vecchia_var (R/vecchia_prediction.R:193-221), in ONE level-scheduled pass over the structure
 * and the factor of the latest evaluation (the schedule of gpv_plan_solve_t): vars_ord[k] = Sigma_kk, every posterior variance
 * of the plan, length Nlocs in the ORDERED latent layout; zeros in the rows k < skip_front (the n dummy rows of cond.yz = 'zy').
 * With column c of R holding the rows N(c) and itself:
 *   Sigma_ic = -(1 / R_cc) sum_{k in N(c)} Sigma_ik R_kc  (i in N(c)),   Sigma_cc = 1 / R_cc^2 - (1 / R_cc) sum_k Sigma_ck R_kc.
 * A term Sigma_ik with i < k both rows of a column c, but i no row of column k, is outside the pattern and counts as 0 (the
 * zero-fill rule of the factor pass).  *n_dropped: the number of such (i, k, c), a property of the structure alone.  0 (fully
 * observed SGV plans, 'z' plans, the filled 'y' structure): vars_ord is diag(W^-1) exactly, what unit rows of gpv_plan_lincomb
 * give.  Otherwise (prediction plans whose sets are no cliques, 'zy') it is the reference's var.exact = FALSE approximation.
 * The factor is only read: gpv_plan_factor_stamp and every later result of the plan stay what they were.  Blocking.  Results are
 * bitwise reproducible from call to call.  GPV_ERR_BAD_ARG: a null pointer, skip_front outside [0, Nlocs); GPV_ERR_STATE: as for
 * gpv_plan_lincomb.  Arguments are validated before the device is touched. */
int gpv_plan_selinv(gpv_plan *plan, int64_t skip_front, double *vars_ord, int64_t *n_dropped);
/* stamp: 0 when the plan holds no factor, else a number that changes with every evaluation that writes one (callers that keep
 * a result of gpv_plan_lincomb's inputs around can tell whether the factor is still the one they mean) */
int gpv_plan_factor_stamp(gpv_plan *plan, int64_t *stamp);

/* Value and analytic gradient of the cond.yz='z' log-likelihood of the plan's data (the density the sums [2], [3] of a
 * GPV_WANT_LOGLIK_Z evaluation describe, R/vecchia_likelihood.R:63-99 with a diagonal W), for gradient-based estimation.
 * Per conditioning set with valid entries J (own point last), S' = C(J, J) + nugget I, u = S'^-1 e_last, w = S'^-1 z_J, q = u'z_J:
 *   l_k = 1/2 log u_last - 1/2 q^2 / u_last - 1/2 log 2 pi,
 *   dl_k/dtheta = -1/2 a / u_last + q b / u_last - 1/2 q^2 a / u_last^2 with a = u'D u, b = w'D u, D = dS'/dtheta elementwise.
 * covType "matern" (covparms = variance, range, smoothness in {0.5, 1.5, 2.5}) or "esqe" (4 covparms); nugget: one constant > 0.
 *   loglik     out: sum of l_k
 *   grad       out, ncovparms + 1: d/d covparms[i], then d/d nugget.  The smoothness entry of "matern" is NaN: the reference's
 *              Matern is discontinuous in nu at the closed-form branches, so it is not differentiated.
 *   n_failed   out: rows whose block was not positive definite (pivot <= 0 or NaN, e.g. a NaN coordinate); they contribute
 *              nothing, and with n_failed > 0 loglik is -Inf (like gpv_loglik_z_from_sums) and every grad entry NaN
 *   row_terms  NULL, or out: Nlocs x (ncovparms + 2) row-major, row k = {l_k, the same derivatives} in the plan's ORDERED row
 *              numbering (NaN in a failed row)
 * Blocking, on the plan's own stream.  Results are bitwise reproducible from call to call.  The plan's last evaluation stays
 * intact: gpv_plan_get_sums, gpv_plan_get_Lentries and gpv_plan_factor_stamp return what they returned before.
 * Arguments are validated before the device is touched.  GPV_ERR_BAD_ARG: a null plan or pointer, ncovparms not 3 / 4, nugget
 * not finite or <= 0; GPV_ERR_COVTYPE; GPV_ERR_UNSUPPORTED_NU: a smoothness other than 0.5, 1.5, 2.5; GPV_ERR_UNSUPPORTED_M:
 * m + 1 > 64; GPV_ERR_STATE: no data set, a communicator attached, a row shard, unobserved locations (gpv_plan_set_observed), or
 * a plan in which some neighbour is conditioned on as latent y (cond.yz other than 'z').
 * covType "matern_scaledim" (ncovparms = dim + 2) is accepted by this entry, gpv_plan_loglik_fisher and gpv_plan_loglik_rep for
 * dim <= 3 and a smoothness in {0.5, 1.5, 2.5}: grad, fisher and row_terms are in the order variance, range_1 .. range_dim,
 * smoothness (NaN, not differentiated), nugget.  dim > 3 is GPV_ERR_STATE: the kernels carry five parameter slots, which the
 * variance, three ranges and the nugget fill.  Another smoothness is GPV_ERR_UNSUPPORTED_NU, from the _nu entries as well, which
 * return for this family what the plain entries return.  The entry writes the plan's scaled copy of the locations itself. */
int gpv_plan_loglik_grad(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms, double nugget,
                         double *loglik, double *grad /* ncovparms + 1 */, int64_t *n_failed,
                         double *row_terms /* NULL, or Nlocs x (ncovparms + 2), row-major */);

/* Value and analytic gradient of the log-likelihood of a plan whose sets condition on latent y (cond.yz = 'SGV', the default of
 * vecchia_specify; R/vecchia_likelihood.R:63-99 with the sparse W), for gradient-based estimation at the default conditioning.
 * Set k with valid entries J (own point l last) and flags c_j (1: conditioned on as latent y, c_l = 1):
 *   S = C(J, J) + nugget diag(1 - c),  u = S^-1 e_l,  M = u / sqrt(u_l);  a_k = sum_{c_j = 0} M_j z_j;  m_k: the latent part of M;
 *   W = sum_k m_k m_k' + I / nugget,  z2 = sum_k m_k a_k - z / nugget,  mu~ = W^-1 z2,  Sigma = W^-1  (on the pattern of W only).
 * With delta_k = a_k - m_k'mu~, v = Sigma_LL m_k over the latent members of the set, f_j = 2 delta_k z_j (c_j = 0),
 * 2 (v_j - delta_k mu~_j) (c_j = 1) and -2 / M_l more at j = l, w~ = S^-1 f, D = dS/dtheta elementwise (the nugget: diag(1 - c)):
 *   c_k = -(w~'D u) / sqrt(u_l) + 1/2 (f'u)(u'D u) / u_l^{3/2},  plus 1/nugget - (Sigma_kk + (z_k + mu~_k)^2) / nugget^2 for the nugget,
 *   d loglik / d theta = -1/2 sum_k c_k.
 * covType, covparms, nugget, grad and n_failed as for gpv_plan_loglik_grad ("matern" at 0.5, 1.5, 2.5 and "esqe").
 *   loglik     out: gpv_loglik_from_sums of the sums of the evaluation this call makes (below)
 *   col_terms  NULL, or out: Nlocs x (ncovparms + 1) row-major, row k = -1/2 c_k in the plan's ORDERED numbering, the nugget's
 *              explicit terms included; the rows sum to grad.  NaN in a failed row.
 * UNLIKE the 'z' entries this call evaluates the plan: it runs gpv_plan_eval(..., GPV_WANT_MEAN) at these parameters on the
 * plan's own stream, then the selected inverse of that evaluation's factor (the pass of gpv_plan_selinv), then one pass over the
 * conditioning sets.  Afterwards the plan's last evaluation IS that evaluation: gpv_plan_get_sums, gpv_plan_get_posterior_mean,
 * gpv_plan_get_Lentries (if materialised), gpv_plan_factor_stamp and a following gpv_plan_selinv return what they return after
 * such a gpv_plan_eval.  Blocking; bitwise reproducible from call to call.
 * Arguments and state are validated before any of this; a refused call leaves every result of the plan as it was (the first
 * call after gpv_plan_build_posterior builds the pass's index data from the plan's arrays, which reads the device).
 * GPV_ERR_BAD_ARG as for gpv_plan_loglik_grad; GPV_ERR_COVTYPE; GPV_ERR_UNSUPPORTED_NU: another smoothness, and
 * "matern_scaledim"; GPV_ERR_UNSUPPORTED_M: m + 1 > 64; GPV_ERR_STATE: no data set, no posterior structure
 * (gpv_plan_build_posterior not called or refused), a filled structure (gpv_plan_build_posterior_fill), unobserved locations, a
 * row shard or a communicator, a structure whose selected inverse drops terms (n_dropped > 0), or index data that do not match
 * the structure.  A cond.yz = 'z' plan with a structure built is accepted: W is diagonal there and the result agrees with
 * gpv_plan_loglik_grad. */
int gpv_plan_loglik_grad_sgv(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms, double nugget,
                             double *loglik, double *grad /* ncovparms + 1 */, int64_t *n_failed,
                             double *col_terms /* NULL, or Nlocs x (ncovparms + 1), row-major */);

/* The value and gradient of gpv_plan_loglik_grad together with the expected Fisher information of the 'z' likelihood, for standard errors and Fisher
 * scoring.  In the notation above, with t_i = D_i u (t = u for the nugget), a_i = u't_i and y_j = S'^-1 t_j, a row contributes
 *   F_k[i][j] = t_i'y_j / u_last - 1/2 a_i a_j / u_last^2
 *             = 1/2 tr(S'^-1 D_i S'^-1 D_j) - 1/2 tr(S'_c^-1 D_i,c S'_c^-1 D_j,c),   c: J without the row's own point,
 * the expectation of -d2 l_k / dtheta_i dtheta_j (and of dl_k/dtheta_i dl_k/dtheta_j) under the exact process; the information
 * is their sum.  It comes out of the pass that computes the gradient: the factorisation of each block is replayed on the
 * ncovparms + 1 vectors t_i, nothing is factorised twice.
 *   loglik, grad, n_failed   as for gpv_plan_loglik_grad
 *   fisher     out, (ncovparms + 1)^2 row-major, parameters in the order of grad; exactly symmetric.  For "matern" every entry
 *              that involves the smoothness is NaN.  With n_failed > 0 every entry is NaN.
 *   row_terms  NULL, or out: Nlocs x (ncovparms + 2 + T) row-major with T = (ncovparms + 1)(ncovparms + 2) / 2, row k =
 *              {l_k, its derivatives, the upper triangle of F_k row-major with i <= j} in the plan's ORDERED row numbering (NaN
 *              in a failed row)
 * Blocking, bitwise reproducible, leaves the plan's last evaluation intact, validates its arguments before the device is touched
 * and returns the statuses of gpv_plan_loglik_grad for the same reasons (fisher NULL: GPV_ERR_BAD_ARG). */
int gpv_plan_loglik_fisher(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms, double nugget,
                           double *loglik, double *grad /* ncovparms + 1 */, double *fisher /* (ncovparms + 1)^2, row-major */,
                           int64_t *n_failed, double *row_terms /* NULL, or Nlocs x (ncovparms + 2 + T), row-major */);

/* gpv_plan_loglik_grad and gpv_plan_loglik_fisher with the smoothness of "matern" differentiated as well: the capability behind
 * gradient-based estimation and standard errors of the model whose smoothness is searched.  Same arguments, same layouts of grad,
 * fisher and row_terms, same state checks, failure semantics and guarantees (blocking, bitwise reproducible, the plan's last
 * evaluation stays intact, arguments validated before the device is touched).
 * For "matern" at any accepted smoothness (finite, > 0, <= 60) other than 0.5, 1.5 and 2.5 the covariance is the general branch
 *   C(r) = sigma^2 c_nu s^nu K_nu(s),  s = r / range,  c_nu = 2^{1-nu} / Gamma(nu)           (no sqrt(2 nu) scaling)
 * which is analytic in nu: all four entries of grad and the full 4 x 4 information are finite,
 *   dC/dsigma^2 = C / sigma^2,   dC/drange = sigma^2 c_nu s^{nu+1} K_{nu-1}(s) / range,
 *   dC/dnu = C (ln s - ln 2 - psi(nu)) + sigma^2 c_nu s^nu dK_nu(s)/dnu,   dK_nu(x)/dnu = int_0^inf e^{-x cosh t} t sinh(nu t) dt.
 * At exactly 0.5, 1.5 and 2.5 the reference's covariance switches to closed forms with another scaling of the distance, so it is
 * not differentiable in nu there: the entries return exactly what gpv_plan_loglik_grad / _fisher return, NaN in the smoothness
 * slot included; likewise for "esqe".  GPV_ERR_UNSUPPORTED_NU is left for a smoothness that no entry accepts.
 * The environment variable GPV_NO_MATERN_TABLE (any value, read at every call) makes the pair passes evaluate the quadrature
 * per pair instead of reading the call's tables: the cross-check of the tables, many times slower. */
int gpv_plan_loglik_grad_nu(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms, double nugget,
                            double *loglik, double *grad /* ncovparms + 1 */, int64_t *n_failed,
                            double *row_terms /* NULL, or Nlocs x (ncovparms + 2), row-major */);
int gpv_plan_loglik_fisher_nu(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms, double nugget,
                              double *loglik, double *grad /* ncovparms + 1 */, double *fisher /* (ncovparms + 1)^2, row-major */,
                              int64_t *n_failed, double *row_terms /* NULL, or Nlocs x (ncovparms + 2 + T), row-major */);
/* The pair functions of the general branch on the host (no device needed), for n arguments s[i] = distance / range >= 0 and
 * sigma^2 = 1: out[3 i] = C, out[3 i + 1] = dC/drange, out[3 i + 2] = dC/dnu.  s = 0 gives exactly {1, 0, 0}; where e^{-s}
 * underflows all three are 0.  Any smoothness in (0, 60] is evaluated by the general formula, the three closed-form values
 * included (there it is NOT the covariance the library evaluates).  GPV_ERR_BAD_ARG: a null pointer with n > 0, n < 0, range not
 * finite or <= 0; GPV_ERR_UNSUPPORTED_NU. */
int gpv_matern_derivs_host(double nu, double range, const double *s, int64_t n, double *out /* 3 n */);

/* Replicated data: R realisations z_1 .. z_R over the plan's locations (an ensemble, repeated time slices, computer-model runs
 * over one design) under one parameter value.  Value, gradient and expected information of sum_r loglik(z_r) come out of ONE pass
 * over the conditioning sets: the factorisation of a block does not depend on the data, and with u, t_p, a_p, y_p = S'^-1 t_p as
 * above a replicate enters only through q_r = u'z_r and b_{p,r} = z_r'y_p (S' is symmetric, so w_r't_p = z_r'y_p):
 *   sum_r l_{k,r}           = R (1/2 log u_last - 1/2 log 2 pi) - 1/2 Q2 / u_last,                      Q2   = sum_r q_r^2
 *   sum_r dl_{k,r}/dtheta_p = -1/2 R a_p / u_last + QB_p / u_last - 1/2 Q2 a_p / u_last^2,             QB_p = sum_r q_r b_{p,r}
 *   information             = R sum_k F_k          (the expected information does not depend on the data)
 * i.e. one gpv_plan_loglik_fisher pass plus ncovparms + 2 dot products per replicate and set.
 *
 * gpv_plan_set_replicates uploads the columns once and keeps them on the device, packed by internal position:
 *   Z_ord   R columns of length Nlocs in the plan's ORDERED row numbering, column-major with leading dimension ldz >= Nlocs
 *           (rows Nlocs .. ldz - 1 of a column are not read)
 *   R       > 0; R = 0 releases the buffer (Z_ord is then not read) and leaves the plan without replicates
 * A second call replaces the first upload.  The column of gpv_plan_set_data is a separate thing: neither call touches the
 * other's data, and gpv_plan_loglik_rep needs no gpv_plan_set_data.  GPV_ERR_BAD_ARG (before the device is touched): a null
 * plan, R < 0, with R > 0 a null Z_ord or ldz < Nlocs.  gpv_plan_replicates returns the R in effect (0: none).
 *
 * gpv_plan_loglik_rep: arguments, layouts of grad, fisher and row_terms, and statuses of gpv_plan_loglik_fisher, with every
 * quantity summed over the replicates (row_terms: row k = {sum_r l_{k,r}, its derivatives, the triangle of R F_k}); fisher may
 * be NULL (value and gradient only).  Values must be finite: a NaN in Z_ord gives NaN sums, not a failed row.  n_failed, -Inf and
 * NaN as for gpv_plan_loglik_fisher; NaN in the smoothness slots of "matern" exactly where the one-column entries put it.
 * gpv_plan_loglik_rep_nu differentiates the smoothness as gpv_plan_loglik_fisher_nu does.  At R = 1 the result agrees with
 * gpv_plan_loglik_fisher on the same column to rounding, not bitwise (b takes another route).
 * Blocking, on the plan's own stream; two ordinary launches; bitwise reproducible from call to call.  Arguments and state are
 * validated before the device is touched.  The plan's last evaluation, its data column and its factor stamp stay intact:
 * gpv_plan_get_sums, gpv_plan_get_Lentries, gpv_plan_factor_stamp and a following gpv_plan_loglik_grad return what they returned
 * before.  GPV_ERR_STATE: no replicates set, a communicator attached, a row shard, unobserved locations, latent conditioning;
 * GPV_ERR_UNSUPPORTED_M: m + 1 > 64; the other statuses as for gpv_plan_loglik_grad. */
int gpv_plan_set_replicates(gpv_plan *plan, const double *Z_ord, int64_t ldz, int R);
int gpv_plan_replicates(gpv_plan *plan, int *R);
int gpv_plan_loglik_rep(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms, double nugget,
                        double *loglik, double *grad /* ncovparms + 1 */,
                        double *fisher /* NULL, or (ncovparms + 1)^2, row-major */, int64_t *n_failed,
                        double *row_terms /* NULL, or Nlocs x (ncovparms + 2 + T), row-major */);
int gpv_plan_loglik_rep_nu(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms, double nugget,
                           double *loglik, double *grad /* ncovparms + 1 */,
                           double *fisher /* NULL, or (ncovparms + 1)^2, row-major */, int64_t *n_failed,
                           double *row_terms /* NULL, or Nlocs x (ncovparms + 2 + T), row-major */);

/* The Vecchia whitening operator of the plan's latest evaluation applied to a block of columns, and their Gram matrix: the
 * primitive behind a generalised-least-squares trend (profile likelihood) and behind the likelihood of replicated data, which
 * share one factor.  Everything is in the plan's ORDERED row numbering.  For row k of a cond.yz='z' plan with the stored entries
 * L_kj of that evaluation (neighbours j in J_k), its own entry d_k (the last one) and its nugget tau_k, a column b whitens to
 *   e_k(b) = (b_k + (sum_{j in J_k} L_kj b_j) / d_k) / sqrt(tau_k + 1/d_k^2),      logdet = sum_k log(tau_k + 1/d_k^2):
 * the standardised conditional residual of z_k given its neighbours' z under C + tau I, i.e. the density the sums [2], [3]
 * describe: sum_k e_k(z)^2 is sums[3] and logdet is sums[2].  Needs an evaluation with GPV_WANT_U: the factor in HBM and the
 * nuggets of THAT evaluation (a constant or a vector) are read, nothing is factorised again.
 *   B_ord     ncols columns of length Nlocs, column-major with leading dimension ldb >= Nlocs (as gpv_plan_solve_t takes E)
 *   E_ord     NULL, or out: the whitened columns, Nlocs x ncols with leading dimension lde >= Nlocs
 *   gram      out, ncols x ncols row-major: E^T E, exactly symmetric
 *   logdet    out
 *   n_failed  out: rows whose block was not positive definite in that evaluation (sums[6]); with n_failed > 0 gram and logdet
 *             are NaN, and so is every entry of E in such a row
 * 1 <= ncols <= gpv_whiten_max_cols().  Blocking, on the plan's own stream; buffers are allocated on first use and belong to the
 * plan.  Bitwise reproducible from call to call.  The plan's last evaluation stays intact: gpv_plan_get_sums,
 * gpv_plan_get_Lentries, the posterior state and gpv_plan_factor_stamp return what they returned before.
 * Arguments and state are validated before the device is touched.  GPV_ERR_BAD_ARG: a null plan or pointer (E_ord excepted),
 * ncols outside [1, 16], ldb < Nlocs, lde < Nlocs with E_ord given; GPV_ERR_STATE: the plan's latest evaluation did not ask for
 * GPV_WANT_U (or there was none, or something has rewritten its nuggets since: a Vecchia-Laplace step), a communicator
 * attached, a row shard, unobserved locations (gpv_plan_set_observed), or a plan in which some neighbour is conditioned on as
 * latent y (cond.yz other than 'z'). */
int gpv_whiten_max_cols(void);         /* 16 */
int gpv_plan_whiten(gpv_plan *plan, const double *B_ord, int64_t ldb, int ncols,
                    double *E_ord /* NULL, or Nlocs x ncols, leading dimension lde */, int64_t lde,
                    double *gram /* ncols x ncols row-major, exactly symmetric */,
                    double *logdet, int64_t *n_failed);

/* The colouring operator of the plan's latest evaluation: the exact inverse of the whitening operator above, and with it
 * simulation from the Vecchia model.  A column e colours to
 *   b_k = sqrt(tau_k + 1/d_k^2) e_k - (sum_{j in J_k} L_kj b_j) / d_k,      k = 0, 1, .., Nlocs - 1 in the ORDERED row sequence
 * (every j in J_k precedes k), so that gpv_plan_whiten of b returns e, and for e ~ N(0, I) the column b is a draw from the
 * Vecchia approximation of N(0, C + tau I) that the evaluation describes: the density whose log the cond.yz='z' likelihood is.
 * Reads the factor in HBM (GPV_WANT_U), the index arrays and the nuggets of THAT evaluation (a constant or a vector); nothing is
 * factorised again, every family an evaluation accepts is covered.  The rows are solved level by level (level(k) = 0 for a row
 * without neighbours, else 1 + max_j level(j)); the schedule is built from the plan's index arrays at first use.  A level of
 * more than gpv_unwhiten_narrow() rows is one kernel launch, a maximal run of consecutive narrower levels is one launch of one
 * workgroup.  Bitwise reproducible from call to call, with or without GPV_NO_GRAPH=1.
 *   gpv_plan_unwhiten_levels  builds the schedule if it is absent; out: the number of levels and of launches per sweep (the runs
 *             of narrow levels plus the wide levels).  GPV_ERR_STATE for a row shard or a plan with latent conditioning.
 *   gpv_plan_unwhiten   E_ord: 1 <= ncols <= gpv_whiten_max_cols() columns of length Nlocs, column-major with leading dimension
 *             lde >= Nlocs, in the ORDERED row numbering; B_ord (leading dimension ldb >= Nlocs) may be E_ord.  n_failed: rows
 *             whose block was not positive definite in that evaluation; with n_failed > 0 every entry of B_ord is NaN.
 *   gpv_plan_simulate   colours the library's own normals: the normal of (ordered location k, draw j) is the function of
 *             (seed, k, j) of gpv_draws_normals_host, made on the device.  Z_ord: the draws col0 .. col0 + ncols - 1, any
 *             ncols >= 1, Nlocs x ncols with leading dimension ldz.  Draw j is always computed in the batch of the 16 draws
 *             [16 floor(j / 16), + 16): a column is bitwise independent of col0, of ncols and of its neighbours in the call.
 * Blocking, on the plan's own stream; buffers are allocated on first use and belong to the plan.  The plan's last evaluation
 * and what a following gpv_plan_whiten returns stay as they were (sums, Lentries, posterior state, factor stamp).  Arguments
 * and state are validated before the device is touched, with the statuses of gpv_plan_whiten: GPV_ERR_BAD_ARG for a null
 * pointer, a column count out of range or a leading dimension < Nlocs; GPV_ERR_STATE where gpv_plan_whiten returns it. */
int gpv_unwhiten_narrow(void);         /* 256 */
int gpv_plan_unwhiten_levels(gpv_plan *plan, int64_t *n_levels, int64_t *n_launches);
int gpv_plan_unwhiten(gpv_plan *plan, const double *E_ord, int64_t lde, int ncols, double *B_ord, int64_t ldb,
                      int64_t *n_failed);
int gpv_plan_simulate(gpv_plan *plan, uint64_t seed, int64_t col0, int64_t ncols, double *Z_ord, int64_t ldz,
                      int64_t *n_failed);

/* The TRANSPOSE of the whitening operator, precision products and leave-one-out cross-validation.  With T the whitening
 * operator of gpv_plan_whiten (row k: T_kk = 1/s_k, T_kj = L_kj / (d_k s_k), s_k = sqrt(tau_k + 1/d_k^2)) the precision matrix of
 * the data vector under the cond.yz='z' likelihood is Q = T^T T, and for a Gaussian model no refitting is needed:
 *   E[z_i | z_-i] = z_i - (Q z)_i / Q_ii,        Var[z_i | z_-i] = 1 / Q_ii.
 * T^T reads the factor by column; the transposed index (for every location the stored entries that name it: 4 bytes per stored
 * entry plus 8 bytes per location) is built on the host from the plan's index arrays at first use, kept with the plan and never
 * rebuilt.  The passes gather, nothing is scattered and there are no floating-point atomics: results are bitwise reproducible
 * from call to call, and a column's bits do not depend on the other columns of the call.  Everything is in the ORDERED row
 * numbering, column-major with the given leading dimensions.
 *   gpv_plan_whiten_t    B = T^T E
 *   gpv_plan_precision   R = Q B = T^T (T B); qdiag: NULL, or out: diag Q (Nlocs)
 *   gpv_plan_loo         from r = Q z and q = diag Q per column: mean (NULL, or Nlocs x ncols, leading dimension ldm) the
 *             leave-one-out predictive means z_i - r_i / q_i; var (NULL, or Nlocs) the leave-one-out variances 1 / q_i, the same
 *             for every column; scores (ncols x GPV_LOO_NSCORES, row-major) per column, with s_i = r_i / sqrt(q_i):
 *               [0] sum (z_i - mean_i)^2   [1] sum |z_i - mean_i|   [2] sum s_i^2   [3] sum log var_i
 *               [4] sum CRPS_i, CRPS_i = sqrt(var_i) [s_i (2 Phi(s_i) - 1) + 2 phi(s_i) - 1/sqrt(pi)]
 *               [5] the count of |s_i| <= 1.959963984540054
 *             the log predictive density is -(Nlocs log(2 pi) + [3] + [2]) / 2.
 *   gpv_plan_loo_index   builds the transposed index if it is absent; out: its entries (own entries are not listed), the longest
 *             column and the number of empty columns.  Needs no evaluation.
 *   gpv_loo_index_host   the builder itself on host arrays, a plan's layout: nn [rows][P] internal positions, valid entries
 *             right-aligned, -1 = missing, the own point last; rowid [rows] the output row of each stored set.  Out: colptr
 *             (Nlocs + 1 starts), owner (Nlocs: flat offset output row x P + left-aligned slot of the own entry of the first set
 *             that ends in the position, -1: none), col (NULL, or col_cap entries: the flat offsets of the entries that name
 *             each position, ascending in stored-set order; a further set that ends in an owned position lists its own entry
 *             here), *nnz their number.  GPV_ERR_INDEX for rows x P >= 2^31 (tested before any array is read).
 * 1 <= ncols <= gpv_whiten_max_cols().  n_failed: rows whose block was not positive definite in that evaluation; with
 * n_failed > 0 every output is NaN.  Blocking, on the plan's own stream; buffers are allocated on first use and belong to the
 * plan.  The plan's last evaluation and what gpv_plan_whiten left on the device stay as they were (sums, Lentries, posterior
 * state, factor stamp).  Arguments and state are validated before the device is touched, with the statuses of gpv_plan_whiten:
 * GPV_ERR_BAD_ARG for a null pointer (the optional outputs excepted), a column count out of range or a leading dimension
 * < Nlocs; GPV_ERR_STATE where gpv_plan_whiten returns it; GPV_ERR_INDEX for a plan with rows x P >= 2^31 (the flat offsets of the
 * index are 32-bit). */
#define GPV_LOO_NSCORES 6
int gpv_loo_nscores(void);             /* GPV_LOO_NSCORES */
int gpv_plan_whiten_t(gpv_plan *plan, const double *E_ord, int64_t lde, int ncols, double *B_ord, int64_t ldb,
                      int64_t *n_failed);
int gpv_plan_precision(gpv_plan *plan, const double *B_ord, int64_t ldb, int ncols, double *R_ord, int64_t ldr,
                       double *qdiag /* NULL, or Nlocs */, int64_t *n_failed);
int gpv_plan_loo(gpv_plan *plan, const double *Z_ord, int64_t ldz, int ncols,
                 double *mean /* NULL, or Nlocs x ncols, leading dimension ldm */, int64_t ldm, double *var /* NULL, or Nlocs */,
                 double *scores /* ncols x GPV_LOO_NSCORES, row-major */, int64_t *n_failed);
int gpv_plan_loo_index(gpv_plan *plan, int64_t *n_entries, int64_t *max_column, int64_t *n_empty);
int gpv_loo_index_host(const int32_t *nn, const int32_t *rowid, int64_t rows, int64_t Nlocs, int P, int32_t *colptr,
                       int32_t *owner, int32_t *col /* NULL, or col_cap entries */, int64_t col_cap, int64_t *nnz);

/* Leave-BLOCK-out cross-validation: hold a whole set B of locations out and predict it from the rest.  With Q = T^T T as above,
 * exactly and without refitting,
 *   z_B | z_-B  ~  N( z_B - Q_BB^-1 (Q z)_B ,  Q_BB^-1 ).
 * A block is any set of at most gpv_blockcv_max_block() = 64 locations (a spatial tile, scattered points, a coincident pair); a
 * block of one is leave-one-out, and one block of every location returns the prior mean and the plan's log-likelihood as its
 * joint density.  For each block the device assembles the dense Q_BB (Q_ab = sum over the conditioning sets that hold both a and
 * b of T_ka T_kb), factors it and solves, one wavefront per block; r = Q z comes from the passes of gpv_plan_precision.  It
 * gathers, nothing is scattered, there are no floating-point atomics: calls repeat bit for bit, a column's bits do not depend
 * on the call's other columns, and the mean and variance of a block depend on its own members only, not on which other blocks
 * exist or how they are labelled.  Scope and statuses are those of gpv_plan_loo.
 *   gpv_plan_set_blocks  block_of_ord[i], i the ORDERED row: -1 = never held out (stays in the conditioning data), or a block
 *             id in [0, Nlocs); ids without a member are skipped, the members of a block are taken in ascending ordered row.
 *             Builds the block index on the host (structure only: it needs no evaluation and stays with the plan until the
 *             labels are replaced) and reports the number of blocks, of held-out locations, the largest block and the length of
 *             the set lists (per block the stored sets with at least one member in it: 4 bytes each, plus 12 bytes per location).
 *             GPV_ERR_BAD_ARG for a label out of range, a block of more than 64 or no block at all, decided before the device is
 *             touched; a refused call leaves the plan's current blocks as they were.
 *   gpv_plan_block_cv    mean (NULL, or Nlocs x ncols, leading dimension ldm) the predictive means, var (NULL, or Nlocs)
 *             diag(Q_BB^-1), the same for every column: both NaN at a location labelled -1.  scores (ncols x
 *             GPV_BLOCKCV_NSCORES, row-major), sums over the N_h held-out locations only, with s = (z - mean) / sqrt(var):
 *               [0] .. [5] as gpv_plan_loo with this mean and variance
 *               [6] sum over the blocks of r_B' Q_BB^-1 r_B      [7] - sum over the blocks of log det Q_BB (the same in every column)
 *             the joint log predictive density of all blocks is -(N_h log(2 pi) + [7] + [6]) / 2.  A block with a pivot that is
 *             not > 0 is counted in n_bad_blocks, returns NaN and stays out of the sums.  GPV_ERR_STATE without blocks; n_failed
 *             as gpv_plan_loo: with n_failed > 0 every output is NaN.  The plan's last evaluation and what gpv_plan_whiten and
 *             gpv_plan_loo left on the device stay as they were.
 *   gpv_blocks_index_host   the builder itself on host arrays (nn, rowid as gpv_loo_index_host; newpos: the internal position of
 *             each ordered row, NULL = the identity).  Out, each NULL or of the documented size: memptr (n_blocks + 1; Nlocs + 1
 *             always suffices), members (n_heldout internal positions), setptr (n_blocks + 1), sets (sets_cap >= n_set_refs stored
 *             sets, ascending per block), blkloc (Nlocs x 2 by internal position: block and local index, -1 -1 = kept). */
#define GPV_BLOCKCV_NSCORES 8
int gpv_blockcv_nscores(void);         /* GPV_BLOCKCV_NSCORES */
int gpv_blockcv_max_block(void);       /* 64 */
int gpv_plan_set_blocks(gpv_plan *plan, const int32_t *block_of_ord /* Nlocs: -1 or id in [0, Nlocs) */,
                        int64_t *n_blocks, int64_t *n_heldout, int *max_size, int64_t *n_set_refs);
int gpv_plan_block_cv(gpv_plan *plan, const double *Z_ord, int64_t ldz, int ncols,
                      double *mean /* NULL, or Nlocs x ncols */, int64_t ldm, double *var /* NULL, or Nlocs */,
                      double *scores /* ncols x GPV_BLOCKCV_NSCORES, row-major */,
                      int64_t *n_failed, int64_t *n_bad_blocks);
int gpv_blocks_index_host(const int32_t *nn, const int32_t *rowid, int64_t rows, int64_t Nlocs, int P,
                          const int32_t *newpos /* NULL, or Nlocs */, const int32_t *block_of_ord,
                          int64_t *n_blocks, int64_t *n_heldout, int *max_size, int64_t *n_set_refs,
                          int32_t *memptr, int32_t *members, int32_t *setptr,
                          int32_t *sets /* NULL, or sets_cap entries */, int64_t sets_cap, int32_t *blkloc);

/* Vecchia-Laplace Newton-Raphson with the state on the device: calculate_posterior_VL of R/vecchia_laplace_NR.R:31-155
 * for fully observed data.  model: position in the reference's family list (:32): 0 gaussian, 1 logistic, 2 poisson,
 * 3 gamma, 4 beta, 5 gamma_alt.  likparms = {alpha, sigma} (:33), for beta {alpha, sigma, beta}.
 * z_ord / prior_mean_ord / y_init_ord: ORDERED layout, length Nlocs; prior_mean_ord NULL = 0, y_init_ord NULL = prior
 * mean (:81-82).  Needs gpv_plan_build_posterior.
 * One gpv_plan_vl_step = one pass of the loop body (:91-129): Hessian/score of the family, pseudo-data and
 * pseudo-nuggets (elementwise kernel), then the plan's ordinary evaluation with GPV_WANT_MEAN (U_NZentries with vector
 * nuggets, U2V, vecchia_mean) and y <- mu + prior_mean.  Returns *dmax = max|y_new - y_prev| (NaN if any entry is NaN:
 * the reference then stops and keeps y_prev) and *flags: bit 0 = a negative Hessian occurred (the reference stops with
 * "Negative variances occurred", :95-98), bit 1 = a non-finite score (:102).  Blocking; only these scalars cross PCIe. */
int gpv_plan_vl_begin(gpv_plan *plan, int model, const double *likparms, const double *z_ord,
                      const double *prior_mean_ord, const double *y_init_ord);
int gpv_plan_vl_step(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms, double *dmax, int *flags);
/* results of the last step in ordered layout (any pointer may be NULL): posterior mean mu.obs + prior_mean,
 * t = pseudo.data + prior_mean, D (:141-144) */
int gpv_plan_vl_get(gpv_plan *plan, double *mean_ord, double *t_ord, double *D_ord);
/* Round 3 additions to the loop above.
 *   model 4 = beta (R/vecchia_laplace_NR.R:283-295; digamma / trigamma on the device), likparms = {alpha, sigma, beta}.
 *   Missing observations: z = NaN (:45-46).  Their pseudo-data / pseudo-nuggets are the substitutes removeNAs of
 *   vecchia_prediction makes (R/vecchia_likelihood.R:45-58: mean and 1e8 x variance of the observed pseudo-data), computed
 *   on the device every step; the convergence test runs over the observed entries only (:84,:115-117).
 *   gpv_plan_set_user_order: ord.z of the vecchia.approx (1-based), uploaded once; the *_user entry points then take and
 *   return vectors in the CALLER's layout and reorder on the device.  In gpv_plan_vl_get_user a missing observation keeps
 *   the substituted pseudo-data in t (the reference has NA there).
 *   gpv_plan_vl_restart: the loop again from the start value of the last begin with the data already resident (what an
 *   optimiser over covparms needs: z, prior mean and start value do not change between its steps); likparms NULL = unchanged.
 *   gpv_plan_vl_loglik: the three terms of vecchia_laplace_likelihood (R/vecchia_laplace_NR.R:376-409) from the state the
 *   last step left on the device: terms[0] pseudo-marginal Vecchia likelihood (one more evaluation with the posterior pass),
 *   terms[1] model_llh(mean, z), terms[2] pseudo-conditional density; loglik = terms[0] - terms[2] + terms[1]. */
int gpv_plan_set_user_order(gpv_plan *plan, const int *ord_z);
int gpv_plan_vl_begin_user(gpv_plan *plan, int model, const double *likparms, const double *z, const double *prior_mean,
                           const double *y_init);
int gpv_plan_vl_restart(gpv_plan *plan, const double *likparms);
int gpv_plan_vl_get_user(gpv_plan *plan, double *mean, double *t, double *D);
int gpv_plan_vl_loglik(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms, double *terms /* 3 */);

/* blocking getters (synchronise the eval's stream first) */
int gpv_plan_get_sums(gpv_plan *plan, double *sums /* GPV_NSUMS */);
int gpv_plan_get_Lentries(gpv_plan *plan, double *Lentries /* (row_end-row_begin) x ncolNN col-major */);
int gpv_plan_get_Zentries(gpv_plan *plan, double *Zentries /* 2*(row_end-row_begin) */);
/* device views for callers that keep U on the GPU: row-major [rows][ld] doubles */
int gpv_plan_Lentries_device(gpv_plan *plan, double **d_ptr, int64_t *ld);
int gpv_plan_rows(gpv_plan *plan, int64_t *row_begin, int64_t *row_end);
/* the shape the plan was created with: Nlocs (rows of locsord = length of z_ord, of a nugget vector, of the posterior mean),
 * dim, ncolNN (= m + 1).  A binding sizes and checks its buffers from these, never from caller-supplied lengths
 * (bindings/R/src/gpvR_plan.c).  Any pointer may be NULL. */
int gpv_plan_dims(gpv_plan *plan, int64_t *Nlocs, int *dim, int *ncolNN);
/* milliseconds the last eval's conditioning-set kernel took on the device (hipEvent pair around that launch) */
int gpv_plan_last_kernel_ms(gpv_plan *plan, double *ms);
/* which conditioning-set kernel the last eval ran, as bit flags: bit 0 = the likelihood-only (lower-triangle) sweep, bit 1 = its
 * lean variant (plan and parameters let it skip the per-task safety work; GPV_NO_LEAN=1 in the environment never selects it).
 * 0 before the first eval.  The results do not depend on it bit for bit; tests and tuning runs read it. */
int gpv_plan_last_set_kernel(gpv_plan *plan);
/* on = 0: evaluations no longer record that event pair (two queue packets per evaluation; they matter only when an
 * evaluation is a fraction of a millisecond, e.g. one rank's shard of an 8-GPU job) and gpv_plan_last_kernel_ms returns
 * GPV_ERR_STATE; default on */
int gpv_plan_set_kernel_timing(gpv_plan *plan, int on);

/* cond.yz='z' log-likelihood from the (all-reduced) sums; n = number of observations.
 * Closed form of R/vecchia_likelihood.R:63-99 when W = U_y U_y^T is diagonal.
 * sums[6] > 0 (some block was not positive definite) gives -Inf, like the reference: the failed row of Lentries
 * stays zero (src/U_NZentries.cpp:64-66), diag(U) = 0, logdet.num = +Inf (R/vecchia_likelihood.R:76,95-96). */
int gpv_loglik_z_from_sums(const double *sums, int64_t n, double *loglik);
/* general form of R/vecchia_likelihood.R:95-96 from sums produced with GPV_WANT_DENOM */
int gpv_loglik_from_sums(const double *sums, int64_t n, double *loglik);
/* numerator pieces of R/vecchia_likelihood.R:74-76: logdet.num, quadform.num */
int gpv_numerator_from_sums(const double *sums, double *logdet_num, double *quadform_num);

/* -------------------------------------------------------------------------
 * Several GPUs from ONE host process (an R session has one): one plan per listed device, contiguous row shards,
 * replicated locations / data; gpv_mplan_eval starts every device, then adds the GPV_NSUMS partial sums on the host
 * in device order (64 bytes per device; deterministic).  Flags: GPV_WANT_U | GPV_WANT_LOGLIK_Z | GPV_WANT_NUMERATOR
 * (the posterior pass does not shard).  `devices` may name a device more than once (then its shards share it). */
typedef struct gpv_mplan gpv_mplan;
int gpv_mplan_create(gpv_mplan **mplan, const int *devices, int ndev, int64_t Nlocs, int dim, int ncolNN,
                     const double *locs, const int *revNNarray, const int *revCondOnLatent);
int gpv_mplan_destroy(gpv_mplan *mplan);
int gpv_mplan_set_data(gpv_mplan *mplan, const double *z_ord);
int gpv_mplan_eval(gpv_mplan *mplan, const char *covType, const double *covparms, int ncovparms, const double *nuggets,
                   int64_t n_nuggets, int flags, double *sums /* GPV_NSUMS, host */);
int gpv_mplan_get_Lentries(gpv_mplan *mplan, double *Lentries /* Nlocs x ncolNN col-major */);

/* REPLICAS: one COMPLETE plan (all rows) per listed device.  This is what several GPUs mean for the parts of the path that
 * do not shard -- the posterior pass U2V of cond.yz='SGV' (R/vecchia_prediction.R:62-83) and therefore every Newton step of
 * vecchia_laplace_likelihood (R/vecchia_laplace_NR.R:88-130; BASELINE.json configs[4]): each device evaluates ITS OWN
 * parameter vector (simplex vertices, grid points, restarts of vecchia_estimate) or its own data set, all in flight
 * together.  gpv_mplan_eval / gpv_mplan_get_Lentries are for row shards and refuse a replica set; the functions below
 * refuse a sharded one.  `devices` may name a device more than once.
 *   gpv_mplan_set_data            the same ordered data on every replica
 *   gpv_mplan_set_data_one        ordered data of one replica
 *   gpv_mplan_build_posterior     gpv_plan_build_posterior on every replica
 *   gpv_mplan_eval_each           covparms: count x ncovparms (row r = replica r), nuggets: one constant nugget per replica,
 *                                 sums: count x GPV_NSUMS out; every replica is enqueued before any is awaited
 *   gpv_mplan_vl_begin_one / _vl_step_each / _vl_get_one   the Vecchia-Laplace loop of gpv_plan_vl_*, the Newton steps of all
 *                                 ACTIVE replicas (active[r] != 0, NULL = all) in flight together; dmax / flags: one per replica */
int gpv_mplan_create_replicas(gpv_mplan **mplan, const int *devices, int ndev, int64_t Nlocs, int dim, int ncolNN,
                              const double *locs, const int *revNNarray, const int *revCondOnLatent);
int gpv_mplan_count(gpv_mplan *mplan, int *n);
int gpv_mplan_set_data_one(gpv_mplan *mplan, int replica, const double *z_ord);
int gpv_mplan_build_posterior(gpv_mplan *mplan, const int *revNNarray, const int *revCondOnLatent);
int gpv_mplan_eval_each(gpv_mplan *mplan, const char *covType, const double *covparms, int ncovparms, const double *nuggets,
                        int flags, double *sums);
int gpv_mplan_vl_begin_one(gpv_mplan *mplan, int replica, int model, const double *likparms, const double *z_ord,
                           const double *prior_mean_ord, const double *y_init_ord);
int gpv_mplan_vl_step_each(gpv_mplan *mplan, const char *covType, const double *covparms, int ncovparms, const int *active,
                           double *dmax, int *flags);
int gpv_mplan_vl_get_one(gpv_mplan *mplan, int replica, double *mean_ord, double *t_ord, double *D_ord);

/* -------------------------------------------------------------------------
 * Several GPUs, ONE PROCESS PER GPU (an MPI-style launch, or torch.distributed.run): each rank creates a plan
 * for its own contiguous block of rows (row_begin / row_end of gpv_plan_create; src/U_NZentries.cpp:37-39: rows never
 * read or write each other) and attaches a communicator.  Every gpv_plan_eval of that plan then sums the GPV_NSUMS
 * partial sums over the ranks with ONE RCCL all-reduce (64 bytes over xGMI), enqueued by the library on the evaluation's
 * own stream right behind the kernel -- no second stream, no event hop, no framework in between -- and gpv_plan_get_sums
 * returns the totals of the WHOLE job on every rank.  RCCL is bound at run time (dlopen of librccl.so.1; GPV_RCCL_LIB
 * names another file): without it these three entries return GPV_ERR_STATE and the rest of the library is unaffected.
 *   id128: 128 bytes (ncclUniqueId); rank 0 fills it with gpv_comm_unique_id and hands it to the other ranks by whatever
 *          channel the launcher offers (MPI_Bcast, a torch.distributed store, a file);
 *   gpv_comm_create is collective: it returns when all `world` ranks have called it with the same id;
 *   gpv_plan_set_comm(plan, NULL) detaches; detach (or destroy) every plan before gpv_comm_destroy.  Flags with a communicator: GPV_WANT_U | GPV_WANT_LOGLIK_Z |
 *   GPV_WANT_NUMERATOR (the posterior pass does not shard: GPV_ERR_STATE). */
typedef struct gpv_comm gpv_comm;
int gpv_rccl_version(void);            /* ncclGetVersion() of the RCCL bound at run time (>= 2000), 0 when none could be bound */
int gpv_comm_unique_id(void *id128);
int gpv_comm_create(gpv_comm **comm, int device, int rank, int world, const void *id128);
int gpv_comm_destroy(gpv_comm *comm);
int gpv_plan_set_comm(gpv_plan *plan, gpv_comm *comm);

/* -------------------------------------------------------------------------
 * Host-side setup helper (no GPU needed, parameter independent, once per data set).
 * Not part of the reference's FFI: the reference runs this as interpreted R
 * (R/whichCondOnLatent.R:2-26, O(n m^3)); exported so that SGV plans can be built at n = 1e6.
 * NNarray: n x ncolNN column-major, 1-based, 0/NA_INTEGER = missing (NOT reversed);
 * Cond out: n x ncolNN column-major R logical (1/0/NA_INTEGER). */
int gpv_whichCondOnLatent(const int *NNarray, int64_t n, int ncolNN, int64_t firstind_pred, int *Cond);

/* Exact max-min-distance ordering, quasi-linear (host): R/ordering_functions.R:147-150 -> src/MaxMin.cpp:661-738.
 * locs n x dim column-major; ord out: n one-based indices (first = closest to the centroid). */
int gpv_order_maxmin_exact(const double *locs, int64_t n, int dim, int *ord);

/* Zero-fill incomplete Cholesky IC(0) of a sparse SPD matrix, in place on its lower triangle in compressed-row form
 * (equivalently the upper triangle in compressed-column form): replaces src/ic0.cpp:43-64 (`ic0`), which
 * R/ichol.R:54 calls and U2V uses when the approximation was specified with ic0 = TRUE (R/vecchia_prediction.R:76-77).
 * ptrs: N+1 row starts (0-based); inds: column index of every stored entry, ascending inside a row, the diagonal last;
 * vals: the matrix entries on input, the factor L (A ~ L L^T on the pattern) on output.
 * Returns GPV_ERR_INDEX for a malformed structure; *n_bad (may be NULL) counts non-positive pivots (NaN rows, like the
 * reference's sqrt of a negative number). */
int gpv_ic0(int64_t N, const int *ptrs, const int *inds, double *vals, int64_t *n_bad);

/* Exact ordered nearest neighbours on the GPU (brute force, bit-exact): the definition of R/NN_kdtree.R:73-83
 * (what GpGp::find_ordered_nn computes at R/vecchia_specify.R:159, without its random jitter).  locs: n x dim
 * column-major in the ORDERED layout; NNarray: n x (m+1) column-major, 1-based, 0 = NA; only rows
 * [row_begin, row_end) are written (a row shard of a multi-GPU plan); an empty shard writes nothing and is GPV_OK.
 * Limits: 1 <= dim <= 8, 0 <= m <= gpv_nn_max_m() (every lane keeps its m+1 best in the LDS of one compute unit; the limit
 * covers every row length the library takes, m + 1 <= gpv_max_p()), 0 < n < 2^31, 0 <= row_begin <= row_end <= n.
 * Statuses: GPV_ERR_BAD_ARG for a NULL pointer or anything outside these limits, checked before the device is touched;
 * GPV_ERR_NO_DEVICE; GPV_ERR_HIP for a failing runtime call.  NNarray is written only by a call that returns GPV_OK.
 * Non-finite coordinates: a candidate at a NaN or infinite distance never enters a list.  The row of a point with such a
 * coordinate is all 0, the row of a finite point lists its finite predecessors only (0-padded if fewer than m + 1); rows
 * with at least m + 1 finite predecessors are those of the definition. */
int gpv_nn_max_m(void);                /* 212 */
int gpv_find_ordered_nn(int device, const double *locs, int64_t n, int dim, int m, int64_t row_begin, int64_t row_end,
                        int *NNarray);

/* Nearest observations of QUERY points that are not plan points, on the GPU, bit-exact: for each query the
 * min(m, #eligible) eligible points of locs closest to it, by ascending distance in the arithmetic of gpv_find_ordered_nn
 * (separately rounded products and sums accumulated left to right, compared on the correctly rounded square root), ties
 * towards the lower index.  locs: n x dim, qlocs: nq x dim, NN: nq x m, all column-major; NN is 1-based and 0-padded.
 * eligible: NULL (every point) or n bytes, 0 = the point enters no list (how missing data stay out of conditioning sets).
 * Two routes give the same arrays bit for bit: brute force, and in one to three dimensions from 2048 searchable points on a
 * uniform grid walked in shells (queries outside the bounding box of the points included); GPV_NN_BRUTE=1 in the environment
 * forces the first.  A point with a NaN or infinite coordinate enters no list; a query with one gets a row of zeros.
 * Limits: 1 <= dim <= 8, 1 <= m <= gpv_nn_max_m(), 0 < n < 2^31, 0 <= nq < 2^31 - 64.
 * Statuses: GPV_ERR_BAD_ARG for a NULL pointer (eligible excepted) or anything outside these limits, checked before the
 * device is touched; GPV_ERR_NO_DEVICE; GPV_ERR_HIP.  NN is written only by a call that returns GPV_OK; nq == 0 is GPV_OK. */
int gpv_find_query_nn(int device, const double *locs, int64_t n, int dim, const unsigned char *eligible, const double *qlocs,
                      int64_t nq, int m, int *NN);

/* Local kriging: the predictive distribution of a cond.yz='z' model at new locations (gpv_krige.hip).  Under that model a
 * prediction location ordered last conditions on its m nearest observations J and on nothing else; with the location as the
 * last row of S = C(J u q, J u q) + diag(tau_J, 0) and u = S^-1 e_last,
 *     var[q] = 1 / u_last (of the latent field y; add the nugget of the location for z),
 *     mean[q, c] = -(sum_{j in J} u_j z_{j,c}) / u_last,
 * one independent solve per location, one wavefront each.  Appending the location to the plan as its last row gives
 * loglik([z; z0]) = loglik(z) + log N(z0; mean, var + tau_0): it is the prediction of the model the likelihood scores.
 *   covType, covparms, ncovparms   "matern" (any smoothness in (0, 60]), "esqe", "matern_scaledim" (up to 8 coordinates)
 *   nuggets, n_nuggets             1 value, or Nlocs in the ORDERED layout; finite and >= 0
 *   Z_ord, ldz, ncols              ncols <= gpv_krige_max_cols() = 16 data columns in the ORDERED layout, ldz >= Nlocs apart;
 *                                  NULL (ncols = 1): the plan's data (gpv_plan_set_data)
 *   qlocs, nq, m                   nq x dim column-major prediction locations; m + 1 <= 64 neighbours each
 *   NNq                            NULL: the search of gpv_find_query_nn on the device, over the plan's locations; else nq x m
 *                                  column-major ORDERED ids, 1-based, 0 = none (eligible_ord and scale are then not used)
 *   scale                          NULL, or one positive number per coordinate: the search runs on the coordinates divided by
 *                                  it, the covariance on the true ones (vecchia_specify(scale=) for "matern_scaledim")
 *   eligible_ord                   NULL, or Nlocs bytes in the ORDERED layout: 0 = never a neighbour (missing data)
 *   chunk                          prediction locations per pass, 0: 262144.  The call streams nq in chunks (queries up, search
 *                                  or neighbours up, the pass, results back), so device memory does not grow with nq; a
 *                                  location's bits do not depend on the chunking, a column's not on the other columns
 *   mean, ldm, var, n_failed       nq x ncols column-major (ldm >= nq), nq, and the count of locations whose block was not
 *                                  positive definite ("pivot <= 0 or NaN", e.g. a location on an observation that has no
 *                                  nugget): their mean and var are NaN
 * Needs no evaluation and disturbs none; whatever it allocates lives for the call or is freed with the plan.
 * Arguments and state are validated before the device is touched, and a refused call writes nothing.  GPV_ERR_BAD_ARG: a null
 * pointer (Z_ord, NNq, scale, eligible_ord excepted), n_nuggets not 1 or Nlocs, a nugget < 0 or not finite, ncols outside
 * [1, 16] (or not 1 with Z_ord NULL), ldz < Nlocs, ldm < nq, nq < 0, m < 1, chunk < 0, a scale <= 0, ncovparms not 3 / 4 /
 * dim + 2; GPV_ERR_COVTYPE; GPV_ERR_UNSUPPORTED_NU; GPV_ERR_UNSUPPORTED_M: m + 1 > 64; GPV_ERR_INDEX: an entry of NNq outside
 * [0, Nlocs]; GPV_ERR_STATE: a row shard, a communicator attached, unobserved locations (gpv_plan_set_observed), latent
 * conditioning (not a cond.yz='z' plan), Z_ord NULL and no data set, a plan without coordinates.
 * nq == 0 is GPV_OK. */
int gpv_krige_max_cols(void);          /* 16 */
int gpv_plan_krige(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms,
                   const double *nuggets, int64_t n_nuggets,          /* 1 or Nlocs, ORDERED */
                   const double *Z_ord, int64_t ldz, int ncols,        /* NULL: the plan's data; ncols <= 16 */
                   const double *qlocs, int64_t nq, int m,             /* nq x dim column-major */
                   const int *NNq,                                     /* NULL: search on the device; else nq x m, ORDERED ids */
                   const double *scale, const unsigned char *eligible_ord, int64_t chunk /* 0: default */,
                   double *mean, int64_t ldm, double *var, int64_t *n_failed);

/* Grouped local kriging: joint predictions of groups of locations under a cond.yz='z' model (gpv_krige_groups.hip).  A group G
 * of g locations is ordered last; member i conditions on one shared set J of observations and on the members before it, which
 * is a valid Vecchia model.  With S = C(J u G, J u G) + diag(tau_J, 0_G), J in front, and the J pivots eliminated,
 *     Sigma_G = K_GG - K_GJ (K_JJ + tau_J)^-1 K_JG    the joint predictive covariance of the latent field y on G,
 *     mean[i, c] = K_iJ (K_JJ + tau_J)^-1 z_{J,c},    var[i] = (Sigma_G)_ii,
 *     gmean[k, c] = sum_i w_i mean[i, c],             gvar[k] = w' Sigma_G w     (an areal average, a contrast, ...).
 * J = the min(m, #eligible) eligible observations nearest (gpv_find_query_nn) to the group's anchor, the coordinate-wise mean
 * of its members (summed in member order in double precision, then divided by g; with `scale`, then divided by it), or NNg.
 * A group of one location is the prediction of gpv_plan_krige there.
 *   covType ... ncols, scale, eligible_ord   as gpv_plan_krige
 *   qlocs, nq                      nq x dim column-major, the members of a group contiguous
 *   gptr, ngroups                  group k = rows gptr[k] .. gptr[k + 1] - 1; gptr[0] = 0, gptr[ngroups] = nq, no group empty
 *   weights                        NULL: 1 / g each; else nq finite values of any sign
 *   m, NNg                         m + g <= gpv_krige_groups_max_rows() = 64 for every group; NNg: NULL (searched at the anchors)
 *                                  or ngroups x m column-major ORDERED ids, 1-based, 0 = none
 *   chunk                          groups per pass, 0: 65536.  Device memory does not grow with nq.  A group's bits depend on
 *                                  neither the chunking, nor the other groups of the call, nor the other columns
 *   mean, ldm, var                 per location: nq x ncols column-major (ldm >= nq), nq
 *   gmean, ldg, gvar               per group: ngroups x ncols column-major (ldg >= ngroups), ngroups
 *   cov                            NULL, or sum_k g_k (g_k + 1) / 2 doubles: the lower triangle of group k's Sigma_G, row-major,
 *                                  at the running offset
 *   n_failed                       groups that failed: a J pivot not > 0 (or NaN) or a diagonal entry of Sigma_G not > 0 (a
 *                                  member on an observation that has no nugget).  Everything of a failed group is NaN.
 *                                  Duplicate members are legal: Sigma_G is singular there
 * Statuses as gpv_plan_krige, and GPV_ERR_BAD_ARG: gptr not increasing from 0 to nq (an empty group included), a weight that
 * is not finite, ldg < ngroups; GPV_ERR_UNSUPPORTED_M: m + g > 64 in any group; GPV_ERR_INDEX: an entry of NNg outside
 * [0, Nlocs].  A refused call writes nothing.  ngroups == 0 is GPV_OK. */
int gpv_krige_groups_max_rows(void);   /* 64: m + g */
int gpv_plan_krige_groups(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms,
                          const double *nuggets, int64_t n_nuggets,
                          const double *Z_ord, int64_t ldz, int ncols,
                          const double *qlocs, int64_t nq,            /* nq x dim column-major, members of a group contiguous */
                          const int64_t *gptr, int64_t ngroups,       /* group k = rows gptr[k] .. gptr[k+1]-1 */
                          const double *weights,                      /* NULL: 1/g; else nq values, any sign */
                          int m, const int *NNg,                      /* NULL: search at the anchors; else ngroups x m ORDERED ids */
                          const double *scale, const unsigned char *eligible_ord, int64_t chunk /* groups per pass, 0: default */,
                          double *mean, int64_t ldm, double *var,     /* per location */
                          double *gmean, int64_t ldg, double *gvar,   /* per group */
                          double *cov,                                /* NULL, or the packed lower triangles */
                          int64_t *n_failed);

/* Conditional simulation of a map under a cond.yz='z' model: the sequential kriging sweep (gpv_csim.hip).  The prediction
 * locations s_0 .. s_{nq-1} are ordered after all observations, in the order they are given (the sweep order).  s_i conditions on
 * N_i, the m nearest points among {the eligible observations} u {s_j : j < i}, in the arithmetic and with the tie rule of
 * gpv_find_ordered_nn: its observations J_i through z (the nugget on the diagonal), its earlier prediction locations P_i
 * through the latent y (no nugget).  With s_i as the last row of S = C(N_i u s_i, N_i u s_i) + diag(tau_J, 0_P, 0) and
 * u = S^-1 e_last,
 *     c_ij = -u_j / u_last,   sd[i] = 1 / sqrt(u_last),   y_i = sum_J c_ij z_j + sum_P c_ip y_p + sd[i] eps_i,
 * that is (I - B) Y = A + D E with B the strictly lower-triangular matrix of the c_ip:
 *     mean[:, c] = (I - B)^-1 A_c      the predictive mean of the joint model (the draw with eps = 0),
 *     dev[:, s]  = (I - B)^-1 D eps_s  a deviation field; the draw (c, s) is mean[:, c] + dev[:, s].
 * With m >= Nlocs + nq - 1 this is the exact GP conditional: mean = K_po (K_oo + tau)^-1 z, and the columns of dev for E = I are
 * the lower Cholesky factor of K_pp - K_po (K_oo + tau)^-1 K_op in sweep order.  A location with P_i empty is gpv_plan_krige there.
 *   covType ... ncols, scale, eligible_ord   as gpv_plan_krige
 *   qlocs, nq, m                   nq x dim column-major, in sweep order; m + 1 <= 64
 *   NNq                            NULL: the ordered search of the library on [observations ; qlocs] (divided by `scale` when
 *                                  given, the ineligible observations taken out); else nq x m column-major ids, 1-based, 0 =
 *                                  none: 1 .. Nlocs an ORDERED observation, Nlocs + 1 + p the sweep row p < own row
 *   E, lde                         NULL: standard normals of the library's generator (gpv_philox.hpp) from (seed, Nlocs + i, draw
 *                                  j), j = col0 .. col0 + nsim - 1, apart from those gpv_plan_simulate uses with the same seed;
 *                                  draw j is always made in the batch [16 floor(j / 16), + 16), so its bits depend on neither
 *                                  col0, nsim nor the other draws.  Else the caller's nq x nsim standard normals (lde >= nq)
 *   mean, ldm; dev, ldd; sd        nq x ncols, nq x nsim (column-major), nq.  sd is the conditional standard deviation GIVEN
 *                                  THE NEIGHBOURS, not the marginal one.  nsim == 0: means only (dev may be NULL)
 *   n_levels, n_launches           levels of the schedule (level(i) = 0 if P_i is empty, else 1 + max level over P_i) and
 *                                  launches per sweep: one per level of more than 256 rows, one per maximal run of narrower ones
 *   n_failed                       locations whose block failed: "a pivot <= 0 or NaN, or u_last <= 0" (a location that
 *                                  coincides with an earlier prediction location, or with an observation that has no nugget).
 *                                  Their sd, mean and dev are NaN, and NaN reaches every location that depends on them (they
 *                                  are not counted)
 * Device memory grows with nq, unlike gpv_plan_krige: about 12 m + 8 (dim + 16 + 2 CP) bytes per location (coefficients and
 * lists, the locations, the observation sums, the columns of a sweep and their staging copy; CP = the padded column count, 16
 * for seeded draws), 0.8 GB for 10^6 locations at m = 30.  A column's bits depend on neither the other columns, the padded
 * column count nor the chunking of the factor pass.
 * Needs no evaluation and disturbs none; its buffers live for the call.  Arguments and state are validated before the device
 * is touched, and a refused call writes nothing.  Statuses as gpv_plan_krige, and GPV_ERR_BAD_ARG: nsim < 0, col0 < 0, ldd < nq
 * or (with E) lde < nq when nsim > 0, dev NULL with nsim > 0; GPV_ERR_INDEX: an entry of NNq outside [0, Nlocs + own row], or
 * Nlocs + nq >= 2^31 - 1; GPV_ERR_UNSUPPORTED_M: m + 1 > 64.  nq == 0 is GPV_OK. */
int gpv_plan_cond_sim(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms,
                      const double *nuggets, int64_t n_nuggets,
                      const double *Z_ord, int64_t ldz, int ncols,          /* as gpv_plan_krige; ncols <= 16 */
                      const double *qlocs, int64_t nq, int m, const int *NNq,
                      const double *scale, const unsigned char *eligible_ord,
                      const double *E, int64_t lde, uint64_t seed, int64_t col0, int64_t nsim,
                      double *mean, int64_t ldm,                            /* nq x ncols */
                      double *dev, int64_t ldd,                             /* nq x nsim: draw (c, s) = mean_c + dev_s */
                      double *sd,                                           /* nq: conditional sd given the neighbours */
                      int64_t *n_levels, int64_t *n_launches, int64_t *n_failed);
/* The level schedule of gpv_plan_cond_sim on the host, from the lists alone (no device): NN nq x m column-major ids as NNq.
 * level[nq]; order[nq]: the rows by ascending level, ascending row inside a level; levptr[*n_levels + 1] (room for nq + 1):
 * where each level starts in order.  GPV_ERR_INDEX for an id outside [0, Nlocs + own row]. */
int gpv_csim_levels_host(const int32_t *NN, int64_t nq, int m, int64_t Nlocs, int32_t *level, int32_t *order, int64_t *levptr,
                         int64_t *n_levels);

/* Summaries of conditional draws of a map, folded on the device (gpv_csim_summary.hip): the operator of gpv_plan_cond_sim is
 * built once, each batch of 16 seeded draws is swept as there and folded while it is in device memory; the draws themselves
 * never reach the host.  Device memory: what gpv_plan_cond_sim keeps, less its staging copy, plus 8 (3 + nthr / 2) + 1 bytes
 * per location, the regions' lists and one batch's region block; nothing grows with ndraws.
 *   covType ... eligible_ord       as gpv_plan_cond_sim, with ONE data column: Z_ord NULL (the plan's data) or Nlocs values in
 *                                  the ORDERED layout; ncols must be 1
 *   seed, col0, ndraws             the draws j = col0 .. col0 + ndraws - 1 of the library's generator, the bits of
 *                                  gpv_plan_cond_sim with E == NULL (draw j is made in the batch [16 floor(j / 16), + 16));
 *                                  ndraws >= 2
 *   offset                         NULL or nq values in sweep order (a trend).  With mean_i and dev_ij of gpv_plan_cond_sim,
 *                                      mu_i = mean_i + offset_i,   y_ij = mu_i + dev_ij
 *                                  (two rounded adds in that order: the host's (mean + offset) + dev has the same bits)
 *   link                           g: 0 identity, 1 exp, 2 logistic (the codes of gpv_plan_draws_summary)
 *   nthr, thr                      0 .. 8 thresholds on the latent scale of y, offset included
 * A location is LIVE when mean_i is not NaN (the failed locations and all that depend on them: the same set in every column).
 * Per location (nq each, sweep order; NaN where the location is not live, but sd, which is that of gpv_plan_cond_sim):
 *   mean = mu;  sd;  with d_ij = g(y_ij) - g(mu_i) and N = ndraws:
 *   mc_mean = g(mu_i) + sum_j d_ij / N,   mc_var = (sum d^2 - (sum d)^2 / N) / (N - 1), clamped at 0,
 *   exceed[t * nq + i] = #{j : y_ij > thr_t} / N.
 * The sums run over the batches in ascending order and inside a batch over one fixed tree of its 16 columns (the columns
 * outside [col0, col0 + ndraws) are exact zeros).
 * Regions in CSR form over sweep rows: region r holds regidx[regptr[r] .. regptr[r + 1]) with the weights regw there (regw NULL:
 * weights 1; any sign, finite).  A location may be in several regions or in none, a region may be empty.  Over the LIVE members:
 *   reg_total[j * nreg + r]              = sum_i w_i g(y_ij)                (j counted from col0)
 *   reg_max, reg_min (same layout)       of y_ij, on the latent scale: g is monotone
 *   reg_area[(j * nthr + t) * nreg + r]  = sum_i w_i [y_ij > thr_t]
 *   reg_weight[r] = sum_i w_i, reg_count[r] = their number                  (once per region)
 * A region without a live member: total 0, areas 0, max = min = NaN, weight 0, count 0.  A region's list is cut from its start
 * into chunks of 128 entries, a chunk is added entry by entry, the chunks meet in ascending order, and there are no
 * floating-point atomics: results are bitwise reproducible, and the region outputs of draw j depend on (seed, j, the region's
 * own list and weights) alone, not on col0, ndraws, nreg, the region's place among the regions or the factor pass's chunks.
 *   n_levels, n_launches, n_failed  as gpv_plan_cond_sim (launches per sweep)
 * Needs no evaluation and disturbs none.  Arguments, then state, are validated before the device is touched, and a refused
 * call writes nothing.  Statuses as gpv_plan_cond_sim, and GPV_ERR_BAD_ARG: ncols != 1, ndraws < 2, col0 < 0 or col0 + ndraws
 * overflows, link outside 0 .. 2, nthr outside 0 .. 8, a required pointer NULL (thr and exceed with nthr > 0; the region
 * arrays with nreg > 0, reg_area with both), nreg < 0, regptr not non-decreasing from 0, a weight that is not finite;
 * GPV_ERR_INDEX: an entry of regidx outside [0, nq).  nq == 0 is GPV_OK (every region is then empty). */
int gpv_plan_cond_sim_summary(gpv_plan *plan, const char *covType, const double *covparms, int ncovparms,
                              const double *nuggets, int64_t n_nuggets,
                              const double *Z_ord, int ncols,               /* NULL or Nlocs values; ncols == 1 */
                              const double *qlocs, int64_t nq, int m, const int *NNq,
                              const double *scale, const unsigned char *eligible_ord,
                              uint64_t seed, int64_t col0, int64_t ndraws,
                              const double *offset, int link, int nthr, const double *thr,
                              int64_t nreg, const int64_t *regptr, const int32_t *regidx, const double *regw,
                              double *mean, double *sd, double *mc_mean, double *mc_var,    /* nq each */
                              double *exceed,                                               /* nthr x nq */
                              double *reg_total, double *reg_max, double *reg_min,          /* nreg x ndraws, column-major */
                              double *reg_area,                                             /* nreg x nthr x ndraws */
                              double *reg_weight, int64_t *reg_count,                       /* nreg */
                              int64_t *n_levels, int64_t *n_launches, int64_t *n_failed);

#ifdef __cplusplus
}
#endif
#endif /* GPVECCHIA_H */
