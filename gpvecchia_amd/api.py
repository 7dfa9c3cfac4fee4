"""Host-side mirror of GPvecchia's R API for the U_NZentries path, on top of the
C ABI of libgpvecchia_hip.so (R is not installed on either box, so this Python
layer plays the part of the R wrappers; INTEGRATION.md shows the R binding).

Same names and argument meaning as the reference:
    vecchia_specify()    R/vecchia_specify.R:29-240
    createU()            R/createU.R:65-201
    vecchia_likelihood() R/vecchia_likelihood.R:14-27
    U_NZentries()        R/RcppExports.R:22-24   (literal C-ABI drop-in)
    U_NZentries_mat()    R/RcppExports.R:26-28
    MaternFun()/EsqeFun  NAMESPACE:3, R/RcppExports.R
All arithmetic of the hot path runs in the HIP library; nothing here falls back
to NumPy for it.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib as L
from . import specify as S
from ._lib import GPV_WANT_DENOM, GPV_WANT_LOGLIK_Z, GPV_WANT_NUMERATOR, GPV_WANT_U, NSUMS, GpvError


WHITEN_MAX_COLS = 16                                  # gpv_whiten_max_cols(): columns per Plan.whiten call
LOO_NSCORES = 6                                       # gpv_loo_nscores(): score sums per column of Plan.loo
BLOCKCV_NSCORES = 8                                   # gpv_blockcv_nscores(): score sums per column of Plan.block_cv
BLOCKCV_MAX_BLOCK = 64                                # gpv_blockcv_max_block(): members of a held-out block
KRIGE_MAX_COLS = 16                                   # gpv_krige_max_cols(): data columns per Plan.krige call
KRIGE_GROUPS_MAX_ROWS = 64                            # gpv_krige_groups_max_rows(): m + the size of a group of Plan.krige_groups


# ---------------------------------------------------------------------------
# device plan
# ---------------------------------------------------------------------------
class Plan:
    """Device-resident image of a vecchia.approx object (gpv_plan)."""

    def __init__(self, locsord, revNNarray, revCond, device=0, row_begin=0, row_end=None):
        locs = np.asfortranarray(locsord, dtype=np.float64)
        self.Nlocs, self.dim = locs.shape
        nn = L.as_r_int_matrix(revNNarray)
        cd = _cond_to_r(revCond)
        self.p = nn.shape[1]
        self.row_begin = int(row_begin)
        self.row_end = int(self.Nlocs if row_end is None else row_end)
        self.rows = self.row_end - self.row_begin
        self._h = C.c_void_p()
        st = L.lib().gpv_plan_create(C.byref(self._h), int(device), self.Nlocs, self.dim, self.p, L.dptr(locs),
                                     L.iptr(nn), L.iptr(cd), self.row_begin, self.row_end)
        L.check(st, "gpv_plan_create")
        self.device = device
        self._nn, self._cd = nn, cd          # kept for build_posterior (the R-layout arrays of this plan)
        self.has_posterior = False

    def build_posterior(self):
        """Structure of the U2V pass (R/vecchia_prediction.R:62-83) for GPV_WANT_DENOM evaluations."""
        self.has_posterior = False                       # the library drops any earlier structure on entry: true only on success
        L.check(L.lib().gpv_plan_build_posterior(self._h, L.iptr(self._nn), L.iptr(self._cd)), "gpv_plan_build_posterior")
        self.has_posterior = True
        nl = C.c_int()
        L.check(L.lib().gpv_plan_posterior_levels(self._h, C.byref(nl)), "gpv_plan_posterior_levels")
        return int(nl.value)

    def ensure_posterior(self):
        """True when the structure of the device posterior pass exists (built now if it did not); False when the library
        refuses it for this plan (GPV_ERR_UNSUPPORTED_M: some conditioning set has more than 64 LATENT entries; the row
        length m + 1 itself may exceed 64): the caller then takes the host route, like the reference's CHOLMOD."""
        if self.has_posterior:
            return True
        if getattr(self, "_post_refused", False):
            return False
        self.has_posterior = False                       # the library drops any earlier structure on entry: true only on success
        st = L.lib().gpv_plan_build_posterior(self._h, L.iptr(self._nn), L.iptr(self._cd))
        if st == 5:
            self._post_refused = True
            return False
        L.check(st, "gpv_plan_build_posterior")
        self.has_posterior = True
        return True

    def build_posterior_fill(self, max_fill=4.0):
        """Structure of the U2V pass on the FILLED pattern (cond.yz='y': the factor fills in, R/vecchia_prediction.R:72-83).
        Returns the fill ratio, or None when the library refuses (fill beyond max_fill x the latent block, or a column of the
        factor beyond 64 rows): the caller then factorises on the host like the reference's CHOLMOD."""
        if getattr(self, "_fill_refused", False):
            return None
        ratio = C.c_double(0.0)
        self.has_posterior = False                       # (as in ensure_posterior: a refused or failed rebuild leaves none)
        st = L.lib().gpv_plan_build_posterior_fill(self._h, L.iptr(self._nn), L.iptr(self._cd), float(max_fill), C.byref(ratio))
        if st == 5:                                       # GPV_ERR_UNSUPPORTED_M: bounded out
            self._fill_refused = True
            self.fill_ratio = float(ratio.value)
            return None
        L.check(st, "gpv_plan_build_posterior_fill")
        self.has_posterior = True
        self.fill_ratio = float(ratio.value)
        return self.fill_ratio

    def set_observed(self, obs_ord):
        """vecchia.approx$obs in ordered layout (True = the location carries an observation); None = all observed.  With
        unobserved locations the posterior pass drops 1/tau and z/tau there (U2V + vecchia_mean for plans with prediction
        locations, R/vecchia_prediction.R:62-126); evaluate with per-location nuggets."""
        if obs_ord is None:
            L.check(L.lib().gpv_plan_set_observed(self._h, None), "gpv_plan_set_observed")
            return
        o = np.ascontiguousarray(np.asarray(obs_ord, dtype=bool), dtype=np.int32)
        if o.size != self.Nlocs:
            raise ValueError("obs must have one entry per ordered location")
        L.check(L.lib().gpv_plan_set_observed(self._h, L.iptr(o)), "gpv_plan_set_observed")

    def posterior_levels(self):
        """Number of levels of the posterior pass's schedule (after build_posterior)."""
        nl = C.c_int()
        L.check(L.lib().gpv_plan_posterior_levels(self._h, C.byref(nl)), "gpv_plan_posterior_levels")
        return int(nl.value)

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                L.lib().gpv_plan_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def set_data(self, z_ord):
        z = np.ascontiguousarray(z_ord, dtype=np.float64)
        if z.shape[0] != self.Nlocs:
            raise ValueError("z_ord must have one entry per ordered location")
        self._user_z = None                              # whatever set_user_data remembered is no longer on the device
        L.check(L.lib().gpv_plan_set_data(self._h, L.dptr(z)), "gpv_plan_set_data")

    def set_user_data(self, z, ord_z):
        """set_data(z[ord_z - 1]) unless exactly this z is the data already on the device: an optimiser evaluates the
        likelihood of ONE data vector hundreds of times (R/vecchia_wrappers.R:72-93), and reordering and uploading 8 MB
        per call costs more than the evaluation itself at n = 1e6.  The comparison is by content, against a private copy."""
        prev = getattr(self, "_user_z", None)
        if prev is not None and prev.shape == z.shape and np.array_equal(prev, z):
            return False
        self.set_data(z[ord_z - 1])
        self._user_z = np.array(z, dtype=np.float64, copy=True)
        return True

    def invalidate_data(self):
        """Called by code that changes the plan's data behind set_data (the Vecchia-Laplace device loop)."""
        self._user_z = None

    def eval(self, covmodel, covparms, nuggets, flags, stream=None, d_sums_out=None):
        cp = np.ascontiguousarray(covparms, dtype=np.float64)
        ng = np.ascontiguousarray(np.atleast_1d(nuggets), dtype=np.float64)
        st = L.lib().gpv_plan_eval(self._h, covmodel.encode() if isinstance(covmodel, str) else bytes(covmodel),
                                   cp.ctypes.data, int(cp.size), ng.ctypes.data, int(ng.size), int(flags), stream or 0,
                                   d_sums_out or 0)
        if st:
            L.check(st, "gpv_plan_eval")

    def sums(self):
        s = np.zeros(NSUMS)
        L.check(L.lib().gpv_plan_get_sums(self._h, L.dptr(s)), "gpv_plan_get_sums")
        return s

    def Lentries(self):
        out = np.zeros((self.rows, self.p), dtype=np.float64, order="F")
        L.check(L.lib().gpv_plan_get_Lentries(self._h, L.dptr(out)), "gpv_plan_get_Lentries")
        return out

    def Zentries(self):
        out = np.zeros(2 * self.rows, dtype=np.float64)
        L.check(L.lib().gpv_plan_get_Zentries(self._h, L.dptr(out)), "gpv_plan_get_Zentries")
        return out

    def Lentries_device(self):
        ptr, ld = C.c_void_p(), C.c_int64()
        L.check(L.lib().gpv_plan_Lentries_device(self._h, C.byref(ptr), C.byref(ld)), "gpv_plan_Lentries_device")
        return ptr.value, int(ld.value)

    def posterior_mean(self):
        """mu.ord of R/vecchia_prediction.R:118-126 after an eval with GPV_WANT_MEAN."""
        out = np.zeros(self.Nlocs)
        L.check(L.lib().gpv_plan_get_posterior_mean(self._h, L.dptr(out)), "gpv_plan_get_posterior_mean")
        return out

    def factor_stamp(self):
        """0 while the plan holds no posterior factor, else a number that changes with every evaluation that writes one."""
        st = C.c_int64(0)
        L.check(L.lib().gpv_plan_factor_stamp(self._h, C.byref(st)), "gpv_plan_factor_stamp")
        return int(st.value)

    def loglik_grad(self, covmodel, covparms, nugget, row_terms=False, smoothness_grad=False):
        """Value and analytic gradient of the cond.yz='z' log-likelihood of the plan's data (gpv_plan_loglik_grad): returns
        (loglik, grad, n_failed) and, with row_terms, a fourth array (Nlocs, len(covparms) + 2) of {l_k, its derivatives} per
        ordered row.  grad = d/d covparms, then d/d nugget; the smoothness entry of 'matern' is NaN (not differentiated).
        smoothness_grad=True (gpv_plan_loglik_grad_nu) accepts 'matern' at any smoothness and differentiates it wherever the
        covariance is differentiable in it, i.e. everywhere but at exactly 0.5, 1.5 and 2.5, where the entry stays NaN.
        The plan's last evaluation (sums, Lentries, factor stamp) is left as it was."""
        cp = np.ascontiguousarray(covparms, dtype=np.float64)
        ll, nf = C.c_double(0.0), C.c_int64(0)
        grad = np.zeros(cp.size + 1)
        rt = np.zeros((self.Nlocs, cp.size + 2)) if row_terms else None
        name = "gpv_plan_loglik_grad_nu" if smoothness_grad else "gpv_plan_loglik_grad"
        st = getattr(L.lib(), name)(self._h, covmodel.encode() if isinstance(covmodel, str) else bytes(covmodel),
                                    L.dptr(cp), int(cp.size), float(nugget), C.byref(ll), L.dptr(grad), C.byref(nf),
                                    L.dptr(rt) if row_terms else None)
        L.check(st, name)
        out = (float(ll.value), grad, int(nf.value))
        return out + (rt,) if row_terms else out

    def loglik_grad_sgv(self, covmodel, covparms, nugget, col_terms=False):
        """Value and analytic gradient of the log-likelihood of a plan with latent conditioning (cond.yz='SGV';
        gpv_plan_loglik_grad_sgv): returns (loglik, grad, n_failed) and, with col_terms, a fourth array (Nlocs, len(covparms) + 1)
        whose rows (ordered numbering) sum to grad.  grad = d/d covparms, then d/d nugget; the smoothness entry of 'matern' is NaN.
        Needs the posterior structure (build_posterior / ensure_posterior).  Unlike loglik_grad this call EVALUATES the plan:
        afterwards sums(), posterior_mean() and factor_stamp() are those of eval(..., GPV_WANT_MEAN) at these parameters."""
        cp = np.ascontiguousarray(covparms, dtype=np.float64)
        ll, nf = C.c_double(0.0), C.c_int64(0)
        grad = np.zeros(cp.size + 1)
        ct = np.zeros((self.Nlocs, cp.size + 1)) if col_terms else None
        st = L.lib().gpv_plan_loglik_grad_sgv(self._h, covmodel.encode() if isinstance(covmodel, str) else bytes(covmodel),
                                              L.dptr(cp), int(cp.size), float(nugget), C.byref(ll), L.dptr(grad), C.byref(nf),
                                              L.dptr(ct) if col_terms else None)
        L.check(st, "gpv_plan_loglik_grad_sgv")
        out = (float(ll.value), grad, int(nf.value))
        return out + (ct,) if col_terms else out

    def loglik_fisher(self, covmodel, covparms, nugget, row_terms=False, smoothness_grad=False):
        """Value, analytic gradient and expected Fisher information of the cond.yz='z' log-likelihood of the plan's data
        (gpv_plan_loglik_fisher): returns (loglik, grad, info, n_failed) and, with row_terms, a fifth array
        (Nlocs, len(covparms) + 2 + T), T = (len(covparms) + 1)(len(covparms) + 2) / 2, of {l_k, its derivatives, the upper triangle
        of the row's information, row-major} per ordered row.  info is (len(covparms) + 1) square, symmetric, in the parameter
        order of grad; for 'matern' the entries that involve the smoothness are NaN, unless smoothness_grad=True
        (gpv_plan_loglik_fisher_nu) and the smoothness is none of 0.5, 1.5, 2.5: then the information is the full matrix.
        The plan's last evaluation is left as it was."""
        cp = np.ascontiguousarray(covparms, dtype=np.float64)
        ll, nf = C.c_double(0.0), C.c_int64(0)
        npar = cp.size + 1
        grad, info = np.zeros(npar), np.zeros((npar, npar))
        rt = np.zeros((self.Nlocs, npar + 1 + npar * (npar + 1) // 2)) if row_terms else None
        name = "gpv_plan_loglik_fisher_nu" if smoothness_grad else "gpv_plan_loglik_fisher"
        st = getattr(L.lib(), name)(self._h, covmodel.encode() if isinstance(covmodel, str) else bytes(covmodel),
                                    L.dptr(cp), int(cp.size), float(nugget), C.byref(ll), L.dptr(grad), L.dptr(info),
                                    C.byref(nf), L.dptr(rt) if row_terms else None)
        L.check(st, name)
        out = (float(ll.value), grad, info, int(nf.value))
        return out + (rt,) if row_terms else out

    def set_replicates(self, Z_ord):
        """Uploads R replicates of the data, the columns of Z_ord (Nlocs, R) in the plan's ORDERED row numbering, and keeps
        them on the device for loglik_replicates (gpv_plan_set_replicates).  None, or an array without columns, releases them.
        The column of set_data is a separate thing and stays what it was."""
        self._user_Z = None                              # whatever set_user_replicates remembered is no longer on the device
        if Z_ord is None or np.asarray(Z_ord).size == 0:
            L.check(L.lib().gpv_plan_set_replicates(self._h, None, 0, 0), "gpv_plan_set_replicates")
            return
        Z = np.asarray(Z_ord, dtype=np.float64)
        if Z.ndim == 1:
            Z = Z[:, None]
        if Z.ndim != 2 or Z.shape[0] != self.Nlocs:
            raise ValueError("Z_ord must have one row per ordered location of the plan")
        Z = np.asfortranarray(Z)
        L.check(L.lib().gpv_plan_set_replicates(self._h, L.dptr(Z), self.Nlocs, int(Z.shape[1])), "gpv_plan_set_replicates")

    def set_user_replicates(self, Z, ord_z):
        """set_replicates(Z[ord_z - 1]) unless exactly this Z is what the device holds already (compared by content against a
        private copy, like set_user_data): an optimiser evaluates one set of replicates many times."""
        prev = getattr(self, "_user_Z", None)
        if prev is not None and prev.shape == Z.shape and np.array_equal(prev, Z):
            return False
        self.set_replicates(Z[ord_z - 1])
        self._user_Z = np.array(Z, dtype=np.float64, copy=True)
        return True

    def replicates(self):
        """The number of replicates on the device (0: none)."""
        R = C.c_int(0)
        L.check(L.lib().gpv_plan_replicates(self._h, C.byref(R)), "gpv_plan_replicates")
        return int(R.value)

    def loglik_replicates(self, covmodel, covparms, nugget, fisher=True, row_terms=False, smoothness_grad=False):
        """Value, gradient and expected information of the cond.yz='z' log-likelihood SUMMED over the replicates of
        set_replicates, from one pass over the conditioning sets (gpv_plan_loglik_rep): returns (loglik, grad, info, n_failed)
        -- info None with fisher=False -- and, with row_terms, a fifth array in the layout of loglik_fisher's whose row k holds
        the sums over the replicates of row k's terms.  info is R times the information of one column.  smoothness_grad as
        for loglik_fisher.  The plan's last evaluation and its data column are left as they were."""
        cp = np.ascontiguousarray(covparms, dtype=np.float64)
        ll, nf = C.c_double(0.0), C.c_int64(0)
        npar = cp.size + 1
        grad = np.zeros(npar)
        info = np.zeros((npar, npar)) if fisher else None
        rt = np.zeros((self.Nlocs, npar + 1 + npar * (npar + 1) // 2)) if row_terms else None
        name = "gpv_plan_loglik_rep_nu" if smoothness_grad else "gpv_plan_loglik_rep"
        st = getattr(L.lib(), name)(self._h, covmodel.encode() if isinstance(covmodel, str) else bytes(covmodel),
                                    L.dptr(cp), int(cp.size), float(nugget), C.byref(ll), L.dptr(grad),
                                    L.dptr(info) if fisher else None, C.byref(nf), L.dptr(rt) if row_terms else None)
        L.check(st, name)
        out = (float(ll.value), grad, info, int(nf.value))
        return out + (rt,) if row_terms else out

    def whiten(self, B_ord, want_E=False):
        """The whitening operator of the plan's latest evaluation (which must have asked for GPV_WANT_U) applied to the columns
        of B_ord, (Nlocs, ncols) or (Nlocs,) in the plan's ORDERED row numbering, ncols <= 16 (gpv_plan_whiten): returns
        (G, logdet, n_failed) and, with want_E, a fourth array E (Nlocs, ncols).  E[k] is the standardised conditional residual
        of row k given its neighbours under C + tau I, G = E'E (exactly symmetric), logdet = sum_k log(tau_k + 1/d_k^2): for
        the plan's data, G is sums[3] and logdet is sums[2].  With n_failed > 0 (blocks that were not positive definite) G and
        logdet are NaN.  The plan's last evaluation (sums, Lentries, factor stamp) is left as it was."""
        B = np.asarray(B_ord, dtype=np.float64)
        if B.ndim == 1:
            B = B[:, None]
        if B.ndim != 2 or B.shape[0] != self.Nlocs:
            raise ValueError("B_ord must have one row per ordered location of the plan")
        ncols = int(B.shape[1])
        if ncols < 1 or ncols > WHITEN_MAX_COLS:
            raise ValueError(f"whiten takes 1 to {WHITEN_MAX_COLS} columns per call")
        B = np.asfortranarray(B)
        G = np.zeros((ncols, ncols))
        E = np.zeros((self.Nlocs, ncols), order="F") if want_E else None
        ld, nf = C.c_double(0.0), C.c_int64(0)
        st = L.lib().gpv_plan_whiten(self._h, L.dptr(B), self.Nlocs, ncols, L.dptr(E) if want_E else None, self.Nlocs,
                                     L.dptr(G), C.byref(ld), C.byref(nf))
        L.check(st, "gpv_plan_whiten")
        out = (G, float(ld.value), int(nf.value))
        return out + (E,) if want_E else out

    def unwhiten(self, E_ord):
        """The inverse of whiten: the colouring operator of the plan's latest evaluation (GPV_WANT_U) applied to the columns of
        E_ord, (Nlocs, ncols) or (Nlocs,) in the plan's ORDERED row numbering, ncols <= 16 (gpv_plan_unwhiten).  Returns
        (B_ord, n_failed), B_ord (Nlocs, ncols): whiten(B_ord) gives E_ord back, and standard normal columns become draws from
        the Vecchia approximation of N(0, C + tau I).  With n_failed > 0 (blocks that were not positive definite) B_ord is all
        NaN.  The plan's last evaluation (sums, Lentries, factor stamp) is left as it was."""
        E = np.asarray(E_ord, dtype=np.float64)
        if E.ndim == 1:
            E = E[:, None]
        if E.ndim != 2 or E.shape[0] != self.Nlocs:
            raise ValueError("E_ord must have one row per ordered location of the plan")
        ncols = int(E.shape[1])
        if ncols < 1 or ncols > WHITEN_MAX_COLS:
            raise ValueError(f"unwhiten takes 1 to {WHITEN_MAX_COLS} columns per call")
        E = np.asfortranarray(E)
        B = np.zeros((self.Nlocs, ncols), order="F")
        nf = C.c_int64(0)
        L.check(L.lib().gpv_plan_unwhiten(self._h, L.dptr(E), self.Nlocs, ncols, L.dptr(B), self.Nlocs, C.byref(nf)),
                "gpv_plan_unwhiten")
        return B, int(nf.value)

    def _loo_columns(self, A_ord, what):
        A = np.asarray(A_ord, dtype=np.float64)
        if A.ndim == 1:
            A = A[:, None]
        if A.ndim != 2 or A.shape[0] != self.Nlocs:
            raise ValueError(f"{what} must have one row per ordered location of the plan")
        if A.shape[1] < 1 or A.shape[1] > WHITEN_MAX_COLS:
            raise ValueError(f"{what}: 1 to {WHITEN_MAX_COLS} columns per call")
        return np.asfortranarray(A), int(A.shape[1])

    def whiten_t(self, E_ord):
        """The TRANSPOSE of the whitening operator of the plan's latest evaluation (GPV_WANT_U) applied to the columns of E_ord,
        (Nlocs, ncols) or (Nlocs,) in the ORDERED row numbering, ncols <= 16 (gpv_plan_whiten_t).  Returns (B_ord, n_failed):
        <whiten(b), e> = <b, whiten_t(e)>.  All NaN with n_failed > 0.  The plan's last evaluation is left as it was."""
        E, ncols = self._loo_columns(E_ord, "E_ord")
        B = np.zeros((self.Nlocs, ncols), order="F")
        nf = C.c_int64(0)
        L.check(L.lib().gpv_plan_whiten_t(self._h, L.dptr(E), self.Nlocs, ncols, L.dptr(B), self.Nlocs, C.byref(nf)),
                "gpv_plan_whiten_t")
        return B, int(nf.value)

    def precision(self, B_ord, want_diag=True):
        """Q B for the precision matrix Q = T'T of the data vector under the plan's latest evaluation (GPV_WANT_U), T the
        whitening operator; B_ord (Nlocs, ncols) or (Nlocs,) in the ORDERED row numbering, ncols <= 16 (gpv_plan_precision).
        Returns (R_ord, qdiag, n_failed): qdiag = diag Q (Nlocs), None without want_diag.  All NaN with n_failed > 0."""
        B, ncols = self._loo_columns(B_ord, "B_ord")
        R = np.zeros((self.Nlocs, ncols), order="F")
        q = np.zeros(self.Nlocs) if want_diag else None
        nf = C.c_int64(0)
        L.check(L.lib().gpv_plan_precision(self._h, L.dptr(B), self.Nlocs, ncols, L.dptr(R), self.Nlocs,
                                           L.dptr(q) if want_diag else None, C.byref(nf)), "gpv_plan_precision")
        return R, q, int(nf.value)

    def loo(self, Z_ord, want_mean=True, want_var=True):
        """Leave-one-out cross-validation of the columns of Z_ord, (Nlocs, ncols) or (Nlocs,) in the ORDERED row numbering,
        ncols <= 16, under the plan's latest evaluation (GPV_WANT_U), without refitting (gpv_plan_loo): with Q the precision of
        the data vector, mean_i = z_i - (Q z)_i / Q_ii and var_i = 1 / Q_ii.  Returns (mean (Nlocs, ncols) or None, var (Nlocs,)
        or None, scores (ncols, 6), n_failed); scores per column: sum (z - mean)^2, sum |z - mean|, sum of squared standardised
        residuals, sum log var, sum CRPS, count of |standardised residual| <= 1.96.  All NaN with n_failed > 0."""
        Z, ncols = self._loo_columns(Z_ord, "Z_ord")
        mean = np.zeros((self.Nlocs, ncols), order="F") if want_mean else None
        var = np.zeros(self.Nlocs) if want_var else None
        scores = np.zeros((ncols, LOO_NSCORES))
        nf = C.c_int64(0)
        L.check(L.lib().gpv_plan_loo(self._h, L.dptr(Z), self.Nlocs, ncols, L.dptr(mean) if want_mean else None, self.Nlocs,
                                     L.dptr(var) if want_var else None, L.dptr(scores), C.byref(nf)), "gpv_plan_loo")
        return mean, var, scores, int(nf.value)

    def loo_index(self):
        """(entries, longest column, empty columns) of the transposed index whiten_t / precision / loo gather through, built at
        first use (gpv_plan_loo_index): for every location the stored entries that name it as a neighbour."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L.check(L.lib().gpv_plan_loo_index(self._h, C.byref(a), C.byref(b), C.byref(c)), "gpv_plan_loo_index")
        return int(a.value), int(b.value), int(c.value)

    def set_blocks(self, block_of_ord):
        """The held-out blocks of Plan.block_cv (gpv_plan_set_blocks): block_of_ord[i], i the ORDERED row, is -1 (never held
        out: stays in the conditioning data) or a block id in [0, Nlocs); a block has at most 64 members of any shape.  Builds
        the block index on the host (structure only: no evaluation needed, kept until the labels are replaced).  Returns
        (n_blocks, n_heldout, max_size, n_set_refs).  A refused call leaves the plan's current blocks as they were."""
        lab = np.asarray(block_of_ord)
        if lab.ndim != 1 or lab.shape[0] != self.Nlocs or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError("block_of_ord must be one integer label per ordered location of the plan")
        if lab.size and (lab.min() < np.iinfo(np.int32).min or lab.max() > np.iinfo(np.int32).max):
            raise ValueError("block_of_ord: labels are -1 or a block id in [0, Nlocs)")
        lab = np.ascontiguousarray(lab, dtype=np.int32)
        nb, nh, nr, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
        L.check(L.lib().gpv_plan_set_blocks(self._h, lab.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nb), C.byref(nh), C.byref(ms),
                                            C.byref(nr)), "gpv_plan_set_blocks")
        return int(nb.value), int(nh.value), int(ms.value), int(nr.value)

    def block_cv(self, Z_ord, want_mean=True, want_var=True):
        """Leave-block-out cross-validation of the columns of Z_ord, (Nlocs, ncols) or (Nlocs,) in the ORDERED row numbering,
        ncols <= 16, for the blocks of Plan.set_blocks under the plan's latest evaluation (GPV_WANT_U), without refitting
        (gpv_plan_block_cv): with Q the precision of the data vector, z_B | z_-B ~ N(z_B - Q_BB^-1 (Q z)_B, Q_BB^-1) for every
        block B.  Returns (mean (Nlocs, ncols) or None, var (Nlocs,) or None, scores (ncols, 8), n_failed, n_bad_blocks); mean
        and var are NaN where the location is not held out.  scores per column over the held-out locations: [0] .. [5] as
        Plan.loo, [6] the sum over the blocks of r_B' Q_BB^-1 r_B, [7] minus the sum of log det Q_BB.  All NaN with
        n_failed > 0."""
        Z, ncols = self._loo_columns(Z_ord, "Z_ord")
        mean = np.zeros((self.Nlocs, ncols), order="F") if want_mean else None
        var = np.zeros(self.Nlocs) if want_var else None
        scores = np.zeros((ncols, BLOCKCV_NSCORES))
        nf, nbad = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().gpv_plan_block_cv(self._h, L.dptr(Z), self.Nlocs, ncols, L.dptr(mean) if want_mean else None, self.Nlocs,
                                          L.dptr(var) if want_var else None, L.dptr(scores), C.byref(nf), C.byref(nbad)),
                "gpv_plan_block_cv")
        return mean, var, scores, int(nf.value), int(nbad.value)

    def krige(self, covmodel, covparms, nuggets_ord, qlocs, m, Z_ord=None, NNq=None, scale=None, eligible_ord=None, chunk=0):
        """Local kriging at the prediction locations qlocs (nq, dim) under the cond.yz='z' model of this plan (gpv_plan_krige):
        every location conditions on its m nearest observations (m + 1 <= 64), one independent solve each; needs no evaluation
        and disturbs none.  nuggets_ord: one value or Nlocs in the ORDERED layout; Z_ord: None (the plan's data) or
        (Nlocs[, ncols <= 16]) in the ORDERED layout; NNq: None (searched on the device, on the coordinates divided by `scale`
        when given, skipping the locations whose eligible_ord is False) or (nq, m) ORDERED ids, 1-based, 0 = none; chunk:
        locations per pass (0: the default), which changes no bit of the result.  Returns (mean (nq, ncols), var (nq,), n_failed):
        the predictive mean of every column and the variance of the latent field; NaN where the location's block was not
        positive definite (counted in n_failed)."""
        q = np.asfortranarray(np.asarray(qlocs, dtype=np.float64).reshape(-1, self.dim))
        nq = q.shape[0]
        cp = np.ascontiguousarray(covparms, dtype=np.float64).reshape(-1)
        nug = np.ascontiguousarray(np.atleast_1d(np.asarray(nuggets_ord, dtype=np.float64)))
        Z, ncols = None, 1
        if Z_ord is not None:
            Z = np.asarray(Z_ord, dtype=np.float64)
            Z = np.asfortranarray(Z[:, None] if Z.ndim == 1 else Z)
            if Z.ndim != 2 or Z.shape[0] != self.Nlocs:
                raise ValueError("Z_ord must have one row per ordered location of the plan")
            ncols = Z.shape[1]
        nn = None
        if NNq is not None:
            nn = np.asfortranarray(NNq, dtype=np.int32)
            if nn.shape != (nq, int(m)):
                raise ValueError("NNq must be (nq, m)")
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
        if sc is not None and sc.size != self.dim:
            raise ValueError("scale must hold one number per coordinate")
        el = None
        if eligible_ord is not None:
            el = np.ascontiguousarray(np.asarray(eligible_ord).astype(bool).reshape(-1), dtype=np.uint8)
            if el.shape[0] != self.Nlocs:
                raise ValueError("eligible_ord must hold one flag per ordered location of the plan")
        mean = np.zeros((nq, ncols), order="F")
        var = np.zeros(nq)
        nf = C.c_int64(0)
        u8 = C.POINTER(C.c_uint8)
        L.check(L.lib().gpv_plan_krige(self._h, str(covmodel).encode(), L.dptr(cp), cp.size, L.dptr(nug), nug.size,
                                       None if Z is None else L.dptr(Z), self.Nlocs, ncols, L.dptr(q), nq, int(m),
                                       None if nn is None else L.iptr(nn), None if sc is None else L.dptr(sc),
                                       None if el is None else el.ctypes.data_as(u8), int(chunk), L.dptr(mean), max(nq, 1),
                                       L.dptr(var), C.byref(nf)), "gpv_plan_krige")
        return mean, var, int(nf.value)

    def cond_sim(self, covmodel, covparms, nuggets_ord, qlocs, m, Z_ord=None, NNq=None, scale=None, eligible_ord=None, E=None,
                 seed=0, col0=0, nsim=0, chunk=0):
        """Conditional simulation over the prediction locations qlocs (nq, dim), taken in the order given (the sweep order), under
        the cond.yz='z' model of this plan (gpv_plan_cond_sim): location i conditions on its m nearest points among the
        observations and the locations before it (m + 1 <= 64); needs no evaluation and disturbs none.  nuggets_ord, Z_ord,
        scale, eligible_ord: as Plan.krige; NNq: None (the library's ordered search) or (nq, m) ids, 1-based, 0 = none:
        1 .. Nlocs an ORDERED observation, Nlocs + 1 + p the sweep row p (before the own row).  E: None (nsim draws col0 ..
        col0 + nsim - 1 of the library's generator under `seed`) or the caller's (nq, nsim) standard normals.  chunk: rows per
        launch of the factor pass (0: the default), which changes no bit.  Returns dict(mean (nq, ncols), dev (nq, nsim): the
        draw (c, s) is mean[:, c] + dev[:, s]; sd (nq,): the conditional standard deviation given the neighbours; n_levels,
        n_launches, n_failed); NaN at a location whose block was not positive definite (counted) and at those that depend on
        it."""
        q = np.asfortranarray(np.asarray(qlocs, dtype=np.float64).reshape(-1, self.dim))
        nq = q.shape[0]
        cp = np.ascontiguousarray(covparms, dtype=np.float64).reshape(-1)
        nug = np.ascontiguousarray(np.atleast_1d(np.asarray(nuggets_ord, dtype=np.float64)))
        Z, ncols = None, 1
        if Z_ord is not None:
            Z = np.asarray(Z_ord, dtype=np.float64)
            Z = np.asfortranarray(Z[:, None] if Z.ndim == 1 else Z)
            if Z.ndim != 2 or Z.shape[0] != self.Nlocs:
                raise ValueError("Z_ord must have one row per ordered location of the plan")
            ncols = Z.shape[1]
        nn = None
        if NNq is not None:
            nn = np.asfortranarray(NNq, dtype=np.int32)
            if nn.shape != (nq, int(m)):
                raise ValueError("NNq must be (nq, m)")
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
        if sc is not None and sc.size != self.dim:
            raise ValueError("scale must hold one number per coordinate")
        el = None
        if eligible_ord is not None:
            el = np.ascontiguousarray(np.asarray(eligible_ord).astype(bool).reshape(-1), dtype=np.uint8)
            if el.shape[0] != self.Nlocs:
                raise ValueError("eligible_ord must hold one flag per ordered location of the plan")
        Ef = None
        if E is not None:
            Ef = np.asfortranarray(np.asarray(E, dtype=np.float64).reshape(nq, -1))
            nsim = Ef.shape[1]
        nsim = int(nsim)
        mean = np.zeros((nq, ncols), order="F")
        dev = np.zeros((nq, max(nsim, 0)), order="F")
        sd = np.zeros(nq)
        nlev, nlaunch, nf = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        u8 = C.POINTER(C.c_uint8)
        lib = L.lib()
        L.check(lib.gpv_plan_debug_csim_chunk(self._h, int(chunk)), "gpv_plan_debug_csim_chunk")
        try:
            L.check(lib.gpv_plan_cond_sim(self._h, str(covmodel).encode(), L.dptr(cp), cp.size, L.dptr(nug), nug.size,
                                          None if Z is None else L.dptr(Z), self.Nlocs, ncols, L.dptr(q), nq, int(m),
                                          None if nn is None else L.iptr(nn), None if sc is None else L.dptr(sc),
                                          None if el is None else el.ctypes.data_as(u8),
                                          None if Ef is None else L.dptr(Ef), max(nq, 1), int(seed), int(col0), nsim,
                                          L.dptr(mean), max(nq, 1), L.dptr(dev), max(nq, 1), L.dptr(sd),
                                          C.byref(nlev), C.byref(nlaunch), C.byref(nf)), "gpv_plan_cond_sim")
        finally:
            lib.gpv_plan_debug_csim_chunk(self._h, 0)
        return dict(mean=mean, dev=dev, sd=sd, n_levels=int(nlev.value), n_launches=int(nlaunch.value), n_failed=int(nf.value))

    def cond_sim_summary(self, covmodel, covparms, nuggets_ord, qlocs, m, ndraws, seed=0, col0=0, Z_ord=None, NNq=None, scale=None,
                         eligible_ord=None, offset=None, link=0, thresholds=None, regions=None, chunk=0):
        """Summaries of the draws col0 .. col0 + ndraws - 1 of Plan.cond_sim(seed=, nsim=) over the prediction locations qlocs
        (nq, dim) in sweep order, folded on the device (gpv_plan_cond_sim_summary): the draws never reach the host.  covmodel ..
        eligible_ord, chunk: as Plan.cond_sim, with ONE data column (Z_ord None: the plan's data).  offset: None or nq values
        added to the mean; link: 0 identity, 1 exp, 2 logistic; thresholds: up to 8, on the latent scale.  regions: None or
        (regptr (nreg + 1,), regidx, regw or None), CSR over sweep rows.  The latent draw is y = (mean + offset) + dev.
        Returns dict(mean, sd, mc_mean, mc_var (nq,), exceed (nthr, nq): NaN where the mean is NaN (sd: as Plan.cond_sim);
        reg_total, reg_max, reg_min (nreg, ndraws): sum of w g(y), max and min of the latent y over the live members; reg_area
        (nthr, nreg, ndraws): sum of w [y > thr]; reg_weight, reg_count (nreg,); n_levels, n_launches, n_failed)."""
        q = np.asfortranarray(np.asarray(qlocs, dtype=np.float64).reshape(-1, self.dim))
        nq = q.shape[0]
        cp = np.ascontiguousarray(covparms, dtype=np.float64).reshape(-1)
        nug = np.ascontiguousarray(np.atleast_1d(np.asarray(nuggets_ord, dtype=np.float64)))
        Z = None
        if Z_ord is not None:
            Z = np.ascontiguousarray(Z_ord, dtype=np.float64)
            if Z.ndim == 2 and Z.shape[1] == 1:
                Z = np.ascontiguousarray(Z[:, 0])
            if Z.ndim != 1 or Z.shape[0] != self.Nlocs:
                raise ValueError("Z_ord must be one column with one value per ordered location of the plan")
        nn = None
        if NNq is not None:
            nn = np.asfortranarray(NNq, dtype=np.int32)
            if nn.shape != (nq, int(m)):
                raise ValueError("NNq must be (nq, m)")
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
        if sc is not None and sc.size != self.dim:
            raise ValueError("scale must hold one number per coordinate")
        el = None
        if eligible_ord is not None:
            el = np.ascontiguousarray(np.asarray(eligible_ord).astype(bool).reshape(-1), dtype=np.uint8)
            if el.shape[0] != self.Nlocs:
                raise ValueError("eligible_ord must hold one flag per ordered location of the plan")
        off = None
        if offset is not None:
            off = np.ascontiguousarray(offset, dtype=np.float64).reshape(-1)
            if off.size != nq:
                raise ValueError("offset must hold one value per prediction location")
        thr = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
        nthr, ndraws = thr.size, int(ndraws)
        nreg, rp, ri, rw = 0, None, None, None
        if regions is not None:
            rp = np.ascontiguousarray(regions[0], dtype=np.int64).reshape(-1)
            ri = np.ascontiguousarray(regions[1], dtype=np.int32).reshape(-1)
            rw = None if len(regions) < 3 or regions[2] is None else np.ascontiguousarray(regions[2], dtype=np.float64).reshape(-1)
            nreg = rp.size - 1
            if nreg < 0 or ri.size != rp[-1] or (rw is not None and rw.size != ri.size):
                raise ValueError("regions must be (regptr (nreg + 1,), regidx (regptr[-1],), regw or None)")
        nd = max(ndraws, 0)
        mean, sd, mc_mean, mc_var = np.zeros(nq), np.zeros(nq), np.zeros(nq), np.zeros(nq)
        exceed = np.zeros((nthr, nq))
        rtot, rmax, rmin = (np.zeros((nreg, nd), order="F") for _ in range(3))
        rarea = np.zeros((nreg, nthr, nd), order="F")
        rwt, rcnt = np.zeros(nreg), np.zeros(nreg, dtype=np.int64)
        nlev, nlaunch, nf = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        u8, i64p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        lib = L.lib()
        L.check(lib.gpv_plan_debug_csim_chunk(self._h, int(chunk)), "gpv_plan_debug_csim_chunk")
        try:
            L.check(lib.gpv_plan_cond_sim_summary(
                self._h, str(covmodel).encode(), L.dptr(cp), cp.size, L.dptr(nug), nug.size, None if Z is None else L.dptr(Z), 1,
                L.dptr(q), nq, int(m), None if nn is None else L.iptr(nn), None if sc is None else L.dptr(sc),
                None if el is None else el.ctypes.data_as(u8), int(seed), int(col0), ndraws, None if off is None else L.dptr(off),
                int(link), nthr, L.dptr(thr) if nthr else None, nreg, None if rp is None else rp.ctypes.data_as(i64p),
                None if ri is None else ri.ctypes.data_as(i32p), None if rw is None else L.dptr(rw),
                L.dptr(mean), L.dptr(sd), L.dptr(mc_mean), L.dptr(mc_var), L.dptr(exceed), L.dptr(rtot), L.dptr(rmax), L.dptr(rmin),
                L.dptr(rarea), L.dptr(rwt), rcnt.ctypes.data_as(i64p), C.byref(nlev), C.byref(nlaunch), C.byref(nf)),
                "gpv_plan_cond_sim_summary")
        finally:
            lib.gpv_plan_debug_csim_chunk(self._h, 0)
        return dict(mean=mean, sd=sd, mc_mean=mc_mean, mc_var=mc_var, exceed=exceed, reg_total=rtot, reg_max=rmax, reg_min=rmin,
                    reg_area=np.ascontiguousarray(rarea.transpose(1, 0, 2)), reg_weight=rwt, reg_count=rcnt,
                    n_levels=int(nlev.value), n_launches=int(nlaunch.value), n_failed=int(nf.value))

    def krige_groups(self, covmodel, covparms, nuggets_ord, qlocs, gptr, m, Z_ord=None, weights=None, NNg=None, scale=None,
                     eligible_ord=None, chunk=0, want_cov=False):
        """Grouped local kriging under the cond.yz='z' model of this plan (gpv_plan_krige_groups): group k is the rows
        gptr[k] .. gptr[k + 1] - 1 of qlocs (nq, dim), its members share the conditioning set of the m observations nearest to
        their mean (m + g <= 64) and are predicted jointly, one solve per group.  nuggets_ord, Z_ord, scale, eligible_ord: as
        Plan.krige; weights: None (1 / g each) or nq numbers of any sign; NNg: None (searched at the groups' anchors) or
        (ngroups, m) ORDERED ids, 1-based, 0 = none; chunk: groups per pass (0: the default), which changes no bit.  Returns
        (mean (nq, ncols), var (nq,), gmean (ngroups, ncols), gvar (ngroups,), cov, n_failed): per location the predictive mean
        and the variance of the latent field, per group the weighted mean, its variance w' Sigma_G w, and with want_cov the
        packed lower triangles of the joint covariances Sigma_G (row-major, group after group; else None).  Everything of a
        group that failed (a member on an observation that has no nugget) is NaN and it is counted in n_failed."""
        q = np.asfortranarray(np.asarray(qlocs, dtype=np.float64).reshape(-1, self.dim))
        nq = q.shape[0]
        gp = np.ascontiguousarray(gptr, dtype=np.int64).reshape(-1)
        if gp.size < 1:
            raise ValueError("gptr must hold ngroups + 1 offsets")
        ng = gp.size - 1
        cp = np.ascontiguousarray(covparms, dtype=np.float64).reshape(-1)
        nug = np.ascontiguousarray(np.atleast_1d(np.asarray(nuggets_ord, dtype=np.float64)))
        Z, ncols = None, 1
        if Z_ord is not None:
            Z = np.asarray(Z_ord, dtype=np.float64)
            Z = np.asfortranarray(Z[:, None] if Z.ndim == 1 else Z)
            if Z.ndim != 2 or Z.shape[0] != self.Nlocs:
                raise ValueError("Z_ord must have one row per ordered location of the plan")
            ncols = Z.shape[1]
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if w.size != nq:
                raise ValueError("weights must hold one number per prediction location")
        nn = None
        if NNg is not None:
            nn = np.asfortranarray(NNg, dtype=np.int32)
            if nn.shape != (ng, int(m)):
                raise ValueError("NNg must be (ngroups, m)")
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
        if sc is not None and sc.size != self.dim:
            raise ValueError("scale must hold one number per coordinate")
        el = None
        if eligible_ord is not None:
            el = np.ascontiguousarray(np.asarray(eligible_ord).astype(bool).reshape(-1), dtype=np.uint8)
            if el.shape[0] != self.Nlocs:
                raise ValueError("eligible_ord must hold one flag per ordered location of the plan")
        mean, var = np.zeros((nq, ncols), order="F"), np.zeros(nq)
        gmean, gvar = np.zeros((ng, ncols), order="F"), np.zeros(ng)
        cov = None
        if want_cov:
            g = np.diff(gp)
            cov = np.zeros(max(int(np.sum(g * (g + 1) // 2)) if ng and np.all(g >= 0) else 0, 1))
        nf = C.c_int64(0)
        u8 = C.POINTER(C.c_uint8)
        L.check(L.lib().gpv_plan_krige_groups(self._h, str(covmodel).encode(), L.dptr(cp), cp.size, L.dptr(nug), nug.size,
                                              None if Z is None else L.dptr(Z), self.Nlocs, ncols, L.dptr(q), nq,
                                              gp.ctypes.data_as(C.POINTER(C.c_int64)), ng, None if w is None else L.dptr(w), int(m),
                                              None if nn is None else L.iptr(nn), None if sc is None else L.dptr(sc),
                                              None if el is None else el.ctypes.data_as(u8), int(chunk), L.dptr(mean), max(nq, 1),
                                              L.dptr(var), L.dptr(gmean), max(ng, 1), L.dptr(gvar),
                                              None if cov is None else L.dptr(cov), C.byref(nf)), "gpv_plan_krige_groups")
        return mean, var, gmean, gvar, cov, int(nf.value)

    def unwhiten_levels(self):
        """(n_levels, n_launches) of the level schedule unwhiten and simulate sweep through, built at first use
        (gpv_plan_unwhiten_levels): the rows of a level depend on earlier levels only; a launch is one level wider than
        gpv_unwhiten_narrow() rows or one maximal run of consecutive narrower ones."""
        nl, nk = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().gpv_plan_unwhiten_levels(self._h, C.byref(nl), C.byref(nk)), "gpv_plan_unwhiten_levels")
        return int(nl.value), int(nk.value)

    def simulate(self, seed, ncols, col0=0):
        """Draws col0 .. col0 + ncols - 1 from the Vecchia approximation of N(0, C + tau I) of the plan's latest evaluation
        (GPV_WANT_U), in the ORDERED row numbering (gpv_plan_simulate): the colouring of the library's own normals, the
        function of (seed, ordered location, draw) that draws_normals_host returns, made on the device.  Returns
        (Z_ord (Nlocs, ncols), n_failed).  A draw's bits do not depend on col0, ncols or the other draws of the call."""
        ncols, col0 = int(ncols), int(col0)
        if ncols < 1 or col0 < 0:
            raise ValueError("simulate needs ncols >= 1 and col0 >= 0")
        Z = np.zeros((self.Nlocs, ncols), order="F")
        nf = C.c_int64(0)
        L.check(L.lib().gpv_plan_simulate(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, col0, ncols, L.dptr(Z), self.Nlocs, C.byref(nf)),
                "gpv_plan_simulate")
        return Z, int(nf.value)

    def lincomb(self, H_ord, cov_mat=False):
        """Var(H y | z) (or, with cov_mat, Cov) for the rows of H_ord, a scipy.sparse or dense matrix with Nlocs columns in
        the plan's ORDERED latent index, from the factor of the latest evaluation with GPV_WANT_DENOM / GPV_WANT_MEAN /
        GPV_WANT_MEAN_B (gpv_plan_lincomb: one batched triangular solve on the device, nothing is factorised again)."""
        import scipy.sparse as sp
        H = H_ord.tocsr() if sp.issparse(H_ord) else sp.csr_matrix(np.atleast_2d(np.asarray(H_ord, dtype=np.float64)))
        if H.shape[1] != self.Nlocs:
            raise ValueError("H_ord must have one column per ordered location of the plan")
        H.sum_duplicates()
        nrows = int(H.shape[0])
        hptr = np.ascontiguousarray(H.indptr, dtype=np.int64)
        hidx = np.ascontiguousarray(H.indices, dtype=np.int32)
        hval = np.ascontiguousarray(H.data, dtype=np.float64)
        vars_ = np.zeros(max(nrows, 1))
        cov = np.zeros((nrows, nrows)) if cov_mat else None
        st = L.lib().gpv_plan_lincomb(self._h, nrows, hptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                      hidx.ctypes.data_as(C.POINTER(C.c_int32)), L.dptr(hval), L.dptr(vars_),
                                      L.dptr(cov) if cov_mat else None)
        L.check(st, "gpv_plan_lincomb")
        return cov if cov_mat else vars_[:nrows]

    def selinv(self, skip_front=0):
        """Every posterior variance of the plan in one pass: the diagonal of the selected inverse of the factor lincomb reads
        (gpv_plan_selinv: the Takahashi recursion on the factor's own pattern, level scheduled, on the device).  Returns
        (vars_ord (Nlocs,), ordered layout, zeros in the first skip_front rows; n_dropped): n_dropped == 0 means vars_ord is
        diag(W^-1) exactly, otherwise n_dropped terms lie outside the pattern and the result is the reference's
        var.exact = FALSE approximation."""
        out = np.zeros(self.Nlocs)
        nd = C.c_int64(0)
        L.check(L.lib().gpv_plan_selinv(self._h, int(skip_front), L.dptr(out), C.byref(nd)), "gpv_plan_selinv")
        return out, int(nd.value)

    def solve_t(self, E_ord):
        """R^T x = e for every row e of E_ord, (ncols, Nlocs) or (Nlocs,) float64 in the plan's ORDERED latent layout, with
        the factor lincomb reads (gpv_plan_solve_t: batched, level scheduled, on the device).  For e ~ N(0, I) the rows of the
        result have covariance W^-1: posterior_mean() + x is a posterior draw.  Returns an array of the same shape."""
        E = np.asarray(E_ord, dtype=np.float64)
        if E.ndim not in (1, 2) or E.shape[-1] != self.Nlocs:
            raise ValueError("E_ord must have one entry per ordered location of the plan in its last dimension")
        E2 = np.ascontiguousarray(np.atleast_2d(E))
        X = np.empty_like(E2)
        ncols = int(E2.shape[0])
        st = L.lib().gpv_plan_solve_t(self._h, ncols, L.dptr(E2), self.Nlocs, L.dptr(X), self.Nlocs)
        L.check(st, "gpv_plan_solve_t")
        return X.reshape(E.shape)

    def draws_normals(self, seed, ncols, col0=0, skip_front=0):
        """The standard normals gpv_plan_draws_summary's device generator writes for the draws [col0, col0 + ncols) with this
        seed, read back (gpv_plan_draws_normals): (ncols, Nlocs) in the plan's ORDERED latent layout, zeros in the first
        skip_front columns.  A function of (seed, location, draw) alone: solve_t of these rows are the draws the summary sums."""
        E = np.empty((int(ncols), self.Nlocs))
        st = L.lib().gpv_plan_draws_normals(self._h, int(seed), int(skip_front), int(col0), int(ncols), L.dptr(E), self.Nlocs)
        L.check(st, "gpv_plan_draws_normals")
        return E

    def draws_summary(self, ndraws, seed=0, skip_front=0, mu_ord=None, link=0, thresholds=None, mask=None, draw_stats=True):
        """Monte-Carlo summaries of ndraws posterior draws y = mu_ord + R^-T e, reduced on the device (gpv_plan_draws_summary):
        normals from the device generator, 32 draws per transposed sweep, sums folded after every sweep.  link 0 / 1 / 2 = g:
        identity / exp / logistic.  Returns dict(mean, var (Nlocs each, of g(y)), exceed (len(thresholds) x Nlocs: the share of
        draws with y > threshold, LATENT scale), draw_max, draw_mean (ndraws each: of g(y) over the locations of `mask`, a
        boolean per ordered location, None = all behind skip_front; None with draw_stats=False)), ordered layout."""
        n, ndraws = self.Nlocs, int(ndraws)
        mu = None if mu_ord is None else np.ascontiguousarray(mu_ord, dtype=np.float64)
        if mu is not None and mu.shape != (n,):
            raise ValueError("mu_ord must have one entry per ordered location of the plan")
        thr = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=bool), dtype=np.uint8)
        if mk is not None and mk.shape != (n,):
            raise ValueError("mask must have one entry per ordered location of the plan")
        mean, var = np.empty(n), np.empty(n)
        exceed = np.empty((thr.size, n))
        dmax, dmean = (np.empty(max(ndraws, 0)), np.empty(max(ndraws, 0))) if draw_stats else (None, None)
        st = L.lib().gpv_plan_draws_summary(
            self._h, ndraws, int(seed), int(skip_front), None if mu is None else L.dptr(mu), int(link), int(thr.size),
            L.dptr(thr) if thr.size else None, None if mk is None else mk.ctypes.data_as(C.POINTER(C.c_uint8)),
            L.dptr(mean), L.dptr(var), L.dptr(exceed) if thr.size else None,
            None if dmax is None else L.dptr(dmax), None if dmean is None else L.dptr(dmean))
        L.check(st, "gpv_plan_draws_summary")
        return dict(mean=mean, var=var, exceed=exceed, draw_max=dmax, draw_mean=dmean)

    kernel_timing = True

    def set_kernel_timing(self, on):
        L.check(L.lib().gpv_plan_set_kernel_timing(self._h, int(bool(on))), "gpv_plan_set_kernel_timing")
        self.kernel_timing = bool(on)

    def last_kernel_ms(self):
        ms = C.c_double()
        L.check(L.lib().gpv_plan_last_kernel_ms(self._h, C.byref(ms)), "gpv_plan_last_kernel_ms")
        return float(ms.value)

    def last_set_kernel(self):
        """Bit flags of the conditioning-set kernel the last eval ran: 1 = likelihood-only sweep, 2 = its lean variant."""
        return int(L.lib().gpv_plan_last_set_kernel(self._h))

    def set_comm(self, comm):
        """Attach (or, with None, detach) a Comm: every eval() then all-reduces its 8 sums over the ranks, inside the library."""
        L.check(L.lib().gpv_plan_set_comm(self._h, comm._h if comm is not None else None), "gpv_plan_set_comm")
        self._comm = comm                                     # keeps the communicator alive as long as the plan uses it


class Comm:
    """gpv_comm: an RCCL communicator owned by the library (one process per GPU).  `exchange(id_bytes_or_None) -> id_bytes`
    carries rank 0's 128-byte id to the other ranks (from_torch() does it over an initialised torch.distributed group)."""

    def __init__(self, device, rank, world, exchange=None, ident=None):
        """exchange(id_bytes_or_None) -> id_bytes carries rank 0's id to the others; or `ident`: the 128 bytes every rank
        already holds (Comm.exchange_id in a first step: negotiate_comm does the exchange on the caller's thread and only the
        collective gpv_comm_create on a helper thread)."""
        raw = ident if ident is not None else Comm.exchange_id(rank, exchange)
        if not isinstance(raw, (bytes, bytearray)) or len(raw) != 128:
            raise ValueError("Comm: the exchange must hand every rank the 128 bytes of rank 0")
        ident = C.create_string_buffer(bytes(raw), 128)
        self._h = C.c_void_p()
        self.device, self.rank, self.world = int(device), int(rank), int(world)
        L.check(L.lib().gpv_comm_create(C.byref(self._h), self.device, self.rank, self.world, ident), "gpv_comm_create")

    @staticmethod
    def exchange_id(rank, exchange):
        """Rank 0 makes the communicator id and `exchange` hands it to every rank.  Rank 0 ALWAYS takes part in the exchange:
        if it could not make the id it hands out an empty one and every rank raises here, instead of rank 0 raising alone
        while the others wait for a broadcast that never comes."""
        ident = C.create_string_buffer(128)
        st0 = L.lib().gpv_comm_unique_id(ident) if rank == 0 else 0
        raw = exchange((bytes(ident.raw) if st0 == 0 else b"") if rank == 0 else None)
        if rank == 0:
            L.check(st0, "gpv_comm_unique_id")
        if raw == b"":
            raise RuntimeError("Comm: rank 0 could not produce the communicator id (no RCCL to bind?)")
        return raw

    @staticmethod
    def torch_exchange(group=None):
        """The exchange over an initialised torch.distributed group (call it on the thread that owns the rank's GPU: with
        the nccl backend the broadcast moves through torch.cuda.current_device() of the CALLING thread)."""
        import torch.distributed as dist

        def exchange(mine):
            box = [mine]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            return box[0]
        return exchange

    @classmethod
    def from_torch(cls, device, group=None):
        """Collective over the torch group.  Raises on EVERY rank alike when rank 0 cannot produce the id; for a route that
        is agreed between the ranks (and a fallback when the library's communicator is unavailable on any of them) use
        gpvecchia_amd.distributed.negotiate_comm."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)

        def exchange(mine):
            box = [mine]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            return box[0]
        return cls(device, rank, world, exchange)

    @staticmethod
    def rccl_version():
        """ncclGetVersion() of the RCCL the library bound at run time; 0 when there is none (gpv_comm_* then return GPV_ERR_STATE)."""
        return int(L.lib().gpv_rccl_version())

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                L.lib().gpv_comm_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


class MultiPlan:
    """gpv_mplan: the same vecchia.approx spread over several GPUs of one host process (row shards)."""

    def __init__(self, locsord, revNNarray, revCond, devices):
        locs = np.asfortranarray(locsord, dtype=np.float64)
        self.Nlocs, self.dim = locs.shape
        nn = L.as_r_int_matrix(revNNarray)
        cd = _cond_to_r(revCond)
        self.p = nn.shape[1]
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        self._h = C.c_void_p()
        L.check(L.lib().gpv_mplan_create(C.byref(self._h), L.iptr(dev), int(dev.size), self.Nlocs, self.dim, self.p,
                                         L.dptr(locs), L.iptr(nn), L.iptr(cd)), "gpv_mplan_create")

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                L.lib().gpv_mplan_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def set_data(self, z_ord):
        z = np.ascontiguousarray(z_ord, dtype=np.float64)
        L.check(L.lib().gpv_mplan_set_data(self._h, L.dptr(z)), "gpv_mplan_set_data")

    def eval(self, covmodel, covparms, nuggets, flags):
        cp = np.ascontiguousarray(covparms, dtype=np.float64)
        ng = np.ascontiguousarray(np.atleast_1d(nuggets), dtype=np.float64)
        s = np.zeros(NSUMS)
        L.check(L.lib().gpv_mplan_eval(self._h, str(covmodel).encode(), L.dptr(cp), int(cp.size), L.dptr(ng),
                                       int(ng.size), int(flags), L.dptr(s)), "gpv_mplan_eval")
        return s

    def Lentries(self):
        out = np.zeros((self.Nlocs, self.p), dtype=np.float64, order="F")
        L.check(L.lib().gpv_mplan_get_Lentries(self._h, L.dptr(out)), "gpv_mplan_get_Lentries")
        return out


class ReplicaPlans:
    """gpv_mplan in REPLICA mode: one complete plan per listed device, each evaluating its own parameter vector (or its
    own data set), all in flight together.  This is what several GPUs mean for the parts of the path that do not shard:
    the posterior pass of cond.yz='SGV' and every Vecchia-Laplace Newton step (BASELINE.json configs[4])."""

    def __init__(self, locsord, revNNarray, revCond, devices):
        locs = np.asfortranarray(locsord, dtype=np.float64)
        self.Nlocs, self.dim = locs.shape
        self._nn = L.as_r_int_matrix(revNNarray)
        self._cd = _cond_to_r(revCond)
        self.p = self._nn.shape[1]
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        self.count = int(dev.size)
        self._h = C.c_void_p()
        L.check(L.lib().gpv_mplan_create_replicas(C.byref(self._h), L.iptr(dev), self.count, self.Nlocs, self.dim, self.p,
                                                  L.dptr(locs), L.iptr(self._nn), L.iptr(self._cd)), "gpv_mplan_create_replicas")
        self.has_posterior = False

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                L.lib().gpv_mplan_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def set_data(self, z_ord, replica=None):
        z = np.ascontiguousarray(z_ord, dtype=np.float64)
        if z.shape[0] != self.Nlocs:
            raise ValueError("z_ord must have one entry per ordered location")
        if replica is None:
            L.check(L.lib().gpv_mplan_set_data(self._h, L.dptr(z)), "gpv_mplan_set_data")
        else:
            L.check(L.lib().gpv_mplan_set_data_one(self._h, int(replica), L.dptr(z)), "gpv_mplan_set_data_one")

    def build_posterior(self):
        self.has_posterior = False
        L.check(L.lib().gpv_mplan_build_posterior(self._h, L.iptr(self._nn), L.iptr(self._cd)), "gpv_mplan_build_posterior")
        self.has_posterior = True

    def eval_each(self, covmodel, covparms, nuggets, flags):
        """covparms: (count, ncovparms), nuggets: (count,) constant nugget of each replica -> sums (count, NSUMS)."""
        cp = np.ascontiguousarray(covparms, dtype=np.float64).reshape(self.count, -1)
        ng = np.ascontiguousarray(np.broadcast_to(np.asarray(nuggets, dtype=np.float64), (self.count,)))
        s = np.zeros((self.count, NSUMS))
        L.check(L.lib().gpv_mplan_eval_each(self._h, str(covmodel).encode(), L.dptr(cp), int(cp.shape[1]), L.dptr(ng),
                                            int(flags), L.dptr(s)), "gpv_mplan_eval_each")
        return s

    def logliks(self, covmodel, covparms, nuggets, cond_yz="SGV"):
        """vecchia_likelihood of every replica's parameter vector: cond.yz='z' fused, 'SGV' with the posterior pass."""
        if cond_yz == "z":
            s = self.eval_each(covmodel, covparms, nuggets, GPV_WANT_LOGLIK_Z)
            return np.array([loglik_z_from_sums(r, self.Nlocs) for r in s])
        if not self.has_posterior:
            self.build_posterior()
        s = self.eval_each(covmodel, covparms, nuggets, GPV_WANT_DENOM)
        return np.array([loglik_from_sums(r, self.Nlocs) for r in s])


_R_LAYOUT_CACHE = []          # [(weakref(revNNarray), weakref(revCond), fingerprint, nn_r, cd_r)] of the last two index-array pairs


def _fingerprint(a):
    """Content fingerprint of an index array: shape, dtype, strides and the library's 128-bit hash of EVERY byte
    (gpv_hash_bytes: the multi-threaded hash the plan cache of the literal drop-in keys on, ~3-4 ms for the two arrays of
    n = 1e6, m = 30; no optional module, no 32-bit fallback).  An in-place edit of the array between two calls changes it.
    None for an empty array (nothing worth caching)."""
    a = np.asarray(a)
    if a.size == 0:
        return None
    buf = a if a.flags.c_contiguous or a.flags.f_contiguous else np.ascontiguousarray(a)
    out = (C.c_uint64 * 2)()
    L.check(L.lib().gpv_hash_bytes(C.c_void_p(buf.ctypes.data), buf.nbytes, 0x6770765F6670, out), "gpv_hash_bytes")
    return (a.shape, a.dtype.str, a.strides, int(out[0]), int(out[1]))


def _r_layout_cached(revNNarray, revCond):
    """Column-major int32 copies (R's representation) of the two index arrays, kept for the arrays last seen: createU hands
    the SAME objects to U_NZentries at every optimiser step, and converting 2 x 31e6 entries costs ~60 ms, six times the
    library call.  A hit needs the same two objects (held by weak reference: the cache keeps no caller array alive) AND an
    unchanged hash of their whole content, so an array edited in place between two calls is converted again."""
    import weakref
    fp = (_fingerprint(revNNarray), _fingerprint(revCond))
    if fp[0] is None or fp[1] is None:                                 # empty arrays: convert, do not cache
        return L.as_r_int_matrix(revNNarray), _cond_to_r(revCond)
    for wa, wb, f, nn_r, cd_r in _R_LAYOUT_CACHE:
        if wa() is revNNarray and wb() is revCond and f == fp:
            return nn_r, cd_r
    nn_r, cd_r = L.as_r_int_matrix(revNNarray), _cond_to_r(revCond)
    try:
        _R_LAYOUT_CACHE.insert(0, (weakref.ref(revNNarray), weakref.ref(revCond), fp, nn_r, cd_r))
    except TypeError:                                                  # not weakly referenceable (a list, ...): do not cache
        return nn_r, cd_r
    del _R_LAYOUT_CACHE[2:]
    return nn_r, cd_r


def _cond_to_r(revCond):
    """logical matrix -> R's int representation: NaN (float input) or -1 (int8 input) -> NA_INTEGER."""
    rc = np.asarray(revCond)
    if rc.dtype.kind == "f":
        return L.as_r_int_matrix(rc)
    out = np.asarray(rc, dtype=np.int32, order="F")                  # one pass: cast and transpose together
    if out is rc or np.shares_memory(out, rc):
        out = out.copy(order="F")
    out[out < 0] = L.NA_INTEGER
    return out


def loglik_z_from_sums(sums, n):
    out = C.c_double()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    L.check(L.lib().gpv_loglik_z_from_sums(L.dptr(s), int(n), C.byref(out)), "gpv_loglik_z_from_sums")
    return float(out.value)


def loglik_from_sums(sums, n):
    """R/vecchia_likelihood.R:95-96 from sums evaluated with GPV_WANT_DENOM."""
    out = C.c_double()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    L.check(L.lib().gpv_loglik_from_sums(L.dptr(s), int(n), C.byref(out)), "gpv_loglik_from_sums")
    return float(out.value)


def numerator_from_sums(sums):
    a, b = C.c_double(), C.c_double()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    L.check(L.lib().gpv_numerator_from_sums(L.dptr(s), C.byref(a), C.byref(b)), "gpv_numerator_from_sums")
    return float(a.value), float(b.value)


# ---------------------------------------------------------------------------
# literal drop-ins (R/RcppExports.R)
# ---------------------------------------------------------------------------
def U_NZentries(Ncores, n, locs, revNNarray, revCondOnLatent, nuggets, nuggets_obsord, covType, covparms):
    """R/RcppExports.R:22-24: returns dict(Lentries=(Nlocs, m+1), Zentries=(2n,)) (+ n_failed).
    Goes through the C symbol gpv_U_NZentries exactly as the R .C() binding would."""
    locs = np.asfortranarray(locs, dtype=np.float64)
    Nlocs, dim = locs.shape
    nn, cd = _r_layout_cached(revNNarray, revCondOnLatent)
    p = nn.shape[1]
    nug = np.ascontiguousarray(nuggets, dtype=np.float64)
    nugo = np.ascontiguousarray(nuggets_obsord, dtype=np.float64)
    cp = np.ascontiguousarray(covparms, dtype=np.float64)
    Lent = np.empty((Nlocs, p), dtype=np.float64, order="F")          # every entry is written by the library
    Z = np.zeros(2 * int(n), dtype=np.float64)
    ci = lambda v: C.byref(C.c_int(int(v)))
    nfail, status = C.c_int(0), C.c_int(0)
    ct = C.c_char_p(str(covType).encode())
    L.lib().gpv_U_NZentries(ci(Ncores), ci(n), ci(Nlocs), ci(dim), ci(p), L.dptr(locs), L.iptr(nn), L.iptr(cd),
                            L.dptr(nug), L.dptr(nugo), C.byref(ct), L.dptr(cp), ci(cp.size), L.dptr(Lent), L.dptr(Z),
                            C.byref(nfail), C.byref(status))
    L.check(status.value, "gpv_U_NZentries")
    return dict(Lentries=Lent, Zentries=Z, n_failed=int(nfail.value))


def U_NZentries_mat(Ncores, n, locs, revNNarray, revCondOnLatent, nuggets, nuggets_obsord, covVals, covparms):
    """R/RcppExports.R:26-28 (locs/revCond/nuggets/covparms are unused by the reference body)."""
    nn = L.as_r_int_matrix(revNNarray)
    Nlocs, p = nn.shape
    nugo = np.ascontiguousarray(nuggets_obsord, dtype=np.float64)
    cv = np.asfortranarray(covVals, dtype=np.float64)
    if cv.shape != (Nlocs, Nlocs):
        raise ValueError("covVals must be Nlocs x Nlocs")
    Lent = np.zeros((Nlocs, p), dtype=np.float64, order="F")
    Z = np.zeros(2 * int(n), dtype=np.float64)
    ci = lambda v: C.byref(C.c_int(int(v)))
    nfail, status = C.c_int(0), C.c_int(0)
    L.lib().gpv_U_NZentries_mat(ci(Ncores), ci(n), ci(Nlocs), ci(p), L.iptr(nn), L.dptr(nugo), L.dptr(cv),
                                L.dptr(Lent), L.dptr(Z), C.byref(nfail), C.byref(status))
    L.check(status.value, "gpv_U_NZentries_mat")
    return dict(Lentries=Lent, Zentries=Z, n_failed=int(nfail.value))


def _covfun(name, distmat, covparms):
    d = np.ascontiguousarray(distmat, dtype=np.float64)
    cp = np.ascontiguousarray(covparms, dtype=np.float64)
    out = np.empty_like(d)
    status = C.c_int(0)
    getattr(L.lib(), name)(L.dptr(d), C.byref(C.c_int(d.size)), L.dptr(cp), L.dptr(out), C.byref(status))
    L.check(status.value, name)
    return out


def MaternFun(distmat, covparms):
    """src/Matern.cpp:24-86 (closed-form smoothness values)."""
    return _covfun("gpv_MaternFun", distmat, covparms)


def EsqeFun(distmat, covparms):
    """src/Esqe.cpp:17-39."""
    return _covfun("gpv_EsqeFun", distmat, covparms)


# ---------------------------------------------------------------------------
# vecchia_specify — R/vecchia_specify.R:29-240
# ---------------------------------------------------------------------------
def vecchia_specify(locs, m=-1, ordering=None, cond_yz=None, locs_pred=None, ordering_pred=None, pred_cond=None,
                    conditioning=None, mra_options=None, ic0=False, verbose=False, NNarray=None, nn_backend="auto", scale=None):
    """Parameter-independent specification of the Vecchia approximation, conditioning='NN':
    ordering in {'coord','maxmin','outsidein','none'}; cond.yz in {'SGV','SGVT','y','z','zy','RVP','LK'}; prediction
    locations with ordering.pred in {'obspred','general'} and pred.cond in {'general','independent'}; the m = 0
    independent case.  MRA / 'firstm' conditioning goes through ic0 in the reference, never through U_NZentries
    (R/createU.R:89): not built (NotImplementedError).
    scale: None, or one positive number per coordinate (for covmodel='matern_scaledim': the ranges).  Ordering and neighbour
    search then run on locs / scale (and locs_pred / scale) -- neighbours chosen in unscaled space are poor under strong
    anisotropy -- while locsord keeps the true coordinates.  scale=None is the specification it always was."""
    locs = np.asarray(locs, dtype=np.float64)
    if locs.ndim != 2:
        warnings.warn("Locations must be in matrix form")                    # :32-35
        return None
    if scale is not None:
        sc = np.asarray(scale, dtype=np.float64).reshape(-1)
        if sc.size != locs.shape[1] or not np.all(np.isfinite(sc)) or not np.all(sc > 0):
            raise ValueError("scale must hold one positive finite number per coordinate")
        lp = None if locs_pred is None else np.asarray(locs_pred, dtype=np.float64).reshape(-1, locs.shape[1])
        va = vecchia_specify(locs / sc, m, ordering=ordering, cond_yz=cond_yz, locs_pred=None if lp is None else lp / sc,
                             ordering_pred=ordering_pred, pred_cond=pred_cond, conditioning=conditioning,
                             mra_options=mra_options, ic0=ic0, verbose=verbose, NNarray=NNarray, nn_backend=nn_backend)
        # the true coordinates in the rows of the scaled specification's locsord: the ordering of (locs, locs_pred), and for the
        # response-latent layouts ('zy') the observed block once more in front (R/vecchia_specify.R:196)
        true = (locs if lp is None else np.vstack([locs, lp]))[va["ord"] - 1]
        if va["locsord"].shape[0] != true.shape[0]:
            true = np.vstack([true[:locs.shape[0]], true])
        assert true.shape == va["locsord"].shape
        va["locsord"] = true
        return va
    if m is None or m == -1:
        raise ValueError("neither m nor r defined!")                        # :36-40
    if conditioning not in (None, "NN"):
        raise NotImplementedError("conditioning='mra'/'firstm' goes through ic0, not U_NZentries (R/createU.R:89)")
    spatial_dim = locs.shape[1]
    n = locs.shape[0]
    have_pred = locs_pred is not None
    if have_pred:                                                            # :46-51
        locs_pred = np.asarray(locs_pred, dtype=np.float64).reshape(-1, spatial_dim)
        la = np.vstack([locs, locs_pred])
        if np.unique(la, axis=0).shape[0] < la.shape[0]:
            raise ValueError("Prediction locations contain observed location(s), remove redundancies.")
    if m > n:                                                                # :53-56
        warnings.warn("Conditioning set size m chosen to be larger than n. Changing to m=n-1")
        m = n - 1
    if m == 0:                                                               # :59-73
        if have_pred:
            warnings.warn("Attempting to make predictions with m=0.  Prediction ignored")
        ord_ = np.arange(1, n + 1)
        NN = np.stack([ord_, np.zeros(n, dtype=np.int64)], axis=1).astype(np.int32)
        Cond = np.stack([np.ones(n), -np.ones(n)], axis=1).astype(np.int8)
        obs = np.ones(n, dtype=bool)
        U_prep = S.U_sparsity(locs, NN, obs, Cond)
        return dict(locsord=locs.copy(), obs=obs, ord=ord_, ord_z=ord_.copy(), ord_pred="general", U_prep=U_prep,
                    cond_yz="false", conditioning="NN", ic0=False)
    if ordering is None:                                                     # :83-85
        ordering = "coord" if spatial_dim == 1 else "maxmin"
    if pred_cond is None:                                                    # :86
        pred_cond = "general"
    if cond_yz is None:                                                      # :92-96
        cond_yz = "SGV" if (not have_pred or spatial_dim == 1) else "zy"
    if ordering not in ("coord", "maxmin", "outsidein", "none"):
        raise ValueError(f"ordering='{ordering}' not defined")
    n_p = 0
    if not have_pred:                                                        # :100-117
        if ordering == "coord":                                              # :102
            ord_ = S.order_coordinate(locs)
        elif ordering == "maxmin":                                           # :103-106
            o = S.order_maxmin_exact(locs)
            cut = min(n, 9)
            ord_ = np.concatenate([o[:1], o[cut:], o[1:cut]])
        elif ordering == "outsidein":                                        # :107-108
            ord_ = S.order_outsidein(locs)
        else:                                                                # :109-110
            ord_ = np.arange(1, n + 1)
        ord_z = ord_.copy()
        locsord = locs[ord_ - 1]
        obs = np.ones(n, dtype=bool)
        ordering_pred = "general"
    else:                                                                    # :119-149 prediction is desired
        n_p = locs_pred.shape[0]
        locs_all = np.vstack([locs, locs_pred])
        observed_obspred = np.concatenate([np.ones(n, bool), np.zeros(n_p, bool)])
        if ordering_pred is None:                                            # :124-126
            ordering_pred = "general" if (spatial_dim == 1 and ordering == "coord") else "obspred"
        if ordering_pred == "general":                                       # :127-131
            ord_ = S.order_coordinate(locs_all) if ordering == "coord" else S.order_maxmin_exact(locs_all)
            ord_obs = ord_[ord_ <= n]
        else:                                                                # :132-145
            if ordering == "coord":
                ord_obs, ord_pr = S.order_coordinate(locs), S.order_coordinate(locs_pred)
            elif ordering == "none":
                ord_obs, ord_pr = np.arange(1, n + 1), np.arange(1, n_p + 1)
            else:
                ord_obs, ord_pr = S.order_maxmin_exact_obs_pred(locs, locs_pred)
            ord_ = np.concatenate([ord_obs, ord_pr + n])
        ord_z = ord_obs
        locsord = locs_all[ord_ - 1]
        obs = observed_obspred[ord_ - 1]
    nall = locsord.shape[0]
    if NNarray is None:                                                      # :157-159
        # both searches implement the same exact definition and return identical arrays (tests); "gpu" is the
        # library's brute-force kernel, "host" the cKDTree search
        use_gpu = (nn_backend == "gpu" or (nn_backend == "auto" and L.device_count() > 0 and nall >= 2000)) and \
            spatial_dim <= 8 and m <= L.lib().gpv_nn_max_m()                 # limits of gpv_find_ordered_nn (LDS of one CU)
        NNarray = S.find_ordered_nn_gpu(locsord, m) if use_gpu else S.find_ordered_nn(locsord, m)
    NNarray = np.asarray(NNarray).astype(np.int32)
    if have_pred and pred_cond == "independent":                             # :168-178
        if ordering_pred == "obspred":
            # every prediction location conditions on itself and its m nearest OBSERVED locations, descending index
            from scipy.spatial import cKDTree
            _, idx = cKDTree(locsord[:n]).query(locsord[n:], k=m)
            idx = np.sort(idx.reshape(n_p, m) + 1, axis=1)[:, ::-1]
            NNarray = NNarray.copy()
            NNarray[n:] = np.concatenate([(n + np.arange(1, n_p + 1))[:, None], idx], axis=1)
        else:
            warnings.warn("indep. conditioning currently only implemented for obspred ordering")
    if cond_yz == "SGV":                                                     # :182-183
        Cond = S.whichCondOnLatent(NNarray, firstind_pred=n + 1)
    elif cond_yz == "SGVT":                                                  # :184-185
        Cond = np.vstack([S.whichCondOnLatent(NNarray[:n]), np.ones((n_p, m + 1), dtype=np.int8)])
    elif cond_yz == "y":                                                     # :186-187
        Cond = np.where(NNarray != 0, 1, -1).astype(np.int8)
    elif cond_yz == "z":                                                     # :189-190
        if have_pred:
            raise ValueError("cond.yz='z' cannot be combined with prediction locations (an unobserved location has no z "
                             "to condition on; the reference fails in U_sparsity)")
        Cond = np.where(NNarray != 0, 0, -1).astype(np.int8)
        Cond[:, 0] = 1
    elif cond_yz in ("RVP", "LK", "zy"):                                     # :191-223 response-latent ('zy') trick
        obs = np.concatenate([np.ones(n, bool), np.zeros(nall, bool)])       # :195
        locsord = np.vstack([locsord[:n], locsord])                          # :196
        NNs = S.get_knn(locsord[:n], m - 1).astype(np.int64)                 # :199
        if cond_yz in ("RVP", "zy"):                                         # :200-203 latent y.obs where it comes earlier
            prev = NNs < np.arange(1, n + 1)[:, None]
            NNs[prev] += n
        NN_z = np.concatenate([np.arange(1, n + 1)[:, None], np.zeros((n, m), dtype=np.int64)], axis=1)       # :206
        NN_y = np.concatenate([(np.arange(1, n + 1) + n)[:, None], np.arange(1, n + 1)[:, None], NNs], axis=1)   # :207
        if not have_pred:                                                    # :208-210
            NN_yp = np.zeros((0, m + 1), dtype=np.int64)
            ordering_pred = "obspred"
        else:
            if ordering_pred != "obspred":
                warnings.warn("ZY only implemented for obspred ordering")
            NN_yp = NNarray[n: n + n_p].astype(np.int64)
            if cond_yz == "zy":                                              # :213-214
                NN_yp = np.where(NN_yp != 0, NN_yp + n, 0)
            else:                                                            # :215-218
                NN_yp = np.where(NN_yp > n, NN_yp + n, NN_yp)
        NNarray = np.vstack([NN_z, NN_y, NN_yp]).astype(np.int32)            # :220
        Cond = np.where(NNarray == 0, -1, (NNarray > n).astype(np.int8)).astype(np.int8)   # :223
        Cond[:, 0] = 1
        cond_yz = "zy"
    else:
        raise ValueError(f"cond.yz='{cond_yz}' not defined")                 # :226
    # a neighbour conditioned on as an observation must have one: the reference would put NA indices into sparseMatrix
    # (R/U_sparsity.R:52) and fail in createU; e.g. cond.yz='SGV' with ordering.pred='general' in two dimensions
    nb = np.where(NNarray > 0, NNarray - 1, 0)
    if np.any((Cond == 0) & (NNarray > 0) & ~np.asarray(obs)[nb]):
        raise ValueError(f"cond.yz='{cond_yz}' with ordering.pred='{ordering_pred}' conditions on the observation of an "
                         "unobserved location; use ordering.pred='obspred' or cond.yz in {'y','zy'}")
    U_prep = S.U_sparsity(locsord, NNarray, obs, Cond)                       # :230
    return dict(locsord=locsord, obs=obs, ord=ord_, ord_z=ord_z, ord_pred=ordering_pred, U_prep=U_prep,
                cond_yz=cond_yz, ic0=ic0, conditioning="NN")                 # :234-235


def _plan_for(va, device=0):
    key = ("_plan", device)
    if key not in va:
        prep = va["U_prep"]
        va[key] = Plan(va["locsord"], prep["revNNarray"], prep["revCond"], device=device)
    return va[key]


def _device_nuggets(va, nug):
    """Nugget argument of Plan.eval: a length-1 array when the nugget is constant (it then travels in the launch
    arguments), else the n-vector in ordering (R/createU.R:75-77)."""
    nug = np.atleast_1d(np.asarray(nug, dtype=np.float64))
    if nug.size == 1 or np.all(nug == nug[0]):
        return nug[:1]
    return nug[va["ord"] - 1]


def _ordered_nuggets(va, nuggets, n):
    """R/createU.R:73-78: (nuggets.all.ord for every row of locsord, nuggets.ord for the observations, nuggets)."""
    nug = np.atleast_1d(np.asarray(nuggets, dtype=np.float64))
    if nug.size == 1:
        nug = np.repeat(nug, n)                                               # :74
    nlat = va["locsord"].shape[0]                                            # = sum(latent)
    nug_all = np.concatenate([nug, np.zeros(nlat - n)])                      # :75 prediction / dummy locations carry none
    ord_ = va["ord"]
    ord_all = np.concatenate([ord_[:n], ord_ + n]) if va["cond_yz"] == "zy" else ord_   # :76
    return nug_all[ord_all - 1], nug_all[va["ord_z"] - 1], nug


# ---------------------------------------------------------------------------
# createU — R/createU.R:65-201 (NN branch)
# ---------------------------------------------------------------------------
def createU(vecchia_approx, covparms, nuggets, covmodel="matern", device=0):
    """Returns the U.obj list of R/createU.R:196-199 as a dict; U is a scipy.sparse CSC matrix."""
    import scipy.sparse as sp
    va = vecchia_approx
    prep = va["U_prep"]
    n = int(np.sum(va["obs"]))
    size = prep["size"]
    latent = np.zeros(size, dtype=bool)
    latent[prep["y_ind"] - 1] = True
    nug_all_ord, nug_ord, nug = _ordered_nuggets(va, nuggets, n)
    revNN, revCond = prep["revNNarray"], prep["revCond"]
    if np.any(nug == 0):                                                     # :83-86
        zero_idx = np.where(nug_ord == 0)[0] + 1
        revCond = revCond.copy()
        revCond[np.isin(revNN, zero_idx)] = 1
    plain = (n == va["locsord"].shape[0]) and va["cond_yz"] != "zy"          # every row observed: the resident plan serves
    if isinstance(covmodel, str):                                            # :152-154
        if np.any(nug == 0) or not plain:
            ent = U_NZentries(prep["n_cores"], n, va["locsord"], revNN, revCond, nug_all_ord, nug_ord, covmodel,
                              covparms)
            Lent, Zent = ent["Lentries"], ent["Zentries"]
        else:
            plan = _plan_for(va, device)
            plan.eval(covmodel, covparms, nug_all_ord if nug.size > 1 and not np.all(nug == nug[0]) else nug[:1],
                      GPV_WANT_U)
            Lent, Zent = plan.Lentries(), plan.Zentries()
    elif isinstance(covmodel, np.ndarray):                                   # :149-151
        ent = U_NZentries_mat(prep["n_cores"], n, va["locsord"], revNN, revCond, nug_all_ord, nug_ord, covmodel,
                              covparms)
        Lent, Zent = ent["Lentries"], ent["Zentries"]
    else:
        raise TypeError("argument 'covmodel' type not supported")            # :155
    # :158-160 keep the first n0 entries of every row (row-major walk), append Zentries
    n0 = (revNN != 0).sum(axis=1)
    keep = np.arange(revNN.shape[1])[None, :] < n0[:, None]
    vals = np.concatenate([np.ascontiguousarray(Lent)[keep], Zent])
    U = sp.csc_matrix((vals, (prep["colindices"] - 1, prep["rowpointers"] - 1)), shape=(size, size))   # :161-162
    ord_, obs, zero_nugg = va["ord"], va["obs"], {}
    if va["cond_yz"] == "zy":                                                # :166-171 rows/columns of the dummy y's
        keepd = np.ones(size, dtype=bool)
        keepd[2 * np.arange(n)] = False                                      # dummy = 2*(1:n)-1 (1-based)
        U = U.tocsr()[keepd][:, keepd].tocsc()
        latent = latent[keepd]
        obs = np.delete(obs, np.arange(n, 2 * n))
        size = int(keepd.sum())
    if np.any(nug == 0):                                                     # :173-193
        # rows/columns of observations with zero noise are removed; the latent variable they pin down
        # takes their place as an "observed" row
        Ucsc = U.tocsc()
        diag = Ucsc.diagonal()
        inds_U = np.where(np.isinf(diag))[0]                                 # :178
        cond_on = np.array([Ucsc.indices[Ucsc.indptr[j]:Ucsc.indptr[j + 1]].min() for j in inds_U])   # :179
        keep = np.ones(size, dtype=bool)
        keep[inds_U] = False
        U = Ucsc[keep][:, keep].tocsc()                                      # :180
        inds_z = np.where(np.isin(np.where(~latent)[0], inds_U))[0]          # :183 (0-based positions)
        inds_locs = np.where(np.isin(np.where(latent)[0], cond_on))[0]       # :184
        zero_nugg = dict(inds_U=inds_U + 1, inds_z=inds_z + 1, inds_locs=inds_locs + 1)
        latent = latent.copy()
        latent[cond_on] = False                                              # :188
        latent = latent[keep]                                                # :189
        rest = np.setdiff1d(np.arange(len(ord_)), inds_locs)
        ord_ = np.concatenate([ord_[rest], ord_[inds_locs]])                 # :190
        obs = np.concatenate([obs[rest], obs[inds_locs]])                    # :191
    return dict(U=U, latent=latent, ord=ord_, obs=obs, zero_nugg=zero_nugg, ord_pred=va["ord_pred"],
                ord_z=va["ord_z"], cond_yz=va["cond_yz"], ic0=va["ic0"], Lentries=Lent, Zentries=Zent)


# ---------------------------------------------------------------------------
# vecchia_likelihood — R/vecchia_likelihood.R
# ---------------------------------------------------------------------------
def _removeNAs(z, nuggets):
    """R/vecchia_likelihood.R:45-58."""
    z = np.asarray(z, dtype=np.float64).copy()
    nug = np.atleast_1d(np.asarray(nuggets, dtype=np.float64)).copy()
    isna = np.isnan(z)
    if isna.any():
        if nug.size < z.size:
            new = np.zeros(z.size)
            new[~isna] = nug if nug.size > 1 else nug[0]
            nug = new
        nug[isna] = np.var(z[~isna], ddof=1) * 1e8
        z[isna] = np.mean(z[~isna])
    return z, nug


def ichol_lower(Wrev):
    """R/ichol.R:16-59 -> src/ic0.cpp:43-64 through the native gpv_ic0: the lower IC(0) factor (CSR) of a sparse SPD
    matrix on its own pattern."""
    import scipy.sparse as sp
    Lw = sp.tril(Wrev, format="csr")
    Lw.sort_indices()
    ptrs = np.ascontiguousarray(Lw.indptr, dtype=np.int32)
    inds = np.ascontiguousarray(Lw.indices, dtype=np.int32)
    vals = np.ascontiguousarray(Lw.data, dtype=np.float64).copy()
    nbad = C.c_int64(0)
    L.check(L.lib().gpv_ic0(Lw.shape[0], L.iptr(ptrs), L.iptr(inds), L.dptr(vals), C.byref(nbad)), "gpv_ic0")
    return sp.csr_matrix((vals, inds, ptrs), shape=Lw.shape)


def _chol_rev(A, ic0):
    """t(chol(revMat(A))) as a sparse lower-triangular matrix (R/vecchia_prediction.R:74-81): SuperLU without pivoting in
    the natural order is L D L^T, the Cholesky factor is L sqrt(D); with ic0 the zero-fill factor of src/ic0.cpp."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    nA = A.shape[0]
    rev = np.arange(nA - 1, -1, -1)
    Arev = A.tocsr()[rev][:, rev].tocsc()
    if ic0:
        return ichol_lower(Arev)
    lu = spla.splu(Arev, permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    if not (np.array_equal(lu.perm_r, np.arange(nA)) and np.array_equal(lu.perm_c, np.arange(nA))):
        raise RuntimeError("U2V: the sparse factorisation pivoted (matrix not positive definite?)")
    d = lu.U.diagonal()
    return (lu.L @ sp.diags(np.sqrt(d))).tocsr()


def U2V(U_obj):
    """R/vecchia_prediction.R:62-111.  Host-side like the reference (CHOLMOD there; sequential sparse factorisation,
    SURVEY §8f-1).  Returns an object with `solve` = (V V^T)^{-1} and `U.diagonal()` = diag(V)^2:
      * general ordering, non-'zy': a SuperLU factor of W.rev = rev(U_y U_y^T) (or the IC(0) factor with ic0 = TRUE, :76-77);
      * 'zy': V.ord is the reversed latent block of U itself, no factorisation (:68-70);
      * obs-pred ordering: prediction columns of U_y unchanged, Cholesky of the observed block only (:85-107)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    U = U_obj["U"].tocsr()
    latent = U_obj["latent"]
    lat_idx = np.where(latent)[0]
    Uy = U[lat_idx, :]
    if U_obj.get("cond_yz") == "zy":                                        # :68-70
        B = Uy[:, lat_idx]
        r = np.arange(B.shape[0] - 1, -1, -1)
        return _TriFactor(B[r][:, r].tocsr())
    if U_obj.get("ord_pred", "general") != "obspred":                       # :72-83
        W = (Uy @ Uy.T).tocsc()
        nW = W.shape[0]
        rev = np.arange(nW - 1, -1, -1)
        Wrev = W[rev][:, rev].tocsc()
        if U_obj.get("ic0", False):                                         # :76-77
            return _TriFactor(ichol_lower(Wrev))
        return spla.splu(Wrev, permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    last_obs = int(np.max(np.where(~latent)[0])) + 1                        # :87
    lat_before = int(latent[:last_obs].sum())                               # :88
    lat_after = int(latent[last_obs:].sum())                                # :89
    Vpr = Uy[:, last_obs:]
    Vpr = Vpr[np.arange(Vpr.shape[0] - 1, -1, -1)][:, np.arange(Vpr.shape[1] - 1, -1, -1)]   # :92 revMat
    Uoo = Uy[:lat_before, :last_obs]                                        # :95
    Voor = _chol_rev((Uoo @ Uoo.T).tocsc(), U_obj.get("ic0", False))        # :96-100
    Vor = sp.vstack([sp.csr_matrix((lat_after, lat_before)), Voor])         # :103-104
    return _TriFactor(sp.hstack([Vpr, Vor]).tocsr())                        # :106


class _TriFactor:
    """V.ord = t(ichol(W.rev)) with the two members vecchia_likelihood_U / vecchia_mean_host use of a SuperLU object:
    `U.diagonal()` such that sum(log) = log det, and `solve` = (V V^T)^{-1}."""

    def __init__(self, V):
        self.V = V.tocsr()
        d = V.diagonal()

        class _D:
            def diagonal(self_inner):
                return d * d
        self.U = _D()

    def solve(self, b):
        import scipy.sparse.linalg as spla
        y = spla.spsolve_triangular(self.V, np.asarray(b, dtype=np.float64), lower=True)
        return spla.spsolve_triangular(self.V.T.tocsr(), y, lower=False)


def vecchia_mean_host(z, U_obj, lu=None):
    """R/vecchia_prediction.R:118-126 on the host: mu.ord = -W^{-1} z2 (ordered layout, one entry per latent variable).
    lu: the factor object of U2V(U_obj) when the caller has it already."""
    U = U_obj["U"].tocsr()
    latent = U_obj["latent"]
    zord = np.asarray(z, dtype=np.float64)[U_obj["ord_z"] - 1]
    z1 = U[np.where(~latent)[0], :].T @ zord
    z2 = U[np.where(latent)[0], :] @ z1
    if lu is None:
        lu = U2V(U_obj)
    return -(lu.solve(z2[::-1]))[::-1]


def split_mean(mu_ord, U_obj):
    """R/vecchia_prediction.R:134-139: ordered posterior mean -> (mu.obs, mu.pred) in the caller's order."""
    orig_order = np.argsort(U_obj["ord"], kind="stable")
    mu = np.asarray(mu_ord)[orig_order]
    obs_orig = np.asarray(U_obj["obs"], dtype=bool)[orig_order]
    return mu[obs_orig], mu[~obs_orig]


def vecchia_likelihood_U(z, U_obj):
    """R/vecchia_likelihood.R:63-99 on a host sparse U (denominator via U2V)."""
    U = U_obj["U"].tocsr()
    latent = U_obj["latent"]
    zord = np.asarray(z, dtype=np.float64)[U_obj["ord_z"] - 1]
    const = np.sum(~latent) * np.log(2 * np.pi)
    z1 = U[np.where(~latent)[0], :].T @ zord
    quadform_num = float(np.sum(z1 ** 2))
    logdet_num = -2.0 * float(np.sum(np.log(U.diagonal())))
    if latent.sum() == 0:
        logdet_denom = quadform_denom = 0.0
    else:
        z2 = U[np.where(latent)[0], :] @ z1
        lu = U2V(U_obj)
        logdet_denom = -float(np.sum(np.log(np.abs(lu.U.diagonal()))))      # -2 sum log diag(V) = -log det W
        y = lu.solve(z2[::-1])
        quadform_denom = float(z2[::-1] @ y)                                # |V^{-1} rev(z2)|^2 = z2' W^{-1} z2
    neg2loglik = logdet_num - logdet_denom + quadform_num - quadform_denom + const
    return -neg2loglik / 2


def vecchia_likelihood(z, vecchia_approx, covparms, nuggets, covmodel="matern", device=0):
    """R/vecchia_likelihood.R:14-27.  cond.yz='z' (and m=0) evaluates fully on the GPU with the
    fused epilogue; other conditioning modes build U on the GPU and finish the denominator
    on the host like the reference does (Matrix::chol)."""
    va = vecchia_approx
    if va["cond_yz"] == "zy":
        warnings.warn("cond.yz='zy' will produce a poor likelihood approximation. Use 'SGV' instead.")
    z_in = np.asarray(z, dtype=np.float64)
    nug_in = np.atleast_1d(np.asarray(nuggets, dtype=np.float64))
    if nug_in.size == 1 and not np.isnan(z_in.sum()):    # nothing for removeNAs to do (a NaN anywhere makes the sum NaN)
        z, nug = z_in, nug_in
    else:
        z, nug = _removeNAs(z, nuggets)
    n = int(np.sum(va["obs"]))
    plain = n == va["locsord"].shape[0]                  # every row of locsord observed: the fused device paths apply
    if plain and va["cond_yz"] in ("z", "false") and isinstance(covmodel, str) and not np.any(nug == 0):
        plan = _plan_for(va, device)
        plan.set_user_data(z, va["ord_z"])
        plan.eval(covmodel, covparms, _device_nuggets(va, nug), GPV_WANT_LOGLIK_Z)
        return loglik_z_from_sums(plan.sums(), n)
    if plain and va["cond_yz"] == "SGV" and isinstance(covmodel, str) and not np.any(nug == 0) and \
            _plan_for(va, device).ensure_posterior():                       # ic0 changes nothing: no fill
        # default mode: U, the numerator AND the posterior pass (U2V) on the GPU; SGV has no fill, so the
        # fixed-pattern factorisation equals the reference's Matrix::chol (R/vecchia_prediction.R:80).  (Refused only
        # when a conditioning set has more than 64 latent entries: the host route below.)
        plan = _plan_for(va, device)
        plan.set_user_data(z, va["ord_z"])
        plan.eval(covmodel, covparms, _device_nuggets(va, nug), GPV_WANT_DENOM)
        return loglik_from_sums(plan.sums(), n)
    if plain and va["cond_yz"] == "y" and isinstance(covmodel, str) and not np.any(nug == 0) and \
            not va.get("ic0", False):
        # latent conditioning throughout: W = U_y U_y^T fills in.  The device pass runs on the filled pattern when the fill is
        # bounded (symbolic factorisation on the host, once per plan); otherwise the host factorisation below, like CHOLMOD
        plan = _plan_for(va, device)
        if plan.has_posterior or plan.build_posterior_fill() is not None:
            plan.set_user_data(z, va["ord_z"])
            plan.eval(covmodel, covparms, _device_nuggets(va, nug), GPV_WANT_DENOM)
            return loglik_from_sums(plan.sums(), n)
    U_obj = createU(va, covparms, nug, covmodel, device=device)
    return vecchia_likelihood_U(z, U_obj)


def _scaledim_checked(name, va, covparms, covmodel):
    """covmodel='matern_scaledim' in the gradient-type functions: what the library refuses (gpv_plan_loglik_grad), said here
    before a plan is built: one range per coordinate, at most three coordinates, a closed-form smoothness."""
    if not (isinstance(covmodel, str) and covmodel == "matern_scaledim"):
        return
    dim = va["locsord"].shape[1]
    cp = np.atleast_1d(np.asarray(covparms, dtype=np.float64))
    if cp.size != dim + 2:
        raise ValueError(f"{name}: covmodel='matern_scaledim' takes variance, {dim} ranges and the smoothness, got {cp.size} covparms")
    if np.any(cp[1:1 + dim] <= 0) or np.any(np.isinf(cp[1:1 + dim])):
        raise ValueError(f"{name}: the ranges of covmodel='matern_scaledim' must be positive and finite")
    if dim > 3:
        raise ValueError(f"{name}: covmodel='matern_scaledim' has a gradient for at most three coordinates (the kernels carry "
                         "five parameter slots: variance, three ranges, nugget)")
    if float(cp[-1]) not in (0.5, 1.5, 2.5):
        raise ValueError(f"{name}: covmodel='matern_scaledim' needs smoothness in {{0.5, 1.5, 2.5}} (it is not differentiated)")


def _grad_plan(name, z, va, nuggets, covmodel, device):
    """The plan and the nugget of vecchia_likelihood_grad / vecchia_likelihood_fisher, after their common refusals."""
    if va["cond_yz"] not in ("z", "false"):
        raise ValueError(f"{name} needs cond_yz='z' (the gradient of the other modes goes through the "
                         "posterior factor)")
    if not isinstance(covmodel, str):
        raise ValueError(f"{name} needs a named covariance family ('matern', 'matern_scaledim' or 'esqe'), not a function or matrix")
    nug = np.atleast_1d(np.asarray(nuggets, dtype=np.float64))
    if nug.size != 1:
        raise ValueError(f"{name} takes one constant nugget")
    z = np.asarray(z, dtype=np.float64)
    if np.isnan(z.sum()):
        raise ValueError(f"{name} needs complete data (no NaN)")
    if int(np.sum(va["obs"])) != va["locsord"].shape[0]:
        raise ValueError(f"{name} does not take plans with prediction locations")
    plan = _plan_for(va, device)
    plan.set_user_data(z, va["ord_z"])
    return plan, float(nug[0])


def vecchia_likelihood_grad(z, vecchia_approx, covparms, nuggets, covmodel="matern", device=0, smoothness_grad=False):
    """(loglik, grad) of the cond.yz='z' Vecchia log-likelihood, both on the GPU in one pass over the conditioning sets
    (Plan.loglik_grad): grad = d loglik / d covparms, then d / d nugget; for 'matern' the smoothness (0.5, 1.5 or 2.5) is not
    differentiated and its entry is NaN.  Only what has an exact, cheap gradient is accepted: cond.yz = 'z' (or m = 0), one
    constant nugget > 0, complete data, no prediction locations, a named covariance family.  smoothness_grad=True: any Matern
    smoothness is accepted and its derivative returned (NaN only at exactly 0.5, 1.5, 2.5: Plan.loglik_grad).
    covmodel='matern_scaledim' (covparms = variance, one range per coordinate, smoothness in {0.5, 1.5, 2.5}; at most three
    coordinates): grad = d / d variance, d / d range_1 .. range_dim, NaN, d / d nugget."""
    _scaledim_checked("vecchia_likelihood_grad", vecchia_approx, covparms, covmodel)
    plan, nug = _grad_plan("vecchia_likelihood_grad", z, vecchia_approx, nuggets, covmodel, device)
    ll, grad, _ = plan.loglik_grad(covmodel, covparms, nug, smoothness_grad=smoothness_grad)
    return ll, grad


def _sgv_grad_checked(name, z, va, nuggets, covmodel):
    """The refusals of vecchia_likelihood_grad_sgv that need no device; returns (z, nugget)."""
    if va["cond_yz"] not in ("SGV", "z", "false"):
        raise ValueError(f"{name} needs cond_yz='SGV' (or 'z'), not {va['cond_yz']!r}")
    if not isinstance(covmodel, str) or covmodel not in ("matern", "esqe"):
        raise ValueError(f"{name} needs a named covariance family ('matern' or 'esqe')")
    nug = np.atleast_1d(np.asarray(nuggets, dtype=np.float64))
    if nug.size != 1:
        raise ValueError(f"{name} takes one constant nugget")
    z = np.asarray(z, dtype=np.float64)
    if np.isnan(z.sum()):
        raise ValueError(f"{name} needs complete data (no NaN)")
    if int(np.sum(va["obs"])) != va["locsord"].shape[0]:
        raise ValueError(f"{name} does not take plans with prediction locations")
    return z, float(nug[0])


def vecchia_likelihood_grad_sgv(z, vecchia_approx, covparms, nuggets, covmodel="matern", device=0):
    """(loglik, grad) of the Vecchia log-likelihood at the default conditioning cond.yz='SGV', on the GPU (Plan.loglik_grad_sgv):
    one evaluation with the posterior mean, the selected inverse of its factor and one pass over the conditioning sets.
    grad = d loglik / d covparms, then d / d nugget; for 'matern' the smoothness (0.5, 1.5 or 2.5) is not differentiated and its
    entry is NaN.  Accepts cond_yz 'SGV' (and 'z' / 'false', where it agrees with vecchia_likelihood_grad), one constant nugget
    > 0, complete data, no prediction locations, 'matern' or 'esqe'; ValueError otherwise, and when the device posterior
    structure is refused for the plan (a conditioning set with more than 64 latent entries)."""
    va = vecchia_approx
    z, nug = _sgv_grad_checked("vecchia_likelihood_grad_sgv", z, va, nuggets, covmodel)
    plan = _plan_for(va, device)
    if not plan.ensure_posterior():
        raise ValueError("vecchia_likelihood_grad_sgv: the device posterior structure is refused for this plan "
                         "(a conditioning set has more than 64 latent entries)")
    plan.set_user_data(z, va["ord_z"])
    ll, grad, _ = plan.loglik_grad_sgv(covmodel, covparms, nug)
    return ll, grad


def vecchia_likelihood_fisher(z, vecchia_approx, covparms, nuggets, covmodel="matern", device=0, smoothness_grad=False):
    """(loglik, grad, info): vecchia_likelihood_grad together with the expected Fisher information of the same likelihood
    (Plan.loglik_fisher), a symmetric matrix over {covparms, nugget} whose inverse at the estimate approximates the covariance of
    the estimator.  For 'matern' the row and column of the smoothness are NaN, unless smoothness_grad=True and the smoothness is
    none of 0.5, 1.5, 2.5.  Accepts what vecchia_likelihood_grad accepts."""
    _scaledim_checked("vecchia_likelihood_fisher", vecchia_approx, covparms, covmodel)
    plan, nug = _grad_plan("vecchia_likelihood_fisher", z, vecchia_approx, nuggets, covmodel, device)
    ll, grad, info, _ = plan.loglik_fisher(covmodel, covparms, nug, smoothness_grad=smoothness_grad)
    return ll, grad, info


def _rep_plan(name, Z, va, nuggets, covmodel, device):
    """The plan and the nugget of vecchia_likelihood_grad_replicates / _fisher_replicates, after the refusals of _grad_plan and
    _user_columns; Z (n x R, the caller's order) is uploaded only when it is not what the plan holds already."""
    if va["cond_yz"] not in ("z", "false"):
        raise ValueError(f"{name} needs cond_yz='z' (the gradient of the other modes goes through the "
                         "posterior factor)")
    if not isinstance(covmodel, str):
        raise ValueError(f"{name} needs a named covariance family ('matern', 'matern_scaledim' or 'esqe'), not a function or matrix")
    nug = np.atleast_1d(np.asarray(nuggets, dtype=np.float64))
    if nug.size != 1:
        raise ValueError(f"{name} takes one constant nugget")
    if int(np.sum(va["obs"])) != va["locsord"].shape[0]:
        raise ValueError(f"{name} does not take plans with prediction locations")
    Z = _user_columns(name, Z, va)
    plan = _plan_for(va, device)
    plan.set_user_replicates(Z, va["ord_z"])
    return plan, float(nug[0])


def vecchia_likelihood_grad_replicates(Z, vecchia_approx, covparms, nuggets, covmodel="matern", device=0,
                                       smoothness_grad=False):
    """(loglik_sum, grad) of R realisations over the same locations, the columns of Z (n x R, in the CALLER's order): the sum
    over the columns of vecchia_likelihood_grad, from ONE pass over the conditioning sets (Plan.loglik_replicates) -- the
    factorisation of a block does not depend on the data.  Accepts what vecchia_likelihood_grad accepts, with complete, finite
    columns."""
    _scaledim_checked("vecchia_likelihood_grad_replicates", vecchia_approx, covparms, covmodel)
    plan, nug = _rep_plan("vecchia_likelihood_grad_replicates", Z, vecchia_approx, nuggets, covmodel, device)
    ll, grad, _, _ = plan.loglik_replicates(covmodel, covparms, nug, fisher=False, smoothness_grad=smoothness_grad)
    return ll, grad


def vecchia_likelihood_fisher_replicates(Z, vecchia_approx, covparms, nuggets, covmodel="matern", device=0,
                                         smoothness_grad=False):
    """(loglik_sum, grad, info): vecchia_likelihood_grad_replicates together with the expected Fisher information of the R
    realisations, R times that of one column (vecchia_likelihood_fisher)."""
    _scaledim_checked("vecchia_likelihood_fisher_replicates", vecchia_approx, covparms, covmodel)
    plan, nug = _rep_plan("vecchia_likelihood_fisher_replicates", Z, vecchia_approx, nuggets, covmodel, device)
    ll, grad, info, _ = plan.loglik_replicates(covmodel, covparms, nug, smoothness_grad=smoothness_grad)
    return ll, grad, info


# ---------------------------------------------------------------------------
# whitening with the resident factor: GLS trend (profile likelihood), replicated data
# ---------------------------------------------------------------------------
def _whiten_plan(name, va, covparms, nuggets, covmodel, device):
    """The plan of vecchia_whiten / vecchia_profile_likelihood / vecchia_likelihood_replicates after their common refusals,
    evaluated with GPV_WANT_U at these parameters: the factor Plan.whiten reads is resident."""
    if va["cond_yz"] not in ("z", "false"):
        raise ValueError(f"{name} needs cond_yz='z' (the whitening of the other modes goes through the posterior factor)")
    if not isinstance(covmodel, str):
        raise ValueError(f"{name} needs a named covariance family ('matern', 'matern_scaledim' or 'esqe'), not a function or matrix")
    n = va["locsord"].shape[0]
    if int(np.sum(va["obs"])) != n:
        raise ValueError(f"{name} does not take plans with prediction locations")
    nug = np.atleast_1d(np.asarray(nuggets, dtype=np.float64))
    if nug.size not in (1, n):
        raise ValueError(f"{name}: nuggets must be one value or one per location")
    plan = _plan_for(va, device)
    plan.eval(covmodel, covparms, _device_nuggets(va, nug), GPV_WANT_U)
    return plan


def _user_columns(name, B, va):
    B = np.asarray(B, dtype=np.float64)
    if B.ndim == 1:
        B = B[:, None]
    if B.ndim != 2 or B.shape[0] != va["locsord"].shape[0]:
        raise ValueError(f"{name}: the columns must have one row per location")
    if not np.all(np.isfinite(B)):
        raise ValueError(f"{name} needs complete, finite columns (no NaN)")
    return B


def vecchia_whiten(B, vecchia_approx, covparms, nuggets, covmodel="matern", device=0):
    """Whitens the columns of B (n x c, or a vector), given in the CALLER's order of the locations, with the Vecchia factor at
    these parameters: one evaluation (GPV_WANT_U), then ceil(c / 16) Plan.whiten calls.  Returns (E, logdet): E (n x c) in the
    ORDERED row numbering of the approximation, E[k] the standardised conditional residual of ordered row k, so that
    E'E = B'(C + tau I)^-1 B under the approximation, and logdet = log det(C + tau I) under it."""
    va = vecchia_approx
    B = _user_columns("vecchia_whiten", B, va)
    plan = _whiten_plan("vecchia_whiten", va, covparms, nuggets, covmodel, device)
    Bord = B[va["ord_z"] - 1]
    E = np.empty(Bord.shape)
    logdet = np.nan
    for c0 in range(0, Bord.shape[1], WHITEN_MAX_COLS):
        _, logdet, _, Ec = plan.whiten(Bord[:, c0:c0 + WHITEN_MAX_COLS], want_E=True)
        E[:, c0:c0 + WHITEN_MAX_COLS] = Ec
    return E, logdet


def vecchia_unwhiten(E, vecchia_approx, covparms, nuggets, covmodel="matern", device=0):
    """The mirror of vecchia_whiten: colours the columns of E (n x c, or a vector), given in the ORDERED row numbering of the
    approximation (as vecchia_whiten returns them), with the Vecchia factor at these parameters: one evaluation (GPV_WANT_U),
    then ceil(c / 16) Plan.unwhiten calls.  Returns B (n x c) in the CALLER's order of the locations, so that
    vecchia_whiten(B, ...)[0] is E; standard normal columns become draws from the approximation of N(0, C + tau I).  All NaN
    when some block was not positive definite at these parameters."""
    va = vecchia_approx
    E = _user_columns("vecchia_unwhiten", E, va)
    plan = _whiten_plan("vecchia_unwhiten", va, covparms, nuggets, covmodel, device)
    Bord = np.empty(E.shape)
    for c0 in range(0, E.shape[1], WHITEN_MAX_COLS):
        Bord[:, c0:c0 + WHITEN_MAX_COLS], _ = plan.unwhiten(E[:, c0:c0 + WHITEN_MAX_COLS])
    B = np.empty(E.shape)
    B[va["ord_z"] - 1] = Bord
    return B


def vecchia_simulate(vecchia_approx, covparms, nuggets, covmodel="matern", nsim=1, seed=0, mean=None, device=0):
    """nsim draws from the Vecchia approximation of N(mean, C + tau I) at these parameters, an (n, nsim) array in the CALLER's
    order of the locations: one evaluation (GPV_WANT_U), then Plan.simulate, which colours normals made on the device (draw j is
    the colouring of draws_normals_host(seed, 0, n, j, 1), reproducible per seed and independent of nsim).  nuggets: one value
    or one per location (caller's order); mean: None, a scalar or one value per location (caller's order), added on the host.
    All NaN when some block was not positive definite at these parameters."""
    va = vecchia_approx
    n = va["locsord"].shape[0]
    if int(nsim) != nsim or int(nsim) < 1:
        raise ValueError("vecchia_simulate: nsim must be an integer >= 1")
    mu = None
    if mean is not None:
        mu = np.asarray(mean, dtype=np.float64)
        if mu.ndim > 1 or (mu.ndim == 1 and mu.size != n):
            raise ValueError("vecchia_simulate: mean must be a scalar or one value per location")
    plan = _whiten_plan("vecchia_simulate", va, covparms, nuggets, covmodel, device)
    Zord, _ = plan.simulate(seed, int(nsim))
    Z = np.empty(Zord.shape)
    Z[va["ord_z"] - 1] = Zord
    if mu is not None:
        Z += mu if mu.ndim == 0 else mu[:, None]
    return Z


def vecchia_precision_multiply(B, vecchia_approx, covparms, nuggets, covmodel="matern", device=0):
    """Q B and diag Q for the precision matrix Q = (C + tau I)^-1 of the data vector under the Vecchia approximation at these
    parameters, everything in the CALLER's order of the locations: one evaluation (GPV_WANT_U), then ceil(c / 16)
    Plan.precision calls.  B: n x c, or a vector.  Returns (QB (n x c), qdiag (n,)); all NaN when some block was not positive
    definite at these parameters."""
    va = vecchia_approx
    B = _user_columns("vecchia_precision_multiply", B, va)
    plan = _whiten_plan("vecchia_precision_multiply", va, covparms, nuggets, covmodel, device)
    o = va["ord_z"] - 1
    Bord = B[o]
    Rord = np.empty(Bord.shape)
    qord = None
    for c0 in range(0, Bord.shape[1], WHITEN_MAX_COLS):
        Rord[:, c0:c0 + WHITEN_MAX_COLS], q, _ = plan.precision(Bord[:, c0:c0 + WHITEN_MAX_COLS], want_diag=c0 == 0)
        qord = q if c0 == 0 else qord
    R, qdiag = np.empty(Bord.shape), np.empty(Bord.shape[0])
    R[o] = Rord
    qdiag[o] = qord
    return R, qdiag


def loo_summary(scores, n):
    """The per-column summary of Plan.loo's score sums (ncols, 6) over n locations: rmse, mae, log_score (mean log predictive
    density), crps (mean), coverage95, mean_sq_std_resid."""
    s = np.atleast_2d(np.asarray(scores, dtype=np.float64))
    return dict(rmse=np.sqrt(s[:, 0] / n), mae=s[:, 1] / n, log_score=-0.5 * (np.log(2.0 * np.pi) + (s[:, 3] + s[:, 2]) / n),
                crps=s[:, 4] / n, coverage95=s[:, 5] / n, mean_sq_std_resid=s[:, 2] / n)


def vecchia_loo(z, vecchia_approx, covparms, nuggets, covmodel="matern", mean=None, device=0):
    """Leave-one-out cross-validation of the data under the Vecchia approximation of N(mean, C + tau I) at these parameters,
    without refitting: one evaluation (GPV_WANT_U), then ceil(R / 16) Plan.loo calls.  z: a vector or n x R (R realisations),
    in the CALLER's order of the locations; mean: None, a scalar or one value per location, subtracted before and added back.
    Returns a dict, everything in the caller's order: mean (n x R: E[z_i | z_-i]), var (n,: Var[z_i | z_-i], the same for every
    column), resid_std (n x R), and per column rmse, mae, log_score (mean log predictive density), crps (mean), coverage95,
    mean_sq_std_resid (arrays of length R).  All NaN when some block was not positive definite at these parameters."""
    va = vecchia_approx
    Z = _user_columns("vecchia_loo", z, va)
    n, R = Z.shape
    mu = None
    if mean is not None:
        mu = np.asarray(mean, dtype=np.float64)
        if mu.ndim > 1 or (mu.ndim == 1 and mu.size != n):
            raise ValueError("vecchia_loo: mean must be a scalar or one value per location")
        mu = mu if mu.ndim == 0 else mu[:, None]
        Z = Z - mu
    plan = _whiten_plan("vecchia_loo", va, covparms, nuggets, covmodel, device)
    o = va["ord_z"] - 1
    Zord = Z[o]
    Mord, scores, vord = np.empty(Zord.shape), np.empty((R, LOO_NSCORES)), None
    for c0 in range(0, R, WHITEN_MAX_COLS):
        Mord[:, c0:c0 + WHITEN_MAX_COLS], v, scores[c0:c0 + WHITEN_MAX_COLS], _ = plan.loo(Zord[:, c0:c0 + WHITEN_MAX_COLS],
                                                                                           want_var=c0 == 0)
        vord = v if c0 == 0 else vord
    M, var = np.empty(Zord.shape), np.empty(n)
    M[o] = Mord
    var[o] = vord
    out = dict(mean=M if mu is None else M + mu, var=var, resid_std=(Z - M) / np.sqrt(var)[:, None])
    out.update(loo_summary(scores, n))
    return out


def spatial_blocks(locs, max_size=BLOCKCV_MAX_BLOCK):
    """Spatial blocks for vecchia_block_cv (host numpy, deterministic): recursive bisection of the locations (n x d) along
    cycling coordinates, each cell split at the middle of a STABLE sort of its points on the coordinate (by rank, not by value:
    duplicated points cannot stall it), until every cell holds <= max_size points.  Returns integer labels 0 .. n_cells - 1 in
    the caller's order, cells numbered left first."""
    locs = np.asarray(locs, dtype=np.float64)
    if locs.ndim == 1:
        locs = locs[:, None]
    if locs.ndim != 2 or locs.shape[0] < 1 or locs.shape[1] < 1:
        raise ValueError("spatial_blocks: locs must be n x d with n >= 1")
    if int(max_size) != max_size or int(max_size) < 1:
        raise ValueError("spatial_blocks: max_size must be an integer >= 1")
    n, d = locs.shape
    labels = np.empty(n, dtype=np.int64)
    stack, nxt = [(np.arange(n), 0)], 0
    while stack:
        idx, axis = stack.pop()
        if idx.size <= max_size:
            labels[idx] = nxt
            nxt += 1
            continue
        srt = idx[np.argsort(locs[idx, axis], kind="stable")]
        half = (idx.size + 1) // 2
        stack.append((np.sort(srt[half:]), (axis + 1) % d))            # (popped second: the left half is numbered first)
        stack.append((np.sort(srt[:half]), (axis + 1) % d))
    return labels


def block_cv_summary(scores, n_heldout):
    """The per-column summary of Plan.block_cv's score sums (ncols, 8) over n_heldout held-out locations: the keys of
    loo_summary (with the block predictive means and variances), and joint_log_score, the joint log predictive density of all
    blocks per held-out location."""
    s = np.atleast_2d(np.asarray(scores, dtype=np.float64))
    out = loo_summary(s[:, :LOO_NSCORES], n_heldout)
    out["joint_log_score"] = -0.5 * (np.log(2.0 * np.pi) + (s[:, 7] + s[:, 6]) / n_heldout)
    return out


def _block_ids(name, blocks, locs, n):
    """labels in the caller's order (None: spatial_blocks of the locations; -1: keep) -> block ids 0 .. through np.unique"""
    if blocks is None:
        return spatial_blocks(locs).astype(np.int32)
    lab = np.asarray(blocks)
    if lab.ndim != 1 or lab.shape[0] != n or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"{name}: blocks must be one integer label per location (-1: never held out)")
    if np.any(lab < -1):
        raise ValueError(f"{name}: block labels are -1 (never held out) or >= 0")
    ids = np.full(n, -1, dtype=np.int32)
    held = lab >= 0
    if not held.any():
        raise ValueError(f"{name}: no location is held out")
    uniq, inv = np.unique(lab[held], return_inverse=True)
    if np.bincount(inv).max() > BLOCKCV_MAX_BLOCK:
        raise ValueError(f"{name}: a block has more than {BLOCKCV_MAX_BLOCK} members")
    ids[held] = inv.astype(np.int32)
    return ids


def vecchia_block_cv(z, vecchia_approx, covparms, nuggets, covmodel="matern", blocks=None, mean=None, device=0):
    """Leave-block-out cross-validation of the data under the Vecchia approximation of N(mean, C + tau I) at these parameters,
    without refitting: one evaluation (GPV_WANT_U), Plan.set_blocks, then ceil(R / 16) Plan.block_cv calls.  z: a vector or
    n x R (R realisations), in the CALLER's order of the locations; blocks: None (spatial_blocks of the locations: cells of at
    most 64 points) or integer labels in the caller's order, -1 = never held out, at most 64 locations to a label; mean: None, a
    scalar or one value per location, subtracted before and added back.  Returns a dict, everything in the caller's order and NaN
    where a location is not held out: mean (n x R: E[z_i | the data outside i's block]), var (n,), resid_std (n x R), per column
    the keys of block_cv_summary (arrays of length R), and n_blocks, n_heldout.  All NaN when some block of the approximation
    was not positive definite at these parameters."""
    va = vecchia_approx
    Z = _user_columns("vecchia_block_cv", z, va)
    n, R = Z.shape
    mu = None
    if mean is not None:
        mu = np.asarray(mean, dtype=np.float64)
        if mu.ndim > 1 or (mu.ndim == 1 and mu.size != n):
            raise ValueError("vecchia_block_cv: mean must be a scalar or one value per location")
        mu = mu if mu.ndim == 0 else mu[:, None]
        Z = Z - mu
    o = va["ord_z"] - 1
    locs = np.empty(va["locsord"].shape)
    locs[o] = va["locsord"]
    ids = _block_ids("vecchia_block_cv", blocks, locs, n)
    plan = _whiten_plan("vecchia_block_cv", va, covparms, nuggets, covmodel, device)
    n_blocks, n_heldout, _, _ = plan.set_blocks(ids[o])
    Zord = Z[o]
    Mord, scores, vord = np.empty(Zord.shape), np.empty((R, BLOCKCV_NSCORES)), None
    for c0 in range(0, R, WHITEN_MAX_COLS):
        Mord[:, c0:c0 + WHITEN_MAX_COLS], v, scores[c0:c0 + WHITEN_MAX_COLS], _, _ = plan.block_cv(Zord[:, c0:c0 + WHITEN_MAX_COLS],
                                                                                                  want_var=c0 == 0)
        vord = v if c0 == 0 else vord
    M, var = np.empty(Zord.shape), np.empty(n)
    M[o] = Mord
    var[o] = vord
    out = dict(mean=M if mu is None else M + mu, var=var, resid_std=(Z - M) / np.sqrt(var)[:, None])
    out.update(block_cv_summary(scores, n_heldout))
    out.update(n_blocks=n_blocks, n_heldout=n_heldout)
    return out


def _krige_inputs(name, z, va, locs_pred, nuggets, covmodel, m, mean, predict):
    """what vecchia_krige and vecchia_krige_groups check and prepare alike: (Z (n, R) with the trend off and the missing values
    zeroed, vector, eligible or None, nug, lp (n_p, dim), m, ordz)"""
    if va["cond_yz"] != "z":
        raise ValueError(f"{name} needs cond_yz='z' (the other modes predict through the posterior factor: vecchia_prediction)")
    n = va["locsord"].shape[0]
    if int(np.sum(va["obs"])) != n:
        raise ValueError(f"{name} does not take plans with prediction locations")
    if not isinstance(covmodel, str):
        raise ValueError(f"{name} needs a named covariance family ('matern', 'matern_scaledim' or 'esqe'), not a function or matrix")
    if predict not in ("y", "z"):
        raise ValueError(f"{name}: predict must be 'y' or 'z'")
    Z = np.array(z, dtype=np.float64)
    vector = Z.ndim == 1
    if vector:
        Z = Z[:, None]
    if Z.ndim != 2 or Z.shape[0] != n or not 1 <= Z.shape[1] <= KRIGE_MAX_COLS:
        raise ValueError(f"{name}: z must be (n,) or (n, R) with R <= {KRIGE_MAX_COLS}")
    if mean is not None:
        mu = np.asarray(mean, dtype=np.float64)
        Z = Z - (mu if mu.ndim == 0 else mu.reshape(n, -1))
    miss = np.isnan(Z)
    eligible = None
    if miss.any():
        if Z.shape[1] > 1:
            raise ValueError(f"{name}: missing values (NaN) are taken in a single column only")
        eligible = ~miss[:, 0]
        Z = np.where(miss, 0.0, Z)
    if not np.all(np.isfinite(Z)):
        raise ValueError(f"{name}: z must be finite (NaN marks a missing value)")
    nug = np.atleast_1d(np.asarray(nuggets, dtype=np.float64))
    if nug.size not in (1, n):
        raise ValueError(f"{name}: nuggets must be one value or one per location")
    lp = np.asarray(locs_pred, dtype=np.float64).reshape(-1, va["locsord"].shape[1])
    if m is None:
        m = va["U_prep"]["revNNarray"].shape[1] - 1
    ordz = va["ord_z"] - 1
    return Z, vector, eligible, nug, lp, int(m), ordz


def vecchia_krige(z, vecchia_approx, locs_pred, covparms, nuggets, covmodel="matern", m=None, mean=None, mean_pred=None,
                  predict="y", nugget_pred=None, scale=None, device=0):
    """Prediction at new locations under the cond.yz='z' Vecchia model, the one vecchia_likelihood scores and
    vecchia_estimate(method="L-BFGS-B" | "fisher") fits: every prediction location is ordered last and conditions on its m
    nearest observations, so its predictive distribution is local kriging, one independent solve per location on the GPU
    (Plan.krige), streamed in chunks: the size of the map is not bounded by device memory.
    z: (n,) or (n, R <= 16) in the CALLER's order; NaN entries of a single column are missing data and never enter a
    conditioning set (NaN in several columns is refused).  vecchia_approx: a cond_yz='z' specification without prediction
    locations; m=None takes its m.  mean / mean_pred: subtracted from z / added to the predictions (a scalar, or one value per
    location[, column]).  predict='y' returns the variance of the latent field, 'z' adds nugget_pred (a scalar or one value
    per prediction location).  scale: what vecchia_specify(scale=) was given ('matern_scaledim': the neighbours are searched
    on locs / scale).  Returns dict(mean_pred (n_p[, R]), var_pred (n_p,), n_failed); a location whose block is not positive
    definite (it coincides with an observation that has no nugget) is NaN."""
    va = vecchia_approx
    name = "vecchia_krige"
    Z, vector, eligible, nug, lp, m, ordz = _krige_inputs(name, z, va, locs_pred, nuggets, covmodel, m, mean, predict)
    n_p = lp.shape[0]
    plan = _plan_for(va, device)
    mu_p, var_p, n_failed = plan.krige(covmodel, covparms, nug if nug.size == 1 else nug[ordz], lp, int(m), Z_ord=Z[ordz],
                                       scale=scale, eligible_ord=None if eligible is None else eligible[ordz])
    if mean_pred is not None:
        mp = np.asarray(mean_pred, dtype=np.float64)
        mu_p = mu_p + (mp if mp.ndim == 0 else mp.reshape(n_p, -1))
    if predict == "z":
        if nugget_pred is None:
            raise ValueError(f"{name}: predict='z' needs nugget_pred")
        var_p = var_p + np.asarray(nugget_pred, dtype=np.float64)
    return dict(mean_pred=mu_p[:, 0] if vector else mu_p, var_pred=var_p, n_failed=n_failed)


_COND_SIM_NOISE_KEY = 0x9E3779B97F4A7C15              # added to the seed (mod 2^64): the key of the predict='z' noise


def vecchia_cond_sim(z, vecchia_approx, locs_pred, covparms, nuggets, covmodel="matern", m=None, nsim=1, seed=0, order="maxmin",
                     mean=None, mean_pred=None, predict="y", nugget_pred=None, scale=None, eps=None, device=0):
    """Spatially coherent conditional draws over a map under the cond.yz='z' Vecchia model (Plan.cond_sim): the prediction
    locations are ordered after all observations, in a sweep order, and each conditions on its m nearest points among the
    observations and the prediction locations before it (the reference's ordering.pred='obspred' with pred.cond='general',
    for a 'z' model).  One factor pass and one level-scheduled sweep per 16 draws on the GPU.
    z, vecchia_approx, m, mean, mean_pred, scale, nuggets and the missing values: as vecchia_krige.  order: "maxmin" (the exact
    max-min ordering of the prediction locations), "given", or a permutation of range(n_p) (position k of the sweep takes
    location order[k]); everything comes back in the CALLER's order.  nsim, seed: draws of the library's generator; eps: the
    caller's (n_p, nsim) standard normals instead, row i for location i.  predict='z' adds independent N(0, nugget_pred) noise
    to the draws, from the same generator under a key of its own.
    Returns dict(mean (n_p[, R]), draws (n_p, nsim) with one data column, else dev (n_p, nsim): draw (c, s) = mean[:, c] +
    dev[:, s]; sd_cond (n_p,): the conditional standard deviation given the neighbours, NOT the marginal one; order (the sweep
    order, 0-based), n_levels, n_failed).  A location that coincides with an earlier one of the sweep, or with an observation
    that has no nugget, fails: it and every location that depends on it are NaN."""
    va = vecchia_approx
    name = "vecchia_cond_sim"
    Z, vector, eligible, nug, lp, m, ordz = _krige_inputs(name, z, va, locs_pred, nuggets, covmodel, m, mean, predict)
    n_p = lp.shape[0]
    if isinstance(order, str):
        if order not in ("maxmin", "given"):
            raise ValueError(f"{name}: order must be 'maxmin', 'given' or a permutation")
        o = (S.order_maxmin_exact(lp) - 1) if (order == "maxmin" and n_p > 1) else np.arange(n_p, dtype=np.int64)
    else:
        o = np.asarray(order, dtype=np.int64).reshape(-1)
        if o.size != n_p or not np.array_equal(np.sort(o), np.arange(n_p)):
            raise ValueError(f"{name}: order must be a permutation of range(n_p)")
    E = None
    if eps is not None:
        E = np.asarray(eps, dtype=np.float64).reshape(n_p, -1)[o]
        nsim = E.shape[1]
    nsim = int(nsim)
    if predict == "z" and nugget_pred is None:
        raise ValueError(f"{name}: predict='z' needs nugget_pred")
    plan = _plan_for(va, device)
    r = plan.cond_sim(covmodel, covparms, nug if nug.size == 1 else nug[ordz], lp[o], int(m), Z_ord=Z[ordz], scale=scale,
                      eligible_ord=None if eligible is None else eligible[ordz], E=E, seed=seed, nsim=nsim)
    mu_p, dev, sd = np.empty_like(r["mean"]), np.empty_like(r["dev"]), np.empty(n_p)
    mu_p[o], dev[o], sd[o] = r["mean"], r["dev"], r["sd"]
    if mean_pred is not None:
        mp = np.asarray(mean_pred, dtype=np.float64)
        mu_p = mu_p + (mp if mp.ndim == 0 else mp.reshape(n_p, -1))
    if predict == "z" and nsim > 0:
        from .lincomb import draws_normals_host
        noise = draws_normals_host((int(seed) + _COND_SIM_NOISE_KEY) % (1 << 64), 0, n_p, 0, nsim).T
        dev = dev + np.sqrt(np.broadcast_to(np.asarray(nugget_pred, dtype=np.float64), (n_p,)))[:, None] * noise
    out = dict(mean=mu_p[:, 0] if vector else mu_p, sd_cond=sd, order=o, n_levels=r["n_levels"], n_failed=r["n_failed"])
    if Z.shape[1] == 1:
        out["draws"] = mu_p[:, :1] + dev
    else:
        out["dev"] = dev
    return out


def cond_sim_regions(regions, weights, n_p, name="vecchia_cond_sim_summary"):
    """The regions of vecchia_cond_sim_summary as lists: (members: one int64 index array per region, in the caller's numbering and
    in the order given; wts: one float64 array per region; region_ids).  regions: None (one region of every location), one
    integer label per location (-1: in none; the regions are the distinct labels, ascending = region_ids), or a list of index
    arrays (region_ids = 0, 1, ..).  weights: None (1), one number per location, or for the list form a list of arrays, one
    number per member.  Raises ValueError for anything else; touches no device."""
    n_p = int(n_p)
    wloc = None
    per_member = False
    if weights is not None:
        if isinstance(weights, (list, tuple)) and len(weights) and not np.isscalar(weights[0]):
            per_member = True
        else:
            wloc = np.asarray(weights, dtype=np.float64).reshape(-1)
            if wloc.size != n_p:
                raise ValueError(f"{name}: weights must hold one number per prediction location")
            if not np.all(np.isfinite(wloc)):
                raise ValueError(f"{name}: weights must be finite")
    if regions is None:
        members, ids = [np.arange(n_p, dtype=np.int64)], np.zeros(1, dtype=np.int64)
    elif isinstance(regions, np.ndarray) or (len(regions) == n_p and all(np.isscalar(r) for r in regions)):
        lab = np.asarray(regions)
        if lab.ndim != 1 or lab.size != n_p or lab.dtype.kind not in "iu":
            raise ValueError(f"{name}: region labels must be one integer per prediction location")
        lab = lab.astype(np.int64)
        if (lab < -1).any():
            raise ValueError(f"{name}: a region label is a number >= 0, or -1 for a location in no region")
        ids = np.unique(lab[lab >= 0])
        order = np.argsort(lab, kind="stable")
        first = np.searchsorted(lab[order], ids, side="left")
        last = np.searchsorted(lab[order], ids, side="right")
        members = [order[a:b].astype(np.int64) for a, b in zip(first, last)]
    else:
        members = []
        for r in regions:
            idx = np.asarray(r)
            if idx.size and idx.dtype.kind not in "iu":
                raise ValueError(f"{name}: a region is an array of location indices")
            idx = idx.astype(np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= n_p):
                raise ValueError(f"{name}: a region names a location outside range(n_p)")
            members.append(idx)
        ids = np.arange(len(members), dtype=np.int64)
    if per_member:
        if regions is None or len(weights) != len(members) or isinstance(regions, np.ndarray):
            raise ValueError(f"{name}: a list of weights goes with a list of regions, one array per region")
        wts = [np.asarray(w, dtype=np.float64).reshape(-1) for w in weights]
        if any(w.size != idx.size for w, idx in zip(wts, members)):
            raise ValueError(f"{name}: weights[r] must hold one number per member of region r")
        if not all(np.all(np.isfinite(w)) for w in wts):
            raise ValueError(f"{name}: weights must be finite")
    else:
        wts = [np.ones(idx.size) if wloc is None else wloc[idx] for idx in members]
    return members, wts, ids


def cond_sim_regions_csr(members, wts, pos):
    """CSR over sweep rows of regions given in the caller's numbering: pos[i] is the sweep row of location i; the members of a
    region are passed in ascending sweep row (a stable sort: equal rows keep their order)."""
    regptr = np.zeros(len(members) + 1, dtype=np.int64)
    idx, w = [], []
    for r, (mem, wt) in enumerate(zip(members, wts)):
        rows = pos[mem]
        k = np.argsort(rows, kind="stable")
        idx.append(rows[k])
        w.append(wt[k])
        regptr[r + 1] = regptr[r] + mem.size
    regidx = np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, dtype=np.int32)
    regw = np.concatenate(w).astype(np.float64) if w else np.zeros(0)
    return regptr, regidx, regw


def vecchia_cond_sim_summary(z, vecchia_approx, locs_pred, covparms, nuggets, covmodel="matern", m=None, nsim=100, seed=0, col0=0,
                             order="maxmin", mean=None, mean_pred=None, scale=None, link=None, thresholds=None, regions=None,
                             weights=None, device=0):
    """Monte-Carlo summaries of the conditional draws of vecchia_cond_sim(nsim=, seed=) over a map, folded on the GPU
    (Plan.cond_sim_summary): totals, areas above thresholds and extremes of regions per draw, and moments and exceedance
    probabilities per location, without the draws ever reaching the host; memory does not grow with nsim.
    z (one column), vecchia_approx, locs_pred, covparms, nuggets, covmodel, m, order, mean, mean_pred, scale and the missing
    values: as vecchia_cond_sim; the draws summarised are its draws col0 .. col0 + nsim - 1 under `seed`, nsim >= 2.
    link: None / 'identity' / 'exp' / 'logistic', the g of vecchia_posterior_summary; thresholds: up to 8 numbers on the LATENT
    scale, mean_pred included.  regions: None (one region of every location), an integer label per location (-1: in none;
    returned in ascending label order), or a list of index arrays (overlap allowed).  weights: None, or one number per location
    (cell areas; any sign), or with a list of regions a list of arrays.  Everything is in the CALLER's order.
    Returns dict(mean, mc_mean, mc_var (n_p,), exceed (nthr, n_p), sd_cond (n_p,); region_ids, region_total = sum w g(y),
    region_mean = total / weight, region_max, region_min (g of the extremes) (nreg, nsim); region_area = sum w [y > thr]
    (nthr, nreg, nsim); region_weight, region_count (nreg,): over the members whose mean is not NaN; order, n_levels,
    n_failed).  A failed location and those that depend on it are NaN per location and take no part in a region."""
    from .lincomb import _LINKS
    va = vecchia_approx
    name = "vecchia_cond_sim_summary"
    if link not in _LINKS:
        raise ValueError(f"{name}: link must be None, 'identity', 'exp' or 'logistic'")
    code, nsim, col0 = _LINKS[link], int(nsim), int(col0)
    if nsim < 2 or col0 < 0:
        raise ValueError(f"{name}: nsim must be at least 2 and col0 not negative")
    thr = np.asarray([] if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
    if thr.size > 8 or np.isnan(thr).any():
        raise ValueError(f"{name}: at most 8 thresholds, none of them NaN")
    if np.ndim(z) != 1 and not (np.ndim(z) == 2 and np.shape(z)[1] == 1):
        raise ValueError(f"{name}: z must be one column (the draws of several columns: vecchia_cond_sim)")
    Z, vector, eligible, nug, lp, m, ordz = _krige_inputs(name, z, va, locs_pred, nuggets, covmodel, m, mean, "y")
    n_p = lp.shape[0]
    members, wts, ids = cond_sim_regions(regions, weights, n_p, name)
    if isinstance(order, str):
        if order not in ("maxmin", "given"):
            raise ValueError(f"{name}: order must be 'maxmin', 'given' or a permutation")
        o = (S.order_maxmin_exact(lp) - 1) if (order == "maxmin" and n_p > 1) else np.arange(n_p, dtype=np.int64)
    else:
        o = np.asarray(order, dtype=np.int64).reshape(-1)
        if o.size != n_p or not np.array_equal(np.sort(o), np.arange(n_p)):
            raise ValueError(f"{name}: order must be a permutation of range(n_p)")
    pos = np.empty(n_p, dtype=np.int64)
    pos[o] = np.arange(n_p)
    off = None
    if mean_pred is not None:
        off = np.broadcast_to(np.asarray(mean_pred, dtype=np.float64).reshape(-1), (n_p,))[o]
    plan = _plan_for(va, device)
    r = plan.cond_sim_summary(covmodel, covparms, nug if nug.size == 1 else nug[ordz], lp[o], int(m), nsim, seed=seed, col0=col0,
                              Z_ord=Z[ordz, 0], scale=scale, eligible_ord=None if eligible is None else eligible[ordz], offset=off,
                              link=code, thresholds=thr, regions=cond_sim_regions_csr(members, wts, pos))
    out = {}
    for k_out, k_in in (("mean", "mean"), ("mc_mean", "mc_mean"), ("mc_var", "mc_var"), ("sd_cond", "sd")):
        a = np.empty(n_p)
        a[o] = r[k_in]
        out[k_out] = a
    ex = np.empty((thr.size, n_p))
    ex[:, o] = r["exceed"]
    g = [lambda y: y, np.exp, lambda y: 1.0 / (1.0 + np.exp(-y))][code]
    with np.errstate(divide="ignore", invalid="ignore"):
        rmean = r["reg_total"] / r["reg_weight"][:, None]
    out.update(exceed=ex, region_ids=ids, region_total=r["reg_total"], region_mean=rmean, region_max=g(r["reg_max"]),
               region_min=g(r["reg_min"]), region_area=r["reg_area"], region_weight=r["reg_weight"], region_count=r["reg_count"],
               order=o, n_levels=r["n_levels"], n_failed=r["n_failed"])
    return out


def vecchia_krige_groups(z, vecchia_approx, locs_pred, groups, covparms, nuggets, covmodel="matern", m=None, weights=None, mean=None,
                         mean_pred=None, predict="y", nugget_pred=None, scale=None, return_cov=False, device=0):
    """Joint prediction of groups of new locations under the cond.yz='z' Vecchia model: the mean of a raster cell, a plot or a
    footprint with its standard error (block kriging), a contrast between locations, the joint covariance of a few sites.  The
    members of a group are ordered last and condition on the m observations nearest to their coordinate-wise mean and on the
    members before them, so a group is one (m + g)-row solve on the GPU (Plan.krige_groups), m + g <= 64; the groups are streamed
    in chunks.  A group of one location is the prediction of vecchia_krige there.
    groups: one integer label per prediction location, in any order.  weights: None (1 / g: the group's average) or one number
    per prediction location, any sign (+1, -1: a contrast).  z, vecchia_approx, m, mean / mean_pred, predict / nugget_pred,
    scale and the refusals: as vecchia_krige.  Returns dict(mean_pred (n_p[, R]), var_pred (n_p,), group_ids (the distinct
    labels, ascending), group_mean (n_groups[, R]) = sum_i w_i mean_i, group_var (n_groups,) = w' Sigma w, n_failed), all in the
    caller's order of the locations, and with return_cov also group_cov: one symmetric g x g array per group, the joint
    predictive covariance of its members in the caller's order.  predict='z' adds nugget_pred to var_pred and to the diagonals
    of group_cov, and sum_i w_i^2 nugget_i to group_var.  Everything of a group that failed (a member on an observation that
    has no nugget) is NaN; n_failed counts groups."""
    va = vecchia_approx
    name = "vecchia_krige_groups"
    Z, vector, eligible, nug, lp, m, ordz = _krige_inputs(name, z, va, locs_pred, nuggets, covmodel, m, mean, predict)
    n_p = lp.shape[0]
    lab = np.asarray(groups)
    if lab.ndim != 1 or lab.shape[0] != n_p or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"{name}: groups must be one integer label per prediction location")
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.size != n_p or not np.all(np.isfinite(w)):
            raise ValueError(f"{name}: weights must be one finite number per prediction location")
    tau_p = None
    if predict == "z":
        if nugget_pred is None:
            raise ValueError(f"{name}: predict='z' needs nugget_pred")
        tau_p = np.broadcast_to(np.asarray(nugget_pred, dtype=np.float64), (n_p,))
    ids, inv = np.unique(lab, return_inverse=True)
    o = np.argsort(inv, kind="stable")                       # the members of a group together, in the caller's order
    size = np.bincount(inv, minlength=ids.size)
    gptr = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    if size.size and m + int(size.max()) > KRIGE_GROUPS_MAX_ROWS:
        raise ValueError(f"{name}: m + the size of a group must be <= {KRIGE_GROUPS_MAX_ROWS} (m = {m}, the largest group: {size.max()})")
    plan = _plan_for(va, device)
    mu_s, var_s, gmean, gvar, cov, n_failed = plan.krige_groups(
        covmodel, covparms, nug if nug.size == 1 else nug[ordz], lp[o], gptr, m, Z_ord=Z[ordz], weights=None if w is None else w[o],
        scale=scale, eligible_ord=None if eligible is None else eligible[ordz], want_cov=return_cov)
    mu_p, var_p = np.empty(mu_s.shape), np.empty(n_p)
    mu_p[o], var_p[o] = mu_s, var_s
    ws = np.repeat(1.0 / np.maximum(size, 1), size) if w is None else w[o]
    if mean_pred is not None:
        mp = np.asarray(mean_pred, dtype=np.float64)
        mp = np.broadcast_to(mp if mp.ndim == 0 else mp.reshape(n_p, -1), mu_p.shape)
        mu_p = mu_p + mp
        if ids.size:
            gmean = gmean + np.add.reduceat(ws[:, None] * mp[o], gptr[:-1], axis=0)
    if tau_p is not None:
        var_p = var_p + tau_p
        if ids.size:
            gvar = gvar + np.add.reduceat(ws * ws * tau_p[o], gptr[:-1])
    out = dict(mean_pred=mu_p[:, 0] if vector else mu_p, var_pred=var_p, group_ids=ids, group_mean=gmean[:, 0] if vector else gmean,
               group_var=gvar, n_failed=n_failed)
    if return_cov:
        covs, at = [], 0
        for k in range(ids.size):
            g = int(size[k])
            S = np.zeros((g, g))
            S[np.tril_indices(g)] = cov[at:at + g * (g + 1) // 2]
            S = S + np.tril(S, -1).T
            if tau_p is not None:
                S[np.diag_indices(g)] += tau_p[o[gptr[k]:gptr[k + 1]]]
            covs.append(S)
            at += g * (g + 1) // 2
        out["group_cov"] = covs
    return out


def profile_from_gram(G, logdet, n):
    """The Gaussian profile likelihood of a linear trend from the Gram matrix of the whitened columns [X | z] (pure host
    algebra): with A = X'QX = G[:q, :q], b = X'Qz = G[:q, q] and s = z'Qz = G[q, q] (Q the precision of the approximation),
    beta_hat = A^-1 b, beta_cov = A^-1, quadform = s - b'beta_hat, loglik = -1/2 logdet - 1/2 quadform - 1/2 n log 2 pi.
    ValueError when A is singular (collinear trend columns)."""
    G = np.asarray(G, dtype=np.float64)
    q = G.shape[0] - 1
    if G.ndim != 2 or G.shape[1] != q + 1 or q < 1:
        raise ValueError("G must be the square Gram matrix of at least one trend column and the data")
    Amat, b, s = G[:q, :q], G[:q, q], float(G[q, q])
    if not np.all(np.isfinite(G)):
        raise ValueError("the Gram matrix is not finite")
    try:
        np.linalg.cholesky(Amat)
        singular = np.linalg.cond(Amat) > 1.0 / np.finfo(float).eps
    except np.linalg.LinAlgError:
        singular = True
    if singular:
        raise ValueError("X'QX is singular: the trend columns are collinear")
    beta_cov = np.linalg.inv(Amat)
    beta_cov = 0.5 * (beta_cov + beta_cov.T)
    beta_hat = np.linalg.solve(Amat, b)
    quadform = s - float(b @ beta_hat)
    loglik = -0.5 * float(logdet) - 0.5 * quadform - 0.5 * n * np.log(2.0 * np.pi)
    return dict(beta_hat=beta_hat, beta_cov=beta_cov, quadform=quadform, logdet=float(logdet), loglik=loglik)


def vecchia_profile_likelihood(data, X, vecchia_approx, covparms, nuggets, covmodel="matern", device=0):
    """Generalised least squares with the trend coefficients profiled out: data = X beta + field, beta_hat(theta) =
    (X'QX)^-1 X'Qz under the Vecchia precision Q at (covparms, nuggets).  One evaluation (GPV_WANT_U) plus one Plan.whiten of
    [X | data]; returns the dict of profile_from_gram (beta_hat, beta_cov, quadform, logdet, loglik).  X: n x q, q + 1 <= 16.
    When some block is not positive definite at these parameters loglik is -Inf (as vecchia_likelihood) and the rest NaN."""
    va = vecchia_approx
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    if X.ndim != 2 or X.shape[1] < 1:
        raise ValueError("vecchia_profile_likelihood: X must be n x q with q >= 1")
    if X.shape[1] + 1 > WHITEN_MAX_COLS:
        raise ValueError(f"vecchia_profile_likelihood takes at most {WHITEN_MAX_COLS - 1} trend columns")
    data = np.asarray(data, dtype=np.float64).reshape(-1)
    if X.shape[0] != data.shape[0]:
        raise ValueError("vecchia_profile_likelihood: X and data must have one row per location")
    n, q = data.shape[0], X.shape[1]
    if n != va["locsord"].shape[0]:
        raise ValueError("vecchia_profile_likelihood: the columns must have one row per location")
    o = va["ord_z"] - 1
    Bord = np.empty((n, q + 1), order="F")               # [X | data] in ordered rows, gathered column by column: one pass each
    for j in range(q):
        np.take(X[:, j], o, out=Bord[:, j])
    np.take(data, o, out=Bord[:, q])
    if not np.isfinite(Bord).all():
        raise ValueError("vecchia_profile_likelihood needs complete, finite columns (no NaN)")
    plan = _whiten_plan("vecchia_profile_likelihood", va, covparms, nuggets, covmodel, device)
    G, logdet, n_failed = plan.whiten(Bord)
    if n_failed > 0:
        return dict(beta_hat=np.full(q, np.nan), beta_cov=np.full((q, q), np.nan), quadform=np.nan, logdet=np.nan,
                    loglik=-np.inf)
    return profile_from_gram(G, logdet, n)


def vecchia_likelihood_replicates(Z, vecchia_approx, covparms, nuggets, covmodel="matern", device=0):
    """The log-likelihoods of R realisations over the same locations (the columns of Z, n x R, in the CALLER's order) under one
    parameter value: ONE evaluation (the factor does not depend on the data), then ceil(R / 16) Plan.whiten calls.  Entry r
    equals vecchia_likelihood(Z[:, r], ...)."""
    va = vecchia_approx
    Z = _user_columns("vecchia_likelihood_replicates", Z, va)
    plan = _whiten_plan("vecchia_likelihood_replicates", va, covparms, nuggets, covmodel, device)
    Zord = Z[va["ord_z"] - 1]
    n, R = Zord.shape
    out = np.empty(R)
    for c0 in range(0, R, WHITEN_MAX_COLS):
        G, logdet, n_failed = plan.whiten(Zord[:, c0:c0 + WHITEN_MAX_COLS])
        if n_failed > 0:
            out[c0:c0 + WHITEN_MAX_COLS] = -np.inf
        else:
            out[c0:c0 + WHITEN_MAX_COLS] = -0.5 * logdet - 0.5 * np.diag(G) - 0.5 * n * np.log(2.0 * np.pi)
    return out
