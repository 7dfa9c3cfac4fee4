"""The folds of gpv_plan_cond_sim_summary in NumPy, as the reference of tests/test_gpu_cond_sim_summary.py: given the latent draws
Y (nq, N) = (mean + offset) + dev, mu = mean + offset and the live mask (the mean is not NaN), the per-location moments and the
per-region, per-draw functionals of include/gpvecchia.h.  Sums are taken with math.fsum (exactly rounded) and come with the
magnitude a summation error scales with, sum |terms|; counts, areas of unit weights and extremes are exact in any order.
Checked against a literal loop by tests/test_cond_sim_summary_host.py.  No device."""
import math

import numpy as np

CHUNK_ROWS = 128          # gpv_csim_summary.h: kCsumChunkRows, the members of a region that one group folds
STEP_ROWS = 4             # kCsumStepRows: the members loaded together


def g(link):
    return [lambda y: y, np.exp, lambda y: 1.0 / (1.0 + np.exp(-y))][link]


def _fsum_cols(A):
    """column sums of A (k, N), exactly rounded"""
    return np.array([math.fsum(A[:, j]) for j in range(A.shape[1])]) if A.shape[0] else np.zeros(A.shape[1])


def location_truth(Y, mu, live, link, thr):
    """dict(mc_mean, mc_var, exceed (nthr, nq)); NaN where not live"""
    nq, N = Y.shape
    gl = g(link)
    with np.errstate(invalid="ignore", over="ignore"):
        D = gl(Y) - gl(mu)[:, None]
    mc_mean, mc_var = np.full(nq, np.nan), np.full(nq, np.nan)
    exceed = np.full((len(thr), nq), np.nan)
    for i in np.flatnonzero(live):
        s1 = math.fsum(D[i])
        s2 = math.fsum(D[i] * D[i])
        mc_mean[i] = gl(mu[i]) + s1 / N
        mc_var[i] = max((s2 - s1 * s1 / N) / (N - 1), 0.0)
        for t, v in enumerate(thr):
            exceed[t, i] = np.count_nonzero(Y[i] > v) / N
    return dict(mc_mean=mc_mean, mc_var=mc_var, exceed=exceed)


def region_truth(Y, live, link, thr, regptr, regidx, regw=None):
    """dict(total, total_mag, max, min (nreg, N), area, area_mag (nthr, nreg, N), weight, count (nreg,)): the functionals over the
    live members of every region; *_mag = sum |terms| of the sum beside it"""
    nq, N = Y.shape
    nreg, nthr = len(regptr) - 1, len(thr)
    gl = g(link)
    total, tmag = np.zeros((nreg, N)), np.zeros((nreg, N))
    mx, mn = np.full((nreg, N), np.nan), np.full((nreg, N), np.nan)
    area, amag = np.zeros((nthr, nreg, N)), np.zeros((nthr, nreg, N))
    weight, count = np.zeros(nreg), np.zeros(nreg, dtype=np.int64)
    for r in range(nreg):
        idx = np.asarray(regidx[regptr[r]:regptr[r + 1]], dtype=np.int64)
        w = np.ones(idx.size) if regw is None else np.asarray(regw[regptr[r]:regptr[r + 1]], dtype=np.float64)
        keep = live[idx]
        idx, w = idx[keep], w[keep]
        count[r] = idx.size
        weight[r] = math.fsum(w)
        if not idx.size:
            continue
        Yr = Y[idx]
        T = w[:, None] * gl(Yr)
        total[r], tmag[r] = _fsum_cols(T), _fsum_cols(np.abs(T))
        mx[r], mn[r] = Yr.max(axis=0), Yr.min(axis=0)
        for t, v in enumerate(thr):
            A = np.where(Yr > v, w[:, None], 0.0)
            area[t, r], amag[t, r] = _fsum_cols(A), _fsum_cols(np.abs(A))
    return dict(total=total, total_mag=tmag, max=mx, min=mn, area=area, area_mag=amag, weight=weight, count=count)


def csr(regions, weights=None):
    """(regptr, regidx, regw or None) of a list of index arrays (and of arrays of weights), in the order given"""
    regptr = np.zeros(len(regions) + 1, dtype=np.int64)
    regptr[1:] = np.cumsum([len(r) for r in regions])
    regidx = np.concatenate([np.asarray(r, dtype=np.int32) for r in regions]) if regions else np.zeros(0, dtype=np.int32)
    regw = None if weights is None else np.concatenate([np.asarray(w, dtype=np.float64) for w in weights])
    return regptr, regidx.astype(np.int32), regw
