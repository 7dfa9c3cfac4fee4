"""The inputs that tests/test_gpu_loglik_grad_sgv.py runs on the GPU and tests/test_sgv_grad_truth_host.py adjudicates on the CPU:
seeded uniform locations in the unit cube, tau = 0.1, range 0.25 sqrt(d / 2) (shorter for nu 1.5 and 2.5 in two dimensions: see
family), variance 1.3, ordering none, exact ordered nearest neighbours from oracle.r_side, the flags of vecchia_specify.  Computed once per process and shared read-only."""
import functools

import numpy as np

TAU = 0.1
N = 300
SHAPES = [(10, 2), (15, 2), (30, 2), (31, 2), (40, 3), (63, 2), (15, 9)]       # (m, d)
FAMILIES = ("nu0.5", "nu1.5", "nu2.5", "esqe")


def family(name, d):
    """Range 0.25 sqrt(d / 2), except the two smooth Matern families in two dimensions.  Under SGV the latent entries of a block
    carry no nugget, so a block of close latent points is as ill conditioned as the covariance itself, and at range 0.25 the
    float64 restatement strays from the long-double one by more than 1e-4 of the 1e-8 bar (worst column, of its scale, n = 300:
    nu 1.5 8.9e-12 at m = 10, 1.8e-12 at m = 63; nu 2.5 1.7e-9 at m = 10 and 15, 6.3e-11 at m = 30, 3.7e-11 at m = 63).  With the
    shorter ranges 0.06 (nu 1.5: 2.2e-13 at m = 10) and 0.03 (nu 2.5) every case stays below it
    (tests/test_sgv_grad_truth_host.py asserts each); d = 3 and d = 9 are benign as they are (1.9e-13, 4.4e-15 at nu 2.5)."""
    r = 0.25 * np.sqrt(d / 2)
    if d == 2 and name in ("nu1.5", "nu2.5"):
        r = 0.06 if name == "nu1.5" else 0.03
    return {"nu0.5": ("matern", [1.3, r, 0.5]), "nu1.5": ("matern", [1.3, r, 1.5]), "nu2.5": ("matern", [1.3, r, 2.5]),
            "esqe": ("esqe", [0.8, r, 0.5, 0.8 * r])}[name]


def family_at(name, d, n):
    """family(name, d) for a plan of n uniform locations: the range shrinks with the point spacing, n^(-1/d), so that the blocks
    of the conditioning sets are distributed as those of the n = N cases above (the covariance depends on distance / range
    alone).  At a fixed range the blocks of a larger plan hold ever closer latent points: with n = 6000 at range 0.25 in two
    dimensions the float64 restatement and the product already differ by 1.9e-7 of a column's scale.  The same distribution
    is not the same worst block: among more blocks the worst is worse (float64 against long double, worst column, nu 1.5, m = 10:
    2.2e-13 at n = 300, 1.1e-12 at n = 1200 with this rule), so no plan beyond n = N is adjudicated by the float64 truth."""
    cm, cp = family(name, d)
    s = (N / n) ** (1.0 / d)
    cp = list(cp)
    cp[1] *= s
    if cm == "esqe":
        cp[3] *= s
    return cm, cp


@functools.lru_cache(maxsize=None)
def setup(m, d, n=N, cond="SGV", seed=11):
    """(locs, z, vecchia.approx); needs no device"""
    import gpvecchia_amd as G
    from oracle import r_side as R
    rng = np.random.default_rng(seed)
    locs = rng.random((n, d))
    z = rng.standard_normal(n)
    NN = np.nan_to_num(R.findOrderedNN(locs, m), nan=0.0).astype(np.int32)
    va = G.vecchia_specify(locs, m, ordering="none", cond_yz=cond, NNarray=NN)
    for a in (locs, z, va["locsord"], va["U_prep"]["revNNarray"], va["U_prep"]["revCond"]):
        a.setflags(write=False)
    return locs, z, va


@functools.lru_cache(maxsize=None)
def truth(m, d, fam, n=N, cond="SGV", dtype="float64"):
    import _sgv_grad_truth as S
    locs, z, va = setup(m, d, n, cond)
    cm, cp = family(fam, d)
    t = S.sgv_truth(va["locsord"], va["U_prep"]["revNNarray"], va["U_prep"]["revCond"], z, cm, cp, TAU, np.dtype(dtype))
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t
