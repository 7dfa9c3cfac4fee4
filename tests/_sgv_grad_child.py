"""Child process of tests/test_gpu_loglik_grad_sgv.py: one call of Plan.loglik_grad_sgv on the (m, d, family) case named on the
command line, under whatever environment the parent set (GPV_POST_TOP, GPV_NO_GRAPH: read when the library first builds a
posterior structure or replays a graph, so they need a fresh process); the result goes to the .npz file named last.

    python _sgv_grad_child.py m d family out.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main(m, d, fam, out):
    import gpvecchia_amd as G
    import _sgv_grad_cases as K
    locs, z, va = K.setup(int(m), int(d))
    cm, cp = K.family(fam, int(d))
    plan = G.Plan(va["locsord"], va["U_prep"]["revNNarray"], va["U_prep"]["revCond"])
    plan.set_data(z)
    plan.build_posterior()
    ll, grad, nfail, cols = plan.loglik_grad_sgv(cm, cp, K.TAU, col_terms=True)
    np.savez(out, ll=ll, grad=grad, nfail=nfail, cols=cols)


if __name__ == "__main__":
    main(*sys.argv[1:5])
