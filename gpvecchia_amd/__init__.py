"""gpvecchia_amd — MI355X-native engine for GPvecchia's U_NZentries / Vecchia
log-likelihood path.  The arithmetic lives in libgpvecchia_hip.so (HIP, gfx950,
C ABI in include/gpvecchia.h); this package is the host-side mirror of the R API."""
from ._lib import (GPV_WANT_DENOM, GPV_WANT_LOGLIK_Z, GPV_WANT_MEAN, GPV_WANT_MEAN_B, GPV_WANT_NUMERATOR, GPV_WANT_U, GpvError,  # noqa: F401
                   device_count)
from .api import (Comm, EsqeFun, MaternFun, MultiPlan, Plan, ReplicaPlans, U2V, U_NZentries, U_NZentries_mat, createU, loglik_from_sums,  # noqa: F401
                  loglik_z_from_sums, numerator_from_sums, vecchia_likelihood, vecchia_likelihood_U, vecchia_likelihood_grad,
                  vecchia_likelihood_fisher, vecchia_specify, profile_from_gram, vecchia_likelihood_replicates,
                  vecchia_profile_likelihood, vecchia_whiten, vecchia_likelihood_grad_replicates,
                  vecchia_likelihood_fisher_replicates, vecchia_unwhiten, vecchia_simulate, vecchia_likelihood_grad_sgv,
                  vecchia_precision_multiply, vecchia_loo, loo_summary, spatial_blocks, block_cv_summary,
                  vecchia_block_cv, vecchia_krige, vecchia_krige_groups, vecchia_cond_sim,
                  vecchia_cond_sim_summary)

from .laplace import (calculate_posterior_VL, vecchia_laplace_likelihood,  # noqa: F401,E402
                      vecchia_laplace_likelihood_from_posterior, vecchia_laplace_prediction, vecchia_prediction)

from .lincomb import draws_normals_host, vecchia_lincomb, vecchia_posterior_sample, vecchia_posterior_summary, vecchia_selinv  # noqa: F401,E402

from .wrappers import vecchia_estimate, vecchia_pred  # noqa: F401,E402

__version__ = "0.1.0"
