from bayesianinferencedl_amd.bayesian_inference.laplace import (LowRankMetric, gauss_newton_map, misfit_jacobian,  # noqa: F401
                                                                pointwise_variance, reduced_value_grad_jac)
