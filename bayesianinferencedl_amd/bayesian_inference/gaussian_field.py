"""Gaussian-random-field prior of the conductivity: host-side factor of the covariance, and the latent Gaussian-field prior of
the reference's HMC model (GaussianFieldPrior).

Call surface of the reference's ``make_cov_chol(V, kern_type, length)``
(bayesian_inference/gaussian_field.py:9-31).  This is one-time setup, kept on the host and
routed through the same SciPy entry points the reference uses (``pdist``/``squareform``
for the distances, ``scipy.linalg.cholesky`` for the UPPER factor): the Matern-5/2
covariance carries no nugget and is close to singular, so where the factorisation happens
matters for reproducing the reference's samples.  The per-sample work
``k = exp(0.5 * U^T xi)`` (deep_learning/generate_fin_dataset.py:87-88) runs on the GPU
(engine.FieldSampler -> finrom_sampler_draw).

``GaussianFieldPrior`` is the prior of the reference's PyMC3 model (bayesian_inference/pymc_func_bayes_inverse.py:191-201:
``pm.gp.Latent(cov_func=pm.gp.cov.Matern52(2, ls=1.2)).prior('nodal_vals', X=points)`` on the same dof coordinates).  PyMC3's
``Latent.prior`` is non-centred: the sampler moves ``v ~ N(0, I)`` and the field is ``k = mean + chol(K + 1e-6 I) v``.  The
chains of hmc.py sample that form with ``prior=``; the two triangular products per leapfrog step run on the GPU
(finrom_sampler_field / finrom_sampler_pullback, finrom_hmc_leapfrog_field)."""
import numpy as np
import scipy.linalg
from scipy.spatial.distance import pdist, squareform


def _matern(nu_sqrt, poly):
    def kern(d, length):
        t = nu_sqrt * d / length
        return poly(t) * np.exp(-t)
    return kern


_KERNELS = {
    # :17-21  squared exponential with a 1e-5 nugget
    'sq_exp': lambda d, length: np.exp(-(1 / (2 * length ** 2)) * d ** 2) + 1e-5 * np.eye(len(d)),
    # :22-25  Matern 5/2, no nugget
    'm52': _matern(np.sqrt(5), lambda t: 1 + t + t * t / 3),
    # :26-29  Matern 3/2 (the reference's fall-through branch)
    'm32': _matern(np.sqrt(3), lambda t: 1 + t),
}


def make_cov_chol(V, kern_type='m52', length=1.6):
    xy = V.tabulate_dof_coordinates().reshape((-1, 2))[V.dofmap().dofs(), :]
    kern = _KERNELS.get(kern_type, _KERNELS['m32'])
    from ..fem import deterministic_blas
    with deterministic_blas():           # one LAPACK thread: the same factor, bit for bit, in every rank of a multi-GPU run
        return scipy.linalg.cholesky(kern(squareform(pdist(xy)), length))


def _dof_points(V):
    return V.tabulate_dof_coordinates().reshape((-1, 2))[V.dofmap().dofs(), :]


class GaussianFieldPrior:
    """The latent Gaussian-field prior k = mean + U^T v, v ~ N(0, I), U the UPPER Cholesky factor of
    amplitude^2 Matern52(length) + jitter I on the dof coordinates of V (the points make_cov_chol uses).

    The defaults are the reference's ``Latent(Matern52(2, ls=1.2)).prior`` (zero mean function, PyMC3's 1e-6 jitter); ``mean``
    is a field [n] or a scalar (None: zero).  Host maps: field(v), pullback(g) (= U g: a field-space gradient as a gradient in v),
    whiten(k) (v of a field, e.g. to start chains at a MAP field).  device(): the factor on the GPU (engine.FieldSampler)."""

    def __init__(self, V, length=1.2, amplitude=1.0, jitter=1e-6, mean=None):
        xy = _dof_points(V)
        self.n = len(xy)
        self.length, self.amplitude, self.jitter = float(length), float(amplitude), float(jitter)
        cov = amplitude ** 2 * _KERNELS['m52'](squareform(pdist(xy)), length) + jitter * np.eye(self.n)
        from ..fem import deterministic_blas
        with deterministic_blas():       # the same factor, bit for bit, in every rank (as make_cov_chol)
            self.U = scipy.linalg.cholesky(cov)
        self.mean = np.zeros(self.n) if mean is None else np.broadcast_to(np.asarray(mean, dtype=np.float64), (self.n,)).copy()
        self._dev = None

    def field(self, v):
        """k = mean + U^T v, row-wise for a batch v [..., n]."""
        return self.mean + np.asarray(v, dtype=np.float64) @ self.U

    def pullback(self, g):
        """U g, row-wise: the gradient of a function of the field k as a gradient in v."""
        return np.asarray(g, dtype=np.float64) @ self.U.T

    def whiten(self, k):
        """v with field(v) = k (a triangular solve U^T v = k - mean), row-wise."""
        d = np.asarray(k, dtype=np.float64) - self.mean
        return scipy.linalg.solve_triangular(self.U, d.T, trans='T', lower=False).T

    def device(self):
        """The factor on the current GPU: engine.FieldSampler (field / pullback / draw), created once."""
        if self._dev is None:
            from ..engine import FieldSampler
            self._dev = FieldSampler(self.U)
        return self._dev
