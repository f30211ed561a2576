"""Laplace approximation at the MAP point in the whitened coordinates of the latent Gaussian-field prior, as the metric of the
HMC chains (hmc.py, metric=).

The reference's working sampler (bayesian_inference/inference.py:102-140,165) finds the MAP point, builds a low-rank Gauss-Newton
Hessian of the misfit there in prior-whitened coordinates by 30 randomized Hessian actions (60 PDE solves), and hands
prior^(1/2) (I - V_r D V_r^T) prior^(1/2) to NUTS as `scaling`.  Here the chains already move the whitened variable v
(k = mean + U^T v, potential phi(v) = misfit(k) / sigma^2 + |v|^2 / 2), and the Gauss-Newton Hessian of phi is

    M = I + G G^T,   G = U J^T / sigma   [n x n_obs],   J the Jacobian of the observables at the field,

whose rank is at most n_obs (9 or 40): ONE batched Jacobian call and the thin SVD of an n_obs x n matrix give it exactly,
G = V S Z^T, lambda = s^2, M = I + V diag(lambda) V^T.  The reference leaves 1 / sigma^2 out of its H-tilde (its misfit is not
divided by the noise variance there); here it is INCLUDED, so that M is the Hessian of the potential the chains integrate.
Every map is y = x + sum_j c_j V_j (V_j . x):

    M: c = lambda    M^-1: -lambda / (1 + lambda)    M^(1/2): sqrt(1 + lambda) - 1    M^(-1/2): 1 / sqrt(1 + lambda) - 1

On the device the maps are finrom_metric_apply (engine.MetricHandle) and, inside a fused proposal, finrom_hmc_begin_metric /
_leapfrog_field_metric / _end_metric."""
from __future__ import annotations

import numpy as np

OPS = ("M", "inv", "sqrt", "invsqrt")


def _coef(lam, op):
    """c_j of the map `op`, in forms without cancellation at small lambda (the library's, finrom_metric_create)."""
    s = np.sqrt(1.0 + lam)
    if op == "M":
        return lam
    if op == "inv":
        return -lam / (1.0 + lam)
    if op == "sqrt":
        return lam / (s + 1.0)
    if op == "invsqrt":
        return -lam / ((1.0 + lam) + s)
    raise ValueError(f"metric op {op!r} (one of {OPS})")


class LowRankMetric:
    """M = I + V diag(lam) V^T with the eigenvectors as the ROWS of Vt [rho, n] (orthonormal) and lam [rho] > 0; rho = 0 is the
    identity.  center: the point the metric was taken at (the whitened MAP), used by draw().
    Host maps: apply(x, op) row-wise for x [..., n]; draw(xi) = center + M^(-1/2) xi (a draw of the Laplace approximation
    N(center, M^-1) from standard normals xi); dense() = M.  device(): the metric on the GPU (engine.MetricHandle), created once."""

    def __init__(self, Vt, lam, center=None):
        self.Vt = np.ascontiguousarray(Vt, dtype=np.float64)
        self.lam = np.ascontiguousarray(lam, dtype=np.float64)
        if self.Vt.ndim != 2 or self.lam.shape != (self.Vt.shape[0],):
            raise ValueError("LowRankMetric: Vt [rho, n] and lam [rho]")
        if not (np.all(np.isfinite(self.lam)) and np.all(self.lam > 0)):
            raise ValueError("LowRankMetric: lam must be finite and positive")
        self.rho, self.n = self.Vt.shape
        self.center = None if center is None else np.array(center, dtype=np.float64).reshape(self.n)
        self._dev = None

    @classmethod
    def from_jacobian(cls, J, prior, sigma, rtol=1e-12, center=None):
        """The Gauss-Newton Hessian of misfit / sigma^2 + |v|^2 / 2 from the Jacobian J [n_obs, n] of the observables with respect
        to the FIELD: G^T = (U J^T)^T / sigma = prior.pullback(J) / sigma, thin SVD, lambda = s^2, eigenpairs with
        lambda_j > rtol * lambda_1 kept.  prior None: the chain's coordinates are the field's (G^T = J / sigma)."""
        J = np.atleast_2d(np.asarray(J, dtype=np.float64))
        Gt = (J if prior is None else prior.pullback(J)) / float(sigma)
        _, s, Vt = np.linalg.svd(Gt, full_matrices=False)
        lam = s ** 2
        keep = lam > rtol * lam[0] if lam.size and lam[0] > 0 else np.zeros(lam.shape, bool)
        return cls(Vt[keep], lam[keep], center=center)

    def apply(self, x, op="M"):
        x = np.asarray(x, dtype=np.float64)
        if self.rho == 0:
            return x.copy()
        return x + ((x @ self.Vt.T) * _coef(self.lam, op)) @ self.Vt

    def draw(self, xi):
        y = self.apply(xi, "invsqrt")
        return y if self.center is None else self.center + y

    def dense(self):
        return np.eye(self.n) + (self.Vt.T * self.lam) @ self.Vt

    def device(self):
        if self._dev is None:
            from ..engine import MetricHandle
            self._dev = MetricHandle(self.Vt, self.lam)
        return self._dev


def misfit_jacobian(kind, k, *, solver=None, solver_r=None, surrogate=None, data=None):
    """J [n_obs, n]: the Jacobian of the model's observables with respect to the nodal field, at the field k [n].
    kind 'fom': the full model's, Fin.sensitivity_batch (solver).
    kind 'rom' / 'romml': the reduced model's (solver_r, an AffineROMFin), from ONE batched gradient call of n_obs + 1 rows at the
    same field with per-sample data d, d + e_1, ..., d + e_n_obs: the gradient of 1/2 |d - y(k)|^2 is affine in d, so
    J_i = g(d) - g(d + e_i).  This is the Jacobian the chains' own gradients use: for 'romml' the learned error enters through the
    network's vector-Jacobian product while the averaged basis functions psi stay frozen, as in the reference's grad_romml.
    (Row 0 of that batch is the value and gradient at the true data: gauss_newton_map uses it, reduced_value_grad_jac.)
    kind 'ml': the pure deep-learning surrogate's (surrogate, a dl_model.Surrogate), the same n_obs + 1 rows through
    Surrogate.misfit_grad_batch: J_i = g(d) - g(d + e_i) = vjp(e_i); data: d (default zeros; J does not depend on it in exact
    arithmetic)."""
    k = np.ascontiguousarray(k, dtype=np.float64).reshape(-1)
    if kind == "fom":
        if solver is None:
            raise ValueError("misfit_jacobian('fom') needs solver=")
        return np.asarray(solver.sensitivity_batch(k[None, :]))[0]
    if kind == "ml":
        if surrogate is None:
            raise ValueError("misfit_jacobian('ml') needs surrogate=")
        n_obs = surrogate.n_out
        d = np.zeros(n_obs) if data is None else np.asarray(data, dtype=np.float64).reshape(n_obs)
        D = np.vstack([d[None, :], d[None, :] + np.eye(n_obs)])
        g = np.asarray(surrogate.misfit_grad_batch(np.ascontiguousarray(np.broadcast_to(k, (n_obs + 1, k.size))), D)["grad"], dtype=np.float64)
        return g[0][None, :] - g[1:]
    if kind not in ("rom", "romml"):
        raise ValueError(f"misfit_jacobian: kind {kind!r} (one of 'fom', 'rom', 'romml', 'ml')")
    if solver_r is None:
        raise ValueError(f"misfit_jacobian({kind!r}) needs solver_r=")
    return _reduced_jacobian(kind, solver_r, k)[0]


def _reduced_jacobian(kind, solver_r, k, data=None):
    n_obs = solver_r.n_obs
    data = getattr(solver_r, "data", None) if data is None else data
    d = np.zeros(n_obs) if data is None else np.asarray(data, dtype=np.float64).reshape(n_obs)   # (J does not depend on d)
    D = np.vstack([d[None, :], d[None, :] + np.eye(n_obs)])
    K = np.ascontiguousarray(np.broadcast_to(k, (n_obs + 1, k.size)))
    if kind == "romml":
        res = solver_r.grad_romml_batch(K, data=D)
        g, loss = np.asarray(res["grad"], dtype=np.float64), np.asarray(res["loss"], dtype=np.float64)
    else:
        res = solver_r.grad_reduced_batch(K, data=D)
        g, loss = np.asarray(res["g_theta"], dtype=np.float64) @ solver_r.dsigma_dk, np.asarray(res["J"], dtype=np.float64)
    info = np.asarray(res["info"])
    return g[0][None, :] - g[1:], float(loss[0]), g[0].copy(), int(info[0])


def reduced_value_grad_jac(solver_r, kind="romml"):
    """The callable gauss_newton_map takes, for the reduced model ('rom' or 'romml') of an AffineROMFin with its data set."""
    def f(K, jac=False):
        K = np.atleast_2d(np.asarray(K, dtype=np.float64))
        if jac:
            J, loss, grad, info = _reduced_jacobian(kind, solver_r, K[0])
            return dict(loss=np.array([loss]), grad=grad[None, :], info=np.array([info]), J=J)
        if kind == "romml":
            res = solver_r.grad_romml_batch(K)
            return dict(loss=np.asarray(res["loss"]), grad=np.asarray(res["grad"]), info=np.asarray(res["info"]))
        res = solver_r.grad_reduced_batch(K)
        return dict(loss=np.asarray(res["J"]), grad=np.asarray(res["g_theta"]) @ solver_r.dsigma_dk, info=np.asarray(res["info"]))
    return f


N_TRIALS = 8                                 # alpha = 1, 1/2, ..., 2^-7


def gauss_newton_map(value_grad_jac, prior, sigma, v0=None, maxiter=50, ftol=1e-9):
    """The MAP point of phi(v) = misfit(k) / sigma^2 + |v|^2 / 2, k = prior.field(v), by damped Gauss-Newton steps
    v <- v - alpha M(v)^-1 grad phi(v), M(v) the low-rank Gauss-Newton Hessian at v (LowRankMetric.from_jacobian).

    value_grad_jac(K [B, n], jac=False) -> dict(loss [B], grad [B, n] (field space), info [B]); with jac=True, B = 1 and the dict
    also holds J [n_obs, n], the Jacobian of the observables at K[0] (reduced_value_grad_jac: row 0 of the Jacobian batch is the
    value and gradient, so an iteration is TWO batched calls: the Jacobian batch, and the trial steps alpha = 1, 1/2, ..., 2^-7 at
    once).  The largest alpha whose trial lowers phi with info == 0 is taken.  Stops when the relative decrease falls below ftol,
    when no trial lowers phi, or after maxiter steps.
    Returns dict(v, k, phi: the history [steps + 1], metric: the LowRankMetric at the end point (center = v), grad_norm: the history
    of |grad phi|, steps)."""
    n = prior.n
    v = np.zeros(n) if v0 is None else np.array(v0, dtype=np.float64).reshape(n)
    c_lik = 1.0 / float(sigma) ** 2
    alphas = 0.5 ** np.arange(N_TRIALS)
    phis, gnorms, steps = [], [], 0
    done = False
    while True:
        res = value_grad_jac(prior.field(v)[None, :], jac=True)
        if int(np.asarray(res["info"])[0]) != 0:
            raise ValueError("gauss_newton_map: the model flags the current point (info != 0)")
        phi = c_lik * float(np.asarray(res["loss"])[0]) + 0.5 * float(v @ v)
        g = v + c_lik * prior.pullback(np.asarray(res["grad"], dtype=np.float64)[0])
        metric = LowRankMetric.from_jacobian(res["J"], prior, sigma, center=v)
        if not phis:
            phis.append(phi); gnorms.append(0.0)
        gnorms[-1] = float(np.linalg.norm(g))                        # (of the point the last step reached)
        if done or steps >= maxiter:
            break
        step = metric.apply(g, "inv")
        Vt = v[None, :] - alphas[:, None] * step[None, :]
        tr = value_grad_jac(prior.field(Vt), jac=False)
        with np.errstate(invalid="ignore", over="ignore"):
            phit = c_lik * np.asarray(tr["loss"], dtype=np.float64) + 0.5 * np.einsum("bn,bn->b", Vt, Vt)
            ok = (np.asarray(tr["info"]) == 0) & np.isfinite(phit) & (phit < phi)
        if not ok.any():
            break
        a = int(np.argmax(ok))                                       # the largest alpha that lowers phi
        v, steps = Vt[a].copy(), steps + 1
        done = phi - phit[a] <= ftol * abs(phi)
        # the history takes the trial's value; the gradient at the accepted point is row 0 of the next Jacobian batch (no extra call)
        phis.append(float(phit[a])); gnorms.append(0.0)
    return dict(v=v, k=prior.field(v), phi=np.array(phis), metric=metric, grad_norm=np.array(gnorms), steps=steps)


def pointwise_variance(prior, metric):
    """The pointwise variance of the FIELD under the Laplace approximation N(v*, M^-1): diag(U^T M^-1 U) =
    diag(U^T U) - sum_j d_j (U^T V_j)^2, d_j = lambda_j / (1 + lambda_j) -- the prior's variance less what the data removed."""
    var = np.einsum("ij,ij->j", prior.U, prior.U)
    if metric.rho:
        W = metric.Vt @ prior.U                                      # rows U^T V_j
        var = var - (metric.lam / (1.0 + metric.lam)) @ (W * W)
    return var
