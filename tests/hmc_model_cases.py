"""NumPy statement of the two model-agnostic halves of a leapfrog step (finrom_hmc_drift / _kick, csrc/hmc_model.hip) and the case
builder for them, shared by tests/test_hmc_model_host.py (which checks the statement against hmc.run_chains) and
tests/test_gpu_hmc_model_kernels.py (which checks the kernels against it).  Imports without a GPU.

The statement restates include/finrom.h, not the kernels:
  * the position update is ONE fused multiply-add, k' = fma(eps, p, k): bit for bit (hmc_cases.fma: exact, one rounding);
  * theta = theta0 + A k' in np.longdouble, returned with its scale |theta0| + |A| |k'|;
  * the kick with a field-space gradient: d = k' - mean (one rounding), dUq = fma(c_lik / c_pri, g, d), P = fma(-(eps c_pri), dUq, P),
    both coefficients formed in double first: bit for bit; a chain with info != 0 gets dUq = 0 and keeps its momentum;
  * the kick with (g_theta, A): g = sum_p g_theta[c, p] A[p, i] in np.longdouble with its scale sum_p |g_theta[c, p] A[p, i]|.
A "case" is a dict with the fields of finrom_hmc_state as NumPy arrays, as hmc_cases.DeviceState takes it."""
import numpy as np

import hmc_cases as H

LD = H.LD
C_LIK = 1.0 / 0.05 ** 2


def ref_drift(k, p, eps, A=None, theta0=None):
    """-> (k' [C, n] float64 bit for bit, theta [C, P] longdouble or None, theta's scale [C, P] or None)."""
    kq = H.fma(eps, p, k)
    if A is None:
        return kq, None, None
    t0 = np.zeros(A.shape[0]) if theta0 is None else np.asarray(theta0, dtype=np.float64)
    with np.errstate(all="ignore"):
        theta = t0.astype(LD) + kq.astype(LD) @ A.astype(LD).T
        scale = np.abs(t0) + np.abs(kq) @ np.abs(A).T
    return kq, theta, scale


def map_gradient(g_theta, A):
    """-> (g [C, n] longdouble = g_theta A, scale [C, n] = sum_p |g_theta[c, p] A[p, i]|)."""
    return g_theta.astype(LD) @ A.astype(LD), np.abs(g_theta) @ np.abs(A)


def ref_kick(kq, mean, P, info, eps, c_lik, c_pri, g):
    """The momentum update behind a gradient g [C, n] (float64) at kq -> (dUq, P) bit for bit."""
    coef, ec = c_lik / c_pri, eps * c_pri
    flagged = (np.asarray(info) != 0)[:, None]
    with np.errstate(all="ignore"):
        d = kq - mean
    du = H.fma(coef, g, d)
    return np.where(flagged, 0.0, du), np.where(flagged, P, H.fma(-ec, du, P))


def kick_bounds(P_map, scale_g, dU_ref, P_ref, eps, c_lik, c_pri):
    """The allowances of a kick with (g_theta, A) against the statement evaluated at the longdouble gradient: the gradient's chain of
    P fused multiply-adds within (P + 1) 2^-53 of its scale; dUq inherits that times |c_lik / c_pri| and is rounded once; the momentum
    inherits dUq's whole allowance times eps c_pri and is rounded once.  -> (tol_g, tol_dU, tol_P)."""
    tol_g = (P_map + 1) * H.U53 * scale_g
    tol_dU = abs(c_lik / c_pri) * tol_g + H.U53 * np.abs(dU_ref)
    tol_P = abs(eps * c_pri) * tol_dU + H.U53 * np.abs(P_ref)
    return tol_g, tol_dU, tol_P


def step_case(n, C, step, seed=0, flags=()):
    """Random state in the middle of a trajectory, before leapfrog step `step`: the position k in Kq[step & 1], the other position
    buffer NaN (the drift's output), dUq NaN (the kick's output), mean != 0, c_pri != 1 (hmc_cases' constants), everything else
    filled, to be found unchanged.  flags: (chain, info value) pairs."""
    rng = np.random.default_rng([n, C, step, seed, 7])
    g = rng.standard_normal
    s = dict(C=C, n=n, eps=H.EPS, c_lik=C_LIK, c_pri=H.C_PRI, mean=1.0 + 0.1 * g((C, n)), K=1.0 + 0.3 * g((C, n)), U=50.0 * np.abs(g(C)),
             dU=3.0 * g((C, n)), Kq0=np.full((C, n), np.nan), Kq1=np.full((C, n), np.nan), P=g((C, n)), dUq=np.full((C, n), np.nan),
             H0=50.0 * np.abs(g(C)), P_block=g((H.B_BLOCK, C, n)), lu_block=-np.abs(g((H.B_BLOCK, C))), jt=1, pt=4,
             accept=10 + 3 * np.arange(C, dtype=np.int64), trace=g((H.TRACE_ROWS, C, n)), loss=np.abs(g(C)), info=np.zeros(C, np.int32))
    s["Kq%d" % (step & 1)] = 1.0 + 0.3 * g((C, n))
    for c, v in flags:
        s["info"][c] = v
    return s


def map_case(n, C, P, seed=0):
    """(A [P, n], theta0 [P], g_theta [C, P], grad [C, n]): a map with rows of mixed sign and size, gradients of the size the chains see."""
    rng = np.random.default_rng([n, C, P, seed, 8])
    A = rng.standard_normal((P, n)) * 10.0 ** rng.uniform(-2, 1, (P, 1))
    return A, rng.uniform(0.5, 1.5, P), 1e-2 * rng.standard_normal((C, P)), 1e-2 * rng.standard_normal((C, n))


class Quadratic:
    """The synthetic model of the host test: loss(k) = |B A k - d|^2 / 2 with A [9, n], B [9, 9] random -- a model that sees the field
    only through theta = A k, as the reduced model does: g_theta = B^T (B theta - d), grad = A^T g_theta."""

    def __init__(self, n, seed=5):
        rng = np.random.default_rng(seed)
        self.A, self.B, self.d = rng.standard_normal((9, n)) / np.sqrt(n), rng.standard_normal((9, 9)), rng.standard_normal(9)

    def reduced(self, theta):
        r = theta @ self.B.T - self.d
        return 0.5 * np.einsum("co,co->c", r, r), r @ self.B

    def __call__(self, K):
        loss, g_theta = self.reduced(K @ self.A.T)
        return loss, g_theta @ self.A, np.zeros(len(K), bool)
