"""The low-rank metric of the Laplace-preconditioned chains on the host (bayesian_inference/laplace.py, hmc.run_chains metric=):
its four maps against dense algebra, its construction from a Jacobian against a dense eigendecomposition, the chain under the
metric against the identity-mass chain in the coordinates where the target is isotropic, and the Gauss-Newton MAP iteration on
a linear model.  No GPU."""
import numpy as np
import pytest
import scipy.linalg

from bayesianinferencedl_amd.bayesian_inference import hmc
from bayesianinferencedl_amd.bayesian_inference.laplace import LowRankMetric, gauss_newton_map, pointwise_variance


class _Prior:
    """A latent Gaussian prior k = mean + U^T v with a random upper factor (GaussianFieldPrior's host maps without a mesh)."""

    def __init__(self, n, seed, mean=0.0):
        rng = np.random.default_rng(seed)
        self.n = n
        self.U = np.triu(rng.standard_normal((n, n))) / np.sqrt(n)
        self.U[np.diag_indices(n)] = np.abs(self.U[np.diag_indices(n)]) + 0.5
        self.mean = np.full(n, float(mean))

    def field(self, v):
        return self.mean + np.asarray(v) @ self.U

    def pullback(self, g):
        return np.asarray(g) @ self.U.T


def _metric(n, lam, seed):
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, len(lam))))[0]
    return LowRankMetric(Q.T, lam)


def test_the_four_maps_match_dense_algebra():
    """n = 60, rho = 7, lambda from 1e-2 to 1e4: M, M^-1, M^(1/2), M^(-1/2) against the dense matrices to 1e-12 relative;
    M^(1/2) twice is M and M M^-1 = I."""
    n, lam = 60, np.logspace(-2, 4, 7)
    m = _metric(n, lam, 0)
    M = m.dense()
    assert np.allclose(M, np.eye(n) + m.Vt.T @ np.diag(lam) @ m.Vt, rtol=1e-14, atol=1e-14)
    w, Q = np.linalg.eigh(M)
    dense = {"M": M, "inv": (Q / w) @ Q.T, "sqrt": (Q * np.sqrt(w)) @ Q.T, "invsqrt": (Q / np.sqrt(w)) @ Q.T}
    X = np.random.default_rng(1).standard_normal((5, n))
    for op, D in dense.items():
        want = X @ D.T
        assert np.linalg.norm(m.apply(X, op) - want) <= 1e-12 * np.linalg.norm(want), op
        assert np.linalg.norm(m.apply(X[0], op) - want[0]) <= 1e-12 * np.linalg.norm(want[0]), op
    assert np.linalg.norm(m.apply(m.apply(X, "sqrt"), "sqrt") - m.apply(X, "M")) <= 1e-12 * np.linalg.norm(m.apply(X, "M"))
    assert np.linalg.norm(m.apply(m.apply(X, "inv"), "M") - X) <= 1e-12 * np.linalg.norm(X)
    c = np.arange(n, dtype=float)
    mc = LowRankMetric(m.Vt, m.lam, center=c)
    assert np.array_equal(mc.draw(X), c + m.apply(X, "invsqrt"))
    with pytest.raises(ValueError):
        m.apply(X, "cube")
    with pytest.raises(ValueError):
        LowRankMetric(m.Vt, -lam)


def test_from_jacobian_matches_a_dense_eigendecomposition():
    """Random upper U, random J [9 x n], sigma = 0.1: eigenvalues of the dense U J^T J U^T / sigma^2 to 1e-10 relative, the
    eigenspace projector to 1e-8 in the 2-norm; a J with two equal rows has rank 8."""
    n, sigma = 60, 0.1
    prior = _Prior(n, 2)
    J = np.random.default_rng(3).standard_normal((9, n))
    m = LowRankMetric.from_jacobian(J, prior, sigma)
    assert m.rho == 9 and m.n == n
    H = prior.U @ J.T @ J @ prior.U.T / sigma ** 2
    w, Q = np.linalg.eigh(H)
    w, Q = w[::-1][:9], Q[:, ::-1][:, :9]
    assert np.all(np.abs(m.lam - w) <= 1e-10 * w)
    assert np.linalg.norm(m.Vt.T @ m.Vt - Q @ Q.T, 2) <= 1e-8
    assert np.linalg.norm(m.dense() - (np.eye(n) + H), 2) <= 1e-10 * np.linalg.norm(H, 2)
    J2 = J.copy(); J2[5] = J2[2]
    assert LowRankMetric.from_jacobian(J2, prior, sigma).rho == 8
    # the field's pointwise variance under N(v*, M^-1), against the dense posterior covariance
    var = pointwise_variance(prior, m)
    want = np.diag(prior.U.T @ np.linalg.inv(np.eye(n) + H) @ prior.U)
    assert np.allclose(var, want, rtol=1e-9, atol=0)


def _gaussian_target(V_lam_Vt, m):
    """value_and_grad of loss(v) = (v - m)^T V diag(lambda) V^T (v - m) / 2."""
    def f(K):
        g = (K - m) @ V_lam_Vt
        return 0.5 * np.einsum("cn,cn->c", K - m, g), g, np.zeros(len(K), bool)
    return f


def test_metric_chain_is_the_identity_mass_chain_in_isotropic_coordinates():
    """A Gaussian target with precision M = I + V diag(lambda) V^T and mean m: the chain under the metric M from v0 and the
    identity-mass chain on z = M^(1/2) (v - m) (a standard normal target) from z0 = M^(1/2) (v0 - m) with the same seeds are the
    same chain -- equal accept vectors and traces' accept patterns, mapped end states within 1e-10 relative.
    n = 400, rho = 9, lambda = logspace(0, 3, 9), eps = 0.2, L = 10, 100 proposals."""
    n, lam, C = 400, np.logspace(0, 3, 9), 2
    metric = _metric(n, lam, 4)
    rng = np.random.default_rng(5)
    m = rng.standard_normal(n)
    v0 = m + metric.apply(rng.standard_normal((C, n)), "invsqrt")
    z0 = metric.apply(v0 - m, "sqrt")
    kw = dict(seeds=[40 + c for c in range(C)], eps=0.2, n_leapfrog=10, sigma=1.0, tau=1.0, keep_trace=True)
    a = hmc.run_chains(_gaussian_target((metric.Vt.T * lam) @ metric.Vt, m), v0, 1001, mean=m, metric=metric, **kw)
    b = hmc.run_chains(lambda K: (np.zeros(len(K)), np.zeros_like(K), np.zeros(len(K), bool)), z0, 1001, mean=0.0, **kw)
    assert a.proposals == b.proposals == 100
    print("accepted", a.accept, b.accept)
    assert np.array_equal(a.accept, b.accept)
    assert np.all(a.accept > 0)
    moved_a = np.any(a.trace[1:] != a.trace[:-1], axis=2)
    moved_b = np.any(b.trace[1:] != b.trace[:-1], axis=2)
    assert np.array_equal(moved_a, moved_b)
    za = metric.apply(a.K - m, "sqrt")
    err = np.linalg.norm(za - b.K) / np.linalg.norm(b.K)
    print("mapped end-state difference", err)
    assert err <= 1e-10


def test_a_rank_zero_metric_gives_the_bits_of_no_metric():
    n, C = 50, 3
    rng = np.random.default_rng(7)
    A = rng.standard_normal((n, n)); A = A @ A.T / n
    m = rng.standard_normal(n)
    v0 = rng.standard_normal((C, n))
    kw = dict(seeds=[1, 2, 3], eps=0.15, n_leapfrog=5, sigma=1.0, tau=1.0, mean=m, keep_trace=True)
    f = _gaussian_target(A, m)
    a = hmc.run_chains(f, v0, 101, **kw)
    b = hmc.run_chains(f, v0, 101, metric=LowRankMetric(np.zeros((0, n)), np.zeros(0)), **kw)
    assert 0 < a.accept.sum()
    assert np.array_equal(a.accept, b.accept) and np.array_equal(a.K, b.K) and np.array_equal(a.trace, b.trace)
    with pytest.raises(ValueError):
        hmc.run_chains(f, v0, 101, metric=_metric(n + 1, np.ones(2), 0), **kw)


def test_gauss_newton_map_reaches_a_linear_models_map_in_one_step():
    """y = J k: phi is quadratic and the Gauss-Newton Hessian is its Hessian, so the full step from v = 0 lands on the closed-form
    MAP v* = (I + A^T A / sigma^2)^-1 A^T (d - J mean) / sigma^2, A = J U^T, to 1e-10; the iteration then stops by itself."""
    n, n_obs, sigma = 80, 9, 0.05
    prior = _Prior(n, 8, mean=1.0)
    rng = np.random.default_rng(9)
    J = rng.standard_normal((n_obs, n))
    d = J @ prior.field(rng.standard_normal(n)) + sigma * rng.standard_normal(n_obs)
    calls = []

    def f(K, jac=False):
        K = np.atleast_2d(K)
        calls.append((len(K), jac))
        r = d - K @ J.T
        out = dict(loss=0.5 * np.einsum("bo,bo->b", r, r), grad=-r @ J, info=np.zeros(len(K), int))
        if jac:
            out["J"] = J
        return out

    A = J @ prior.U.T
    v_star = scipy.linalg.solve(np.eye(n) + A.T @ A / sigma ** 2, A.T @ (d - J @ prior.mean) / sigma ** 2, assume_a="pos")
    one = gauss_newton_map(f, prior, sigma, maxiter=1)
    assert one["steps"] == 1 and np.linalg.norm(one["v"] - v_star) <= 1e-10 * np.linalg.norm(v_star)
    assert calls == [(1, True), (8, False), (1, True)]
    res = gauss_newton_map(f, prior, sigma)
    assert res["steps"] <= 3 and np.linalg.norm(res["v"] - v_star) <= 1e-10 * np.linalg.norm(v_star)
    assert np.all(np.diff(res["phi"]) < 0) and len(res["phi"]) == res["steps"] + 1 == len(res["grad_norm"])
    assert res["grad_norm"][-1] <= 1e-8 * res["grad_norm"][0]
    assert np.allclose(res["k"], prior.field(res["v"])) and res["metric"].rho == n_obs
    assert np.array_equal(res["metric"].center, res["v"])
    H = np.eye(n) + A.T @ A / sigma ** 2
    assert np.linalg.norm(res["metric"].dense() - H, 2) <= 1e-10 * np.linalg.norm(H, 2)
