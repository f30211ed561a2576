"""CPU tests of the batched multi-start minimiser's specification (bayesian_inference/lbfgs.py: minimize_host) against SciPy's
L-BFGS-B, its edge semantics, and the host-side checks of the finrom_lbfgs_* entry points (no GPU: nothing reaches a device)."""
import ctypes as C

import numpy as np
import pytest
from scipy.optimize import minimize

from bayesianinferencedl_amd.bayesian_inference import lbfgs


def _quadratic(d=50, seed=0):
    """A strictly convex quadratic with cond(A) = 1e3 built from its bounded minimiser x*: a third of x* on the box, with
    gradients g* that point out of it there (strict complementarity) and zero elsewhere.  f(x) = 0.5 e^T A e + g*^T e, e = x - x*,
    is evaluated in that form, so that f is small near x* and its decrease resolves x to 1e-8.  -> (fun, x*, lo, hi)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    A = (Q * np.logspace(0, 3, d)) @ Q.T
    A = 0.5 * (A + A.T)
    xs = rng.uniform(-1.0, 1.0, d)
    lo, hi = xs - rng.uniform(0.5, 1.5, d), xs + rng.uniform(0.5, 1.5, d)
    gs = np.zeros(d)
    for j in rng.permutation(d)[: d // 3]:
        if rng.uniform() < 0.5:
            lo[j] = xs[j]; gs[j] = rng.uniform(1.0, 10.0)
        else:
            hi[j] = xs[j]; gs[j] = -rng.uniform(1.0, 10.0)

    def fun(x):
        e = x - xs
        Ae = A @ e
        return 0.5 * (e @ Ae) + gs @ e, Ae + gs
    return fun, xs, lo, hi


def _batched(fun):
    def f(X):
        vals = [fun(x) for x in np.asarray(X)]
        return np.array([v[0] for v in vals]), np.stack([v[1] for v in vals]), np.zeros(len(vals), bool)
    return f


def _rosen(x):
    f = np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2)
    g = np.zeros_like(x)
    g[:-1] = -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2.0 * (1.0 - x[:-1])
    g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
    return f, g


def test_quadratic_with_active_bounds_matches_scipy():
    fun, xs, lo, hi = _quadratic()
    x0 = np.zeros(len(xs))
    ref = minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                   options=dict(ftol=0.0, gtol=1e-11, maxiter=20000, maxfun=20000))
    res = lbfgs.minimize_host(_batched(fun), x0[None], bounds=(lo, hi), ftol=0.0, gtol=1e-11, maxiter=20000, maxfun=20000)
    x = res.x[0]
    act_ref = (ref.x == lo) | (ref.x == hi)
    act = (x == lo) | (x == hi)
    assert act_ref.sum() == len(xs) // 3                     # a third of the solution is on the box
    assert np.array_equal(act, act_ref)
    assert np.linalg.norm(ref.x - xs) <= 1e-8 * np.linalg.norm(xs)
    assert np.linalg.norm(x - ref.x) <= 1e-8 * np.linalg.norm(ref.x)
    assert res.status[0] == 0 and res.success[0]


def test_bounded_rosenbrock_matches_scipy():
    d = 10
    lo, hi = np.full(d, -1.5), np.full(d, 0.8)               # the unconstrained minimiser (1, ..., 1) is outside
    x0 = np.full(d, -0.5)
    ref = minimize(_rosen, x0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                   options=dict(ftol=1e-15, gtol=1e-11, maxiter=20000, maxfun=20000))
    res = lbfgs.minimize_host(_batched(_rosen), x0[None], bounds=(lo, hi), ftol=1e-15, gtol=1e-11, maxiter=20000, maxfun=20000)
    assert np.any(np.abs(ref.x - hi) < 1e-12)
    assert np.linalg.norm(res.x[0] - ref.x) <= 1e-6 * np.linalg.norm(ref.x)
    assert res.status[0] == 0


def test_infeasible_start_is_projected_and_fixed_components_never_move():
    fun, _, _, _ = _quadratic(d=12, seed=3)
    lo, hi = np.full(12, -0.5), np.full(12, 0.5)
    lo[[2, 7]] = hi[[2, 7]] = [0.25, -0.1]                   # fixed components
    seen = []

    def f(X):
        seen.append(np.array(X, copy=True))
        return _batched(fun)(X)
    x0 = np.linspace(-3.0, 3.0, 12)
    res = lbfgs.minimize_host(f, x0[None], bounds=(lo, hi), gtol=1e-9)
    assert np.array_equal(seen[0][0], np.clip(x0, lo, hi))
    for X in seen:
        assert np.all(X >= lo) and np.all(X <= hi)
        assert X[0, 2] == 0.25 and X[0, 7] == -0.1
    assert res.x[0, 2] == 0.25 and res.x[0, 7] == -0.1 and res.status[0] == 0


def test_iteration_limit_gives_status_1():
    res = lbfgs.minimize_host(_batched(_rosen), np.full((1, 6), -1.0), maxiter=3)
    assert res.status[0] == 1 and res.nit[0] == 3 and not res.success[0]
    assert "ITERATIONS" in res.message[0]


def test_infinite_trials_end_the_line_search_with_status_2():
    calls = []

    def f(X):
        calls.append(1)
        x = np.asarray(X)[0]
        if len(calls) == 1:
            return np.array([x @ x]), (2.0 * x)[None], np.zeros(1, bool)
        return np.array([np.inf]), np.zeros_like(X), np.zeros(1, bool)
    res = lbfgs.minimize_host(f, np.ones((1, 4)), maxls=7)
    assert res.status[0] == 2 and res.nit[0] == 0
    assert res.nfev[0] == 1 + 7 and len(calls) == 1 + 7
    assert res.message[0] == "ABNORMAL_TERMINATION_IN_LNSRCH"


def test_flagged_start_gives_status_3():
    def f(X):
        X = np.asarray(X)
        return np.sum(X * X, 1), 2.0 * X, np.array([False, True])
    res = lbfgs.minimize_host(f, np.ones((2, 3)), gtol=1e-10)
    assert res.status[1] == 3 and res.nfev[1] == 1 and res.nit[1] == 0 and np.isinf(res.fun[1])
    assert res.status[0] == 0


def test_starts_in_one_call_equal_each_start_alone_bit_for_bit():
    rng = np.random.default_rng(5)
    X0 = rng.uniform(-1.2, 1.2, (5, 8))
    bounds = (-1.0, 0.9)
    batch = lbfgs.minimize_host(_batched(_rosen), X0, bounds=bounds, keep_history=True)
    for i in range(5):
        one = lbfgs.minimize_host(_batched(_rosen), X0[i:i + 1], bounds=bounds, keep_history=True)
        assert np.array_equal(one.x[0], batch.x[i]) and one.fun[0] == batch.fun[i]
        assert one.nit[0] == batch.nit[i] and one.nfev[0] == batch.nfev[i] and one.status[0] == batch.status[i]
        n = one.nit[0] + 1
        assert np.array_equal(one.fhist[:n, 0], batch.fhist[:n, i])
        assert np.all(np.isnan(batch.fhist[n:, i]))


def test_rowdot_is_the_device_summation_order():
    """_rowdot restates block_sum_256 over lanes t = j mod 256: per-lane running sums, a butterfly inside each wave of 64, the
    four waves pairwise.  Exact on integers, and the same bits for a row whatever the other rows are."""
    rng = np.random.default_rng(1)
    a = rng.integers(-50, 50, (3, 1597)).astype(float)
    assert np.array_equal(lbfgs._rowdot(a, a), np.einsum("sd,sd->s", a, a))
    x = rng.standard_normal((4, 700))
    assert np.array_equal(lbfgs._rowdot(x, x)[2:3], lbfgs._rowdot(x[2:3], x[2:3]))


def test_lower_above_upper_bound_raises():
    with pytest.raises(ValueError, match="lo > hi"):
        lbfgs.minimize_host(_batched(_rosen), np.zeros((1, 3)), bounds=(np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.5, 1.0])))
    with pytest.raises(ValueError, match="lo > hi"):                # before any device is touched
        lbfgs.minimize_device(None, np.zeros((1, 3)), bounds=(1.0, 0.0))


def test_lbfgs_entry_points_validate_their_state_before_any_device_call():
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()

    def state(**kw):
        base = dict(S=4, d=10, m=5, ftol=1e-9, gtol=1e-5, maxiter=10, maxfun=10, maxls=20)
        base.update(kw)
        return _ffi.LbfgsState(**base)
    for fn in (L.finrom_lbfgs_begin, L.finrom_lbfgs_propose):
        assert fn(C.byref(state(S=0)), None) == -1 and b"S = 0" in L.finrom_last_error()
        assert fn(C.byref(state(m=0)), None) == -1 and b"m = 0" in L.finrom_last_error()
        assert fn(C.byref(state(m=17)), None) == -1 and b"m = 17" in L.finrom_last_error()
        assert fn(C.byref(state(d=0)), None) == -1 and b"d = 0" in L.finrom_last_error()
        assert fn(C.byref(state()), None) == -1 and b"null x" in L.finrom_last_error()
        assert fn(C.byref(state(gdim=3)), None) == -1 and b"gdim" in L.finrom_last_error()
        assert fn(None, None) == -1 and b"null state" in L.finrom_last_error()
    assert L.finrom_lbfgs_accept(C.byref(state(S=-1)), None, None, None, None) == -1 and b"S = -1" in L.finrom_last_error()
    assert L.finrom_lbfgs_accept(C.byref(state()), None, None, None, None) == -1 and b"null x" in L.finrom_last_error()
    assert L.finrom_deferred_count() == 0
