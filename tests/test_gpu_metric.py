"""Laplace-preconditioned HMC on the HIP path: the low-rank metric's maps (finrom_metric_apply) against extended precision, the
Jacobian and Gauss-Newton metric of the ROM + learned-error misfit against the oracle, chains under prior + metric -- host
recursion, torch form, fused form, with and without a captured graph -- against each other, and the point of the feature: at
sigma = 1e-3 the chains under the metric taken at the MAP accept at eps = 0.3 where identity-mass chains reject at eps = 0.12."""
import os
import sys

import numpy as np
import pytest

from oracle import fin_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 4, 17, 64, 300)
OPS = ("M", "inv", "sqrt", "invsqrt")
LD = np.longdouble


def _coef_ld(lam, op):
    lam = lam.astype(LD)
    return {"M": lam, "inv": -lam / (1 + lam), "sqrt": np.sqrt(1 + lam) - 1, "invsqrt": 1 / np.sqrt(1 + lam) - 1}[op]


@pytest.mark.parametrize("rho", [1, 9, 40, 64])
@pytest.mark.parametrize("n", [37, 1597, 4101])
def test_metric_apply_matches_extended_precision_and_is_row_independent(n, rho):
    """y = x + sum_j c_j V_j (V_j . x) for the four maps, S in 1, 4, 17, 64, 300, lambda from 1e-2 up to 1e5: within
    2e-13 * (|x| + sum_j |c_j| |V_j| (|V_j| . |x|)) of the np.longdouble result element by element, quad = x . y within the same
    bound summed against |x|; run to run bitwise identical; a row alone has the bits of the same row in a batch.
    (n = 37 holds at most 37 orthonormal rows: at rho = 40 and 64 the case is that create refuses the handle.)"""
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.engine import MetricHandle
    rng = np.random.default_rng(1000 * rho + n)
    lam = np.logspace(-2, 5, rho) if rho > 1 else np.array([1e5])
    if rho > n:
        with pytest.raises(_ffi.FinromError):
            MetricHandle(rng.standard_normal((rho, n)) / np.sqrt(n), lam)
        return
    Vt = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((n, rho)))[0].T)
    mh = MetricHandle(Vt, lam)
    X = rng.standard_normal((max(SIZES), n))
    # rows checked against extended precision (all of them below n = 4101; there a sample -- the other rows are the same
    # computation, as the row-independence check shows)
    rows = np.arange(max(SIZES)) if n < 4000 else np.array([0, 1, 2, 3, 16, 63, 64, 65, 127, 128, 255, 299])
    VL, XL = Vt.astype(LD), X[rows].astype(LD)
    dots = XL @ VL.T
    adots = np.abs(X[rows]) @ np.abs(Vt).T
    for op in OPS:
        c = _coef_ld(lam, op)
        yref = XL + (dots * c) @ VL
        scale = np.abs(X[rows]) + (adots * np.abs(c).astype(np.float64)) @ np.abs(Vt)
        qref = np.einsum("sn,sn->s", XL, yref)
        qscale = np.einsum("sn,sn->s", np.abs(X[rows]), scale)
        full, qfull = mh.apply(X, op, want_quad=True)
        for S in SIZES:
            y, q = mh.apply(X[:S], op, want_quad=True)
            assert y.shape == (S, n) and q.shape == (S,)
            sel = rows < S
            err = np.abs(y[rows[sel]].astype(LD) - yref[sel]).astype(np.float64)
            assert np.all(err <= 2e-13 * scale[sel]), (n, rho, op, S, float(np.max(err / scale[sel])))
            qerr = np.abs(q[rows[sel]].astype(LD) - qref[sel]).astype(np.float64)
            assert np.all(qerr <= 2e-13 * qscale[sel]), (n, rho, op, S, float(np.max(qerr / qscale[sel])))
            y2, q2 = mh.apply(X[:S], op, want_quad=True)
            assert np.array_equal(y, y2) and np.array_equal(q, q2), (n, rho, op, S)
            assert np.array_equal(y, full[:S]) and np.array_equal(q, qfull[:S]), (n, rho, op, S)
            assert np.array_equal(mh.apply(X[:S], op), y), (n, rho, op, S)         # (without quad: the same rows)
        for r in (0, 5, 63, 299):
            y1, q1 = mh.apply(X[r:r + 1], op, want_quad=True)
            assert np.array_equal(y1[0], full[r]) and q1[0] == qfull[r], (n, rho, op, r)


def test_metric_create_refuses_bad_arguments():
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.engine import MetricHandle
    n = 100
    Q = np.linalg.qr(np.random.default_rng(0).standard_normal((n, 65)))[0].T
    MetricHandle(Q[:64], np.ones(64))
    for Vt, lam in ((Q[:0], np.ones(0)), (Q[:65], np.ones(65)), (Q[:3], np.array([1.0, 0.0, 2.0])), (Q[:3], np.array([1.0, -1.0, 2.0])),
                    (Q[:3], np.array([1.0, np.inf, 2.0])), (Q[:3], np.array([1.0, np.nan, 2.0])), (1.001 * Q[:3], np.ones(3)),
                    (np.stack([Q[0], Q[0]]), np.ones(2))):
        with pytest.raises(_ffi.FinromError):
            MetricHandle(Vt, lam)


@pytest.fixture(scope="module")
def setup(problems, spaces):
    """The setting of test_gpu_field_prior.py: m = 12, r = 81, GaussianFieldPrior(V, amplitude=0.1, mean=1.0), bench.hmc_error_model."""
    sys.path.insert(0, ROOT)
    import bench
    from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.rom.basis import pod_basis
    m, r = 12, 81
    prob, V = problems(m), spaces(m)
    solver = Fin(V)
    phi = pod_basis(solver, r, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1)
    model = bench.hmc_error_model(V.dim())
    k_true = np.exp(0.25 * np.random.default_rng(11).standard_normal(V.dim()))
    data = solver.qoi_operator(solver.forward(k_true)[0])
    ro = O.AffineROMOracle(prob, phi); ro.set_data(data)
    prior = GaussianFieldPrior(V, amplitude=0.1, mean=1.0)
    return V, phi, model, data, ro, prior, solver


def _rom(setup):
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    V, phi, model, data = setup[:4]
    rom = AffineROMFin(V, model, phi); rom.set_data(data)
    return rom


@pytest.fixture(scope="module")
def maps(setup):
    """gauss_newton_map from v = 0 per noise level, once."""
    from bayesianinferencedl_amd.bayesian_inference.laplace import gauss_newton_map, reduced_value_grad_jac
    prior = setup[5]
    rom = _rom(setup)
    cache = {}

    def get(sigma):
        if sigma not in cache:
            cache[sigma] = gauss_newton_map(reduced_value_grad_jac(rom, "romml"), prior, sigma)
            print("gauss_newton_map sigma", sigma, "steps", cache[sigma]["steps"], "phi", cache[sigma]["phi"][[0, -1]],
                  "grad norm", cache[sigma]["grad_norm"][[0, -1]], "lambda_max", cache[sigma]["metric"].lam.max())
        return cache[sigma]
    return get


def test_jacobian_and_metric_match_the_oracle(setup):
    """Rows of misfit_jacobian('romml') within 1e-5 relative (the project's ROM + ML gradient tolerance) of differences of
    O.grad_romml_oracle with shifted data; the metric built from them, applied on the device to the identity, within
    1e-4 |M_oracle - I|_2 of the oracle's (twice the row tolerance, factor 5 on top); for kind='fom', J^T J u against
    Fin.GN_hessian_action to 1e-9."""
    from bayesianinferencedl_amd.bayesian_inference.laplace import LowRankMetric, misfit_jacobian
    V, phi, model, data, ro, prior, solver = setup
    n, sigma = V.dim(), 1e-3
    k = prior.field(0.5 * np.random.default_rng(21).standard_normal(n))
    J = misfit_jacobian("romml", k, solver_r=_rom(setup))
    n_obs = len(data)
    assert J.shape == (n_obs, n)
    g0, _ = O.grad_romml_oracle(ro, model, k)
    Jo = np.zeros_like(J)
    try:
        for i in range(n_obs):
            d = np.array(data, dtype=np.float64); d[i] += 1.0
            ro.set_data(d)
            Jo[i] = g0 - O.grad_romml_oracle(ro, model, k)[0]
    finally:
        ro.set_data(data)
    for i in range(n_obs):
        rel = np.linalg.norm(J[i] - Jo[i]) / np.linalg.norm(Jo[i])
        print("jacobian row", i, "relative difference", rel)
        assert rel <= 1e-5, (i, rel)
    md, mo = LowRankMetric.from_jacobian(J, prior, sigma), LowRankMetric.from_jacobian(Jo, prior, sigma)
    M_dev = md.device().apply(np.eye(n), "M")
    M_o = mo.dense()
    num, den = np.linalg.norm(M_dev - M_o, 2), np.linalg.norm(M_o - np.eye(n), 2)
    print("metric difference", num, "of", den)
    assert num <= 1e-4 * den
    Jf = misfit_jacobian("fom", k, solver=solver)
    u = np.random.default_rng(22).standard_normal(n)
    want = solver.GN_hessian_action(k, u)
    assert np.linalg.norm(Jf.T @ (Jf @ u) - want) <= 1e-9 * np.linalg.norm(want)
    # kind='rom': the same differences of the oracle's reduced gradient (the ROM part of the gradient above: the same tolerance)
    Jr = misfit_jacobian("rom", k, solver_r=_rom(setup))
    gr0 = ro.grad_reduced(k)[0]
    try:
        for i in (0, n_obs - 1):
            d = np.array(data, dtype=np.float64); d[i] += 1.0
            ro.set_data(d)
            want = gr0 - ro.grad_reduced(k)[0]
            assert np.linalg.norm(Jr[i] - want) <= 1e-5 * np.linalg.norm(want), i
    finally:
        ro.set_data(data)


def _starts(metric, n):
    return np.stack([metric.draw(np.random.default_rng(6 + c).standard_normal(n)) for c in range(4)])


def _host(setup, maps, sigma, metric=None):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    prior = setup[5]
    metric = maps(sigma)["metric"] if metric is None else metric
    want = {0, 1, 10, 55, 120}
    kw = dict(seeds=[100 + c for c in range(4)], eps=0.3, n_leapfrog=10, prior=prior, sigma=sigma)
    V0 = _starts(maps(sigma)["metric"], prior.n)
    res = hmc.run_chains(hmc.romml_value_and_grad(_rom(setup)), V0, 121, record=want, keep_trace=True, metric=metric, **kw)
    return kw, want, V0, res


@pytest.fixture(scope="module")
def host_chains(setup, maps):
    cache = {}

    def get(sigma):
        if sigma not in cache:
            cache[sigma] = _host(setup, maps, sigma)
        return cache[sigma]
    return get


@pytest.fixture(scope="module")
def host_rounding(setup, maps, host_chains):
    """The deviation, at sigma = 1e-3, between the host recursion in float64 and the same recursion with the metric's products
    formed in np.longdouble (rounded to float64 on return): what the rounding of the metric maps alone does to the trace."""
    from bayesianinferencedl_amd.bayesian_inference.laplace import LowRankMetric
    m = maps(1e-3)["metric"]

    class Extended(LowRankMetric):
        def apply(self, x, op="M"):
            xl, vl = np.asarray(x, dtype=np.float64).astype(LD), self.Vt.astype(LD)
            return (xl + ((xl @ vl.T) * _coef_ld(self.lam, op)) @ vl).astype(np.float64)

    ext = _host(setup, maps, 1e-3, metric=Extended(m.Vt, m.lam, center=m.center))[3]
    host = host_chains(1e-3)[3]
    dev = float(np.max(np.abs(ext.trace - host.trace)) / np.max(np.abs(host.trace)))
    print("host float64 against longdouble metric products: relative trace deviation", dev, "accept", host.accept, ext.accept)
    return dev


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("graph", [True, False])
def test_device_chains_under_the_metric_walk_the_host_chains_path(setup, maps, host_chains, graph, fused):
    """sigma = 0.05, prior + metric at the MAP, starts drawn from the Laplace approximation, eps = 0.3, L = 10, 121 evaluations:
    run_chains_device(metric=...), fused (finrom_hmc_begin_metric / _leapfrog_field_metric / _end_metric) or torch form
    (MetricHandle.apply around the field-prior evaluation), replayed as a graph or in stream order, gives the host chain's accept
    vector, and its trace, end fields and whitened end states within 1e-9 (the tolerances of the chains under the prior alone)."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    kw, want, V0, host = host_chains(0.05)
    dev = hmc.run_chains_device(_rom(setup), V0, 121, record=want, keep_trace=True, graph=graph, fused=fused,
                                metric=maps(0.05)["metric"], **kw)
    assert dev.fused == fused and dev.graph == graph
    assert dev.n_evals == host.n_evals == 121 and dev.proposals == host.proposals == 12
    print("accept", host.accept, dev.accept, "trace", np.max(np.abs(dev.trace - host.trace)) / np.max(np.abs(host.trace)))
    assert np.array_equal(dev.accept, host.accept)
    assert host.accept.sum() > 0
    assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    assert np.linalg.norm(dev.K - host.K) <= 1e-9 * np.linalg.norm(host.K)
    assert np.linalg.norm(dev.V - host.V) <= 1e-9 * np.linalg.norm(host.V)
    assert [e for e, *_ in dev.recorded] == [e for e, *_ in host.recorded]
    for (ev, K, loss, grad), (_, Kh, lossh, gradh) in zip(dev.recorded, host.recorded):
        assert np.linalg.norm(K - Kh) <= 1e-9 * np.linalg.norm(Kh), ev
        assert np.linalg.norm(grad - gradh) <= 1e-6 * np.linalg.norm(gradh), ev


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("graph", [True, False])
def test_device_chains_under_the_metric_at_small_noise(setup, maps, host_chains, host_rounding, graph, fused):
    """The same at sigma = 1e-3 (lambda_max ~ 1e3): equal accept vectors, and the trace within 16x (the project's allowance) the
    deviation between the host recursion in float64 and the same recursion with the metric's products in np.longdouble.
    Measured on an MI355X: the two host recursions differ by 2.1e-6 of the trace (so 3.4e-5 is allowed); fused and torch form,
    graph and stream order, are each 7.5e-7 from the float64 host chain, with its accept vector (12, 11, 11, 12)."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    kw, want, V0, host = host_chains(1e-3)
    dev = hmc.run_chains_device(_rom(setup), V0, 121, keep_trace=True, graph=graph, fused=fused, metric=maps(1e-3)["metric"], **kw)
    assert dev.fused == fused and dev.graph == graph and dev.proposals == host.proposals == 12
    got = float(np.max(np.abs(dev.trace - host.trace)) / np.max(np.abs(host.trace)))
    print("accept", host.accept, dev.accept, "trace deviation", got, "allowed", 16 * host_rounding)
    assert np.array_equal(dev.accept, host.accept)
    assert got <= 16 * host_rounding


def test_fused_chains_need_the_prior_for_a_metric(setup, maps):
    """run_chains_fused(metric=...) without prior= is FINROM_ERR_UNSUPPORTED (no metric form of the i.i.d.-prior leapfrog step)."""
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc
    prior = setup[5]
    K0 = prior.field(np.zeros((2, prior.n)))
    with pytest.raises(_ffi.FinromError, match="status -4"):
        hmc.run_chains_fused(_rom(setup), K0, 11, seeds=[1, 2], metric=maps(0.05)["metric"])


def test_the_metric_at_the_map_lets_chains_move_at_small_noise(setup, maps):
    """sigma = 1e-3.  gauss_newton_map from v = 0: phi never rises, ends at <= 0.05 x its start (oracle: 7960 -> 122.8), the
    whitened gradient norm falls >= 100x (oracle: 4e4 x), the field is positive.  Chains from draws of the Laplace approximation,
    seeds 100 + c, C = 4, 121 evaluations, L = 10, each run a single call: under the metric at eps = 0.3 at least 36 of 48
    proposals are accepted (oracle: 46); with the identity mass at eps = 0.12 at most 4 of 48 (oracle: 0)."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    prior = setup[5]
    sigma = 1e-3
    res = maps(sigma)
    phi, gn = res["phi"], res["grad_norm"]
    print("phi", phi, "grad norm", gn)
    assert np.all(np.diff(phi) <= 0)
    assert phi[-1] <= 0.05 * phi[0]
    assert gn[-1] <= gn[0] / 100
    assert np.all(res["k"] > 0)
    metric = res["metric"]
    assert np.array_equal(metric.center, res["v"])
    V0 = _starts(metric, prior.n)
    kw = dict(seeds=[100 + c for c in range(4)], n_leapfrog=10, prior=prior, sigma=sigma)
    with_metric = hmc.run_chains_device(_rom(setup), V0, 121, eps=0.3, metric=metric, **kw)
    without = hmc.run_chains_device(_rom(setup), V0, 121, eps=0.12, **kw)
    print("accepted with the metric", with_metric.accept, "without", without.accept)
    assert with_metric.proposals == without.proposals == 12
    assert with_metric.accept.sum() >= 36
    assert without.accept.sum() <= 4
