"""HMC chains under the reference's latent Gaussian-field prior on the HIP path (bayesian_inference/pymc_func_bayes_inverse.py:
191-201, pm.gp.Latent(Matern52(2, ls=1.2)).prior, sampled non-centred): the two triangular products of the sampler handle
(finrom_sampler_field / _pullback) against extended precision, and chains under the prior -- host recursion, torch form, fused
form, with and without a captured graph -- against each other and the oracle."""
import os
import sys

import numpy as np
import pytest

from oracle import fin_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 4, 17, 64, 300)


def _factor(n, seed):
    """An upper factor with the Matern factor's character (positive diagonal, decaying rows) at any n."""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((n, n))) / np.sqrt(np.arange(1, n + 1))[None, :]
    U[np.diag_indices(n)] = np.abs(U[np.diag_indices(n)]) + 0.5
    return U


@pytest.mark.parametrize("n", [37, 1597, 4101])
def test_field_and_pullback_match_extended_precision_and_are_row_independent(n):
    """k = mean + U^T v and g_v = U g for S in 1, 4, 17, 64, 300 (300 = five launches): within 2e-13 of the np.longdouble products
    relative to |U^T| |v| (|U| |g|) element by element; run to run bitwise identical; row c bitwise the same whether it is
    computed alone or inside a batch (the fixed summation order depends on n alone)."""
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.engine import FieldSampler
    U = _factor(n, n)
    rng = np.random.default_rng(1)
    v = rng.standard_normal((max(SIZES), n))
    g = rng.standard_normal((max(SIZES), n))
    mean = rng.uniform(0.5, 1.5, n)
    fs = FieldSampler(U)
    # rows checked against extended precision (all of them below n = 4101; there a sample across the launch boundaries -- the
    # other rows are the same computation, as the row-independence check below shows)
    rows = np.arange(max(SIZES)) if n < 4000 else np.array([0, 1, 2, 3, 16, 63, 64, 65, 127, 128, 255, 299])
    UL = U.astype(np.longdouble)
    kref = (v[rows].astype(np.longdouble) @ UL + mean.astype(np.longdouble)).astype(np.float64)
    gref = (g[rows].astype(np.longdouble) @ UL.T).astype(np.float64)
    kscale = np.abs(v[rows]) @ np.abs(U) + np.abs(mean)
    gscale = np.abs(g[rows]) @ np.abs(U).T
    full_k, full_g = fs.field(v, mean=mean), fs.pullback(g)
    for S in SIZES:
        k, gv = fs.field(v[:S], mean=mean), fs.pullback(g[:S])
        assert k.shape == gv.shape == (S, n)
        sel = rows[rows < S]
        assert np.all(np.abs(k[sel] - kref[:len(sel)]) <= 2e-13 * kscale[:len(sel)]), (n, S)
        assert np.all(np.abs(gv[sel] - gref[:len(sel)]) <= 2e-13 * gscale[:len(sel)]), (n, S)
        assert np.array_equal(k, fs.field(v[:S], mean=mean)) and np.array_equal(gv, fs.pullback(g[:S])), (n, S)
        assert np.array_equal(k, full_k[:S]) and np.array_equal(gv, full_g[:S]), (n, S)
    for c in (0, 5, 63):
        assert np.array_equal(fs.field(v[c:c + 1], mean=mean)[0], full_k[c])
        assert np.array_equal(fs.pullback(g[c:c + 1])[0], full_g[c])
    assert np.all(np.abs(fs.field(v[:4]) - (v[:4] @ U)) <= 2e-13 * (np.abs(v[:4]) @ np.abs(U)))
    with pytest.raises(_ffi.FinromError):
        FieldSampler(np.ascontiguousarray(U.T))                                   # a lower factor is still refused at create


@pytest.fixture(scope="module")
def setup(problems, spaces):
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
    prior = GaussianFieldPrior(V, amplitude=0.1, mean=1.0)            # fields 1 +- a few tenths: positive conductivities
    V0 = np.stack([np.random.default_rng(6 + c).standard_normal(V.dim()) for c in range(4)])
    return V, phi, model, data, ro, prior, V0


def _rom(setup):
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    V, phi, model, data = setup[:4]
    rom = AffineROMFin(V, model, phi); rom.set_data(data)
    return rom


@pytest.fixture(scope="module")
def host_chain(setup):
    """The host recursion under the prior at the first step size whose chains accept some proposals and reject others."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    prior, V0 = setup[5], setup[6]
    rom = _rom(setup)
    want = {0, 1, 10, 55, 120}
    for eps in (0.3, 0.2, 0.12, 0.08, 0.05, 0.03):
        kw = dict(seeds=[100 + c for c in range(4)], eps=eps, n_leapfrog=10, prior=prior)
        res = hmc.run_chains(hmc.romml_value_and_grad(rom), V0, 121, record=want, keep_trace=True, **kw)
        if 0 < res.accept.sum() < 4 * 12:
            return kw, want, res
    pytest.fail("no step size gave both accepted and rejected proposals: %s" % res.accept)


def test_host_chain_under_the_prior_matches_the_oracle(setup, host_chain):
    """Every recorded evaluation of the host chain -- at a field k = mean + U^T v the chain's own gradients produced -- against the
    oracle's dense restatement (tolerances of test_gpu_hmc.py); the whitened gradient the chain integrates there is
    v + c_lik U grad_k."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    V, phi, model, data, ro, prior, V0 = setup
    kw, want, res = host_chain
    assert res.n_evals == 121 and res.proposals == 12 and len(res.recorded) == len(want)
    assert np.allclose(res.K, prior.field(res.V)) and (res.K > 0).all()
    f = hmc.whitened_potential(hmc.romml_value_and_grad(_rom(setup)), prior, 0.05)
    for ev, K, loss, grad in res.recorded:
        for c in range(4):
            go, lo = O.grad_romml_oracle(ro, model, K[c])
            assert abs(loss[c] - lo) <= 2e-5 * abs(lo), (ev, c, loss[c], lo)
            assert np.linalg.norm(grad[c] - go) <= 1e-5 * np.linalg.norm(go), (ev, c)
        v = prior.whiten(K)
        U_, dU, Kf, loss2, grad2, bad = f(v)
        assert np.allclose(Kf, K, rtol=1e-12, atol=1e-12) and not bad.any()
        want_dU = v + (prior.U @ grad2.T).T / 0.05 ** 2
        assert np.linalg.norm(dU - want_dU) <= 1e-12 * np.linalg.norm(want_dU), ev


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("graph", [True, False])
def test_device_chains_under_the_prior_walk_the_host_chains_path(setup, host_chain, graph, fused):
    """run_chains_device(prior=...): fused (finrom_hmc_begin + finrom_hmc_leapfrog_field + finrom_hmc_end) or torch form
    (FieldSampler.field / .pullback around grad_romml_batch), replayed as a graph or in stream order: the host chain's accept
    vector, trace, end points and recorded evaluations."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    V, phi, model, data, ro, prior, V0 = setup
    kw, want, host = host_chain
    dev = hmc.run_chains_device(_rom(setup), V0, 121, record=want, keep_trace=True, graph=graph, fused=fused, **kw)
    assert dev.fused == fused and dev.graph == graph
    assert dev.n_evals == host.n_evals == 121 and dev.proposals == host.proposals == 12
    assert 0 < host.accept.sum() < 4 * 12, host.accept
    assert np.array_equal(dev.accept, host.accept)
    assert dev.trace.shape == host.trace.shape == (13, 4, V.dim())
    assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    assert np.linalg.norm(dev.K - host.K) <= 1e-9 * np.linalg.norm(host.K)
    assert np.linalg.norm(dev.V - host.V) <= 1e-9 * np.linalg.norm(host.V)
    assert [e for e, *_ in dev.recorded] == [e for e, *_ in host.recorded]
    for (ev, K, loss, grad), (_, Kh, lossh, gradh) in zip(dev.recorded, host.recorded):
        assert np.linalg.norm(K - Kh) <= 1e-9 * np.linalg.norm(Kh), ev
        assert np.linalg.norm(grad - gradh) <= 1e-6 * np.linalg.norm(gradh), ev


def test_device_trace_is_the_field_of_the_whitened_trace(setup, host_chain):
    """keep_trace=True under the prior: the trace the device returns is prior.field of the whitened trace -- its first row is the
    field of the start points, and its last row is bitwise the end fields K (the same rows mapped by the same kernel)."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    V, phi, model, data, ro, prior, V0 = setup
    kw, want, host = host_chain
    dev = hmc.run_chains_device(_rom(setup), V0, 61, keep_trace=True, **kw)
    assert dev.fused and dev.graph and dev.trace.shape == (7, 4, V.dim())
    f0 = prior.field(V0)
    assert np.max(np.abs(dev.trace[0] - f0)) <= 1e-13 * np.max(np.abs(f0))
    assert np.array_equal(dev.trace[-1], dev.K)
    assert np.max(np.abs(dev.K - prior.field(dev.V))) <= 1e-13 * np.max(np.abs(dev.K))
    vt = prior.whiten(dev.trace)
    assert np.max(np.abs(prior.field(vt) - dev.trace)) <= 1e-12 * np.max(np.abs(dev.trace))
