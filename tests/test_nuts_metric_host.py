"""The No-U-turn transition under the Laplace metric on the CPU (nuts.py metric=, hmc.run_chains(..., nuts=Nuts(max_depth, metric=...))):
the recursive and the iterative form return the same tree under a metric; a transition under M is the identity-mass transition in
isotropic coordinates; a rank-zero metric is no metric, bit for bit; the chains sample a stiff linear-Gaussian posterior under its own
Hessian and a variant with the wrong kinetic energy does not; every refusal.  Cases: tests/nuts_metric_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

import nuts_cases as NC
import nuts_metric_cases as NM

from bayesianinferencedl_amd.bayesian_inference import hmc, nuts as N, philox
from bayesianinferencedl_amd.bayesian_inference.laplace import LowRankMetric


@functools.lru_cache(maxsize=None)
def _walks(which):
    """[(iterative, recursive)] over every transition of the potential's runs, both ranks."""
    out = []
    for *a, m in NM.host_runs(which):
        out += list(zip(NC.walk(N.transition_iterative, *a, metric=m), NC.walk(N.transition_recursive, *a, metric=m)))
    return out


@functools.lru_cache(maxsize=None)
def _iso(index):
    """[(under the metric, in isotropic coordinates, the metric)] over the transitions of NM.ISO_RUNS[index]: each chain follows its own
    states, the isotropic one from q = M^1/2 k."""
    which, rho, eps, depth = NM.ISO_RUNS[index]
    f, K0, seeds = NM.iso_potential(which)
    m = NM.metric(K0.shape[1], rho)
    under = NC.walk(N.transition_iterative, f, K0, 0.0, 1.0, NM.ISO_C_PRI, eps, depth, seeds, NM.ISO_TRANSITIONS, metric=m)
    iso = NC.walk(N.transition_iterative, NM.isotropic(f, m), m.apply(K0, "sqrt"), 0.0, 1.0, NM.ISO_C_PRI, eps, depth, seeds, NM.ISO_TRANSITIONS)
    return [(u, q, m) for u, q in zip(under, iso)]


# ---- 1. the same tree from both forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["toy", "surrogate"])
def test_the_recursive_and_the_iterative_form_agree_under_a_metric(which):
    pairs = _walks(which)
    per = NC.TOY_CHAINS * NM.TOY_TRANSITIONS * len(NM.TOY_RUNS) if which == "toy" else 4 * NM.SUR_TRANSITIONS * len(NM.SUR_RUNS)
    assert len(pairs) == per * len(NM.RHOS)
    for it, rec in pairs:
        assert np.array_equal(it.tree, rec.tree) and it.directions == rec.directions, (it.tree, rec.tree)
        assert np.max(np.abs(it.k - rec.k)) <= 1e-12 * np.max(np.abs(it.k)) and np.max(np.abs(it.dU - rec.dU)) <= 1e-12 * max(1.0, np.max(np.abs(it.dU)))
        assert abs(it.U - rec.U) <= 1e-12 * abs(it.U) and abs(it.accept_stat - rec.accept_stat) <= 1e-12
        assert 1 <= it.steps <= 2 ** it.tree[0] * 2 - 1 and 0.0 <= it.accept_stat <= 1.0
    its = [it for it, _ in pairs]
    assert {int(r.reason) for r in its} >= {0, 1, 3} and {int(r.moved) for r in its} == {0, 1}
    assert max(r.steps for r in its) >= 15                           # (trees with checkpoints of several levels)


def test_the_metric_changes_the_transition():
    """The runs above are not the identity-mass runs in disguise: the same run without the metric builds other trees."""
    *a, m = NM.host_runs("toy")[4]
    with_m, without = NC.walk(N.transition_iterative, *a, metric=m), NC.walk(N.transition_iterative, *a)
    assert any(not np.array_equal(x.tree, y.tree) for x, y in zip(with_m, without))
    assert all(not np.array_equal(x.k, y.k) for x, y in zip(with_m, without) if x.moved and y.moved)


# ---- 2. isotropic coordinates ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(NM.ISO_RUNS)), ids=["-".join(map(str, r)) for r in NM.ISO_RUNS])
def test_a_transition_under_m_is_the_identity_mass_transition_in_isotropic_coordinates(index):
    """Only rounding separates the two, amplified by at most sqrt(1 + lambda_max) = 10 over at most 15 leaves: 1e-9 relative."""
    runs = _iso(index)
    assert len(runs) == 4 * NM.ISO_TRANSITIONS
    for u, q, m in runs:
        assert np.array_equal(u.tree, q.tree) and u.directions == q.directions, (u.tree, q.tree)
        back = m.apply(q.k, "invsqrt")
        assert np.max(np.abs(back - u.k)) <= 1e-9 * np.max(np.abs(u.k))
        assert abs(u.U - q.U) <= 1e-9 * abs(u.U) and abs(u.accept_stat - q.accept_stat) <= 1e-9
        assert u.steps <= 15


def test_no_case_decides_a_comparison_closely():
    """A condition on the inputs (seeds, eps, max_depth), over ALL cases of tests 1 and 2: none is left out."""
    m1 = min(min(it.margin, rec.margin) for which in ("toy", "surrogate") for it, rec in _walks(which))
    m2 = min(min(u.margin, q.margin) for index in range(len(NM.ISO_RUNS)) for u, q, _ in _iso(index))
    print(f"NUTS metric host cases: smallest decision margin {m1:.3e} (both forms), {m2:.3e} (isotropic coordinates)")
    assert min(m1, m2) >= NC.MARGIN


# ---- 3. a rank-zero metric ---------------------------------------------------------------------------------------------------------------
def _toy_kw(**more):
    return dict(seeds=[NC.TOY_SEED0 + c for c in range(NC.TOY_CHAINS)], eps=0.12, n_leapfrog=1, sigma=1.0, tau=1.0, mean=0.0, rng="philox", **more)


def test_a_rank_zero_metric_on_nuts_gives_the_bits_of_no_metric():
    K0 = NC.toy_starts()
    zero = LowRankMetric(np.zeros((0, NC.TOY_N)), np.zeros(0))
    a = hmc.run_chains(NC.toy_value_and_grad, K0, 1 + 5, keep_trace=True, **_toy_kw(nuts=N.Nuts(5)))
    b = hmc.run_chains(NC.toy_value_and_grad, K0, 1 + 5, keep_trace=True, **_toy_kw(nuts=N.Nuts(5, metric=zero)))
    c = hmc.run_chains(NC.toy_value_and_grad, K0, 1 + 5, keep_trace=True, **_toy_kw(nuts=N.Nuts(5, metric=None)))
    for x in (b, c):
        assert np.array_equal(a.K, x.K) and np.array_equal(a.trace, x.trace) and np.array_equal(a.tree, x.tree)
        assert np.array_equal(a.accept_stat, x.accept_stat) and a.margin == x.margin and x.metric_rho == 0
    m = NM.metric(NC.TOY_N, 9)
    d = hmc.run_chains(NC.toy_value_and_grad, K0, 1 + 5, keep_trace=True, **_toy_kw(nuts=N.Nuts(5, metric=m)))
    assert d.metric_rho == 9 and not np.array_equal(d.K, a.K) and N.Nuts(5, metric=m).metric is m


def test_run_chains_under_a_prior_takes_the_metric_in_whitened_coordinates():
    """The whitened chain under Nuts(metric=) is the i.i.d. chain of the composed callable with mean 0, tau 1 and the same metric."""
    import hmc_ml_cases as MC
    K0, prior, m = NC.toy_starts(), MC.point_prior(NC.TOY_N), NM.metric(NC.TOY_N, 9)
    kw = _toy_kw(nuts=N.Nuts(4, metric=m))
    del kw["mean"]
    got = hmc.run_chains(NC.toy_value_and_grad, K0, 1 + 3, keep_trace=True, prior=prior, **kw)
    f = lambda V: (lambda r: (r[0], prior.pullback(r[1]), r[2]))(NC.toy_value_and_grad(prior.field(V)))
    same = hmc.run_chains(f, K0, 1 + 3, keep_trace=True, **dict(kw, mean=0.0, tau=1.0))
    assert got.metric_rho == 9 and np.array_equal(same.tree, got.tree) and np.allclose(same.K, got.V, rtol=1e-12, atol=1e-12)


# ---- 4. correctness ----------------------------------------------------------------------------------------------------------------------
def _lg_run(monkeypatch, broken):
    f, mean, var, m, stiff = NM.stiff_linear_gaussian()
    assert stiff >= 100.0
    if broken:                                                       # kinetic energy |p|^2 / 2 while the drift uses M^-1 p
        monkeypatch.setattr(N._Transition, "kinetic", lambda self, p, v: 0.5 * self.dot(p, p))
    K0 = np.tile(mean, (NM.LGM_CHAINS, 1)) + 0.1 * m.apply(np.random.default_rng(3).standard_normal((NM.LGM_CHAINS, NM.LGM_N)), "invsqrt")
    seeds64 = philox.check_seeds(range(900, 900 + NM.LGM_CHAINS))
    res = hmc._run_chains_nuts(f, K0, 1 + NM.LGM_TRANSITIONS, seeds64, NM.LGM_EPS, 1, NM.LGM_SIGMA, NM.LGM_TAU, 0.0, False, None, 0,
                               hmc.ChainStats(burn=NM.LGM_BURN, batch=NM.LGM_BATCH), N.Nuts(NM.LGM_DEPTH, metric=m))
    monkeypatch.undo()
    s = res.stats.summarize()
    t = res.stats.t * NM.LGM_CHAINS
    z_mean = np.abs(s.mean - mean) / s.mcse
    z_var = np.abs(s.std ** 2 - var) / (var * np.sqrt(2.0 / np.minimum(s.ess, t)))      # (as tests/test_nuts_host.py's test 6)
    return z_mean, z_var, res


def test_the_chains_sample_a_stiff_posterior_under_its_hessian_and_a_wrong_kinetic_energy_does_not(monkeypatch):
    z_mean, z_var, res = _lg_run(monkeypatch, False)
    print(f"NUTS under the metric, stiff linear-Gaussian: |mean error| / mcse {z_mean.max():.2f}, |variance error| / se {z_var.max():.2f}, "
          f"mean depth {res.tree[:, :, 0].mean():.2f}, moved {res.tree[:, :, 3].mean():.2f}, diverged {(res.tree[:, :, 2] == 3).mean():.3f}")
    assert z_mean.max() <= 4.0 and z_var.max() <= 4.0
    assert (res.tree[:, :, 2] == 3).mean() <= 0.01 and res.tree[:, :, 3].mean() >= 0.5
    b_mean, b_var, _ = _lg_run(monkeypatch, True)
    print(f"NUTS under the metric with kinetic energy |p|^2 / 2: {b_mean.max():.2f}, {b_var.max():.2f}")
    assert not (max(b_mean.max(), b_var.max()) <= 4.0)                     # the test can fail
    # what the metric is for: identity mass at the same step size diverges or does not move
    f, mean, var, m, _ = NM.stiff_linear_gaussian()
    K0 = np.tile(mean, (NM.LGM_CHAINS, 1))
    plain = hmc._run_chains_nuts(f, K0, 1 + 50, philox.check_seeds(range(900, 900 + NM.LGM_CHAINS)), NM.LGM_EPS, 1, NM.LGM_SIGMA, NM.LGM_TAU,
                                 0.0, False, None, 0, None, N.Nuts(NM.LGM_DEPTH))
    assert (plain.tree[:, :, 2] == 3).mean() >= 0.5 or plain.tree[:, :, 3].mean() <= 0.1


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason():
    K0, f = NC.toy_starts(), NC.toy_value_and_grad
    m = NM.metric(NC.TOY_N, 2)
    with pytest.raises(ValueError, match=r"metric=.*Nuts\(max_depth, metric="):      # beside nuts= the keyword is still refused
        hmc.run_chains(f, K0, 5, metric=m, **_toy_kw(nuts=N.Nuts(3)))
    with pytest.raises(ValueError, match=r"metric="):
        hmc.run_chains(f, K0, 5, metric=m, **_toy_kw(nuts=N.Nuts(3, metric=m)))
    wrong = NM.metric(NC.TOY_N - 1, 2)
    with pytest.raises(ValueError, match=r"n = 36.*37 coordinates"):
        hmc.run_chains(f, K0, 5, **_toy_kw(nuts=N.Nuts(3, metric=wrong)))
    with pytest.raises(ValueError, match=r"n = 36.*37 coordinates"):
        N.transition_iterative(f, K0[0], 0.0, K0[0], 0.0, K0[0], seed=1, proposal=0, eps=0.1, c_lik=1.0, c_pri=1.0, mean=0.0, max_depth=2,
                               metric=wrong)
    with pytest.raises(ValueError, match="LowRankMetric"):
        N.Nuts(3, metric=object())
    dkw = dict(seeds=[1, 2], rng="philox", data=np.ones(9), model="ml", surrogate=object())
    for who in (hmc.run_chains_device, hmc.run_chains_fused):      # before anything is touched
        with pytest.raises(ValueError, match=r"n = 36.*5 coordinates"):
            who(None, np.ones((2, 5)), 5, nuts=N.Nuts(3, metric=wrong), **dkw)
        with pytest.raises(ValueError, match=r"metric=.*Nuts\(max_depth, metric="):
            who(None, np.ones((2, 5)), 5, nuts=N.Nuts(3), metric=wrong, **dkw)


def test_the_entry_point_checks_its_arguments_without_a_device():
    """What finrom_hmc_nuts_ml_metric refuses before it looks at a handle's device memory: finrom_hmc_nuts_ml's checks in its order, and
    a null metric handle in front of the model's."""
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    err = L.finrom_last_error
    assert hasattr(L, "finrom_hmc_nuts_ml_metric") and L.finrom_version() == _ffi.ABI_VERSION == 12
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    st = _ffi.HmcState(C=1, n=4, eps=0.1, c_lik=1.0, c_pri=1.0, mean=p, K=p, U=p, dU=p, Kq=(ctypes.c_void_p * 2)(p, p), P=p, dUq=p, H0=p,
                       P_block=p, lu_block=p, jt=p, pt=p, accept=p, trace=None, loss=p, info=p)
    call = lambda mlp, s, seeds, p0, depth, data: L.finrom_hmc_nuts_ml_metric(mlp, s, None, seeds, p0, depth, data, 0, None, None, None)
    assert call(None, None, p, 0, 3, p) == -1 and b"hmc_nuts_ml_metric: null field" in err()
    for depth in (0, 11, -1):
        assert call(None, ctypes.byref(st), p, 0, depth, p) == -1 and b"max_depth = %d is outside 1 .. 10" % depth in err()
    assert call(None, ctypes.byref(st), p, -1, 3, p) == -1 and b"proposal0 < 0" in err()
    assert call(None, ctypes.byref(st), None, 0, 3, p) == -1 and b"null seeds" in err()
    assert call(None, ctypes.byref(st), p, 0, 3, p) == -1 and b"hmc_nuts_ml_metric: null metric handle" in err()
