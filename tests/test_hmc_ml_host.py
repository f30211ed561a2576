"""CPU tests of the fused chains under the pure deep-learning surrogate (hmc.py model="ml" with ml_form=; csrc/hmc_ml.hip): the
whitening of the first layer as an identity of float64 arithmetic, every refusal of ml_form with no device present, the conditions
the GPU tests rest on (tests/hmc_ml_cases.py: the shapes reach the branches they name, the chains' numbers accept some proposals and
reject others on the whitened surrogate) and the two entry points' checks that need no device.  Nothing here reaches a device."""
import numpy as np
import pytest

import hmc_ml_cases as MC
import mlp_cases as K
import surrogate_cases as SC


# ---- whitening ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def priors(spaces):
    return {MC.N4: MC.prior4(spaces(4)), 37: MC.point_prior(37)}


@pytest.mark.parametrize("n", [MC.N4, 37])
def test_the_whitened_model_at_v_is_the_model_at_the_field(priors, n):
    """dtype=float64: misfit64 of the whitened model at v = misfit64 of the original at prior.field(v), gradient = prior.pullback of
    the field-space gradient, both to 1e-12 relative; the float32 model is the cast of the float64 one, entry for entry; everything
    behind the first layer is shared."""
    from bayesianinferencedl_amd.deep_learning.dl_model import whiten_first_layer
    prior = priors[n]
    model = K.make_model(n, 50 if n == MC.N4 else 17, 3 if n == MC.N4 else 0, 9, seed=31)
    data = np.random.default_rng(2).uniform(0.2, 1.0, 9)
    V = np.random.default_rng(3).standard_normal((5, n))
    w64 = whiten_first_layer(model, prior, dtype=np.float64)
    assert w64.W0.dtype == w64.b0.dtype == np.float64 and w64.W0.shape == model.W0.shape and w64.b0.shape == model.b0.shape
    loss_v, grad_v = MC.misfit64(w64, V, data)
    loss_k, grad_k = MC.misfit64(model, prior.field(V), data)
    assert np.max(np.abs(loss_v - loss_k)) <= 1e-12 * np.max(np.abs(loss_k))
    want = prior.pullback(grad_k)
    assert np.max(np.abs(grad_v - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.max(np.abs(want)) > 0 and not np.allclose(prior.field(V), V)
    w32 = whiten_first_layer(model, prior)
    assert w32.W0.dtype == w32.b0.dtype == np.float32
    assert np.array_equal(w32.W0, w64.W0.astype(np.float32)) and np.array_equal(w32.b0, w64.b0.astype(np.float32))
    for w in (w32, w64):
        assert w.units is model.units and w.head is model.head
        assert (w.n_in, w.n_out, w.n_layers, w.n_weights) == (model.n_in, model.n_out, model.n_layers, model.n_weights)
    assert model.W0.dtype == np.float32 and not np.array_equal(model.W0, w32.W0)        # the original is untouched


def test_whiten_first_layer_refuses_a_prior_of_another_size(priors):
    from bayesianinferencedl_amd.deep_learning.dl_model import whiten_first_layer
    with pytest.raises(ValueError, match="nodes"):
        whiten_first_layer(K.make_model(40, 8, 1, 3), priors[37])


def test_surrogate_whitened_keeps_the_device_setting_and_evaluates_the_field(priors):
    """Surrogate.whitened on the host: the fp32 statement at v against the original at the field, to fp32 accuracy."""
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    prior = priors[MC.N4]
    model = SC.hmc_model()
    data = SC.hmc_data(model)
    sur = Surrogate(model, device=False)
    w = sur.whitened(prior)
    assert isinstance(w, Surrogate) and w.device is False and w.n_in == MC.N4 and w.n_out == 9
    V = SC.hmc_starts(field=True)
    a, b = w.misfit_grad_batch(V, data), sur.misfit_grad_batch(prior.field(V), data)
    assert np.max(np.abs(a["loss"] - b["loss"])) <= 1e-4 * np.max(np.abs(b["loss"]))
    want = prior.pullback(b["grad"])
    assert np.max(np.abs(a["grad"] - want)) <= 1e-4 * np.max(np.abs(want))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_ml_form_is_raised_with_no_device_present():
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.laplace import LowRankMetric
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    assert hmc.MODELS == ("romml", "rom", "fom", "ml")
    sur = Surrogate(K.make_model(20, 8, 1, 3, seed=2), device=False)
    K0 = np.ones((2, 20))
    kw = dict(seeds=[1, 2], surrogate=sur, data=np.ones(3))
    for run in (hmc.run_chains_device, hmc.run_chains_fused):
        with pytest.raises(ValueError, match="unknown ml_form"):
            run(None, K0, 7, model="ml", ml_form="fused", **kw)
        with pytest.raises(ValueError, match="ml_form= belongs to model='ml'"):
            run(object(), K0, 7, model="rom", ml_form="steps", seeds=[1, 2], data=np.ones(3))
        for form in hmc.ML_FORMS:
            Vt = np.linalg.qr(np.random.default_rng(1).standard_normal((20, 2)))[0].T
            with pytest.raises(_ffi.FinromError, match=r"status %d\).*no metric form" % _ffi.ERR_UNSUPPORTED):
                run(None, K0, 7, model="ml", ml_form=form, metric=LowRankMetric(Vt, np.array([2.0, 0.5])), **kw)
            with pytest.raises(ValueError, match=r"data must be \[3\]"):
                run(None, K0, 7, model="ml", ml_form=form, seeds=[1, 2], surrogate=sur, data=np.ones(4))
    for form in hmc.ML_FORMS:
        with pytest.raises(ValueError, match="fused=False"):
            hmc.run_chains_device(None, K0, 7, model="ml", ml_form=form, fused=False, **kw)
    # without ml_form everything is as it was: the refusal of the fused form and its message
    with pytest.raises(_ffi.FinromError, match=r"status %d\).*model='ml' has no fused leapfrog step" % _ffi.ERR_UNSUPPORTED):
        hmc.run_chains_fused(None, K0, 7, model="ml", **kw)
    with pytest.raises(_ffi.FinromError, match=r"status %d\).*model='ml' has no fused leapfrog step" % _ffi.ERR_UNSUPPORTED):
        hmc.run_chains_fused(None, K0, 7, model="ml", ml_form=None, **kw)


def test_the_entry_points_refuse_null_arguments_without_a_device():
    """A null state, a state with null fields, a null handle: FINROM_ERR_ARG with the entry point's name, before any device call."""
    import ctypes as C
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    err = L.finrom_last_error
    st = _ffi.HmcState(C=2, n=8, eps=0.1, c_lik=1.0, c_pri=1.0)
    p = C.c_void_p(8)                                                     # (never dereferenced)
    assert L.finrom_hmc_leapfrog_ml(None, None, 0, p, 0, None, None, None) == -1 and b"hmc_leapfrog_ml: null field" in err()
    assert L.finrom_hmc_leapfrog_ml(p, C.byref(st), 0, p, 0, None, None, None) == -1 and b"hmc_leapfrog_ml: null field" in err()
    assert L.finrom_hmc_trajectory_ml(None, None, 3, p, 0, None) == -1 and b"hmc_trajectory_ml: null field" in err()
    assert L.finrom_hmc_trajectory_ml(p, C.byref(st), 3, p, 0, None) == -1 and b"hmc_trajectory_ml: null field" in err()
    assert _ffi.ABI_VERSION == 12 and L.finrom_version() == 12


# ---- conditions of the GPU tests -----------------------------------------------------------------------------------------------------------
def test_the_kernel_shapes_reach_the_branches_they_are_chosen_for():
    assert [MC.owned(s[0]) for s in MC.SHAPES] == [{0, 1}, {0, 1}, {1, 2}, {2, 3}]
    chunks = {s[0]: K.forward_chunks(s[0]) for s in MC.SHAPES}
    assert all(full == 0 and mid == 0 and 2 <= tail <= 3 for full, mid, tail in chunks[37])        # scalar tails alone
    assert set(chunks[245]) == {(0, 0, 15), (0, 1, 0)}                                           # a batch of 16, or 15 scalar rows
    assert set(chunks[1100]) == {(2, 0, 4), (2, 0, 5)} and set(chunks[2049]) == {(4, 0, 0), (4, 0, 1)}      # batches of 32, with and without tails
    assert [K.layer_loops(s[1]) for s in MC.SHAPES] == [(1, 1), (3, 2), (4, 0), (3, 2)]
    assert {s[2] for s in MC.SHAPES} == {0, 1, 3} and {s[3] for s in MC.SHAPES} == {9, 40}
    assert all(s[0] <= K.FORWARD_MAX_IN and s[1] <= K.MLP_MAX_W for s in MC.SHAPES)
    assert {st & 1 for st in MC.STEPS} == {0, 1} and max(MC.CHAINS) > 64


@pytest.fixture(scope="module")
def chain_rig(spaces):
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    model = SC.hmc_model()
    return Surrogate(model, device=False), SC.hmc_data(model), MC.prior4(spaces(4))


@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_the_host_chains_under_the_gpu_tests_numbers_accept_some_and_reject_some(chain_rig, field):
    """Under the prior the chain of the GPU tests is the host chain on the WHITENED surrogate, mean 0 and tau 1."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    sur, data, prior = chain_rig
    x0 = SC.hmc_starts(field=field)
    kw = MC.chain_kw(field)
    if field:
        kw.update(mean=0.0, tau=1.0)
        sur = sur.whitened(prior)
    res = hmc.run_chains(hmc.ml_value_and_grad(sur, data), x0, MC.HMC_EVALS, **kw)
    print("host accepts", res.accept)
    assert res.proposals == MC.HMC_PROPOSALS and 0 < res.accept.sum() < len(x0) * MC.HMC_PROPOSALS, res.accept


def test_the_wide_host_chain_accepts_some_and_rejects_some(chain_rig):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    sur, data, _ = chain_rig
    res = hmc.run_chains(hmc.ml_value_and_grad(sur, data), SC.hmc_starts(MC.WIDE_C), MC.HMC_EVALS, seeds=list(range(400, 400 + MC.WIDE_C)),
                         eps=MC.HMC_EPS_WIDE, n_leapfrog=MC.HMC_LEAPFROG, sigma=MC.HMC_SIGMA, tau=MC.HMC_TAU, rng="philox")
    assert 0 < res.accept.sum() < MC.WIDE_C * MC.HMC_PROPOSALS, res.accept


def test_the_whitened_host_chain_is_the_host_chain_under_the_prior(chain_rig):
    """run_chains on surrogate.whitened(prior) with mean 0 and tau 1, mapped through prior.field, against run_chains(prior=) on the
    original: the same potential up to the fp32 rounding of the folded first layer -- the same accept counts and nearby end states
    under the GPU tests' numbers (what lets the device tests compare against the whitened host statement)."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    sur, data, prior = chain_rig
    V0 = SC.hmc_starts(field=True)
    kw = MC.chain_kw(True)
    a = hmc.run_chains(hmc.ml_value_and_grad(sur.whitened(prior), data), V0, MC.HMC_EVALS, **dict(kw, mean=0.0, tau=1.0))
    b = hmc.run_chains(hmc.ml_value_and_grad(sur, data), V0, MC.HMC_EVALS, prior=prior, **kw)
    assert np.array_equal(a.accept, b.accept)
    assert np.linalg.norm(prior.field(a.K) - b.K) <= 1e-3 * np.linalg.norm(b.K)
