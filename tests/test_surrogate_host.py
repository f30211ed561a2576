"""CPU tests of the pure deep-learning surrogate as the fourth model (model="ml"): the NumPy statement Surrogate(device=False)
against torch autograd in float64, the reference's MLSolverWrapper surface, objective("ml").host, the host chains, every argument
error, and the conditions the GPU tests rest on (tests/surrogate_cases.py: the exact case is exact, the chains' step sizes accept
some proposals and reject others).  Nothing here reaches a device."""
import numpy as np
import pytest

import mlp_cases as K
import surrogate_cases as SC


def _torch_misfit(model, X, data):
    """loss [S], d loss / d x [S, n], out [S, n_out] of 1/2 |d - NN(x)|^2 through torch ops and autograd in float64."""
    import torch
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    a = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in DeviceErrorModel.fold(model).items()}
    x = torch.from_numpy(np.asarray(X, dtype=np.float32).astype(np.float64)).requires_grad_(True)
    y = x @ a["W0"] + a["b0"]
    L = model.n_layers
    for l in range(L + 1):
        act = torch.nn.functional.elu(y * a["scale"][l] + a["shift"][l])
        y = y + act @ a["W"][l] + a["b"][l] if l < L else act @ a["Wh"] + a["bh"]
    loss = 0.5 * ((torch.from_numpy(np.broadcast_to(data, y.shape).copy()) - y) ** 2).sum(dim=1)
    loss.sum().backward()
    return loss.detach().numpy(), x.grad.numpy(), y.detach().numpy()


@pytest.mark.parametrize("shape", [(37, 17, 0, 1), (245, 50, 3, 9), (64, 50, 3, 40)], ids=str)
@pytest.mark.parametrize("per_sample", [False, True])
def test_host_surrogate_is_the_autograd_misfit(shape, per_sample):
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    n_in, n_w, L, n_out = shape
    model = K.make_model(n_in, n_w, L, n_out, seed=5)
    X = K.rom_inputs(n_in, 6, seed=1)
    data = np.random.default_rng(3).uniform(0.2, 1.0, (6, n_out) if per_sample else n_out)
    loss, grad, out = _torch_misfit(model, X, data)
    sur = Surrogate(model, device=False)
    r = sur.misfit_grad_batch(X, data)
    assert r["loss"].dtype == r["grad"].dtype == r["qoi"].dtype == np.float64 and r["info"].dtype == np.int32
    assert r["grad"].shape == (6, n_in) and r["qoi"].shape == (6, n_out) and r["loss"].shape == r["info"].shape == (6,)
    assert np.max(np.abs(r["qoi"] - out)) <= 1e-4 * np.max(np.abs(out))
    assert np.max(np.abs(r["loss"] - loss)) <= 1e-4 * np.max(np.abs(loss))
    assert np.max(np.abs(r["grad"] - grad)) <= 1e-4 * np.max(np.abs(grad))
    assert not r["info"].any()
    # the float64 reference of the GPU tests is the same misfit, to rounding
    ref, host = SC.misfit_refs(model, X, data)
    assert np.max(np.abs(ref["loss"] - loss)) <= 1e-12 * np.max(np.abs(loss))
    assert np.max(np.abs(ref["grad"] - grad)) <= 1e-12 * np.max(np.abs(grad))
    assert np.array_equal(host["grad"], r["grad"]) and np.array_equal(host["loss"], r["loss"])
    p = sur.predict_batch(X)
    assert p["loss"] is None and p["grad"] is None and p["info"] is None and np.array_equal(p["qoi"], r["qoi"])
    v = sur.misfit_grad_batch(X, data, want_grad=False)
    assert v["grad"] is None and np.array_equal(v["loss"], r["loss"])


def test_host_surrogate_flags_a_loss_that_is_not_finite():
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    model = K.make_model(20, 8, 1, 3, seed=2)
    X = K.rom_inputs(20, 3)
    X[1, 4] = np.nan
    with np.errstate(all="ignore"):
        r = Surrogate(model, device=False).misfit_grad_batch(X, np.ones(3))
    assert list(r["info"]) == [0, 1, 0] and np.isfinite(r["loss"][[0, 2]]).all()


def test_ml_solver_wrapper_is_the_references_surface(spaces):
    """cost = 1/2 |NN(z) - d|^2 + 1/2 gamma z^T K1 z, its gradient the autograd gradient + gamma K1 z; timers accumulate."""
    from bayesian_inference.estimate_MAP import MLSolverWrapper                  # (the reference's import path)
    from bayesianinferencedl_amd.bayesian_inference.estimate_MAP import unit_stiffness
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    V = spaces(4)
    solver = Fin(V)
    model = SC.hmc_model()
    data = SC.hmc_data(model)
    w = MLSolverWrapper(Surrogate(model, device=False), data, solver)
    z = SC.hmc_starts()[1]
    loss, grad, _ = _torch_misfit(model, z[None], data)
    K1 = unit_stiffness(solver.ops)
    cost = w.cost_function(z)
    assert cost == w.cost and abs(cost - (loss[0] + 0.5 * solver.gamma * z @ (K1 @ z))) <= 1e-4 * abs(cost)
    assert 0.5 * solver.gamma * z @ (K1 @ z) > 0
    g = w.gradient(z)
    assert g is w.grad and np.max(np.abs(g - (grad[0] + solver.gamma * (K1 @ z)))) <= 1e-4 * np.max(np.abs(g))
    assert w.fwd_time > 0 and w.grad_time > 0
    assert np.array_equal(w.data, data)


def test_objective_ml_host_applies_the_library_terms_in_the_librarys_order(spaces):
    from bayesianinferencedl_amd.bayesian_inference import lbfgs
    from bayesianinferencedl_amd.bayesian_inference.estimate_MAP import objective, unit_stiffness
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    solver = Fin(spaces(4))
    model = SC.hmc_model()
    data = SC.hmc_data(model)
    sur = Surrogate(model, device=False)
    X = SC.hmc_starts()
    obj = objective("ml", data, surrogate=sur, solver=solver, gamma=1e-6)
    assert obj.d == SC.N4 and obj.gmap is None and obj.tikhonov[0] == 1e-6
    f, g, bad = obj.host(X)
    raw = sur.misfit_grad_batch(X, data)
    f2, g2 = lbfgs.library_terms(X, raw["loss"], raw["grad"], None, (1e-6, unit_stiffness(solver.ops)))
    assert np.array_equal(f, f2) and np.array_equal(g, g2) and not bad.any() and np.all(f > raw["loss"])
    plain = objective("ml", data, surrogate=sur)                               # no regulariser: no solver needed
    f0, g0, _ = plain.host(X)
    assert np.array_equal(f0, raw["loss"]) and np.array_equal(g0, raw["grad"])


def test_objective_ml_argument_errors():
    from bayesianinferencedl_amd.bayesian_inference.estimate_MAP import _FILES, objective
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    sur = Surrogate(K.make_model(20, 8, 1, 3, seed=2), device=False)
    with pytest.raises(ValueError, match="surrogate="):
        objective("ml", np.ones(3))
    with pytest.raises(ValueError, match="nodal fields"):
        objective("ml", np.ones(3), surrogate=sur, params="five")
    with pytest.raises(ValueError, match="outputs"):
        objective("ml", np.ones(4), surrogate=sur)
    with pytest.raises(ValueError, match="Tikhonov"):
        objective("ml", np.ones(3), surrogate=sur, gamma=1e-6)
    with pytest.raises(ValueError, match="unknown model"):
        objective("dl", np.ones(3), surrogate=sur)
    assert _FILES["ml"] == "res_ML.npy"


def test_check_model_and_the_fused_form_refuse_what_the_issue_lists():
    """model="ml" without surrogate= or data=, surrogate= beside another model, solver= beside "ml": ValueError from both entry points
    before anything is touched; the fused form: FinromError with FINROM_ERR_UNSUPPORTED, no device needed before the raise."""
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    assert hmc.MODELS == ("romml", "rom", "fom", "ml")
    sur = Surrogate(K.make_model(20, 8, 1, 3, seed=2), device=False)
    K0, kw = np.ones((2, 20)), dict(seeds=[1, 2])
    for run in (hmc.run_chains_device, hmc.run_chains_fused):
        with pytest.raises(ValueError, match="needs surrogate="):
            run(None, K0, 7, model="ml", data=np.ones(3), **kw)
        with pytest.raises(ValueError, match="needs data="):
            run(None, K0, 7, model="ml", surrogate=sur, **kw)
        with pytest.raises(ValueError, match="surrogate= belongs to model='ml'"):
            run(None, K0, 7, model="rom", surrogate=sur, data=np.ones(3), **kw)
        with pytest.raises(ValueError, match="solver= belongs to model='fom'"):
            run(None, K0, 7, model="ml", surrogate=sur, data=np.ones(3), solver=object(), **kw)
        with pytest.raises(ValueError, match="unknown model"):
            run(None, K0, 7, model="dl", **kw)
    with pytest.raises(_ffi.FinromError, match=r"status %d\).*model='ml'" % _ffi.ERR_UNSUPPORTED):
        hmc.run_chains_fused(None, K0, 7, model="ml", surrogate=sur, data=np.ones(3), **kw)


def test_misfit_jacobian_ml_on_the_host():
    from bayesianinferencedl_amd.bayesian_inference.laplace import misfit_jacobian
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    model = K.make_model(30, 12, 2, 5, seed=4)
    k = K.rom_inputs(30, 1)[0]
    with pytest.raises(ValueError, match="surrogate="):
        misfit_jacobian("ml", k)
    J = misfit_jacobian("ml", k, surrogate=Surrogate(model, device=False))
    ref = K.vjp64(model, np.broadcast_to(k, (5, 30)), np.eye(5))
    assert J.shape == (5, 30) and np.max(np.abs(J - ref)) <= 1e-4 * np.max(np.abs(ref))


def test_load_surrogate_model_checks_the_references_sizes(tmp_path):
    from bayesianinferencedl_amd.deep_learning import dl_model as D
    D.ResBnFcModel(30, 40, 3, 50).save(tmp_path / "a.npz")
    D.ResBnFcModel(30, 9, 3, 50).save(tmp_path / "b.npz")
    D.ResBnFcModel(30, 9, 5, 50).save(tmp_path / "c.npz")
    assert D.load_surrogate_model(tmp_path / "a.npz").n_out == 40
    assert D.load_surrogate_model(tmp_path / "b.npz", randobs=False).n_out == 9
    with pytest.raises(ValueError, match="surrogate"):
        D.load_surrogate_model(tmp_path / "b.npz")
    with pytest.raises(ValueError, match="surrogate"):
        D.load_surrogate_model(tmp_path / "c.npz", randobs=False)


def test_train_surrogate_model_fits_the_references_sizes_on_the_host():
    from bayesianinferencedl_amd.deep_learning import dl_model as D
    rng = np.random.default_rng(0)
    z, zv = rng.uniform(0.5, 1.5, (40, 12)), rng.uniform(0.5, 1.5, (10, 12))
    q = lambda a: np.stack([a.mean(axis=1), a[:, 0], a[:, 1] * a[:, 2]], axis=1)
    model, hist = D.train_surrogate_model(epochs=3, batch_size=20, lr=3e-4, data=(z, q(z), zv, q(zv)), device=False)
    assert (model.n_in, model.n_out, model.n_layers, model.n_weights) == (12, 3, D.SURROGATE_LAYERS, D.SURROGATE_WIDTH) == (12, 3, 3, 50)
    assert len(hist.history["loss"]) == 3 and "val_loss" in hist.history


# ---- conditions of the GPU tests -----------------------------------------------------------------------------------------------------------
def test_the_exact_case_is_exact_in_fp32():
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    model, X, data, out, loss, grad = SC.exact_case()
    a = DeviceErrorModel.fold(model)
    assert np.all(a["scale"] == 1) and np.all(a["shift"] == 0)
    assert not np.array_equal(model.W0[:37, :37], model.W0[:37, :37].T) and not np.array_equal(a["Wh"][:40], a["Wh"][:40, :40].T)
    ref, host = SC.misfit_refs(model, X, data)
    for name, want in (("out", out), ("loss", loss), ("grad", grad)):
        assert np.array_equal(ref[name], want) and np.array_equal(host[name], want), name
        assert np.array_equal(2 * want, np.round(2 * want)) and np.max(np.abs(want)) < 2 ** 23      # (the loss: half-integers)
    assert K.forward64(model, X)[1].min() > 0                            # positive pre-activations: ELU is the identity


@pytest.fixture(scope="module")
def chain_rig(spaces):
    from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    model = SC.hmc_model()
    return Surrogate(model, device=False), SC.hmc_data(model), GaussianFieldPrior(spaces(4), amplitude=0.1, mean=1.0)


@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_the_host_chains_under_the_gpu_tests_numbers_accept_some_and_reject_some(chain_rig, field):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    sur, data, prior = chain_rig
    res = hmc.run_chains(hmc.ml_value_and_grad(sur, data), SC.hmc_starts(field=field), SC.HMC_EVALS, seeds=SC.HMC_SEEDS,
                         eps=SC.HMC_EPS["field" if field else "iid"], n_leapfrog=SC.HMC_LEAPFROG, sigma=SC.HMC_SIGMA, tau=SC.HMC_TAU,
                         keep_trace=True, prior=prior if field else None)
    print("host accepts", res.accept)
    assert res.proposals == SC.HMC_PROPOSALS and 0 < res.accept.sum() < 4 * SC.HMC_PROPOSALS, res.accept


def test_the_wide_host_chain_accepts_some_and_rejects_some(chain_rig):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    sur, data, _ = chain_rig
    res = hmc.run_chains(hmc.ml_value_and_grad(sur, data), SC.hmc_starts(SC.WIDE_C), SC.HMC_EVALS, seeds=list(range(400, 400 + SC.WIDE_C)),
                         eps=SC.HMC_EPS_WIDE, n_leapfrog=SC.HMC_LEAPFROG, sigma=SC.HMC_SIGMA, tau=SC.HMC_TAU, rng="philox")
    assert 0 < res.accept.sum() < SC.WIDE_C * SC.HMC_PROPOSALS, res.accept


def test_host_chain_with_delayed_acceptance_against_a_second_network(chain_rig):
    """run_chains(ml_value_and_grad(...), correct=): the trajectory under the surrogate, the second test under another model of the
    same observables (here a second network's misfit, value only): every final acceptance passed the first stage."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    sur, data, _ = chain_rig
    other = SC.hmc_model()
    other.head["W"] = other.head["W"] * np.float32(1.05)
    full = Surrogate(other, device=False)

    def correct(Kc):
        r = full.misfit_grad_batch(Kc, data, want_grad=False)
        return r["loss"], r["info"] != 0
    res = hmc.run_chains(hmc.ml_value_and_grad(sur, data), SC.hmc_starts(), SC.HMC_EVALS, seeds=SC.HMC_SEEDS, eps=SC.HMC_EPS["iid"],
                         n_leapfrog=SC.HMC_LEAPFROG, sigma=SC.HMC_SIGMA, tau=SC.HMC_TAU, rng="philox", correct=correct)
    assert res.n_fom == SC.HMC_PROPOSALS + 1 and np.all(res.accept1 >= res.accept) and res.accept1.sum() > 0
