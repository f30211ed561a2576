"""The dual-averaging step-size warm-up of the No-U-turn chains on the host (bayesian_inference/nuts.py StepAdapt; hmc.py
nuts=Nuts(max_depth, adapt=StepAdapt(target_accept, tune))): the statement finrom_hmc_step_adapt_update is tested against
(tests/test_gpu_hmc_nuts_adapt.py).

(a) the recursion against an independent transcription of Hoffman & Gelman 2014, Algorithm 5 in its textbook form; (b) a deterministic
acceptance curve, so that what is tested is the recursion and not a sampler's noise; (c) tune = 0 and the tune boundary; (d) a run
continued across the boundary; (e) what is refused; and what the library's entry point refuses before any device call."""
import ctypes

import numpy as np
import pytest

import nuts_cases as NC


def _mods():
    from bayesianinferencedl_amd.bayesian_inference import hmc, nuts
    return hmc, nuts


# ---- (a) the recursion against the textbook form ---------------------------------------------------------------------------------------------
def _textbook(a, eps0, target, tune, gamma=0.05, t0=10.0, kappa=0.75):
    """Algorithm 5 as printed, for one chain: a [T] -> (H-bar [T], log eps-bar [T], the step in use after each transition [T])."""
    mu = np.log(10.0 * eps0)
    hbar, log_eps_bar, eps = 0.0, 0.0, eps0
    out = []
    for m, am in enumerate(a, start=1):
        if m <= tune:
            hbar = (1.0 - 1.0 / (m + t0)) * hbar + (target - am) / (m + t0)
            log_eps = mu - np.sqrt(m) / gamma * hbar
            eta = m ** -kappa
            log_eps_bar = eta * log_eps + (1.0 - eta) * log_eps_bar
            eps = np.exp(log_eps) if m < tune else np.exp(log_eps_bar)
        out.append((hbar, log_eps_bar, eps))
    return tuple(np.array(x) for x in zip(*out))


@pytest.mark.parametrize("target,tune,eps0", [(0.8, 150, 0.1), (0.98, 200, 0.4), (0.65, 100, 1e-3)])
def test_the_recursion_is_algorithm_5_in_its_textbook_form(target, tune, eps0):
    """200 accept_stat values per chain, exact 0.0, 1.0 and `target` among them.  Relative: to the largest magnitude the quantity
    takes along the chain (hbar and xbar pass through zero)."""
    _, N = _mods()
    C, T = 3, 200
    A = np.random.default_rng(5).uniform(0.0, 1.0, (T, C))
    A[[0, 7, 31, 120], 0], A[[1, 8, 32, 121], 0], A[[2, 9, 33, 122], 0] = 0.0, 1.0, target
    A[:40, 1], A[40:80, 2] = 1.0, 0.0                               # long runs of the extremes
    ad = N.StepAdapt(target, tune).begin(eps0, C, 0)
    assert np.array_equal(ad.eps, np.full(C, eps0)) and not ad.hbar.any() and not ad.xbar.any() and ad.mu == np.log(10.0 * eps0)
    got = []
    for p in range(T):
        ad.update(A[p], p)
        got.append((ad.hbar.copy(), ad.xbar.copy(), ad.eps.copy()))
    assert ad.next == T
    for c in range(C):
        ref = _textbook(A[:, c], eps0, target, tune)
        for q, name in enumerate(("hbar", "xbar", "eps")):
            mine = np.array([g[q][c] for g in got])
            err = np.max(np.abs(mine - ref[q])) / np.max(np.abs(ref[q]))
            assert err <= 1e-12, (name, c, err)
        assert np.all(np.array([g[2][c] for g in got])[tune - 1:] == got[tune - 1][2][c])      # frozen from t = tune on


# ---- (b) a deterministic acceptance curve ----------------------------------------------------------------------------------------------------
def _curve(eps):
    return np.exp(-4.0 * eps * eps)


@pytest.mark.parametrize("eps0", [1e-3, 0.1, 3.0])
@pytest.mark.parametrize("target", [0.65, 0.8, 0.98])
def test_the_adapted_step_meets_the_target_on_a_deterministic_acceptance_curve(target, eps0):
    """a(eps) = exp(-4 eps^2), tune = 100: a(final eps) within 0.02 of the target (worst of the nine: target 0.98 from eps0 = 3.0,
    0.9660)."""
    _, N = _mods()
    ad = N.StepAdapt(target, 100).begin(eps0, 1, 0)
    for p in range(100):
        ad.update(_curve(ad.eps), p)
    final = float(ad.eps[0])
    assert final == float(np.exp(ad.xbar[0]))
    print(f"StepAdapt target {target} eps0 {eps0}: final eps {final:.6g}, a(final) {_curve(final):.4f}")
    assert abs(_curve(final) - target) <= 0.02
    ad.update(np.array([0.0]), 100)                                  # past the warm-up: nothing moves
    assert float(ad.eps[0]) == final and ad.next == 101


def test_the_first_update_moves_the_step_up_from_full_acceptance_and_down_from_none():
    _, N = _mods()
    target, eps0 = 0.8, 0.1
    ad = N.StepAdapt(target, 100).begin(eps0, 3, 0)
    ad.update(np.array([1.0, target, 0.0]), 0)
    assert ad.eps[0] > ad.eps[1] > ad.eps[2]
    assert ad.hbar[1] == 0.0 and ad.eps[1] == np.exp(ad.mu) and np.isclose(ad.eps[1], 10.0 * eps0, rtol=1e-15)
    # a = 1: hbar = (target - 1) / 11, x = mu - hbar / gamma
    assert ad.eps[0] == np.exp(ad.mu - ((1.0 / 11.0) * (target - 1.0)) * 1.0 / 0.05)


# ---- (c) tune = 0 and the tune boundary ------------------------------------------------------------------------------------------------------
EPS, DEPTH = NC.TOY_RUNS[0]
SEEDS = [NC.TOY_SEED0 + c for c in range(NC.TOY_CHAINS)]


def _toy(transitions, nuts, K0=None, **more):
    hmc, _ = _mods()
    kw = dict(seeds=SEEDS, eps=EPS, n_leapfrog=1, sigma=1.0, tau=2.0, mean=0.0, rng="philox", keep_trace=True, nuts=nuts)
    kw.update(more)
    return hmc.run_chains(NC.toy_value_and_grad, NC.toy_starts() if K0 is None else K0, 1 + transitions, **kw)


def _same(a, b, names=("K", "trace", "tree", "accept_stat", "accept")):
    for name in names:
        assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes(), name


def test_tune_zero_is_the_run_without_adaptation_to_the_byte():
    _, N = _mods()
    plain = _toy(6, N.Nuts(DEPTH))
    zero = _toy(6, N.Nuts(DEPTH, adapt=N.StepAdapt(tune=0)))
    _same(plain, zero)
    assert "step_size" not in plain and "adapt" not in plain
    assert np.array_equal(zero.step_size, np.full((6, NC.TOY_CHAINS), EPS)) and zero.adapt.next == 6
    assert np.array_equal(zero.adapt.eps, np.full(NC.TOY_CHAINS, EPS)) and not zero.adapt.hbar.any() and not zero.adapt.xbar.any()


def test_the_step_is_frozen_at_exp_xbar_from_row_tune_on():
    _, N = _mods()
    tune = 5
    res = _toy(9, N.Nuts(DEPTH, adapt=N.StepAdapt(0.8, tune)))
    assert res.step_size.shape == (9, NC.TOY_CHAINS) and np.array_equal(res.step_size[0], np.full(NC.TOY_CHAINS, EPS))
    assert np.all(res.step_size[tune:] == res.step_size[tune]) and np.array_equal(res.step_size[tune], np.exp(res.adapt.xbar))
    assert np.array_equal(res.adapt.eps, res.step_size[tune]) and res.adapt.mu == np.log(10.0 * EPS) and res.adapt.next == 9
    assert np.all(res.step_size[1:tune] != res.step_size[tune])      # (it moved while it tuned, each chain by itself)
    assert len(set(res.step_size[tune].tolist())) == NC.TOY_CHAINS
    # the recursion over the run's own accept_stat
    ad = N.StepAdapt(0.8, tune).begin(EPS, NC.TOY_CHAINS, 0)
    for p in range(9):
        assert np.array_equal(res.step_size[p], ad.eps)
        ad.update(res.accept_stat[p], p)
    assert res.margin >= NC.MARGIN


# ---- (d) continuation across the boundary ----------------------------------------------------------------------------------------------------
def test_four_and_four_transitions_are_the_eight_to_the_byte():
    _, N = _mods()
    tune = 6
    whole = _toy(8, N.Nuts(DEPTH, adapt=N.StepAdapt(0.8, tune)))
    first = _toy(4, N.Nuts(DEPTH, adapt=N.StepAdapt(0.8, tune)))
    assert first.adapt.next == 4
    second = _toy(4, N.Nuts(DEPTH, adapt=N.StepAdapt(resume=first.adapt)), K0=first.K, proposal0=first.adapt.next)
    assert second.adapt.next == 8 and (second.adapt.tune, second.adapt.target_accept) == (tune, 0.8)
    for name in ("tree", "accept_stat", "step_size"):
        assert np.concatenate([first[name], second[name]]).tobytes() == whole[name].tobytes(), name
    assert np.concatenate([first.trace, second.trace[1:]]).tobytes() == whole.trace.tobytes()
    for name in ("eps", "hbar", "xbar"):
        assert getattr(second.adapt, name).tobytes() == getattr(whole.adapt, name).tobytes(), name
    assert second.K.tobytes() == whole.K.tobytes() and second.adapt.mu == whole.adapt.mu
    with pytest.raises(ValueError, match="ended before transition 4; this one starts at proposal0 = 3"):
        _toy(4, N.Nuts(DEPTH, adapt=N.StepAdapt(resume=first.adapt)), K0=first.K, proposal0=3)


# ---- (e) refusals ----------------------------------------------------------------------------------------------------------------------------
def test_what_step_adapt_refuses():
    hmc, N = _mods()
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="target_accept = .* is outside \\(0, 1\\)"):
            N.StepAdapt(bad, 10)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="tune = .* is not a number of transitions >= 0"):
            N.StepAdapt(0.8, bad)
    with pytest.raises(ValueError, match="resume= takes the adapt a run returned"):
        N.StepAdapt(resume=N.StepAdapt(0.8, 10))
    started = N.StepAdapt(0.9, 10).begin(0.1, 2, 0)
    with pytest.raises(ValueError, match="differ from the resumed run's 0.9, 10"):
        N.StepAdapt(0.7, 10, resume=started)
    with pytest.raises(ValueError, match="differ from the resumed run's 0.9, 10"):
        N.StepAdapt(0.8, 100, resume=started)                        # (the defaults' values, given: not the resumed run's)
    same = N.StepAdapt(0.9, resume=started)
    assert (same.target_accept, same.tune) == (0.9, 10) and (N.StepAdapt().target_accept, N.StepAdapt().tune) == (0.8, 100)
    with pytest.raises(ValueError, match="the resumed run had 2 chains, this one 3"):
        N.StepAdapt(resume=started).begin(0.1, 3, 0)
    with pytest.raises(ValueError, match="adapt= takes a StepAdapt"):
        N.Nuts(3, adapt=0.8)
    with pytest.raises(ValueError, match="transition 3 after transition -1"):
        started.update(np.zeros(2), 3)
    with pytest.raises(ValueError, match="burn=3.*the tuning draws are not draws of the target"):
        _toy(6, N.Nuts(DEPTH, adapt=N.StepAdapt(0.8, 4)), stats=hmc.ChainStats(burn=3, batch=1))
    res = _toy(6, N.Nuts(DEPTH, adapt=N.StepAdapt(0.8, 4)), stats=hmc.ChainStats(burn=4, batch=1))
    assert res.stats.t == 2


def test_the_entry_points_are_exported_and_the_update_refuses_without_a_device():
    """What finrom_hmc_step_adapt_update and the per-chain entry points refuse before any device call: the library loads without a GPU."""
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    err = L.finrom_last_error
    for name in ("finrom_hmc_step_adapt_update", "finrom_hmc_nuts_ml_adapt", "finrom_hmc_nuts_ml_metric_adapt", "finrom_hmc_nuts_begin_adapt",
                 "finrom_hmc_nuts_leaf_adapt"):
        assert hasattr(L, name) and name in _ffi.SIGNATURES
    ARG = -1
    buf = (ctypes.c_double * 8)()                                   # never dereferenced: every call below is refused, or has C = 0
    p = ctypes.addressof(buf)

    def desc(**kw):
        d = dict(eps=p, hbar=p, xbar=p, mu=0.0, target=0.8, gamma=0.05, t0=10.0, tune=10)
        d.update(kw)
        return _ffi.HmcStepAdapt(**d)

    def call(d, C=2, p0=0, pt=p, stat=p):
        return L.finrom_hmc_step_adapt_update(ctypes.byref(d) if d is not None else None, C, p0, pt, stat, None, None)
    assert call(None) == ARG and b"hmc_step_adapt_update: null descriptor" in err()
    for field in ("eps", "hbar", "xbar"):
        assert call(desc(**{field: None})) == ARG and b"null eps, hbar or xbar" in err()
    assert call(desc(tune=-1)) == ARG and b"tune < 0" in err()
    for bad in (0.0, 1.0, float("nan")):
        assert call(desc(target=bad)) == ARG and b"is outside (0, 1)" in err()
    assert call(desc(gamma=0.0)) == ARG and call(desc(t0=-1.0)) == ARG and call(desc(mu=float("inf"))) == ARG
    assert call(desc(), C=-1) == ARG and b"C < 0" in err()
    assert call(desc(), p0=-1) == ARG and b"proposal0 < 0" in err()
    assert call(desc(), pt=None) == ARG and b"null pt" in err()
    assert call(desc(), stat=None) == ARG and b"null accept_stat" in err()
    assert call(desc(), C=0, pt=None, stat=None) == 0               # C == 0: no launch
    st = _ffi.HmcState()                                             # (a null state is refused after the null eps)
    assert L.finrom_hmc_nuts_ml_adapt(None, ctypes.byref(st), None, None, 0, 3, None, 0, None, None, None) == ARG and b"hmc_nuts_ml_adapt: null eps" in err()
    assert L.finrom_hmc_nuts_ml_metric_adapt(None, ctypes.byref(st), None, None, None, 0, 3, None, 0, None, None, None) == ARG
    assert b"hmc_nuts_ml_metric_adapt: null eps" in err()
    assert L.finrom_hmc_nuts_begin_adapt(ctypes.byref(st), None, None, None, None, 0, None, None) == ARG and b"hmc_nuts_begin_adapt: null eps" in err()
    assert L.finrom_hmc_nuts_leaf_adapt(ctypes.byref(st), None, None, None, None, None, None, 0, None, None) == ARG
    assert b"hmc_nuts_leaf_adapt: null eps" in err()
    assert L.finrom_hmc_nuts_begin_adapt(ctypes.byref(st), None, p, None, None, 0, None, None) == ARG and b"hmc_nuts_begin_adapt: null field" in err()
