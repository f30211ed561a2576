"""Delayed-acceptance HMC on the host (hmc.run_chains correct=, philox.draw_block_stage2): exactness for the full-order posterior on
a linear-Gaussian toy whose surrogate is wrong on purpose, the decision rule against its bit-reproducible restatement
(hmc_da_cases.ref_stage2), correct=None as a no-op, the second Philox uniform, and the new entry points' argument checks (host-side:
no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import hmc_da_cases as D
from bayesianinferencedl_amd.bayesian_inference import hmc, philox

SEEDS = list(range(200, 264))
EPS, L, PROPOSALS = 0.3, 5, 600


def _run(toy, correct, **kw):
    return hmc.run_chains(toy["value_and_grad"], np.zeros((64, 3)), 1 + PROPOSALS * L, seeds=SEEDS, eps=EPS, n_leapfrog=L,
                          sigma=toy["sigma"], tau=toy["tau"], rng="philox", keep_trace=True, correct=correct, **kw)


@pytest.fixture(scope="module")
def toy():
    return D.toy()


@pytest.fixture(scope="module")
def corrected(toy):
    return _run(toy, toy["correct"])


def test_the_corrected_chain_samples_the_full_order_posterior(toy, corrected):
    """64 chains, 600 proposals of 5 steps at eps = 0.3, burn 100, batches of 25.  With correct=: every coordinate of the pooled mean
    within 4 Monte-Carlo standard errors (summarize()'s) of the exact full-order posterior mean, every pooled standard deviation
    within 5 % of the exact one.  The same chains without correct= sample the surrogate's posterior: more than 20 standard errors
    off in at least one coordinate."""
    res = corrected
    assert res.proposals == PROPOSALS and res.n_fom == PROPOSALS + 1 and res.correction.shape == (PROPOSALS + 1, 64)
    assert np.array_equal(res.accept, (res.stage == 2).sum(0)) and np.array_equal(res.accept1, (res.stage >= 1).sum(0))
    s = hmc.stats_from_trace(res.trace, 100, 25).summarize()
    z = np.abs(s.mean - toy["mean"]) / s.mcse
    print("corrected: |mean - exact| / mcse", z, "std ratio", s.std / toy["std"], "stage-1 rate", res.accept1.mean() / PROPOSALS,
          "final rate", res.accept.mean() / PROPOSALS, "ess", s.ess)
    assert np.all(z <= 4.0), z
    assert np.all(np.abs(s.std / toy["std"] - 1.0) <= 0.05), s.std / toy["std"]
    plain = _run(toy, None)
    assert "correction" not in plain and "accept1" not in plain
    p = hmc.stats_from_trace(plain.trace, 100, 25).summarize()
    zp = np.abs(p.mean - toy["mean"]) / p.mcse
    print("uncorrected: |mean - exact| / mcse", zp)
    assert np.max(zp) > 20.0, zp


def test_ref_stage2_is_the_decision_rule(toy, corrected):
    """hmc_da_cases.ref_stage2 -- include/finrom.h's statement, every operation reproducible to the bit -- replayed over the toy's
    chain: from the kept trace (the state before each proposal), the stage-1 flags, the surrogate's and the full-order model's
    values at each end point, it decides every proposal as run_chains(correct=) did, and its D is the recorded correction."""
    res = corrected
    c_lik = 1.0 / toy["sigma"] ** 2
    ends, calls = [], []

    def vg(K):
        out = toy["value_and_grad"](K)
        ends.append((K.copy(), out[0].copy()))
        return out

    def correct(K):
        calls.append(K.copy())
        return toy["correct"](K)
    n_prop = 40
    again = hmc.run_chains(vg, np.zeros((64, 3)), 1 + n_prop * L, seeds=SEEDS, eps=EPS, n_leapfrog=L, sigma=toy["sigma"], tau=toy["tau"],
                           rng="philox", keep_trace=True, correct=correct)
    assert np.array_equal(again.trace, res.trace[:n_prop + 1]) and np.array_equal(again.stage, res.stage[:n_prop])
    assert len(calls) == n_prop + 1 and len(ends) == 1 + n_prop * L
    Dcur = again.correction[0].copy()
    loss_f = toy["correct"](calls[0])[0]
    accept, accept1 = np.zeros(64, np.int64), np.zeros(64, np.int64)
    for q in range(n_prop):
        Kend, loss_s = ends[(q + 1) * L]
        assert np.array_equal(Kend, calls[q + 1])                    # the correcting model sees the trajectory's end point
        state = dict(K=again.trace[q], U=np.zeros(64), dU=np.zeros((64, 3)), dUq=np.zeros((64, 3)), Kq0=Kend, Kq1=Kend, c_lik=c_lik,
                     loss=loss_s, accept=accept, jt=0, pt=q)
        da = dict(ok1=(again.stage[q] >= 1).astype(np.int32), Uq=np.zeros(64), qoi_f=Kend @ toy["A"].T, info_f=np.zeros(64, np.int32),
                  data=toy["d"], lu2_block=philox.draw_block_stage2(SEEDS, q, 1), D=Dcur, loss_f=loss_f, accept1=accept1)
        ref = D.ref_stage2(state, da, 0)
        assert np.array_equal(ref["ok"], again.stage[q] == 2), q
        assert np.array_equal(ref["trace_row"], again.trace[q + 1]), q
        assert np.allclose(ref["correction_row"], again.correction[q + 1], rtol=0, atol=1e-12 * c_lik), q
        Dcur, loss_f, accept, accept1 = ref["D"], ref["loss_f"], ref["accept"], ref["accept1"]
    assert np.array_equal(accept, again.accept) and np.array_equal(accept1, again.accept1)
    assert (again.stage == 1).any() and (again.stage == 2).any() and (again.stage == 0).any()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_correct_none_is_a_no_op(toy, rng):
    """correct=None gives the bits of a call without the argument."""
    kw = dict(seeds=SEEDS[:5], eps=EPS, n_leapfrog=L, sigma=toy["sigma"], tau=toy["tau"], rng=rng, keep_trace=True,
              stats=hmc.ChainStats(2, 3))
    a = hmc.run_chains(toy["value_and_grad"], np.zeros((5, 3)), 101, **kw)
    b = hmc.run_chains(toy["value_and_grad"], np.zeros((5, 3)), 101, correct=None, **kw)
    assert set(a) == set(b) and np.array_equal(a.K, b.K) and np.array_equal(a.accept, b.accept) and np.array_equal(a.trace, b.trace)
    assert np.array_equal(a.stats.mean, b.stats.mean) and np.array_equal(a.stats.misfit, b.stats.misfit)


def test_the_numpy_stream_draws_the_second_uniform_behind_the_first(toy):
    """rng="numpy" with correct=: per proposal n normals, the first uniform, the second uniform, from the chain's own generator --
    drawn whatever stage 1 said.  Replayed by hand over ref_stage2's rule, the flags are run_chains'."""
    res = hmc.run_chains(toy["value_and_grad"], np.zeros((3, 3)), 1 + 30 * L, seeds=[7, 8, 9], eps=EPS, n_leapfrog=L, sigma=toy["sigma"],
                         tau=toy["tau"], correct=toy["correct"], keep_trace=True, stats=hmc.ChainStats(0, 5))
    gens = [np.random.default_rng(s) for s in (7, 8, 9)]
    lu2 = np.zeros((30, 3))
    for q in range(30):
        for c, r in enumerate(gens):
            r.standard_normal(3); r.uniform()
            lu2[q, c] = np.log(r.uniform())
    moved = np.any(res.trace[1:] != res.trace[:-1], axis=2)
    assert np.array_equal(moved, res.stage == 2) and np.array_equal(res.stats.accepted[1:], moved.astype(np.int32))
    Dq, Dcur = res.correction[1:], res.correction[0].copy()
    for q in range(30):
        ok = (res.stage[q] >= 1) & (lu2[q] < Dcur - Dq[q])
        assert np.array_equal(ok, res.stage[q] == 2), q
        Dcur = np.where(ok, Dq[q], Dcur)
    # stats' misfit is the correcting model's, at the current state
    assert np.allclose(res.stats.misfit, np.stack([toy["correct"](k)[0] for k in res.trace]), rtol=1e-12, atol=0)


def test_the_second_philox_uniform():
    """draw_block_stage2: finite and <= 0; differs from the first uniform at every (seed, p); a function of (seed, p) alone -- a
    block cut at any point equals the uncut block, and so does any order of the chains."""
    seeds = [0, 1, 200, 2 ** 32 + 5, 2 ** 64 - 1]
    for first in (0, 7, 2 ** 33 + 5):
        whole = philox.draw_block_stage2(seeds, first, 12)
        assert whole.shape == (12, 5) and np.isfinite(whole).all() and (whole <= 0).all()
        assert np.all(whole != philox.draw_block(seeds, first, 12, 1)[1])
        for cut in range(13):
            parts = [philox.draw_block_stage2(seeds, first, cut), philox.draw_block_stage2(seeds, first + cut, 12 - cut)]
            assert np.array_equal(np.concatenate(parts), whole), (first, cut)
        assert np.array_equal(philox.draw_block_stage2(seeds[::-1], first, 12), whole[:, ::-1])
    assert philox.draw_block_stage2(seeds, 3, 0).shape == (0, 5)
    assert len(np.unique(philox.draw_block_stage2(seeds, 0, 12))) == 60


def test_refusals_on_the_host(toy):
    """A flagged or non-finite start of the correcting model, and ChainStats(resume=...) with correct=: ValueError."""
    kw = dict(seeds=[1, 2], eps=EPS, n_leapfrog=L, sigma=toy["sigma"], tau=toy["tau"])
    with pytest.raises(ValueError, match="start point"):
        hmc.run_chains(toy["value_and_grad"], np.zeros((2, 3)), 11, correct=lambda K: (np.ones(2), np.array([False, True])), **kw)
    with pytest.raises(ValueError, match="start point"):
        hmc.run_chains(toy["value_and_grad"], np.zeros((2, 3)), 11, correct=lambda K: (np.array([1.0, np.nan]), np.zeros(2, bool)), **kw)
    first = hmc.run_chains(toy["value_and_grad"], np.zeros((2, 3)), 11, rng="philox", stats=hmc.ChainStats(0, 1), **kw)
    with pytest.raises(ValueError, match="resume"):
        hmc.run_chains(toy["value_and_grad"], first.K, 11, rng="philox", proposal0=2, mean=np.zeros((2, 3)),
                       stats=hmc.ChainStats(resume=first.stats), correct=toy["correct"], **kw)


def test_entry_points_validate_their_arguments_before_any_device_call():
    """finrom_hmc_end_stage1 / _stage2 / finrom_hmc_draw_stage2: FINROM_ERR_ARG with a message for a state with null fields, a null
    descriptor, negative counts, a null pointer with work to do; B = 0 or C = 0 returns 0 -- host-side checks, no GPU needed."""
    from bayesianinferencedl_amd import _ffi
    Lb = _ffi.lib()
    st = _ffi.HmcState(C=2, n=8, eps=0.1, c_lik=1.0, c_pri=1.0)
    da = _ffi.HmcDa(n_obs=9)
    assert Lb.finrom_hmc_end_stage1(C.byref(st), 10, None, None, None) == -1 and b"null field" in Lb.finrom_last_error()
    assert Lb.finrom_hmc_end_stage2(C.byref(st), 10, C.byref(da), None) == -1 and b"null field" in Lb.finrom_last_error()
    assert Lb.finrom_hmc_end_stage1(None, 10, None, None, None) == -1 and Lb.finrom_hmc_end_stage2(None, 10, None, None) == -1
    assert Lb.finrom_hmc_draw_stage2(None, -1, 0, 1, None, None) == -1 and b"C < 0" in Lb.finrom_last_error()
    assert Lb.finrom_hmc_draw_stage2(None, 1, 0, -1, None, None) == -1 and b"B < 0" in Lb.finrom_last_error()
    assert Lb.finrom_hmc_draw_stage2(None, 1, -1, 1, None, None) == -1 and b"first_proposal < 0" in Lb.finrom_last_error()
    assert Lb.finrom_hmc_draw_stage2(None, 2, 0, 3, None, None) == -1 and b"null seeds or lu2_block" in Lb.finrom_last_error()
    assert Lb.finrom_hmc_draw_stage2(None, 0, 0, 3, None, None) == 0 and Lb.finrom_hmc_draw_stage2(None, 4, 0, 0, None, None) == 0
