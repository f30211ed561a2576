"""Delayed-acceptance HMC on the device (hmc.run_chains_device / run_chains_fused correct=Fin): the fused form (finrom_hmc_end_stage1,
one finrom_fom_solve without w, finrom_hmc_end_stage2, captured with the trajectory) and the torch-op form, replayed as a graph or
in stream order, under the i.i.d. and the latent Gaussian-field prior, against the host recursion hmc.run_chains(correct=fom_value);
the full-order misfit behind `correction` against the oracle; device summaries, device draws, the refusals, correct=None.

The settings of tests/test_gpu_hmc_models.py: m = 4 with the committed basis (n = 245, r = 8), model="rom"; m = 12, r = 81 (n = 1597)
with bench.hmc_error_model, model="romml".  Four chains, 61 evaluations (6 proposals of 10 steps).

The step size (and, if none serves at sigma = 0.05, sigma = 0.1, then 0.2) is the first of _Setting.host's list at which the host
chains have at least one proposal that passes stage 1 and fails stage 2 and at least one that passes both; the scan prints what it
took and the counts per chain."""
import os
import sys

import numpy as np
import pytest

from test_gpu_hmc_models import J_TOL, SEEDS, _Setting

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fin_m4_r8.npz")
N_EVALS, N_PROP = 61, 6
EPS_LIST = (0.3, 0.2, 0.12, 0.08, 0.05, 0.03, 0.02, 0.01)
FIRST_EPS = {("small", False): 0.1, ("small", True): 0.3, ("survey", False): 0.03, ("survey", True): 0.3}   # test_gpu_hmc_models.py's
# (setting, field prior) -> (sigma, eps, stage-1 passes, accepts per chain of the 6 proposals) the scan is expected to take: every
# setting serves at sigma = 0.05 and the first step size of its list.  "small": found with the CPU oracle in the device's place
# (oracle.AffineROMOracle.grad_reduced for the trajectory, oracle.FinOracle for the correction); "survey": the host recursion's own
# counts on an MI355X (the oracle was not run at that mesh).  The scan prints its counts beside these.
EXPECTED = {("small", False): (0.05, 0.1, [0, 2, 1, 4], [0, 1, 1, 3]), ("small", True): (0.05, 0.3, [3, 3, 4, 6], [3, 0, 3, 3]),
            ("survey", False): (0.05, 0.03, [6, 6, 5, 5], [6, 5, 3, 5]), ("survey", True): (0.05, 0.3, [6, 6, 6, 6], [3, 1, 3, 2])}


class _DA:
    """A setting of test_gpu_hmc_models.py with its surrogate: the plain reduced model, or ROM + the benchmark's error model."""

    def __init__(self, name, s, model):
        from bayesianinferencedl_amd.bayesian_inference import hmc
        self.name, self.s, self.model = name, s, model
        if model == "romml":
            sys.path.insert(0, ROOT)
            import bench
            from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
            self.rom = AffineROMFin(s.V, bench.hmc_error_model(s.n), s.phi); self.rom.set_data(s.data)
            self.vg = hmc.romml_value_and_grad(self.rom)
        else:
            self.rom, self.vg = s.rom, hmc.rom_value_and_grad(s.rom)
        self.fom_value = hmc.fom_value(s.solver, s.data)
        self._host = {}

    def host(self, field, **kw):
        """(eps, sigma, host result): the host recursion at the first (sigma, eps) with both kinds of proposal (module docstring)."""
        from bayesianinferencedl_amd.bayesian_inference import hmc
        if field not in self._host:
            first = FIRST_EPS[(self.name, field)]
            for sigma in (0.05, 0.1, 0.2):
                for eps in [first] + [e for e in EPS_LIST if e < first]:
                    res = hmc.run_chains(self.vg, self.s.start(field), N_EVALS, seeds=SEEDS, eps=eps, n_leapfrog=10, sigma=sigma, tau=0.5,
                                         keep_trace=True, prior=self.s.prior if field else None, correct=self.fom_value,
                                         stats=hmc.ChainStats(1, 2), record=set(range(0, N_EVALS, 10)))
                    print(self.name, self.model, "field" if field else "iid", "sigma", sigma, "eps", eps, "stage-1 passes", res.accept1,
                          "accepts", res.accept)
                    if (res.accept1 - res.accept).sum() >= 1 and res.accept.sum() >= 1:
                        break
                else:
                    continue
                break
            else:
                pytest.fail("no (sigma, eps) gave a proposal stopped at stage 2 and an accepted one")
            print("taken:", self.name, self.model, "field" if field else "iid", "sigma", sigma, "eps", eps, "expected (sigma, eps, stage-1 "
                  "passes, accepts):", EXPECTED[(self.name, field)])
            self._host[field] = (eps, sigma, res)
        return self._host[field]

    def device(self, field, eps, sigma, x0=None, **kw):
        from bayesianinferencedl_amd.bayesian_inference import hmc
        if field:
            kw["prior"] = self.s.prior
        kw.setdefault("correct", self.s.solver)
        return hmc.run_chains_device(self.rom, self.s.start(field) if x0 is None else x0, N_EVALS, model=self.model, data=self.s.data,
                                     seeds=SEEDS, n_leapfrog=10, eps=eps, sigma=sigma, tau=0.5, **kw)


@pytest.fixture(scope="module")
def small(problems, spaces):
    return _DA("small", _Setting(problems, spaces, 4, np.load(GOLDEN)["phi"]), "rom")


@pytest.fixture(scope="module")
def survey(problems, spaces):
    from bayesianinferencedl_amd.rom.basis import pod_basis
    return _DA("survey", _Setting(problems, spaces, 12, lambda solver: pod_basis(solver, 81, n_snapshots=200, low=0.1, high=10.0,
                                                                                 params="nine", seed=1)), "romml")


def _same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def _check_against_host(d, field, dev, host, sigma, fp32=False):
    c_lik = 1.0 / sigma ** 2
    loss_s = np.stack([loss for _, _, loss, _ in host.recorded])    # the surrogate's misfit at the start and at every end point
    assert dev.model == d.model and dev.proposals == host.proposals == N_PROP and dev.n_evals == host.n_evals
    assert dev.n_fom == host.n_fom == N_PROP + 1
    assert (host.accept1 - host.accept).sum() >= 1 and host.accept.sum() >= 1
    assert np.array_equal(dev.accept, host.accept), (dev.accept, host.accept)
    assert np.array_equal(dev.accept1, host.accept1), (dev.accept1, host.accept1)
    assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    assert np.linalg.norm(dev.K - host.K) <= 1e-9 * np.linalg.norm(host.K)
    if field:
        assert np.linalg.norm(dev.V - host.V) <= 1e-9 * np.linalg.norm(host.V)
    assert dev.correction.shape == host.correction.shape == (N_PROP + 1, 4) and _same_nan(dev.correction, host.correction)
    assert loss_s.shape == host.correction.shape
    bound = 1e-9 * np.nanmax(np.abs(host.correction)) + (1e-6 * c_lik * np.abs(loss_s) if fp32 else np.zeros_like(loss_s))
    err = np.abs(dev.correction - host.correction)
    fin = ~np.isnan(err)
    print(d.name, "field" if field else "iid", "max |correction - host|", err[fin].max(), "smallest bound", bound[fin].min(),
          "max |correction|", np.nanmax(np.abs(host.correction)))
    assert np.all(err[fin] <= bound[fin]), (err, bound)


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_device_chains_walk_the_host_chains_path(small, field, fused, graph):
    """model="rom" corrected by the full-order model, fused and graph as asked: accept and accept1 equal the host's; trace, K (and V)
    within 1e-9 relative; correction within 1e-9 of its largest entry; n_fom = 7."""
    eps, sigma, host = small.host(field)
    dev = small.device(field, eps, sigma, keep_trace=True, graph=graph, fused=fused)
    assert dev.fused == fused
    assert dev.graph == graph, "HIP graph capture of the proposal failed" if graph else "graph not requested"
    _check_against_host(small, field, dev, host, sigma)


@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_fused_chains_at_the_survey_mesh(survey, field):
    """m = 12, r = 81, model="romml" (the fp32 error network: correction within 1e-9 max|correction| + 1e-6 c_lik |loss|), fused,
    graph replayed."""
    eps, sigma, host = survey.host(field)
    dev = survey.device(field, eps, sigma, keep_trace=True)
    assert dev.fused and dev.graph
    _check_against_host(survey, field, dev, host, sigma, fp32=True)


@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_the_full_order_misfit_behind_the_correction_is_the_oracles(small, field):
    """Every row of `correction`: loss_surrogate + correction / c_lik at the recorded end point (evaluations 0, 10, .. 60) is the
    oracle's 0.5 |B w - d|^2 at the recorded field to 1e-10 relative."""
    eps, sigma, _ = small.host(field)
    c_lik = 1.0 / sigma ** 2
    dev = small.device(field, eps, sigma, record=set(range(0, N_EVALS, 10)))
    assert [e for e, *_ in dev.recorded] == list(range(0, N_EVALS, 10)) and dev.n_fom == len(dev.recorded)
    s = small.s
    for q, (ev, K, loss, grad) in enumerate(dev.recorded):
        for c in range(4):
            if np.isnan(dev.correction[q, c]):
                continue
            J_ref = 0.5 * np.sum((s.fo.qoi_operator(s.fo.forward(K[c])) - s.data) ** 2)
            J = loss[c] + dev.correction[q, c] / c_lik
            assert abs(J - J_ref) <= J_TOL * abs(J_ref), (q, c, J, J_ref, loss[c])
    assert np.isfinite(dev.correction).sum() >= 4 * N_PROP          # (not a way out: at most four flagged candidates)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_device_summaries(small, field, fused):
    """stats=ChainStats(1, 2): K, accept, accept1, trace and correction are those of the call without stats=; misfit rows are the
    full-order misfit of the current state (the host's, 1e-9; unchanged across a rejected proposal); accepted sums to accept; the
    sums are stats_from_trace of the kept trace -- bit for bit under the i.i.d. prior, within test_gpu_hmc_models.py's bounds under
    the field prior (the trace is mapped to fields after the run)."""
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats, stats_from_trace
    eps, sigma, host = small.host(field)
    plain = small.device(field, eps, sigma, keep_trace=True, fused=fused)
    res = small.device(field, eps, sigma, keep_trace=True, fused=fused, stats=ChainStats(1, 2))
    assert res.fused == fused and res.graph and plain.stats is None
    for k in ("K", "accept", "accept1", "trace"):
        assert np.array_equal(res[k], plain[k]), k
    assert np.array_equal(res.correction, plain.correction, equal_nan=True)
    st, ref = res.stats, stats_from_trace(res.trace, 1, 2)
    assert (st.t, st.n_batches, st.first, st.next) == (ref.t, ref.n_batches, ref.first, ref.next) == (5, 2, 0, 6)
    assert np.array_equal(st.accepted, ref.accepted) and np.array_equal(st.accepted.sum(0), res.accept)
    assert np.isfinite(st.misfit).all() and np.max(np.abs(st.misfit - host.stats.misfit)) <= 1e-9 * np.max(np.abs(host.stats.misfit))
    stay = st.accepted[1:] == 0
    assert np.array_equal(st.misfit[1:][stay], st.misfit[:-1][stay]) and np.array_equal(st.cur_loss, st.misfit[-1])
    if field:
        assert np.max(np.abs(st.mean - ref.mean)) <= 1e-12 and np.max(np.abs(st.m2 - ref.m2)) <= 1e-12 * st.t
        assert np.max(np.abs(st.bm_mean - ref.bm_mean)) <= 1e-12 and np.max(np.abs(st.bm_m2 - ref.bm_m2)) <= 1e-12 * st.n_batches
    else:
        for k in ChainStats.SUMS + ("cur",):
            assert np.array_equal(getattr(st, k), getattr(ref, k)), k


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_device_draws_do_not_depend_on_the_block(small, field, fused):
    """rng="philox": blocks of 2 proposals reproduce one block of 32 bit for bit; the host recursion with the same stream accepts
    the same proposals at both stages."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    eps, sigma, _ = small.host(field)
    kw = dict(keep_trace=True, rng="philox", fused=fused)
    if not field:
        kw["mean"] = small.s.K0
    one = small.device(field, eps, sigma, **kw)
    cut = small.device(field, eps, sigma, block=2, **kw)
    for k in ("K", "accept", "accept1", "trace"):
        assert np.array_equal(one[k], cut[k]), k
    assert np.array_equal(one.correction, cut.correction, equal_nan=True)
    host = hmc.run_chains(small.vg, small.s.start(field), N_EVALS, seeds=SEEDS, eps=eps, n_leapfrog=10, sigma=sigma, tau=0.5, rng="philox",
                          prior=small.s.prior if field else None, mean=None if field else small.s.K0, correct=small.fom_value)
    print("philox", "field" if field else "iid", "stage-1 passes", host.accept1, "accepts", host.accept)
    assert np.array_equal(one.accept, host.accept) and np.array_equal(one.accept1, host.accept1)


def test_refusals(small):
    """correct= with model="fom" and with ChainStats(resume=...): ValueError.  metric= with correct=: fused=None takes the torch-op
    form (and walks the host chain's path), fused=True raises FinromError."""
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats
    from bayesianinferencedl_amd.bayesian_inference.laplace import LowRankMetric
    s = small.s
    eps, sigma, _ = small.host(False)
    with pytest.raises(ValueError, match="nothing to correct"):
        hmc.run_chains_device(None, s.K0, N_EVALS, model="fom", solver=s.solver, data=s.data, seeds=SEEDS, correct=s.solver)
    first = small.device(False, eps, sigma, rng="philox", mean=s.K0, stats=ChainStats(0, 1))
    with pytest.raises(ValueError, match="resume"):
        small.device(False, eps, sigma, x0=first.K, rng="philox", mean=s.K0, proposal0=N_PROP, stats=ChainStats(resume=first.stats))
    again = small.device(False, eps, sigma, x0=first.K, rng="philox", mean=s.K0, proposal0=N_PROP, stats=ChainStats(N_PROP, 1))
    assert again.proposals == N_PROP and again.stats.first == N_PROP  # (proposal0 works as before: the start is evaluated anew)
    eps, sigma, _ = small.host(True)
    rng = np.random.default_rng(4)
    metric = LowRankMetric(np.ascontiguousarray(np.linalg.qr(rng.standard_normal((s.n, 3)))[0].T), np.array([0.5, 4.0, 20.0]))
    dev = small.device(True, eps, sigma, metric=metric, fused=None, keep_trace=True)
    assert dev.fused is False and dev.n_fom == N_PROP + 1
    host = hmc.run_chains(small.vg, s.V0, N_EVALS, seeds=SEEDS, eps=eps, n_leapfrog=10, sigma=sigma, prior=s.prior, metric=metric,
                          keep_trace=True, correct=small.fom_value)
    assert np.array_equal(dev.accept, host.accept) and np.array_equal(dev.accept1, host.accept1)
    assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    with pytest.raises(_ffi.FinromError, match="no metric form"):
        small.device(True, eps, sigma, metric=metric, fused=True)


def test_the_default_is_unchanged(small):
    """correct=None passed explicitly equals the call without the argument bit for bit, model="romml", fused and graph replayed."""
    sys.path.insert(0, ROOT)
    import bench
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    s = small.s
    rom = AffineROMFin(s.V, bench.hmc_error_model(s.n), s.phi); rom.set_data(s.data)
    kw = dict(seeds=SEEDS, eps=0.03, n_leapfrog=10, keep_trace=True, model="romml")
    a = hmc.run_chains_device(rom, s.K0, N_EVALS, **kw)
    b = hmc.run_chains_device(rom, s.K0, N_EVALS, correct=None, **kw)
    assert a.fused and b.fused and a.graph and b.graph and set(a) == set(b) and "correction" not in a
    assert np.array_equal(a.K, b.K) and np.array_equal(a.accept, b.accept) and np.array_equal(a.trace, b.trace)
