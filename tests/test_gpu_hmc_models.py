"""The device-resident HMC chains under the full-order model and the plain reduced model (hmc.py model="fom" | "rom"): the fused steps
(finrom_hmc_leapfrog_fom / _field_fom / _rom) and the torch-op form, replayed as a graph or in stream order, under the i.i.d. prior
and the latent Gaussian-field prior, against the host recursion hmc.run_chains over the model's host callable and, at recorded
evaluations, against the oracle (the bounds of tests/test_gpu_parity.py for the same calls); device draws, device summaries and
the continuation rule; the metric's fall-back; the default model unchanged.

m = 4 with the committed basis (tests/golden/fin_m4_r8.npz: n = 245, r = 8); one case per model at m = 12, r = 81 (n = 1597)."""
import os
import sys

import numpy as np
import pytest

from oracle import fin_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fin_m4_r8.npz")
SEEDS = [100, 101, 102, 103]
WANT = {0, 1, 10, 55, 120}
# (model, prior) -> (eps, accept counts of the 12 proposals found with the CPU oracle in the device's place): the step size the
# scan for chains that both accept and reject starts at; the host chains' own counts are printed beside them
ORACLE_ACCEPTS = {("fom", False): (0.1, [7, 12, 5, 10]), ("rom", False): (0.1, [8, 9, 9, 9]),
                  ("fom", True): (0.3, [12, 12, 11, 11]), ("rom", True): (0.3, [11, 12, 11, 11])}
J_TOL = 1e-10
G_TOL = {"fom": 1e-9, "rom": 1e-8}


class _Setting:
    def __init__(self, problems, spaces, m, phi):
        from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
        from bayesianinferencedl_amd.fom.forward_solve import Fin
        from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
        self.prob, self.V = problems(m), spaces(m)
        self.n = self.V.dim()
        self.solver = Fin(self.V)
        self.phi = phi(self.solver) if callable(phi) else phi
        k_true = np.exp(0.25 * np.random.default_rng(11).standard_normal(self.n))
        self.data = self.solver.qoi_operator(self.solver.forward(k_true)[0])
        self.rom = AffineROMFin(self.V, None, self.phi); self.rom.set_data(self.data)
        self.fo = O.FinOracle(self.prob)
        self.ro = O.AffineROMOracle(self.prob, self.phi); self.ro.set_data(self.data)
        self.prior = GaussianFieldPrior(self.V, amplitude=0.1, mean=1.0)
        self.K0 = np.stack([np.exp(0.1 * np.random.default_rng(6 + c).standard_normal(self.n)) for c in range(4)])
        self.V0 = np.stack([np.random.default_rng(6 + c).standard_normal(self.n) for c in range(4)])
        self._host = {}

    def callable(self, model):
        from bayesianinferencedl_amd.bayesian_inference import hmc
        return hmc.fom_value_and_grad(self.solver, self.data) if model == "fom" else hmc.rom_value_and_grad(self.rom)

    def start(self, field):
        return self.V0 if field else self.K0

    def device(self, model, field, n_evals, x0=None, **kw):
        from bayesianinferencedl_amd.bayesian_inference import hmc
        if field:
            kw["prior"] = self.prior
        return hmc.run_chains_device(self.rom if model == "rom" else None, self.start(field) if x0 is None else x0, n_evals, model=model,
                                     solver=self.solver if model == "fom" else None, data=self.data, seeds=SEEDS, n_leapfrog=10,
                                     sigma=0.05, tau=0.5, **kw)

    def host(self, model, field, n_evals=121, want=WANT, first_eps=None):
        """(eps, host result): the host recursion at the first step size whose chains accept some proposals and reject others."""
        from bayesianinferencedl_amd.bayesian_inference import hmc
        key = (model, field, n_evals)
        if key not in self._host:
            first = first_eps if first_eps is not None else ORACLE_ACCEPTS[(model, field)][0]
            n_prop = (n_evals - 1) // 10
            for eps in [first] + [e for e in (0.3, 0.2, 0.12, 0.08, 0.05, 0.03, 0.02, 0.01) if e < first]:
                res = hmc.run_chains(self.callable(model), self.start(field), n_evals, seeds=SEEDS, eps=eps, n_leapfrog=10, sigma=0.05, tau=0.5,
                                     record=want, keep_trace=True, prior=self.prior if field else None)
                if 0 < res.accept.sum() < 4 * n_prop:
                    break
            else:
                pytest.fail("no step size gave both accepted and rejected proposals: %s" % res.accept)
            print(model, "field" if field else "iid", "eps", eps, "host accepts", res.accept, "oracle chains:", ORACLE_ACCEPTS.get((model, field)))
            self._host[key] = (eps, res)
        return self._host[key]

    def positive_definite(self, model, k):
        """Whether the oracle's operator at the field k -- the full-order one, or the reduced one at its sub-fin averages -- is."""
        A = self.prob.assemble_fom(k).toarray() if model == "fom" else self.phi.T @ (self.prob.assemble_affine(self.prob.S @ k) @ self.phi)
        return bool(np.isfinite(A).all() and np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0)

    def check_oracle(self, model, recorded, chains=range(4)):
        """Every recorded evaluation of the listed chains against the oracle at the issue's bounds.  An evaluation the model flagged
        (a chain that stepped to a field whose operator cannot be factored: loss NaN, the proposal is rejected) has no value to
        compare -- the oracle's LU solve does not look at definiteness; there the oracle's operator must indeed not be positive
        definite, and at every other point it must be."""
        flagged = 0
        for ev, K, loss, grad in recorded:
            for c in chains:
                if not np.isfinite(loss[c]):
                    assert not self.positive_definite(model, K[c]), (model, ev, c, "flagged, but the oracle's operator is positive definite")
                    flagged += 1
                    continue
                if self.n < 1000:
                    assert self.positive_definite(model, K[c]), (model, ev, c)
                if model == "fom":
                    g_ref = self.fo.gradient(K[c], self.data)
                    J_ref = 0.5 * np.sum((self.fo.qoi_operator(self.fo.forward(K[c])) - self.data) ** 2)
                else:
                    g_ref, J_ref = self.ro.grad_reduced(K[c])
                assert abs(loss[c] - J_ref) <= J_TOL * abs(J_ref), (model, ev, c, loss[c], J_ref)
                assert np.linalg.norm(grad[c] - g_ref) <= G_TOL[model] * np.linalg.norm(g_ref), (model, ev, c)
        assert flagged <= 1, (model, flagged)                        # (not a way out: at most one of the 20 compared points)
        return flagged


@pytest.fixture(scope="module")
def small(problems, spaces):
    return _Setting(problems, spaces, 4, np.load(GOLDEN)["phi"])


@pytest.fixture(scope="module")
def survey(problems, spaces):
    from bayesianinferencedl_amd.rom.basis import pod_basis
    return _Setting(problems, spaces, 12, lambda solver: pod_basis(solver, 81, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1))


def _check_against_host(s, model, field, dev, host, n_prop):
    assert dev.model == model
    assert dev.n_evals == host.n_evals and dev.proposals == host.proposals == n_prop
    assert 0 < host.accept.sum() < 4 * n_prop, host.accept            # some accepted, some rejected
    assert np.array_equal(dev.accept, host.accept), (dev.accept, host.accept)
    assert dev.trace.shape == host.trace.shape == (n_prop + 1, 4, s.n)
    assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    assert np.linalg.norm(dev.K - host.K) <= 1e-9 * np.linalg.norm(host.K)
    if field:
        assert np.linalg.norm(dev.V - host.V) <= 1e-9 * np.linalg.norm(host.V)
    assert [e for e, *_ in dev.recorded] == [e for e, *_ in host.recorded]
    for (ev, K, loss, grad), (_, Kh, lossh, gradh) in zip(dev.recorded, host.recorded):
        assert np.linalg.norm(K - Kh) <= 1e-9 * np.linalg.norm(Kh), ev
        assert np.array_equal(np.isfinite(loss), np.isfinite(lossh)), (ev, loss, lossh)      # the same evaluations flagged


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
@pytest.mark.parametrize("model", ["fom", "rom"])
def test_device_chains_walk_the_host_chains_path(small, model, field, fused, graph):
    """121 evaluations (12 proposals of 10 steps), four chains: fused and graph as asked; the host chain's accept vector; its end
    points and kept trace within 1e-9 relative (tests/test_gpu_hmc.py's bound for the same comparison); the recorded evaluations
    0, 1, 10, 55, 120 -- at points the chains' own gradients produced -- against the oracle: J 1e-10, gradient 1e-9 (FOM) / 1e-8 (ROM);
    blocks of 5 proposals (5, 5, 2) reproduce one block of 32 bit for bit.
    Under the i.i.d. prior at eps = 0.1 the full-order chains accept [6, 11, 5, 10] where chains over the oracle accept [7, 12, 5,
    10]: chains 0 and 1 each propose one field with a conductivity below zero, whose operator the device's Cholesky factorisation
    refuses (info != 0: rejected) and the oracle's LU solve does not; chain 0's is evaluation 120 (_Setting.check_oracle)."""
    eps, host = small.host(model, field)
    dev = small.device(model, field, 121, eps=eps, record=WANT, keep_trace=True, graph=graph, fused=fused)
    assert dev.fused == fused
    assert dev.graph == graph, "HIP graph capture of the proposal failed" if graph else "graph not requested"
    _check_against_host(small, model, field, dev, host, 12)
    assert len(dev.recorded) == len(WANT)
    small.check_oracle(model, dev.recorded)
    cut = small.device(model, field, 121, eps=eps, keep_trace=True, graph=graph, fused=fused, block=5)
    assert np.array_equal(cut.accept, dev.accept) and np.array_equal(cut.trace, dev.trace) and np.array_equal(cut.K, dev.K)


@pytest.mark.parametrize("model,field", [("fom", False), ("rom", False), ("rom", True)], ids=["fom-iid", "rom-iid", "rom-field"])
def test_fused_chains_at_the_survey_mesh(survey, model, field):
    """m = 12, r = 81 (n = 1597: seven workgroups per chain in the kick, seven strides in the drift), fused and graph on, 61
    evaluations: the checks of the small mesh, the oracle on two chains."""
    want = {0, 1, 10, 55}
    eps, host = survey.host(model, field, 61, want, first_eps=0.3 if field else 0.03)
    dev = survey.device(model, field, 61, eps=eps, record=want, keep_trace=True)
    assert dev.fused and dev.graph
    _check_against_host(survey, model, field, dev, host, 6)
    survey.check_oracle(model, dev.recorded, chains=(0, 2))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
@pytest.mark.parametrize("model", ["fom", "rom"])
def test_device_draws_and_device_summaries(small, model, field, fused):
    """rng="philox" and stats=ChainStats(burn=2, batch=3), graph replayed: K, accept and trace bit-identical to the same call without
    stats=; the host recursion with the same stream walks the same path (1e-9, equal accepts); the device's sums against
    stats_from_trace of the kept trace -- bit for bit under the i.i.d. prior, where the sums see the position buffer the trace row
    is copied from; under the field prior the trace is mapped to fields after the run in one launch over all rows while the sums
    see one chain-batch launch per proposal: mean 1e-12 absolute, m2 1e-12 t (tests/test_gpu_hmc_stats.py's bounds); accepted sums
    to accept; the misfit stays across a rejected proposal."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats, stats_from_trace
    eps = small.host(model, field)[0]
    kw = dict(eps=eps, keep_trace=True, rng="philox", graph=True, fused=fused)
    if not field:
        kw["mean"] = small.K0
    plain = small.device(model, field, 121, **kw)
    res = small.device(model, field, 121, stats=ChainStats(2, 3), **kw)
    assert res.fused == fused and res.graph and res.proposals == 12 and plain.stats is None
    assert np.array_equal(res.K, plain.K) and np.array_equal(res.accept, plain.accept) and np.array_equal(res.trace, plain.trace)
    host = hmc.run_chains(small.callable(model), small.start(field), 121, seeds=SEEDS, eps=eps, n_leapfrog=10, sigma=0.05, tau=0.5,
                          keep_trace=True, rng="philox", prior=small.prior if field else None, mean=None if field else small.K0)
    print(model, "field" if field else "iid", "fused", fused, "accept", res.accept)
    assert 0 < res.accept.sum() < 4 * 12
    assert np.array_equal(res.accept, host.accept)
    assert np.max(np.abs(res.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    s, ref = res.stats, stats_from_trace(res.trace, 2, 3)
    assert (s.t, s.n_batches, s.first, s.next) == (ref.t, ref.n_batches, ref.first, ref.next) == (10, 3, 0, 12)
    if field:
        dm, d2 = np.max(np.abs(s.mean - ref.mean)), np.max(np.abs(s.m2 - ref.m2))
        print("max |mean - ref|", dm, "max |m2 - ref|", d2)
        assert dm <= 1e-12 and d2 <= 1e-12 * s.t
        assert np.max(np.abs(s.bm_mean - ref.bm_mean)) <= 1e-12 and np.max(np.abs(s.bm_m2 - ref.bm_m2)) <= 1e-12 * s.n_batches
        assert np.max(np.abs(s.mean - 1.0)) < 1.0                    # fields around the prior's mean 1, not whitened states around 0
    else:
        for k in ChainStats.SUMS + ("cur",):
            assert np.array_equal(getattr(s, k), getattr(ref, k)), k
    assert np.array_equal(s.accepted, ref.accepted) and np.array_equal(s.accepted.sum(0), res.accept) and np.isfinite(s.misfit).all()
    stay = s.accepted[1:] == 0
    assert np.array_equal(s.misfit[1:][stay], s.misfit[:-1][stay]) and np.array_equal(s.cur_loss, s.misfit[-1])


@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
@pytest.mark.parametrize("model", ["fom", "rom"])
def test_fused_chains_continue_from_their_end_state(small, model, field):
    """rng="philox", fused, graph: 6 proposals, then 6 more from the end state with proposal0=6 and stats=ChainStats(resume=...),
    against one run of 12 -- equal accept sums per chain, end states within 1e-9 (tests/test_gpu_hmc_rng.py's bound), and the
    continued sums those of the whole run within the bounds of test_device_draws_and_device_summaries."""
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats
    eps = small.host(model, field)[0]
    kw = dict(eps=eps, rng="philox", graph=True, fused=True)
    if not field:
        kw["mean"] = small.K0
    end = "V" if field else "K"
    whole = small.device(model, field, 121, stats=ChainStats(2, 3), **kw)
    one = small.device(model, field, 61, stats=ChainStats(2, 3), **kw)
    two = small.device(model, field, 61, x0=one[end], proposal0=6, stats=ChainStats(resume=one.stats), **kw)
    assert one.proposals == two.proposals == 6 and one.stats.next == 6 and two.stats.next == 12
    assert np.array_equal(one.accept + two.accept, whole.accept)
    assert np.linalg.norm(two[end] - whole[end]) <= 1e-9 * np.linalg.norm(whole[end])
    assert np.linalg.norm(two.K - whole.K) <= 1e-9 * np.linalg.norm(whole.K)
    a, b = two.stats, whole.stats
    assert (a.t, a.n_batches, a.first, a.next) == (b.t, b.n_batches, b.first, b.next)
    assert np.array_equal(a.accepted, b.accepted)
    assert np.max(np.abs(a.mean - b.mean)) <= 1e-12 and np.max(np.abs(a.m2 - b.m2)) <= 1e-12 * b.t


def test_a_metric_takes_the_torch_form(small):
    """No metric forms of the new fused steps: metric= with model="rom" and fused=None runs the torch-op form; fused=True raises
    FinromError; the chains under the metric accept the proposals the host recursion accepts."""
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.laplace import LowRankMetric
    rng = np.random.default_rng(4)
    metric = LowRankMetric(np.ascontiguousarray(np.linalg.qr(rng.standard_normal((small.n, 3)))[0].T), np.array([0.5, 4.0, 20.0]))
    eps = small.host("rom", True)[0]
    dev = small.device("rom", True, 61, eps=eps, metric=metric, fused=None, keep_trace=True)
    assert dev.fused is False and dev.model == "rom" and dev.proposals == 6
    host = hmc.run_chains(small.callable("rom"), small.V0, 61, seeds=SEEDS, eps=eps, n_leapfrog=10, sigma=0.05, prior=small.prior, metric=metric,
                          keep_trace=True)
    assert np.array_equal(dev.accept, host.accept)
    assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    with pytest.raises(_ffi.FinromError, match="no metric form"):
        small.device("rom", True, 61, eps=eps, metric=metric, fused=True)
    with pytest.raises(_ffi.FinromError, match="no metric form"):
        small.device("fom", True, 61, eps=eps, metric=metric, fused=True)


def test_the_default_model_is_unchanged(small):
    """model="romml" given explicitly equals the default call bit for bit (K, accept, trace): the form fused=None picks, and torch-op."""
    sys.path.insert(0, ROOT)
    import bench
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    rom = AffineROMFin(small.V, bench.hmc_error_model(small.n), small.phi); rom.set_data(small.data)
    kw = dict(seeds=SEEDS, eps=0.03, n_leapfrog=10, keep_trace=True)
    for fused in (None, False):
        a = hmc.run_chains_device(rom, small.K0, 61, fused=fused, **kw)
        b = hmc.run_chains_device(rom, small.K0, 61, fused=fused, model="romml", **kw)
        assert a.fused == b.fused and (fused is None or not a.fused) and a.model == b.model == "romml"
        assert np.array_equal(a.K, b.K) and np.array_equal(a.accept, b.accept) and np.array_equal(a.trace, b.trace)
