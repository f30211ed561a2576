"""The No-U-turn transition on the device under the full-order model, the plain reduced model and the reduced model with its learned
correction (hmc.py model="fom" | "rom" | "romml" with nuts=; finrom_hmc_nuts_begin / _leaf / _end, one leaf per round): against the host
statement hmc.run_chains(nuts=) over the model's callable, under both priors, replayed as graphs or in stream order, any block, a
continued run, stats=, the refusals, model="ml" as before; one run at the survey mesh against the oracle.

m = 4 with the committed basis (tests/golden/fin_m4_r8.npz: n = 245, r = 8), the setting of tests/test_gpu_hmc_models.py: four chains,
seeds 100 .. 103, sigma = 0.05.  Every compared host run decides none of its comparisons closer than nuts_cases.MARGIN (asserted)."""
import os
import sys

import numpy as np
import pytest

import hmc_ml_cases as MC
import nuts_cases as NC
import surrogate_cases as SC
from oracle import fin_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fin_m4_r8.npz")
SEEDS = [100, 101, 102, 103]
MODELS = ("fom", "rom", "romml")
DEPTH, TRANSITIONS = 4, 6
EPS = {False: 0.1, True: 0.3}                                        # i.i.d., field: the step sizes of tests/test_gpu_hmc_models.py


def _nuts(depth=DEPTH, **kw):
    from bayesianinferencedl_amd.bayesian_inference.nuts import Nuts
    return Nuts(depth, **kw)


class _Setting:
    def __init__(self, problems, spaces, m, phi):
        sys.path.insert(0, ROOT)
        import bench
        from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
        from bayesianinferencedl_amd.fom.forward_solve import Fin
        from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
        self.prob, self.V = problems(m), spaces(m)
        self.n = self.V.dim()
        self.solver = Fin(self.V)
        self.phi = phi(self.solver) if callable(phi) else phi
        k_true = np.exp(0.25 * np.random.default_rng(11).standard_normal(self.n))
        self.data = self.solver.qoi_operator(self.solver.forward(k_true)[0])
        self.net = bench.hmc_error_model(self.n)
        self.rom = AffineROMFin(self.V, None, self.phi); self.rom.set_data(self.data)
        self.romml = AffineROMFin(self.V, self.net, self.phi); self.romml.set_data(self.data)
        self.ro = O.AffineROMOracle(self.prob, self.phi); self.ro.set_data(self.data)
        self.prior = GaussianFieldPrior(self.V, amplitude=0.1, mean=1.0)
        self.K0 = np.stack([np.exp(0.1 * np.random.default_rng(6 + c).standard_normal(self.n)) for c in range(4)])
        self.V0 = np.stack([np.random.default_rng(6 + c).standard_normal(self.n) for c in range(4)])
        self._host, self._dev = {}, {}

    def callable(self, model):
        from bayesianinferencedl_amd.bayesian_inference import hmc
        return {"fom": lambda: hmc.fom_value_and_grad(self.solver, self.data), "rom": lambda: hmc.rom_value_and_grad(self.rom),
                "romml": lambda: hmc.romml_value_and_grad(self.romml)}[model]()

    def kw(self, field, transitions=TRANSITIONS, depth=DEPTH, **more):
        kw = dict(seeds=SEEDS, eps=EPS[field], n_leapfrog=1, sigma=0.05, tau=0.5, rng="philox", nuts=_nuts(depth), keep_trace=True)
        if field:
            kw["prior"] = self.prior
        else:
            kw["mean"] = self.K0                                     # (explicit: a continued run keeps it)
        return 1 + transitions, dict(kw, **more)

    def host(self, model, field):
        from bayesianinferencedl_amd.bayesian_inference import hmc
        if (model, field) not in self._host:
            n_evals, kw = self.kw(field)
            self._host[(model, field)] = hmc.run_chains(self.callable(model), self.V0 if field else self.K0, n_evals, **kw)
        return self._host[(model, field)]

    def device(self, model, field, x0=None, transitions=TRANSITIONS, depth=DEPTH, **more):
        from bayesianinferencedl_amd.bayesian_inference import hmc
        key = (model, field, transitions, depth) + tuple(sorted((k, str(v)) for k, v in more.items()))
        if x0 is not None or key not in self._dev:
            n_evals, kw = self.kw(field, transitions, depth, **more)
            res = hmc.run_chains_device({"rom": self.rom, "romml": self.romml}.get(model), (self.V0 if field else self.K0) if x0 is None else x0,
                                        n_evals, model=model, solver=self.solver if model == "fom" else None, data=self.data, **kw)
            assert res.fused is True and res.model == model and res.nuts == depth and res.proposals == transitions
            if x0 is not None:
                return res
            self._dev[key] = res
        return self._dev[key]


@pytest.fixture(scope="module")
def small(problems, spaces):
    return _Setting(problems, spaces, 4, np.load(GOLDEN)["phi"])


def _same_bytes(a, b, field):
    for name in ("K", "trace", "accept", "tree", "accept_stat") + (("V",) if field else ()):
        assert np.array_equal(a[name], b[name]) and a[name].tobytes() == b[name].tobytes(), name


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "stream"])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
@pytest.mark.parametrize("model", MODELS)
def test_the_device_chains_follow_the_host_statement(small, model, field, graph):
    host = small.host(model, field)
    print(f"NUTS {model} {'field' if field else 'iid'}: host margin {host.margin:.3e}, tree rows {host.tree.reshape(-1, 4).tolist()}")
    assert host.margin >= NC.MARGIN                                  # the condition on the inputs
    dev = small.device(model, field, graph=graph)
    rel = lambda a, b: np.max(np.abs(a - b)) / np.max(np.abs(b))
    print(f"  device ({'graph' if graph else 'stream'}): trace {rel(dev.trace, host.trace):.2e}, K {rel(dev.K, host.K):.2e}, accept_stat "
          f"{np.max(np.abs(dev.accept_stat - host.accept_stat) / np.abs(host.accept_stat)):.2e}, rounds {dev.nuts_rounds}, "
          f"read-backs {dev.nuts_readbacks}")
    assert dev.graph == graph
    assert np.array_equal(dev.tree, host.tree), (dev.tree.tolist(), host.tree.tolist())
    assert np.array_equal(dev.accept, host.accept) and np.array_equal(dev.accept, dev.tree[:, :, 3].sum(axis=0))
    assert dev.trace.shape == host.trace.shape == (TRANSITIONS + 1, 4, small.n)
    assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    assert np.linalg.norm(dev.K - host.K) <= 1e-9 * np.linalg.norm(host.K)
    if field:
        assert np.linalg.norm(dev.V - host.V) <= 1e-9 * np.linalg.norm(host.V)
    assert np.max(np.abs(dev.accept_stat - host.accept_stat)) <= 1e-9 * np.max(np.abs(host.accept_stat))
    assert dev.n_evals == host.n_evals
    assert dev.tree[:, :, 3].any() and dev.tree[:, :, 0].max() > 1   # some transition moved, some tree is deeper than one doubling
    assert dev.nuts_readbacks <= DEPTH * TRANSITIONS and dev.nuts_rounds >= dev.tree[:, :, 1].max(axis=1).sum()


@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
@pytest.mark.parametrize("model", MODELS)
def test_graph_stream_and_block_give_the_same_bytes(small, model, field):
    a = small.device(model, field, graph=True)
    _same_bytes(a, small.device(model, field, graph=False), field)
    _same_bytes(small.device(model, field, graph=True, block=5), small.device(model, field, graph=True, block=32), field)
    _same_bytes(a, small.device(model, field, graph=True, block=5), field)


@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
@pytest.mark.parametrize("model", MODELS)
def test_three_and_three_transitions_are_six_to_the_byte(small, model, field):
    whole = small.device(model, field, graph=True)
    first = small.device(model, field, transitions=3, graph=True)
    second = small.device(model, field, x0=first.V if field else first.K, transitions=3, graph=True, proposal0=3)
    assert first.proposals == second.proposals == 3
    for name in ("tree", "accept_stat"):
        assert np.concatenate([first[name], second[name]]).tobytes() == whole[name].tobytes(), name
    assert np.concatenate([first.trace, second.trace[1:]]).tobytes() == whole.trace.tobytes()
    assert second.K.tobytes() == whole.K.tobytes() and (first.accept + second.accept).tobytes() == whole.accept.tobytes()
    if field:
        assert second.V.tobytes() == whole.V.tobytes()


@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
@pytest.mark.parametrize("model", MODELS)
def test_device_stats_are_the_recursion_over_the_devices_own_trace(small, model, field):
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats, stats_from_trace
    plain = small.device(model, field, graph=True)
    res = small.device(model, field, graph=True, stats=ChainStats(burn=1, batch=2))
    _same_bytes(plain, res, field)
    s, ref = res.stats, stats_from_trace(res.trace, 1, 2)
    assert (s.t, s.n_batches, s.first, s.next) == (ref.t, ref.n_batches, ref.first, ref.next) == (5, 2, 0, 6)
    for name in ChainStats.SUMS + ("cur",):
        assert getattr(s, name).tobytes() == getattr(ref, name).tobytes(), name
    assert np.array_equal(s.accepted, ref.accepted) and np.array_equal(s.accepted[1:], res.tree[:, :, 3])
    assert np.isfinite(s.misfit).all()
    stay = s.accepted[1:] == 0
    assert np.array_equal(s.misfit[1:][stay], s.misfit[:-1][stay]) and np.all(s.misfit[1:][~stay] != s.misfit[:-1][~stay])


def test_what_is_still_refused_says_so(small):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.laplace import LowRankMetric
    Vt = np.linalg.qr(np.random.default_rng(0).standard_normal((small.n, 2)))[0].T
    metric = LowRankMetric(np.ascontiguousarray(Vt), np.array([3.0, 1.0]))
    for model in MODELS:
        n_evals, kw = small.kw(False)
        args = ({"rom": small.rom, "romml": small.romml}.get(model), small.K0, n_evals)
        kw.update(model=model, solver=small.solver if model == "fom" else None, data=small.data)
        for run in (hmc.run_chains_device, hmc.run_chains_fused):
            with pytest.raises(ValueError, match=r"Nuts\(metric=\.\.\.\) with model="):
                run(*args, **dict(kw, nuts=_nuts(metric=metric)))
            with pytest.raises(ValueError, match="nuts= with record="):
                run(*args, **dict(kw, record={0}))
            if model != "fom":
                with pytest.raises(ValueError, match="nuts= with correct="):
                    run(*args, **dict(kw, correct=small.solver))
            with pytest.raises(ValueError, match="needs rng='philox'"):
                run(*args, **dict(kw, rng="numpy"))
        with pytest.raises(ValueError, match="fused=False asks for the torch-op form"):
            hmc.run_chains_device(*args, **dict(kw, fused=False))


def test_the_surrogate_keeps_its_one_launch_transition(small):
    """model="ml" with nuts= is finrom_hmc_nuts_ml as before: it reports its ml_form and the host statement's tree."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    model = SC.hmc_model()
    sur, data = Surrogate(model), SC.hmc_data(model)
    kw = MC.chain_kw(False, rng="philox", nuts=_nuts(), keep_trace=True)
    host = hmc.run_chains(hmc.ml_value_and_grad(sur, data), SC.hmc_starts(), MC.HMC_EVALS, **kw)
    dev = hmc.run_chains_device(None, SC.hmc_starts(), MC.HMC_EVALS, model="ml", surrogate=sur, data=data, ml_form="trajectory", **kw)
    assert host.margin >= NC.MARGIN
    assert dev.ml_form == "trajectory" and dev.fused is True and dev.nuts == DEPTH and "nuts_rounds" not in dev
    assert np.array_equal(dev.tree, host.tree) and np.array_equal(dev.accept, host.accept)


def test_at_the_survey_mesh_the_draws_misfit_is_the_oracles(problems, spaces):
    """m = 12, r = 81 (n = 1597), ROM + ML, Nuts(5), two transitions.  The end states are evaluated again by finrom_romml_grad, the four
    together as a round evaluates them: the misfit the chains hold is that call's, and it is the oracle's -- its reduced QoI in float64
    with the correction e_NN that call's own float32 network returned there -- within 1e-10."""
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats
    from bayesianinferencedl_amd.engine import romml_grad
    from bayesianinferencedl_amd.rom.basis import pod_basis
    s = _Setting(problems, spaces, 12, lambda solver: pod_basis(solver, 81, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1))
    res = s.device("romml", False, transitions=2, depth=5, graph=True, eps=3e-2, stats=ChainStats(burn=0, batch=1))
    print(f"NUTS romml m=12: tree rows {res.tree.reshape(-1, 4).tolist()}, rounds {res.nuts_rounds}, read-backs {res.nuts_readbacks}")
    assert res.tree[:, :, 3].any() and res.tree[:, :, 1].max() > 1 and np.all(res.tree[:, :, 2] >= 0)
    again = romml_grad(s.romml._rom, s.romml._dev_model, s.romml._avg._S, res.K, s.data)
    assert not np.any(again["info"])
    for c in range(4):
        obs = s.ro.qoi_reduced(s.ro.forward_reduced(res.K[c]))
        r = s.data - (obs + np.asarray(again["e_NN"][c], dtype=np.float64))
        want = 0.5 * float(r @ r)
        print(f"  chain {c}: misfit held {res.stats.cur_loss[c]:.15e}, evaluated again {again['loss'][c]:.15e}, oracle {want:.15e}")
        assert abs(again["loss"][c] - want) <= 1e-10 * abs(want), (c, again["loss"][c], want)
        assert abs(res.stats.cur_loss[c] - want) <= 1e-10 * abs(want), (c, res.stats.cur_loss[c], want)
