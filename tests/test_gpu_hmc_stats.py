"""The chains' posterior summaries accumulated on the device (finrom_hmc_stats_update, hmc.py stats=): the kernel alone against
ChainStats.update over a scripted run, bit for bit and inside its buffers; chains in every form against stats_from_trace of their own
trace; the cut into blocks and the continuation; under the prior and the metric; and against the host recursion -- at the fixture
sizes of tests/test_gpu_hmc_rng.py (m = 12, r = 81, 4 chains)."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 5                              # elements of NaN (integers: SENTINEL) kept behind each buffer's end
SENTINEL = -7777
SUMS = ("mean", "m2", "bsum", "bm_mean", "bm_m2")
# 11 proposals: the first one rejected, two rejections in a row (twice), acceptances in a row; chain c plays it rotated by 3 c
SCRIPT = [0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 0]
BURN, BATCH, PROPOSAL0 = 2, 3, 5


def _padded(a):
    import torch
    a = np.ascontiguousarray(a)
    fill = float("nan") if a.dtype == np.float64 else SENTINEL
    t = torch.full((a.size + PAD,), fill, dtype=torch.float64 if a.dtype == np.float64 else getattr(torch, a.dtype.name), device="cuda")
    t[:a.size].copy_(torch.from_numpy(a.reshape(-1)))
    return t


def _unpad(t, like, what):
    out = t.cpu().numpy()
    tail = out[like.size:]
    assert len(tail) == PAD and (np.isnan(tail).all() if out.dtype == np.float64 else (tail == SENTINEL).all()), f"{what}: written behind its end"
    return out[:like.size].reshape(like.shape)


def _play(C, n):
    """The script through the ABI and through ChainStats.update: (device arrays by name, host ChainStats, final accept counters)."""
    import torch
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats, stats_from_trace
    L = _ffi.lib()
    rng = np.random.default_rng(1000 * C + n)
    # proposals 0 .. 4 happened in an earlier run (burn = 2: three draws, one closed batch): the sums start non-zero
    before = np.cumsum(rng.standard_normal((PROPOSAL0 + 1, C, n)), axis=0)
    prev = stats_from_trace(before, BURN, BATCH, loss=rng.random((PROPOSAL0 + 1, C)))
    P = len(SCRIPT)
    host = ChainStats(resume=prev).begin(before[-1], prev.cur_loss, PROPOSAL0, P)
    row0 = host._row
    acc = 3 + np.arange(C, dtype=np.int64)                            # the counters need not start at zero
    host_arrays = dict(cur=host.cur, cur_loss=host.cur_loss, acc_prev=np.stack([acc, np.full(C, -1)]),
                       misfit=np.concatenate([host.cur_loss[None], np.full((P, C), np.nan)]),
                       accepted=np.concatenate([np.zeros((1, C), np.int32), np.full((P, C), SENTINEL, np.int32)]),
                       **{k: getattr(host, k) for k in SUMS})
    dev = {k: _padded(v) for k, v in host_arrays.items()}
    pt, acc_t = _padded(np.zeros(1, np.int64)), _padded(acc)
    cand, cand_loss = _padded(np.zeros((C, n))), _padded(np.zeros(C))
    desc = _ffi.HmcStats(C=C, n=n, proposal0=PROPOSAL0, burn=BURN, batch=BATCH, pt=pt.data_ptr(), accept=acc_t.data_ptr(),
                         cand=cand.data_ptr(), cand_loss=cand_loss.data_ptr(), **{k: t.data_ptr() for k, t in dev.items()})
    stream = torch.cuda.current_stream().cuda_stream
    for q in range(1, P + 1):
        ok = np.array([SCRIPT[(q - 1 + 3 * c) % P] for c in range(C)], dtype=bool)
        x, lo = rng.standard_normal((C, n)) + 2.0, rng.random(C)
        acc = acc + ok
        pt[:1].fill_(q)
        acc_t[:C].copy_(torch.from_numpy(acc))
        cand[:C * n].copy_(torch.from_numpy(x.reshape(-1)))
        cand_loss[:C].copy_(torch.from_numpy(lo))
        _ffi.check(L.finrom_hmc_stats_update(ctypes.byref(desc), stream), "finrom_hmc_stats_update")
        host.update(x, lo, ok, PROPOSAL0 + q - 1)
    torch.cuda.synchronize()
    out = {k: _unpad(t, host_arrays[k], k) for k, t in dev.items()}
    for t, like, what in ((pt, np.zeros(1), "pt"), (acc_t, acc, "accept"), (cand, x, "cand"), (cand_loss, lo, "cand_loss")):
        _unpad(t, like, what)
    return out, host, row0, acc, (desc, dev)


def _check_script(C, n):
    out, host, row0, acc, _ = _play(C, n)
    assert host.t == 14 and host.n_batches == 4
    for k in SUMS + ("cur", "cur_loss"):
        assert np.array_equal(out[k], getattr(host, k)), k
    assert np.array_equal(out["misfit"], host.misfit[row0:]) and np.array_equal(out["accepted"][1:], host.accepted[row0 + 1:])
    assert not out["accepted"][0].any()                               # (row 0 is the caller's: the start)
    assert out["accepted"][1:].min() == 0 and out["accepted"][1:].max() == 1 and not out["accepted"][1, 0]
    assert np.array_equal(out["acc_prev"][len(SCRIPT) & 1], acc)      # the slot the last launch wrote
    assert np.array_equal(acc - out["acc_prev"][1 - (len(SCRIPT) & 1)], out["accepted"][-1])


@pytest.mark.parametrize("C,n", [(1, 1), (3, 2), (2, 255), (2, 256), (4, 257), (2, 515), (4, 1597)])
def test_kernel_plays_the_script_bit_for_bit_inside_its_buffers(C, n):
    """11 proposals (first rejected, rejections in a row), burn = 2, batch = 3, proposal0 = 5, sums continued from an earlier run:
    every output equals ChainStats.update's, bit for bit; n below, at and above one and two workgroups of 256; the 5 elements
    behind every buffer's end untouched."""
    _check_script(C, n)


def test_kernel_at_the_largest_shape():
    """(C, n) = (64, 4101): 17 workgroups per chain, the last one 5 threads wide."""
    _check_script(64, 4101)


def test_argument_checks_launch_nothing():
    """Every refused call returns FINROM_ERR_ARG with a message and leaves the buffers as they were."""
    import torch
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    out, host, row0, acc, (desc, dev) = _play(3, 2)
    fields = {f: getattr(desc, f) for f, _ in _ffi.HmcStats._fields_}
    bad = [dict(C=-1), dict(n=0), dict(batch=0), dict(burn=-1), dict(proposal0=-1), dict(mean=None), dict(pt=None), dict(cand=None)]
    for change in bad:
        d = _ffi.HmcStats(**{**fields, **change})
        assert L.finrom_hmc_stats_update(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == -1, change
        assert L.finrom_last_error().decode().startswith("hmc_stats_update:"), change
    assert L.finrom_hmc_stats_update(ctypes.byref(_ffi.HmcStats(**{**fields, "C": 0})), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for k, t in dev.items():
        assert np.array_equal(t.cpu().numpy()[:out[k].size].reshape(out[k].shape), out[k], equal_nan=True), k


# ---- chains ----------------------------------------------------------------------------------------------------------------------
CHAIN_SEEDS = [100, 101, 102, 103]
EPS = 3e-2


@pytest.fixture(scope="module")
def setup(problems, spaces):
    """tests/test_gpu_hmc_rng.py's setting (m = 12, r = 81, bench.hmc_error_model, test_gpu_metric.py's prior)."""
    sys.path.insert(0, ROOT)
    import bench
    from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    from bayesianinferencedl_amd.rom.basis import pod_basis
    m, r = 12, 81
    V = spaces(m)
    solver = Fin(V)
    phi = pod_basis(solver, r, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1)
    model = bench.hmc_error_model(V.dim())
    k_true = np.exp(0.25 * np.random.default_rng(11).standard_normal(V.dim()))
    data = solver.qoi_operator(solver.forward(k_true)[0])
    rom = AffineROMFin(V, model, phi); rom.set_data(data)
    K0 = np.stack([np.exp(0.1 * np.random.default_rng(6 + c).standard_normal(V.dim())) for c in range(4)])
    prior = GaussianFieldPrior(V, amplitude=0.1, mean=1.0)
    return rom, K0, prior


def _iid(setup, n_evals=141, **kw):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    rom, K0, _ = setup
    kw = {**dict(seeds=CHAIN_SEEDS, eps=EPS, n_leapfrog=10, keep_trace=True, rng="philox", mean=K0), **kw}
    return hmc.run_chains_device(rom, kw.pop("x0", K0), n_evals, **kw)


def _same_sums(a, b, names=SUMS + ("cur", "accepted")):
    assert (a.t, a.n_batches, a.first, a.next) == (b.t, b.n_batches, b.first, b.next)
    for k in names:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.fixture(scope="module")
def fused_whole(setup):
    """Fused, graph, one block, burn = 3, batch = 2: shared by the cases below."""
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats
    return _iid(setup, graph=True, fused=True, stats=ChainStats(3, 2))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("graph", [True, False])
def test_chains_stats_are_the_recursion_over_their_own_trace(setup, fused_whole, graph, fused):
    """14 proposals, rng="philox", burn = 3, batch = 2: res.stats equals stats_from_trace of the run's own trace bit for bit; K, accept
    and trace are bit-identical to the same call without stats=; accepted sums to accept, misfit stays across a rejected proposal
    and moves with an accepted one (the chains both accept and reject: asserted)."""
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats, stats_from_trace
    plain = _iid(setup, graph=graph, fused=fused)
    res = fused_whole if (graph and fused) else _iid(setup, graph=graph, fused=fused, stats=ChainStats(3, 2))
    assert plain.stats is None and res.fused == fused and res.graph == graph and res.proposals == 14
    assert np.array_equal(res.K, plain.K) and np.array_equal(res.accept, plain.accept) and np.array_equal(res.trace, plain.trace)
    s = res.stats
    print("fused", fused, "graph", graph, "accept", res.accept)
    assert 0 < res.accept.sum() < 4 * 14
    _same_sums(s, stats_from_trace(res.trace, 3, 2))
    assert s.t == 11 and s.n_batches == 5 and s.misfit.shape == s.accepted.shape == (15, 4)
    assert np.array_equal(s.accepted.sum(0), res.accept) and np.isfinite(s.misfit).all()
    stay = s.accepted[1:] == 0
    assert np.array_equal(s.misfit[1:][stay], s.misfit[:-1][stay]) and np.all(s.misfit[1:][~stay] != s.misfit[:-1][~stay])
    assert np.array_equal(s.cur_loss, s.misfit[-1])


def test_fused_stats_do_not_depend_on_the_cut_and_continue(setup, fused_whole):
    """block=5 against block=32: identical stats.  7 proposals, then resume= with proposal0=7 for 7 more: the stats of the run of 14,
    bit for bit -- with burn = 3, batch = 2 (the cut falls on a batch's end: draws 4 of 11) and with burn = 2, batch = 2 (the cut
    falls inside a batch: 5 draws, the open batch's sum is carried over)."""
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats
    names = SUMS + ("cur", "cur_loss", "misfit", "accepted")
    cut = _iid(setup, graph=True, fused=True, block=5, stats=ChainStats(3, 2))
    _same_sums(cut.stats, fused_whole.stats, names)
    for burn, whole in ((3, fused_whole), (2, _iid(setup, graph=True, fused=True, stats=ChainStats(2, 2)))):
        one = _iid(setup, 71, graph=True, fused=True, stats=ChainStats(burn, 2))
        two = _iid(setup, 71, graph=True, fused=True, x0=one.K, proposal0=7, stats=ChainStats(resume=one.stats))
        assert one.stats.next == 7 and one.stats.t == 7 - burn and np.any(one.stats.bsum != 0.0) == (burn == 2)
        _same_sums(two.stats, whole.stats, names)
        assert np.array_equal(two.K, whole.K)


@pytest.fixture(scope="module")
def metric(setup):
    from bayesianinferencedl_amd.bayesian_inference.laplace import gauss_newton_map, reduced_value_grad_jac
    rom, _, prior = setup
    return gauss_newton_map(reduced_value_grad_jac(rom, "romml"), prior, 0.05)["metric"]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("form", ["prior", "prior+metric"])
def test_stats_under_the_prior_are_of_fields(setup, metric, form, fused):
    """prior=GaussianFieldPrior (eps = 0.1, starts v ~ N(0, I)) and prior + metric in tests/test_gpu_metric.py's setting (sigma = 0.05,
    starts from the Laplace approximation, eps = 0.3, 121 evaluations), graph replayed.  The stats see the step's field buffer (one
    chain-batch launch); the trace is mapped to fields after the run in one launch over all rows, so the two are compared within
    mean 1e-12 absolute and m2 1e-12 t (fields are O(1); the maxima are printed).  misfit[0] is the start point's misfit
    (evaluation 0, recorded); misfit stays across a rejected proposal."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats, stats_from_trace
    rom, _, prior = setup
    if form == "prior":
        x0 = np.stack([np.random.default_rng(6 + c).standard_normal(prior.n) for c in range(4)])
        kw = dict(eps=0.1)
    else:
        x0 = np.stack([metric.draw(np.random.default_rng(6 + c).standard_normal(prior.n)) for c in range(4)])
        kw = dict(eps=0.3, sigma=0.05, metric=metric)
    kw.update(seeds=CHAIN_SEEDS, n_leapfrog=10, prior=prior, keep_trace=True, rng="philox", graph=True, fused=fused, record={0})
    plain = hmc.run_chains_device(rom, x0, 121, **kw)
    res = hmc.run_chains_device(rom, x0, 121, stats=ChainStats(3, 2), **kw)
    assert res.fused == fused and res.graph and res.proposals == 12
    assert np.array_equal(res.V, plain.V) and np.array_equal(res.accept, plain.accept) and np.array_equal(res.trace, plain.trace)
    s, ref = res.stats, stats_from_trace(res.trace, 3, 2)
    dm, d2 = np.max(np.abs(s.mean - ref.mean)), np.max(np.abs(s.m2 - ref.m2))
    print(form, "fused", fused, "accept", res.accept, "max |mean - ref|", dm, "max |m2 - ref|", d2, "cur", np.max(np.abs(s.cur - ref.cur)),
          "bm_mean", np.max(np.abs(s.bm_mean - ref.bm_mean)), "bm_m2", np.max(np.abs(s.bm_m2 - ref.bm_m2)))
    assert s.t == ref.t == 9 and s.n_batches == 4
    assert dm <= 1e-12 and d2 <= 1e-12 * s.t
    assert np.max(np.abs(s.bm_mean - ref.bm_mean)) <= 1e-12 and np.max(np.abs(s.bm_m2 - ref.bm_m2)) <= 1e-12 * s.n_batches
    assert np.array_equal(s.accepted, ref.accepted) and np.array_equal(s.accepted.sum(0), res.accept)
    assert np.max(np.abs(s.mean - 1.0)) < 1.0                        # fields around the prior's mean 1, not whitened states around 0
    (ev, _, loss0, _), = res.recorded
    assert ev == 0 and np.array_equal(s.misfit[0], loss0)
    stay = s.accepted[1:] == 0
    assert np.array_equal(s.misfit[1:][stay], s.misfit[:-1][stay])


def test_device_stats_against_the_host_recursion(setup, fused_whole):
    """run_chains(romml_value_and_grad(rom), stats=) against the fused device run: the two traces agree to 1e-9 max|trace|
    (tests/test_gpu_hmc_rng.py's bound), so with d = 1e-9 max|trace| the means (averages of the draws) agree to d, and the sums of
    squared deviations, whose derivative with respect to a draw is 2 (x - mean), |x - mean| <= 2 max|trace|, to 4 max|trace| d per
    draw; the misfits to 2e-5 relative (tests/test_gpu_hmc.py's bound for a loss); equal accept flags."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats
    rom, K0, _ = setup
    host = hmc.run_chains(hmc.romml_value_and_grad(rom), K0, 141, seeds=CHAIN_SEEDS, eps=EPS, n_leapfrog=10, keep_trace=True, rng="philox",
                          stats=ChainStats(3, 2))
    h, s = host.stats, fused_whole.stats
    M = np.max(np.abs(host.trace))
    d = 1e-9 * M
    print("mean", np.max(np.abs(s.mean - h.mean)) / d, "m2", np.max(np.abs(s.m2 - h.m2)) / (4 * M * d * h.t), "(in units of the bound)",
          "misfit", np.max(np.abs(s.misfit - h.misfit) / np.abs(h.misfit)))
    assert (s.t, s.n_batches) == (h.t, h.n_batches) == (11, 5)
    assert np.array_equal(s.accepted, h.accepted)
    assert np.max(np.abs(s.mean - h.mean)) <= d and np.max(np.abs(s.bm_mean - h.bm_mean)) <= d and np.max(np.abs(s.cur - h.cur)) <= d
    assert np.max(np.abs(s.m2 - h.m2)) <= 4 * M * d * h.t and np.max(np.abs(s.bm_m2 - h.bm_m2)) <= 4 * M * d * h.n_batches
    assert np.max(np.abs(s.bsum - h.bsum)) <= 2 * d
    assert np.all(np.abs(s.misfit - h.misfit) <= 2e-5 * np.abs(h.misfit))
