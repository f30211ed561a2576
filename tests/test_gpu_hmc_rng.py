"""The HMC chains' counter-based random stream on the device (hmc.py rng="philox", finrom_hmc_draw): the draw kernel against the
oracle's NumPy restatement, its bounds, its invariance under the cut into blocks and the deal of chains, and chains -- host
recursion against torch form and fused form, under the i.i.d. prior and under prior + metric, cut into blocks and continued --
at the fixture sizes of tests/test_gpu_hmc.py (m = 12, r = 81, 4 chains)."""
import os
import sys

import numpy as np
import pytest

from oracle import fin_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 7, (1 << 32) + 7, (1 << 63) + 1]
GRID_CAP = 16384                     # workgroups of 256 threads: launch_hmc_draw's cap (launch_philox_normal's), csrc/util_kernels.hip
PAD = 5                              # elements of NaN kept behind each buffer's block


def _draw(seeds, first, B, n):
    """finrom_hmc_draw into NaN-filled buffers PAD elements longer than the block: (P [B, C, n], lu [B, C]); nothing behind the block
    may have changed, and everything inside must have."""
    import torch
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    C = len(seeds)
    st = torch.as_tensor(np.array(seeds, dtype=np.uint64).view(np.int64), device="cuda")
    P = torch.full((B * C * n + PAD,), float("nan"), dtype=torch.float64, device="cuda")
    lu = torch.full((B * C + PAD,), float("nan"), dtype=torch.float64, device="cuda")
    _ffi.check(L.finrom_hmc_draw(st.data_ptr(), C, n, first, B, P.data_ptr(), lu.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "finrom_hmc_draw")
    P, lu = P.cpu().numpy(), lu.cpu().numpy()
    assert np.isnan(P[B * C * n:]).all() and np.isnan(lu[B * C:]).all(), "finrom_hmc_draw wrote behind its block"
    assert not np.isnan(P[:B * C * n]).any() and not np.isnan(lu[:B * C]).any(), "finrom_hmc_draw left an element of its block unwritten"
    return P[:B * C * n].reshape(B, C, n), lu[:B * C].reshape(B, C)


def _oracle(seeds, first, B, n):
    P = np.stack([O.philox_normal(s, first, B, n) for s in seeds], axis=1)
    p = np.uint64(first) + np.arange(B, dtype=np.uint64)
    lu = np.empty((B, len(seeds)))
    for c, s in enumerate(seeds):
        o = O.philox4x32_10([p & np.uint64(0xFFFFFFFF), p >> np.uint64(32), np.zeros(B, np.uint64), np.ones(B, np.uint64)],
                            s & 0xFFFFFFFF, s >> 32)
        a = (o[1] << np.uint64(32)) | o[0]
        lu[:, c] = np.log(((a >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53)
    return P, lu


@pytest.mark.parametrize("first", [0, (1 << 32) - 2])
@pytest.mark.parametrize("B,C,n", [(1, 1, 1), (1, 3, 2), (4, 3, 5), (2, 2, 515), (3, 4, 1597)])
def test_draw_matches_the_oracle_and_stays_inside_its_block(B, C, n, first):
    """Normals within 1e-13 absolute of O.philox_normal (finrom_sampler_draw_seeded's bound); lu within 1e-13 absolute of the log of
    the oracle's uniform (|lu| <= 53 ln 2 = 36.7, one ulp there is 7e-15), finite and <= 0.  Odd n: the last pair writes one element."""
    P, lu = _draw(SEEDS[:C], first, B, n)
    Po, luo = _oracle(SEEDS[:C], first, B, n)
    print("max |P - oracle|", np.max(np.abs(P - Po)), "max |lu - oracle|", np.max(np.abs(lu - luo)))
    assert np.max(np.abs(P - Po)) <= 1e-13
    assert np.max(np.abs(lu - luo)) <= 1e-13
    assert np.all(lu <= 0.0) and np.all(np.isfinite(lu))


def test_draw_under_the_capped_grid():
    """(B, C, n) = (33, 64, 4101): 33 x 64 x 2051 = 4 331 712 pairs, more than the GRID_CAP x 256 = 4 194 304 threads of the capped grid,
    so the grid-stride loop takes a second trip; the same bounds against the oracle."""
    B, C, n = 33, 64, 4101
    assert B * C * ((n + 1) // 2) > GRID_CAP * 256
    seeds = (SEEDS * 16)[:C]
    seeds = [s ^ (i << 20) for i, s in enumerate(seeds)]
    P, lu = _draw(seeds, 3, B, n)
    Po, luo = _oracle(seeds, 3, B, n)
    print("max |P - oracle|", np.max(np.abs(P - Po)), "max |lu - oracle|", np.max(np.abs(lu - luo)))
    assert np.max(np.abs(P - Po)) <= 1e-13
    assert np.max(np.abs(lu - luo)) <= 1e-13


def test_draw_does_not_depend_on_the_cut_or_the_deal():
    n = 515
    P, lu = _draw(SEEDS, 7, 5, n)
    Pa, la = _draw(SEEDS, 7, 2, n)
    Pb, lb = _draw(SEEDS, 9, 3, n)
    assert np.array_equal(P, np.concatenate([Pa, Pb])) and np.array_equal(lu, np.concatenate([la, lb]))
    Ps, ls = _draw([SEEDS[1], SEEDS[3]], 7, 5, n)
    assert np.array_equal(Ps, P[:, [1, 3]]) and np.array_equal(ls, lu[:, [1, 3]])


# ---- chains ----------------------------------------------------------------------------------------------------------------------
CHAIN_SEEDS = [100, 101, 102, 103]
EPS = 3e-2


@pytest.fixture(scope="module")
def setup(problems, spaces):
    """tests/test_gpu_hmc.py's setting (m = 12, r = 81, bench.hmc_error_model) with test_gpu_metric.py's prior."""
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


@pytest.fixture(scope="module")
def host(setup):
    """The host recursion with rng="philox": the reference of the chain cases, computed once."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    rom, K0, _ = setup
    res = hmc.run_chains(hmc.romml_value_and_grad(rom), K0, 141, seeds=CHAIN_SEEDS, eps=EPS, n_leapfrog=10, keep_trace=True, rng="philox")
    print("host chain (philox) accept", res.accept)
    return res


@pytest.fixture(scope="module")
def device_runs(setup):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    rom, K0, _ = setup
    cache = {}

    def get(fused, block):
        if (fused, block) not in cache:
            cache[fused, block] = hmc.run_chains_device(rom, K0, 141, seeds=CHAIN_SEEDS, eps=EPS, n_leapfrog=10, keep_trace=True,
                                                        graph=True, fused=fused, block=block, rng="philox")
        return cache[fused, block]
    return get


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("block", [32, 5])
def test_device_chains_with_device_draws_walk_the_host_chains_path(host, device_runs, block, fused):
    """run_chains(romml_value_and_grad(rom), rng="philox") against run_chains_device(rng="philox"), graph replayed, 14 proposals in one
    block or in blocks of 5, 5, 4 (one finrom_hmc_draw launch each): equal accept vectors, trace and end states within 1e-9 (the
    bound of tests/test_gpu_hmc.py).  eps = 3e-2 as there: with seeds 100..103 the host chain under the philox stream must both
    accept and reject for the case to count (asserted below; the accept vector is printed)."""
    dev = device_runs(fused, block)
    assert dev.fused == fused and dev.graph and dev.n_evals == host.n_evals == 141 and dev.proposals == host.proposals == 14
    print("accept host", host.accept, "device", dev.accept, "trace", np.max(np.abs(dev.trace - host.trace)) / np.max(np.abs(host.trace)))
    assert 0 < host.accept.sum() < 4 * 14, host.accept
    assert np.array_equal(dev.accept, host.accept)
    assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    assert np.linalg.norm(dev.K - host.K) <= 1e-9 * np.linalg.norm(host.K)


def test_fused_chains_do_not_depend_on_the_block(device_runs):
    """Fused, graph: blocks of 5 against one block of 32 -- the same draws whatever the cut, so the traces are bitwise equal."""
    a, b = device_runs(True, 5), device_runs(True, 32)
    assert np.array_equal(a.trace, b.trace) and np.array_equal(a.K, b.K) and np.array_equal(a.accept, b.accept)


def test_fused_chains_under_prior_and_metric_with_device_draws(setup):
    """prior=GaussianFieldPrior, metric= the Gauss-Newton metric at the MAP, built as in tests/test_gpu_metric.py (sigma = 0.05,
    starts drawn from the Laplace approximation, eps = 0.3, 121 evaluations): the fused device chains against the host recursion
    with the same arguments, both with rng="philox" -- equal accept vectors, trace, fields and whitened end states within 1e-9
    (that file's bound for this comparison)."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.laplace import gauss_newton_map, reduced_value_grad_jac
    rom, _, prior = setup
    sigma = 0.05
    metric = gauss_newton_map(reduced_value_grad_jac(rom, "romml"), prior, sigma)["metric"]
    V0 = np.stack([metric.draw(np.random.default_rng(6 + c).standard_normal(prior.n)) for c in range(4)])
    kw = dict(seeds=CHAIN_SEEDS, eps=0.3, n_leapfrog=10, prior=prior, sigma=sigma, metric=metric, keep_trace=True, rng="philox")
    ref = hmc.run_chains(hmc.romml_value_and_grad(rom), V0, 121, **kw)
    dev = hmc.run_chains_device(rom, V0, 121, graph=True, fused=True, **kw)
    assert dev.fused and dev.graph and dev.proposals == ref.proposals == 12
    print("accept", ref.accept, dev.accept, "trace", np.max(np.abs(dev.trace - ref.trace)) / np.max(np.abs(ref.trace)))
    assert np.array_equal(dev.accept, ref.accept)
    assert ref.accept.sum() > 0
    assert np.max(np.abs(dev.trace - ref.trace)) <= 1e-9 * np.max(np.abs(ref.trace))
    assert np.linalg.norm(dev.K - ref.K) <= 1e-9 * np.linalg.norm(ref.K)
    assert np.linalg.norm(dev.V - ref.V) <= 1e-9 * np.linalg.norm(ref.V)


@pytest.mark.parametrize("form", ["iid", "prior"])
def test_fused_chains_continue_from_their_end_state(setup, form):
    """7 proposals, then 7 more from the end state (K with the first run's mean passed explicitly; under the prior V, the prior
    carrying the mean) with proposal0=7, against one run of 14: equal accept sums per chain, end states within 1e-9."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    rom, K0, prior = setup
    if form == "iid":
        x0, kw, end = K0, dict(mean=K0, eps=EPS), "K"
    else:
        x0 = np.stack([np.random.default_rng(6 + c).standard_normal(prior.n) for c in range(4)])
        kw, end = dict(prior=prior, eps=0.1), "V"
    kw.update(seeds=CHAIN_SEEDS, n_leapfrog=10, graph=True, fused=True, rng="philox")
    whole = hmc.run_chains_device(rom, x0, 141, **kw)
    one = hmc.run_chains_device(rom, x0, 71, **kw)
    two = hmc.run_chains_device(rom, one[end], 71, proposal0=7, **kw)
    assert whole.proposals == 14 and one.proposals == two.proposals == 7
    print(form, "accept", whole.accept, one.accept, two.accept)
    assert np.array_equal(one.accept + two.accept, whole.accept)
    assert np.linalg.norm(two[end] - whole[end]) <= 1e-9 * np.linalg.norm(whole[end])
    assert np.linalg.norm(two.K - whole.K) <= 1e-9 * np.linalg.norm(whole.K)
