"""Batched multi-start MAP estimation on the device (bayesian_inference/lbfgs.py: minimize_device over finrom_lbfgs_*,
bayesian_inference/estimate_MAP.py) at the HMC tests' sizes (m = 12, r = 81): the device minimiser against its NumPy
specification (minimize_host) on torch-defined objectives and on the models, recovery of a five-parameter truth (FOM, and the ROM
through the G map) from many starts, the oracle at every returned point, and the reference's MAP study feeding HMC."""
import os
import sys

import numpy as np
import pytest

from oracle import fin_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def setup(problems, spaces):
    sys.path.insert(0, ROOT)
    import bench
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    from bayesianinferencedl_amd.rom.basis import pod_basis
    m, r = 12, 81
    prob, V = problems(m), spaces(m)
    solver = Fin(V)
    phi = pod_basis(solver, r, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1)
    model = bench.hmc_error_model(V.dim())
    rom = AffineROMFin(V, model, phi)
    k_true = np.exp(0.25 * np.random.default_rng(11).standard_normal(V.dim()))
    return prob, V, solver, phi, model, rom, k_true


# ---- torch-defined objectives whose rows do not depend on the batch: sums over columns as elementwise adds in a fixed order ------
def _colsum(T):
    s = T[:, 0].clone()
    for j in range(1, T.shape[1]):
        s = s + T[:, j]
    return s


def _torch_quadratic(d=50, seed=0):
    import torch
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    A = (Q * np.logspace(0, 3, d)) @ Q.T
    A = 0.5 * (A + A.T)
    xs = rng.uniform(-1.0, 1.0, d)
    lo, hi = xs - rng.uniform(0.5, 1.5, d), xs + rng.uniform(0.5, 1.5, d)
    gs = np.zeros(d)
    for j in rng.permutation(d)[: d // 3]:
        if rng.uniform() < 0.5:
            lo[j] = xs[j]; gs[j] = rng.uniform(1.0, 10.0)
        else:
            hi[j] = xs[j]; gs[j] = -rng.uniform(1.0, 10.0)
    dev = dict(dtype=torch.float64, device="cuda")
    At, xst, gst = torch.tensor(A, **dev), torch.tensor(xs, **dev), torch.tensor(gs, **dev)

    def f(X):
        E = X - xst
        AE = E[:, 0:1] * At[0]
        for j in range(1, d):
            AE = AE + E[:, j:j + 1] * At[j]
        val = _colsum(0.5 * (E * AE) + gst * E)
        return val, AE + gst, torch.zeros(X.shape[0], dtype=torch.bool, device=X.device)
    return f, (lo, hi), xs


def _torch_rosenbrock(d=10):
    import torch

    def f(X):
        a, b = X[:, :-1], X[:, 1:]
        t = b - a * a
        val = _colsum(100.0 * t * t + (1.0 - a) * (1.0 - a))
        g = torch.zeros_like(X)
        g[:, :-1] = -400.0 * a * t - 2.0 * (1.0 - a)
        g[:, 1:] = g[:, 1:] + 200.0 * t
        return val, g, torch.zeros(X.shape[0], dtype=torch.bool, device=X.device)
    return f, (np.full(d, -1.5), np.full(d, 0.8))


def _as_host(f):
    import torch

    def h(X):
        v, g, b = f(torch.as_tensor(np.ascontiguousarray(X), dtype=torch.float64, device="cuda"))
        return v.cpu().numpy(), g.cpu().numpy(), b.cpu().numpy()
    return h


@pytest.mark.parametrize("problem", ["quadratic", "rosenbrock"])
def test_device_minimiser_matches_its_host_specification(setup, problem):
    """minimize_device == minimize_host on torch objectives at S = 1, 6 and 64: fhist, x, fun and jac bit for bit, the same nit /
    nfev / status; graph and stream order bit-identical, two runs bit-identical, start i alone == start i inside the batch of 64.
    (Both sides sum in the same order without contraction and evaluate the objective with the same torch kernels on the same
    inputs; tests/test_gpu_lbfgs_kernels.py holds the kernels to the same equality against an objective that stays on the host.)"""
    import torch
    from bayesianinferencedl_amd.bayesian_inference import lbfgs
    if problem == "quadratic":
        f, bounds, _ = _torch_quadratic()
        kw = dict(ftol=0.0, gtol=1e-10, maxiter=400, keep_history=True)
    else:
        f, bounds = _torch_rosenbrock()
        kw = dict(gtol=1e-9, maxiter=400, keep_history=True)
    lo, hi = bounds
    rng = np.random.default_rng(3)
    X64 = lo + (hi - lo) * rng.uniform(0.0, 1.0, (64, len(lo)))
    X64[::7] += 0.5 * (hi - lo)                               # some starts outside the box: projected
    # the objective's rows do not depend on the batch (what the bit-for-bit comparisons below need)
    X_t = torch.as_tensor(X64, dtype=torch.float64, device="cuda")
    v64, g64, _ = f(X_t)
    v1, g1, _ = f(X_t[5:6].clone())
    assert torch.equal(v64[5:6], v1) and torch.equal(g64[5:6], g1)
    for S in (1, 6, 64):
        X0 = X64[:S]
        dev = lbfgs.minimize_device(f, X0, bounds=bounds, **kw)
        host = lbfgs.minimize_host(_as_host(f), X0, bounds=bounds, **kw)
        assert dev["graph"]
        assert np.array_equal(dev.nit, host.nit) and np.array_equal(dev.status, host.status), (S, dev.nit, host.nit)
        fh_d, fh_h = dev.fhist, host.fhist
        assert fh_d.shape == fh_h.shape
        fin = np.isfinite(fh_h)
        assert np.array_equal(np.isfinite(fh_d), fin)
        print(f"{problem}, S = {S}: max |fhist_dev - fhist_host| = {np.max(np.abs(fh_d[fin] - fh_h[fin])):.3e}, "
              f"max |x_dev - x_host| = {np.max(np.abs(dev.x - host.x)):.3e}")
        assert np.array_equal(fh_d, fh_h, equal_nan=True)
        assert np.array_equal(dev.x, host.x) and np.array_equal(dev.fun, host.fun) and np.array_equal(dev.jac, host.jac)
        assert np.array_equal(dev.nfev, host.nfev)
        assert np.all(dev.x >= lo) and np.all(dev.x <= hi)
        if S == 64:
            again = lbfgs.minimize_device(f, X0, bounds=bounds, **kw)
            stream = lbfgs.minimize_device(f, X0, bounds=bounds, graph=False, **kw)
            assert not stream["graph"]
            for other in (again, stream):
                assert np.array_equal(other.x, dev.x) and np.array_equal(other.fun, dev.fun)
                assert np.array_equal(other.nit, dev.nit) and np.array_equal(other.nfev, dev.nfev)
                assert np.array_equal(other.fhist, dev.fhist, equal_nan=True)
            for i in (0, 5, 63):
                one = lbfgs.minimize_device(f, X0[i:i + 1], bounds=bounds, **kw)
                assert np.array_equal(one.x[0], dev.x[i]) and one.fun[0] == dev.fun[i]
                assert one.nit[0] == dev.nit[i] and one.nfev[0] == dev.nfev[i] and one.status[0] == dev.status[i]


def test_five_parameter_truth_is_recovered_by_fom_and_rom(setup):
    """Data from a five-parameter truth inside the box, no regulariser, ftol = 0: 6 starts and 1024 uniform starts (beyond the
    small-batch schedule: the band adjoint) recover the truth to 1e-6 with the FOM; SciPy's L-BFGS-B over the one-sample FOM
    gradient reaches the same point from the same 6 starts.  The ROM (theta = E59 x, the library applies G = E59) recovers a
    truth whose data come from the ROM."""
    from scipy.optimize import minimize
    from bayesianinferencedl_amd.bayesian_inference import estimate_MAP as E
    prob, V, solver, phi, model, rom, k_true = setup
    truth = np.array([0.9, 1.6, 2.4, 0.6, 3.1])
    bounds = (0.1, 4.0)
    data = np.asarray(solver.forward_batch(truth[None], params="five")["qoi"])[0]
    obj = E.objective("fom", data, solver=solver, params="five")
    rng = np.random.default_rng(4)
    X6 = rng.uniform(0.2, 3.8, (6, 5))
    kw = dict(bounds=bounds, ftol=0.0, gtol=1e-12, maxiter=2000, maxfun=4000)
    res6 = obj.minimize(X6, **kw)
    err6 = np.linalg.norm(res6.x - truth, axis=1) / np.linalg.norm(truth)
    assert np.all(err6 <= 1e-6), err6
    X1024 = rng.uniform(0.2, 3.8, (1024, 5))
    res1k = obj.minimize(X1024, **kw)
    err1k = np.linalg.norm(res1k.x - truth, axis=1) / np.linalg.norm(truth)
    assert np.all(err1k <= 1e-6), (np.max(err1k), np.sum(err1k > 1e-6))

    def one(x):
        r = solver.gradient_batch(x[None], data, params="five")
        return float(r["J"][0]), np.asarray(r["grad"][0])
    for i in range(6):
        ref = minimize(one, X6[i], jac=True, method="L-BFGS-B", bounds=[bounds] * 5, options=dict(ftol=0.0, gtol=1e-12, maxiter=2000))
        assert np.linalg.norm(ref.x - res6.x[i]) <= 1e-6 * np.linalg.norm(truth), (i, ref.x, res6.x[i])
    # the ROM through the G map: data from the ROM at the truth
    E59 = solver.ops.E59
    data_r = np.asarray(rom.forward_nine_param_reduced_batch((E59 @ truth)[None])["qoi_r"])[0]
    obj_r = E.objective("rom", data_r, solver_r=rom, params="five")
    res_r = obj_r.minimize(X6, **kw)
    err_r = np.linalg.norm(res_r.x - truth, axis=1) / np.linalg.norm(truth)
    assert np.all(err_r <= 1e-6), err_r


@pytest.mark.parametrize("kind", ["fom", "rom", "romml"])
def test_field_map_matches_the_host_driver_and_the_oracle(setup, kind):
    """Field problems with the reference's recipe (box from k_true, Tikhonov gamma = 1e-6, starts exp(0.5 U^T xi)):
    minimize_device against minimize_host driving the same device value-and-gradient (the G map and the Tikhonov term then on the
    host, lbfgs.library_terms): fhist over the first 10 iterations to 1e-9, final fun to 1e-8, the same nit (iteration cap: no
    borderline stopping test); the oracle re-evaluates fun and jac at every returned x within the parity tolerances
    (FOM: J 1e-10, grad 1e-9; ROM: 1e-10 / 1e-8; ROM + ML: 2e-5 / 1e-5, the network is fp32).  Measured maxima (MI355X): host
    against device 0 (fhist and fun, every model: the same steps to the last bit); oracle fun / jac: FOM 6.2e-12 / 3.4e-10, ROM
    3.0e-11 / 1.4e-10, ROM + ML 1.8e-6 / 6.7e-7."""
    from bayesianinferencedl_amd.bayesian_inference import estimate_MAP as E
    prob, V, solver, phi, model, rom, k_true = setup
    data = np.asarray(solver.qoi_operator(solver.forward(k_true)[0]))
    rom.set_data(data)
    obj = E.objective(kind, data, solver=solver, solver_r=rom, gamma=E.GAMMA)
    X0 = E.starting_points(V, 6, seed=2)
    bounds = (0.95 * k_true.min(), 1.05 * k_true.max())
    kw = dict(bounds=bounds, ftol=1e-10, gtol=1e-8, maxiter=40, keep_history=True)
    dev = obj.minimize(X0, device=True, **kw)
    host = obj.minimize(X0, device=False, **kw)
    assert np.array_equal(dev.nit, host.nit), (dev.nit, host.nit)
    n = min(11, dev.fhist.shape[0])
    assert np.allclose(dev.fhist[:n], host.fhist[:n], rtol=1e-9, atol=0.0, equal_nan=True)
    assert np.all(np.abs(dev.fun - host.fun) <= 1e-8 * np.abs(host.fun))
    assert np.all(dev.fun < dev.fhist[0])                      # every start went down
    fo = O.FinOracle(prob)
    ro = O.AffineROMOracle(prob, phi); ro.set_data(data)
    tol_f, tol_g = {"fom": (1e-10, 1e-9), "rom": (1e-10, 1e-8), "romml": (2e-5, 1e-5)}[kind]

    def oracle(x):
        if kind == "fom":
            g, J = fo.gradient(x, data), 0.5 * np.sum((fo.qoi_operator(fo.forward(x)) - data) ** 2)
        elif kind == "rom":
            g, J = ro.grad_reduced(x)
        else:
            g, J = O.grad_romml_oracle(ro, model, x)
        return J + fo.reg(x, E.GAMMA), g + fo.grad_reg(x, E.GAMMA)
    rf, rg = [], []
    for s in range(len(X0)):
        x = dev.x[s]
        F, G = oracle(x)
        # the fp32 network's rounding is an absolute error on the residual, which is small at a MAP point: for the ROM + ML misfit
        # the gradient's tolerance is relative to the gradient at the start
        scale = np.linalg.norm(oracle(np.clip(X0[s], *bounds))[1]) if kind == "romml" else np.linalg.norm(G)
        rf.append(abs(dev.fun[s] - F) / abs(F)); rg.append(np.linalg.norm(dev.jac[s] - G) / scale)
        assert rf[-1] <= tol_f and rg[-1] <= tol_g, (s, rf[-1], rg[-1])
        if dev.status[s] == 0 and dev.message[s].startswith("CONVERGENCE: NORM"):
            pg = np.max(np.abs(np.clip(x - G, *bounds) - x))
            assert pg <= 1e-8 + tol_g * scale, (s, pg)
    print(f"MEASURED {kind}: fhist[:10] {np.nanmax(np.abs(dev.fhist[:n] - host.fhist[:n]) / np.abs(host.fhist[:n])):.2e}, "
          f"fun {np.max(np.abs(dev.fun - host.fun) / np.abs(host.fun)):.2e}, oracle fun {max(rf):.2e}, oracle jac {max(rg):.2e}")


def test_estimate_map_study_and_hmc_from_its_romml_map(setup, tmp_path):
    """The reference's study with six starts: every reported error equals its recomputation, the best start is the argmin of the
    reconstruction error, the files carry the reference's names and shapes, and HMC chains started at prior.whiten of the ROMML
    MAP have a finite start potential and complete 21 evaluations."""
    from bayesianinferencedl_amd.bayesian_inference import estimate_MAP as E
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
    prob, V, solver, phi, model, rom, k_true = setup
    out = E.estimate_map(solver, rom, k_true, n_starting_pts=6, seed=0, out_dir=str(tmp_path), maxiter=30)
    data = out["data"]
    M = solver.M
    nt = np.sqrt(k_true @ M @ k_true)
    for kind, fname in (("fom", "res_FOM.npy"), ("rom", "res_ROM.npy"), ("romml", "res_ROMML.npy")):
        r = out[kind]
        assert r["x"].shape == (6, V.dim()) and r["status"].shape == (6,)
        for s in range(6):
            x = r["x"][s]
            q = solver.qoi_operator(solver.forward(x)[0])
            assert abs(r["obs_err"][s] - np.linalg.norm(data - q) / np.linalg.norm(data)) <= 1e-12
            e = k_true - x
            assert abs(r["l2_err"][s] - np.sqrt(e @ M @ e) / nt) <= 1e-12
            assert abs(r["pw_err"][s] - np.linalg.norm(e) / np.sqrt(nt)) <= 1e-12
        assert r["best"] == int(np.argmin(r["l2_err"]))
        saved = np.load(tmp_path / fname)
        assert saved.shape == (V.dim(),) and np.array_equal(saved, r["x"][r["best"]])
    prior = GaussianFieldPrior(V)
    best = np.load(tmp_path / "res_ROMML.npy")
    rom.set_data(data)
    res = hmc.run_chains_fused(rom, prior.whiten(best)[None], 21, seeds=[0], prior=prior, graph=False)
    assert res.n_evals == 21 and np.all(np.isfinite(res.K))
