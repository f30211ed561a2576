"""Cost of batched multi-start MAP estimation (bayesian_inference/lbfgs.py, estimate_MAP.py) at the HMC tests' sizes (m = 12,
r = 81, the bench's error model), one JSON line per measurement:

  rounds   us per round (finrom_lbfgs_propose + the model's launches + finrom_lbfgs_accept) for the FOM (fields), the ROM and the
           ROM + ML misfit with the reference's Tikhonov term, at S = 1, 6, 64, captured graph vs stream order.  Every start runs
           the same number of rounds (ftol = gtol = 0, maxfun = rounds + 1); the time is the host loop's wall time over the rounds,
           its status reads every `block` rounds included.
  study    the reference's six-start study, per model: one batched minimize_device call against the reference's pattern -- SciPy
           L-BFGS-B over the one-sample wrappers (SolverWrapper / RSolverWrapper / ROMMLSolverWrapper), the starts in series --
           from the same starts, with nit / nfev of both (--maxiter caps both).
  stats    (--stats CSV) the two new kernels' rows of a `rocprofv3 --kernel-trace --stats` run of `--kernels` (S = 64 ROM + ML
           rounds in stream order, nothing else): calls, mean and total time.

  python tools/map_probe.py [--rounds 64] [--maxiter 200] [--out profiles/map_probe.jsonl]
  rocprofv3 --kernel-trace --stats -d DIR -o map -- python tools/map_probe.py --kernels
  python tools/map_probe.py --stats DIR/.../map_kernel_stats.csv"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(m=12, r=81):
    import bench
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.fom.thermal_fin import get_space
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    from bayesianinferencedl_amd.rom.basis import pod_basis
    V = get_space(None, m=m)
    solver = Fin(V)
    phi = pod_basis(solver, r, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1)
    model = bench.hmc_error_model(V.dim())
    rom = AffineROMFin(V, model, phi)
    k_true = np.exp(0.25 * np.random.default_rng(11).standard_normal(V.dim()))
    data = np.asarray(solver.qoi_operator(solver.forward(k_true)[0]))
    rom.set_data(data)
    return V, solver, rom, k_true, data


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def rounds(V, solver, rom, k_true, data, n_rounds, out):
    from bayesianinferencedl_amd.bayesian_inference import estimate_MAP as E
    X = E.starting_points(V, 64, seed=5)
    bounds = (0.95 * k_true.min(), 1.05 * k_true.max())
    for kind in ("fom", "rom", "romml"):
        obj = E.objective(kind, data, solver=solver, solver_r=rom, gamma=E.GAMMA)
        for S in (1, 6, 64):
            for graph in (True, False):
                kw = dict(bounds=bounds, ftol=0.0, gtol=0.0, maxiter=10 ** 6, maxfun=n_rounds + 1, graph=graph, block=16)
                obj.minimize(X[:S], **kw)                                   # (warm: workspaces, pool)
                res = obj.minimize(X[:S], **kw)
                emit(dict(kind="rounds", model=kind, S=S, graph=bool(res["graph"]), rounds=res["rounds"],
                          us_per_round=1e6 * res["loop_s"] / max(res["rounds"], 1), nfev_max=int(res.nfev.max())), out)


def study(V, solver, rom, k_true, data, maxiter, out):
    from scipy.optimize import minimize
    from bayesianinferencedl_amd.bayesian_inference import estimate_MAP as E
    X0 = E.starting_points(V, 6, seed=0)
    bounds = (0.95 * k_true.min(), 1.05 * k_true.max())
    wrappers = {"fom": lambda: E.SolverWrapper(solver, data), "rom": lambda: E.RSolverWrapper(rom.dl_model, rom, solver),
                "romml": lambda: E.ROMMLSolverWrapper(rom.dl_model, rom, solver)}
    for kind in ("fom", "rom", "romml"):
        obj = E.objective(kind, data, solver=solver, solver_r=rom, gamma=E.GAMMA)
        obj.minimize(X0[:1], bounds=bounds, ftol=1e-10, gtol=1e-8, maxiter=2)          # (warm)
        t0 = time.perf_counter()
        res = obj.minimize(X0, bounds=bounds, ftol=1e-10, gtol=1e-8, maxiter=maxiter)
        t_dev = time.perf_counter() - t0
        w = wrappers[kind]()
        nit, nfev, fun = [], [], []
        t0 = time.perf_counter()
        for x0 in X0:
            r = minimize(w.cost_function, x0, method="L-BFGS-B", jac=w.gradient, bounds=[bounds] * len(x0),
                         options={"ftol": 1e-10, "gtol": 1e-8, "maxiter": maxiter})
            nit.append(int(r.nit)); nfev.append(int(r.nfev)); fun.append(float(r.fun))
        t_ref = time.perf_counter() - t0
        emit(dict(kind="study", model=kind, starts=6, maxiter=maxiter, device_s=t_dev, device_nit=res.nit.tolist(),
                  device_nfev=res.nfev.tolist(), device_rounds=res["rounds"], device_fun=res.fun.tolist(), reference_s=t_ref,
                  reference_nit=nit, reference_nfev=nfev, reference_fun=fun), out)


def kernels(V, solver, rom, k_true, data):
    from bayesianinferencedl_amd.bayesian_inference import estimate_MAP as E
    X = E.starting_points(V, 64, seed=5)
    bounds = (0.95 * k_true.min(), 1.05 * k_true.max())
    obj = E.objective("romml", data, solver=solver, solver_r=rom, gamma=E.GAMMA)
    res = obj.minimize(X, bounds=bounds, ftol=0.0, gtol=0.0, maxiter=10 ** 6, maxfun=65, graph=False, block=16)
    print("rounds", res["rounds"], flush=True)


def stats(path, out):
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            k = re.search(r"lbfgs_\w+_kernel(<\d+>)?", name)
            if k:
                emit(dict(kind="stats", kernel=k.group(0), calls=int(row["Calls"]), mean_us=float(row["AverageNs"]) / 1e3,
                          min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3,
                          total_us=float(row["TotalDurationNs"]) / 1e3), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--maxiter", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-study", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        stats(a.stats, a.out)
        return
    ctx = setup()
    if a.kernels:
        kernels(*ctx)
        return
    rounds(*ctx, a.rounds, a.out)
    if not a.skip_study:
        study(*ctx, a.maxiter, a.out)


if __name__ == "__main__":
    main()
