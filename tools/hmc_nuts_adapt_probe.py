"""What the dual-averaging step-size warm-up of the No-U-turn chains costs and what it buys (model="ml",
nuts=Nuts(max_depth, adapt=StepAdapt(target_accept, tune))) at the reference's sizes (n = 1597, 3 units of 50, 40 outputs, max_depth = 7)
with C = 4 and 64 chains.  One JSON object (stdout, and --out FILE, default profiles/hmc_nuts_adapt_probe.json):

  cost      per C: us per transition, median and spread (min, max) of --rounds alternating rounds, graph-replayed, for
              adapt     nuts=Nuts(7, adapt=StepAdapt(tune=0)): finrom_hmc_nuts_ml_adapt and, behind it, finrom_hmc_step_adapt_update --
                        the per-chain step's load, the update's node, its read of pt and its step_size row; with tune = 0 the step
                        never moves, so both runs build the SAME trees (asserted on the tree rows);
              plain     nuts=Nuts(7): the transition as it was, in the same run;
            at a step size at which every tree has 127 leapfrog steps; the difference, three times the larger spread, and whether the
            difference is below it.  The recursion's own arithmetic (a dozen operations and one exp per chain while t <= tune) runs in
            the sampling part below and is not timed apart: not measured.
  sampling  the sigma = 1e-3 study of the metric's README row (rank-40 metric, four chains from the mode): StepAdapt(0.98, tune=100)
            from eps0 = 0.4, 150 transitions -- the steps the chains adapted to, and over the 50 transitions behind the warm-up the
            mean accept_stat, tree depths, divergences -- beside the hand-scanned eps = 0.00625 over the same 50 transitions.  Reported,
            not gated.

A timing figure is the wall time of a long run minus a short one (set-up and capture cancel) over the transitions between them.
usage (GPU box): python tools/hmc_nuts_adapt_probe.py [--out FILE] [--quick] [--rounds R]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEPTH = 7
EPS_FULL_TREES = 0.0025                                              # tools/hmc_nuts_probe.py: every measured tree has 127 steps


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmc_nuts_adapt_probe.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes, one round: a rehearsal of the paths, not a measurement")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc, laplace
    from bayesianinferencedl_amd.bayesian_inference.nuts import Nuts, StepAdapt
    from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel, Surrogate
    from bayesianinferencedl_amd.fom.thermal_fin import get_space
    _ffi.check(_ffi.lib().finrom_set_device(0))
    torch.cuda.init()
    n = get_space(None, m=4 if a.quick else 12).dim()
    rounds = 1 if a.quick else max(7, a.rounds)
    t_short, t_long = (2, 6) if a.quick else (5, 25)
    data = np.random.default_rng(3).uniform(0.2, 1.0, 40)
    net = ResBnFcModel(n, 40, 3, 50, seed=2)
    net.head["b"] = np.asarray(data, dtype=np.float32)               # (an untrained network whose outputs sit at the observations)
    sur = Surrogate(net)
    tau = 0.5
    res = {"device": torch.cuda.get_device_name(0), "n": n, "n_out": 40, "max_depth": DEPTH, "rounds": rounds, "eps": EPS_FULL_TREES}

    def starts(C):
        return np.stack([np.exp(0.1 * np.random.default_rng(6 + c).standard_normal(n)) for c in range(C)])

    def run(C, T, adapt):
        t0 = time.perf_counter()
        r = hmc.run_chains_device(None, starts(C), 1 + T, seeds=list(range(100, 100 + C)), eps=EPS_FULL_TREES, n_leapfrog=1, sigma=0.05,
                                  tau=tau, rng="philox", model="ml", surrogate=sur, data=data, nuts=Nuts(DEPTH, adapt=adapt))
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        assert r.graph, "the run was not graph-replayed"
        return t, r

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    res["cost"] = {}
    for C in ((4,) if a.quick else (4, 64)):
        v = {"adapt": [], "plain": []}
        run(C, t_short, StepAdapt(tune=0)); run(C, t_short, None)
        for _ in range(rounds):
            t1, _ = run(C, t_short, StepAdapt(tune=0))
            t2, ra = run(C, t_long, StepAdapt(tune=0))
            v["adapt"].append((t2 - t1) * 1e6 / (t_long - t_short))
            t1, _ = run(C, t_short, None)
            t2, rp = run(C, t_long, None)
            v["plain"].append((t2 - t1) * 1e6 / (t_long - t_short))
        assert np.array_equal(ra.tree, rp.tree) and np.array_equal(ra.K, rp.K), "tune = 0 did not leave the plain run's trees"
        row = {k: stat(x) for k, x in v.items()}
        row["median_steps"] = float(np.median(ra.tree[:, :, 1]))
        larger = max(row["adapt"]["spread"], row["plain"]["spread"])
        row["added_us_per_transition"] = row["adapt"]["median"] - row["plain"]["median"]
        row["three_times_larger_spread_us"] = 3 * larger
        row["below_three_spreads"] = bool(abs(row["added_us_per_transition"]) < 3 * larger)
        res["cost"][str(C)] = row
        write()                                                      # (what has been measured is kept if the run is cut short)

    # the README's sigma = 1e-3 study: four chains (their seeds differ) from ONE point that is the mode, the rank-40 metric there
    sigma, tune = 1e-3, (6 if a.quick else 100)
    T = tune + (4 if a.quick else 50)
    k0 = starts(1)[0]
    K0 = np.ascontiguousarray(np.broadcast_to(k0, (4, n)))
    d0 = np.asarray(sur.misfit_grad_batch(k0[None, :], data, want_grad=False)["qoi"], dtype=np.float64)[0]
    full = laplace.LowRankMetric.from_jacobian(laplace.misfit_jacobian("ml", k0, surrogate=sur, data=d0), None, sigma)
    m = laplace.LowRankMetric(full.Vt[:40], full.lam[:40])

    def sample(eps, adapt):
        r = hmc.run_chains_device(None, K0, 1 + T, seeds=list(range(100, 104)), eps=eps, n_leapfrog=1, sigma=sigma, tau=tau, rng="philox",
                                  model="ml", surrogate=sur, data=d0, nuts=Nuts(DEPTH, metric=m, adapt=adapt))
        tree, stat_ = r.tree[tune:], r.accept_stat[tune:]
        out = {"eps0": eps, "accept_stat_after_tune": float(stat_.mean()), "mean_depth_after_tune": float(tree[:, :, 0].mean()),
               "median_steps_after_tune": float(np.median(tree[:, :, 1])), "divergent_after_tune": int((tree[:, :, 2] == 3).sum()),
               "divergent_while_tuning": int((r.tree[:tune, :, 2] == 3).sum()), "moved_after_tune": float(tree[:, :, 3].mean()),
               "moved_distance": float(np.linalg.norm(r.K - K0, axis=1).mean())}
        if adapt is not None:
            out["adapted_steps"] = r.adapt.eps.tolist()
            out["step_size_every_tenth"] = r.step_size[::10].tolist()
        return out
    res["sampling"] = {"sigma": sigma, "C": 4, "rank": m.rho, "tune": tune, "transitions": T, "target_accept": 0.98,
                       "adapted": sample(0.4, StepAdapt(0.98, tune)), "hand_scanned": sample(0.00625, None)}
    print(json.dumps(res, indent=1))
    write()


if __name__ == "__main__":
    main()
