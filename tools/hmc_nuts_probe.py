"""What a leapfrog step costs inside the No-U-turn transition of the chains under the pure deep-learning surrogate (model="ml",
nuts=Nuts(max_depth): finrom_hmc_nuts_ml, one call per transition), at the reference's sizes (n = 1597, 3 units of 50, 40 outputs)
with C = 4, 64 and 256 chains.  One JSON object (stdout, and --out FILE, default profiles/hmc_nuts_probe.json):

  calibration  the step size: the first of a fixed list at which the median tree of a short run at C = 4 has 31 .. 127 leapfrog steps
               (max_depth = 7, the reference's); the trees of every measured run are reported beside it;
  per C        us per leapfrog step, median and spread (min, max) of --rounds alternating rounds, for
                 nuts         run_chains_device(nuts=): a launch takes as long as its longest tree, so the steps counted are the sum
                              over the transitions of the LONGEST tree among the chains;
                 trajectory   ml_form="trajectory" with n_leapfrog = 10 at the same step size: baseline (a), reported -- the tree's
                              overhead per step -- not gated;
                 host_tree    baseline (b), the host-driven tree at its cheapest: per leaf ONE finrom_hmc_leapfrog_ml (three launches,
                              all chains in lockstep), the least the leaf's decision needs beside it -- the full-step momentum,
                              |p|^2, |k - mean|^2 and rho_sub += p as torch ops -- and ONE read-back of (misfit, |p|^2, |k - mean|^2);
                              the candidate's copies, the checkpoints and the U-turn products would come on top;
                 host_step    the same loop without those torch ops (the step and a read-back of the misfits alone), for scale;
               and whether "nuts" is ahead of "host_tree" by more than three times the larger spread.

Every chain run is graph-replayed (asserted) and ends in a device synchronisation; a figure is the wall time of a long run minus a
short one (set-up and capture cancel) over the steps between them.
The host-driven tree is a host loop and its wall time is the noisy figure here (its spread reached 23 us over runs of 500 leaves):
it is timed over 2500 leaves.  The committed profile was taken with --rounds 7.
usage (GPU box): python tools/hmc_nuts_probe.py [--out FILE] [--quick] [--rounds R]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EPS_LIST = (0.08, 0.04, 0.02, 0.01, 0.005, 0.0025)
DEPTH = 7


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmc_nuts_probe.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes, one round: a rehearsal of the paths, not a measurement")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.nuts import Nuts
    from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel, Surrogate
    from bayesianinferencedl_amd.fom.thermal_fin import get_space
    L = _ffi.lib()
    _ffi.check(L.finrom_set_device(0))
    torch.cuda.init()
    n = get_space(None, m=4 if a.quick else 12).dim()
    rounds = 1 if a.quick else max(3, a.rounds)
    t_short, t_long = (2, 6) if a.quick else (5, 25)                 # transitions
    e_short, e_long = (21, 61) if a.quick else (201, 1201)           # evaluations of the trajectory form
    l_short, l_long = (10, 40) if a.quick else (500, 3000)           # leaves of the host-driven tree (long: its host loop is the noisy one)
    data = np.random.default_rng(3).uniform(0.2, 1.0, 40)
    m = ResBnFcModel(n, 40, 3, 50, seed=2)
    m.head["b"] = np.asarray(data, dtype=np.float32)                 # (an untrained network whose outputs sit at the observations)
    sur = Surrogate(m)
    sigma, tau = 0.05, 0.5
    res = {"device": torch.cuda.get_device_name(0), "n": n, "n_out": 40, "max_depth": DEPTH, "rounds": rounds}

    def starts(C):
        return np.stack([np.exp(0.1 * np.random.default_rng(6 + c).standard_normal(n)) for c in range(C)])

    def chains(C, eps, **kw):
        t0 = time.perf_counter()
        r = hmc.run_chains_device(None, starts(C), seeds=list(range(100, 100 + C)), eps=eps, sigma=sigma, tau=tau, rng="philox", model="ml",
                                  surrogate=sur, data=data, **kw)
        torch.cuda.synchronize()
        assert r.graph, "the run was not graph-replayed"
        return time.perf_counter() - t0, r

    def nuts_run(C, eps, T):
        t, r = chains(C, eps, n_evals=1 + T, n_leapfrog=1, nuts=Nuts(DEPTH))
        return t, r, int(r.tree[:, :, 1].max(axis=1).sum())          # a launch lasts as long as its longest tree

    def host_tree(C, eps, leaves, sums=True):
        """`leaves` lockstep steps of finrom_hmc_leapfrog_ml, behind each the leaf's energy terms (sums) and one read-back: the wall time."""
        f64 = dict(dtype=torch.float64, device="cuda")
        K = torch.as_tensor(starts(C), **f64)
        z = lambda *s: torch.zeros(*s, **f64)
        Kq, P = [K.clone(), K.clone()], torch.as_tensor(np.random.default_rng(1).standard_normal((C, n)), **f64)
        mean, U, dU, dUq, H0, lu, loss = K.clone(), z(C), z(C, n), z(C, n), z(C), z(1, C), z(C)
        Pb, rho = z(1, C, n), z(C, n)
        half = 0.5 * eps / tau ** 2
        i64 = dict(dtype=torch.int64, device="cuda")
        jt, pt, acc = torch.zeros(1, **i64), torch.zeros(1, **i64), torch.zeros(C, **i64)
        info, data_t = torch.zeros(C, dtype=torch.int32, device="cuda"), torch.as_tensor(data, **f64)
        st = _ffi.HmcState(C=C, n=n, eps=eps, c_lik=1.0 / sigma ** 2, c_pri=1.0 / tau ** 2, mean=mean.data_ptr(), K=K.data_ptr(),
                           U=U.data_ptr(), dU=dU.data_ptr(), Kq=(ctypes.c_void_p * 2)(Kq[0].data_ptr(), Kq[1].data_ptr()), P=P.data_ptr(),
                           dUq=dUq.data_ptr(), H0=H0.data_ptr(), P_block=Pb.data_ptr(), lu_block=lu.data_ptr(), jt=jt.data_ptr(),
                           pt=pt.data_ptr(), accept=acc.data_ptr(), trace=None, loss=loss.data_ptr(), info=info.data_ptr())
        stream = torch.cuda.current_stream().cuda_stream
        step = lambda i: _ffi.check(L.finrom_hmc_leapfrog_ml(sur._dev._h, ctypes.byref(st), i, data_t.data_ptr(), 0, None, None, stream),
                                    "finrom_hmc_leapfrog_ml")
        step(0)                                                      # (workspaces)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(leaves):
            step(i)
            if sums:                                                 # the host's decision needs the leaf's energy: one read-back
                Pf = torch.add(P, dUq, alpha=half)                   # (the step leaves the momentum half a kick ahead)
                D = Kq[(i + 1) & 1] - mean
                rho.add_(Pf)
                torch.stack([loss, torch.linalg.vecdot(Pf, Pf), torch.linalg.vecdot(D, D)]).cpu()
            else:
                loss.cpu()
        return time.perf_counter() - t0

    # the step size at which trees have 31 .. 127 steps
    cal, eps = [], None
    for e in EPS_LIST:
        r = nuts_run(4, e, t_long)[1]
        med = float(np.median(r.tree[:, :, 1]))
        cal.append({"eps": e, "median_steps": med, "stop_reasons": np.bincount(r.tree[:, :, 2].ravel(), minlength=4).tolist()})
        if eps is None and 31 <= med <= 127:
            eps = e
    res["calibration"] = cal
    res["eps"] = eps if eps is not None else EPS_LIST[-1]
    res["trees_in_range"] = eps is not None
    eps = res["eps"]

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    res["per_C"] = {}
    for C in ((4,) if a.quick else (4, 64, 256)):
        v = {"nuts": [], "trajectory": [], "host_tree": [], "host_step": []}
        nuts_run(C, eps, t_short); chains(C, eps, n_evals=e_short, n_leapfrog=10, ml_form="trajectory"); host_tree(C, eps, l_short)
        for _ in range(rounds):
            t1, _, s1 = nuts_run(C, eps, t_short)
            t2, r, s2 = nuts_run(C, eps, t_long)
            v["nuts"].append((t2 - t1) * 1e6 / (s2 - s1))
            t1 = chains(C, eps, n_evals=e_short, n_leapfrog=10, ml_form="trajectory")[0]
            t2 = chains(C, eps, n_evals=e_long, n_leapfrog=10, ml_form="trajectory")[0]
            v["trajectory"].append((t2 - t1) * 1e6 / (e_long - e_short))
            v["host_tree"].append((host_tree(C, eps, l_long) - host_tree(C, eps, l_short)) * 1e6 / (l_long - l_short))
            v["host_step"].append((host_tree(C, eps, l_long, False) - host_tree(C, eps, l_short, False)) * 1e6 / (l_long - l_short))
        row = {k: stat(x) for k, x in v.items()}
        row["trees"] = {"median_steps": float(np.median(r.tree[:, :, 1])), "longest_per_launch_mean": float(r.tree[:, :, 1].max(axis=1).mean()),
                        "stop_reasons": np.bincount(r.tree[:, :, 2].ravel(), minlength=4).tolist(), "moved": float(r.tree[:, :, 3].mean()),
                        "accept_stat": float(r.accept_stat.mean())}
        larger = max(row["nuts"]["spread"], row["host_tree"]["spread"])
        row["tree_overhead_per_step_us"] = row["nuts"]["median"] - row["trajectory"]["median"]
        row["nuts_ahead_of_host_tree_us"] = row["host_tree"]["median"] - row["nuts"]["median"]
        row["three_times_larger_spread_us"] = 3 * larger
        row["nuts_beats_host_tree"] = bool(row["nuts_ahead_of_host_tree_us"] > 3 * larger)
        res["per_C"][str(C)] = row
        write()                                                      # (what has been measured is kept if the run is cut short)
    print(json.dumps(res, indent=1))
    write()


if __name__ == "__main__":
    main()
