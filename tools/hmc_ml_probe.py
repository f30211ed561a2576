"""What a leapfrog step of the chains under the pure deep-learning surrogate costs (model="ml") in its three forms, at the reference's
sizes (n = 1597, 3 units of 50, 40 outputs, n_leapfrog = 10).  One JSON object (stdout, and --out FILE, default
profiles/hmc_ml_probe.json):

  leapfrog   us per leapfrog step at C = 4, 64, 256, 1024 under the i.i.d. prior and under the Gaussian-field prior, for
               torch_op     run_chains_device(fused=False): the torch-op form, the code as it was before ml_form= existed;
               steps        ml_form="steps": finrom_hmc_begin, 10 x finrom_hmc_leapfrog_ml (3 launches each), finrom_hmc_end;
               trajectory   ml_form="trajectory": finrom_hmc_begin, ONE finrom_hmc_trajectory_ml launch, finrom_hmc_end;
             and per (prior, C) whether "trajectory" is ahead of "torch_op" by more than three times the larger spread;
  da         us per ten-step delayed-acceptance proposal (correct=Fin: one full-order forward solve per proposal) at C = 4 and 64,
             i.i.d. prior, nine outputs (the fin's observables), the same three forms.

Every run is graph-replayed (asserted) and ends in a device synchronisation; a figure is the wall time of a long run minus a short one
(set-up and capture cancel) over the evaluations between them.  The forms of one (prior, C) are measured in turn and the turn
repeated --rounds times: median and spread (min, max) of the rounds.
usage (GPU box): python tools/hmc_ml_probe.py [--out FILE] [--quick] [--rounds R] [--skip-da]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMS = {"torch_op": dict(fused=False), "steps": dict(ml_form="steps"), "trajectory": dict(ml_form="trajectory")}


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmc_ml_probe.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes, one round: a rehearsal of the paths, not a measurement")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-da", action="store_true")
    a = ap.parse_args()
    import torch
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
    from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel, Surrogate
    from bayesianinferencedl_amd.fom.thermal_fin import get_space
    _ffi.check(_ffi.lib().finrom_set_device(0))
    torch.cuda.init()
    V = get_space(None, m=4 if a.quick else 12)
    n = V.dim()
    n_leap = 10
    rounds = 1 if a.quick else max(3, a.rounds)
    n1, n2 = (21, 61) if a.quick else (201, 1201)
    res = {"device": torch.cuda.get_device_name(0), "n": n, "n_leapfrog": n_leap, "rounds": rounds, "evals_short_long": [n1, n2]}
    prior = GaussianFieldPrior(V, amplitude=0.1, mean=1.0)

    def surrogate(n_out, data):
        m = ResBnFcModel(n, n_out, 3, 50, seed=2)
        m.head["b"] = np.asarray(data, dtype=np.float32)       # (an untrained network whose outputs sit at the observations)
        return Surrogate(m)

    def run(sur, data, C, n_evals, field, **kw):
        if field:
            x0 = np.stack([0.1 * np.random.default_rng(6 + c).standard_normal(n) for c in range(C)])
        else:
            x0 = np.stack([np.exp(0.1 * np.random.default_rng(6 + c).standard_normal(n)) for c in range(C)])
        t0 = time.perf_counter()
        r = hmc.run_chains_device(None, x0, n_evals, seeds=list(range(100, 100 + C)), eps=0.01, n_leapfrog=n_leap, sigma=0.05, tau=0.5,
                                  rng="philox", model="ml", surrogate=sur, data=data, prior=prior if field else None, **kw)
        torch.cuda.synchronize()
        assert r.graph, "the run was not graph-replayed"
        return time.perf_counter() - t0, r

    def measure(sur, data, C, field, per_what, **kw):
        """{form: stat} of the three forms in alternating rounds."""
        v, info = {f: [] for f in FORMS}, {}
        for f, fk in FORMS.items():                            # warm-up of every form (workspaces, function attributes)
            run(sur, data, C, n1, field, **fk, **kw)
        for _ in range(rounds):
            for f, fk in FORMS.items():
                t1 = run(sur, data, C, n1, field, **fk, **kw)[0]
                t2, r = run(sur, data, C, n2, field, **fk, **kw)
                v[f].append((t2 - t1) * 1e6 / ((n2 - n1) / (1 if per_what == "step" else n_leap)))
                info[f] = dict(fused=bool(r.get("fused")), ml_form=r.get("ml_form"), accept_rate=float(r.accept.mean() / r.proposals))
        row = {f: dict(stat(v[f]), **info[f]) for f in FORMS}
        larger = max(row["torch_op"]["spread"], row["trajectory"]["spread"])
        row["trajectory_ahead_of_torch_op_us"] = row["torch_op"]["median"] - row["trajectory"]["median"]
        row["three_times_larger_spread_us"] = 3 * larger
        row["trajectory_beats_torch_op"] = bool(row["trajectory_ahead_of_torch_op_us"] > 3 * larger)
        return row

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    data40 = np.random.default_rng(3).uniform(0.2, 1.0, 40)
    sur40 = surrogate(40, data40)
    res["n_out"] = 40
    res["leapfrog"] = {"iid": {}, "field": {}}
    res["da"] = "not measured"
    for C in ((4,) if a.quick else (4, 64, 256, 1024)):
        for name, field in (("iid", False), ("field", True)):
            res["leapfrog"][name][str(C)] = measure(sur40, data40, C, field, "step")
            write()                                            # (what has been measured is kept if the run is cut short)
    if not a.skip_da:
        from bayesianinferencedl_amd.fom.forward_solve import Fin
        fin = Fin(V)
        k_true = np.exp(0.25 * np.random.default_rng(11).standard_normal(n))
        data9 = np.asarray(fin.qoi_operator(fin.forward(k_true)[0]))
        sur9 = surrogate(len(data9), data9)
        res["da"] = {str(C): measure(sur9, data9, C, False, "proposal", correct=fin) for C in ((4,) if a.quick else (4, 64))}
    print(json.dumps(res, indent=1))
    write()


if __name__ == "__main__":
    main()
