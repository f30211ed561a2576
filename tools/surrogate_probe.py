"""What the pure deep-learning surrogate costs (finrom_mlp_misfit_grad, model="ml"), at the reference's sizes (n = 1597, 3 units of
50, 40 outputs).  One JSON object (stdout, and --out FILE, default profiles/surrogate_probe.json):

  per_sample   us per misfit_grad call (value and gradient) in the per-sample form at S = 1, 4, 64;
  batches      at S = 65, 256, 4096, 100 000: forward only (prediction) and value-and-gradient, in the tile form and in the per-sample
               form (set_tile_min above S), and finrom_mlp_predict at the same inputs -- the entry point this change leaves alone: it
               launches the kernel it launched before, so it is the yardstick and never the code under test.  GB/s = the bytes of k
               (forward: S n 8; value and gradient: k in, grad out, 2 S n 8) over the median time, beside the HBM peak;
  leapfrog     us per leapfrog step of run_chains_device(model="ml") at C = 4 / 64 / 1024, graph-replayed, with model="romml" beside
               it (C = 4, 64: its fused form; 1024: the torch-op form);
  da           us per delayed-acceptance proposal (ten steps under "ml", the FOM deciding) at C = 4 and 64.

Device events around `reps` back-to-back calls on one stream; every shape is warmed up first; the series of one S are measured in
turn and the turn repeated `--rounds` times: median and spread (min, max) of the rounds.  The chain figures are the wall time of a
long run minus a short one (set-up and capture cancel), every run ending in a device synchronisation.  --skip-chains leaves the last
two out ("not measured").
usage (GPU box): python tools/surrogate_probe.py [--out FILE] [--quick] [--rounds R] [--skip-chains]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0                      # MI355X: 8 TB/s HBM3E (spec)


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surrogate_probe.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes, one round: a rehearsal of the paths, not a measurement")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-chains", action="store_true")
    a = ap.parse_args()
    import torch
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel, Surrogate
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    L = _ffi.lib()
    _ffi.check(L.finrom_set_device(0))
    torch.cuda.init()
    n, n_out = 1597, 40
    rng = np.random.default_rng(0)
    model = ResBnFcModel(n, n_out, 3, 50, seed=1)
    model.b0 = rng.normal(0, 0.3, 50).astype(np.float32)
    dev = DeviceErrorModel(model)
    f64 = dict(dtype=torch.float64, device="cuda")
    data = torch.rand(n_out, **f64)
    rounds = 1 if a.quick else a.rounds
    res = {"device": torch.cuda.get_device_name(0), "n": n, "n_out": n_out, "rounds": rounds, "hbm_peak_GBs": HBM_PEAK_GBS}

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps          # us per call

    # 1. the per-sample form, one call at a time
    res["per_sample"] = {}
    for S in (1, 4, 64):
        Kt = torch.exp(0.3 * torch.randn(S, n, **f64))
        dev.set_tile_min(1 << 40)
        fn = lambda: dev.misfit_grad(Kt, data)
        timed(fn, 20)
        res["per_sample"][str(S)] = dict(stat([timed(fn, 200) for _ in range(rounds)]), form=dev.last_form())
    # 2. batches: the series of one S in turn
    res["batches"] = {}
    for S in ((65, 256) if a.quick else (65, 256, 4096, 100000)):
        Kt = torch.exp(0.3 * torch.randn(S, n, **f64))
        reps = 3 if S >= 100000 else 20 if S >= 4096 else 100

        def series(tile, grad):
            def fn():
                dev.set_tile_min(1 if tile else 1 << 40)
                if grad:
                    dev.misfit_grad(Kt, data)
                else:
                    dev.misfit_grad(Kt, None, want_grad=False)
            return fn
        runs = {"tile_forward": series(True, False), "tile_value_grad": series(True, True), "per_sample_forward": series(False, False),
                "per_sample_value_grad": series(False, True), "mlp_predict": lambda: dev.predict(Kt)}
        for fn in runs.values():
            timed(fn, 2)
        t = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                t[k].append(timed(fn, reps))
        row = {}
        for k, v in t.items():
            row[k] = stat(v)
            bytes_ = S * n * 8 * (2 if k.endswith("value_grad") else 1)
            row[k]["GBs"] = bytes_ / (row[k]["median"] * 1e-6) / 1e9
            row[k]["share_of_hbm_peak"] = row[k]["GBs"] / HBM_PEAK_GBS
        spread = max(row[k]["max"] - row[k]["min"] for k in ("tile_forward", "mlp_predict"))
        row["tile_forward_ahead_of_mlp_predict_us"] = row["mlp_predict"]["median"] - row["tile_forward"]["median"]
        row["three_times_larger_spread_us"] = 3 * spread
        row["tile_forward_ahead"] = bool(row["tile_forward_ahead_of_mlp_predict_us"] > 3 * spread)
        row["tile_value_grad_ahead_of_per_sample"] = bool(row["per_sample_value_grad"]["median"] > row["tile_value_grad"]["median"])
        res["batches"][str(S)] = row
        del Kt
        torch.cuda.empty_cache()
    dev.set_tile_min(4096)
    res["leapfrog"] = res["da"] = "not measured"

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    write()                                                # (the kernels' figures are kept if the chains' part is cut short)
    if not a.skip_chains:
        chains(res, a, model, rounds)
    print(json.dumps(res, indent=1))
    write()


def chains(res, a, model, rounds):
    import bench
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel, Surrogate
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.fom.thermal_fin import get_space
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    from bayesianinferencedl_amd.rom.basis import pod_basis
    import torch
    V = get_space(None, m=12)
    n = V.dim()
    fin = Fin(V)
    phi = pod_basis(fin, 81, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1)
    rom = AffineROMFin(V, bench.hmc_error_model(n), phi)
    k_true = np.exp(0.25 * np.random.default_rng(11).standard_normal(n))
    data = np.asarray(fin.qoi_operator(fin.forward(k_true)[0]))
    rom.set_data(data)
    m9 = ResBnFcModel(n, len(data), 3, 50, seed=2)
    m9.head["b"] = data.astype(np.float32)                 # (an untrained network whose outputs sit at the observations)
    sur = Surrogate(m9)
    n_leap = 10
    n1, n2 = (21, 61) if a.quick else (201, 1201)

    def run(C, n_evals, **kw):
        K0 = np.stack([np.exp(0.1 * np.random.default_rng(6 + c).standard_normal(n)) for c in range(C)])
        t0 = time.perf_counter()
        r = hmc.run_chains_device(kw.pop("solver_r", None), K0, n_evals, seeds=list(range(100, 100 + C)), eps=0.01, n_leapfrog=n_leap,
                                  sigma=0.05, tau=0.5, rng="philox", **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def per(C, per_what, **kw):
        run(C, n1, **kw)
        v = []
        for _ in range(rounds):
            t1 = run(C, n1, **kw)[0]
            t2, r = run(C, n2, **kw)
            v.append((t2 - t1) * 1e6 / ((n2 - n1) / (1 if per_what == "step" else n_leap)))
        return dict(stat(v), graph=bool(r.get("graph")), fused=bool(r.get("fused")), accept_rate=float(r.accept.mean() / r.proposals))
    res["leapfrog"] = {}
    for C in ((4,) if a.quick else (4, 64, 1024)):
        res["leapfrog"][str(C)] = {"ml": per(C, "step", model="ml", surrogate=sur, data=data),
                                   "romml": per(C, "step", solver_r=rom, model="romml")}
    res["da"] = {str(C): {"ml_fom": per(C, "proposal", model="ml", surrogate=sur, data=data, correct=fin)}
                 for C in ((4,) if a.quick else (4, 64))}


if __name__ == "__main__":
    main()
