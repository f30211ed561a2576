"""Cost of a leaf inside the tree of the device-resident No-U-turn chains under the full-order model, the plain reduced model and
the reduced model with its learned correction (hmc.run_chains_device(model="fom" | "rom" | "romml", nuts=Nuts(7)): one leaf per round,
finrom_hmc_nuts_begin / _leaf / _end around the model's own launches), at the bench's shape (m = 12, r = 81, n = 1597).

Reports, as one JSON object (stdout, and --out FILE), for C = 4 and C = 64 chains, three models, both priors, graph-replayed:
  * `device`: us per ROUND (one leaf of every chain still inside its tree), and the read-backs per transition;
  * baseline (a) `host`: hmc.run_chains(nuts=) over romml_ / rom_ / fom_value_and_grad -- the only No-U-turn form these models had
    before: a host recursion, chain by chain, one S = 1 device call and one read-back per leaf -- as us per leaf of ONE chain and as
    us per round of the same C chains (the host's time for the work a device round does: its time over the device's rounds).  At
    C = 64 the host walks chains 0 .. 3 of the 64 (the same seeds) and its time is scaled by 16: its recursion is chain by chain,
    and the full-order model's 64 x 127 leaves of 3 ms each would not fit a probe; `host_scaled` says so per entry;
  * baseline (b) `fixed`: the same model's fused fixed-length step (run_chains_device(fused=True), 10 steps per proposal), us per step:
    device minus fixed is what the tree costs per leaf;
  * `leaf_kernel`: finrom_hmc_nuts_leaf alone, us per launch in stream order, on free-flying chains that stay inside their trees.
A figure is the wall time of a long run minus a short one over the difference of their rounds (steps, leaves): set-up, capture and
the first evaluation cancel; every run ends in a device synchronisation.  The forms of one (model, prior, C) are measured in turn,
the whole turn repeated `--rounds` times (default seven) after one warm-up turn; median [min, max] are reported.
usage (GPU box): python tools/hmc_nuts_model_probe.py [--out FILE] [--quick] [--rounds R]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEPTH = 7


def leaf_kernel_alone(C, n, launches):
    """us per finrom_hmc_nuts_leaf launch (HIP events around `launches` launches in stream order): zero gradient and misfit and an
    all but flat prior, so every chain flies straight, never turns or diverges and stays inside a tree of depth 10."""
    import torch
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    f64 = dict(dtype=torch.float64, device="cuda")
    z = lambda *s: torch.zeros(*s, **f64)
    K, P_block = torch.randn(C, n, **f64), torch.randn(1, C, n, **f64)
    t = dict(mean=K.clone(), K=K, U=z(C), dU=z(C, n), Kq0=z(C, n), Kq1=z(C, n), P=z(C, n), dUq=z(C, n), H0=z(C), P_block=P_block, lu=z(1, C),
             jt=torch.zeros(1, dtype=torch.int64, device="cuda"), pt=torch.zeros(1, dtype=torch.int64, device="cuda"),
             acc=torch.zeros(C, dtype=torch.int64, device="cuda"), loss=z(C), info=torch.zeros(C, dtype=torch.int32, device="cuda"), grad=z(C, n),
             ws=z(L.finrom_hmc_nuts_ws_bytes(C, n, 10) // 8), seeds=torch.arange(C, dtype=torch.int64, device="cuda"), sl=z(C),
             active=torch.zeros(C, dtype=torch.int32, device="cuda"))
    p = {k: v.data_ptr() for k, v in t.items()}
    st = _ffi.HmcState(C=C, n=n, eps=1e-3, c_lik=1.0, c_pri=1e-12, mean=p["mean"], K=p["K"], U=p["U"], dU=p["dU"],
                       Kq=(ctypes.c_void_p * 2)(p["Kq0"], p["Kq1"]), P=p["P"], dUq=p["dUq"], H0=p["H0"], P_block=p["P_block"], lu_block=p["lu"],
                       jt=p["jt"], pt=p["pt"], accept=p["acc"], trace=None, loss=p["loss"], info=p["info"])
    tr = _ffi.HmcNutsTree(ws=p["ws"], seeds=p["seeds"], proposal0=0, max_depth=10, state_loss=p["sl"], tree=None, accept_stat=None,
                          active=p["active"])
    s = torch.cuda.current_stream().cuda_stream
    out = []
    for _ in range(3):                                               # (the first pass warms up)
        _ffi.check(L.finrom_hmc_nuts_begin(ctypes.byref(st), ctypes.byref(tr), None, None, 0, None, s), "finrom_hmc_nuts_begin")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            _ffi.check(L.finrom_hmc_nuts_leaf(ctypes.byref(st), ctypes.byref(tr), p["grad"], None, None, None, 0, None, s), "finrom_hmc_nuts_leaf")
        e1.record()
        torch.cuda.synchronize()
        assert bool(t["active"].all()), "a chain left its tree: the launches timed were not all leaves"
        out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return [round(statistics.median(out[1:]), 2), round(min(out[1:]), 2), round(max(out[1:]), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="short runs, one round: a rehearsal of the paths, not a measurement")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    import bench
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
    from bayesianinferencedl_amd.bayesian_inference.nuts import Nuts
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.fom.thermal_fin import get_space
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    from bayesianinferencedl_amd.rom.basis import pod_basis
    _ffi.check(_ffi.lib().finrom_set_device(0))
    torch.cuda.init()
    V = get_space(None, m=12)
    n = V.dim()
    fin = Fin(V)
    phi = pod_basis(fin, 81, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1)
    rom = AffineROMFin(V, bench.hmc_error_model(n), phi)
    k_true = np.exp(0.25 * np.random.default_rng(11).standard_normal(n))
    data = fin.qoi_operator(fin.forward(k_true)[0])
    rom.set_data(data)
    prior = GaussianFieldPrior(V, amplitude=0.1, mean=1.0)
    host_f = {"romml": hmc.romml_value_and_grad(rom), "rom": hmc.rom_value_and_grad(rom), "fom": hmc.fom_value_and_grad(fin, data)}
    # transitions of the short and the long run (a transition is up to 127 rounds), evaluations of the fixed-length runs
    trans = {"romml": (1, 9), "rom": (1, 9), "fom": (1, 3), "host_romml": (1, 3), "host_rom": (1, 3), "host_fom": (1, 2)}
    evals = {"romml": (201, 2201), "rom": (201, 2201), "fom": (51, 251)}
    if a.quick:
        trans, evals = {k: (1, 2) for k in trans}, {k: (21, 61) for k in evals}
    rounds = 1 if a.quick else a.rounds
    HOST_CHAINS = 4
    res = {"device": torch.cuda.get_device_name(0), "n": n, "r": 81, "max_depth": DEPTH, "rounds": rounds, "transitions": trans, "evals": evals,
           "unit": "us: median [min, max] over the rounds", "host_chains": HOST_CHAINS}
    for C in (4, 64):
        res[f"leaf_kernel_C{C}"] = leaf_kernel_alone(C, n, 20 if a.quick else 500)
        print(f"leaf_kernel_C{C}", res[f"leaf_kernel_C{C}"], flush=True)

    def timed(run, N):
        t0 = time.perf_counter()
        out = run(N)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for C in (4, 64):
        seeds = [100 + c for c in range(C)]
        K0 = np.exp(0.1 * np.random.default_rng(6).standard_normal((C, n)))
        V0 = np.random.default_rng(6).standard_normal((C, n))
        Ch = min(C, HOST_CHAINS)
        for pname, x0, pkw in (("iid", K0, {}), ("field", V0, {"prior": prior})):
            for model in ("romml", "rom", "fom"):
                solver_r = None if model == "fom" else rom
                common = dict(eps=1e-2, **pkw)
                nkw = dict(n_leapfrog=1, rng="philox", nuts=Nuts(DEPTH), **common)
                dkw = dict(model=model, solver=fin if model == "fom" else None, data=data, graph=True)
                forms = {
                    "device": (trans[model], lambda T: hmc.run_chains_device(solver_r, x0, 1 + T, seeds=seeds, **dkw, **nkw)),
                    "host": (trans["host_" + model], lambda T: hmc.run_chains(host_f[model], x0[:Ch], 1 + T, seeds=seeds[:Ch], **nkw)),
                    "fixed": (evals[model], lambda N: hmc.run_chains_device(solver_r, x0, N, seeds=seeds, fused=True, n_leapfrog=10, **dkw, **common)),
                }
                samples = {k: [] for k in ("device", "host_leaf", "host_round", "fixed", "ratio")}
                readbacks = None
                for rnd in range(rounds + 1):                            # (round 0 warms every form up and is dropped)
                    got = {}
                    for f, ((n1, n2), run) in forms.items():             # the forms in turn, so that drift of the host hits all alike
                        t1, r1 = timed(run, n1)
                        t2, r2 = timed(run, n2)
                        got[f] = (t2 - t1, r1, r2)
                    dt, r1, r2 = got["device"]
                    assert r2.graph and r2.fused and r2.model == model and r2.nuts == DEPTH
                    d_rounds = r2.nuts_rounds - r1.nuts_rounds
                    readbacks = r2.nuts_readbacks / r2.proposals
                    ht, h1, h2 = got["host"]
                    h_leaves = int(h2.tree[:, :, 1].sum() - h1.tree[:, :, 1].sum())
                    # the host's rounds: the leaves of the longest tree per transition, as the device counts its own
                    h_rounds = int(h2.tree[:, :, 1].max(axis=1).sum() - h1.tree[:, :, 1].max(axis=1).sum())
                    ft, f1, f2 = got["fixed"]
                    if rnd or a.quick:
                        samples["device"].append(dt / d_rounds * 1e6)
                        samples["host_leaf"].append(ht / h_leaves * 1e6)
                        samples["host_round"].append(ht * (C / Ch) / h_rounds * 1e6)
                        samples["fixed"].append(ft / (forms["fixed"][0][1] - forms["fixed"][0][0]) * 1e6)
                        samples["ratio"].append(samples["host_round"][-1] / samples["device"][-1])
                key = f"{model}_{pname}_C{C}"
                res[key] = {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in samples.items()}
                res[key].update(readbacks_per_transition=round(readbacks, 2), host_scaled=C // Ch,
                                tree_cost_per_leaf=round(res[key]["device"][0] - res[key]["fixed"][0], 2))
                print(key, res[key], flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
