"""What the chains' streaming posterior summaries cost: hmc.run_chains_device fused and graph-replayed, rng="philox", with and
without stats=ChainStats (one finrom_hmc_stats_update launch more in every proposal's graph).

Reports, as one JSON object (stdout, and --out FILE):
  * us per PROPOSAL (m = 12, r = 81, n = 1597, L = 10, block = 32) at C = 4 and C = 64 chains, i.i.d. prior and Gaussian-field
    prior, each without and with stats=: tools/hmc_rng_probe.py's set-up and timing -- the wall time of a run with N2 evaluations
    minus one with N1, per proposal (set-up, capture and the first evaluation cancel; every run ends in a device-to-host copy of
    the end state, with stats= also of the [C, n] sums and the [proposals + 1, C] rows).  Each point is repeated --repeats times,
    the two alternating inside a repeat, after one untimed pair: the list, its median and its spread (max - min) are reported, so
    that the difference can be held against the plain runs' own spread;
  * finrom_hmc_stats_update alone at (C, n) = (4, 1597), (64, 1597) and (64, 4101): device-event time per launch over back-to-back
    launches (the counter held at 1, so every launch sees an accepted proposal and closes a batch of one: the most traffic a
    launch can have), and the bytes a launch moves at 72 B per (chain, node);
  * the bytes the kept trace of the same run would have taken ((proposals + 1) x C x n doubles) against the stats' buffers.
usage (GPU box): python tools/hmc_stats_probe.py [--out FILE] [--quick] [--repeats R]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats_kernel(C, n, iters):
    import torch
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    f64 = dict(dtype=torch.float64, device="cuda")
    i64 = dict(dtype=torch.int64, device="cuda")
    cand, cur = torch.randn(C, n, **f64), torch.randn(C, n, **f64)
    cand_loss, cur_loss = torch.rand(C, **f64), torch.rand(C, **f64)
    sums = [torch.zeros(C, n, **f64) for _ in range(5)]
    pt, acc, acc_prev = torch.ones(1, **i64), torch.ones(C, **i64), torch.zeros(2, C, **i64)     # pt stays 1: slot 0 is read, slot 1 written
    desc = _ffi.HmcStats(C=C, n=n, proposal0=0, burn=0, batch=1, pt=pt.data_ptr(), accept=acc.data_ptr(), cand=cand.data_ptr(),
                         cand_loss=cand_loss.data_ptr(), cur=cur.data_ptr(), cur_loss=cur_loss.data_ptr(), acc_prev=acc_prev.data_ptr(),
                         mean=sums[0].data_ptr(), m2=sums[1].data_ptr(), bsum=sums[2].data_ptr(), bm_mean=sums[3].data_ptr(),
                         bm_m2=sums[4].data_ptr(), misfit=None, accepted=None)
    st = torch.cuda.current_stream().cuda_stream

    def call():
        _ffi.check(L.finrom_hmc_stats_update(ctypes.byref(desc), st), "finrom_hmc_stats_update")

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) / iters * 1e3)
    return {"us_per_launch": round(statistics.median(us), 2), "us_spread": round(max(us) - min(us), 2), "launches": iters,
            "bytes_per_launch_at_72B": 72 * C * n}


def proposals(chains, n_short, n_long, repeats, batch):
    import bench
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.fom.thermal_fin import get_space
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    from bayesianinferencedl_amd.rom.basis import pod_basis
    V = get_space(None, m=12)
    fin = Fin(V)
    phi = pod_basis(fin, 81, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1)
    rom = AffineROMFin(V, bench.hmc_error_model(V.dim()), phi)
    k_true = np.exp(0.25 * np.random.default_rng(11).standard_normal(V.dim()))
    rom.set_data(fin.qoi_operator(fin.forward(k_true)[0]))
    prior = GaussianFieldPrior(V, amplitude=0.1, mean=1.0)
    L, out = 10, {}
    for C in chains:
        seeds = [100 + c for c in range(C)]
        K0 = np.exp(0.1 * np.random.default_rng(6).standard_normal((C, V.dim())))
        V0 = np.random.default_rng(6).standard_normal((C, V.dim()))
        for form, x0, kw in (("iid", K0, {}), ("prior", V0, {"prior": prior})):
            us = {"plain": [], "stats": []}
            for rep in range(repeats + 1):                               # (repeat 0 warms everything up and is not kept)
                for which in ("plain", "stats"):
                    t = {}
                    for N in (n_short, n_long):
                        spec = hmc.ChainStats(burn=0, batch=batch) if which == "stats" else None
                        t0 = time.perf_counter()
                        res = hmc.run_chains_device(rom, x0, N, seeds=seeds, eps=1e-2, n_leapfrog=L, fused=True, graph=True, rng="philox",
                                                    stats=spec, **kw)
                        t[N] = time.perf_counter() - t0
                        assert res.graph and res.fused and (res.stats is None) == (spec is None)
                    if rep:
                        us[which].append(round((t[n_long] - t[n_short]) / ((n_long - n_short) // L) * 1e6, 2))
            for which in us:
                out[f"{form}_C{C}_{which}"] = {"us_per_proposal": us[which], "median": round(statistics.median(us[which]), 2),
                                               "spread": round(max(us[which]) - min(us[which]), 2), "evals": [n_short, n_long]}
                print(form, C, which, out[f"{form}_C{C}_{which}"], flush=True)
            out[f"{form}_C{C}_stats_minus_plain_us"] = round(out[f"{form}_C{C}_stats"]["median"] - out[f"{form}_C{C}_plain"]["median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    from bayesianinferencedl_amd import _ffi
    _ffi.check(_ffi.lib().finrom_set_device(0))
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "block": 32, "n_leapfrog": 10, "batch": 32}
    for C, n in ((4, 1597), (64, 1597), (64, 4101)):
        res[f"stats_kernel_C{C}_n{n}"] = stats_kernel(C, n, 20 if a.quick else 200)
        print("stats kernel", C, n, res[f"stats_kernel_C{C}_n{n}"], flush=True)
        for P in (10001,):
            res[f"bytes_C{C}_n{n}_P{P}"] = {"kept_trace": (P + 1) * C * n * 8, "stats_buffers": 6 * C * n * 8 + (P + 1) * C * 12 + 3 * C * 8}
    res.update(proposals((4, 64), 101, 301, 1, 32) if a.quick else proposals((4, 64), 201, 1201, max(1, a.repeats), 32))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
