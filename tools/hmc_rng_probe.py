"""What the HMC chains' random numbers cost: host NumPy generators + upload (rng="numpy") against one finrom_hmc_draw launch per
block (rng="philox"), hmc.run_chains_device fused and graph-replayed.

Reports, as one JSON object (stdout, and --out FILE):
  * us per leapfrog step (m = 12, r = 81, n = 1597, L = 10, block = 32) at C = 4 and C = 64 chains, i.i.d. prior and Gaussian-field
    prior, each with rng="numpy" and rng="philox": tools/hmc_prior_probe.py's set-up and timing -- the wall time of a run with N2
    evaluations minus one with N1, per step (set-up, capture and the first evaluation cancel; every run ends in a device-to-host
    copy of the end state).  Each point is repeated --repeats times, numpy and philox alternating inside a repeat, after one
    untimed pair per rng: the list, its median and its spread (max - min) are reported, so that a difference can be held against
    the numpy runs' own spread;
  * the host loop of rng="numpy" alone (hmc.py: per proposal and chain n normals, then one uniform per chain), per block of 32
    proposals, without and with the two uploads, at (C, n) = (4, 1597), (64, 1597), (64, 4101);
  * finrom_hmc_draw alone at (B, C, n) = (32, 64, 1597) and (32, 64, 4101): device-event time per launch over back-to-back launches.
usage (GPU box): python tools/hmc_rng_probe.py [--out FILE] [--quick] [--repeats R]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_loop(B, C, n, iters):
    """The draws of one block as rng="numpy" makes them, and the same followed by the two uploads (pageable memory, synchronised)."""
    import torch
    rngs = [np.random.default_rng(100 + c) for c in range(C)]
    P_dev = torch.zeros(B, C, n, dtype=torch.float64, device="cuda")
    lu_dev = torch.zeros(B, C, dtype=torch.float64, device="cuda")

    def block():
        P_host, lu_host = np.zeros((B, C, n)), np.zeros((B, C))
        for j in range(B):
            for c_, r in enumerate(rngs):
                P_host[j, c_] = r.standard_normal(n)
            lu_host[j] = np.log(np.array([r.uniform() for r in rngs]))
        return P_host, lu_host

    block()
    t_loop, t_all = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        P_host, lu_host = block()
        t1 = time.perf_counter()
        P_dev.copy_(torch.from_numpy(P_host)); lu_dev.copy_(torch.from_numpy(lu_host))
        torch.cuda.synchronize()
        t_loop.append(t1 - t0); t_all.append(time.perf_counter() - t0)
    return {"loop_ms_per_block": round(statistics.median(t_loop) * 1e3, 3), "loop_and_upload_ms_per_block": round(statistics.median(t_all) * 1e3, 3),
            "loop_ms_spread": round((max(t_loop) - min(t_loop)) * 1e3, 3), "iters": iters}


def draw_kernel(B, C, n, iters):
    import torch
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    seeds = torch.arange(100, 100 + C, dtype=torch.int64, device="cuda")
    P = torch.zeros(B, C, n, dtype=torch.float64, device="cuda")
    lu = torch.zeros(B, C, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(first):
        _ffi.check(L.finrom_hmc_draw(seeds.data_ptr(), C, n, first, B, P.data_ptr(), lu.data_ptr(), st), "finrom_hmc_draw")

    for i in range(10):
        call(i * B)
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            call(i * B)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) / iters * 1e3)
    return {"us_per_launch": round(statistics.median(us), 2), "us_spread": round(max(us) - min(us), 2), "launches": iters,
            "GB_per_s_written": round(B * C * n * 8 / (statistics.median(us) * 1e-6) / 1e9, 1)}


def steps(chains, n_short, n_long, repeats):
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
    out = {}
    for C in chains:
        seeds = [100 + c for c in range(C)]
        K0 = np.exp(0.1 * np.random.default_rng(6).standard_normal((C, V.dim())))
        V0 = np.random.default_rng(6).standard_normal((C, V.dim()))
        for form, x0, kw in (("iid", K0, {}), ("prior", V0, {"prior": prior})):
            us = {"numpy": [], "philox": []}
            for rep in range(repeats + 1):                               # (repeat 0 warms everything up and is not kept)
                for rng in ("numpy", "philox"):
                    t = {}
                    for N in (n_short, n_long):
                        t0 = time.perf_counter()
                        res = hmc.run_chains_device(rom, x0, N, seeds=seeds, eps=1e-2, n_leapfrog=10, fused=True, graph=True, rng=rng, **kw)
                        t[N] = time.perf_counter() - t0
                        assert res.graph and res.fused
                    if rep:
                        us[rng].append(round((t[n_long] - t[n_short]) / (n_long - n_short) * 1e6, 2))
            for rng in us:
                out[f"{form}_C{C}_{rng}"] = {"us_per_leapfrog_step": us[rng], "median": round(statistics.median(us[rng]), 2),
                                             "spread": round(max(us[rng]) - min(us[rng]), 2), "evals": [n_short, n_long]}
                print(form, C, rng, out[f"{form}_C{C}_{rng}"], flush=True)
            out[f"{form}_C{C}_philox_minus_numpy_us"] = round(out[f"{form}_C{C}_philox"]["median"] - out[f"{form}_C{C}_numpy"]["median"], 2)
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
    res = {"device": torch.cuda.get_device_name(0), "host_cpus_usable": len(os.sched_getaffinity(0)), "block": 32, "n_leapfrog": 10}
    for B, C, n in ((32, 64, 1597), (32, 64, 4101)):
        res[f"draw_kernel_B{B}_C{C}_n{n}"] = draw_kernel(B, C, n, 20 if a.quick else 200)
        print("draw kernel", B, C, n, res[f"draw_kernel_B{B}_C{C}_n{n}"], flush=True)
    for C, n in ((4, 1597), (64, 1597), (64, 4101)):
        res[f"host_loop_B32_C{C}_n{n}"] = host_loop(32, C, n, 2 if a.quick else 5)
        print("host loop", C, n, res[f"host_loop_B32_C{C}_n{n}"], flush=True)
    res.update(steps((4, 64), 101, 301, max(1, a.repeats if not a.quick else 1)) if a.quick else steps((4, 64), 201, 1201, max(1, a.repeats)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
