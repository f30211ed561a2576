"""Cost of the latent Gaussian-field prior in the HMC step (hmc.run_chains_device(prior=...), finrom_hmc_leapfrog_field).

Reports, as one JSON object (stdout, and --out FILE):
  * us per leapfrog step of the fused, graph-replayed chains (m = 12, r = 81, n = 1597) with the i.i.d. prior and with the
    Gaussian-field prior, at C = 4 and C = 64 chains: the wall time of a run with N2 evaluations minus one with N1, per step
    (set-up, capture and the first evaluation cancel);
  * the two triangular products alone (finrom_sampler_field / _pullback) at n = 1597 and n = 4101 for S = 1, 4, 64: the kernel time
    per launch from the library's profile slot (misc) and the wall time per call on a torch stream.
usage (GPU box): python tools/hmc_prior_probe.py [--out FILE] [--quick]   (--quick: few iterations, for a profiler run)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def products(n, sizes, iters):
    import torch
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.engine import FieldSampler
    rng = np.random.default_rng(n)
    U = np.triu(rng.standard_normal((n, n))) / np.sqrt(n)
    U[np.diag_indices(n)] = np.abs(U[np.diag_indices(n)]) + 1.0
    fs = FieldSampler(U)
    L = _ffi.lib()
    out = {}
    for S in sizes:
        v = torch.randn(S, n, dtype=torch.float64, device="cuda")
        mean = torch.ones(n, dtype=torch.float64, device="cuda")
        for name, call in (("field", lambda: fs.field(v, mean=mean)), ("pullback", lambda: fs.pullback(v))):
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            L.finrom_profile_reset(); L.finrom_profile_enable(1)
            t0 = time.perf_counter()
            for _ in range(iters):
                call()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / iters
            L.finrom_profile_enable(0)
            cnt, ms = _ffi.profile_read()["misc"]
            out[f"{name}_n{n}_S{S}"] = {"kernel_us": round(ms / cnt * 1e3, 2), "wall_us_per_call": round(wall * 1e6, 2)}
            print(name, n, S, out[f"{name}_n{n}_S{S}"], flush=True)
    fs.close()
    return out


def steps(chains, n_short, n_long):
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
            t = {}
            for N in (n_short, n_long, n_short, n_long):                 # (twice each: the first pair warms everything up)
                t0 = time.perf_counter()
                res = hmc.run_chains_device(rom, x0, N, seeds=seeds, eps=1e-2, n_leapfrog=10, fused=True, graph=True, **kw)
                t[N] = time.perf_counter() - t0
                assert res.graph and res.fused
            us = (t[n_long] - t[n_short]) / (n_long - n_short) * 1e6
            out[f"{form}_C{C}"] = {"us_per_leapfrog_step": round(us, 2), "evals": [n_short, n_long]}
            print(form, C, out[f"{form}_C{C}"], flush=True)
        out[f"prior_minus_iid_C{C}_us"] = round(out[f"prior_C{C}"]["us_per_leapfrog_step"] - out[f"iid_C{C}"]["us_per_leapfrog_step"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch
    from bayesianinferencedl_amd import _ffi
    _ffi.check(_ffi.lib().finrom_set_device(0))
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0)}
    it = 20 if a.quick else 200
    for n in (1597, 4101):
        res.update(products(n, (1, 4, 64), it))
    res.update(steps((4, 64), 101, 301) if a.quick else steps((4, 64), 201, 1201))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
