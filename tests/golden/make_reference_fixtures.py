#!/usr/bin/env python3
"""Generates tests/golden/reference_fixtures.npz from a checkout of the reference repository.

The suite must not read the reference itself, so what tests/test_oracle.py pins against it is stored here as data:
  B_obs_data, B_obs_rom   data/B_obs.txt and rom/B_obs.txt as parsed by np.loadtxt(delimiter=",")
  basis_five_first_row    the first row of data/basis_five_param.txt
  enrich_basis, enrich_w  seeded inputs of the Gram-Schmidt `enrich` of rom/model_constr_adaptive_sampling.py
  enrich_out              what the reference's `enrich` returns for them
Run from the repo root:  python tests/golden/make_reference_fixtures.py <path of the reference checkout>"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    out = {"B_obs_data": np.loadtxt(os.path.join(ref, "data", "B_obs.txt"), delimiter=","),
           "B_obs_rom": np.loadtxt(os.path.join(ref, "rom", "B_obs.txt"), delimiter=",")}
    with open(os.path.join(ref, "data", "basis_five_param.txt")) as f:
        out["basis_five_first_row"] = np.array([float(v) for v in f.readline().split(",")])
    spec = importlib.util.spec_from_file_location("ref_mcas", os.path.join(ref, "rom", "model_constr_adaptive_sampling.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(9)
    basis = np.linalg.qr(rng.standard_normal((50, 6)))[0]
    w = rng.standard_normal((50, 1))
    out.update(enrich_basis=basis, enrich_w=w, enrich_out=np.asarray(mod.enrich(basis.copy(), w.copy()), dtype=np.float64))
    path = os.path.join(HERE, "reference_fixtures.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
