"""GPU tests of the error model's trainer (csrc/mlp_train.hip through ctypes: engine.DeviceTrainer, ResBnFcModel.fit).
Yardstick: the host statement in float64 (ResBnFcModel.train_gradients / fit_host), which tests/test_train_host.py ties to torch
autograd.  Allowances for the fp32 kernels are multiples of what the host statement in fp32 deviates from the same yardstick on
the same data, computed here, with a floor of 4 ulp of fp32 at the tensor's largest entry."""
import copy

import numpy as np
import pytest

from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel
from train_cases import ULP32, deviations, leaves, perturbed, probe

pytestmark = pytest.mark.gpu


def cuda_rows(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()


# ---- 6. one batch: every gradient, batch statistic, loss, MAPE ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(245, 64, 50, 5, 9), (1597, 500, 50, 5, 9), (120, 33, 37, 2, 9), (1597, 4096, 50, 5, 9),
                                   (4101, 500, 50, 5, 9)])
def test_train_grad_matches_the_fp64_statement(shape):
    """Allowance per tensor: 16 x the deviation of train_gradients in fp32 from the fp64 yardstick on the same batch (both are
    fp32 evaluations of the same sums; the device's first-layer sums are sequential chains of up to K = 1597 terms, NumPy's are
    blocked; sqrt(K) = 40 is the statistical ceiling of the difference).  The measured factor per shape (device deviation over
    NumPy-fp32 deviation, the largest over the tensors) is printed.  Recorded on an MI355X: (245, 64) 1.5 (b0, 9.1e-8 against
    6.0e-8); (1597, 500) 1.3 (l3_gamma, 6.0e-7 / 4.5e-7); (120, 33, n_w 37) 0.9 (W0); (1597, 4096) 2.3 (l2_mean, 1.3e-7 / 5.6e-8);
    (4101, 500) 1.6 (l3_gamma); the largest device deviation of any tensor 2.9e-6, loss within 5.8e-8, MAPE within 2.0e-7."""
    from bayesianinferencedl_amd.engine import DeviceTrainer
    n_in, B, n_w, L, n_out = shape
    m = perturbed(n_in, n_w, L, n_out)
    X, Y = probe(n_in, B + 7, n_out)                                        # (the batch: rows 7 .. B + 6 through the index array)
    rows = np.arange(7, B + 7)
    l64, p64, g64 = m.train_gradients(X[rows], Y[rows], np.float64)
    l32, p32, g32 = m.train_gradients(X[rows], Y[rows], np.float32)
    dev32 = deviations(g32, g64)
    tr = DeviceTrainer(m, max_batch=B)
    try:
        tr.grad(tr.to_device(X, n_in), tr.to_device(Y, n_out), cuda_rows(rows))
        ld, pd, gd = tr.get_grads()
    finally:
        tr.close()
    devd = deviations(gd, g64)
    factor = {nm: devd[nm] / max(dev32[nm], ULP32 / 4) for nm in devd}
    worst = max(factor, key=factor.get)
    print(f"shape {shape}: device / NumPy-fp32 deviation, worst tensor {worst}: {devd[worst]:.3g} / {dev32[worst]:.3g};"
          f" largest device deviation {max(devd.values()):.3g}; loss {abs(ld - l64) / l64:.3g} (fp32 {abs(l32 - l64) / l64:.3g});"
          f" MAPE {abs(pd - p64) / p64:.3g} (fp32 {abs(p32 - p64) / p64:.3g})")
    for nm in devd:
        assert devd[nm] <= max(16 * dev32[nm], 4 * ULP32), (nm, devd[nm], dev32[nm])
    assert abs(ld - l64) <= max(16 * abs(float(l32) - l64), 4 * ULP32 * l64)
    assert abs(pd - p64) <= max(16 * abs(float(p32) - p64), 4 * ULP32 * p64)


# ---- 7. Adam alone -----------------------------------------------------------------------------------------------------------------
def test_train_apply_matches_adam_apply_elementwise():
    """Gradients, m, v, t, lr set to seeded values that include exact zeros, 1e-8 noise and entries near 1e-7; the result against
    adam_apply in fp32.  Elementwise, no sums: within 2 ulp of fp32 of the result.  How many values differ at all and the largest
    difference are printed.  With `__fsqrt_rn` (the bare hardware approximation) in the kernel, 18 of 22 005
    values differed, by up to 4 ulp of the result; the kernel now takes sqrtf, correctly rounded, and every operation is rounded
    as NumPy rounds it -- only lr_t, formed in double on both sides, can differ in its last bit."""
    from bayesianinferencedl_amd.engine import DeviceTrainer
    m = perturbed(100, 37, 2, 9)
    rng = np.random.default_rng(5)

    def seeded(a, scale):
        v = (scale * rng.standard_normal(a.shape)).astype(np.float32)
        kind = rng.integers(0, 4, a.shape)
        v[kind == 0] = 0.0
        v[kind == 1] = (1e-8 * rng.standard_normal(a.shape)).astype(np.float32)[kind == 1]
        v[kind == 2] = (1e-7 * (1 + 0.1 * rng.standard_normal(a.shape))).astype(np.float32)[kind == 2]
        return v
    from bayesianinferencedl_amd.deep_learning.dl_model import tree_map
    grads = tree_map(lambda a: seeded(a, 1e-2), m._tree())
    for u in grads["layers"]:                                              # the batch statistics of the step
        u["mean"] = rng.normal(0, 0.5, u["mean"].shape).astype(np.float32)
        u["var"] = rng.uniform(0.1, 2.0, u["var"].shape).astype(np.float32)
    m.opt["m"] = tree_map(lambda a: seeded(a, 1e-2), m._tree())
    m.opt["v"] = tree_map(lambda a: np.abs(seeded(a, 1e-4)), m._tree())
    for tree in (m.opt["m"], m.opt["v"]):
        for u in tree["layers"]:
            u["mean"][...] = 0; u["var"][...] = 0
    m.opt["t"] = 7
    host, start = copy.deepcopy(m), copy.deepcopy(m)
    host.adam_apply(grads, 8, 1e-3)
    tr = DeviceTrainer(m, max_batch=64)
    try:
        tr.set_lr(1e-3)
        tr.set_grads(grads, loss=0.5, mape=20.0, B=64)
        tr.apply()
        tr.pull()
        loss, mape, rows = tr.epoch_stats()
    finally:
        tr.close()
    assert m.opt["t"] == 8 and rows == 64 and loss == 0.5 and mape == 20.0
    worst, differing, total = 0.0, 0, 0
    names = [f"{k}.{nm}" for k in ("p", "m", "v") for nm, _, _ in leaves(m._tree())]
    trees = lambda mod: leaves(mod._tree()) + leaves(mod.opt["m"]) + leaves(mod.opt["v"])
    for name, (_, a, _), (_, b, _), (_, o, _) in zip(names, trees(m), trees(host), trees(start)):
        scale = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)      # an ulp of the result
        ulps = np.abs(a - b) / scale
        differing += int((a != b).sum()); total += a.size
        if ulps.max() > worst:
            i = np.unravel_index(np.argmax(ulps), ulps.shape)
            worst = float(ulps.max())
            print(f"  {name}{list(i)}: before {o[i]!r} host {b[i]!r} device {a[i]!r} ({worst} ulp)")
        assert ulps.max() <= 2, (name, ulps.max())
    print(f"Adam and moving statistics, device against adam_apply in fp32: {differing} of {total} values differ, largest {worst} ulp")


# ---- 8. bits ------------------------------------------------------------------------------------------------------------------------
def run(graph, S=150, B=64, epochs=3, shuffle=True, record_steps=False, seed=0):
    from bayesianinferencedl_amd.engine import DeviceTrainer
    X, Y = probe(60, S, 4)
    m = ResBnFcModel(60, 4, 2, 16, seed=1)
    tr = DeviceTrainer(m, max_batch=B)
    try:
        h = tr.fit(X, Y, epochs=epochs, batch_size=B, shuffle=shuffle, validation_data=(X[:40], Y[:40]), lr=1e-3, seed=seed, graph=graph,
                   record_steps=record_steps)
        used = tr.graph_used
    finally:
        tr.close()
    return m, h, used


def test_same_bits_run_to_run_and_graph_against_stream_order():
    """A run with a short last batch (64 + 64 + 22 rows): twice through the graph, once in stream order -- identical bits in every
    parameter, moving statistic, m, v and in the history."""
    a, ha, ga = run(True)
    b, hb, gb = run(True)
    c, hc, gc = run(False)
    assert ga and gb and not gc
    assert a.opt["t"] == b.opt["t"] == c.opt["t"] == 9
    for other, h in ((b, hb), (c, hc)):
        assert np.array_equal(ResBnFcModel.flatten(a._tree()).view(np.uint32), ResBnFcModel.flatten(other._tree()).view(np.uint32))
        for k in ("m", "v"):
            assert np.array_equal(ResBnFcModel.flatten(a.opt[k]).view(np.uint32), ResBnFcModel.flatten(other.opt[k]).view(np.uint32))
        assert ha.history == h.history
    assert not np.allclose(a.head["mean"], 0)
    assert len(ha.mse) == 3 and all(0 < e < l for e, l in zip(ha.mse, ha.history["loss"]))      # (the loss without the regulariser)


@pytest.mark.parametrize("shuffle", [False, True])
def test_every_step_sees_the_rows_fit_host_sees(shuffle):
    """rows as the identity and as a permutation: the per-step loss of the device run follows fit_host's in float64 (a step on
    other rows would differ in the second digit)."""
    m, h, _ = run(False, shuffle=shuffle, record_steps=True, seed=3)
    X, Y = probe(60, 150, 4)
    ref = ResBnFcModel(60, 4, 2, 16, seed=1)
    h64 = ref.fit_host(X, Y, epochs=3, batch_size=64, shuffle=shuffle, validation_data=(X[:40], Y[:40]), lr=1e-3, seed=3, dtype=np.float64)
    d, y = np.array(h.step_loss), np.array(h64.step_loss)
    assert len(d) == 9
    spread = np.abs(np.diff(y)).min() / np.abs(y).max()
    print("per-step loss, device against fit_host fp64:", np.abs(d - y).max() / np.abs(y).max(), "smallest step-to-step change", spread)
    assert spread > 1e-4                                   # (ten times the tolerance below: another row set would not pass)
    assert np.abs(d - y).max() <= 1e-5 * np.abs(y).max()
    # (inference form sees b0 and the units' b, which move on rounding noise by about 0.1 lr per step: fp32 runs agree on the
    #  validation figures to about 1e-4 here, not to the 1e-6 of the training form, where batch normalisation removes them)
    assert np.allclose(h.history["val_loss"], h64.history["val_loss"], rtol=1e-3)


# ---- 9. the curve on device-generated pairs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("resolution,r", [(14, 8), (40, 24)])               # lattice divisor m = 4 (n = 245), m = 12 (n = 1597)
def test_fit_follows_the_fp64_curve_on_generated_pairs(resolution, r, tmp_path):
    """25 epochs x 4 steps of fit(device=True) against fit_host(float64), same seed: per-epoch loss, val_loss and both MAPE
    within 16 x the deviation of fit_host in fp32 from that yardstick; the training loss falls on device and host alike."""
    from bayesianinferencedl_amd.deep_learning.generate_fin_dataset import gen_affine_avg_rom_dataset
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.fom.thermal_fin import get_space
    from bayesianinferencedl_amd.rom.basis import pod_basis
    V = get_space(resolution)
    phi = pod_basis(Fin(V), r, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1)
    z, err = gen_affine_avg_rom_dataset(2200, resolution=resolution, phi=phi, seed=11, out_dir=str(tmp_path / "none"))
    z, err = np.asarray(z), np.asarray(err)
    tr_, va_ = (z[:2000], err[:2000]), (z[2000:], err[2000:])
    kw = dict(epochs=25, batch_size=500, validation_data=va_, lr=3e-4, seed=2)
    hists = {}
    for name, run_ in (("f64", lambda m: m.fit_host(*tr_, dtype=np.float64, **kw)), ("f32", lambda m: m.fit_host(*tr_, **kw)),
                       ("dev", lambda m: m.fit(*tr_, device=True, graph=True, **kw))):
        hists[name] = run_(ResBnFcModel(V.dim(), 9, 5, 50, seed=0)).history
    for key in ("loss", "val_loss", "mean_absolute_percentage_error", "val_mean_absolute_percentage_error"):
        y = np.array(hists["f64"][key])
        d32 = np.abs(np.array(hists["f32"][key]) - y).max() / np.abs(y).max()
        dd = np.abs(np.array(hists["dev"][key]) - y).max() / np.abs(y).max()
        print(f"n = {V.dim()} {key}: device {dd:.3g}, fit_host fp32 {d32:.3g}, first / last {y[0]:.4g} / {y[-1]:.4g}")
        assert dd <= max(16 * d32, 4 * ULP32), (key, dd, d32)
    for name in ("f64", "dev"):
        assert hists[name]["loss"][-1] < hists[name]["loss"][0]


# ---- 10. through every layer --------------------------------------------------------------------------------------------------------
def test_a_fitted_model_serves_predict_the_misfit_gradient_and_hmc():
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.fom.thermal_fin import get_space
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    from bayesianinferencedl_amd.rom.basis import pod_basis
    V = get_space(14)
    n = V.dim()
    solver = Fin(V)
    phi = pod_basis(solver, 8, n_snapshots=200, low=0.1, high=10.0, params="nine", seed=1)
    X, Y = probe(n, 300)
    model = ResBnFcModel(n, 9, 5, 50, seed=0)
    h = model.fit(X, Y, epochs=3, batch_size=100, lr=3e-4, seed=0)
    assert len(h.history["loss"]) == 3 and model.opt["t"] == 9 and model.W0.dtype == np.float32
    rng = np.random.default_rng(3)
    K = np.exp(0.3 * rng.standard_normal((7, n)))
    e_dev, e_host = DeviceErrorModel(model).predict(K), model.predict(K).astype(np.float64)
    assert np.max(np.abs(e_dev - e_host)) <= 1e-5 * np.max(np.abs(e_host))
    rom = AffineROMFin(V, model, phi)
    rom.set_data(np.asarray(solver.qoi_operator(solver.forward(K[0])[0])))
    out = rom.grad_romml_batch(K)
    assert np.all(np.asarray(out["info"]) == 0) and np.all(np.isfinite(out["grad"]))
    res = hmc.run_chains_device(rom, K[:2], 31, seeds=[1, 2], eps=1e-2, n_leapfrog=3)      # 1 + 10 x 3 evaluations
    assert res.proposals == 10 and np.all(np.isfinite(res.K))


# ---- 11. argument checks that need a handle -----------------------------------------------------------------------------------------
def test_train_grad_refuses_bad_batches_by_name():
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.engine import DeviceTrainer
    L = _ffi.lib()
    m = ResBnFcModel(60, 4, 2, 16, seed=1)
    tr = DeviceTrainer(m, max_batch=64)
    try:
        X, Y = probe(60, 100, 4)
        Xd, Yd, rows = tr.to_device(X, 60), tr.to_device(Y, 4), cuda_rows(np.arange(100))
        before = ResBnFcModel.flatten(m._tree()).copy()
        assert L.finrom_mlp_train_grad(tr._h, Xd.data_ptr(), Yd.data_ptr(), rows.data_ptr(), 1, None) == -1
        assert b"B must be at least 2" in L.finrom_last_error()
        assert L.finrom_mlp_train_grad(tr._h, Xd.data_ptr(), Yd.data_ptr(), rows.data_ptr(), 65, None) == -1
        assert b"max_batch" in L.finrom_last_error()
        assert L.finrom_mlp_train_grad(tr._h, None, Yd.data_ptr(), rows.data_ptr(), 64, None) == -1 and b"null" in L.finrom_last_error()
        tr.pull()
        assert np.array_equal(before, ResBnFcModel.flatten(m._tree()))
        with pytest.raises(ValueError, match="max_batch"):
            tr.fit(X, Y, epochs=1, batch_size=100)
    finally:
        tr.close()
