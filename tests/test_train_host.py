"""CPU tests of the error model's training run, host statement (deep_learning/dl_model.py: train_gradients, adam_apply, fit_host).
Yardstick: torch autograd in fp64 on the CPU, the model written out below in torch ops -- independent of the NumPy statement.
Bounds: two fp64 statements of the same sums in another order, 1e-10 of each tensor's largest entry (for the biases whose
gradient is zero in exact arithmetic -- b0 and the units' b -- absolute against the step's largest gradient); fp32 against fp64,
a multiple of what torch's own fp32 run deviates on the same data, with a floor of 4 ulp of fp32 at the tensor's largest entry."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesianinferencedl_amd.deep_learning import dl_model as D
from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel

ULP32 = float(np.finfo(np.float32).eps)
SHAPES = [(245, 64, 50, 5, 9), (1597, 500, 50, 5, 9), (120, 33, 37, 2, 9)]       # n_in, B, n_w, L, n_out


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def t_params(model, dtype):
    mk = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype, requires_grad=True)
    return {"W0": mk(model.W0), "b0": mk(model.b0),
            "layers": [{k: mk(u[k]) for k in ("gamma", "beta", "W", "b")} for u in model.units + [model.head]]}


def t_forward(P, X, Y, stats=None):
    """Training form (stats None) or inference form (stats: [(mean, var)]) -> loss, mape, [(batch mean, batch var)]."""
    y = X @ P["W0"] + P["b0"]
    out_stats, n = [], len(P["layers"])
    reg = 1e-4 * P["W0"].abs().sum() + 1e-4 * (P["W0"] ** 2).sum()
    for i, u in enumerate(P["layers"]):
        if stats is None:
            mu = y.mean(0); var = ((y - mu) ** 2).mean(0)
        else:
            mu, var = stats[i]
        out_stats.append((mu.detach(), var.detach()))
        a = torch.nn.functional.elu((y - mu) / torch.sqrt(var + 1e-3) * u["gamma"] + u["beta"])
        d = a @ u["W"] + u["b"]
        if i == n - 1:
            y = d
        else:
            y = y + d
            reg = reg + 1e-4 * u["W"].abs().sum() + 1e-4 * (u["W"] ** 2).sum()
    loss = ((y - Y) ** 2).mean() + reg
    mape = 100 * ((Y - y).abs() / Y.abs().clamp_min(1e-7)).mean()
    return loss, mape, out_stats


def t_leaves(P):
    return [P["W0"], P["b0"]] + [u[k] for u in P["layers"] for k in ("gamma", "beta", "W", "b")]


def t_gradients(P, X, Y):
    for p in t_leaves(P):
        p.grad = None
    loss, mape, stats = t_forward(P, X, Y)
    loss.backward()
    return float(loss.detach()), float(mape.detach()), stats


def t_adam(P, st, t, lr, dtype):
    """Adam in Keras 1.x form written out; st: {"m", "v"} lists over t_leaves."""
    one = torch.tensor(1.0, dtype=dtype)
    b1, b2 = torch.tensor(0.9, dtype=dtype), torch.tensor(0.999, dtype=dtype)
    lr_t = torch.tensor(lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t), dtype=dtype)
    with torch.no_grad():
        for p, m, v in zip(t_leaves(P), st["m"], st["v"]):
            m.copy_(b1 * m + (one - b1) * p.grad)
            v.copy_(b2 * v + (one - b2) * p.grad * p.grad)
            p.copy_(p - lr_t * m / (torch.sqrt(v) + 1e-7))


def tree_pairs(model_tree, P, what=lambda p: p.grad):
    """[(name, NumPy array from the statement, array from the yardstick, zero-gradient bias?)]"""
    out = [("W0", model_tree["W0"], what(P["W0"]), False), ("b0", model_tree["b0"], what(P["b0"]), True)]
    n = len(P["layers"])
    for i, (u, tu) in enumerate(zip(model_tree["layers"], P["layers"])):
        for k in ("gamma", "beta", "W", "b"):
            out.append((f"l{i}_{k}", u[k], what(tu[k]), k == "b" and i < n - 1))
    return [(nm, np.asarray(a, dtype=np.float64), b.detach().numpy().astype(np.float64), z) for nm, a, b, z in out]


def deviations(pairs):
    """name -> max |a - b| relative to the yardstick tensor's largest entry (zero-gradient biases: to the largest of all)."""
    gmax = max(np.abs(b).max() for _, _, b, _ in pairs)
    return {nm: np.abs(a - b).max() / (gmax if z or np.abs(b).max() == 0 else np.abs(b).max()) for nm, a, b, z in pairs}


def probe(n_in, S, n_out=9, seed=0):
    """Seeded synthetic pairs: fields exp(0.3 xi), targets 0.05 tanh(20 log(x) T), T = randn(n_in, n_out) / n_in."""
    rng = np.random.default_rng(seed)
    X = np.exp(0.3 * rng.standard_normal((S, n_in)))
    T = rng.standard_normal((n_in, n_out)) / n_in
    return X, 0.05 * np.tanh(20 * np.log(X) @ T)


def perturbed(n_in, n_w, L, n_out, seed=1):
    """A model away from the Glorot start: non-trivial gamma, beta, biases."""
    m = ResBnFcModel(n_in, n_out, L, n_w, seed)
    rng = np.random.default_rng(seed + 100)
    for u in m.units + [m.head]:
        u["gamma"] = rng.uniform(0.5, 1.5, u["gamma"].shape).astype(np.float32)
        u["beta"] = rng.normal(0, 0.3, u["beta"].shape).astype(np.float32)
        u["b"] = rng.normal(0, 0.1, u["b"].shape).astype(np.float32)
    m.b0 = rng.normal(0, 0.1, m.b0.shape).astype(np.float32)
    return m


# ---- 1. gradients in fp64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_train_gradients_fp64_match_autograd(shape):
    n_in, B, n_w, L, n_out = shape
    m = perturbed(n_in, n_w, L, n_out)
    X, Y = probe(n_in, B, n_out)
    loss, mape, g = m.train_gradients(X, Y, np.float64)
    P = t_params(m, torch.float64)
    tl, tm, ts = t_gradients(P, torch.tensor(X), torch.tensor(Y))
    dev = deviations(tree_pairs(g, P))
    print("fp64 gradient deviations", shape, max(dev.values()))
    assert max(dev.values()) < 1e-10, dev
    assert abs(loss - tl) < 1e-10 * abs(tl) and abs(mape - tm) < 1e-10 * abs(tm)
    for u, (mu, var) in zip(g["layers"], ts):
        assert np.abs(u["mean"] - mu.numpy()).max() < 1e-10 * np.abs(mu.numpy()).max()
        assert np.abs(u["var"] - var.numpy()).max() < 1e-10 * np.abs(var.numpy()).max()


# ---- 2. twenty steps in fp64 -------------------------------------------------------------------------------------------------------
def test_twenty_steps_fp64_match_autograd_with_adam_written_out():
    n_in, B, n_w, L, n_out = 245, 64, 50, 5, 9
    X, Y = probe(n_in, 5 * B, n_out)
    m = ResBnFcModel(n_in, n_out, L, n_w, seed=2)
    P = t_params(m, torch.float64)
    st = {k: [torch.zeros_like(p) for p in t_leaves(P)] for k in ("m", "v")}
    mov = [(torch.zeros(n_w, dtype=torch.float64), torch.ones(n_w, dtype=torch.float64)) for _ in range(L + 1)]
    hist = m.fit_host(X, Y, epochs=4, batch_size=B, shuffle=True, lr=3e-4, seed=5, dtype=np.float64)
    plan = D.EpochPlan(5 * B, B, True, 5)
    t, tl = 0, []
    for _ in range(4):
        for r in plan.batches(plan.next_rows()):
            loss, _, stats = t_gradients(P, torch.tensor(X[r]), torch.tensor(Y[r]))
            t += 1
            t_adam(P, st, t, 3e-4, torch.float64)
            mov = [(0.99 * a + 0.01 * mu, 0.99 * b + 0.01 * var) for (a, b), (mu, var) in zip(mov, stats)]
            tl.append(loss)
    assert t == 20 == m.opt["t"] and len(hist.step_loss) == 20
    assert np.abs(np.array(hist.step_loss) - np.array(tl)).max() < 1e-10 * max(tl)
    for what, tree in ((lambda p: p, m._tree()), (lambda p: st["m"][[id(q) for q in t_leaves(P)].index(id(p))], m.opt["m"]),
                       (lambda p: st["v"][[id(q) for q in t_leaves(P)].index(id(p))], m.opt["v"])):
        dev = deviations(tree_pairs(tree, P, what))        # (b0 and the units' b, their m and v: noise, held against the largest tensor)
        assert max(dev.values()) < 1e-10, dev
    for u, (a, b) in zip(m.units + [m.head], mov):
        assert np.abs(u["mean"] - a.numpy()).max() < 1e-10 * np.abs(a.numpy()).max()
        assert np.abs(u["var"] - b.numpy()).max() < 1e-10 * np.abs(b.numpy()).max()


# ---- 3. gradients in fp32 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_train_gradients_fp32_deviate_no_more_than_torch_fp32(shape):
    """Recorded, largest deviation over the tensors, relative to each tensor's largest entry (NumPy fp32 / torch fp32, x86 CPU):
    (245, 64) 2.0e-6 / 1.9e-6; (1597, 500) 2.1e-6 / 2.4e-6; (120, 33, n_w 37) 1.2e-6 / 1.2e-6.  (With NumPy's own axis-0 sums,
    sequential fp32 chains, b0 alone stood at 8.5e-7 of the step's largest gradient against torch's 4.2e-8: the batch's column
    sums are now carried in double, dl_model._colsum.)"""
    n_in, B, n_w, L, n_out = shape
    m = ResBnFcModel(n_in, n_out, L, n_w, seed=3)                          # the Glorot start
    X, Y = probe(n_in, B, n_out)
    P64, P32 = t_params(m, torch.float64), t_params(m, torch.float32)
    t_gradients(P64, torch.tensor(X), torch.tensor(Y))
    t_gradients(P32, torch.tensor(X, dtype=torch.float32), torch.tensor(Y, dtype=torch.float32))
    g64 = {"W0": P64["W0"].grad.numpy(), "b0": P64["b0"].grad.numpy(),
           "layers": [{k: u[k].grad.numpy() for k in u} for u in P64["layers"]]}
    dev_torch = deviations(tree_pairs(g64, P32))                            # torch fp32 against the yardstick
    _, _, g = m.train_gradients(X, Y, np.float32)
    assert g["W0"].dtype == np.float32
    dev = deviations(tree_pairs(g, P64))
    print("fp32 gradient deviations", shape, "numpy", max(dev.values()), "torch", max(dev_torch.values()))
    for nm in dev:
        assert dev[nm] <= max(4 * dev_torch[nm], 4 * ULP32), (nm, dev[nm], dev_torch[nm])


# ---- 4. semantics ------------------------------------------------------------------------------------------------------------------
def small_run(seed=0, epochs=3, S=150, B=64, **kw):
    X, Y = probe(60, S, 4)
    m = ResBnFcModel(60, 4, 2, 16, seed=1)
    return m, m.fit_host(X, Y, epochs=epochs, batch_size=B, seed=seed, **kw), (X, Y)


def test_short_last_batch_and_one_row_remainder():
    m, h, _ = small_run(S=150, B=64)                                        # 64 + 64 + 22
    assert m.opt["t"] == 9 and len(h.step_loss) == 9
    with pytest.raises(ValueError, match="one row"):
        small_run(S=129, B=64)
    with pytest.raises(ValueError, match="at least 2"):
        small_run(S=10, B=1)


def test_seeds_history_keys_and_lr_callable():
    _, h0, _ = small_run(seed=0)
    _, h1, _ = small_run(seed=0)
    _, h2, _ = small_run(seed=1)
    assert h0.history == h1.history and h0.history["loss"] != h2.history["loss"]
    assert set(h0.history) == {"loss", "mean_absolute_percentage_error"}
    seen = []
    X, Y = probe(60, 150, 4)
    _, hv, _ = small_run(lr=lambda e: seen.append(e) or 1e-3, validation_data=(X[:40], Y[:40]))
    assert seen == [0, 1, 2]
    assert set(hv.history) == {"loss", "mean_absolute_percentage_error", "val_loss", "val_mean_absolute_percentage_error"}
    assert all(len(v) == 3 for v in hv.history.values())
    assert D.lr_schedule(0) == 3e-4 and D.lr_schedule(1000) == 3e-4 and D.lr_schedule(1001) == 1e-5 and D.lr_schedule(7500) == 5e-6 \
        and D.lr_schedule(7501) == 1e-7 and D.lr_schedule_pre(500) == 3e-4 and D.lr_schedule_pre(501) == 3e-5 \
        and D.lr_schedule_pre(1501) == 1e-6 and D.lr_schedule_pre(2001) == 5e-7


def test_validation_uses_the_moving_statistics():
    X, Y = probe(60, 150, 4)
    m, h, _ = small_run(validation_data=(X[:40], Y[:40]), dtype=np.float64)
    P = t_params(m, torch.float64)
    stats = [(torch.tensor(u["mean"]), torch.tensor(u["var"])) for u in m.units + [m.head]]
    with torch.no_grad():
        loss, mape, _ = t_forward(P, torch.tensor(X[:40]), torch.tensor(Y[:40]), stats)
    assert abs(h.history["val_loss"][-1] - float(loss)) < 1e-10 * float(loss)
    assert abs(h.history["val_mean_absolute_percentage_error"][-1] - float(mape)) < 1e-10 * float(mape)
    assert not np.allclose(m.head["mean"], 0) and not np.allclose(m.head["var"], 1)


def test_save_load_continue_gives_the_bits_of_an_uninterrupted_run(tmp_path):
    m_full, _, (X, Y) = small_run(epochs=4)
    m_a, _, _ = small_run(epochs=2)
    m_a.save(tmp_path / "mid.npz")
    m_b = ResBnFcModel.load(tmp_path / "mid.npz")
    assert m_b.opt["t"] == 6 and m_b.opt["epoch"] == 2
    m_b.fit_host(X, Y, epochs=2, batch_size=64, seed=0)
    for a, b in zip(ResBnFcModel.flatten(m_full._tree()), ResBnFcModel.flatten(m_b._tree())):
        assert a == b
    assert np.array_equal(ResBnFcModel.flatten(m_full.opt["v"]), ResBnFcModel.flatten(m_b.opt["v"]))


def test_a_file_from_the_old_save_loads(tmp_path):
    m = ResBnFcModel(30, 9, 2, 16, seed=4)
    arrs = {"meta": np.array([m.n_in, m.n_out, m.n_layers, m.n_weights]), "W0": m.W0, "b0": m.b0}      # the old save, verbatim
    for i, u in enumerate(m.units + [m.head]):
        for k, v in u.items():
            arrs[f"l{i}_{k}"] = v
    np.savez(tmp_path / "old.npz", **arrs)
    m2 = ResBnFcModel.load(tmp_path / "old.npz")
    x = np.random.default_rng(0).normal(size=(3, 30))
    assert np.array_equal(m.predict(x), m2.predict(x)) and m2.opt["t"] == 0 and m2.opt["m"] is None


# ---- 5. the loss goes down, and fp32 follows fp64 ----------------------------------------------------------------------------------
def test_fit_host_lowers_the_loss_and_fp32_follows_the_fp64_curve():
    """25 epochs x 4 steps at (1597, 500).  Recorded (x86 CPU): per-step loss over the 100 steps against the fp64 yardstick,
    fit_host fp32 1.7e-6, torch fp32 1.7e-6 (both land on the same fp32 value at the worst step); MSE 0.907 -> 0.0397 (ratio
    0.044); loss with the regulariser 1.335 -> 0.449.  fit_host in float64 follows the yardstick within 1e-10."""
    n_in, S, B = 1597, 2000, 500
    X, Y = probe(n_in, S)
    curves = {}
    for dtype in (torch.float64, torch.float32):
        m0 = ResBnFcModel(n_in, 9, 5, 50, seed=0)
        P = t_params(m0, dtype)
        st = {k: [torch.zeros_like(p) for p in t_leaves(P)] for k in ("m", "v")}
        Xt, Yt = torch.tensor(X, dtype=dtype), torch.tensor(Y, dtype=dtype)
        plan, t, ls = D.EpochPlan(S, B, True, 0), 0, []
        for _ in range(25):
            for r in plan.batches(plan.next_rows()):
                ls.append(t_gradients(P, Xt[r], Yt[r])[0])
                t += 1
                t_adam(P, st, t, 3e-4, dtype)
        curves[dtype] = np.array(ls)
    y64 = curves[torch.float64]
    dev_torch = np.abs(curves[torch.float32] - y64).max() / np.abs(y64).max()
    m = ResBnFcModel(n_in, 9, 5, 50, seed=0)
    h = m.fit_host(X, Y, epochs=25, batch_size=B, lr=3e-4, seed=0)
    assert m.W0.dtype == np.float32
    dev = np.abs(np.array(h.step_loss) - y64).max() / np.abs(y64).max()
    print("per-step loss over 100 steps: fit_host fp32 vs yardstick", dev, "torch fp32 vs yardstick", dev_torch,
          "first / last epoch loss", h.history["loss"][0], h.history["loss"][-1], "MSE", h.mse[0], h.mse[-1])
    assert dev <= max(16 * dev_torch, 4 * ULP32)
    assert h.history["loss"][-1] < h.history["loss"][0]
    assert h.mse[-1] < 0.1 * h.mse[0]                      # (the loss without the regulariser, which is 0.45 of it and hardly moves)
    m64 = ResBnFcModel(n_in, 9, 5, 50, seed=0)
    h64 = m64.fit_host(X, Y, epochs=25, batch_size=B, lr=3e-4, seed=0, dtype=np.float64)
    assert np.abs(np.array(h64.step_loss) - y64).max() < 1e-10 * np.abs(y64).max()


# ---- 11. argument checks of the device trainer: host side, before any device call ---------------------------------------------------
def test_trainer_entry_points_check_their_arguments_before_any_device_call():
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    h = C.c_void_p()
    d = _ffi.MlpTrainDesc(n_in=100, n_w=65, n_layers=2, n_out=9, max_batch=64)
    assert L.finrom_mlp_train_create(C.byref(d), C.byref(h)) == -4 and b"n_w" in L.finrom_last_error() and not h.value
    d = _ffi.MlpTrainDesc(n_in=100, n_w=50, n_layers=9, n_out=9, max_batch=64)
    assert L.finrom_mlp_train_create(C.byref(d), C.byref(h)) == -4 and b"n_layers" in L.finrom_last_error()
    d = _ffi.MlpTrainDesc(n_in=100, n_w=50, n_layers=2, n_out=9, max_batch=1)
    assert L.finrom_mlp_train_create(C.byref(d), C.byref(h)) == -1 and b"max_batch" in L.finrom_last_error()
    assert L.finrom_mlp_train_create(None, C.byref(h)) == -1
    assert L.finrom_mlp_train_grad(None, None, None, None, 64, None) == -1 and b"null handle" in L.finrom_last_error()
    assert L.finrom_mlp_train_apply(None, None) == -1 and b"null handle" in L.finrom_last_error()
    assert L.finrom_mlp_train_set_params(None, None, None, None, 0) == -1
    assert L.finrom_mlp_train_eval(None, None, None, 1, None, None) == -1
    assert L.finrom_mlp_train_set_lr(None, 1e-3, None) == -1
    assert L.finrom_mlp_train_param_count(None) == 0
