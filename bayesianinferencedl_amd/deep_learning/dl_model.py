"""The reference's error model (deep_learning/dl_model.py:149-176 `res_bn_fc_model`): a residual, batch-normalised, fully
connected network  R^n -> R^n_obs  evaluated in fp32 like the Keras original, with the two operations the inverse-problem
callers need -- `predict` (rom/averaged_affine_ROM.py:360) and the vector-Jacobian product behind
`tf.gradients(loss, model.input)` (:226-228) -- and the training run of :230-243: `fit` (HIP kernels, engine.DeviceTrainer) and
its host statement `fit_host` (NumPy; in float64 the yardstick of the device tests).  Host NumPy for inference: at one sample
per call (the HMC / MAP call pattern) the network is two skinny GEMVs.

Training restates what Keras 1.x does in the reference's run (TensorFlow is not a dependency): batch normalisation in training
form (batch mean, biased batch variance, eps 1e-3; moving <- 0.99 moving + 0.01 batch), loss = mean squared error + l1_l2(1e-4,
1e-4) on W0 and the units' W (:154-167; not the head), Adam with  lr_t = lr sqrt(1 - 0.999^t) / (1 - 0.9^t),
p <- p - lr_t m / (sqrt(v) + 1e-7),  lr constant within an epoch (LearningRateScheduler, :238).  Divergence: the row permutation
of each epoch comes from np.random.default_rng(seed) (Keras is unseeded).  b0 and the units' b have a gradient that is zero in
exact arithmetic (the next batch normalisation removes a constant); they stay trainable as in Keras and move on rounding noise.

Architecture as the reference builds it (the first BN-activation-Dense triple of `residual_unit` is overwritten before it
is used, :150-158, so a unit is  x + Dense(act(BN(x)))):
    y0 = Dense(n_in -> n_w)(x);  y_{i+1} = y_i + Dense(n_w -> n_w)(ELU(BN(y_i))), i < n_layers;
    out = Dense(n_w -> n_out)(ELU(BN(y_L)))
Weights live in an .npz (`save` / `load`); Keras checkpoints cannot be read here (no h5py / tensorflow)."""
from __future__ import annotations

import numpy as np

BN_EPS = 1e-3                     # Keras BatchNormalization default


def _elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def _colsum(a):
    """Sum over the batch rows, accumulated in double and rounded once.  (NumPy's axis-0 sum of a row-major array is a sequential
    chain in the array's precision: in fp32 its rounding alone put 8e-7 of the step's largest gradient on b0, whose gradient is
    zero in exact arithmetic -- twenty times what torch's fp32 sum leaves.  The device kernels carry these sums in double too.)"""
    return a.sum(axis=0, dtype=np.float64).astype(a.dtype)


def _elu_grad(x):
    return np.where(x > 0, 1.0, np.exp(np.minimum(x, 0))).astype(x.dtype)


class ResBnFcModel:
    def __init__(self, n_in, n_out=9, n_layers=5, n_weights=50, seed=0):
        rng = np.random.default_rng(seed)
        self.n_in, self.n_out, self.n_layers, self.n_weights = n_in, n_out, n_layers, n_weights

        def glorot(a, b):
            lim = np.sqrt(6.0 / (a + b))
            return rng.uniform(-lim, lim, (a, b)).astype(np.float32)
        self.W0, self.b0 = glorot(n_in, n_weights), np.zeros(n_weights, np.float32)
        self.units = [{"gamma": np.ones(n_weights, np.float32), "beta": np.zeros(n_weights, np.float32),
                       "mean": np.zeros(n_weights, np.float32), "var": np.ones(n_weights, np.float32),
                       "W": glorot(n_weights, n_weights), "b": np.zeros(n_weights, np.float32)} for _ in range(n_layers)]
        self.head = {"gamma": np.ones(n_weights, np.float32), "beta": np.zeros(n_weights, np.float32),
                     "mean": np.zeros(n_weights, np.float32), "var": np.ones(n_weights, np.float32),
                     "W": glorot(n_weights, n_out), "b": np.zeros(n_out, np.float32)}
        # optimiser state: Adam's step count, epochs done, m and v (trees, None before the first step)
        self.opt = {"t": 0, "epoch": 0, "m": None, "v": None}

    # -- the two operations used by AffineROMFin.grad_romml --------------------------------------------------------
    def _as_batch(self, x):
        return np.asarray(x, dtype=np.float32).reshape(-1, self.n_in)

    @staticmethod
    def _bn(u, y):
        s = u["gamma"] / np.sqrt(u["var"] + BN_EPS)
        return y * s + (u["beta"] - u["mean"] * s), s

    def _forward(self, X):
        y = X @ self.W0 + self.b0
        tape = []
        for u in self.units + [self.head]:
            z, s = self._bn(u, y)
            tape.append((z, s))
            d = _elu(z) @ u["W"] + u["b"]
            y = d if u is self.head else y + d
        return y, tape

    def predict(self, x):
        """x [S, n_in] (or Keras-style nested lists) -> [S, n_out] float32."""
        return self._forward(self._as_batch(x))[0]

    def vjp(self, x, upstream):
        """upstream [S, n_out] = dLoss/d(output) -> dLoss/d(input) [S, n_in] (what tf.gradients(loss, input) returns)."""
        X = self._as_batch(x)
        _, tape = self._forward(X)
        g = np.asarray(upstream, dtype=np.float32).reshape(-1, self.n_out)
        layers = self.units + [self.head]
        z, s = tape[-1]
        g = (g @ self.head["W"].T) * _elu_grad(z) * s                       # through the head: no skip connection
        for u, (z, s) in zip(reversed(layers[:-1]), reversed(tape[:-1])):
            g = g + (g @ u["W"].T) * _elu_grad(z) * s                       # skip + branch
        return g @ self.W0.T

    # -- training: the host statement (NumPy) ------------------------------------------------------------------------------------
    # Trees of arrays: {"W0", "b0", "layers": [{"gamma", "beta", "mean", "var", "W", "b"} per unit, then the head]}.  For the
    # gradients "mean" / "var" hold the batch statistics of the step; for Adam's m and v they are unused zeros.
    def _tree(self):
        return {"W0": self.W0, "b0": self.b0, "layers": self.units + [self.head]}

    def _cast(self, dtype):
        self.W0, self.b0 = np.asarray(self.W0, dtype), np.asarray(self.b0, dtype)
        for u in self.units + [self.head]:
            for k in u:
                u[k] = np.asarray(u[k], dtype)
        for name in ("m", "v"):
            if self.opt.get(name) is not None:
                self.opt[name] = tree_map(lambda a: np.asarray(a, dtype), self.opt[name])

    def train_gradients(self, Xb, Yb, dtype=None):
        """One batch in training form -> (loss, MAPE, gradient tree).  loss = MSE + regulariser; the tree's "mean" / "var" are the
        batch statistics.  Arithmetic in `dtype` (default: the dtype of the model's arrays)."""
        dt = np.dtype(dtype or self.W0.dtype).type
        X = np.asarray(Xb, dtype=dt).reshape(-1, self.n_in)
        Y = np.asarray(Yb, dtype=dt).reshape(-1, self.n_out)
        B = X.shape[0]
        if B < 2 or Y.shape[0] != B:
            raise ValueError("train_gradients: a batch needs at least two rows (batch statistics) and as many targets as inputs")
        c = lambda a: np.asarray(a, dtype=dt)
        W0, layers = c(self.W0), [{k: c(v) for k, v in u.items()} for u in self.units + [self.head]]
        eps = dt(BN_EPS)
        y = X @ W0 + c(self.b0)
        tape = []
        for i, u in enumerate(layers):
            mu = _colsum(y) / dt(B)
            d = y - mu
            var = _colsum(d * d) / dt(B)
            rstd = dt(1) / np.sqrt(var + eps)
            xh = d * rstd
            z = xh * u["gamma"] + u["beta"]
            a = _elu(z)
            tape.append((xh, rstd, z, a, mu, var))
            dd = a @ u["W"] + u["b"]
            y = dd if i == len(layers) - 1 else y + dd
        diff = y - Y
        reg = dt(0)
        for W in [W0] + [u["W"] for u in layers[:-1]]:
            reg = reg + dt(REG_L1) * np.abs(W).sum() + dt(REG_L2) * (W * W).sum()
        mse = (diff * diff).mean()
        loss = mse + reg
        mape = dt(100) * (np.abs(diff) / np.maximum(np.abs(Y), dt(1e-7))).mean()
        g = diff * dt(2.0 / (B * self.n_out))                              # d loss / d out
        reg_grad = lambda W: dt(REG_L1) * np.sign(W) + dt(2 * REG_L2) * W
        glayers = [None] * len(layers)
        for i in range(len(layers) - 1, -1, -1):
            u = layers[i]
            xh, rstd, z, a, mu, var = tape[i]
            head = i == len(layers) - 1
            gW = a.T @ g
            if not head:
                gW = gW + reg_grad(u["W"])
            gz = (g @ u["W"].T) * _elu_grad(z)
            gbeta, ggamma = _colsum(gz), _colsum(gz * xh)
            gy = (u["gamma"] * rstd) * (gz - gbeta / dt(B) - xh * (ggamma / dt(B)))
            glayers[i] = {"gamma": ggamma, "beta": gbeta, "mean": mu, "var": var, "W": gW, "b": _colsum(g)}
            g = gy if head else g + gy
        grads = {"W0": X.T @ g + reg_grad(W0), "b0": _colsum(g), "layers": glayers, "mse": float(mse)}
        return loss, mape, grads

    def adam_apply(self, grads, t, lr, moving=True):
        """Adam in Keras 1.x form on every trainable array, in the dtype of the model's arrays; t >= 1 is the step count of the
        whole run.  moving: also  moving <- 0.99 moving + 0.01 batch  with the batch statistics carried by `grads`."""
        dt = self.W0.dtype.type
        o = self.opt
        if o["m"] is None:
            o["m"], o["v"] = (tree_map(np.zeros_like, self._tree()) for _ in range(2))
        lr_t = dt(float(lr) * np.sqrt(1.0 - ADAM_B2 ** int(t)) / (1.0 - ADAM_B1 ** int(t)))      # (formed in double, used in dt)
        b1, b2, eps = dt(ADAM_B1), dt(ADAM_B2), dt(ADAM_EPS)
        c1, c2 = dt(1) - b1, dt(1) - b2                       # (as Keras: 1 - beta in the arrays' precision)

        def step(p, g, m, v):
            g = np.asarray(g, dtype=dt)
            m[...] = b1 * m + c1 * g
            v[...] = b2 * v + c2 * (g * g)
            p[...] = p - (lr_t * m) / (np.sqrt(v) + eps)
        P, M, V = self._tree(), o["m"], o["v"]
        step(P["W0"], grads["W0"], M["W0"], V["W0"]); step(P["b0"], grads["b0"], M["b0"], V["b0"])
        for u, g, m, v in zip(P["layers"], grads["layers"], M["layers"], V["layers"]):
            for k in ("gamma", "beta", "W", "b"):
                step(u[k], g[k], m[k], v[k])
            if moving:
                for k in ("mean", "var"):
                    u[k][...] = dt(BN_MOMENTUM) * u[k] + dt(1.0 - BN_MOMENTUM) * np.asarray(g[k], dtype=dt)
        o["t"] = int(t)

    def evaluate(self, X, Y, dtype=None):
        """Inference form (moving statistics) -> (loss with the regulariser, MAPE), in `dtype`."""
        dt = np.dtype(dtype or self.W0.dtype).type
        c = lambda a: np.asarray(a, dtype=dt)
        X, Y = c(X).reshape(-1, self.n_in), c(Y).reshape(-1, self.n_out)
        y = X @ c(self.W0) + c(self.b0)
        layers = self.units + [self.head]
        reg = dt(REG_L1) * np.abs(c(self.W0)).sum() + dt(REG_L2) * (c(self.W0) * c(self.W0)).sum()
        for i, u in enumerate(layers):
            s = c(u["gamma"]) / np.sqrt(c(u["var"]) + dt(BN_EPS))
            z = y * s + (c(u["beta"]) - c(u["mean"]) * s)
            dd = _elu(z) @ c(u["W"]) + c(u["b"])
            if i == len(layers) - 1:
                y = dd
            else:
                y = y + dd
                reg = reg + dt(REG_L1) * np.abs(c(u["W"])).sum() + dt(REG_L2) * (c(u["W"]) * c(u["W"])).sum()
        diff = y - Y
        return (diff * diff).mean() + reg, dt(100) * (np.abs(diff) / np.maximum(np.abs(Y), dt(1e-7))).mean()

    def fit_host(self, z, errors, *, epochs, batch_size=500, shuffle=True, validation_data=None, lr=3e-4, seed=0, dtype=np.float32):
        """The reference's training run (dl_model.py:239-241) on the host in `dtype`; see the module docstring for the algorithm.
        The model's arrays are cast to `dtype` and hold the trained weights afterwards, in that dtype (a float64 run leaves float64
        arrays: predict and save then work in double; DeviceErrorModel casts to fp32).  dtype=float32 means fp32 products and
        elementwise arithmetic with the batch's column sums carried in double (_colsum).  Epochs are counted on from
        self.opt["epoch"] (the permutations of the epochs already done are drawn and dropped), so that save -> load -> fit
        continues a run bit for bit.  -> History."""
        dt = np.dtype(dtype).type
        X, Y = np.asarray(z, dtype=dt).reshape(-1, self.n_in), np.asarray(errors, dtype=dt).reshape(-1, self.n_out)
        plan = EpochPlan(X.shape[0], batch_size, shuffle, seed, self.opt["epoch"])
        val = None if validation_data is None else tuple(np.asarray(a, dtype=dt) for a in validation_data)
        self._cast(dt)
        hist = History(val is not None)
        for _ in range(int(epochs)):
            e = self.opt["epoch"]
            lr_e = float(lr(e)) if callable(lr) else float(lr)
            rows = plan.next_rows()
            sl, sm, se = 0.0, 0.0, 0.0
            for r in plan.batches(rows):
                loss, mape, grads = self.train_gradients(X[r], Y[r], dt)
                self.adam_apply(grads, self.opt["t"] + 1, lr_e)
                hist.step_loss.append(float(loss))
                sl += float(loss) * len(r); sm += float(mape) * len(r); se += grads["mse"] * len(r)
            hist.mse.append(se / plan.S)
            self.opt["epoch"] = e + 1
            hist.add(sl / plan.S, sm / plan.S, self.evaluate(*val, dtype=dt) if val is not None else None)
        return hist

    def fit(self, z, errors, *, epochs, batch_size=500, shuffle=True, validation_data=None, lr=3e-4, seed=0, device=True, graph=True):
        """The training run on the device in fp32 (engine.DeviceTrainer: HIP kernels, an epoch captured in one HIP graph and
        replayed); device=False is fit_host.  Same permutations, same history object; afterwards the model's arrays hold the
        trained weights, moving statistics and optimiser state."""
        if not device:
            return self.fit_host(z, errors, epochs=epochs, batch_size=batch_size, shuffle=shuffle, validation_data=validation_data,
                                 lr=lr, seed=seed)
        from ..engine import DeviceTrainer
        tr = DeviceTrainer(self, max_batch=max(2, min(int(batch_size), np.asarray(z).reshape(-1, self.n_in).shape[0])))
        try:
            return tr.fit(z, errors, epochs=epochs, batch_size=batch_size, shuffle=shuffle, validation_data=validation_data, lr=lr,
                          seed=seed, graph=graph)
        finally:
            tr.close()

    # -- flat fp32 layout of the C ABI (finrom_mlp_train_set_params): W0, b0, then per layer gamma, beta, mean, var, W, b ---------
    @staticmethod
    def flatten(tree, dtype=np.float32):
        parts = [tree["W0"], tree["b0"]] + [u[k] for u in tree["layers"] for k in TREE_KEYS]
        return np.concatenate([np.asarray(a, dtype=dtype).ravel() for a in parts])

    def unflatten(self, flat):
        """-> a tree of fresh arrays shaped like the model's, filled from `flat`."""
        out, pos = tree_map(np.zeros_like, self._tree()), 0
        arrs = [out["W0"], out["b0"]] + [u[k] for u in out["layers"] for k in TREE_KEYS]
        for a in arrs:
            a[...] = np.asarray(flat[pos:pos + a.size]).reshape(a.shape)
            pos += a.size
        assert pos == len(flat)
        return out

    def set_tree(self, tree):
        self.W0, self.b0 = tree["W0"], tree["b0"]
        for u, t in zip(self.units + [self.head], tree["layers"]):
            u.update({k: t[k] for k in TREE_KEYS})

    # -- persistence -------------------------------------------------------------------------------------------------
    def save(self, path):
        arrs = {"meta": np.array([self.n_in, self.n_out, self.n_layers, self.n_weights]), "W0": self.W0, "b0": self.b0}
        for i, u in enumerate(self.units + [self.head]):
            for k, v in u.items():
                arrs[f"l{i}_{k}"] = v
        o = self.opt
        arrs["opt_t"] = np.array([o["t"], o["epoch"]], dtype=np.int64)
        if o["m"] is not None:                                 # (Adam's state: a run can be continued)
            arrs["opt_m"], arrs["opt_v"] = self.flatten(o["m"], self.W0.dtype), self.flatten(o["v"], self.W0.dtype)
        np.savez(path, **arrs)

    @classmethod
    def load(cls, path):
        d = np.load(path)
        n_in, n_out, n_layers, n_weights = (int(v) for v in d["meta"])
        m = cls(n_in, n_out, n_layers, n_weights)
        m.W0, m.b0 = d["W0"], d["b0"]
        for i, u in enumerate(m.units + [m.head]):
            for k in u:
                u[k] = d[f"l{i}_{k}"]
        if "opt_t" in d.files:                                 # (files written before training existed have no optimiser state)
            m.opt["t"], m.opt["epoch"] = (int(v) for v in d["opt_t"])
            if "opt_m" in d.files:
                m.opt["m"], m.opt["v"] = m.unflatten(d["opt_m"]), m.unflatten(d["opt_v"])
        return m


TREE_KEYS = ("gamma", "beta", "mean", "var", "W", "b")
REG_L1 = REG_L2 = 1e-4            # kernel_regularizer=l1_l2(1e-4, 1e-4), reference dl_model.py:154-167
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-7      # Keras defaults (epsilon = K.epsilon())
BN_MOMENTUM = 0.99                # Keras BatchNormalization default


def tree_map(f, tree):
    return {"W0": f(tree["W0"]), "b0": f(tree["b0"]), "layers": [{k: f(v) for k, v in u.items()} for u in tree["layers"]]}


class EpochPlan:
    """Which rows each step of each epoch sees: with shuffle a fresh permutation per epoch from np.random.default_rng(seed), drawn
    in epoch order (skip: epochs already done, whose permutations are drawn and dropped); batches of batch_size rows, the last one
    the S mod batch_size remaining rows.  A remainder of one row has no batch statistics and is refused."""

    def __init__(self, S, batch_size, shuffle, seed, skip=0):
        self.S, self.B = int(S), min(int(batch_size), int(S))
        if self.B < 2:
            raise ValueError("fit: batch_size and the number of rows must be at least 2 (batch statistics)")
        if self.S % self.B == 1:
            raise ValueError(f"fit: {self.S} rows in batches of {self.B} leave a last batch of one row, which has no batch "
                             "statistics; change batch_size or drop a row")
        self.shuffle, self.rng = bool(shuffle), np.random.default_rng(seed)
        for _ in range(int(skip) if self.shuffle else 0):
            self.rng.permutation(self.S)

    def next_rows(self):
        return self.rng.permutation(self.S) if self.shuffle else np.arange(self.S)

    def batches(self, rows):
        return [rows[i:i + self.B] for i in range(0, self.S, self.B)]


class History:
    """What Keras's fit returns, as far as the reference reads it (dl_model.py:84, :245-246): .history, a dict of per-epoch lists
    under Keras 1.13's names.  step_loss: the training loss of every step (before its update); mse: the epoch's loss without the regulariser."""

    def __init__(self, with_val=False):
        self.history = {"loss": [], "mean_absolute_percentage_error": []}
        if with_val:
            self.history.update({"val_loss": [], "val_mean_absolute_percentage_error": []})
        self.step_loss, self.mse = [], []

    def add(self, loss, mape, val=None):
        self.history["loss"].append(float(loss)); self.history["mean_absolute_percentage_error"].append(float(mape))
        if val is not None:
            self.history["val_loss"].append(float(val[0])); self.history["val_mean_absolute_percentage_error"].append(float(val[1]))


def lr_schedule(epoch):
    """The training run's learning rate by epoch (reference dl_model.py:178-188)."""
    for last, lr in ((1000, 3e-4), (3000, 1e-5), (7500, 5e-6)):
        if epoch <= last:
            return lr
    return 1e-7


def lr_schedule_pre(epoch):
    """The pre-training schedule (reference dl_model.py:190-200)."""
    for last, lr in ((500, 3e-4), (1000, 3e-5), (1500, 3e-6), (2000, 1e-6)):
        if epoch <= last:
            return lr
    return 5e-7


def load_dataset_avg_rom(load_prev=True, tr_size=6000, v_size=500, genrand=False, data_dir='../data', **gen_kwargs):
    """Reader contract of the reference's training scripts (deep_learning/dl_model.py:19-36): conductivity fields and
    QoI errors for training and validation, loaded from `<data_dir>/z_aff_avg_{tr,eval}.npy` /
    `errors_aff_avg_{tr,eval}.npy` when present (and load_prev), otherwise generated on the device by
    gen_affine_avg_rom_dataset (which writes the `*_avg_obs_3` files of its own, :102-110).
    -> (z_train, errors_train, z_val, errors_val)."""
    import os
    from .generate_fin_dataset import gen_affine_avg_rom_dataset
    out = []
    for tag, size in (("tr", tr_size), ("eval", v_size)):
        zf, ef = os.path.join(data_dir, f"z_aff_avg_{tag}.npy"), os.path.join(data_dir, f"errors_aff_avg_{tag}.npy")
        if load_prev and os.path.isfile(zf) and os.path.isfile(ef):
            out += [np.load(zf), np.load(ef)]
        else:
            out += list(gen_affine_avg_rom_dataset(size, genrand=genrand, out_dir=data_dir, **gen_kwargs))
    return tuple(out)


def res_bn_fc_model(n_layers, n_weights, input_shape=1446, output_shape=9, seed=0):
    """Constructor with the reference's argument meaning (activation and optimiser dropped: ELU and Adam are what the reference
    uses everywhere; the learning rate is an argument of fit)."""
    return ResBnFcModel(input_shape, output_shape, n_layers, n_weights, seed)


def train_error_model(out_path=None, *, n_layers=5, n_weights=50, epochs=5000, batch_size=500, lr=lr_schedule, seed=0, data=None,
                      tr_size=6000, v_size=500, data_dir='../data', load_prev=True, device=True, graph=True, **gen_kwargs):
    """The reference's training run (dl_model.py:230-243) with sizes and epochs as arguments: load or generate the (field, QoI
    error) pairs (data = (z_train, errors_train, z_val, errors_val) skips that), build the network, fit under lr_schedule with
    the validation set, save the weights to out_path (.npz) when given.  -> (model, history)."""
    if data is None:
        data = load_dataset_avg_rom(load_prev, tr_size, v_size, data_dir=data_dir, **gen_kwargs)
    z_tr, e_tr, z_v, e_v = (np.asarray(a) for a in data)
    model = ResBnFcModel(z_tr.shape[1], e_tr.shape[1], n_layers, n_weights, seed)
    hist = model.fit(z_tr, e_tr, epochs=epochs, batch_size=batch_size, shuffle=True, validation_data=(z_v, e_v), lr=lr, seed=seed,
                     device=device, graph=graph)
    if out_path is not None:
        model.save(out_path)
    return model, hist


# ---- the pure deep-learning surrogate (reference dl_model.py:202-214 `load_surrogate_model`) ---------------------------------------
SURROGATE_LAYERS, SURROGATE_WIDTH = 3, 50      # res_bn_fc_model(ELU(), Adam, 3e-4, 3, 50, 1446, 40): the error model's network


class Surrogate:
    """The same network as a model of its own: nodal conductivity -> observables, misfit 1/2 |data - NN(k)|^2.
    device=True: engine.DeviceErrorModel.misfit_grad (finrom_mlp_misfit_grad: NumPy in, NumPy out; torch in, torch out on the
    current stream); device=False: the NumPy statement through ResBnFcModel.predict / .vjp (fp32 network, loss and gradient
    widened to double as the device stores them)."""

    def __init__(self, model, device=True):
        self.model, self.device = model, bool(device)
        self.n_in, self.n_out = model.n_in, model.n_out
        self._dev = None
        if self.device:
            from ..engine import DeviceErrorModel
            self._dev = DeviceErrorModel(model)

    @staticmethod
    def _pack(loss, grad, qoi):
        if loss is None:
            info = None
        elif hasattr(loss, "is_cuda"):
            import torch
            info = (~torch.isfinite(loss)).to(torch.int32)
        else:
            info = (~np.isfinite(loss)).astype(np.int32)
        return {"loss": loss, "grad": grad, "qoi": qoi, "info": info}

    def predict_batch(self, K):
        """-> dict(loss None, grad None, qoi [S, n_out], info None)."""
        if self.device:
            r = self._dev.misfit_grad(K, None, want_grad=False)
            return self._pack(None, None, r["out"])
        return self._pack(None, None, np.asarray(self.model.predict(np.asarray(K, dtype=np.float64)), dtype=np.float64))

    def misfit_grad_batch(self, K, data, want_grad=True):
        """K [S, n]; data [n_out] or [S, n_out] -> dict(loss [S], grad [S, n], qoi [S, n_out], info [S]: 1 where the loss is not finite)."""
        if self.device:
            r = self._dev.misfit_grad(K, data, want_grad=want_grad)
            return self._pack(r["loss"], r["grad"], r["out"])
        X = np.asarray(K, dtype=np.float64).reshape(-1, self.n_in)
        out = np.asarray(self.model.predict(X), dtype=np.float64)
        r = np.asarray(data, dtype=np.float64).reshape(-1, self.n_out) - out
        loss = 0.5 * np.sum(r * r, axis=1)
        grad = -np.asarray(self.model.vjp(X, r), dtype=np.float64) if want_grad else None
        return self._pack(loss, grad, out)

    def whitened(self, prior):
        """The Surrogate of whiten_first_layer(self.model, prior) on the same device setting: its misfit at whitened coordinates v is
        this one's at the field prior.field(v), its gradient the pullback of this one's (up to the fp32 rounding of the folded first
        layer).  What the fused chains of hmc.run_chains_fused(model="ml", ml_form=...) run on under a prior."""
        return Surrogate(whiten_first_layer(self.model, prior), device=self.device)

    def set_tile_min(self, tile_min):
        if self._dev is not None:
            self._dev.set_tile_min(tile_min)

    def last_form(self):
        return self._dev.last_form() if self._dev is not None else 0

    def close(self):
        if self._dev is not None:
            self._dev.close()
            self._dev = None


def whiten_first_layer(model, prior, dtype=np.float32):
    """The latent Gaussian-field prior folded into the first layer.  With k = m + U^T v (prior.field),
        W0^T k + b0 = (U W0)^T v + (b0 + W0^T m),
    so the network with W0' = U W0 and b0' = b0 + W0^T m evaluated at v is the network evaluated at the field, and its input
    gradient is the pullback U grad_k: the whitened potential loss(k(v)) / sigma^2 + |v|^2 / 2 is the i.i.d. potential (mean 0,
    tau = 1) of that network.  Both products are formed in float64 and then cast to `dtype`; every other array is SHARED with
    `model` (not copied), the optimiser state is not taken over.  -> ResBnFcModel."""
    U, m = np.asarray(prior.U, dtype=np.float64), np.asarray(prior.mean, dtype=np.float64)
    if U.shape != (model.n_in, model.n_in) or m.shape != (model.n_in,):
        raise ValueError(f"whiten_first_layer: the prior has {U.shape[0]} nodes, the network {model.n_in} inputs")
    W0 = np.asarray(model.W0, dtype=np.float64)
    out = ResBnFcModel.__new__(ResBnFcModel)
    out.n_in, out.n_out, out.n_layers, out.n_weights = model.n_in, model.n_out, model.n_layers, model.n_weights
    out.W0 = np.ascontiguousarray(U @ W0).astype(dtype)
    out.b0 = (np.asarray(model.b0, dtype=np.float64) + m @ W0).astype(dtype)
    out.units, out.head = model.units, model.head
    out.opt = {"t": 0, "epoch": 0, "m": None, "v": None}
    return out


def load_surrogate_model(path, randobs=True):
    """The reference's surrogate (dl_model.py:202-214): 3 units, 50 wide, 40 outputs (randobs) or 9 (sub-fin averages), read from
    an .npz written by ResBnFcModel.save (Keras checkpoints cannot be read here).  -> ResBnFcModel."""
    model = ResBnFcModel.load(path)
    want = (SURROGATE_LAYERS, SURROGATE_WIDTH, 40 if randobs else 9)
    if (model.n_layers, model.n_weights, model.n_out) != want:
        raise ValueError(f"load_surrogate_model: {path} holds (units, width, outputs) = {(model.n_layers, model.n_weights, model.n_out)}, "
                         f"the reference's surrogate is {want}")
    return model


def train_surrogate_model(out_path=None, *, epochs=5000, batch_size=500, lr=lr_schedule, seed=0, data=None, tr_size=6000, v_size=500,
                          data_dir='../data', device=True, graph=True, **gen_kwargs):
    """train_error_model for the surrogate: the reference's sizes (3 units, 50 wide, n_obs outputs), targets the FOM observables
    of the dataset generator (gen_affine_avg_rom_dataset(want_qoi=True)); data = (z_train, qoi_train, z_val, qoi_val) skips the
    generation.  -> (model, history)."""
    if data is None:
        from .generate_fin_dataset import gen_affine_avg_rom_dataset
        data = []
        for size in (tr_size, v_size):
            z, _, q = gen_affine_avg_rom_dataset(size, out_dir=data_dir, want_qoi=True, **gen_kwargs)
            data += [z, q]
    z_tr, q_tr, z_v, q_v = (np.asarray(a) for a in data)
    model = ResBnFcModel(z_tr.shape[1], q_tr.shape[1], SURROGATE_LAYERS, SURROGATE_WIDTH, seed)
    hist = model.fit(z_tr, q_tr, epochs=epochs, batch_size=batch_size, shuffle=True, validation_data=(z_v, q_v), lr=lr, seed=seed,
                     device=device, graph=graph)
    if out_path is not None:
        model.save(out_path)
    return model, hist
