"""MAP estimation of the fin's conductivity from its observations: the study of the reference's bayesian_inference/
estimate_MAP.py, with the starts batched.

The reference minimises  0.5 |y(k) - d|^2 + reg(k)  (reg = 0.5 gamma k^T K1 k, fom/forward_solve.py:186-191) over the nodal
conductivity with SciPy's L-BFGS-B inside the box [0.95 min k_true, 1.05 max k_true] (:274-281, ftol 1e-10, gtol 1e-8), from
n_starting_pts = 6 draws exp(0.5 U^T xi) (:246-263), one start after another, for three models: the FOM (SolverWrapper
:86-109), the ROM (RSolverWrapper :186-213) and the ROM + learned error model (ROMMLSolverWrapper :111-145).  Its best start
per model is saved as res_FOM.npy / res_ROM.npy / res_ROMML.npy (:318, 382, 454); the reference's HMC starts from that file.

Here:
  * objective(kind, ...) gives a model's misfit as a device callable (torch tensors in and out, the model's library calls in
    place, for lbfgs.minimize_device) and as a NumPy callable (for lbfgs.minimize_host), plus the pieces the library adds itself
    (the G map of the ROM's sub-fin averages, the Tikhonov term);
  * SolverWrapper / RSolverWrapper / ROMMLSolverWrapper restate the reference's one-sample cost_function / gradient surface with
    its timers, so that the reference's SciPy loop runs unchanged (and is the yardstick of the tests);
  * estimate_map(...) is the reference's study as a function, one batched minimize_device call per model.
The pure-DL surrogate inversion (MLSolverWrapper :147-184, res_ML.npy) is the fourth model, "ml": the network of
deep_learning/dl_model.py as a model of its own (Surrogate, finrom_mlp_misfit_grad)."""
from __future__ import annotations

import os
import time

import numpy as np

from . import lbfgs
from ..fem import Function, as_nodal

GAMMA = 1e-6          # the reference's Fin.gamma


class Objective:
    """A model's misfit in the two forms lbfgs takes.
    device(Xt) -> (f [S], g [S, gdim or d], bad [S]) on torch tensors; host(X) -> the same in NumPy, with `gmap` and `tikhonov`
    applied as finrom_lbfgs_accept adds them on the device (lbfgs.library_terms: the same order).  gmap: G [gdim x d] or None; tikhonov: (gamma, K1) or None."""

    def __init__(self, device, host_raw, d, gmap=None, tikhonov=None):
        self.device, self._host_raw, self.d, self.gmap, self.tikhonov = device, host_raw, d, gmap, tikhonov

    def host(self, X):
        X = np.asarray(X, dtype=np.float64)
        f, g, bad = self._host_raw(X)
        f, g = lbfgs.library_terms(X, f, g, self.gmap, self.tikhonov)
        return f, g, np.asarray(bad, dtype=bool)

    def minimize(self, X0, *, device=True, **kw):
        if device:
            return lbfgs.minimize_device(self.device, X0, gmap=self.gmap, tikhonov=self.tikhonov, **kw)
        return lbfgs.minimize_host(self.host, X0, **kw)


def _torch_data(data, S=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(data, dtype=np.float64), dtype=torch.float64,
                           device=torch.device("cuda", torch.cuda.current_device()))


def objective(kind, data, *, solver=None, solver_r=None, params=None, gamma=None, surrogate=None):
    """kind 'fom' (solver: Fin; params None = nodal fields, 'five' / 'nine' = fin conductivities through Fin.gradient_batch),
    'rom' (solver_r: AffineROMFin; fields through finrom_subfin_avg -> finrom_rom_grad, or params='five' / 'nine' with theta the
    nine fin values; the library maps the gradient back with G), 'romml' (solver_r with a device error model; fields:
    finrom_romml_grad), 'ml' (surrogate: dl_model.Surrogate; fields only: finrom_mlp_misfit_grad; the Tikhonov term needs
    solver= or solver_r= for K1).  gamma: the reference's Tikhonov term 0.5 gamma k^T K1 k (K1 = Fin._unit_stiffness(); fields only;
    None: no regulariser).  data: the observations [n_obs]."""
    data = np.ascontiguousarray(data, dtype=np.float64)
    dt = {}

    def data_t():
        if "t" not in dt:
            dt["t"] = _torch_data(data)
        return dt["t"]

    if kind == "fom":
        if solver is None:
            raise ValueError("objective('fom'): needs solver=Fin")
        d = {None: solver.dofs, "five": 5, "nine": 9}[params]

        def dev(X):
            r = solver.gradient_batch(X, data_t(), params=params)
            return r["J"], r["grad"], r["info"].ne(0)

        def host(X):
            r = solver.gradient_batch(X, data, params=params)
            return r["J"], r["grad"], np.asarray(r["info"]) != 0
        ops, gmap = solver.ops, None
    elif kind == "rom":
        if solver_r is None:
            raise ValueError("objective('rom'): needs solver_r=AffineROMFin")
        ops = solver_r.ops
        if params is None:
            d, gmap, avg = solver_r.n, ops.S, solver_r._avg
        else:
            from ..engine import SubfinAverager
            gmap = np.asarray(ops.E59 if params == "five" else np.eye(9))
            d, avg = gmap.shape[1], SubfinAverager(gmap)

        def dev(X):
            r = solver_r.grad_reduced_batch(None, data=data_t(), theta=avg(X))
            return r["J"], r["g_theta"], r["info"].ne(0)

        def host(X):
            r = solver_r.grad_reduced_batch(None, data=data, theta=avg(np.ascontiguousarray(X)))
            return r["J"], r["g_theta"], np.asarray(r["info"]) != 0
    elif kind == "romml":
        if solver_r is None or solver_r._dev_model is None:
            raise ValueError("objective('romml'): needs solver_r=AffineROMFin with a device error model (a ResBnFcModel)")
        if params is not None:
            raise ValueError("objective('romml'): the error model takes nodal fields (params=None)")
        d, gmap, ops = solver_r.n, None, solver_r.ops

        def dev(X):
            r = solver_r.grad_romml_batch(X, data=data_t())
            return r["loss"], r["grad"], r["info"].ne(0)

        def host(X):
            r = solver_r.grad_romml_batch(np.asarray(X), data=data)
            return r["loss"], r["grad"], np.asarray(r["info"]) != 0
    elif kind == "ml":
        if surrogate is None:
            raise ValueError("objective('ml'): needs surrogate=Surrogate")
        if params is not None:
            raise ValueError("objective('ml'): the surrogate takes nodal fields (params=None)")
        if data.shape[-1] != surrogate.n_out:
            raise ValueError(f"objective('ml'): {data.shape[-1]} observations, the surrogate has {surrogate.n_out} outputs")
        d, gmap = surrogate.n_in, None
        ops = solver.ops if solver is not None else (solver_r.ops if solver_r is not None else None)
        if gamma is not None and ops is None:
            raise ValueError("objective('ml'): the Tikhonov term needs solver= or solver_r= (K1)")

        def dev(X):
            r = surrogate.misfit_grad_batch(X, data_t())
            return r["loss"], r["grad"], r["info"].ne(0)

        def host(X):
            r = surrogate.misfit_grad_batch(np.asarray(X), data)
            return r["loss"], r["grad"], np.asarray(r["info"]) != 0
    else:
        raise ValueError(f"unknown model {kind!r} (fom, rom, romml, ml)")
    tik = None
    if gamma is not None:
        if params is not None:
            raise ValueError("the Tikhonov term is defined on nodal fields (params=None)")
        tik = (float(gamma), unit_stiffness(ops))
    return Objective(dev, host, d, gmap=gmap, tikhonov=tik)


def unit_stiffness(ops):
    """K1 = int grad u . grad v dx as CSR (Fin._unit_stiffness)."""
    return ops.csr(ops.sub_vals.sum(axis=0))


# ---- the reference's one-sample surface (estimate_MAP.py:86-213), restated ------------------------------------------------------
class SolverWrapper:
    """FOM misfit + Tikhonov term, one sample per call (estimate_MAP.py:86-109)."""

    def __init__(self, solver, data):
        self.solver, self.data = solver, np.asarray(data, dtype=np.float64)
        self.z = Function(solver.V)
        self.fwd_time = 0.0
        self.grad_time = 0.0

    def cost_function(self, z_v):
        self.z.vector().set_local(z_v)
        t_i = time.time()
        w, _, _, _, _ = self.solver.forward(self.z)
        y = self.solver.qoi_operator(w)
        self.fwd_time += time.time() - t_i
        self.solver._k.assign(self.z)
        return 0.5 * np.linalg.norm(y - self.data) ** 2 + self.solver.reg

    def gradient(self, z_v):
        self.z.vector().set_local(z_v)
        t_i = time.time()
        grad = self.solver.gradient(self.z, self.data)
        self.grad_time += time.time() - t_i
        self.solver._k.assign(self.z)
        return grad + self.solver.grad_reg


class RSolverWrapper:
    """ROM misfit + Tikhonov term (estimate_MAP.py:186-213)."""

    def __init__(self, err_model, solver_r, solver):
        self.err_model, self.solver_r, self.solver = err_model, solver_r, solver
        self.z = Function(solver.V)
        self.data = self.solver_r.data
        self.cost = None
        self.grad = None
        self.fwd_time = 0.0
        self.grad_time = 0.0

    def cost_function(self, z_v):
        self.z.vector().set_local(z_v)
        w_r = self.solver_r.forward_reduced(self.z)
        y_r = self.solver_r.qoi_reduced(w_r)
        self.fwd_time = self.solver_r.fwd_time
        self.solver._k.assign(self.z)
        self.cost = 0.5 * np.linalg.norm(y_r - self.data) ** 2 + self.solver.reg
        return self.cost

    def gradient(self, z_v):
        self.z.vector().set_local(z_v)
        self.solver._k.assign(self.z)
        self.grad, self.cost = self.solver_r.grad_reduced(self.z)
        self.grad = self.grad + self.solver.grad_reg
        self.grad_time = self.solver_r.rom_grad_time
        return self.grad


class ROMMLSolverWrapper:
    """ROM + learned-error misfit + Tikhonov term (estimate_MAP.py:111-145)."""

    def __init__(self, err_model, solver_r, solver):
        self.err_model, self.solver_r, self.solver = err_model, solver_r, solver
        self.z = Function(solver.V)
        self.data = self.solver_r.data
        self.cost = None
        self.grad = None
        self.fwd_time_dl = 0.0
        self.fwd_time_rom = 0.0
        self.grad_time = 0.0
        self.grad_time_dl = 0.0

    def cost_function(self, z_v):
        self.z.vector().set_local(z_v)
        w_r = self.solver_r.forward_reduced(self.z)
        y_r = self.solver_r.qoi_reduced(w_r)
        t_i = time.time()
        e_nn = np.asarray(self.err_model.predict(np.asarray(z_v, dtype=np.float64)[None, :])[0], dtype=np.float64)
        self.fwd_time_dl += time.time() - t_i
        self.solver._k.assign(self.z)
        self.cost = 0.5 * np.linalg.norm(y_r + e_nn - self.data) ** 2 + self.solver.reg
        self.fwd_time_rom = self.solver_r.fwd_time
        return self.cost

    def gradient(self, z_v):
        self.z.vector().set_local(z_v)
        self.solver._k.assign(self.z)
        self.grad, self.cost = self.solver_r.grad_romml(self.z)
        self.grad = self.grad + self.solver.grad_reg
        self.grad_time = self.solver_r.romml_grad_time
        self.grad_time_dl = self.solver_r.romml_grad_time_dl
        return self.grad


class MLSolverWrapper:
    """Surrogate misfit + Tikhonov term, one sample per call (estimate_MAP.py:147-184): cost 1/2 |NN(z) - d|^2 + reg,
    gradient tf.gradients(loss, input) + grad_reg.  surrogate: dl_model.Surrogate (device or host)."""

    def __init__(self, surrogate_model, data, solver):
        self.model, self.solver, self.data = surrogate_model, solver, np.asarray(data, dtype=np.float64)
        self.z = Function(solver.V)
        self.cost = None
        self.grad = None
        self.fwd_time = 0.0
        self.grad_time = 0.0

    def cost_function(self, z_v):
        self.z.vector().set_local(z_v)
        t_i = time.time()
        y_NN = np.asarray(self.model.predict_batch(np.asarray(z_v, dtype=np.float64)[None, :])["qoi"][0], dtype=np.float64)
        self.fwd_time += time.time() - t_i
        self.solver._k.assign(self.z)
        self.cost = 0.5 * np.linalg.norm(y_NN - self.data) ** 2 + self.solver.reg
        return self.cost

    def gradient(self, z_v):
        t_i = time.time()
        grad_NN = np.asarray(self.model.misfit_grad_batch(np.asarray(z_v, dtype=np.float64)[None, :], self.data)["grad"][0])
        self.grad_time += time.time() - t_i
        self.z.vector().set_local(z_v)
        self.solver._k.assign(self.z)
        self.grad = grad_NN + self.solver.grad_reg
        return self.grad


# ---- the study ------------------------------------------------------------------------------------------------------------
def starting_points(V, n_starting_pts=6, seed=0, length=1.6):
    """exp(0.5 U^T xi), xi ~ N(0, I), U = make_cov_chol(V, length) (estimate_MAP.py:246-263) -> [n_starting_pts, n]."""
    from .gaussian_field import make_cov_chol
    chol = make_cov_chol(V, length=length)
    rng = np.random.default_rng(seed)
    return np.stack([np.exp(0.5 * chol.T @ rng.standard_normal(chol.shape[0])) for _ in range(n_starting_pts)])


def reconstruction_errors(solver, k_true, X, data):
    """Per row of X: the relative observation error |d - B w(x)| / |d| from an FOM solve (:295-300), the relative L2
    reconstruction error |k_true - x|_M / |k_true|_M (:302-305) and the reference's pointwise error
    |k_true - x|_2 / sqrt(|k_true|_M) (:322)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    M = solver.M
    q = np.asarray(solver.forward_batch(X, want_w=False)["qoi"])
    obs = np.linalg.norm(q - data[None, :], axis=1) / np.linalg.norm(data)
    E = k_true[None, :] - X
    norm_true = np.sqrt(k_true @ M @ k_true)
    l2 = np.sqrt(np.einsum("sn,nm,sm->s", E, M, E)) / norm_true
    pw = np.linalg.norm(E, axis=1) / np.sqrt(norm_true)
    return obs, l2, pw


_FILES = {"fom": "res_FOM.npy", "rom": "res_ROM.npy", "romml": "res_ROMML.npy", "ml": "res_ML.npy"}


def estimate_map(solver, solver_r, k_true, *, n_starting_pts=6, seed=0, length=1.6, models=("fom", "rom", "romml"),
                 gamma=GAMMA, ftol=1e-10, gtol=1e-8, out_dir=None, device=True, X0=None, surrogate=None, **options):
    """The reference's MAP study (estimate_MAP.py) as a function: synthetic data d = B w(k_true) from an FOM solve, the box
    [0.95 min k_true, 1.05 max k_true], n_starting_pts starts exp(0.5 U^T xi) (or X0), and per model ONE batched minimisation
    of its misfit + the Tikhonov term (lbfgs.minimize_device; device=False: minimize_host over the same callables).
    solver_r must carry the data (set_data) for the ROM models; it is set here.
    Returns {model: dict(x [S, n], fun, nit, nfev, status, message, obs_err, l2_err, pw_err, best (index), time_s)}, with
    `data` and `starts` beside; out_dir: res_FOM.npy / res_ROM.npy / res_ROMML.npy hold each model's best x (by l2_err, as the
    reference keeps the start of least reconstruction error).  "ml" in models needs surrogate= (dl_model.Surrogate) and writes
    res_ML.npy."""
    k_true = as_nodal(k_true).astype(np.float64)
    data = np.asarray(solver.qoi_operator(solver.forward(k_true)[0]), dtype=np.float64)
    if solver_r is not None:
        solver_r.set_data(data)
    X0 = starting_points(solver.V, n_starting_pts, seed, length) if X0 is None else np.atleast_2d(np.asarray(X0, dtype=np.float64))
    bounds = (0.95 * float(k_true.min()), 1.05 * float(k_true.max()))
    out = {"data": data, "starts": X0, "bounds": bounds}
    for kind in models:
        obj = objective(kind, data, solver=solver, solver_r=solver_r, gamma=gamma, surrogate=surrogate)
        t0 = time.perf_counter()
        res = obj.minimize(X0, device=device, bounds=bounds, ftol=ftol, gtol=gtol, **options)
        dt = time.perf_counter() - t0
        obs, l2, pw = reconstruction_errors(solver, k_true, res["x"], data)
        best = int(np.argmin(l2))
        out[kind] = dict(x=res["x"], fun=res["fun"], nit=res["nit"], nfev=res["nfev"], status=res["status"], message=res["message"],
                         obs_err=obs, l2_err=l2, pw_err=pw, best=best, time_s=dt)
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
            np.save(os.path.join(out_dir, _FILES[kind]), res["x"][best])
    return out
