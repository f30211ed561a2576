"""Reference and case builder for the leapfrog step in whitened coordinates (finrom_hmc_leapfrog_field / _field_metric,
csrc/api_hmc.hip: hmc_velocity_kernel, field_prior_kernel<false> in its fused form, the plain finrom_romml_grad launches,
field_prior_kernel<true> with its tail), shared by tests/test_hmc_leapfrog_field_host.py (which ties this reference to
hmc.run_chains and checks that the cases are what they claim) and tests/test_gpu_hmc_leapfrog_field.py (which checks the kernels
against it).  Imports without a GPU.

The reference restates include/finrom.h and hmc.run_chains / hmc.whitened_potential, not the kernels.  One step maps
(v, p, eps, c_lik, U, field mean, optional (Vt, lam)) and a value-and-gradient supplied from outside to
    vel = M^-1 p (metric only), w = v + eps q (q = vel under a metric, p otherwise), field = mean + U^T w,
    dU = w + c_lik U grad(field) (0 for a flagged chain), p' = p - eps dU (p for a flagged chain);
  * the elementwise updates are ONE fused multiply-add each, exact with one rounding (hmc_cases.fma);
  * the products with U and the metric's dot products are in np.longdouble, each with its scale (the sum of the absolute values
    of its terms).
Conventions (sentinel padding, DeviceState, same_bits) are those of tests/hmc_cases.py.

The flagged chains.  A chain is flagged (info != 0) when its reduced operator cannot be factored: a pivot that is not > 0.  The
reduced model is least-squares Petrov-Galerkin, A_r = psi^T psi, so NO finite field of moderate size makes A_r indefinite -- a
negated positive field gives the positive definite A_r of another operator (tests/test_hmc_leapfrog_field_host.py asserts this; it
is why tests/test_gpu_parity.py says "an indefinite reduced operator cannot occur").  The finite poison is therefore a negated
positive field of size POISON_SCALE = 1e200: v_c from a triangular solve with U, every number the step writes for the chain
(position, field, dU = 0, momentum) finite and checkable, and psi^T psi beyond the largest double, so that no positive pivot
sequence exists (the host test asserts the oracle's A_r is not finite there).  The second poison is a NaN in one entry of v_c."""
import functools
from collections import namedtuple

import numpy as np
import scipy.linalg

import hmc_cases as H
import mlp_cases as K

LD = H.LD
EPS, C_LIK, STEPS = 0.0123, 1.0 / 0.3 ** 2, 3        # neither a power of two nor 1; c_pri = 1 as the API requires
FIELD_TOL = 2e-13                                    # tests/test_gpu_field_prior.py's constant for the triangular products
POISON_SCALE = 1e200
NET = {4: (17, 2), 8: (31, 4), 12: (50, 5)}          # (n_w, n_layers) of the error model per mesh
RANK = {4: 8, 8: 8, 12: 16}                          # basis width per mesh: the rigs tests/mlp_cases.py already builds
FP_B, FP_PIECE = 128, 64                             # field_prior.hip: super-tile edge, batch rows per launch

Case = namedtuple("Case", "name m C rho per_sample projection poison outputs")


def _case(m, C, rho=0, per_sample=False, projection="direct", poison=None, outputs=False):
    name = f"m{m}-C{C}" + (f"-rho{rho}" if rho else "") + ("-per-sample" if per_sample else "") + \
           ("-oo" if projection != "direct" else "") + ("-outputs" if outputs else "") + (f"-{poison}" if poison else "")
    return Case(name, m, C, rho, per_sample, projection, poison, outputs)


# n = 245 (NB 2, 117 columns in the last super-tile: both sub-tiles live): RT = 1 / 2 / 4 at their edges, 17 = a row chunk with one
# live row, 65 = a second launch of one row, 70 = a second piece with RT = 2; C > 64 also takes finrom_romml_grad's batched form.
# n = 777 (NB 7, 9 columns in the last strip: second sub-tile dead).  n = 1597 (NB 13): nq = 13 partial strips against
# G = 16 / 8 / 4.  One row with per-sample data, one with the offline-online projection (the batched romml form at C <= 64), one
# that passes qoi_r and e_nn; the metric with rho = 1 (one sweep, one live wave), 17 (a second sweep of one eigenvector), 64.
CLEAN = ([_case(4, C) for C in (1, 4)] + [_case(4, 5, outputs=True)] + [_case(4, C) for C in (8, 9, 17, 64, 65, 70)] +
         [_case(8, 3, per_sample=True), _case(8, 8), _case(12, 4), _case(12, 8), _case(12, 17), _case(12, 4, projection="offline_online"),
          _case(4, 5, rho=1), _case(4, 65, rho=17), _case(12, 8, rho=64)])
POISON_BASES = [_case(4, 5, outputs=True), _case(4, 65), _case(4, 70), _case(12, 8), _case(4, 65, rho=17)]
POISONED = [b._replace(name=b.name + "-" + p, poison=p) for b in POISON_BASES for p in ("finite", "nan")]
CASES = CLEAN + POISONED
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def clean_of(lc):
    return BY_NAME[lc.name[:-len(lc.poison) - 1]] if lc.poison else lc


def fused_row(lc):
    """The case as a row of tests/mlp_cases.py's table (its reduced model and error model are built from one): nine averages, nine
    observables, no pins; which form finrom_romml_grad takes for it is not claimed here (form, staged, pre: None)."""
    n_w, n_layers = NET[lc.m]
    return K.Fused(lc.name, lc.m, RANK[lc.m], lc.projection, 9, 9, n_w, n_layers, lc.C, lc.per_sample, False, None, None, None)


def poisoned_chains(lc):
    """A first, a middle and a last chain (C = 65, 70: the last sits behind index 64)."""
    return sorted({0, lc.C // 2, lc.C - 1}) if lc.poison else []


def nan_column(n, c):
    """Where chain c's NaN sits: the first chain's in column 0, the last one's in the last column, the others' in between."""
    return 0 if c == 0 else (n - 1 if c % 2 == 0 else (7 + 50 * c) % n)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def factor(n):
    """An upper factor with the Matern factor's character (positive diagonal, decaying rows; tests/test_gpu_field_prior.py's),
    scaled by 1/4 so that mean + U^T w stays positive for the cases' w."""
    rng = np.random.default_rng([n, 77])
    U = np.triu(rng.standard_normal((n, n))) / np.sqrt(np.arange(1, n + 1))[None, :]
    U[np.diag_indices(n)] = np.abs(U[np.diag_indices(n)]) + 0.5
    U *= 0.25
    U.setflags(write=False)
    return U


@functools.lru_cache(maxsize=None)
def field_mean(n):
    m = np.random.default_rng([n, 78]).uniform(0.8, 1.2, n)
    m.setflags(write=False)
    return m


def velocity(p, metric):
    """M^-1 p = p - sum_j lam_j / (1 + lam_j) V_j (V_j . p), row-wise -> (longdouble, scale)."""
    Vt, lam = metric
    VL, c = Vt.astype(LD), -(lam.astype(LD) / (1 + lam.astype(LD)))
    with np.errstate(all="ignore"):
        vel = p + ((p.astype(LD) @ VL.T) * c) @ VL
        scale = np.abs(p) + ((np.abs(p) @ np.abs(Vt).T) * np.abs(c).astype(np.float64)) @ np.abs(Vt)
    return vel, scale


def field_of(w, U, mean):
    """mean + U^T w, row-wise -> (longdouble, scale |w| |U| + |mean|)."""
    with np.errstate(all="ignore"):
        return w.astype(LD) @ U.astype(LD) + mean.astype(LD), np.abs(w) @ np.abs(U) + np.abs(mean)


def pullback_of(g, U):
    """U g, row-wise -> (longdouble, scale |U| |g|)."""
    with np.errstate(all="ignore"):
        return g.astype(LD) @ U.astype(LD).T, np.abs(g) @ np.abs(U).T


def ref_step(v, p, eps, c_lik, U, mean, value_and_grad, metric=None):
    """One step.  value_and_grad(field [C, n] float64) -> (loss [C], grad [C, n], bad [C] bool).  -> dict: vel / vel_scale (metric
    only), w (exact), field (longdouble) / field_scale, loss, grad, bad, g_v (longdouble) / g_scale, dU (exact on the rounded g_v; 0
    where bad) / dU_scale = |w| + c_lik |U| |grad|, p (exact; the old p where bad)."""
    out = {}
    q = p
    if metric is not None:
        out["vel"], out["vel_scale"] = velocity(p, metric)
        q = out["vel"].astype(np.float64)
    w = H.fma(eps, q, v)
    fld, fscale = field_of(w, U, mean)
    loss, grad, bad = value_and_grad(fld.astype(np.float64))
    bad = np.asarray(bad, dtype=bool)
    gv, gscale = pullback_of(np.where(bad[:, None], 0.0, grad), U)
    dU = np.where(bad[:, None], 0.0, H.fma(c_lik, gv.astype(np.float64), np.where(bad[:, None], 0.0, w)))
    out.update(w=w, field=fld, field_scale=fscale, loss=loss, grad=grad, bad=bad, g_v=gv, g_scale=gscale, dU=dU,
               dU_scale=np.abs(w) + c_lik * gscale, p=np.where(bad[:, None], p, H.fma(-eps, dU, p)))
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _start(m, C, rho):
    n = K.MESH_N[m]
    rng = np.random.default_rng([m, C, rho, 5])
    v0, p0 = 0.3 * rng.standard_normal((C, n)), rng.standard_normal((C, n))
    metric = H.metric_case(n, rho) if rho else None
    if metric is not None:                                           # a momentum with weight inside the metric's subspace
        p0 = p0 + (3.0 * rng.standard_normal((C, rho))) @ metric[0]
    return v0, p0, metric


def problem(lc):
    """-> dict(n, U, mean, v0, p0, metric, data, chains (the poisoned ones), clean (bool [C])).  A poisoned case is its clean case
    with the rows `chains` of v0 replaced."""
    n = K.MESH_N[lc.m]
    v0, p0, metric = _start(lc.m, lc.C, lc.rho)
    U, mean = factor(n), field_mean(n)
    v0 = v0.copy()
    chains = poisoned_chains(lc)
    if lc.poison == "finite":
        f = K.rom_inputs(n, len(chains), seed=9)
        v0[chains] = scipy.linalg.solve_triangular(U, (-POISON_SCALE * f - mean).T, trans="T", lower=False).T
    elif lc.poison == "nan":
        for c in chains:
            v0[c, nan_column(n, c)] = np.nan
    clean = np.ones(lc.C, bool)
    clean[chains] = False
    return dict(n=n, U=U, mean=mean, v0=v0, p0=p0.copy(), metric=metric, data=K.fused_data(fused_row(lc)), chains=chains, clean=clean)


def state(lc, pr=None):
    """The finrom_hmc_state of a case as hmc_cases.DeviceState takes it: positions v0 in Kq0, momenta in P, st->mean zeros, c_pri 1;
    the step's outputs (Kq1, dUq, loss) NaN and info 5, everything else filled, to be found unchanged."""
    pr = problem(lc) if pr is None else pr
    C, n = lc.C, pr["n"]
    g = np.random.default_rng([lc.m, C, 6]).standard_normal
    return dict(C=C, n=n, eps=EPS, c_lik=C_LIK, c_pri=1.0, mean=np.zeros((C, n)), K=g((C, n)), U=np.abs(g(C)), dU=g((C, n)),
                Kq0=pr["v0"].copy(), Kq1=np.full((C, n), np.nan), P=pr["p0"].copy(), dUq=np.full((C, n), np.nan), H0=g(C),
                P_block=g((2, C, n)), lu_block=g((2, C)), jt=1, pt=2, accept=10 + 3 * np.arange(C, dtype=np.int64), trace=g((4, C, n)),
                loss=np.full(C, np.nan), info=np.full(C, 5, np.int32))


def romml_value_and_grad(lc, pr, flagged=()):
    """The float64 reference of the misfit (mlp_cases.romml_ref) as a value-and-gradient for ref_step; the chains `flagged` are
    not evaluated: NaN and bad."""
    row = fused_row(lc)
    prob, phi, ro = K.oracle_rig(row.m, row.r, row.n_obs)
    model = K.fused_model(row)

    def f(field):
        C, n = field.shape
        loss, grad, bad = np.full(C, np.nan), np.full((C, n), np.nan), np.zeros(C, bool)
        for c in range(C):
            if c in flagged:
                bad[c] = True
                continue
            r = K.romml_ref(ro, model, field[c], pr["data"][c] if lc.per_sample else pr["data"], "f64")
            loss[c], grad[c] = r["loss"], r["grad"]
        return loss, grad, bad
    return f


def reduced_operator(lc, field):
    """The oracle's A_r = psi^T psi at one field (AffineROMOracle.forward_nine_param_reduced without its solve)."""
    row = fused_row(lc)
    prob, phi, ro = K.oracle_rig(row.m, row.r, row.n_obs)
    with np.errstate(all="ignore"):
        psi = prob.assemble_affine(ro.dsigma_dk @ field) @ phi
        return np.asarray(psi.T @ psi)
