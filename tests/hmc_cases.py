"""Reference and case builder for the four kernels that open and close an HMC proposal (finrom_hmc_begin / _end, csrc/hmc_kernels.hip;
finrom_hmc_begin_metric / _end_metric, csrc/hmc_metric.hip), shared by tests/test_hmc_kernels_host.py (which checks this reference
against hmc.run_chains) and tests/test_gpu_hmc_kernels.py (which checks the kernels against it).  Imports without a GPU.

The reference restates include/finrom.h and hmc.run_chains, not the kernels:
  * elementwise outputs bit for bit: the half steps of the momentum are ONE fused multiply-add, p +- (0.5 eps c_pri) dU with the
    coefficient formed in double first; the exact result comes from fractions.Fraction and one float() rounding;
  * sums (H0, the end point's U, H1, the metric's dot products) in np.longdouble, each returned with its scale, the sum of the
    absolute values of its terms;
  * the decision as H0 - H1 with its scale, so that a case can put log u on a chosen side of it.
A "case" is a dict with the fields of finrom_hmc_state as NumPy arrays (Kq0 / Kq1 for Kq[0] / Kq[1]; jt, pt Python ints; trace None
or [rows, C, n]).  DeviceState uploads one with PAD sentinel elements behind every array and hands every array back."""
import functools
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
PAD = 5                               # sentinel elements behind each buffer's end: NaN for doubles, SENTINEL for integers
SENTINEL = -7777
U53 = 2.0 ** -53
METRIC_TOL = 2e-13                    # tests/test_gpu_metric.py's constant for what goes through the metric's dot products
U_LIMIT = 1.7e308                     # a potential beyond +-U_LIMIT counts as not finite
EPS, C_PRI = 0.0123, 1.0 / 0.7 ** 2   # neither a power of two nor 1
B_BLOCK, TRACE_ROWS = 3, 9
ARRAYS = (("mean", np.float64), ("K", np.float64), ("U", np.float64), ("dU", np.float64), ("Kq0", np.float64), ("Kq1", np.float64),
          ("P", np.float64), ("dUq", np.float64), ("H0", np.float64), ("P_block", np.float64), ("lu_block", np.float64),
          ("jt", np.int64), ("pt", np.int64), ("accept", np.int64), ("trace", np.float64), ("loss", np.float64), ("info", np.int32))
ROLES = ("clear accept", "clear reject", "near accept", "near reject", "role 1 with info = 2", "role 1 with info = -1", "loss = nan",
         "loss = +inf", "loss = -inf", "loss = 1.75e308", "nan in P", "inf in P")
ROLE_ACCEPTS = (True, False, True, False) + (False,) * 8


def sum_tol(n):
    """Relative bound of a plain sum of n terms in the documented order (a thread's chain of ceil(n / 256) fused multiply-adds, six
    butterfly levels, two additions across the waves) and the at most four rounded scalar operations behind it."""
    return (math.ceil(n / 256) + 12) * U53


def fma(a, x, y):
    """round(a * x + y) with ONE rounding, elementwise (broadcast).  Non-finite operands: the plain double expression (its NaN / inf
    is the fused one's)."""
    a, x, y = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, x, y)))
    with np.errstate(all="ignore"):
        plain = a * x + y
    fin = np.isfinite(a) & np.isfinite(x) & np.isfinite(y)
    out = [float(Fraction(p) * Fraction(q) + Fraction(r)) if f else pl
           for p, q, r, f, pl in zip(a.ravel().tolist(), x.ravel().tolist(), y.ravel().tolist(), fin.ravel().tolist(), plain.ravel().tolist())]
    return np.array(out, dtype=np.float64).reshape(a.shape)


def block_sum_256_emulated(p):
    """sum_i p_i^2 in double in the order block_reduce.h documents: thread t sums i = t, t + 256, ... (fused multiply-adds), a
    butterfly with offsets 32 .. 1 inside each wave of 64, then (w0 + w1) + (w2 + w3)."""
    p = np.asarray(p, dtype=np.float64)
    s = np.zeros(256)
    for i0 in range(0, len(p), 256):
        seg = p[i0:i0 + 256]
        s[:len(seg)] = fma(seg, seg, s[:len(seg)])
    lanes = np.arange(256)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[lanes ^ off]
    return (s[0] + s[64]) + (s[128] + s[192])


def half_step(s):
    """0.5 eps c_pri, formed in double first."""
    return 0.5 * s["eps"] * s["c_pri"]


def _sq(x):
    x = np.asarray(x).astype(LD)
    return np.sum(x * x, axis=-1)


def metric_case(n, rho):
    """(Vt [rho, n] with orthonormal rows from a QR, lam = logspace(-2, 5, rho); rho = 1: lam = 1e5), as tests/test_gpu_metric.py's."""
    rng = np.random.default_rng(1000 * rho + n)
    lam = np.logspace(-2, 5, rho) if rho > 1 else np.array([1e5])
    return np.ascontiguousarray(np.linalg.qr(rng.standard_normal((n, rho)))[0].T), lam


def ref_begin(s, metric=None):
    """finrom_hmc_begin (metric=(Vt, lam): finrom_hmc_begin_metric) on the case s ->
    P [C, n]: bit for bit (float64); under a metric M^(1/2) xi - 0.5 eps c_pri dU in longdouble, with P_scale;
    Kq0 = K and dUq = dU; H0 = U + |xi|^2 / 2 in longdouble with H0_scale."""
    xi = s["P_block"][s["jt"]]
    half = half_step(s)
    with np.errstate(all="ignore"):
        pp = _sq(xi)
        out = dict(Kq0=s["K"].copy(), dUq=s["dU"].copy(), H0=s["U"].astype(LD) + 0.5 * pp, H0_scale=(np.abs(s["U"]) + 0.5 * pp).astype(np.float64))
        if metric is None:
            out["P"] = fma(-half, s["dU"], xi)
            return out
        Vt, lam = metric
        VL, lamL = Vt.astype(LD), lam.astype(LD)
        c = lamL / (np.sqrt(1 + lamL) + 1)                           # sqrt(1 + lambda) - 1 without cancellation
        out["P"] = xi + ((xi.astype(LD) @ VL.T) * c) @ VL - LD(half) * s["dU"]
        out["P_scale"] = np.abs(xi) + ((np.abs(xi) @ np.abs(Vt).T) * c.astype(np.float64)) @ np.abs(Vt) + np.abs(half * s["dU"])
    return out


def ref_end(s, n_steps, metric=None):
    """finrom_hmc_end (metric=(Vt, lam): finrom_hmc_end_metric) on the case s after n_steps leapfrog steps -> dict:
    ok [C] the Metropolis decisions; diff = H0 - H1 (longdouble) with diff_scale; Uq (longdouble) the end point's potential with
    U_scale; and the state afterwards: K, dU, accept, jt, pt, trace_row (the row written at pt + 1), U (float64: Uq rounded where
    accepted).  A chain is rejected if info != 0, if its potential is NaN or beyond +-1.7e308, or if H1 is not finite."""
    C, n = s["K"].shape
    Kq = s["Kq%d" % (n_steps & 1)]
    p = fma(half_step(s), s["dUq"], s["P"])                          # the last update was a whole step: back to a half
    with np.errstate(all="ignore"):
        d = Kq - s["mean"]
        dd, pp = _sq(d), _sq(p)
        lik = LD(s["c_lik"]) * s["loss"].astype(LD)
        Uq = lik + LD(0.5) * LD(s["c_pri"]) * dd
        U_scale = np.abs(lik) + LD(0.5) * LD(s["c_pri"]) * dd
        if metric is None:
            kin = kin_scale = 0.5 * pp
        else:                                                        # p^T M^-1 p = |p - V V^T p|^2 + sum_j (V_j . p)^2 / (1 + lambda_j)
            Vt, lam = metric
            VL, lamL = Vt.astype(LD), lam.astype(LD)
            pL = p.astype(LD)
            w = pL @ VL.T
            kin = 0.5 * (_sq(pL - w @ VL) + np.sum(w * w / (1 + lamL), axis=-1))
            aw = np.abs(p) @ np.abs(Vt).T
            kin_scale = 0.5 * (pp + np.sum((lam / (1 + lam)) * aw * aw, axis=-1))
        flagged = (s["info"] != 0) | ~(np.abs(Uq) <= U_LIMIT)
        H1 = Uq + kin
        diff = s["H0"].astype(LD) - H1
        diff_scale = np.abs(s["H0"]).astype(LD) + U_scale + kin_scale
        lu = s["lu_block"][s["jt"]]
        ok = ~flagged & np.isfinite(H1) & (lu.astype(LD) < diff)
        K = np.where(ok[:, None], Kq, s["K"])
        return dict(ok=ok, diff=diff, diff_scale=diff_scale, Uq=Uq, U_scale=U_scale, K=K, dU=np.where(ok[:, None], s["dUq"], s["dU"]),
                    U=np.where(ok, Uq.astype(np.float64), s["U"]), accept=s["accept"] + ok, jt=s["jt"] + 1, pt=s["pt"] + 1,
                    trace_row=K.copy(), p=p)


def decision_bound(n, diff_scale, metric=None):
    """b: the tolerance of H0 - H1."""
    return (METRIC_TOL if metric is not None else sum_tol(n)) * np.asarray(diff_scale).astype(np.float64)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def _nan(*shape):
    return np.full(shape, np.nan)


def begin_case(n, C, jt, seed=0):
    """Random state for finrom_hmc_begin / _begin_metric: mean != 0, rows of the draw block that differ per (proposal, chain), the
    outputs (Kq0, P, dUq, H0) NaN, everything else (Kq1, trace, loss, ...) filled, to be found unchanged."""
    rng = np.random.default_rng([n, C, seed, 1])
    g = rng.standard_normal
    return dict(C=C, n=n, eps=EPS, c_lik=1.0 / 0.05 ** 2, c_pri=C_PRI, mean=1.0 + 0.1 * g((C, n)), K=1.0 + 0.3 * g((C, n)),
                U=50.0 * np.abs(g(C)), dU=3.0 * g((C, n)), Kq0=_nan(C, n), Kq1=g((C, n)), P=_nan(C, n), dUq=_nan(C, n), H0=_nan(C),
                P_block=g((B_BLOCK, C, n)), lu_block=-np.abs(g((B_BLOCK, C))), jt=jt, pt=4, accept=10 + 3 * np.arange(C, dtype=np.int64),
                trace=g((TRACE_ROWS, C, n)), loss=np.abs(g(C)), info=np.zeros(C, np.int32))


@functools.lru_cache(maxsize=None)
def end_base(n, C, rho=0, seed=0):
    """The part of an end case that does not depend on (n_steps, jt, pt, trace): chain c plays role c % 12 (ROLES).  c_lik = 1.
    log u is placed by the reference itself: with b the tolerance of H0 - H1, a "near" role at the difference -+ 64 b, a "clear" one
    at -+ 1; the roles that must reject for another reason get a log u that would accept the same chain with a finite loss / P.
    Returns a dict: the arrays (Kq_end: the end point's position; lu [C]), `ref` = ref_end's result and `b`.  Cached: read-only."""
    metric = metric_case(n, rho) if rho else None
    rng = np.random.default_rng([n, C, rho, seed, 2])
    g = rng.standard_normal
    mean = 1.0 + 0.1 * g((C, n))
    P = g((C, n))
    if metric is not None:                                           # most of |p|^2 inside the metric's subspace: pp - low cancels
        P = P + (4.0 * g((C, rho))) @ metric[0]
    s = dict(C=C, n=n, eps=EPS, c_lik=1.0, c_pri=C_PRI, mean=mean, K=1.0 + 0.3 * g((C, n)), U=50.0 * np.abs(g(C)), dU=3.0 * g((C, n)),
             Kq_end=mean + 0.3 * g((C, n)), P=P, dUq=3.0 * g((C, n)), H0=np.zeros(C), lu=np.zeros(C), loss=5.0 * np.abs(g(C)),
             info=np.zeros(C, np.int32), accept=10 + 3 * np.arange(C, dtype=np.int64), shift=rng.uniform(-0.5, 0.5, C))
    role = np.arange(C) % 12
    for c in range(C):                                               # roles 4 and 5: the data of their group's role 0
        if role[c] in (4, 5):
            for k in ("mean", "Kq_end", "P", "dUq", "loss", "shift"):
                s[k][c] = s[k][c - role[c]]

    def run():
        full = dict(s, Kq0=s["Kq_end"], Kq1=s["Kq_end"], lu_block=s["lu"][None], jt=0, pt=0)
        return ref_end(full, 0, metric)
    first = run()                                                    # every chain still finite: H1, and from it H0 and log u
    H1 = (-first["diff"]).astype(np.float64)                         # (H0 = 0 so far)
    s["H0"] = H1 + s["shift"]
    first = run()
    b = decision_bound(n, first["diff_scale"], metric)
    diff = first["diff"]
    off = np.choose(role, [-1.0, 1.0, -64 * b, 64 * b] + [-1.0] * 8)
    s["lu"] = (diff + off.astype(LD)).astype(np.float64)
    s["info"][role == 4], s["info"][role == 5] = 2, -1
    s["loss"][role == 6], s["loss"][role == 7], s["loss"][role == 8] = np.nan, np.inf, -np.inf
    s["loss"][role == 9], s["H0"][role == 9], s["lu"][role == 9] = 1.75e308, 1.79e308, -1.0
    s["P"][role == 10, n // 2], s["P"][role == 11, n - 1] = np.nan, np.inf
    ref = run()
    assert np.array_equal(ref["ok"], np.array(ROLE_ACCEPTS)[role]), "the reference does not decide the roles as they are defined"
    for a in list(s.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return dict(s, role=role, ref=ref, b=b, metric=metric)


def end_variant(base, n_steps, jt, pt, trace_rows):
    """(case, want): the base placed at (n_steps, jt, pt, trace): the position buffer NOT chosen by n_steps & 1 is NaN, the rows of
    the draw block other than jt hold a log u that decides every chain the other way, the trace is NaN.  want: every array after the
    call except U (ref["U"] within the bound where accepted)."""
    C, n, ref = base["C"], base["n"], base["ref"]
    rng = np.random.default_rng([n, C, 3])
    lu_block = np.repeat(np.where(ref["ok"], 1e300, -1e300)[None], B_BLOCK, axis=0)
    lu_block[jt] = base["lu"]
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()
            if k in ("C", "n", "eps", "c_lik", "c_pri", "mean", "K", "U", "dU", "P", "dUq", "H0", "loss", "info", "accept")}
    case.update(Kq0=_nan(C, n), Kq1=_nan(C, n), P_block=rng.standard_normal((B_BLOCK, C, n)), lu_block=lu_block, jt=jt, pt=pt,
                trace=_nan(trace_rows, C, n) if trace_rows else None)
    case["Kq%d" % (n_steps & 1)] = base["Kq_end"].copy()
    want = {k: np.asarray(v).copy() for k, v in case.items() if k in dict(ARRAYS) and v is not None}
    want.update(K=ref["K"], dU=ref["dU"], accept=ref["accept"], jt=np.array(jt + 1), pt=np.array(pt + 1))
    if trace_rows:
        want["trace"][pt + 1] = ref["trace_row"]
    return case, want


def chain_subset(case, c):
    """Chain c of a case alone (C = 1)."""
    out = dict(case, C=1)
    for k, v in case.items():
        if isinstance(v, np.ndarray):
            out[k] = v[:, c:c + 1].copy() if k in ("P_block", "lu_block", "trace") else v[c:c + 1].copy()
    return out


# ---- device state ----------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


class DeviceState:
    """Every array of a finrom_hmc_state as a torch tensor on the GPU with PAD sentinel elements behind its end, filled from a case.
    `up[name]`: what was uploaded (flat, padding included); download() -> the same arrays now; `st`: the _ffi.HmcState."""

    def __init__(self, case):
        import ctypes
        import torch
        from bayesianinferencedl_amd import _ffi
        self._ffi, self._L, self.case = _ffi, _ffi.lib(), case
        self.up, self.t = {}, {}
        for name, dt in ARRAYS:
            if case[name] is None:
                continue
            pad = np.full(PAD, np.nan if dt is np.float64 else SENTINEL, dtype=dt)
            self.up[name] = np.concatenate([np.asarray(case[name], dtype=dt).reshape(-1), pad])
            self.t[name] = torch.from_numpy(self.up[name].copy()).cuda()
        p = {k: t.data_ptr() for k, t in self.t.items()}
        self.st = _ffi.HmcState(C=case["C"], n=case["n"], eps=case["eps"], c_lik=case["c_lik"], c_pri=case["c_pri"], mean=p["mean"],
                                K=p["K"], U=p["U"], dU=p["dU"], Kq=(ctypes.c_void_p * 2)(p["Kq0"], p["Kq1"]), P=p["P"], dUq=p["dUq"],
                                H0=p["H0"], P_block=p["P_block"], lu_block=p["lu_block"], jt=p["jt"], pt=p["pt"], accept=p["accept"],
                                trace=p.get("trace"), loss=p["loss"], info=p["info"])

    def call(self, name, *args):
        """finrom_<name>(&st, *args, stream) on torch's current stream -> the status."""
        import ctypes
        import torch
        return getattr(self._L, "finrom_" + name)(ctypes.byref(self.st), *args, torch.cuda.current_stream().cuda_stream)

    def download(self):
        import torch
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in self.t.items()}

    def body(self, arrays, name):
        """The array `name` of a download (or of `up`) without its padding, in the case's shape."""
        return arrays[name][:-PAD].reshape(np.shape(self.case[name]))

    def assert_bits(self, got, want, skip=()):
        """Every array of the download `got` outside `skip` has the bits of want[name] (an array without padding: the uploaded
        padding is put behind it), or of what was uploaded where want has no entry."""
        for name, _ in ARRAYS:
            if name in skip or name not in self.up:
                continue
            w = self.up[name] if name not in want else np.concatenate([np.asarray(want[name], dtype=self.up[name].dtype).reshape(-1),
                                                                       self.up[name][-PAD:]])
            if not same_bits(got[name], w):
                bad = np.flatnonzero((got[name].view(np.uint8).reshape(len(w), -1) != w.view(np.uint8).reshape(len(w), -1)).any(axis=1))
                raise AssertionError(f"{name}: {len(bad)} of {len(w)} elements differ (padding: the last {PAD}); first at {bad[:8]}: "
                                     f"got {got[name][bad[:4]]}, want {w[bad[:4]]}")
