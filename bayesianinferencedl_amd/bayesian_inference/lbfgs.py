"""Batched multi-start bound-constrained minimisation for MAP estimation: S starts advance in lockstep, each independent.

The reference minimises 0.5 |y(k) - d|^2 + reg(k) with SciPy's L-BFGS-B, one start after another
(bayesian_inference/estimate_MAP.py:246-281, ``options={'ftol': 1e-10, 'gtol': 1e-8}``).  This module has SciPy's option names,
defaults, stopping tests and messages, and one call of ``value_and_grad(X [S, d]) -> (f [S], g [S, d], bad [S])`` per ROUND for
all starts at once -- on the device a round is three launch groups (finrom_lbfgs_propose, the model, finrom_lbfgs_accept) that are
captured once and replayed.

The algorithm is a projected L-BFGS with Armijo backtracking along the projection arc, NOT Byrd, Lu, Nocedal and Zhu's
L-BFGS-B: there is no generalised Cauchy point, no subspace minimisation and no More-Thuente line search.  Per start, with
P = clip(., lo, hi):
  0. x = P(x0); f, g at x.  Flagged / not finite: status 3.  |P(x - g) - x|_inf <= gtol: status 0, nit = 0.
     A point is FLAGGED when the objective says so, when its value is NaN or +-inf, or when any component of its gradient is
     (after the library's terms: G^T and Tikhonov) -- a model's info != 0 means the same elsewhere in the library.  A value
     without a usable gradient is never accepted, so the stored g is always finite while a start runs.
  1. Free set: variables strictly inside the box, and those on a bound where -g points into the box (g < 0 at lo, g > 0 at hi);
     lo == hi is never free.  q = g on the free set, 0 elsewhere.
  2. d = -H q by the two-loop recursion over the stored pairs (newest first), H0 = (s^T y / y^T y) I from the newest pair, or I;
     d = 0 outside the free set.  If g^T d >= 0 (round-off only): drop the history, d = -q.
  3. alpha = min(1, 1 / |d|_2) with an empty history, else 1;  xt = P(x + alpha d), p = xt - x.
  4. Accept if xt is not flagged and f(xt) <= f + 1e-4 g^T p; else alpha *= clip(t*, 0.1, 0.5),
     t* = -g^T p / (2 (f(xt) - f - g^T p)) (0.1 if xt is flagged), same d.  After maxls rejected trials: drop a non-empty
     history and go to 1 (steepest descent); with an empty history, status 2.
  5. On accept: keep (s, y) = (p, g(xt) - g) in a ring of maxcor pairs if s^T y > eps y^T y; move; nit += 1.
  6. Status 0 when |P(x - g) - x|_inf <= gtol, or when f_old - f <= ftol max(|f_old|, |f|, 1) (SciPy's tests and messages);
     status 1 when nit >= maxiter or nfev >= maxfun.
Where the box is inactive near the solution this is the L-BFGS iteration SciPy runs there and converges to the same point; the
path in between differs (another line search), so nit / nfev differ from SciPy's.  (rom/error_optimization.py documents its own
departure from the reference's optimiser in the same way.)

Arithmetic: every dot product is summed in the device's fixed order (_rowdot: per-lane partial sums over 256 lanes, a butterfly
inside each 64-lane wave, then the four waves pairwise) and no step is contracted into a fused multiply-add, so minimize_host and
minimize_device take the same steps wherever the objective returns the same bits."""
from __future__ import annotations

import time
import warnings

import numpy as np

EPS = float(np.finfo(np.float64).eps)
RUNNING = -1
# the stop reasons the device keeps per start (workspace scalar 5) and SciPy's message for each
MESSAGES = {0: "CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL",
            1: "CONVERGENCE: RELATIVE REDUCTION OF F <= FACTR*EPSMCH",
            2: "STOP: TOTAL NO. OF ITERATIONS REACHED LIMIT",
            3: "STOP: TOTAL NO. OF F,G EVALUATIONS EXCEEDS LIMIT",
            4: "ABNORMAL_TERMINATION_IN_LNSRCH",
            5: "the start point is flagged, or its value or gradient is not finite"}
_STATUS_OF_REASON = {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 3}
_LANES, _WAVE = 256, 64


class MinimizeResult(dict):
    """scipy.optimize.OptimizeResult's fields, one entry per start: x [S, d], fun [S], jac [S, d], nit, nfev, status, success,
    message [S]; fhist [nit_max + 1, S] (f after each iteration, NaN past a start's stop) with keep_history."""
    __getattr__ = dict.__getitem__


def _rowdot(A, B):
    """Row-wise dot products of A, B [R, d] in the device's order (lbfgs_kernels.hip: block_sum_256 over lanes t = j mod 256)."""
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    R, d = A.shape
    nc = max(1, -(-d // _LANES))
    prod = np.zeros((R, nc * _LANES))
    prod[:, :d] = A * B
    prod = prod.reshape(R, nc, _LANES)
    s = prod[:, 0].copy()
    for i in range(1, nc):
        s = s + prod[:, i]
    v = s.reshape(R, _LANES // _WAVE, _WAVE)
    lane = np.arange(_WAVE)
    off = _WAVE // 2
    while off > 0:
        v = v + v[:, :, lane ^ off]
        off //= 2
    r = v[:, :, 0]
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])


def _dot(a, b):
    return float(_rowdot(a[None, :], b[None, :])[0])


def _clip(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def _box(bounds, d):
    """bounds: None, (lo, hi) with scalars / [d] arrays / None, or a scipy.optimize.Bounds -> lo, hi [d] (+-inf where open)."""
    if bounds is None:
        lo, hi = None, None
    elif hasattr(bounds, "lb"):
        lo, hi = bounds.lb, bounds.ub
    else:
        lo, hi = bounds
    lo = np.full(d, -np.inf) if lo is None else np.broadcast_to(np.asarray(lo, dtype=np.float64), (d,)).copy()
    hi = np.full(d, np.inf) if hi is None else np.broadcast_to(np.asarray(hi, dtype=np.float64), (d,)).copy()
    lo[np.isnan(lo)] = -np.inf
    hi[np.isnan(hi)] = np.inf
    if np.any(lo > hi):
        j = int(np.nonzero(lo > hi)[0][0])
        raise ValueError(f"bounds: lo > hi at component {j} ({lo[j]} > {hi[j]})")
    return lo, hi


def _check_options(maxcor, maxls):
    if not 1 <= int(maxcor) <= 16:
        raise ValueError(f"maxcor = {maxcor}: the device keeps 1 to 16 pairs")
    if int(maxls) < 1:
        raise ValueError(f"maxls = {maxls}: need at least one trial per direction")


def _result(x, f, g, nit, nfev, reason, fhist):
    status = np.array([_STATUS_OF_REASON[int(r)] for r in reason], dtype=np.int64)
    res = MinimizeResult(x=x, fun=f, jac=g, nit=np.asarray(nit, dtype=np.int64), nfev=np.asarray(nfev, dtype=np.int64),
                         status=status, success=status == 0, message=np.array([MESSAGES[int(r)] for r in reason], dtype=object))
    if fhist is not None:
        res["fhist"] = fhist[:int(res["nit"].max()) + 1]
    return res


def library_terms(X, f_in, g_in, gmap=None, tikhonov=None):
    """What finrom_lbfgs_accept adds to a model's value and gradient, in its order, on the host: g = G^T g_in (sums over the
    model's variables in order, from 0.0) and the Tikhonov term 0.5 gamma x^T K1 x (the row sums of K1 x in CSR order, the dot
    in _rowdot's) with gradient gamma K1 x.  X [S, d], f_in [S], g_in [S, gdim or d] -> f [S], g [S, d]."""
    import scipy.sparse as sp
    X = np.asarray(X, dtype=np.float64)
    f = np.array(f_in, dtype=np.float64).reshape(X.shape[0])
    g_in = np.asarray(g_in, dtype=np.float64)
    if gmap is not None:
        G = np.asarray(gmap.toarray() if sp.issparse(gmap) else gmap, dtype=np.float64)
        g = np.zeros(X.shape)
        for p in range(G.shape[0]):
            g = g + G[p][None, :] * g_in[:, p:p + 1]
    else:
        g = np.array(g_in, copy=True).reshape(X.shape)
    if tikhonov is not None:
        gamma, K1 = tikhonov
        K1 = sp.csr_matrix(K1)
        K1.sort_indices()
        ptr, idx, val = K1.indptr, K1.indices, K1.data
        cnt = np.diff(ptr)
        KX = np.zeros(X.shape)
        for t in range(int(cnt.max()) if cnt.size else 0):
            rows = np.nonzero(cnt > t)[0]
            q = ptr[rows] + t
            KX[:, rows] = KX[:, rows] + val[q][None, :] * X[:, idx[q]]
        f = f + 0.5 * gamma * _rowdot(X, KX)
        g = g + gamma * KX
    return f, g


class _Start:
    """The per-start state of minimize_host (the device keeps the same in finrom_lbfgs_state and its workspace)."""

    def __init__(self, m, d):
        self.s = np.zeros((m, d)); self.y = np.zeros((m, d)); self.sy = np.zeros(m); self.yy = np.zeros(m)
        self.k = 0; self.head = 0; self.nls = 0; self.alpha = 0.0; self.dir = np.zeros(d)
        self.phase = "new"; self.reason = None; self.nit = 0; self.nfev = 0


def _pgnorm(x, g, lo, hi):
    return float(np.max(np.abs(_clip(x - g, lo, hi) - x))) if x.size else 0.0


def _direction(st, x, g, lo, hi, m):
    """Steps 1-3: the stored direction and alpha of a new line search, and xt."""
    free = (lo < hi) & (((x > lo) & (x < hi)) | ((x <= lo) & (g < 0.0)) | ((x >= hi) & (g > 0.0)))
    q = np.where(free, g, 0.0)
    a = np.zeros(m)
    for i_ in range(st.k):                                   # newest first
        i = (st.head - 1 - i_) % m
        a[i] = (1.0 / st.sy[i]) * _dot(st.s[i], q)
        q = q - a[i] * st.y[i]
    if st.k > 0:
        nw = (st.head - 1) % m
        q = (st.sy[nw] / st.yy[nw]) * q
    for i_ in range(st.k - 1, -1, -1):                       # oldest first
        i = (st.head - 1 - i_) % m
        b = (1.0 / st.sy[i]) * _dot(st.y[i], q)
        q = q + st.s[i] * (a[i] - b)
    d = np.where(free, -q, 0.0)
    if not _dot(g, d) < 0.0:                                 # round-off: steepest descent on the free set
        st.k = 0
        d = np.where(free, -g, 0.0)
    alpha = 1.0
    if st.k == 0:
        with np.errstate(divide="ignore"):
            alpha = min(1.0, float(1.0 / np.sqrt(_dot(d, d))))
    st.dir, st.alpha, st.nls, st.phase = d, alpha, 0, "ls"


def _first(s, x, g, bad, lo, hi, gtol, maxiter, maxfun):
    """Step 0 for one start after the evaluation at x0 (bad: flagged, or a value or gradient component that is not finite)."""
    s.nfev = 1
    s.phase = "new"
    if bad:
        s.reason = 5
    elif _pgnorm(x, g, lo, hi) <= gtol:
        s.reason = 0
    elif s.nfev >= maxfun:
        s.reason = 3
    elif maxiter <= 0:
        s.reason = 2


def _accept(s, x, f, g, xt, ft, gt, bt, lo, hi, m, ftol, gtol, maxiter, maxfun, maxls):
    """Steps 4-6 for one running start with value ft, gradient gt and flag bt at its trial point xt: on acceptance x and g (rows,
    written in place) move and the pair goes to the ring; otherwise the step shrinks, the history is dropped or the start stops.
    -> (the start's value afterwards, whether it moved)."""
    s.nfev += 1
    p = xt - x
    gtp = _dot(g, p)
    flagged = bool(bt) or not np.isfinite(ft) or not bool(np.all(np.isfinite(gt)))
    if not flagged and ft <= f + 1e-4 * gtp:
        y = gt - g
        sy, yy = _dot(p, y), _dot(y, y)
        if sy > EPS * yy:
            s.s[s.head], s.y[s.head], s.sy[s.head], s.yy[s.head] = p, y, sy, yy
            s.head = (s.head + 1) % m
            s.k = min(s.k + 1, m)
        f_old = f
        x[:], g[:] = xt, gt
        f = float(ft)
        s.nit += 1
        s.phase = "new"
        if _pgnorm(x, g, lo, hi) <= gtol:
            s.reason = 0
        elif f_old - f <= ftol * max(abs(f_old), abs(f), 1.0):
            s.reason = 1
        elif s.nit >= maxiter:
            s.reason = 2
        elif s.nfev >= maxfun:
            s.reason = 3
        return f, True
    s.nls += 1
    if s.nls >= maxls:
        if s.k > 0:
            s.k, s.phase = 0, "new"
        else:
            s.reason = 4
    else:
        tq = 0.1
        if not flagged:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                tq = float(-gtp / (2.0 * (ft - f - gtp)))
        tq = (tq if tq < 0.5 else 0.5) if tq > 0.1 else 0.1      # (NaN: 0.1)
        s.alpha = s.alpha * tq
    if s.reason is None and s.nfev >= maxfun:
        s.reason = 3
    return f, False


def minimize_host(value_and_grad, X0, *, bounds=None, maxcor=10, ftol=2.220446049250313e-09, gtol=1e-5, maxiter=15000,
                  maxfun=15000, maxls=20, keep_history=False):
    """Minimise S independent starts X0 [S, d] in lockstep on the host (NumPy): the specification of minimize_device.
    value_and_grad(X [S, d]) -> (f [S], g [S, d], bad [S] bool), called once per round with the trial points of all starts
    (a stopped start's row is its final x).  bounds: None, (lo, hi) (scalars, [d] arrays or None) or scipy.optimize.Bounds.
    Returns a MinimizeResult (see the module docstring for the algorithm and its difference from SciPy's L-BFGS-B)."""
    _check_options(maxcor, maxls)
    X = np.array(X0, dtype=np.float64, copy=True, ndmin=2)
    S, d = X.shape
    lo, hi = _box(bounds, d)
    m = int(maxcor)
    X = _clip(X, lo, hi)
    st = [_Start(m, d) for _ in range(S)]
    f, G, bad = value_and_grad(X.copy())
    f = np.array(f, dtype=np.float64).reshape(S); G = np.array(G, dtype=np.float64).reshape(S, d)
    bad = np.asarray(bad, dtype=bool).reshape(S) | ~np.isfinite(f) | ~np.all(np.isfinite(G), axis=1)
    f = np.where(bad, np.inf, f)
    hist = [f.copy()] if keep_history else None
    for c in range(S):
        _first(st[c], X[c], G[c], bad[c], lo, hi, gtol, maxiter, maxfun)
    Xt = X.copy()
    while any(s.reason is None for s in st):
        for c in range(S):                                   # propose
            s = st[c]
            if s.reason is not None:
                Xt[c] = X[c]
                continue
            if s.phase == "new":
                _direction(s, X[c], G[c], lo, hi, m)
            Xt[c] = _clip(X[c] + s.alpha * s.dir, lo, hi)
        ft, Gt, bt = value_and_grad(Xt.copy())
        ft = np.array(ft, dtype=np.float64).reshape(S); Gt = np.array(Gt, dtype=np.float64).reshape(S, d)
        bt = np.asarray(bt, dtype=bool).reshape(S)
        row = np.full(S, np.nan) if keep_history else None
        for c in range(S):                                   # accept
            s = st[c]
            if s.reason is not None:
                continue
            f[c], moved = _accept(s, X[c], f[c], G[c], Xt[c], ft[c], Gt[c], bt[c], lo, hi, m, ftol, gtol, maxiter, maxfun, maxls)
            if moved and row is not None:
                row[c] = f[c]
        if keep_history and any(np.isfinite(row)):
            hist.append(row)
    fhist = None
    if keep_history:                                         # row i = f after iteration i of each start
        nit = np.array([s.nit for s in st])
        fhist = np.full((int(nit.max()) + 1, S), np.nan)
        fhist[0] = hist[0]
        it = np.zeros(S, np.int64)
        for row in hist[1:]:
            for c in np.nonzero(np.isfinite(row))[0]:
                it[c] += 1
                fhist[it[c], c] = row[c]
    return _result(X, f, G, [s.nit for s in st], [s.nfev for s in st], [s.reason for s in st], fhist)


def minimize_device(value_and_grad, X0, *, bounds=None, gmap=None, tikhonov=None, graph=True, block=16, maxcor=10,
                    ftol=2.220446049250313e-09, gtol=1e-5, maxiter=15000, maxfun=15000, maxls=20, keep_history=False):
    """minimize_host with the state on the current CUDA device (torch tensors) and the bookkeeping in the library
    (finrom_lbfgs_begin / _propose / _accept, include/finrom.h).  Same options, same result.

    value_and_grad(Xt) takes the trial points as a float64 CUDA tensor [S, d] (read it, do not keep it: the buffer is reused) and
    returns torch tensors on the same device: f [S], g [S, d] -- or [S, gdim] with gmap -- and bad [S] (bool or int; non-zero:
    flagged).  Any torch-defined objective works; the model's library calls run on torch's current stream.
    gmap: G [gdim x d] (gdim <= 16) when the model's gradient is in other variables theta = G x: the library forms G^T g.
    tikhonov: (gamma, K1) with K1 a [d x d] sparse matrix: the library adds 0.5 gamma x^T K1 x and its gradient gamma K1 x.
    graph: one round (propose, the model, accept) is captured in a torch.cuda.CUDAGraph after a warm-up round on a side stream and
    replayed; if the capture is refused, the rounds run in stream order (with a warning).  The host reads the status every `block`
    rounds and stops when no start is running."""
    import ctypes as C

    import scipy.sparse as sp
    import torch

    from .. import _ffi
    _check_options(maxcor, maxls)
    X0 = np.array(X0.detach().cpu().numpy() if hasattr(X0, "detach") else X0, dtype=np.float64, ndmin=2)
    S, d = X0.shape
    lo_np, hi_np = _box(bounds, d)                           # (lo > hi: ValueError before the device is touched)
    L = _ffi.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    f64 = dict(dtype=torch.float64, device=dev)
    m = int(maxcor)
    x = torch.as_tensor(X0, **f64).clone()
    xt, g = torch.empty_like(x), torch.zeros_like(x)
    f = torch.zeros(S, **f64)
    work = torch.zeros(_ffi.lbfgs_work_doubles(S, d, m), **f64)
    status = torch.full((S,), RUNNING, dtype=torch.int32, device=dev)
    nit, nfev = torch.zeros(S, dtype=torch.int64, device=dev), torch.zeros(S, dtype=torch.int64, device=dev)
    rows = min(int(maxiter), int(maxfun)) + 1
    fhist = torch.full((rows, S), float("nan"), **f64) if keep_history else None
    lo = torch.as_tensor(lo_np, **f64) if np.any(np.isfinite(lo_np)) else None
    hi = torch.as_tensor(hi_np, **f64) if np.any(np.isfinite(hi_np)) else None
    keep = [lo, hi]
    st = _ffi.LbfgsState(S=S, d=d, m=m, ftol=float(ftol), gtol=float(gtol), maxiter=int(maxiter), maxfun=int(maxfun),
                         maxls=int(maxls), lo=lo.data_ptr() if lo is not None else None, hi=hi.data_ptr() if hi is not None else None,
                         x=x.data_ptr(), f=f.data_ptr(), g=g.data_ptr(), xt=xt.data_ptr(), work=work.data_ptr(),
                         status=status.data_ptr(), nit=nit.data_ptr(), nfev=nfev.data_ptr(),
                         fhist=fhist.data_ptr() if fhist is not None else None, fhist_rows=rows if fhist is not None else 0)
    if gmap is not None:
        Gm = torch.as_tensor(np.ascontiguousarray(np.asarray(gmap.toarray() if sp.issparse(gmap) else gmap, dtype=np.float64)), **f64)
        if Gm.ndim != 2 or Gm.shape[1] != d:
            raise ValueError(f"gmap: need [gdim x {d}], got {tuple(Gm.shape)}")
        keep.append(Gm)
        st.G, st.gdim = Gm.data_ptr(), Gm.shape[0]
    if tikhonov is not None:
        gamma, K1 = tikhonov
        K1 = sp.csr_matrix(K1)
        K1.sort_indices()
        if K1.shape != (d, d):
            raise ValueError(f"tikhonov: K1 must be [{d} x {d}], got {K1.shape}")
        kp = torch.as_tensor(K1.indptr.astype(np.int32), device=dev)
        ki = torch.as_tensor(K1.indices.astype(np.int32), device=dev)
        kv = torch.as_tensor(K1.data.astype(np.float64), device=dev)
        keep += [kp, ki, kv]
        st.gamma, st.k1_ptr, st.k1_idx, st.k1_val = float(gamma), kp.data_ptr(), ki.data_ptr(), kv.data_ptr()

    def stream():
        return torch.cuda.current_stream().cuda_stream

    gdim = int(st.gdim) if st.G else d

    def evaluate():
        fv, gv, bv = value_and_grad(xt)
        fv = fv.to(torch.float64).contiguous(); gv = gv.to(torch.float64).contiguous()
        iv = torch.as_tensor(bv, device=dev).to(torch.int32).contiguous()
        if fv.numel() != S or tuple(gv.shape) != (S, gdim) or iv.numel() != S or not (fv.is_cuda and gv.is_cuda):
            raise ValueError(f"value_and_grad: need f [{S}], g [{S}, {gdim}] and bad [{S}] on the device, got "
                             f"{tuple(fv.shape)}, {tuple(gv.shape)}, {tuple(iv.shape)}")
        _ffi.check(L.finrom_lbfgs_accept(C.byref(st), fv.data_ptr(), gv.data_ptr(), iv.data_ptr(), stream()), "finrom_lbfgs_accept")

    def round_():
        _ffi.check(L.finrom_lbfgs_propose(C.byref(st), stream()), "finrom_lbfgs_propose")
        evaluate()

    _ffi.check(L.finrom_lbfgs_begin(C.byref(st), stream()), "finrom_lbfgs_begin")
    evaluate()                                               # f, g at x0 (also warms the model's library calls up)
    gr = None
    if graph:
        state = [x, xt, g, f, work, status, nit, nfev] + ([fhist] if fhist is not None else [])
        saved = [t.clone() for t in state]
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                    # warm-up on a side stream, as torch's graph recipe asks
                round_()
            torch.cuda.current_stream().wait_stream(side)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                round_()
        except Exception as exc:                             # no graph for this model's launches: stream order
            warnings.warn(f"lbfgs: HIP graph capture failed ({exc!r}); the rounds are launched in stream order")
            gr = None
        for t, t0 in zip(state, saved):                      # (the warm-up moved the state; the capture does not run)
            t.copy_(t0)
    B = max(1, int(block))
    rounds = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while bool((status == RUNNING).any()):
        for _ in range(B):
            gr.replay() if gr is not None else round_()
        rounds += B
    torch.cuda.synchronize()
    loop_s = time.perf_counter() - t0
    w = work.reshape(S, -1).cpu().numpy()
    reason = w[:, (2 * m + 1) * d + 2 * m + 5].astype(np.int64)
    out = _result(x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), nit.cpu().numpy(), nfev.cpu().numpy(), reason,
                  fhist.cpu().numpy() if fhist is not None else None)
    out["graph"] = gr is not None
    out["rounds"], out["loop_s"] = rounds, loop_s            # (rounds launched after the first evaluation, and their wall time)
    del keep
    return out
