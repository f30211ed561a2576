"""Shared cases of the No-U-turn transition (bayesian_inference/nuts.py, finrom_hmc_nuts_ml in csrc/hmc_nuts.hip; hmc.py nuts=):
tests/test_nuts_host.py on the CPU, tests/test_gpu_hmc_nuts.py on the device.  Imports without a GPU.

What is stated here:
  * the kernel's arithmetic for nuts.transition_iterative: `fma` (one rounding: libm's through ctypes where it agrees with
    hmc_cases.fma on a sample, else hmc_cases.fma itself -- the same bits, a tenth of the time) and `block_dot_1024`, a dot product in
    the order block_reduce.h documents for block_sum_1024 (thread t chains fused multiply-adds over i = t, t + 1024, ..., a butterfly
    inside each wave of 64, the 16 wave sums pairwise in index order);
  * MARGIN: every case here is chosen so that no comparison a transition makes is closer than this (a condition on the inputs);
  * a closed-form potential (an anisotropic Gaussian, n = 37, stiffness 0.5 .. 50) and the m = 4 surrogate in its float64 statement
    (hmc_ml_cases.misfit64), each with the (eps, max_depth) under which the host tests walk their chains;
  * a linear-Gaussian posterior with known moments;
  * the kernel tests' states: hmc_ml_cases.state_case with a potential and a gradient that belong to the position."""
import ctypes
import ctypes.util

import numpy as np

import hmc_cases as H
import hmc_ml_cases as MC
import surrogate_cases as SC

MARGIN = 1e-6
THREADS = 1024


def _libm_fma():
    try:
        f = ctypes.CDLL(ctypes.util.find_library("m")).fma
        f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double] * 3
        u = np.frompyfunc(f, 3, 1)
        g = np.random.default_rng(0).standard_normal
        a, x, y = g(64) * 1e3, g(64), g(64) * 1e-3
        y[:8] = -(a[:8] * x[:8])                                     # cancellation: where one rounding and two differ
        fast = lambda a, x, y: np.asarray(u(a, x, y), dtype=np.float64)
        return fast if H.same_bits(fast(a, x, y), H.fma(a, x, y)) else None
    except Exception:
        return None


_FAST = _libm_fma()


def fma(a, x, y):
    """round(a * x + y) with ONE rounding, elementwise: hmc_cases.fma's bits."""
    a, x, y = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, x, y)))
    if _FAST is None or not (np.isfinite(a).all() and np.isfinite(x).all() and np.isfinite(y).all()):
        return H.fma(a, x, y)
    return _FAST(a, x, y).reshape(a.shape)


def block_dot_1024(a, b):
    """sum_i a_i b_i in double in block_sum_1024's order."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.zeros(THREADS)
    for i0 in range(0, len(a), THREADS):
        m = len(a[i0:i0 + THREADS])
        s[:m] = fma(a[i0:i0 + THREADS], b[i0:i0 + THREADS], s[:m])
    lanes = np.arange(THREADS)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[lanes ^ off]
    r = s[::64]
    while len(r) > 1:
        r = r[0::2] + r[1::2]
    return float(r[0])


# ---- host cases --------------------------------------------------------------------------------------------------------------------------
TOY_N = 37
TOY_STIFF = np.logspace(np.log10(0.5), np.log10(50.0), TOY_N)
TOY_RUNS = ((0.05, 5), (0.12, 7), (0.3, 4))       # (eps, max_depth)
TOY_CHAINS, TOY_TRANSITIONS, TOY_SEED0 = 4, 12, 100


def toy_value_and_grad(K):
    K = np.asarray(K, dtype=np.float64)
    return 0.5 * np.sum(TOY_STIFF * K * K, axis=1), TOY_STIFF * K, np.zeros(len(K), bool)


def toy_starts():
    g = np.random.default_rng(0)
    return np.stack([g.standard_normal(TOY_N) / np.sqrt(TOY_STIFF) for _ in range(TOY_CHAINS)])


SUR_RUNS = ((0.12, 4), (0.3, 3))                  # the m = 4 surrogate under the i.i.d. prior of the chain tests
SUR_TRANSITIONS = 3


def surrogate_value_and_grad():
    model = SC.hmc_model()
    data = SC.hmc_data(model)

    def f(K):
        loss, grad = MC.misfit64(model, K, data)
        return loss, grad, ~np.isfinite(loss)
    return f


def state_at(value_and_grad, K, mean, c_lik, c_pri):
    """(U [C], dU [C, n] = grad U / c_pri, loss [C]) of the chain states K, in the conventions of the statement."""
    loss, grad, bad = value_and_grad(K)
    assert not np.any(bad)
    d = K - mean
    return c_lik * loss + 0.5 * c_pri * np.einsum("cn,cn->c", d, d), (c_lik / c_pri) * grad + d, np.asarray(loss, dtype=np.float64)


def walk(transition, value_and_grad, K0, mean, c_lik, c_pri, eps, max_depth, seeds, transitions, **kw):
    """`transitions` transitions of every chain with the momenta of philox.draw_block -> the list of results, chain-major."""
    from bayesianinferencedl_amd.bayesian_inference import philox
    K = np.array(K0, dtype=np.float64)
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), K.shape)
    U, dU, loss = state_at(value_and_grad, K, mean, c_lik, c_pri)
    out = []
    for c in range(len(K)):
        k, u, du, ls = K[c], U[c], dU[c], loss[c]
        for q in range(transitions):
            r = transition(value_and_grad, k, u, du, ls, philox.momentum(seeds[c], q, K.shape[1]), seed=seeds[c], proposal=q, eps=eps,
                           c_lik=c_lik, c_pri=c_pri, mean=mean[c], max_depth=max_depth, **kw)
            out.append(r)
            k, u, du, ls = r.k, r.U, r.dU, r.loss
    return out


# ---- a linear-Gaussian posterior ---------------------------------------------------------------------------------------------------------
LG_N, LG_OBS, LG_SIGMA, LG_TAU = 6, 4, 0.5, 1.0
LG_CHAINS, LG_TRANSITIONS, LG_BURN, LG_BATCH, LG_DEPTH = 8, 1200, 50, 25, 2


def linear_gaussian():
    """loss = 1/2 |y - A k|^2 under N(0, tau^2): -> (value_and_grad, posterior mean [n], posterior variance [n], eps).  eps: 1.975
    standard deviations of the stiffest direction, just inside the leapfrog's stability limit of 2: the energy error is large there, so
    the leaves' weights differ and a selection that ignores them shows in the variance."""
    g = np.random.default_rng(21)
    A, y = g.standard_normal((LG_OBS, LG_N)), g.standard_normal(LG_OBS)
    cov = np.linalg.inv(A.T @ A / LG_SIGMA ** 2 + np.eye(LG_N) / LG_TAU ** 2)

    def f(K):
        r = np.asarray(K, dtype=np.float64) @ A.T - y
        return 0.5 * np.sum(r * r, axis=1), r @ A, np.zeros(len(r), bool)
    return f, cov @ (A.T @ y) / LG_SIGMA ** 2, np.diag(cov).copy(), 1.975 * np.sqrt(np.linalg.eigvalsh(cov)[0])


# ---- kernel cases ------------------------------------------------------------------------------------------------------------------------
# (shape, C, eps, max_depth, proposal0, which chains the statement is evaluated for: None = all).  Every shape runs with C = 1, 4 and
# 80.  The statement costs a second per thousand elements and leaf, so an eighty-chain case restates three chains on the host; the
# test then compares EVERY one of the eighty with the same chain run alone on the device (C = 1), on the raw bytes.
KERNEL_CASES = (
    (MC.SHAPES[0], 1, 0.05, 4, 0, None), (MC.SHAPES[0], 4, 0.5, 4, 0, None), (MC.SHAPES[0], 80, 0.2, 3, 1 << 40, (0, 41, 79)),
    (MC.SHAPES[1], 1, 0.05, 4, 0, None), (MC.SHAPES[1], 4, 0.2, 4, 0, None), (MC.SHAPES[1], 4, 0.3, 4, 0, None),
    (MC.SHAPES[1], 80, 0.08, 2, 2, (0, 41, 79)),
    (MC.SHAPES[2], 1, 0.02, 3, 0, None), (MC.SHAPES[2], 4, 0.2, 4, 0, None), (MC.SHAPES[2], 80, 0.12, 2, 6, (0, 41, 79)),
    (MC.SHAPES[3], 1, 0.01, 3, 0, None), (MC.SHAPES[3], 4, 0.2, 4, 0, None), (MC.SHAPES[3], 80, 0.08, 2, 13, (0, 41, 79)),
)
KERNEL_SEEDS0 = 7000


def kernel_state(shape, C, eps, seed=0):
    """hmc_ml_cases.state_case as the state BEFORE a transition: the position in K, both Kq buffers NaN (the kernel writes Kq[0]).
    U, dU and loss do not yet belong to K: see with_potential."""
    s = MC.state_case(shape, C, eps=eps, seed=seed)
    s["Kq0"] = np.full_like(s["K"], np.nan)
    return s


def with_potential(s, loss, grad):
    """The case with the potential, the gradient / c_pri and the misfit of its position K, in the kernel's arithmetic."""
    d = s["K"] - s["mean"]
    dd = np.array([block_dot_1024(r, r) for r in d])
    return dict(s, loss=np.asarray(loss, dtype=np.float64).copy(), U=fma(s["c_lik"], loss, 0.5 * s["c_pri"] * dd),
                dU=fma(s["c_lik"] / s["c_pri"], grad, d))
