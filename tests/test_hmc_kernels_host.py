"""The reference of tests/hmc_cases.py is only worth comparing the kernels against if it is itself right: here it walks whole chains
against hmc.run_chains (the host recursion), the summation bound of tests/test_gpu_hmc_kernels.py is checked against exact
arithmetic, and the host-side argument checks of the four entry points that tests/test_host_and_abi.py does not reach.  No GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import hmc_cases as H
from bayesianinferencedl_amd.bayesian_inference import hmc, philox
from bayesianinferencedl_amd.bayesian_inference.laplace import LowRankMetric

N, CHAINS, L, PROPOSALS = 37, 4, 5, 20
SEEDS = [11, 12, (1 << 40) + 13, 14]
SIGMA, TAU = 0.5, 0.7


def _quadratic(bad_at=()):
    """value_and_grad of loss(k) = |A k - y|^2 / 2 (closed-form gradient A^T (A k - y)); chain 2 is flagged `bad` (NaN loss and
    gradient) on the evaluations listed in bad_at.  The counter restarts with every new function."""
    rng = np.random.default_rng(5)
    A, y = rng.standard_normal((9, N)), rng.standard_normal(9)
    calls = [0]

    def f(K):
        r = K @ A.T - y
        loss, grad, bad = 0.5 * np.einsum("co,co->c", r, r), r @ A, np.zeros(len(K), bool)
        if calls[0] in bad_at:
            loss, grad = loss.copy(), grad.copy()
            loss[2], grad[2], bad[2] = np.nan, np.nan, True
        calls[0] += 1
        return loss, grad, bad
    return f


def _reference_chains(f, K0, mean, eps, metric=None):
    """run_chains' recursion with the proposal opened by H.ref_begin and closed by H.ref_end (the statements of finrom_hmc_begin /
    _end, under a metric _begin_metric / _end_metric), the leapfrog steps between them in NumPy as include/finrom.h states them:
    k <- k + eps p (M^-1 p), dU = (k - mean) + (c_lik / c_pri) grad (0 for a flagged sample), p <- p - eps c_pri dU.
    -> (trace [PROPOSALS + 1, C, n], accept [C])."""
    c_lik, c_pri = 1.0 / SIGMA ** 2, 1.0 / TAU ** 2
    pair = None if metric is None else (metric.Vt, metric.lam)
    loss, grad, bad = f(K0)
    assert not bad.any()
    d = K0 - mean
    s = dict(C=CHAINS, n=N, eps=eps, c_lik=c_lik, c_pri=c_pri, mean=mean, K=K0.copy(), U=c_lik * loss + 0.5 * c_pri * np.einsum("cn,cn->c", d, d),
             dU=d + (c_lik / c_pri) * grad, accept=np.zeros(CHAINS, np.int64), jt=0, pt=0)
    trace = [K0.copy()]
    for j in range(PROPOSALS):
        s["P_block"], s["lu_block"] = philox.draw_block(philox.check_seeds(SEEDS), j, 1, N)
        s["jt"] = 0
        b = H.ref_begin(s, pair)
        P, Kq, dUq = np.asarray(b["P"], dtype=np.float64), b["Kq0"], b["dUq"]
        s["H0"] = b["H0"].astype(np.float64)
        for _ in range(L):
            Kq = Kq + eps * (P if metric is None else metric.apply(P, "inv"))
            loss, grad, bad = f(Kq)
            dUq = np.where(bad[:, None], 0.0, (Kq - mean) + (c_lik / c_pri) * grad)
            P = P - eps * c_pri * dUq
        s.update(P=P, dUq=dUq, loss=loss, info=bad.astype(np.int32))
        s["Kq%d" % (L & 1)], s["Kq%d" % (1 - (L & 1))] = Kq, np.full_like(Kq, np.nan)
        e = H.ref_end(s, L, pair)
        s.update(K=e["K"], U=e["U"], dU=e["dU"], accept=e["accept"])
        assert e["pt"] == j + 1 and e["jt"] == 1
        s["pt"] = e["pt"]
        trace.append(e["trace_row"])
    return np.stack(trace), s["accept"]


@pytest.mark.parametrize("form", ["plain", "flagged", "metric"])
def test_reference_begin_and_end_walk_the_host_chains(form):
    """rng="philox", C = 4, n = 37, 20 proposals of 5 steps, eps at which chains both accept and reject: the trace within 1e-12
    relative of run_chains', the accept counters exactly.  "flagged": chain 2's evaluation is bad at the end points of proposals 1
    and 6 (and once in the middle of a trajectory, which only removes that step's force): those proposals are rejected and the trace
    row repeats.  "metric": under a LowRankMetric of rank 3."""
    assert np.finfo(H.LD).nmant >= 63, "np.longdouble is no wider than double here: the reference has no extended precision"
    rng = np.random.default_rng(3)
    K0 = 1.0 + 0.2 * rng.standard_normal((CHAINS, N))
    mean = np.broadcast_to(1.0 + 0.05 * rng.standard_normal(N), K0.shape).copy()
    metric, eps = None, 0.12
    if form == "metric":
        metric, eps = LowRankMetric(np.linalg.qr(rng.standard_normal((N, 3)))[0].T, np.array([0.5, 20.0, 300.0])), 0.12
    bad_at = (2 * L, 4 * L + 2, 7 * L) if form == "flagged" else ()
    want = hmc.run_chains(_quadratic(bad_at), K0, 1 + PROPOSALS * L, seeds=SEEDS, eps=eps, n_leapfrog=L, sigma=SIGMA, tau=TAU, mean=mean,
                          keep_trace=True, metric=metric, rng="philox")
    assert want.proposals == PROPOSALS
    trace, accept = _reference_chains(_quadratic(bad_at), K0, mean, eps, metric)
    print(form, "accepted", want.accept, "of", PROPOSALS)
    assert 0 < want.accept.sum() < CHAINS * PROPOSALS and np.all(want.accept > 0) and np.all(want.accept < PROPOSALS)
    assert np.array_equal(accept, want.accept)
    err = np.max(np.abs(trace - want.trace)) / np.max(np.abs(want.trace))
    print(form, "trace difference", err)
    assert err <= 1e-12
    if form == "flagged":
        for j in (1, 6):
            assert np.array_equal(trace[j + 1, 2], trace[j, 2]) and np.array_equal(want.trace[j + 1, 2], want.trace[j, 2])


def test_the_role_table_is_what_the_reference_decides():
    """The twelve roles of the end cases, plain and under a metric: the reference accepts roles 1 and 3 (one-based) and rejects the
    rest (end_base asserts it); the near roles sit 64 bounds from the difference, the clear ones 1 away, on the stated side."""
    for n, rho in ((65, 0), (257, 0), (65, 9)):
        base = H.end_base(n, 12, rho)
        ref, b, lu = base["ref"], base["b"], base["lu"].astype(H.LD)
        assert list(ref["ok"]) == list(H.ROLE_ACCEPTS)
        assert np.all(b[:4] > 0) and np.all(np.isfinite(b[:4]))
        gap = (lu - ref["diff"]).astype(np.float64)
        assert abs(gap[0] + 1) < 1e-9 and abs(gap[1] - 1) < 1e-9
        assert -65 * b[2] < gap[2] < -63 * b[2] and 63 * b[3] < gap[3] < 65 * b[3]
        assert np.all(b[:4] < 1e-8), "a near case further than 1e-8 from its threshold is no near case"


def test_summation_bound_holds_for_the_documented_order():
    """sum p_i^2 in the order of block_sum_256 behind a thread's chain of fused multiply-adds (H.block_sum_256_emulated) against
    exact arithmetic: within (ceil(n / 256) + 12) 2^-53 of the exact sum, n in 1, 63, 64, 65, 255, 256, 257, 511, 1597, 20 rows
    each, |p| spread over six decades."""
    rng = np.random.default_rng(8)
    worst = 0.0
    for n in (1, 63, 64, 65, 255, 256, 257, 511, 1597):
        for _ in range(20):
            p = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
            exact = sum(Fraction(v) ** 2 for v in p.tolist())
            err = abs(Fraction(H.block_sum_256_emulated(p)) - exact)
            bound = Fraction(H.sum_tol(n)) * exact                   # (the terms are positive: the scale is the sum)
            assert err <= bound, (n, float(err / bound))
            worst = max(worst, float(err / bound))
    print("worst error / bound", worst)


def test_fma_is_one_rounding():
    """H.fma against cases where two roundings differ from one, and with non-finite operands."""
    a, x = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30                        # a x = 1 - 2^-60 exactly
    assert H.fma(a, x, -1.0) == -2.0 ** -60 and a * x - 1.0 == 0.0
    assert H.fma(0.1, 10.0, -1.0) == 2.0 ** -54
    out = H.fma(np.array([np.nan, np.inf, 2.0]), 3.0, np.array([1.0, 1.0, np.inf]))
    assert np.isnan(out[0]) and out[1] == np.inf and out[2] == np.inf


def _host_state(n=8, C_=2):
    """A finrom_hmc_state whose pointers are all non-null HOST addresses: good for checks that return before any device call."""
    buf = np.zeros(64)
    p = buf.ctypes.data
    from bayesianinferencedl_amd import _ffi
    st = _ffi.HmcState(C=C_, n=n, eps=0.1, c_lik=1.0, c_pri=1.0, mean=p, K=p, U=p, dU=p, Kq=(C.c_void_p * 2)(p, p), P=p, dUq=p, H0=p,
                       P_block=p, lu_block=p, jt=p, pt=p, accept=p, trace=None, loss=p, info=p)
    return st, buf


def test_entry_points_refuse_a_null_metric_and_negative_steps_before_any_device_call():
    """finrom_hmc_begin_metric / _end_metric with a null metric handle, finrom_hmc_end with n_steps < 0: FINROM_ERR_ARG with a
    message, and the (host) buffers the state points to untouched.  (A metric whose n differs from the state's, and _end_metric's
    n_steps < 0 behind a valid handle, need a handle, which only a GPU can hold: tests/test_gpu_hmc_kernels.py.)"""
    from bayesianinferencedl_amd import _ffi
    lib = _ffi.lib()
    st, buf = _host_state()
    assert lib.finrom_hmc_begin_metric(C.byref(st), None, None) == -1 and b"hmc_begin_metric: null metric" in lib.finrom_last_error()
    assert lib.finrom_hmc_end_metric(C.byref(st), None, 3, None) == -1 and b"hmc_end_metric: null metric" in lib.finrom_last_error()
    assert lib.finrom_hmc_end_metric(C.byref(st), None, -1, None) == -1
    assert lib.finrom_hmc_end(C.byref(st), -1, None) == -1 and b"hmc_end: n_steps < 0" in lib.finrom_last_error()
    assert not buf.any()
