"""The statement of tests/hmc_model_cases.py is only worth comparing the kernels against if it is itself right: here its drift and
kick, between hmc_cases.ref_begin and hmc_cases.ref_end, walk whole chains against hmc.run_chains (the host recursion) over a
synthetic model, in the three forms the device chains use them (a field-space gradient; the gradient through a map A; whitened
coordinates with A = Sop U^T); the two low-rank identities behind the whitened form are checked on the fin itself; and the
argument checks of the chain functions and of the two entry points that return before any device call.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import hmc_cases as H
import hmc_model_cases as M
from bayesianinferencedl_amd.bayesian_inference import hmc, philox

N, CHAINS, L, PROPOSALS = 37, 4, 5, 20
SEEDS = [11, 12, (1 << 40) + 13, 14]
SIGMA, TAU = 0.5, 0.7
EPS_IID, EPS_WHITENED = 0.15, 0.3       # step sizes at which every chain both accepts and rejects (asserted)


class _Prior:
    """What hmc.whitened_potential asks of a GaussianFieldPrior."""

    def __init__(self, U, mean):
        self.U, self.mean, self.n = U, mean, len(mean)

    def field(self, v):
        return self.mean + np.asarray(v, dtype=np.float64) @ self.U

    def pullback(self, g):
        return np.asarray(g, dtype=np.float64) @ self.U.T


def _factor(n, seed):
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((n, n))) / np.sqrt(np.arange(1, n + 1))[None, :]
    U[np.diag_indices(n)] = np.abs(U[np.diag_indices(n)]) + 0.5
    return 0.3 * U


def _statement_chains(model, form, X0, mean, eps, prior=None):
    """run_chains' recursion with the proposal opened by H.ref_begin and closed by H.ref_end and every leapfrog step M.ref_drift,
    the model, M.ref_kick -- the half steps folded as the device folds them.  form "grad": the model's field-space gradient;
    "map": theta from the drift with A = model.A, the kick's gradient A^T g_theta; "whitened": the same with A = model.A U^T and
    theta0 = model.A m in the coordinates v of k = m + U^T v (mean 0, c_pri 1).  -> (trace of the coordinates, accept)."""
    c_lik = 1.0 / SIGMA ** 2
    c_pri = 1.0 if form == "whitened" else 1.0 / TAU ** 2
    A, theta0 = None, None
    if form == "map":
        A = model.A
    elif form == "whitened":
        A, theta0 = model.A @ prior.U.T, model.A @ prior.mean
    loss, grad, bad = model(prior.field(X0) if form == "whitened" else X0)
    assert not bad.any()
    d = X0 - mean
    g0 = prior.pullback(grad) if form == "whitened" else grad
    s = dict(C=CHAINS, n=N, eps=eps, c_lik=c_lik, c_pri=c_pri, mean=mean, K=X0.copy(), U=c_lik * loss + 0.5 * c_pri * np.einsum("cn,cn->c", d, d),
             dU=d + (c_lik / c_pri) * g0, accept=np.zeros(CHAINS, np.int64), jt=0, pt=0)
    trace = [X0.copy()]
    info = np.zeros(CHAINS, np.int32)
    for j in range(PROPOSALS):
        s["P_block"], s["lu_block"] = philox.draw_block(philox.check_seeds(SEEDS), j, 1, N)
        s["jt"] = 0
        b = H.ref_begin(s)
        P, x = np.asarray(b["P"], dtype=np.float64), b["Kq0"]
        s["H0"] = b["H0"].astype(np.float64)
        for _ in range(L):
            x, theta, _ = M.ref_drift(x, P, eps, A, theta0)
            if A is None:
                loss, g, _ = model(x)
            else:
                th = theta.astype(np.float64)
                loss, g_theta = model.reduced(th)
                g = M.map_gradient(g_theta, A)[0].astype(np.float64)
            dUq, P = M.ref_kick(x, mean, P, info, eps, c_lik, c_pri, g)
        s.update(P=P, dUq=dUq, loss=loss, info=info)
        s["Kq%d" % (L & 1)], s["Kq%d" % (1 - (L & 1))] = x, np.full_like(x, np.nan)
        e = H.ref_end(s, L)
        s.update(K=e["K"], U=e["U"], dU=e["dU"], accept=e["accept"], pt=e["pt"])
        trace.append(e["trace_row"])
    return np.stack(trace), s["accept"]


@pytest.mark.parametrize("form", ["grad", "map", "whitened"])
def test_statement_steps_walk_the_host_chains(form):
    """rng="philox", C = 4, n = 37, 20 proposals of 5 steps over loss = |B A k - d|^2 / 2 (A [9 x n], B [9 x 9] random), at a step
    size at which chains both accept and reject: the accept counters of hmc.run_chains exactly, the trace (of fields) and the end
    points within 1e-12 relative -- the rounding of merging two half steps into one fused multiply-add, of theta through A U^T
    instead of through the field."""
    assert np.finfo(H.LD).nmant >= 63, "np.longdouble is no wider than double here: the statement has no extended precision"
    rng = np.random.default_rng(3)
    model = M.Quadratic(N)
    if form == "whitened":
        prior = _Prior(_factor(N, 9), 1.0 + 0.05 * rng.standard_normal(N))
        X0, mean, eps = 0.5 * rng.standard_normal((CHAINS, N)), np.zeros((CHAINS, N)), EPS_WHITENED
        want = hmc.run_chains(model, X0, 1 + PROPOSALS * L, seeds=SEEDS, eps=eps, n_leapfrog=L, sigma=SIGMA, keep_trace=True, prior=prior,
                              rng="philox")
    else:
        prior = None
        X0 = 1.0 + 0.2 * rng.standard_normal((CHAINS, N))
        mean, eps = np.broadcast_to(1.0 + 0.05 * rng.standard_normal(N), X0.shape).copy(), EPS_IID
        want = hmc.run_chains(model, X0, 1 + PROPOSALS * L, seeds=SEEDS, eps=eps, n_leapfrog=L, sigma=SIGMA, tau=TAU, mean=mean,
                              keep_trace=True, rng="philox")
    assert want.proposals == PROPOSALS
    trace, accept = _statement_chains(model, form, X0, mean, eps, prior)
    print(form, "accepted", want.accept, "of", PROPOSALS)
    assert 0 < want.accept.sum() < CHAINS * PROPOSALS and np.all(want.accept > 0) and np.all(want.accept < PROPOSALS)
    assert np.array_equal(accept, want.accept)
    fields = prior.field(trace) if prior is not None else trace
    err = np.max(np.abs(fields - want.trace)) / np.max(np.abs(want.trace))
    end = want.V if prior is not None else want.K
    err_end = np.max(np.abs(trace[-1] - end)) / np.max(np.abs(end))
    print(form, "trace difference", err, "end points", err_end)
    assert err <= 1e-12 and err_end <= 1e-12


def test_a_flagged_chain_keeps_its_momentum_and_a_nan_reaches_the_others():
    """The kick's statement: info 2 and -1 give dUq = 0 and the momentum's bits; a NaN in an unflagged chain's gradient reaches
    its dUq and momentum at that node alone."""
    s = M.step_case(65, 3, 0, flags=((1, 2), (2, -1)))
    kq, _, _ = M.ref_drift(s["Kq0"], s["P"], s["eps"])
    g = M.map_case(65, 3, 9)[3]
    g[0, 7] = np.nan
    dU, P = M.ref_kick(kq, s["mean"], s["P"], s["info"], s["eps"], s["c_lik"], s["c_pri"], g)
    assert not dU[1:].any() and H.same_bits(P[1:], s["P"][1:])
    assert np.flatnonzero(np.isnan(dU[0])).tolist() == [7] and np.flatnonzero(np.isnan(P[0])).tolist() == [7]
    want = (kq[0] - s["mean"][0]) + (s["c_lik"] / s["c_pri"]) * g[0]
    ok = np.arange(65) != 7
    assert np.max(np.abs(dU[0, ok] - want[ok])) <= 4 * H.U53 * np.max(np.abs(want[ok]))


def test_the_two_low_rank_identities_on_the_fin(spaces):
    """m = 4 (n = 245), GaussianFieldPrior(V, amplitude=0.1, mean=1.0), Sop = V.operators().S, W = Sop U^T: the sub-fin averages of
    the field k = m + U^T v are Sop m + W v, and the whitened gradient U Sop^T g_theta of a function of theta is W^T g_theta --
    each within 1e-13 relative (the two sides sum in different orders; measured 2e-16 and 1.2e-15)."""
    from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
    V = spaces(4)
    prior = GaussianFieldPrior(V, amplitude=0.1, mean=1.0)
    Sop = np.asarray(V.operators().S)
    assert Sop.shape == (9, 245) and prior.U.shape == (245, 245)
    W = Sop @ prior.U.T
    rng = np.random.default_rng(2)
    v, g_theta = rng.standard_normal((4, 245)), rng.standard_normal((4, 9))
    theta, theta_w = prior.field(v) @ Sop.T, Sop @ prior.mean + v @ W.T
    e1 = np.max(np.abs(theta - theta_w)) / np.max(np.abs(theta))
    gv, gv_w = prior.pullback(g_theta @ Sop), g_theta @ W
    e2 = np.max(np.abs(gv - gv_w)) / np.max(np.abs(gv))
    print("theta", e1, "gradient", e2)
    assert e1 <= 1e-13 and e2 <= 1e-13


def test_chain_functions_refuse_wrong_model_arguments():
    """model="fom" without solver= or without data=, an unknown model, solver= beside another model, a reduced model without a
    solver: ValueError before anything touches the device."""
    K0 = np.ones((2, 5))
    kw = dict(seeds=[1, 2])
    for f in (hmc.run_chains_device, hmc.run_chains_fused):
        with pytest.raises(ValueError, match="needs solver=Fin"):
            f(None, K0, 11, model="fom", data=np.zeros(9), **kw)
        with pytest.raises(ValueError, match="needs data="):
            f(None, K0, 11, model="fom", solver=object(), **kw)
        with pytest.raises(ValueError, match="unknown model 'pod'"):
            f(None, K0, 11, model="pod", **kw)
        with pytest.raises(ValueError, match="solver= belongs to model='fom'"):
            f(object(), K0, 11, model="rom", solver=object(), data=np.zeros(9), **kw)
        with pytest.raises(ValueError, match="needs solver_r"):
            f(None, K0, 11, model="rom", data=np.zeros(9), **kw)
    assert callable(hmc.fom_value_and_grad(object(), np.zeros(9))) and callable(hmc.rom_value_and_grad(object()))


def _host_state(n=8, C_=2, c_pri=1.0):
    """A finrom_hmc_state whose pointers are all non-null HOST addresses: good for checks that return before any device call."""
    buf = np.zeros(64)
    p = buf.ctypes.data
    from bayesianinferencedl_amd import _ffi
    st = _ffi.HmcState(C=C_, n=n, eps=0.1, c_lik=1.0, c_pri=c_pri, mean=p, K=p, U=p, dU=p, Kq=(C.c_void_p * 2)(p, p), P=p, dUq=p, H0=p,
                       P_block=p, lu_block=p, jt=p, pt=p, accept=p, trace=None, loss=p, info=p)
    return st, buf


def test_drift_and_kick_check_their_arguments_before_any_device_call():
    """A null state, step < 0, P = 0 and P = 17 with a map, a map without theta_out, both or neither of grad and g_theta, g_theta
    without A, c_pri = 0: FINROM_ERR_ARG with a message and the (host) buffers untouched.  The fused steps refuse null handles."""
    from bayesianinferencedl_amd import _ffi
    lib = _ffi.lib()
    st, buf = _host_state()
    p = buf.ctypes.data
    err = lib.finrom_last_error
    assert lib.finrom_hmc_drift(None, 0, None, None, 0, None, None) == -1 and b"hmc_drift: null field" in err()
    assert lib.finrom_hmc_drift(C.byref(st), -1, None, None, 0, None, None) == -1 and b"hmc_drift: step < 0" in err()
    for P in (0, 17, -3):
        assert lib.finrom_hmc_drift(C.byref(st), 0, p, None, P, p, None) == -1 and b"hmc_drift: P = %d is outside 1 .. 16" % P in err()
        assert lib.finrom_hmc_kick(C.byref(st), 0, None, p, p, P, None, None) == -1 and b"hmc_kick: P = %d is outside 1 .. 16" % P in err()
    assert lib.finrom_hmc_drift(C.byref(st), 0, p, p, 9, None, None) == -1 and b"hmc_drift: A without theta_out" in err()
    assert lib.finrom_hmc_kick(None, 0, p, None, None, 0, None, None) == -1 and b"hmc_kick: null field" in err()
    assert lib.finrom_hmc_kick(C.byref(st), -1, p, None, None, 0, None, None) == -1 and b"hmc_kick: step < 0" in err()
    assert lib.finrom_hmc_kick(C.byref(st), 0, p, p, p, 9, None, None) == -1 and b"exactly one of grad and g_theta" in err()
    assert lib.finrom_hmc_kick(C.byref(st), 0, None, None, p, 9, None, None) == -1 and b"exactly one of grad and g_theta" in err()
    assert lib.finrom_hmc_kick(C.byref(st), 0, None, p, None, 9, None, None) == -1 and b"hmc_kick: g_theta without A" in err()
    st0, _ = _host_state(c_pri=0.0)
    assert lib.finrom_hmc_kick(C.byref(st0), 0, p, None, None, 0, None, None) == -1 and b"hmc_kick: c_pri = 0" in err()
    assert lib.finrom_hmc_leapfrog_fom(None, C.byref(st), 0, p, 0, None, None, None) == -1 and b"hmc_leapfrog_fom: null fom" in err()
    assert lib.finrom_hmc_leapfrog_field_fom(None, None, None, p, p, C.byref(st), 0, p, 0, None, None) == -1 and b"hmc_leapfrog_field_fom: null prior" in err()
    assert lib.finrom_hmc_leapfrog_rom(None, p, None, C.byref(st), 0, p, 0, p, p, None, None, None) == -1 and b"hmc_leapfrog_rom: null rom" in err()
    assert not buf.any()
