"""Reference and case builder for delayed-acceptance HMC (hmc.py correct=; finrom_hmc_end_stage1 / _stage2, finrom_hmc_draw_stage2),
shared by tests/test_hmc_da_host.py, tests/test_gpu_hmc_da_kernels.py and tests/test_gpu_hmc_da.py.  Imports without a GPU.

  * toy(): a linear-Gaussian inverse problem with a deliberately wrong surrogate, whose full-order posterior is known in closed form;
  * ref_stage2(): include/finrom.h's statement of finrom_hmc_end_stage2 restated with hmc_cases.fma -- every operation of the
    second stage is reproducible to the bit, so the kernel's outputs are compared bit for bit;
  * stage2_case(): hand-made state in which chain c plays role c % 11 (ROLES);
  * DeviceDA: the arrays of a finrom_hmc_da on the GPU with hmc_cases' padding convention."""
import numpy as np

import hmc_cases as H

ROLES = ("ok1 & clear accept", "ok1 & clear reject", "ok1 & lu2 one ulp below D - Dq: accept", "ok1 & lu2 == D - Dq: reject (strict)",
         "ok1 = 0 with an lu2 that would accept", "ok1 & info_f = 3", "ok1 & a NaN in qoi_f", "ok1 & +inf in qoi_f",
         "ok1 & qoi_f = 1e200 (lossF overflows)", "ok1 = 0 & info_f flagged", "ok1 = 0 with Uq = +inf")
ROLE_ACCEPTS = (True, False, True, False) + (False,) * 7
ROLE_GOOD = (True,) * 5 + (False,) * 5 + (True,)
ROLE_OK1 = (1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0)
DA_ARRAYS = (("ok1", np.int32), ("Uq", np.float64), ("qoi_f", np.float64), ("info_f", np.int32), ("data", np.float64),
             ("lu2_block", np.float64), ("D", np.float64), ("loss_f", np.float64), ("accept1", np.int64), ("cand_loss_f", np.float64),
             ("correction", np.float64))


# ---- the linear-Gaussian toy -----------------------------------------------------------------------------------------------------
def toy():
    """n = 3 unknowns, 4 observations: full-order model A k against d, surrogate A' k against d' (15 % off and perturbed, data
    shifted by 0.3), sigma = 0.7, prior N(0, 1).  -> dict: the callables for run_chains (value_and_grad: the surrogate's; correct: the
    full-order misfit; qoi: A k), and the exact posterior mean and standard deviation under the full-order model."""
    rng = np.random.default_rng(5)
    A = rng.standard_normal((4, 3))
    d = rng.standard_normal(4) + 1
    As = 1.15 * A + 0.1 * rng.standard_normal((4, 3))
    ds = d + 0.3
    sigma, tau = 0.7, 1.0

    def value_and_grad(K):
        r = K @ As.T - ds
        return 0.5 * np.einsum("co,co->c", r, r), r @ As, np.zeros(len(K), bool)

    def correct(K):
        r = K @ A.T - d
        return 0.5 * np.einsum("co,co->c", r, r), np.zeros(len(K), bool)

    prec = A.T @ A / sigma ** 2 + np.eye(3) / tau ** 2
    cov = np.linalg.inv(prec)
    return dict(A=A, d=d, As=As, ds=ds, sigma=sigma, tau=tau, value_and_grad=value_and_grad, correct=correct,
                mean=cov @ (A.T @ d) / sigma ** 2, std=np.sqrt(np.diag(cov)))


# ---- the second stage, operation by operation ------------------------------------------------------------------------------------
def fom_misfit(qoi_f, data):
    """lossF [C]: s = 0; s = fma(r, r, s) over the observations in order, r = qoi_f - d; 0.5 s.  (A square that overflows is +inf,
    as the fused operation gives it; hmc_cases.fma takes finite results only.)"""
    qoi_f = np.asarray(qoi_f, dtype=np.float64)
    data = np.broadcast_to(np.asarray(data, dtype=np.float64), qoi_f.shape)
    s = np.zeros(len(qoi_f))
    with np.errstate(all="ignore"):
        for o in range(qoi_f.shape[1]):
            r = qoi_f[:, o] - data[:, o]
            plain = r * r + s
            fin = np.isfinite(plain)
            s = np.where(fin, H.fma(np.where(fin, r, 0.0), np.where(fin, r, 0.0), np.where(fin, s, 0.0)), plain)
        return 0.5 * s


def ref_stage2(s, a, n_steps):
    """finrom_hmc_end_stage2 on the state s (a case of hmc_cases) and the descriptor a (dict with the fields of finrom_hmc_da as
    NumPy arrays; correction None or [rows, C]) -> dict: ok, good, lossF, Dq and every array the call writes, afterwards: K, U, dU,
    accept, jt, pt, trace_row | D, loss_f, accept1, cand_loss_f, correction_row."""
    Kq = s["Kq%d" % (n_steps & 1)]
    jt = int(s["jt"])
    with np.errstate(all="ignore"):
        lossF = fom_misfit(a["qoi_f"], a["data"])
        Dq = s["c_lik"] * (lossF - s["loss"])
        good = (a["info_f"] == 0) & (np.abs(lossF) <= H.U_LIMIT) & np.isfinite(Dq)
        ok1 = a["ok1"] != 0
        ok = ok1 & good & (a["lu2_block"][jt] < a["D"] - Dq)
    K = np.where(ok[:, None], Kq, s["K"])
    return dict(ok=ok, good=good, lossF=lossF, Dq=Dq, K=K, U=np.where(ok, a["Uq"], s["U"]), dU=np.where(ok[:, None], s["dUq"], s["dU"]),
                accept=s["accept"] + ok, jt=jt + 1, pt=int(s["pt"]) + 1, trace_row=K.copy(), D=np.where(ok, Dq, a["D"]),
                loss_f=np.where(ok, lossF, a["loss_f"]), accept1=a["accept1"] + ok1, cand_loss_f=np.where(good, lossF, np.nan),
                correction_row=np.where(good, Dq, np.nan))


def stage2_case(n, C, n_obs, per_sample, n_steps, jt, pt, trace_rows, with_correction):
    """(state, descriptor, want): chain c plays role c % 11.  The position buffer NOT chosen by n_steps & 1 is NaN; the rows of the
    second draw block other than jt decide every chain the other way; the trace and the correction table are NaN.  want: every
    array of both after the call (arrays the call must leave alone are absent: their uploaded bits are the expectation)."""
    rng = np.random.default_rng([n, C, n_obs, int(per_sample), 7])
    g = rng.standard_normal
    nan = lambda *shape: np.full(shape, np.nan)
    role = np.arange(C) % 11
    s = dict(C=C, n=n, eps=H.EPS, c_lik=1.0 / 0.05 ** 2, c_pri=H.C_PRI, mean=1.0 + 0.1 * g((C, n)), K=1.0 + 0.3 * g((C, n)),
             U=50.0 * np.abs(g(C)), dU=3.0 * g((C, n)), Kq0=nan(C, n), Kq1=nan(C, n), P=g((C, n)), dUq=3.0 * g((C, n)), H0=g(C),
             P_block=g((H.B_BLOCK, C, n)), lu_block=-np.abs(g((H.B_BLOCK, C))), jt=jt, pt=pt, accept=10 + 3 * np.arange(C, dtype=np.int64),
             trace=nan(trace_rows, C, n) if trace_rows else None, loss=0.02 * np.abs(g(C)), info=np.zeros(C, np.int32))
    s["Kq%d" % (n_steps & 1)] = 1.0 + 0.3 * g((C, n))
    data = 1.0 + 0.1 * g((C, n_obs) if per_sample else (n_obs,))
    a = dict(n_obs=n_obs, data_per_sample=int(per_sample), ok1=np.array(ROLE_OK1, np.int32)[role], Uq=40.0 * np.abs(g(C)),
             qoi_f=np.broadcast_to(data, (C, n_obs)) + 0.05 * g((C, n_obs)), info_f=np.zeros(C, np.int32), data=data,
             lu2_block=np.zeros((H.B_BLOCK, C)), D=0.5 * g(C), loss_f=0.01 * np.abs(g(C)), accept1=5 + 2 * np.arange(C, dtype=np.int64),
             cand_loss_f=nan(C), correction=nan(H.TRACE_ROWS, C) if with_correction else None)
    a["info_f"][(role == 5) | (role == 9)] = 3
    a["qoi_f"][role == 6, n_obs // 2], a["qoi_f"][role == 7, n_obs - 1], a["qoi_f"][role == 8, 0] = np.nan, np.inf, 1e200
    a["Uq"][role == 10] = np.inf
    with np.errstate(all="ignore"):                                  # the threshold, in the kernel's own arithmetic: one subtraction
        thr = a["D"] - s["c_lik"] * (fom_misfit(a["qoi_f"], data) - s["loss"])
    lu2 = np.full(C, -1e300)                                         # (roles 5 .. 10: would accept any finite threshold)
    lu2[role == 0], lu2[role == 1], lu2[role == 4] = thr[role == 0] - 1.0, thr[role == 1] + 1.0, thr[role == 4] - 1.0
    lu2[role == 2], lu2[role == 3] = np.nextafter(thr[role == 2], -np.inf), thr[role == 3]
    a["lu2_block"][:] = np.where(np.array(ROLE_ACCEPTS)[role], 1e300, -1e300)[None]
    a["lu2_block"][jt] = lu2
    ref = ref_stage2(s, a, n_steps)
    assert np.array_equal(ref["ok"], np.array(ROLE_ACCEPTS)[role]) and np.array_equal(ref["good"], np.array(ROLE_GOOD)[role]), \
        "the reference does not decide the roles as they are defined"
    want = dict(K=ref["K"], U=ref["U"], dU=ref["dU"], accept=ref["accept"], jt=np.array(ref["jt"]), pt=np.array(ref["pt"]))
    if trace_rows:
        want["trace"] = s["trace"].copy()
        want["trace"][pt + 1] = ref["trace_row"]
    want_da = dict(D=ref["D"], loss_f=ref["loss_f"], accept1=ref["accept1"], cand_loss_f=ref["cand_loss_f"])
    if with_correction:
        want_da["correction"] = a["correction"].copy()
        want_da["correction"][pt + 1] = ref["correction_row"]
    return s, a, want, want_da, ref


# ---- device state ----------------------------------------------------------------------------------------------------------------
class DeviceDA:
    """The arrays of a finrom_hmc_da as torch tensors on the GPU, PAD sentinel elements behind each (hmc_cases.DeviceState's
    convention); `desc`: the _ffi.HmcDa.  assert_bits: every array has the bits of want[name], or its uploaded ones."""

    def __init__(self, a):
        import torch
        from bayesianinferencedl_amd import _ffi
        self.a, self.up, self.t = a, {}, {}
        for name, dt in DA_ARRAYS:
            if a[name] is None:
                continue
            pad = np.full(H.PAD, np.nan if dt is np.float64 else H.SENTINEL, dtype=dt)
            self.up[name] = np.concatenate([np.asarray(a[name], dtype=dt).reshape(-1), pad])
            self.t[name] = torch.from_numpy(self.up[name].copy()).cuda()
        p = {k: t.data_ptr() for k, t in self.t.items()}
        self.desc = _ffi.HmcDa(n_obs=a["n_obs"], data_per_sample=a["data_per_sample"], **p)

    def download(self):
        import torch
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in self.t.items()}

    def assert_bits(self, got, want):
        for name, _ in DA_ARRAYS:
            if name not in self.up:
                continue
            w = self.up[name] if name not in want else np.concatenate([np.asarray(want[name], dtype=self.up[name].dtype).reshape(-1),
                                                                       self.up[name][-H.PAD:]])
            if not H.same_bits(got[name], w):
                bad = np.flatnonzero((got[name].view(np.uint8).reshape(len(w), -1) != w.view(np.uint8).reshape(len(w), -1)).any(axis=1))
                raise AssertionError(f"{name}: {len(bad)} of {len(w)} elements differ (padding: the last {H.PAD}); first at {bad[:8]}: "
                                     f"got {got[name][bad[:4]]}, want {w[bad[:4]]}")
