"""CPU tests of the batched multi-start minimiser's specification (bayesian_inference/lbfgs.py: minimize_host) against SciPy's
L-BFGS-B, its edge semantics, and the host-side checks of the finrom_lbfgs_* entry points (no GPU: nothing reaches a device)."""
import ctypes as C

import numpy as np
import pytest
from scipy.optimize import minimize

from bayesianinferencedl_amd.bayesian_inference import lbfgs


def _quadratic(d=50, seed=0):
    """A strictly convex quadratic with cond(A) = 1e3 built from its bounded minimiser x*: a third of x* on the box, with
    gradients g* that point out of it there (strict complementarity) and zero elsewhere.  f(x) = 0.5 e^T A e + g*^T e, e = x - x*,
    is evaluated in that form, so that f is small near x* and its decrease resolves x to 1e-8.  -> (fun, x*, lo, hi)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    A = (Q * np.logspace(0, 3, d)) @ Q.T
    A = 0.5 * (A + A.T)
    xs = rng.uniform(-1.0, 1.0, d)
    lo, hi = xs - rng.uniform(0.5, 1.5, d), xs + rng.uniform(0.5, 1.5, d)
    gs = np.zeros(d)
    for j in rng.permutation(d)[: d // 3]:
        if rng.uniform() < 0.5:
            lo[j] = xs[j]; gs[j] = rng.uniform(1.0, 10.0)
        else:
            hi[j] = xs[j]; gs[j] = -rng.uniform(1.0, 10.0)

    def fun(x):
        e = x - xs
        Ae = A @ e
        return 0.5 * (e @ Ae) + gs @ e, Ae + gs
    return fun, xs, lo, hi


def _batched(fun):
    def f(X):
        vals = [fun(x) for x in np.asarray(X)]
        return np.array([v[0] for v in vals]), np.stack([v[1] for v in vals]), np.zeros(len(vals), bool)
    return f


def _rosen(x):
    f = np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2)
    g = np.zeros_like(x)
    g[:-1] = -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2.0 * (1.0 - x[:-1])
    g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
    return f, g


def test_quadratic_with_active_bounds_matches_scipy():
    fun, xs, lo, hi = _quadratic()
    x0 = np.zeros(len(xs))
    ref = minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                   options=dict(ftol=0.0, gtol=1e-11, maxiter=20000, maxfun=20000))
    res = lbfgs.minimize_host(_batched(fun), x0[None], bounds=(lo, hi), ftol=0.0, gtol=1e-11, maxiter=20000, maxfun=20000)
    x = res.x[0]
    act_ref = (ref.x == lo) | (ref.x == hi)
    act = (x == lo) | (x == hi)
    assert act_ref.sum() == len(xs) // 3                     # a third of the solution is on the box
    assert np.array_equal(act, act_ref)
    assert np.linalg.norm(ref.x - xs) <= 1e-8 * np.linalg.norm(xs)
    assert np.linalg.norm(x - ref.x) <= 1e-8 * np.linalg.norm(ref.x)
    assert res.status[0] == 0 and res.success[0]


def test_bounded_rosenbrock_matches_scipy():
    d = 10
    lo, hi = np.full(d, -1.5), np.full(d, 0.8)               # the unconstrained minimiser (1, ..., 1) is outside
    x0 = np.full(d, -0.5)
    ref = minimize(_rosen, x0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                   options=dict(ftol=1e-15, gtol=1e-11, maxiter=20000, maxfun=20000))
    res = lbfgs.minimize_host(_batched(_rosen), x0[None], bounds=(lo, hi), ftol=1e-15, gtol=1e-11, maxiter=20000, maxfun=20000)
    assert np.any(np.abs(ref.x - hi) < 1e-12)
    assert np.linalg.norm(res.x[0] - ref.x) <= 1e-6 * np.linalg.norm(ref.x)
    assert res.status[0] == 0


def test_infeasible_start_is_projected_and_fixed_components_never_move():
    fun, _, _, _ = _quadratic(d=12, seed=3)
    lo, hi = np.full(12, -0.5), np.full(12, 0.5)
    lo[[2, 7]] = hi[[2, 7]] = [0.25, -0.1]                   # fixed components
    seen = []

    def f(X):
        seen.append(np.array(X, copy=True))
        return _batched(fun)(X)
    x0 = np.linspace(-3.0, 3.0, 12)
    res = lbfgs.minimize_host(f, x0[None], bounds=(lo, hi), gtol=1e-9)
    assert np.array_equal(seen[0][0], np.clip(x0, lo, hi))
    for X in seen:
        assert np.all(X >= lo) and np.all(X <= hi)
        assert X[0, 2] == 0.25 and X[0, 7] == -0.1
    assert res.x[0, 2] == 0.25 and res.x[0, 7] == -0.1 and res.status[0] == 0


def test_iteration_limit_gives_status_1():
    res = lbfgs.minimize_host(_batched(_rosen), np.full((1, 6), -1.0), maxiter=3)
    assert res.status[0] == 1 and res.nit[0] == 3 and not res.success[0]
    assert "ITERATIONS" in res.message[0]


def test_infinite_trials_end_the_line_search_with_status_2():
    calls = []

    def f(X):
        calls.append(1)
        x = np.asarray(X)[0]
        if len(calls) == 1:
            return np.array([x @ x]), (2.0 * x)[None], np.zeros(1, bool)
        return np.array([np.inf]), np.zeros_like(X), np.zeros(1, bool)
    res = lbfgs.minimize_host(f, np.ones((1, 4)), maxls=7)
    assert res.status[0] == 2 and res.nit[0] == 0
    assert res.nfev[0] == 1 + 7 and len(calls) == 1 + 7
    assert res.message[0] == "ABNORMAL_TERMINATION_IN_LNSRCH"


def test_flagged_start_gives_status_3():
    def f(X):
        X = np.asarray(X)
        return np.sum(X * X, 1), 2.0 * X, np.array([False, True])
    res = lbfgs.minimize_host(f, np.ones((2, 3)), gtol=1e-10)
    assert res.status[1] == 3 and res.nfev[1] == 1 and res.nit[1] == 0 and np.isinf(res.fun[1])
    assert res.status[0] == 0


def test_starts_in_one_call_equal_each_start_alone_bit_for_bit():
    rng = np.random.default_rng(5)
    X0 = rng.uniform(-1.2, 1.2, (5, 8))
    bounds = (-1.0, 0.9)
    batch = lbfgs.minimize_host(_batched(_rosen), X0, bounds=bounds, keep_history=True)
    for i in range(5):
        one = lbfgs.minimize_host(_batched(_rosen), X0[i:i + 1], bounds=bounds, keep_history=True)
        assert np.array_equal(one.x[0], batch.x[i]) and one.fun[0] == batch.fun[i]
        assert one.nit[0] == batch.nit[i] and one.nfev[0] == batch.nfev[i] and one.status[0] == batch.status[i]
        n = one.nit[0] + 1
        assert np.array_equal(one.fhist[:n, 0], batch.fhist[:n, i])
        assert np.all(np.isnan(batch.fhist[n:, i]))


def test_rowdot_is_the_device_summation_order():
    """_rowdot restates block_sum_256 over lanes t = j mod 256: per-lane running sums, a butterfly inside each wave of 64, the
    four waves pairwise.  Exact on integers, and the same bits for a row whatever the other rows are."""
    rng = np.random.default_rng(1)
    a = rng.integers(-50, 50, (3, 1597)).astype(float)
    assert np.array_equal(lbfgs._rowdot(a, a), np.einsum("sd,sd->s", a, a))
    x = rng.standard_normal((4, 700))
    assert np.array_equal(lbfgs._rowdot(x, x)[2:3], lbfgs._rowdot(x[2:3], x[2:3]))


def test_lower_above_upper_bound_raises():
    with pytest.raises(ValueError, match="lo > hi"):
        lbfgs.minimize_host(_batched(_rosen), np.zeros((1, 3)), bounds=(np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.5, 1.0])))
    with pytest.raises(ValueError, match="lo > hi"):                # before any device is touched
        lbfgs.minimize_device(None, np.zeros((1, 3)), bounds=(1.0, 0.0))


def test_lbfgs_entry_points_validate_their_state_before_any_device_call():
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()

    def state(**kw):
        base = dict(S=4, d=10, m=5, ftol=1e-9, gtol=1e-5, maxiter=10, maxfun=10, maxls=20)
        base.update(kw)
        return _ffi.LbfgsState(**base)
    for fn in (L.finrom_lbfgs_begin, L.finrom_lbfgs_propose):
        assert fn(C.byref(state(S=0)), None) == -1 and b"S = 0" in L.finrom_last_error()
        assert fn(C.byref(state(m=0)), None) == -1 and b"m = 0" in L.finrom_last_error()
        assert fn(C.byref(state(m=17)), None) == -1 and b"m = 17" in L.finrom_last_error()
        assert fn(C.byref(state(d=0)), None) == -1 and b"d = 0" in L.finrom_last_error()
        assert fn(C.byref(state()), None) == -1 and b"null x" in L.finrom_last_error()
        assert fn(C.byref(state(gdim=3)), None) == -1 and b"gdim" in L.finrom_last_error()
        assert fn(None, None) == -1 and b"null state" in L.finrom_last_error()
    assert L.finrom_lbfgs_accept(C.byref(state(S=-1)), None, None, None, None) == -1 and b"S = -1" in L.finrom_last_error()
    assert L.finrom_lbfgs_accept(C.byref(state()), None, None, None, None) == -1 and b"null x" in L.finrom_last_error()
    assert L.finrom_deferred_count() == 0


# ---- the cases of tests/test_gpu_lbfgs_kernels.py: each takes, on the host alone, the branch it is named for ----------------------
import lbfgs_cases as K  # noqa: E402


def test_lbfgs_e_is_restated_from_the_kernel_source_and_the_ladder_covers_every_form():
    import os
    import re
    src = open(os.path.join(os.path.dirname(lbfgs.__file__), "..", "csrc", "lbfgs_kernels.hip")).read()
    assert re.search(r"n <= 1 \? 1 : n <= 2 \? 2 : n <= 4 \? 4 : n <= 8 \? 8 : n <= LBFGS_MAX_E \? LBFGS_MAX_E : 0", src)
    hdr = open(os.path.join(os.path.dirname(lbfgs.__file__), "..", "csrc", "finrom_internal.h")).read()
    assert re.search(r"LBFGS_MAX_E\s*=\s*17\b", hdr)
    assert [K.lbfgs_e(d) for d in (1, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4352, 4353)] == [1, 1, 2, 2, 4, 4, 8, 8, 17, 17, 0]
    assert [K.lbfgs_e(d) for d in K.FORM_D] == list(K.FORMS)
    for e in K.FORMS:
        ds = [d for d in K.LADDER if K.lbfgs_e(d) == e]
        assert len(ds) >= 2 and (ds[0] == 1 or K.lbfgs_e(ds[0] - 1) != e) and K.lbfgs_e(ds[-1] + 1) != e, (e, ds)   # both ends of the form


@pytest.mark.parametrize("d", K.LADDER)
def test_ladder_cases_iterate(d):
    res, tr = K.ladder_case(d).check()
    assert np.all(res.nit >= 3) and tr["accepted"] == res.nit.sum()
    if d >= 255:
        assert tr["wrapped"] > 0 and np.all(res.nit == 24)


@pytest.mark.parametrize("d,maxcor,mode", K.OPTION_GRID)
def test_option_cases_wrap_the_ring_and_backtrack(d, maxcor, mode):
    res, tr = K.option_case(d, maxcor, mode).check()
    lo, hi = lbfgs._box(K.option_case(d, maxcor, mode).kw["bounds"], d)
    assert np.all(res.x >= lo) and np.all(res.x <= hi)
    if mode == "both":                                       # starts outside the box, fixed components, active bounds at the end
        assert np.any(K.option_case(d, maxcor, mode).X0 > hi) and np.any(lo == hi) and np.any((res.x == lo) | (res.x == hi))


@pytest.mark.parametrize("d", K.FORM_D)
def test_batch_case_runs_past_three_rings(d):
    K.batch_case(d, S=8).check()


@pytest.mark.parametrize("which", K.TERMS)
@pytest.mark.parametrize("d", K.FORM_D)
def test_library_terms_cases_iterate(d, which):
    case = K.terms_case(d, which)
    res, tr = case.check()
    assert (case.gmap is None or case.gmap.shape == ({"gmap1": 1, "gmap9": 9, "gmap16": 16, "both": 9}[which], d))
    assert (case.tikhonov is not None) == (which in ("tikhonov", "both"))


@pytest.mark.parametrize("name,d", K.STOP_GRID)
def test_stop_cases_end_for_the_reason_they_are_named_for(name, d):
    K.stop_case(name, d).check()


def test_every_stop_reason_has_a_case():
    seen = set()
    for name in K.STOPS:
        seen |= set(K._reasons(K.stop_case(name).host()))
    assert seen == {0, 1, 2, 3, 4, 5}


def test_a_finite_value_with_a_gradient_that_is_not_finite_is_flagged():
    """The decision of step 0 / step 4: status 3 at x0 (the device used to stop with status 0 and a NaN in jac when every other
    component was within gtol, the host ran on), a rejected trial later (never a NaN in the stored gradient or the history)."""
    res = K.stop_case("gnan_at_rest").host()
    assert res.status[0] == 3 and res.nit[0] == 0 and res.nfev[0] == 1 and "gradient" in res.message[0]
    for kind in ("gnan", "ginf"):
        res, tr = K.stop_case(kind).traced()
        assert tr["flagged"] > 10 and np.all(np.isfinite(res.jac[1:])) and np.all(np.isfinite(res.fhist[0, 1:]))


# ---- the kernels' resources, read from the build: registers without scratch ------------------------------------------------------
def test_lbfgs_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """All eleven kernels of csrc/lbfgs_kernels.hip, compiled for gfx950 with _build.py's flags: no private segment (scratch) and
    no spilled VGPR -- the register forms are sized so that a start's vectors stay in registers up to d = 4352."""
    import os
    import re
    import subprocess
    from bayesianinferencedl_amd import _build
    try:
        hipcc = _build._hipcc()
        subprocess.run([hipcc, "--version"], capture_output=True, check=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError) as exc:
        pytest.skip(f"hipcc not found ({exc})")
    asm = tmp_path / "lbfgs_kernels.s"
    src = os.path.join(_build.CSRC, "lbfgs_kernels.hip")
    r = subprocess.run([hipcc, *_build.FLAGS, _build.OPT.get("lbfgs_kernels.hip", "-O3"), "--cuda-device-only", "-S", src, "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = asm.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for blk in re.split(r"\n  - (?=\.)", meta)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", blk, flags=re.M)
        if name is None:
            continue
        kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s*(\d+)", blk, flags=re.M)}
    want = [r"lbfgs_begin_kernel"] + [rf"lbfgs_{k}_kernelILi{e}E" for k in ("propose", "accept") for e in K.FORMS]
    assert len(kernels) == len(want) == 11, sorted(kernels)
    for pat in want:
        hit = [n for n in kernels if re.search(pat, n)]
        assert len(hit) == 1, (pat, sorted(kernels))
        res = kernels[hit[0]]
        print(f"{pat:32s} VGPRs {res['vgpr_count']:3d}  SGPRs {res['sgpr_count']:3d} ({res['sgpr_spill_count']} kept in VGPR lanes)  "
              f"scratch {res['private_segment_fixed_size']}")
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (pat, res)


def test_d_above_4352_is_unsupported_by_all_three_entry_points():
    """The size check comes after the null-pointer checks: the state carries non-null pointers (nothing is dereferenced: the call
    returns before any device call).  d = 4352 passes the checks and runs: tests/test_gpu_lbfgs_kernels.py."""
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    ptrs = dict(x=p, f=p, g=p, xt=p, work=p, status=p, nit=p, nfev=p)
    st = _ffi.LbfgsState(S=1, d=4353, m=5, ftol=1e-9, gtol=1e-5, maxiter=10, maxfun=10, maxls=20, **ptrs)
    unsupported = -4                                         # FINROM_ERR_UNSUPPORTED (include/finrom.h)
    for call in (lambda: L.finrom_lbfgs_begin(C.byref(st), None), lambda: L.finrom_lbfgs_propose(C.byref(st), None),
                 lambda: L.finrom_lbfgs_accept(C.byref(st), p, p, None, None)):
        assert call() == unsupported and b"4352" in L.finrom_last_error() and b"d = 4353" in L.finrom_last_error()
    assert L.finrom_deferred_count() == 0
