"""The full-order solve (finrom_fom_solve), its adjoint gradient (finrom_fom_gradient), general right-hand sides on the stored factor
(finrom_fom_solve_rhs), the Hessian action and the sensitivity built on them, on the device against the extended-precision
yardstick of tests/fom_ld_cases.py, path by path as csrc/api_fom.hip dispatches them.

Allowance, per case and per quantity (w, qoi, J, grad, out, H u, the Jacobian rows): d_host = the largest relative deviation of
host64 (plain fp64 SuperLU and SciPy products) from the yardstick over the checked samples; the device must be within
max(8 d_host, 1e-12), and under 1e-10.  Device and host are two fp64 factorisations of one matrix in different elimination orders.
8 d_host <= 1e-10 is a condition on the inputs, held on the host by tests/test_fom_ld_host.py for exactly these cases, with the
controls that must fail.  EVERY sample of every batch is checked; grad and H u also in the entrywise norm (largest entry error over
the largest entry).  Batches are S = 70 (one full block of 64 lanes plus 6 live lanes) unless a test says otherwise.

Every case asserts which kernel ran (finrom_fom_last_path) and moves the small-batch threshold where it is about a throughput
kernel.  The inputs of the yardstick are the handle's own: c0, W, F and B_obs are compared bit for bit when a handle is made.
Every test prints its measured device and host deviations and records them in its docstring."""
import numpy as np
import pytest

import fom_ld_cases as Y

pytestmark = pytest.mark.gpu
BAND_PATH = {4: "band_registers", 8: "band_registers", 12: "band_registers", 16: "band_lds_4wave", 20: "band_lds_4wave",
             24: "band_lds_4wave", 28: "band_lds_4wave"}
HALF_PLAN_M = (4, 8, 12)                                     # the meshes the library has the half plan's window sizes for
S = Y.S_BATCH


@pytest.fixture(scope="module")
def handles(spaces):
    """(Fin, FomEngine, Case) per (m, kind, band plan or not, observations), made once; the yardstick's inputs are the handle's."""
    import bayesianinferencedl_amd.engine as E
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    fins = {}

    def get(m, kind, band=True, external_obs=False):
        c = Y.case(m, kind, external_obs)
        old = E.USE_BAND
        try:
            E.USE_BAND = band
            if (m, band, external_obs) not in fins:
                fins[(m, band, external_obs)] = Fin(spaces(m), external_obs=external_obs)
            fin = fins[(m, band, external_obs)]
            eng = fin._engine(kind)
        finally:
            E.USE_BAND = old
        assert (eng.band is not None) == band
        inp = c.inp
        assert (eng._W != inp.W).nnz == 0 and np.array_equal(fin.ops.robin_vals, inp.c0) and np.array_equal(fin.ops.F, inp.F)
        assert np.array_equal(np.asarray(fin.B_obs), inp.B)
        assert np.array_equal(fin.ops.indptr, inp.indptr) and np.array_equal(fin.ops.indices, inp.indices)
        return fin, eng, c
    return get


def _small(eng, on):
    """The small-batch schedule at its default threshold, or out of the way."""
    import bayesianinferencedl_amd.engine as E
    in_lds = (eng.plan.nnzL + 3 * eng.plan.n + eng.xdim) * 8 <= 156 * 1024
    eng.set_small_max((E.SMALL_MAX if in_lds else E.SMALL_MAX_GLOBAL) if on else 0)


def _check(label, c, out, samples, quantities, per_sample=None, what=None):
    info = out.get("info") if isinstance(out, dict) else None
    assert info is None or not np.asarray(info).any(), label
    assert Y.report(label, c.against(out, samples, quantities, per_sample, what)), label


def _params(kind):
    return None if kind == "field" else kind


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Y.KINDS)
@pytest.mark.parametrize("m", Y.FORWARD_M)
def test_forward_band_sweep(handles, m, kind):
    """finrom_fom_solve on the band sweep, with w and QoI-only: the front in registers (m = 4, 8, 12: fom_band_kernel), the post's
    window over four waves (m = 16, 24: fom_band_ldsw_kernel; at m = 24 extras' rows in the workspace); QoI-only calls take the
    functional form of the fins, and for five fin conductivities at m <= 12 the half plan of the mirror-symmetric operator
    (finrom_fom_band_mirror_form != 0; the library has no half-plan windows beyond m = 12: 0 there, the full plan's QoI-only form).
    Measured (device / host64, the largest over the 70 samples; w and qoi alike to within 20 %): qoi, field: m = 4 1.8e-14 / 1.1e-14,
    m = 8 4.7e-14 / 2.0e-14, m = 12 7.9e-14 / 2.7e-14, m = 16 1.4e-13 / 7.0e-14, m = 24 2.8e-13 / 7.0e-14 (factor 4.0, the largest of the
    forward solve); nine: 7.5e-14 / 5.5e-14, 3.1e-13 / 2.0e-13, 4.1e-13 / 2.7e-13, 1.4e-12 / 9.1e-13, 1.6e-12 / 7.0e-13; five: 8.3e-14 /
    5.0e-14, 3.2e-13 / 2.2e-13, 5.9e-13 / 2.8e-13, 9.7e-13 / 5.6e-13, 2.2e-12 / 6.3e-13.  QoI-only returns the same figures except on
    the half plan (five, m = 4: 1.1e-13, m = 8: 4.8e-13, m = 12: 5.8e-13)."""
    from bayesianinferencedl_amd._ffi import lib
    fin, eng, c = handles(m, kind)
    res = fin.forward_batch(c.X[:S], want_w=True, params=_params(kind))
    assert eng.last_path() == BAND_PATH[m]
    _check(f"forward, band sweep, m = {m}, {kind}, with w", c, res, range(S), ("w", "qoi"))
    res_q = fin.forward_batch(c.X[:S], want_w=False, params=_params(kind))
    assert eng.last_path() == BAND_PATH[m] + "_qoi" and res_q["w"] is None
    if kind == "five":
        form = int(lib().finrom_fom_band_mirror_form(eng._h))
        assert (form != 0) == (m in HALF_PLAN_M), form
    _check(f"forward, band sweep, m = {m}, {kind}, QoI-only", c, res_q, range(S), ("qoi",))


@pytest.mark.parametrize("m,small,path", [(4, False, "interpreter"), (12, True, "small_lds"), (16, True, "small_global")])
def test_forward_without_a_band_plan(handles, m, small, path):
    """finrom_fom_solve on a handle made without a band plan (USE_BAND = False): the schedule interpreter (small-batch schedule
    out of the way), and the small-batch kernel with the value vector in LDS (m = 12) and in the workspace (m = 16); nine fin
    conductivities, with w and QoI-only.
    Measured (qoi, device / host64): interpreter m = 4 7.5e-14 / 5.5e-14; small_lds m = 12 3.7e-13 / 2.7e-13; small_global m = 16
    1.5e-12 / 9.1e-13; w the same to the digits shown."""
    fin, eng, c = handles(m, "nine", band=False)
    _small(eng, small)
    for want_w in (True, False):
        res = fin.forward_batch(c.X[:S], want_w=want_w, params="nine")
        assert eng.last_path() == path
        _check(f"forward, {path}, m = {m}, want_w = {want_w}", c, res, range(S), ("w", "qoi") if want_w else ("qoi",))


# ---- adjoint gradient ------------------------------------------------------------------------------------------------------------
def _check_gradient(label, fin, eng, c, kind, path, n=S):
    """grad, J and the returned qoi of every sample, with shared and with per-sample data."""
    for per_sample, data in ((False, c.data), (True, c.D[:n])):
        res = fin.gradient_batch(c.X[:n], data, params=_params(kind))
        assert eng.last_path() == path, eng.last_path()
        _check(f"{label}, {'per-sample' if per_sample else 'shared'} data", c, res, range(n), ("grad", "grad_max", "J", "qoi"), per_sample)


@pytest.mark.parametrize("kind", Y.KINDS)
@pytest.mark.parametrize("m", Y.ADJOINT_M)
def test_gradient_band_adjoint(handles, m, kind):
    """finrom_fom_gradient beyond the small-batch schedule (threshold moved to 0): the full band sweep leaves the factor and w in the
    workspace, fom_band_adjoint_kernel solves the adjoint on the stored columns and contracts the gradient -- every built window
    size: <3,6,4> (m = 4) and <4,10,4> (m = 8), which no other test runs, <5,14,4>, <6,18,8>, <7,22,8>, <8,26,10>, <9,30,12>.
    This test found the one defect of the set: the contraction dealt a parameter's triples alternately to two accumulators.  A
    parameter's triples come row by row of A, and a row's terms v_a sum_b dA_ab/dx_j w_b cancel; for a fin conductivity the whole sum
    cancels by five to six digits.  Dealt to two sums, each half grows to the size of the terms and the digits go in g0 + g1:
    m = 12, five conductivities, per-sample data measured grad 2.13e-11 against host64's 1.67e-12 (12.8 x; entrywise 2.64e-11 /
    2.00e-12), shared data 9.6e-12 / 1.3e-12 (7.4 x), nine 3.0e-12 / 5.8e-13 (5.2 x); the fp64 NumPy sum of the EXACT v, w in that
    order gives 1.6e-11, in table order 1.5e-12.  The kernel (and fom_adjoint_kernel, which did the same) now keeps one accumulator
    in table order.
    Measured since (device / host64, the larger of shared and per-sample data; grad in the 2-norm, entrywise within 1.4 x of it):
      field  m = 4 3.7e-14 / 2.6e-14, 8: 9.0e-14 / 7.4e-14, 12: 1.5e-13 / 1.5e-13, 16: 3.4e-13 / 2.7e-13, 20: 5.8e-13 / 6.3e-13,
             24: 6.2e-13 / 6.6e-13, 28: 1.0e-12 / 1.1e-12
      nine   1.9e-13 / 2.6e-13, 6.4e-13 / 1.6e-12, 6.1e-13 / 7.8e-13, 2.0e-12 / 4.5e-12, 1.5e-12 / 3.4e-12, 2.3e-12 / 1.3e-12, 3.5e-12 / 5.8e-12
      five   1.7e-13 / 3.6e-13, 1.1e-12 / 2.1e-12, 2.7e-12 / 1.7e-12, 1.5e-12 / 3.5e-12, 2.8e-12 / 3.9e-12, 1.0e-11 / 5.2e-12, 4.4e-12 / 4.3e-12
    J: 9.6e-15 .. 4.4e-12, device / host64 at most 4.6 where the allowance is above its floor; at m = 28, field, per-sample data
    4.2e-13 / 4.5e-14 (9.2 x, under the floor of 1e-12: J carries the returned qoi's 3.6e-13 / 7.9e-14).  qoi as in the forward solve."""
    fin, eng, c = handles(m, kind)
    _small(eng, False)
    _check_gradient(f"gradient, band adjoint, m = {m}, {kind}", fin, eng, c, kind, BAND_PATH[m])


def test_gradient_band_adjoint_with_forty_observations(handles):
    """The band adjoint with the 40 point observations of external_obs=True (m = 12, nine fin conductivities): 40 residual rows in
    LDS, B_obs^T with several rows per dof.
    Measured (device / host64): grad 9.2e-13 / 8.8e-13 (entrywise 1.7e-12 / 1.0e-12), J 3.8e-13 / 2.7e-13, qoi 4.0e-13 / 2.8e-13."""
    fin, eng, c = handles(12, "nine", external_obs=True)
    assert fin.n_obs == 40 and c.inp.B.shape[0] == 40
    _small(eng, False)
    _check_gradient("gradient, band adjoint, m = 12, nine, 40 observations", fin, eng, c, "nine", BAND_PATH[12])


@pytest.mark.parametrize("m,kind,path", [(4, "field", "small_lds"), (12, "field", "small_lds"), (16, "field", "small_global"),
                                         (12, "five", "small_lds")])
def test_gradient_small_batch_kernel(handles, m, kind, path):
    """finrom_fom_gradient at the default threshold: value and gradient in one workgroup per sample (fom_small_kernel), the value
    vector in LDS (m = 4, 12) and in the workspace (m = 16), nodal fields; and five fin conductivities at m = 12, where a
    parameter's 1100 .. 3200 triples cancel by five digits and the kernel deals them to 16 lanes.
    Measured (grad, device / host64): field m = 4 3.1e-14 / 2.6e-14, m = 12 2.4e-13 / 1.5e-13, m = 16 4.3e-13 / 2.7e-13; five, m = 12:
    3.5e-12 / 1.3e-12 (2.7 x; entrywise 5.0e-12 / 1.8e-12) -- sixteen strided partial sums cost a factor 3 to 4 over one sum in
    table order (the NumPy sum of the exact v, w in that order: 6.4e-12 at worst), within the margin."""
    fin, eng, c = handles(m, kind)
    _small(eng, True)
    _check_gradient(f"gradient, {path}, m = {m}, {kind}", fin, eng, c, kind, path)


@pytest.mark.parametrize("m,kind", [(4, "nine"), (12, "five")])
def test_gradient_interpreter(handles, m, kind):
    """finrom_fom_gradient on a handle without a band plan and the small-batch schedule out of the way: the interpreter's stored
    factor, the resolve op stream and fom_adjoint_kernel's contraction; m = 4 with nine fin conductivities, and m = 12 with five,
    where the order of the contraction's sums shows (see test_gradient_band_adjoint).
    Measured (grad, device / host64): m = 4, nine 1.6e-13 / 2.6e-13; m = 12, five 3.8e-12 / 1.7e-12 (2.3 x; entrywise 4.8e-12 /
    2.0e-12); J 8.0e-13 / 2.8e-13, qoi 5.3e-13 / 2.8e-13."""
    fin, eng, c = handles(m, kind, band=False)
    _small(eng, False)
    _check_gradient(f"gradient, interpreter, m = {m}, {kind}", fin, eng, c, kind, "interpreter")


# ---- general right-hand sides ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", Y.ADJOINT_M)
def test_right_hand_sides_on_the_stored_factor(handles, m):
    """finrom_fom_solve_rhs, nodal fields, three right-hand sides per sample -- dense random, five unit entries, the load F --:
    fom_band_resolve_kernel at every built window size (m = 4, 8, 16, 28 run here for the first time).  The third must reproduce the
    forward solve's w: held to the yardstick's w under the allowance of w, and set beside the device's own forward solve.
    Measured (out, device / host64): m = 4 1.6e-14 / 9.4e-15, 8: 4.0e-14 / 1.7e-14, 12: 6.4e-14 / 2.4e-14, 16: 1.2e-13 / 5.8e-14,
    20: 1.8e-13 / 5.5e-14, 24: 2.4e-13 / 6.7e-14, 28: 3.0e-13 / 6.4e-14 (4.7 x, the largest); A^-1 F against the yardstick's w the
    same figures."""
    fin, eng, c = handles(m, "field")
    res = eng.solve_rhs(c.X[:S], c.R[:S])
    assert eng.last_path() == BAND_PATH[m]
    _check(f"right-hand sides, m = {m}", c, res, range(S), ("out",), what="rhs")
    out = np.asarray(res["out"])
    _check(f"right-hand sides, m = {m}, rhs = F against w", c, {"w": out[:, 2]}, range(S), ("w",))
    fwd = fin.forward_batch(c.X[:S], want_w=True)
    dw = max(Y.dev(out[s, 2], np.asarray(fwd["w"])[s]) for s in range(S))
    d_host = c.d_host(range(S), ("w",))["w"]
    print(f"right-hand sides, m = {m}: A^-1 F against the device's forward w: {dw:.2e} (host64 vs yardstick {d_host:.2e})")
    assert dw <= 2.0 * Y.allowance(d_host)                   # both stand within the allowance of the same yardstick


@pytest.mark.parametrize("m", [12, 16])
def test_right_hand_sides_flag_indefinite_samples(handles, m):
    """A negative conductivity in every fin of sample 17 and in the centre post of sample 69 (the tail block), nine fin
    conductivities: info is non-zero exactly there and their `out` is NaN in every entry -- the failed pivot's reciprocal square
    root is NaN in the stored factor (fom_band.hip: rsq of a non-positive pivot, then the Newton steps), the forward substitution
    carries it down and the backward sweep to every dof.  Lane = sample: every other sample has the bits of the same call with those
    two samples replaced by valid ones."""
    fin, eng, c = handles(m, "nine")
    rhs = Y.case(m, "field").R[:S]
    X = c.X[:S].copy()
    X[17] = -X[17]
    X[69, 4] = -5.0
    res = eng.solve_rhs(X, rhs)
    assert eng.last_path() == BAND_PATH[m]
    bad = [17, 69]
    assert np.nonzero(np.asarray(res["info"]))[0].tolist() == bad
    out = np.asarray(res["out"])
    assert np.isnan(out[bad]).all()
    ref = eng.solve_rhs(c.X[:S], rhs)
    assert not np.asarray(ref["info"]).any()
    good = np.setdiff1d(np.arange(S), bad)
    assert np.isfinite(out[good]).all()
    assert _same_bits(out[good], np.asarray(ref["out"])[good])


# ---- Hessian action and sensitivity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [4, 12, 16])
def test_hessian_action_against_the_four_solves(handles, m):
    """Fin.hessian_action_batch for six samples (the forward solve, the adjoint and incremental state as two right-hand sides, the
    incremental adjoint as a third; the products in between on the host) against fom_ld's four solves in extended precision: the
    direct reference beside the finite-difference check of tests/test_gpu_band.py.
    Measured (H u, device / host64; entrywise in brackets): m = 4 2.9e-14 / 1.3e-14 (2.8e-14 / 2.0e-14), m = 12 8.6e-14 / 3.7e-14
    (9.1e-14 / 3.0e-14), m = 16 1.2e-13 / 7.4e-14 (1.1e-13 / 5.6e-14)."""
    fin, eng, c = handles(m, "field")
    n = Y.HESSIAN[(m, "field", False)]
    H = fin.hessian_action_batch(c.X[:n], c.U[:n], c.data)
    assert eng.last_path() == BAND_PATH[m]
    _check(f"Hessian action, m = {m}", c, {"Hu": H}, range(n), ("Hu", "Hu_max"), what="hess")


@pytest.mark.parametrize("n,path", [(56, "small_lds"), (57, "band_registers")])
def test_sensitivity_against_the_yardstick_jacobian(handles, n, path):
    """Fin.sensitivity_batch at m = 4, nodal fields: one QoI-only forward solve, then S n_obs value-and-gradient evaluations whose
    residuals are the unit vectors -- 504 of them (S = 56: the small-batch kernel) and 513 (S = 57: the band adjoint, one past the
    default threshold of 512).  Every Jacobian row of every sample.
    Measured (the worst Jacobian row, device / host64): S n_obs = 504: 3.2e-14 / 2.3e-14; 513: 3.8e-14 / 2.3e-14."""
    fin, eng, c = handles(4, "field")
    _small(eng, True)
    assert n * fin.n_obs in (504, 513)
    Jb = fin.sensitivity_batch(c.X[:n])
    assert eng.last_path() == path
    assert Jb.shape == (n, fin.n_obs, c.inp.n)
    _check(f"sensitivity, m = 4, S n_obs = {n * fin.n_obs}", c, {"jac": Jb}, range(n), ("jac",), what="sens")


# ---- pieces ----------------------------------------------------------------------------------------------------------------------
def _in_pieces(monkeypatch, call):
    """-> (the call's result without a bound, with FINROM_FOM_WORKSPACE_BYTES=1: pieces of 64 samples)."""
    whole = call()
    monkeypatch.setenv("FINROM_FOM_WORKSPACE_BYTES", "1")
    try:
        pieces = call()
    finally:
        monkeypatch.delenv("FINROM_FOM_WORKSPACE_BYTES")
    return whole, pieces


@pytest.mark.parametrize("band", [True, False], ids=["band", "interpreter"])
def test_gradient_in_pieces(handles, monkeypatch, band):
    """finrom_fom_gradient, m = 4, nine fin conductivities, S = 130 with per-sample data, the workspace bound at its floor: three
    pieces (64 + 64 + 2) through the band branch and through the interpreter branch, each offsetting x, data, grad, J, qoi and
    info.  The same bits as the call in one piece, and every sample -- sample 64, the first of the second piece, above all --
    within the allowance of the yardstick FOR ITS OWN DATA ROW: a piece that read the first piece's data again would not pass.
    Measured (sample 64, device / host64): band grad 5.0e-14 / 2.4e-14, J 1.4e-14 / 1.6e-14; interpreter grad 3.7e-14 / 2.4e-14.  With
    the band branch's `data + s0 * n_obs` replaced by `data` in a scratch build this test fails (grad: other bits)."""
    fin, eng, c = handles(4, "nine", band=band)
    _small(eng, False)
    n = Y.PIECES[(4, "nine", False)]
    assert n == 130 and not np.array_equal(c.D[64], c.D[0])
    whole, pieces = _in_pieces(monkeypatch, lambda: fin.gradient_batch(c.X[:n], c.D[:n], params="nine"))
    assert eng.last_path() == ("band_registers" if band else "interpreter")
    for k in ("grad", "J", "qoi", "info"):
        assert _same_bits(np.asarray(pieces[k]), np.asarray(whole[k])), k
    _check(f"gradient in pieces, {'band' if band else 'interpreter'}, sample 64", c, pieces, [64], ("grad", "grad_max", "J", "qoi"), True)
    _check(f"gradient in pieces, {'band' if band else 'interpreter'}, all 130", c, pieces, range(n), ("grad", "grad_max", "J", "qoi"), True)


def test_right_hand_sides_in_pieces(handles, monkeypatch):
    """finrom_fom_solve_rhs, m = 4, nodal fields, S = 130, three pieces: x, rhs, out and info offset per piece.  The same bits as
    in one piece; sample 64 (and every other) within the allowance of the yardstick for its own right-hand sides.
    Measured (out, device / host64): sample 64 1.1e-14 / 3.5e-15, all 130 1.6e-14 / 9.4e-15."""
    fin, eng, c = handles(4, "field")
    n = Y.PIECES[(4, "field", False)]
    assert n == 130
    whole, pieces = _in_pieces(monkeypatch, lambda: eng.solve_rhs(c.X[:n], c.R[:n]))
    assert eng.last_path() == "band_registers"
    for k in ("out", "info"):
        assert _same_bits(np.asarray(pieces[k]), np.asarray(whole[k])), k
    _check("right-hand sides in pieces, sample 64", c, pieces, [64], ("out",), what="rhs")
    _check("right-hand sides in pieces, all 130", c, pieces, range(n), ("out",), what="rhs")
