"""The half plan's post as functionals on the device (csrc/fom_band.hip fom_band_half_fn_kernel, DESIGN 4c'): the five distinct
observation rows ride the post's forward sweep as right-hand sides, q_o = (L^-1 c_o)^T (L^-1 f), nothing of the post's factor is
stored and no backward sweep runs.  Lane tails and more than one wave, against the oracle, the full plan (FINROM_NO_MIRROR=1) and
the stored-factor form of the half plan (FINROM_FOM_POST_STORED=1, both at engine creation); mirror copies and repeatability bit
for bit; failure flags; the sample-pair path; a call that runs in pieces."""
import itertools
import os

import numpy as np
import pytest

from oracle import fin_oracle as O

pytestmark = pytest.mark.gpu
MS = [4, 8, 12]
SIZES = [1, 63, 64, 65, 200]
SMAX = 200
PICKS = (0, 31, 62, 63, 64, 199)                          # corners, lane 63 and 0 of two waves, the tail wave's last lane


def _rel(a, b):
    return np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1))


def _fin(V, env=None):
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    old = os.environ.get(env) if env else None
    if env:
        os.environ[env] = "1"
    try:
        fin = Fin(V)
        fin._engine("five").set_small_max(0)
    finally:
        if env:
            if old is None:
                del os.environ[env]
            else:
                os.environ[env] = old
    return fin


def _batch(m):
    """The 32 corners of [0.1, 10]^5 first, then uniform samples: every prefix of a size in SIZES holds corners."""
    corners = np.array(list(itertools.product((0.1, 10.0), repeat=5)))
    rest = np.random.default_rng(900 + m).uniform(0.1, 10.0, (SMAX - len(corners), 5))
    return np.vstack([corners, rest])


@pytest.fixture(scope="module")
def cases(spaces):
    """Per mesh, once: the three engines, the batch, and the results of the largest batch."""
    made = {}

    def get(m):
        if m not in made:
            V = spaces(m)
            X = _batch(m)
            fin = _fin(V)
            eng = fin._engine("five")
            assert eng.band_mirror is not None and eng.band_mirror_form == 2, "functional form not installed"
            fin_full = _fin(V, "FINROM_NO_MIRROR")
            assert fin_full._engine("five").band_mirror is None and fin_full._engine("five").band is not None
            fin_st = _fin(V, "FINROM_FOM_POST_STORED")
            assert fin_st._engine("five").band_mirror is not None and fin_st._engine("five").band_mirror_form == 1
            ref_full = fin_full.forward_batch(X, want_w=False, params="five")
            ref_st = fin_st.forward_batch(X, want_w=False, params="five")
            assert fin_st._engine("five").last_path() == "band_registers_qoi"
            made[m] = (fin, X, np.asarray(ref_full["qoi"]), np.asarray(ref_st["qoi"]))
        return made[m]
    return get


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("m", MS)
def test_functional_form_matches_oracle_full_plan_and_stored_form(problems, cases, m, S):
    """Batches of S samples (a single lane, a wave short of one lane, a full wave, one lane into the second wave, three waves and
    a tail of 8): 1e-10 against the oracle on the picks that exist, 1e-11 against the full plan and against the stored-factor half
    plan; no sample flagged; mirrored columns equal bit for bit; a second call returns the same bits.
    Measured on MI355X, worst over the sizes, max over the batch of the relative QoI difference:
    against the full plan m = 4: 8.4e-14, m = 8: 3.5e-13, m = 12: 4.6e-13; against the stored form m = 4: 6.6e-16, m = 8: 1.3e-15,
    m = 12: 2.3e-15."""
    fin, X, ref_full, ref_st = cases(m)
    res = fin.forward_batch(X[:S], want_w=False, params="five")
    assert fin._engine("five").last_path() == "band_registers_qoi"
    q = np.asarray(res["qoi"])
    assert q.shape == (S, 9) and (np.asarray(res["info"]) == 0).all()
    fo = O.FinOracle(problems(m))
    for s in PICKS:
        if s < S:
            qo = fo.qoi_operator(fo.forward(fo.five_param_to_function(X[s])))
            assert np.linalg.norm(q[s] - qo) < 1e-10 * np.linalg.norm(qo), s
    d_full, d_st = _rel(q, ref_full[:S]), _rel(q, ref_st[:S])
    print(f"functional form, m = {m}, S = {S}: vs full plan {d_full:.3e}, vs stored half plan {d_st:.3e}")
    assert d_full < 1e-11 and d_st < 1e-11
    assert np.array_equal(q[:, ::-1], q)
    again = fin.forward_batch(X[:S], want_w=False, params="five")
    assert np.array_equal(np.asarray(again["qoi"]), q) and np.array_equal(np.asarray(again["info"]), np.asarray(res["info"]))


@pytest.mark.parametrize("m", MS)
def test_functional_form_flags_indefinite_samples(cases, m):
    """A negative fin conductivity in the second wave (a fin's sweep sees it) and a negative post conductivity in the tail wave
    (the post's sweep sees it): exactly those two samples are flagged and NaN in all nine columns; their lane neighbours are finite."""
    fin, X, _, _ = cases(m)
    Xb = X.copy()
    Xb[70, 2] = -3.0
    Xb[195, 4] = -5.0
    res = fin.forward_batch(Xb, want_w=False, params="five")
    assert fin._engine("five").last_path() == "band_registers_qoi"
    bad = [70, 195]
    q = np.asarray(res["qoi"])
    assert np.nonzero(res["info"])[0].tolist() == bad
    assert np.isnan(q[bad]).all()
    assert np.isfinite(q[np.setdiff1d(np.arange(SMAX), bad)]).all()
    assert np.isfinite(q[[69, 71, 194, 196]]).all()


@pytest.mark.parametrize("m", MS)
def test_a_call_in_pieces_returns_the_same_bits(cases, monkeypatch, m):
    """With the workspace bound at its floor (64 samples a piece) the 200 samples run as four pieces: the same bits as in one."""
    fin, X, _, _ = cases(m)
    whole = fin.forward_batch(X, want_w=False, params="five")
    monkeypatch.setenv("FINROM_FOM_WORKSPACE_BYTES", "1")
    pieces = fin.forward_batch(X, want_w=False, params="five")
    monkeypatch.delenv("FINROM_FOM_WORKSPACE_BYTES")
    assert np.array_equal(np.asarray(pieces["qoi"]), np.asarray(whole["qoi"]))
    assert np.array_equal(np.asarray(pieces["info"]), np.asarray(whole["info"]))


def test_pair_path_takes_the_functional_form(problems, spaces):
    """finrom_solve_pairs at m = 12, r = 16, S = 130: the FOM half is the functional form's sweep -- the bits of
    forward_batch(want_w=False) -- and err is the difference of the two halves exactly."""
    from bayesianinferencedl_amd.pairs import FinPairSolver
    m, r, Sp = 12, 16, 130
    prob, V = problems(m), spaces(m)
    fo = O.FinOracle(prob)
    rng = np.random.default_rng(5)
    Y = np.array([fo.forward(fo.nine_param_to_function(rng.uniform(0.1, 3.5, 9))) for _ in range(40)])
    phi = O.pod_basis(Y, r)
    X = rng.uniform(0.1, 10.0, (Sp, 5))
    ps = FinPairSolver(V, phi, params="five")
    eng = ps.solver._engine("five")
    assert eng.band_mirror is not None and eng.band_mirror_form == 2
    res = ps.solve_pairs(X)
    assert eng.last_path() == "band_registers_qoi"
    assert (np.asarray(res["info"]) == 0).all()
    ref = ps.solver.forward_batch(X, want_w=False, params="five")
    assert np.array_equal(np.asarray(res["qoi"]), np.asarray(ref["qoi"]))
    assert np.array_equal(np.asarray(res["err"]), np.asarray(res["qoi"]) - np.asarray(res["qoi_r"]))
