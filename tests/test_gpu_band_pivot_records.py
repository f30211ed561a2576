"""The functional form of the half plan on pivot records (csrc/fom_band.hip band_sweep_rec / fom_band_half_fnrec_kernel, DESIGN
4c'): the sweeps fetch one prefetched record per pivot instead of nine tables, and the load of a fin's g is unconditional.  The
arithmetic is the table-reading kernel's operation by operation, so every output is compared BIT FOR BIT with an engine created
under FINROM_FOM_NO_PIVOT_RECORDS=1: lane tails and more than one wave, indefinite samples, a call in pieces, the pair path."""
import itertools
import os

import numpy as np
import pytest

from oracle import fin_oracle as O

pytestmark = pytest.mark.gpu
MS = [4, 8, 12]
SIZES = [1, 63, 64, 65, 130]
SMAX = 130
PICKS = (0, 31, 62, 63, 64, 129)                          # corners, lane 63 and 0 of two waves, the tail wave's last lane
SWITCH = "FINROM_FOM_NO_PIVOT_RECORDS"


def _with_env(env, make):
    old = os.environ.get(env) if env else None
    if env:
        os.environ[env] = "1"
    try:
        return make()
    finally:
        if env:
            if old is None:
                del os.environ[env]
            else:
                os.environ[env] = old


def _fin(V, env=None):
    from bayesianinferencedl_amd.fom.forward_solve import Fin

    def make():
        fin = Fin(V)
        fin._engine("five").set_small_max(0)
        return fin
    return _with_env(env, make)


def _batch(m):
    """The 32 corners of [0.1, 10]^5 first, then uniform samples: every prefix of a size in SIZES holds corners."""
    corners = np.array(list(itertools.product((0.1, 10.0), repeat=5)))
    rest = np.random.default_rng(1200 + m).uniform(0.1, 10.0, (SMAX - len(corners), 5))
    return np.vstack([corners, rest])


def _same_bits(a, b):
    """Equal as bit patterns (NaNs included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cases(spaces):
    """Per mesh, once: the engine on records, the engine on tables, the batch."""
    made = {}

    def get(m):
        if m not in made:
            V = spaces(m)
            fin = _fin(V)
            eng = fin._engine("five")
            assert eng.band_mirror is not None and eng.band_mirror_form == 2 and eng.band_mirror_records is True
            fin_t = _fin(V, SWITCH)
            eng_t = fin_t._engine("five")
            assert eng_t.band_mirror is not None and eng_t.band_mirror_form == 2 and eng_t.band_mirror_records is False
            made[m] = (fin, fin_t, _batch(m))
        return made[m]
    return get


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("m", MS)
def test_records_return_the_bits_of_the_tables(problems, cases, m, S):
    """qoi and info bit-identical to the switched-off engine; both within 1e-10 of the oracle on the picks that exist."""
    fin, fin_t, X = cases(m)
    res = fin.forward_batch(X[:S], want_w=False, params="five")
    ref = fin_t.forward_batch(X[:S], want_w=False, params="five")
    assert fin._engine("five").last_path() == "band_registers_qoi" and fin_t._engine("five").last_path() == "band_registers_qoi"
    q, qt = np.asarray(res["qoi"]), np.asarray(ref["qoi"])
    assert q.shape == (S, 9) and (np.asarray(res["info"]) == 0).all()
    assert _same_bits(q, qt) and _same_bits(np.asarray(res["info"]), np.asarray(ref["info"]))
    fo = O.FinOracle(problems(m))
    for s in PICKS:
        if s < S:
            qo = fo.qoi_operator(fo.forward(fo.five_param_to_function(X[s])))
            assert np.linalg.norm(q[s] - qo) < 1e-10 * np.linalg.norm(qo), s
            assert np.linalg.norm(qt[s] - qo) < 1e-10 * np.linalg.norm(qo), s


@pytest.mark.parametrize("m", MS)
def test_indefinite_samples_flag_alike(cases, m):
    """A negative conductivity in lanes 0 and 63 of the first wave (a fin's sweep and the post's see one each) and in the tail
    wave's last lane: the same flags and NaNs as the switched-off engine, exactly those three samples."""
    fin, fin_t, X = cases(m)
    Xb = X.copy()
    Xb[0, 1] = -2.0
    Xb[63, 4] = -5.0
    Xb[SMAX - 1, 2] = -3.0
    res = fin.forward_batch(Xb, want_w=False, params="five")
    ref = fin_t.forward_batch(Xb, want_w=False, params="five")
    q, info = np.asarray(res["qoi"]), np.asarray(res["info"])
    bad = [0, 63, SMAX - 1]
    assert np.nonzero(info)[0].tolist() == bad
    assert np.isnan(q[bad]).all() and np.isfinite(q[np.setdiff1d(np.arange(SMAX), bad)]).all()
    assert _same_bits(q, np.asarray(ref["qoi"])) and _same_bits(info, np.asarray(ref["info"]))


@pytest.mark.parametrize("m", MS)
def test_a_call_in_pieces_returns_the_same_bits(cases, monkeypatch, m):
    """With the workspace bound at its floor (64 samples a piece) the 130 samples run as three pieces: the same bits as in one."""
    fin, _, X = cases(m)
    whole = fin.forward_batch(X, want_w=False, params="five")
    monkeypatch.setenv("FINROM_FOM_WORKSPACE_BYTES", "1")
    pieces = fin.forward_batch(X, want_w=False, params="five")
    monkeypatch.delenv("FINROM_FOM_WORKSPACE_BYTES")
    assert _same_bits(np.asarray(pieces["qoi"]), np.asarray(whole["qoi"]))
    assert _same_bits(np.asarray(pieces["info"]), np.asarray(whole["info"]))


def test_pair_path_returns_the_bits_of_the_tables(problems, spaces):
    """finrom_solve_pairs at m = 4, r = 16, S = 65: every output of the pair path equals the switched-off engine's bit for bit.
    (A batch this small is not confined to the CU-masked stream, and there the pair path sweeps on the tables even with records
    installed: what this pins is that installing them changes no output of the path.  The record kernel against the table kernel
    ON the pair path is tests/test_gpu_bench_contract.py::test_cu_masked_fom_stream_gives_the_same_outputs: 20 000 samples, masked
    -- records -- against FINROM_FOM_CUS=0 -- tables --, equal checksums.)"""
    from bayesianinferencedl_amd.pairs import FinPairSolver
    m, r, Sp = 4, 16, 65
    prob, V = problems(m), spaces(m)
    fo = O.FinOracle(prob)
    rng = np.random.default_rng(12)
    Y = np.array([fo.forward(fo.nine_param_to_function(rng.uniform(0.1, 3.5, 9))) for _ in range(40)])
    phi = O.pod_basis(Y, r)
    X = rng.uniform(0.1, 10.0, (Sp, 5))
    ps = FinPairSolver(V, phi, params="five")
    eng = ps.solver._engine("five")
    assert eng.band_mirror_form == 2 and eng.band_mirror_records is True

    def switched_off():                                   # (the engine is made on first use: the switch is read then)
        p = FinPairSolver(V, phi, params="five")
        p.solver._engine("five")
        return p
    ps_t = _with_env(SWITCH, switched_off)
    assert ps_t.solver._engine("five").band_mirror_form == 2 and ps_t.solver._engine("five").band_mirror_records is False
    res, ref = ps.solve_pairs(X), ps_t.solve_pairs(X)
    assert eng.last_path() == "band_registers_qoi"
    for k in ("qoi", "qoi_r", "err", "theta", "info"):
        assert _same_bits(np.asarray(res[k]), np.asarray(ref[k])), k
