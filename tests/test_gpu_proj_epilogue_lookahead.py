"""The roomy projection kernel's epilogue without fixed waits between dependent MFMAs (fused_solve_sw<NB, true, true>):
an MFMA that accumulates onto its predecessor's result is ordered by the hardware (tools/mfma_f64_chain.hip), so the 80-cycle waits
stay only where a result is read as an operand or by ordinary code.  Every product and sum keeps its place, so the bits are those
of the form with the waits (a second instantiation, the parent's code).  finrom_solve_pairs takes the short waits only beside a
sweep on its masked stream (one case checks that choice with a handle under neither switch, at 16 384 samples and one fewer),
which the other batches are too small for: their handles are created with FINROM_PROJ_SHORT_WAITS=1 (at every batch size) and
FINROM_PROJ_FIXED_WAITS=1 (never).  Through finrom_solve_pairs at m = 4, the FOM's half plan, QoI-only (the
widest bases of this small mesh are not mirror-symmetric: their projection walks the full list); every case asserts which form
ran (finrom_rom_last_epilogue: "roomy-short-waits" / "roomy").
Every NB from 1 to 5 with a full and a one-column last block; batches of 1 (a lone wave), 5, 65 and 301 (a last workgroup with one
live wave).  (The file keeps the name of the look-ahead it was first written for, DESIGN 5 round 13: measured as no gain, not built.)"""
import os

import numpy as np
import pytest

from test_gpu_proj_roomy import TOL, _basis, _oracle_qoi_r, _ten, _with_env, rel

pytestmark = pytest.mark.gpu
M = 4
BASES = [8, 16, 17, 32, 33, 48, 49, 64, 65, 80]
BATCHES = [1, 5, 65, 301]
KEYS = ("qoi_r", "err", "theta", "info")


def _pair(V, prob, r, fin):
    """The pair solvers whose reduced models were created under the two switches, on one basis and one FOM solver."""
    from bayesianinferencedl_amd.pairs import FinPairSolver
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    phi = _basis(prob, r)
    rom = _with_env("FINROM_PROJ_SHORT_WAITS", lambda: AffineROMFin(V, None, phi))
    rom0 = _with_env("FINROM_PROJ_FIXED_WAITS", lambda: AffineROMFin(V, None, phi))
    return (phi, rom, FinPairSolver(V, phi, params="five", solver=fin, solver_r=rom),
            rom0, FinPairSolver(V, phi, params="five", solver=fin, solver_r=rom0))


def _both(made, X):
    """The batch through both forms; asserts that each ran its own instantiation of the one-wave roomy kernel."""
    _, rom, ps, rom0, ps0 = made
    a = ps.solve_pairs(X)
    assert rom._rom.last_epilogue() == "roomy-short-waits"
    b = ps0.solve_pairs(X)
    assert rom0._rom.last_epilogue() == "roomy"
    return ({k: np.array(np.asarray(a[k])) for k in KEYS}, {k: np.array(np.asarray(b[k])) for k in KEYS})


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def solvers(problems, spaces):
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    made, fins = {}, {}

    def get(m, r):
        if (m, r) not in made:
            if m not in fins:
                fins[m] = Fin(spaces(m))
            made[(m, r)] = _pair(spaces(m), problems(m), r, fins[m])
        return made[(m, r)]
    return get


@pytest.mark.parametrize("S", BATCHES)
@pytest.mark.parametrize("r", BASES)
def test_bits_of_the_fixed_waits_form(solvers, r, S):
    X = np.random.default_rng(3000 + 10 * r + S).uniform(0.1, 10.0, (S, 5))
    a, b = _both(solvers(M, r), X)
    assert not a["info"].any()
    for k in KEYS:
        assert _same_bits(a[k], b[k]), k


@pytest.mark.parametrize("r", [17, 48, 80])
def test_flagged_samples_keep_their_flags_and_their_neighbours_their_bits(solvers, r):
    """A NaN conductivity (A_r non-finite through the ungrouped loop) and overflowing ones (1e200: A_r = inf) at the first sample of a
    workgroup (4), a middle one (9) and the last one (15) of a batch of 65: the same info and the same NaN rows in both forms, and
    every other sample keeps the bits of the clean batch."""
    made = solvers(M, r)
    S, bad = 65, [4, 9, 15]
    X = np.random.default_rng(4000 + r).uniform(0.1, 10.0, (S, 5))
    clean, _ = _both(made, X)
    Y = X.copy()
    Y[4, 1] = np.nan
    Y[9] = 1e200
    Y[15, 3] = 1e200
    a, b = _both(made, Y)
    for k in ("qoi_r", "err", "info"):
        assert _same_bits(a[k], b[k]), k
    for s in bad:
        assert a["info"][s] != 0 and np.isnan(a["qoi_r"][s]).all(), (s, a["info"][s], a["qoi_r"][s])
    good = np.setdiff1d(np.arange(S), bad)
    assert not a["info"][good].any()
    assert _same_bits(np.ascontiguousarray(a["qoi_r"][good]), np.ascontiguousarray(clean["qoi_r"][good]))


def _without_env(names, make):
    old = {n: os.environ.pop(n, None) for n in names}
    try:
        return make()
    finally:
        os.environ.update({n: v for n, v in old.items() if v is not None})


def test_the_default_takes_the_short_waits_where_the_sweep_is_masked(problems, spaces, solvers):
    """A handle created under NEITHER switch: finrom_solve_pairs confines the half sweep to its CU-masked stream from 16 384 samples
    on, and there -- only there -- the projection runs the short-waits form; one sample fewer keeps the fixed waits.  The bits of
    the large batch are those of the handle that never takes the short waits."""
    from bayesianinferencedl_amd.pairs import FinPairSolver
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    r, S = 17, 16384
    phi, _, _, rom0, ps0 = solvers(M, r)
    V = spaces(M)
    rom = _without_env(("FINROM_PROJ_SHORT_WAITS", "FINROM_PROJ_FIXED_WAITS"), lambda: AffineROMFin(V, None, phi))
    ps = FinPairSolver(V, phi, params="five", solver=ps0.solver, solver_r=rom)
    X = np.random.default_rng(6000).uniform(0.1, 10.0, (S, 5))
    a = ps.solve_pairs(X)
    assert rom._rom.last_epilogue() == "roomy-short-waits"
    b = ps0.solve_pairs(X)
    assert rom0._rom.last_epilogue() == "roomy"
    assert not np.asarray(a["info"]).any()
    for k in KEYS:
        assert _same_bits(np.array(np.asarray(a[k])), np.array(np.asarray(b[k]))), k
    ps.solve_pairs(X[:S - 1])
    assert rom._rom.last_epilogue() == "roomy"


def test_against_the_oracle_at_the_headline_sizes(problems, solvers):
    m, r, S = 12, 80, 301
    made = solvers(m, r)
    X = np.random.default_rng(5000).uniform(0.1, 10.0, (S, 5))
    a, b = _both(made, X)
    assert not a["info"].any()
    for k in KEYS:
        assert _same_bits(a[k], b[k]), k
    rows = _ten(S)
    d = rel(a["qoi_r"][rows], _oracle_qoi_r(problems(m), made[0], X, rows))
    print(f"m = {m}, r = {r}, S = {S}: short waits, qoi_r vs oracle {d:.3e}")
    assert d < TOL
