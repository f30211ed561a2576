"""The roomy projection kernel's epilogue that eliminates each block row in place (fused_solve_sw<NB, true, true, true>):
the 4 x 4 block steps that factor a diagonal tile scale and eliminate the whole block row [A_kk | A(kb, kb + 1 ..) | G_kb], so the
tile's inverse U_kk^-T is never formed.  Other products and sums than the short-waits form: qoi_r differs from it at rounding level
(printed, not bounded on its own) and is held to the yardsticks themselves -- the 80-bit LSPG of the list the sample walks
(tests/rom_lspg_cases.py: checked samples, max(8 d_host, 1e-12), under 1e-10), the oracle (1e-10), the pivoted solve on the
reference-recipe basis.  qoi, theta and info are the FOM half's and the averages': bit for bit those of the short-waits handle;
err is qoi - qoi_r of the same call.
Through finrom_solve_pairs at m = 4, five-parameter, the benchmark-recipe basis, handles created with FINROM_PROJ_BLOCK_ROW=1 (at
every batch size and width) beside handles created with FINROM_PROJ_SHORT_WAITS=1; every case asserts which form ran
(finrom_rom_last_epilogue: "roomy-block-row" / "roomy-short-waits").  Every NB from 1 to 5 with a full and a one-column last block;
batches of 1 (a lone wave), 5, 65 and 301 (a last workgroup with one live wave); m = 12, r = 80 once."""
import os

import numpy as np
import pytest

import rom_lspg_cases as Y
from oracle import fin_oracle as O
from test_gpu_proj_roomy import TOL, _basis, _oracle_qoi_r, _reference_recipe_basis, _ten, _with_env, rel

pytestmark = pytest.mark.gpu
M = 4
BASES = [8, 16, 17, 32, 33, 48, 49, 64, 65, 80]
BATCHES = [1, 5, 65, 301]
KEYS = ("qoi", "qoi_r", "err", "theta", "info")
SWITCHES = ("FINROM_PROJ_SHORT_WAITS", "FINROM_PROJ_FIXED_WAITS", "FINROM_PROJ_BLOCK_ROW", "FINROM_PROJ_NO_BLOCK_ROW")


def _without_env(names, make):
    old = {n: os.environ.pop(n, None) for n in names}
    try:
        return make()
    finally:
        os.environ.update({n: v for n, v in old.items() if v is not None})


def _under(name, make):
    """A handle created with `name` set and none of the other switches."""
    return _without_env(SWITCHES, lambda: _with_env(name, make))


def _pair(V, prob, r, fin):
    """The pair solvers whose reduced models were created under the two switches, on one basis and one FOM solver."""
    from bayesianinferencedl_amd.pairs import FinPairSolver
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    phi = _basis(prob, r)
    rom = _under("FINROM_PROJ_BLOCK_ROW", lambda: AffineROMFin(V, None, phi))
    rom0 = _under("FINROM_PROJ_SHORT_WAITS", lambda: AffineROMFin(V, None, phi))
    return (phi, rom, FinPairSolver(V, phi, params="five", solver=fin, solver_r=rom),
            rom0, FinPairSolver(V, phi, params="five", solver=fin, solver_r=rom0))


def _both(made, X):
    """The batch through both forms; asserts that each ran its own instantiation of the one-wave roomy kernel."""
    _, rom, ps, rom0, ps0 = made
    a = ps.solve_pairs(X)
    assert rom._rom.last_epilogue() == "roomy-block-row"
    b = ps0.solve_pairs(X)
    assert rom0._rom.last_epilogue() == "roomy-short-waits"
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


def _walked(rom):
    """The list the handle's in-range samples walked in its last launch, in the words of rom_lspg_cases.Case."""
    if rom._rom.last_form() != "half":
        return "full"
    return "short" if rom._rom.mirror_dropped else "half"


def _check(label, prob, made, X, a, b):
    """What every clean batch is held to.  a: the block-row form's outputs, b: the short-waits form's."""
    phi, rom = made[0], made[1]
    S = len(X)
    assert not a["info"].any() and not b["info"].any()
    for k in ("qoi", "theta", "info"):
        assert _same_bits(a[k], b[k]), k
    assert np.array_equal(a["err"], a["qoi"] - a["qoi_r"])
    print(f"{label}: block row vs short waits, qoi_r {rel(a['qoi_r'], b['qoi_r']):.3e}, err rows {rel(a['err'], b['err']):.3e}")
    rows = _ten(S)
    d = rel(a["qoi_r"][rows], _oracle_qoi_r(prob, phi, X, rows))
    print(f"{label}: block row, qoi_r vs oracle {d:.3e}")
    assert d < TOL
    c = Y.Case.from_rom(rom, a["theta"])
    assert Y.report(f"{label}: block row against the 80-bit LSPG of its list",
                    c.against_ld(a, Y.checked_samples(S), ("qoi_r",), form=_walked(rom)))


@pytest.mark.parametrize("S", BATCHES)
@pytest.mark.parametrize("r", BASES)
def test_every_width_and_batch(problems, solvers, r, S):
    made = solvers(M, r)
    X = np.random.default_rng(7000 + 10 * r + S).uniform(0.1, 10.0, (S, 5))
    a, b = _both(made, X)
    _check(f"m = {M}, r = {r}, S = {S}", problems(M), made, X, a, b)


def test_the_headline_sizes(problems, solvers):
    m, r, S = 12, 80, 301
    made = solvers(m, r)
    X = np.random.default_rng(7001).uniform(0.1, 10.0, (S, 5))
    a, b = _both(made, X)
    _check(f"m = {m}, r = {r}, S = {S}", problems(m), made, X, a, b)


_RECIPE = {}


@pytest.mark.parametrize("S", [13, 130])
def test_ill_conditioned_basis(problems, spaces, S):
    """tests/test_gpu_proj_roomy.py's case with its bound: the reference-recipe basis at r = 80 (the full list under this epilogue),
    cond(A_r) > 1e9, qoi_r against the oracle's pivoted solve."""
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.pairs import FinPairSolver
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    m, r = 12, 80
    prob, V = problems(m), spaces(m)
    if not _RECIPE:                                          # once for both batch sizes
        fin = Fin(V)
        phi = np.ascontiguousarray(_reference_recipe_basis(fin, 81, np.random.default_rng(21))[:, :r])
        rom = _under("FINROM_PROJ_BLOCK_ROW", lambda: AffineROMFin(V, None, phi))
        rom0 = _under("FINROM_PROJ_SHORT_WAITS", lambda: AffineROMFin(V, None, phi))
        assert not rom._rom.mirror
        _RECIPE.update(fin=fin, phi=phi, rom=rom, rom0=rom0)
    fin, phi, rom, rom0 = _RECIPE["fin"], _RECIPE["phi"], _RECIPE["rom"], _RECIPE["rom0"]
    X = np.random.default_rng(22 + S).uniform(0.1, 10.0, (S, 5))
    res = FinPairSolver(V, phi, params="five", solver=fin, solver_r=rom).solve_pairs(X)
    assert rom._rom.last_epilogue() == "roomy-block-row" and rom._rom.last_form() == "full"
    ref = FinPairSolver(V, phi, params="five", solver=fin, solver_r=rom0).solve_pairs(X)
    assert rom0._rom.last_epilogue() == "roomy-short-waits"
    assert not np.asarray(res["info"]).any()
    ro = O.AffineROMOracle(prob, phi)
    th = np.asarray(res["theta"])
    conds, worst, worst0 = [], 0.0, 0.0
    for s in _ten(S):
        w_r, A_r, _, _ = ro.forward_nine_param_reduced(th[s], True)       # np.linalg.solve (pivoted LU)
        conds.append(np.linalg.cond(A_r))
        q = ro.qoi_reduced(w_r)
        worst = max(worst, np.linalg.norm(np.asarray(res["qoi_r"])[s] - q) / np.linalg.norm(q))
        worst0 = max(worst0, np.linalg.norm(np.asarray(ref["qoi_r"])[s] - q) / np.linalg.norm(q))
    print(f"reference-recipe basis, S = {S}: max cond(A_r) {max(conds):.3e}, qoi_r vs pivoted solve: block row {worst:.3e}, "
          f"short waits {worst0:.3e}; block row vs short waits {rel(res['qoi_r'], ref['qoi_r']):.3e}")
    assert max(conds) > 1e9, max(conds)
    assert worst < 1e-10, worst


@pytest.mark.parametrize("turn", [0, 1, 2])
@pytest.mark.parametrize("r", [17, 48, 80])
def test_flagged_samples_keep_their_flags_and_their_neighbours_their_bits(solvers, r, turn):
    """A NaN conductivity, rows of 1e200 (A_r = inf) and an all-zero row (the FOM half flags it) at the first sample, a middle one
    and the last one of a batch of 65, each kind at each place over the three turns: the same info and the same NaN rows as the
    short-waits form, and every other sample keeps the bits of the clean batch of the same form."""
    made = solvers(M, r)
    S = 65
    bad = [0, 33, 64]
    X = np.random.default_rng(8000 + r).uniform(0.1, 10.0, (S, 5))
    clean, clean0 = _both(made, X)
    Yb = X.copy()
    Yb[bad[turn % 3], 1] = np.nan
    Yb[bad[(turn + 1) % 3]] = 1e200
    Yb[bad[(turn + 2) % 3]] = 0.0
    a, b = _both(made, Yb)
    assert _same_bits(a["info"], b["info"])
    assert np.array_equal(np.isnan(a["qoi_r"]), np.isnan(b["qoi_r"])) and np.array_equal(np.isnan(a["err"]), np.isnan(b["err"]))
    for s in bad:
        assert a["info"][s] != 0 and np.isnan(a["qoi_r"][s]).all() and np.isnan(a["err"][s]).all(), (s, a["info"][s], a["qoi_r"][s])
    good = np.setdiff1d(np.arange(S), bad)
    assert not a["info"][good].any()
    for k in ("qoi_r", "err", "qoi"):
        assert _same_bits(np.ascontiguousarray(a[k][good]), np.ascontiguousarray(clean[k][good])), k
        assert _same_bits(np.ascontiguousarray(b[k][good]), np.ascontiguousarray(clean0[k][good])), k


def test_the_default_takes_the_block_rows_where_it_pays(problems, spaces, solvers):
    """A handle created under NO switch: from 16 384 samples on (the half sweep on its CU-masked stream) a basis of 65 .. 80 columns
    runs the block-row form, one sample fewer keeps the fixed waits, and r = 17 keeps the short-waits form at 16 384.  A handle
    created with FINROM_PROJ_NO_BLOCK_ROW=1 returns the bits of the short-waits handle."""
    from bayesianinferencedl_amd.pairs import FinPairSolver
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    S = 16384
    V = spaces(M)
    X = np.random.default_rng(9000).uniform(0.1, 10.0, (S, 5))
    phi, _, ps1, rom0, ps0 = solvers(M, 80)
    rom = _without_env(SWITCHES, lambda: AffineROMFin(V, None, phi))
    ps = FinPairSolver(V, phi, params="five", solver=ps0.solver, solver_r=rom)
    a = ps.solve_pairs(X)
    assert rom._rom.last_epilogue() == "roomy-block-row"
    a = {k: np.array(np.asarray(a[k])) for k in KEYS}
    forced = ps1.solve_pairs(X)
    for k in KEYS:
        assert _same_bits(a[k], np.array(np.asarray(forced[k]))), k
    ps.solve_pairs(X[:S - 1])
    assert rom._rom.last_epilogue() == "roomy"
    off = _under("FINROM_PROJ_NO_BLOCK_ROW", lambda: AffineROMFin(V, None, phi))
    b = FinPairSolver(V, phi, params="five", solver=ps0.solver, solver_r=off).solve_pairs(X)
    assert off._rom.last_epilogue() == "roomy-short-waits"
    c = ps0.solve_pairs(X)
    assert rom0._rom.last_epilogue() == "roomy-short-waits"
    for k in KEYS:
        assert _same_bits(np.array(np.asarray(b[k])), np.array(np.asarray(c[k]))), k
    print(f"m = {M}, r = 80, S = {S}: block row vs short waits, qoi_r {rel(a['qoi_r'], np.asarray(c['qoi_r'])):.3e}")
    phi17 = solvers(M, 17)[0]
    rom17 = _without_env(SWITCHES, lambda: AffineROMFin(V, None, phi17))
    FinPairSolver(V, phi17, params="five", solver=ps0.solver, solver_r=rom17).solve_pairs(X)
    assert rom17._rom.last_epilogue() == "roomy-short-waits"
