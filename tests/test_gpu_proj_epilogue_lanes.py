"""The roomy projection kernel's epilogue factors its diagonal tiles through LDS (diag_tile_inverse<true>): each wave
writes the 4 x 4 block and the table of its inverse to an area of its own and reads them back.  NB = 1 .. 5 with and without padded
columns; S = 1 (a lone wave), 5 (a second workgroup with one live wave) and 130 (full workgroups).  Against the oracle and the
handle's solve-based epilogue as test_gpu_proj_roomy.py does; a wave's area is its own (neighbouring samples at opposite ends of
the conductivity range return the bits of one-sample calls); a NaN sample inside a workgroup is flagged alone.  The short half list
these calls walk is the scale-free one (tests/test_rom_short_scale_free_host.py)."""
import numpy as np
import pytest

from test_gpu_proj_roomy import TOL, _basis, _oracle_qoi_r, _ten, rel

pytestmark = pytest.mark.gpu
CASES = [(4, 16), (12, 17), (12, 33), (12, 64), (12, 80)]
SIZES = [1, 5, 130]


def _alternating(S, seed):
    """Neighbouring samples at opposite ends of the range: even ones near 0.1, odd ones near 10, in all five parameters."""
    rng = np.random.default_rng(seed)
    X = np.where((np.arange(S) % 2 == 0)[:, None], rng.uniform(0.1, 0.12, (S, 5)), rng.uniform(9.0, 10.0, (S, 5)))
    return np.ascontiguousarray(X)


@pytest.fixture(scope="module")
def cases(problems, spaces):
    """Per (m, r), once: basis, model with the half list, pair solver, and per batch size the inputs and the result."""
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    from bayesianinferencedl_amd.pairs import FinPairSolver
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    made, fins = {}, {}

    def get(m, r):
        if (m, r) not in made:
            prob, V = problems(m), spaces(m)
            if m not in fins:
                fins[m] = Fin(V)
            phi = _basis(prob, r)
            rom = AffineROMFin(V, None, phi)
            assert rom._rom.mirror, f"half list not installed (eps_probe {rom._rom.mirror_eps})"
            ps = FinPairSolver(V, phi, params="five", solver=fins[m], solver_r=rom)
            runs = {}
            for S in SIZES:
                X = np.random.default_rng(2000 * m + 10 * r + S).uniform(0.1, 10.0, (S, 5))
                res = ps.solve_pairs(X)
                assert rom._rom.last_epilogue() == "roomy" and rom._rom.last_form() == "half"
                runs[S] = (X, {k: np.array(np.asarray(res[k])) for k in ("qoi_r", "qoi", "info", "theta")})
            made[(m, r)] = (prob, phi, rom, ps, runs)
        return made[(m, r)]
    return get


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("m,r", CASES)
def test_against_the_oracle_and_the_solve_based_path(cases, m, r, S):
    prob, phi, rom, _, runs = cases(m, r)
    X, res = runs[S]
    assert not res["info"].any()
    rows = _ten(S)
    d = rel(res["qoi_r"][rows], _oracle_qoi_r(prob, phi, X, rows))
    b = rom.forward_nine_param_reduced_batch(res["theta"], want_w=True)
    assert rom._rom.last_epilogue() == "standard" and not np.asarray(b["info"]).any()
    e = rel(res["qoi_r"], b["qoi_r"])
    print(f"m = {m}, r = {r}, S = {S}: roomy qoi_r vs oracle {d:.3e}, vs solve-based {e:.3e}")
    assert d < TOL
    assert e < 1e-11


@pytest.mark.parametrize("S", [5, 130])
@pytest.mark.parametrize("m,r", CASES)
def test_each_wave_has_its_own_lds_area(cases, m, r, S):
    """The four waves of a workgroup factor blocks that differ by orders of magnitude; each sample comes back with the bits of a
    call that runs it alone (the first, a middle and the last workgroup at S = 130)."""
    _, _, rom, ps, _ = cases(m, r)
    X = _alternating(S, 7 * m + r + S)
    res = ps.solve_pairs(X)
    assert rom._rom.last_epilogue() == "roomy" and rom._rom.last_form() == "half"
    q, info = np.array(np.asarray(res["qoi_r"])), np.array(np.asarray(res["info"]))
    assert not info.any()
    rows = range(S) if S <= 8 else [0, 1, 2, 3, 64, 65, 66, 67, S - 2, S - 1]
    for s in rows:
        one = ps.solve_pairs(X[s:s + 1])
        assert rom._rom.last_epilogue() == "roomy"
        assert np.array_equal(np.asarray(one["qoi_r"])[0], q[s]), (s, np.asarray(one["qoi_r"])[0], q[s])


@pytest.mark.parametrize("S", [5, 130])
@pytest.mark.parametrize("m,r", CASES)
def test_a_nan_sample_inside_a_workgroup(cases, m, r, S):
    """Sample 1 (the second wave of the first workgroup) gets a NaN parameter: info bit 1 (the ROM's pivot test) and NaN in qoi_r for
    that sample alone; every other sample keeps the bits of the unpoisoned batch."""
    _, _, rom, ps, runs = cases(m, r)
    X, res = runs[S]
    Y = X.copy()
    Y[1, 2] = np.nan
    c = ps.solve_pairs(Y)
    assert rom._rom.last_epilogue() == "roomy"
    q, info = np.asarray(c["qoi_r"]), np.asarray(c["info"])
    assert info[1] & 2 and np.isnan(q[1]).all(), (info[1], q[1])
    good = np.setdiff1d(np.arange(S), [1])
    assert not info[good].any() and np.array_equal(q[good], res["qoi_r"][good])
