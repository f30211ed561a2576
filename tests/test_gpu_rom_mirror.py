"""The projection on HALF the rows for mirror-symmetric reduced models (finrom_rom_set_mirror, DESIGN 4b'): with a basis from
five-parameter snapshots, a sample whose nine sub-fin conductivities mirror about x = 3 walks the half list (the left rows twice,
the centre line once, on the symmetrised basis) instead of all rows.  Against a handle created with FINROM_ROM_NO_MIRROR=1 and
against the oracle, the per-sample fallback inside one launch, the QoI-only form, and the sample-pair path."""
import os

import numpy as np
import pytest

import rom_lspg_cases as Y
from oracle import fin_oracle as O

pytestmark = pytest.mark.gpu
S = 301                                                   # 76 workgroups of four samples, the last one with a single live wave
CASES = [(4, 16), (12, 33), (12, 80)]
TWIN = np.array([8, 7, 6, 5, 4, 3, 2, 1, 0])


def _without_mirror(make):
    old = os.environ.get("FINROM_ROM_NO_MIRROR")
    os.environ["FINROM_ROM_NO_MIRROR"] = "1"
    try:
        return make()
    finally:
        if old is None:
            del os.environ["FINROM_ROM_NO_MIRROR"]
        else:
            os.environ["FINROM_ROM_NO_MIRROR"] = old


_SNAPSHOTS = {}


def _basis(prob, r, kind):
    """POD basis of 400 oracle snapshots of U(0.1, 10) parameters, seed 1 (the benchmark's recipe); snapshots once per mesh."""
    key = (prob.m if hasattr(prob, "m") else id(prob), kind)
    if key not in _SNAPSHOTS:
        fo = O.FinOracle(prob)
        rng = np.random.default_rng(1)
        lift = fo.five_param_to_function if kind == "five" else fo.nine_param_to_function
        _SNAPSHOTS[key] = np.array([fo.forward(lift(rng.uniform(0.1, 10.0, 5 if kind == "five" else 9))) for _ in range(400)])
    return O.pod_basis(_SNAPSHOTS[key], r)


@pytest.fixture(scope="module")
def cases(problems, spaces):
    """Per (m, r), once: the basis of five-parameter oracle snapshots, the model with the half list, the model created with the
    switch set, a mirror-symmetric batch in [0.1, 10] and both results with the state."""
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    made = {}

    def get(m, r):
        if (m, r) not in made:
            prob, V = problems(m), spaces(m)
            phi = _basis(prob, r, "five")
            rom = AffineROMFin(V, None, phi)
            assert rom._rom.mirror, f"half list not installed (eps_probe {rom._rom.mirror_eps})"
            full = _without_mirror(lambda: AffineROMFin(V, None, phi))
            assert not full._rom.mirror
            assert list(rom.mirror_form(V.operators(), rom._psi_tables)["twin"]) == list(TWIN)
            rng = np.random.default_rng(100 * m + r)
            TH = np.exp(rng.uniform(np.log(0.1), np.log(10.0), (S, 9)))
            TH = TH[:, np.minimum(np.arange(9), TWIN)]
            res = rom.forward_nine_param_reduced_batch(TH, want_state=True)
            assert rom._rom.last_form() == "half"
            ref = full.forward_nine_param_reduced_batch(TH, want_state=True)
            assert full._rom.last_form() == "full"
            made[(m, r)] = (prob, phi, rom, full, TH, res, ref)
        return made[(m, r)]
    return get


def _close(a, b):
    """Two forms on in-range samples: each is held to its allowance of the extended-precision yardstick (tests/test_gpu_rom_lspg.py,
    test_half_form_matches_full_form_and_oracle below), which the inputs keep at or under 1e-10; hence within 2e-10 of each other,
    per sample and relative in the 2-norm."""
    a, b = np.atleast_2d(np.asarray(a)), np.atleast_2d(np.asarray(b))
    return bool(np.all(np.linalg.norm(a - b, axis=-1) <= 2.0 * Y.CAP * np.linalg.norm(b, axis=-1)))


@pytest.mark.parametrize("m,r", CASES)
def test_half_form_matches_full_form_and_oracle(cases, m, r):
    """Measured, qoi_r (device / host64): the list that ran against its own 80-bit LSPG on four samples: (4, 16): 9.3e-14 / 9.2e-14,
    (12, 33): 6.3e-13 / 3.0e-12, (12, 80): 3.3e-13 / 4.8e-13; the full handle against QR on all 301: 5.2e-12 / 5.5e-12,
    8.0e-12 / 8.4e-12, 1.1e-11 / 8.7e-12."""
    prob, phi, rom, full, TH, res, ref = cases(m, r)
    A, A0 = np.asarray(res["A_r"]), np.asarray(ref["A_r"])
    assert np.array_equal(np.asarray(res["info"]), np.asarray(ref["info"])) and not np.asarray(res["info"]).any()
    dA = np.max(np.abs(A - A0)) / np.max(np.abs(A0))
    dq = np.max(np.abs(np.asarray(res["qoi_r"]) / np.asarray(ref["qoi_r"]) - 1.0))
    print(f"m = {m}, r = {r}: eps_probe {rom._rom.mirror_eps:.3e}, half vs full: max|dA_r|/max|A_r| {dA:.3e}, max rel qoi_r {dq:.3e}")
    assert dA < 1e-12
    assert not np.array_equal(A, A0)                         # another sum: the half list did run
    ro = O.AffineROMOracle(prob, phi)
    for s in (0, 77, 150, 300):
        w, Ar, Br, _ = ro.forward_nine_param_reduced(TH[s], return_parts=True)
        assert np.linalg.norm(A[s] - Ar) < 1e-12 * np.linalg.norm(Ar), s
    # each form against the extended-precision LSPG of ITS OWN list (tests/rom_lspg_cases.py), within max(8 d_host, 1e-12): the
    # handle with the half list -- whose in-range samples walk the short list where one is installed -- on four samples, the full
    # handle on the same four and, by the QR yardstick, on all; then the two against each other on every sample, within the two
    # allowances added (the lists' own LSPGs differ by 1.5e-14 at most, tests/test_rom_lspg_host.py)
    c = Y.Case.from_rom(full, TH)
    own = "short" if rom._rom.mirror_dropped else "half"
    r_own = c.against_ld(res, (0, 77, 150, 300), ("qoi_r", "Phi_w"), form=own)
    r_full = c.against_ld(ref, (0, 77, 150, 300), ("qoi_r", "Phi_w"))
    r_all = c.against_qr(ref, S, ("qoi_r", "Phi_w"))
    assert Y.report(f"m = {m}, r = {r}: {own} list against its own LSPG", r_own)
    assert Y.report(f"m = {m}, r = {r}: full list, 80-bit", r_full) and Y.report(f"m = {m}, r = {r}: full list, QR on all", r_all)
    for key, k in (("qoi_r", "qoi_r"), ("w_r", "Phi_w")):
        a, b = np.asarray(res[key]), np.asarray(ref[key])
        if key == "w_r":
            a, b = a @ phi.T, b @ phi.T
        d = np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1))
        assert d <= Y.allowance(r_own[k][1]) + Y.allowance(r_all[k][1]), (key, d)


def _mixed_batch(TH):
    """Samples that must take the half list (0: one entry 1 ulp off its twin) and samples that must not."""
    X = TH.copy()
    X[0, 8] = np.nextafter(X[0, 0], np.inf)
    X[1, 8] = X[1, 0] * (1.0 + 1e-10)
    X[2] = np.random.default_rng(9).uniform(0.1, 10.0, 9)
    X[3, 2] = X[3, 6] = np.nan
    X[150, 1] = X[150, 7] = 0.0
    X[300, 4] = 1e61
    return X, [1, 2, 3, 150, 300]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("m,r", CASES)
def test_samples_that_do_not_mirror_keep_the_full_loop(cases, m, r):
    """One launch, decided per sample: 1 ulp between a parameter and its twin still takes the half list; 1e-10 relative, a generic
    nine-parameter sample, and NaN / 0.0 / 1e61 (mirrored: what sends them away is the grouped form's own test) run the loop they
    ran before -- the same bits as the handle without the half list, flags included."""
    _, _, rom, full, TH, res, ref = cases(m, r)
    X, keep_full = _mixed_batch(TH)
    a = rom.forward_nine_param_reduced_batch(X, want_state=True)
    assert rom._rom.last_form() == "half"
    b = full.forward_nine_param_reduced_batch(X, want_state=True)
    assert _same(a["info"], b["info"])
    for key in ("A_r", "B_r", "w_r", "qoi_r"):
        assert _same(np.asarray(a[key])[keep_full], np.asarray(b[key])[keep_full]), key
    assert not np.array_equal(np.asarray(a["A_r"])[0], np.asarray(b["A_r"])[0])
    assert _close(np.asarray(a["qoi_r"])[0], np.asarray(b["qoi_r"])[0])
    rest = np.setdiff1d(np.arange(S), keep_full + [0])
    assert _same(np.asarray(a["A_r"])[rest], np.asarray(res["A_r"])[rest])      # the neighbours are what they were


@pytest.mark.parametrize("m,r", CASES)
def test_qoi_only_form(cases, m, r):
    _, _, rom, full, TH, res, ref = cases(m, r)
    X, keep_full = _mixed_batch(TH)
    a = rom.forward_nine_param_reduced_batch(X, want_w=False)
    assert rom._rom.last_form() == "half"
    b = full.forward_nine_param_reduced_batch(X, want_w=False)
    assert _same(a["info"], b["info"])
    assert _same(np.asarray(a["qoi_r"])[keep_full], np.asarray(b["qoi_r"])[keep_full])
    ok = np.setdiff1d(np.arange(S), [3, 150, 300])
    assert _close(np.asarray(a["qoi_r"])[ok], np.asarray(b["qoi_r"])[ok])
    assert not np.array_equal(np.asarray(a["qoi_r"])[ok], np.asarray(b["qoi_r"])[ok])
    rest = np.setdiff1d(np.arange(S), keep_full + [0])
    assert _close(np.asarray(a["qoi_r"])[rest], np.asarray(ref["qoi_r"])[rest])


@pytest.mark.parametrize("m,r", CASES)
def test_pair_path_with_five_parameters(spaces, cases, m, r):
    from bayesianinferencedl_amd.pairs import FinPairSolver
    _, phi, rom, full, _, _, _ = cases(m, r)
    V = spaces(m)
    X = np.random.default_rng(3).uniform(0.1, 10.0, (S, 5))
    ps = FinPairSolver(V, phi, params="five", solver_r=rom)
    a = ps.solve_pairs(X)
    assert rom._rom.last_form() == "half"
    b = FinPairSolver(V, phi, params="five", solver=ps.solver, solver_r=full).solve_pairs(X)
    assert full._rom.last_form() == "full"
    for key in ("qoi", "theta", "info"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert not np.asarray(a["info"]).any()
    qa, qb = np.asarray(a["qoi_r"]), np.asarray(b["qoi_r"])
    assert _close(qa, qb) and not np.array_equal(qa, qb)
    assert np.allclose(qa[:, ::-1], qa, rtol=1e-7, atol=0.0)      # (the basis' own asymmetry, not rounding: as it was)


def test_nine_parameter_basis_installs_nothing(problems, spaces):
    """A basis from nine-parameter snapshots fails the gate by orders of magnitude: the handle is the one a set switch gives, and
    the nine-parameter pair path returns the same bits."""
    from bayesianinferencedl_amd.pairs import FinPairSolver
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    m, r = 12, 33
    prob, V = problems(m), spaces(m)
    phi = _basis(prob, r, "nine")
    rom = AffineROMFin(V, None, phi)
    assert not rom._rom.mirror and rom._rom.mirror_eps > 1e-6
    full = _without_mirror(lambda: AffineROMFin(V, None, phi))
    assert full._rom.mirror_eps is None
    X = np.random.default_rng(4).uniform(0.1, 10.0, (S, 9))
    ps = FinPairSolver(V, phi, params="nine", solver_r=rom)
    a = ps.solve_pairs(X, want_w_r=True)
    assert rom._rom.last_form() == "full"
    b = FinPairSolver(V, phi, params="nine", solver=ps.solver, solver_r=full).solve_pairs(X, want_w_r=True)
    for key in ("qoi", "qoi_r", "err", "w_r", "theta", "info"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
