"""The COMPACT list on the device (DESIGN 4b'', finrom_rom_set_mirror_compact): the short list's rows rotated per pattern class, the
rotated rows below the gate's threshold left out.  Handles created under FINROM_ROM_COMPACT=1 offer it wherever the short list is
offered; a default handle offers it only to the pair path's large batches; FINROM_ROM_NO_COMPACT=1 never.  The kernels are the
short list's: a sample outside the gate's range, a sample that is flagged and every launch that keeps the full list (at r = 80 the
batches up to 64, which take the split-K projection) return the bits they returned before.
The compact list's A_r differs from the short list's by the truncated rows' squares, below an ulp of most entries; that the list
RAN shows in the handle's counts and in bits that differ somewhere in every batch that walks it."""
import itertools
import os

import numpy as np
import pytest

import rom_lspg_cases as Y
from test_gpu_rom_mirror import TWIN, _basis
from test_rom_compact_host import _desc_tables, _load
from test_rom_short_scale_free_host import _walk

pytestmark = pytest.mark.gpu
CASES = [(4, 16), (12, 80)]
SIZES = [1, 5, 64, 65, 301]
OUTSIDE, FLAGGED = 32, 33                                   # rows of the 301-sample batch behind its 32 corners


def _with_env(name, make):
    old = os.environ.get(name)
    os.environ[name] = "1"
    try:
        return make()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _batch(m, r, S):
    TH = np.exp(np.random.default_rng(100 * m + r + S).uniform(np.log(0.1), np.log(10.0), (S, 9)))[:, np.minimum(np.arange(9), TWIN)]
    if S == 301:
        TH[:32] = np.array(list(itertools.product((0.1, 10.0), repeat=5)))[:, np.minimum(np.arange(9), TWIN)]
        TH[OUTSIDE, [1, 7]] = 12.0
        TH[FLAGGED, 4] = np.nan
    return TH


@pytest.fixture(scope="module")
def cases(problems, spaces):
    """Per (m, r), once: the four handles and, per batch size, the batch with the four results."""
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    made = {}

    def get(m, r):
        if (m, r) not in made:
            V = spaces(m)
            phi = _basis(problems(m), r, "five")
            roms = {"default": AffineROMFin(V, None, phi)}
            for key, env in (("compact", "FINROM_ROM_COMPACT"), ("off", "FINROM_ROM_NO_COMPACT"), ("allrows", "FINROM_ROM_KEEP_ROWS")):
                roms[key] = _with_env(env, lambda: AffineROMFin(V, None, phi))
            runs = {}
            for S in SIZES:
                TH = _batch(m, r, S)
                runs[S] = (TH, {k: rom.forward_nine_param_reduced_batch(TH, want_state=True) for k, rom in roms.items()})
                for rom in roms.values():
                    assert rom._rom.last_form() == ("full" if r >= 49 and S <= 64 else "half")
            made[(m, r)] = (V, phi, roms, runs)
        return made[(m, r)]
    return get


def _same(a, b, rows=slice(None)):
    return all(np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k])[rows], equal_nan=True) for k in ("A_r", "B_r", "w_r", "qoi_r", "info"))


@pytest.mark.parametrize("m,r", CASES)
def test_counts_on_the_handles(cases, m, r):
    _, _, roms, _ = cases(m, r)
    c, s = roms["compact"]._rom.mirror_info(compact=True), roms["compact"]._rom.mirror_info(short=True)
    print(f"m = {m}, r = {r}: compact list {c[1]} k-steps for {c[0]} rows, short list {s[1]} for {s[0]}; "
          f"eps {roms['compact']._rom.mirror_eps_compact:.3e} (short {roms['compact']._rom.mirror_eps:.3e})")
    assert 0 < c[0] < s[0] and 0 < c[1] < s[1] and roms["compact"]._rom.mirror_eps_compact <= 1e-9
    assert roms["default"]._rom.mirror_info(compact=True) == c and roms["default"]._rom.mirror_info(short=True) == s
    assert roms["off"]._rom.mirror_info(compact=True) == (0, 0, 0) and roms["off"]._rom.mirror_info(short=True) == s
    assert roms["allrows"]._rom.mirror_info(compact=True) == (0, 0, 0) and roms["allrows"]._rom.mirror_info(short=True) == (0, 0, 0)


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("m,r", CASES)
def test_compact_list_against_its_own_lspg_and_the_other_handles(cases, m, r, S):
    """Measured, qoi_r against the compact list's own 80-bit LSPG (device / host64, largest over the sizes): (4, 16): 5.5e-14 /
    3.4e-14, (12, 80): 7.9e-14 / 3.0e-13; compact against short list, per entry: 3.1e-10 and 1.5e-9 (the corners of [0.1, 10]);
    norm(dA_r) / norm(A_r) between the two lists 5.9e-15."""
    V, phi, roms, runs = cases(m, r)
    TH, res = runs[S]
    got = res["compact"]
    # the switch: the default handle's bits at every S (finrom_rom_solve on a default handle keeps the short list)
    assert _same(res["off"], res["default"])
    if r >= 49 and S <= 64:                                  # the split-K projection: the full list on every handle
        assert _same(got, res["default"]) and _same(got, res["allrows"])
        return
    good = np.ones(S, bool)
    if S == 301:
        good[[OUTSIDE, FLAGGED]] = False
        # outside the gate's range, and flagged: what the handle with all rows returns, bit for bit
        assert _same(got, res["allrows"], [OUTSIDE, FLAGGED]) and _same(res["default"], res["allrows"], [OUTSIDE, FLAGGED])
        assert np.asarray(got["info"])[FLAGGED] != 0 and np.isnan(np.asarray(got["qoi_r"])[FLAGGED]).all()
    info = np.asarray(got["info"])
    assert not info[good].any() and np.array_equal(info, np.asarray(res["default"]["info"]))
    # in-range samples: the default handle's values to rtol 1e-7, other bits
    q, q0 = np.asarray(got["qoi_r"])[good], np.asarray(res["default"]["qoi_r"])[good]
    A, A0 = np.asarray(got["A_r"])[good], np.asarray(res["default"]["A_r"])[good]
    print(f"m = {m}, r = {r}, S = {S}: compact vs short list: max rel qoi_r {np.max(np.abs(q / q0 - 1.0)):.3e}, "
          f"max norm(dA_r)/norm(A_r) {np.max(np.linalg.norm(A - A0, axis=(1, 2)) / np.linalg.norm(A0, axis=(1, 2))):.3e}")
    assert np.allclose(q, q0, rtol=1e-7, atol=0.0)
    assert not np.array_equal(A, A0) and not np.array_equal(np.asarray(got["w_r"])[good], np.asarray(res["default"]["w_r"])[good])
    # qoi_r, Phi w_r against the 80-bit LSPG of the compact list's own rows; A_r against the NumPy walk of the builder's tables
    c = Y.Case.from_rom(roms["compact"], TH)
    form = c.form
    d, keep = form["desc_compact"], form["keep_compact"]
    Tc = _desc_tables(d, keep, d.P)[:, np.diff(np.asarray(keep[0][0])) > 0]
    full = np.zeros((10,) + Tc.shape[1:])
    full[:Tc.shape[0]] = Tc
    kw = dict(row_tables=list(full), rows=np.arange(Tc.shape[1]), weight=np.ones(Tc.shape[1]))
    tb = _load(d, keep, r)
    ss = [s for s in sorted({0, S // 3, S - 1})]
    result = {}
    for k in ("qoi_r", "Phi_w"):
        dd = dh = 0.0
        for s in ss:
            ref = Y.lspg_ld(c.tables, c.F, c.C, TH[s], phi=c.phi, **kw)
            h = Y.host64(c.tables, c.F, c.C, TH[s], phi=c.phi, **kw)
            x = np.asarray(got["w_r"])[s] @ c.phi.T if k == "Phi_w" else np.asarray(got[k])[s]
            dd, dh = max(dd, Y.dev(x, ref[k])), max(dh, Y.dev(h[k], ref[k]))
        result[k] = (dd, dh)
    assert Y.report(f"m = {m}, r = {r}, S = {S}: compact list against its own LSPG", result)
    for s in ss:
        want = _walk(tb, r, TH[s])
        assert np.linalg.norm(np.asarray(got["A_r"])[s] - want) <= 1e-12 * np.linalg.norm(want), s      # (the bound of the other lists' walks)


@pytest.mark.parametrize("m,r", CASES)
def test_pair_path_offers_the_compact_list_to_large_batches_only(spaces, cases, m, r):
    """finrom_solve_pairs on a default handle: at S = 16 384 (the batches whose sweep is masked by default) the compact list is
    walked -- fewer k-steps than the short list on the handle, qoi_r within 1e-7 of the FINROM_ROM_NO_COMPACT=1 handle's and not
    its bits, qoi / theta / info bit for bit --, at S = 4096 every output is that handle's bits."""
    from bayesianinferencedl_amd.pairs import FinPairSolver
    V, phi, roms, _ = cases(m, r)
    e = roms["default"]._rom
    assert 0 < e.mirror_info(compact=True)[1] < e.mirror_info(short=True)[1]
    ps = FinPairSolver(V, phi, params="five", solver_r=roms["default"])
    ps_off = FinPairSolver(V, phi, params="five", solver=ps.solver, solver_r=roms["off"])
    for S in (16384, 4096):
        X = np.random.default_rng(S + m).uniform(0.1, 10.0, (S, 5))
        a, b = ps.solve_pairs(X), ps_off.solve_pairs(X)
        assert e.last_form() == roms["off"]._rom.last_form() == "half" and e.last_epilogue() == roms["off"]._rom.last_epilogue()
        for key in ("qoi", "theta", "info"):
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (S, key)
        assert not np.asarray(a["info"]).any()
        qa, qb = np.asarray(a["qoi_r"]), np.asarray(b["qoi_r"])
        print(f"m = {m}, r = {r}, S = {S}: pair path, compact vs short: max rel qoi_r {np.max(np.abs(qa / qb - 1.0)):.3e}")
        if S == 4096:
            assert np.array_equal(qa, qb) and np.array_equal(np.asarray(a["err"]), np.asarray(b["err"]))
        else:
            assert np.allclose(qa, qb, rtol=1e-7, atol=0.0) and not np.array_equal(qa, qb)
