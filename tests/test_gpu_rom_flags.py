"""The failure side of the dispatch table of csrc/api_rom.hip: every form finrom_rom_solve and finrom_rom_grad take, run with poisoned
samples and held to the flagged-sample contract of tests/flag_cases.py ("What a flagged sample is held to"):
exactly the poisoned samples flagged with bit 2, their qoi_r / J / g NaN in every entry and their w_r not all finite, and every other
sample's every output -- qoi_r, w_r, A_r, B_r, J, g -- the bits of the same call on the clean batch (same handle, same S, same
last_form() / last_epilogue()).  No yardstick here: tests/test_gpu_rom_lspg.py holds the clean batches' accuracy.

Handles and batches are those of tests/rom_lspg_cases.py (Y.case, c.TH, Case.NARROW where it applies).  Poisons: one entry NaN, +inf,
1e200, the whole row 1e200, at rows {1} (S = 3), {4, 9, 63} (S = 64), {4, 9, 21, S - 1} (S >= 65), rotated by case; gradients with
per-sample data also a NaN in a sample's DATA row (info stays 0, qoi_r and w_r keep their bits, J and g are NaN).
Once per kernel family: clean, poisoned, clean, and a clean call four samples shorter on one handle return the first call's bits (no
residue in the grow-only scratch, the arrival counters of the gradient's small contraction back at zero); a prefilled info is OR-ed
into; and both piece loops with s0 > 0 (FINROM_ROM_WORKSPACE_BYTES).  Every test prints the form taken, the kinds of poison and the
rows it compared.
Measured on the MI355X: no form violated the contract -- +inf and the overflowing 1e200 are flagged by every kernel, no NaN crosses
from a sample to its tile or pair neighbours, no flagged w_r row has a finite entry, the arrival counters are back at zero."""
import contextlib
import os

import numpy as np
import pytest

import flag_cases as F
import rom_lspg_cases as Y

pytestmark = pytest.mark.gpu
VARIANTS = (("w_r", {}), ("QoI-only", {"want_w": False}), ("state", {"want_state": True}))


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def models(spaces):
    """(AffineROMFin, Case) per (m, r, basis, creation switch, observations, projection), made once (as tests/test_gpu_rom_lspg.py)."""
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    made = {}

    def get(m, r, kind="parity", env=None, external_obs=False, projection=None):
        key = (m, r, kind, env, external_obs, projection)
        c = Y.case(m, r, kind, external_obs)
        if key not in made:
            with _env(**({env: "1"} if env else {})):
                made[key] = AffineROMFin(spaces(m), None, c.phi, external_obs=external_obs, projection=projection)
        return made[key], c
    return get


def _form(eng):
    return eng.last_form(), eng.last_epilogue()


def _keys(out):
    return tuple(k for k in out if k != "info")


def _solve_pair(label, rom, TH, S, case_id, kw, form="full"):
    """The same finrom_rom_solve call on the clean and on the poisoned batch -> (clean, poisoned batch, bad rows)."""
    eng = rom._rom
    clean = eng.solve(TH[:S], **kw)
    f0 = _form(eng)
    dirty_TH, bad = F.poisoned(TH, S, case_id)
    dirty = eng.solve(dirty_TH, **kw)
    assert _form(eng) == f0 == (form, "standard"), (label, f0, _form(eng))
    kinds = F.kinds_at(S, case_id)
    F.check_contract(f"{label}, S = {S}, form {f0}, poisons {dict(zip(bad, kinds))}", clean, dirty, bad, _keys(clean), F.ROM_FLAG)
    return clean, dirty_TH, bad


def _raw(eng, name, TH, info0, data=None, want_w=True, want_state=False):
    """finrom_rom_solve / finrom_rom_grad through the C ABI with the caller's own info -> info after the call."""
    from bayesianinferencedl_amd._ffi import DeviceBuffer, check, lib
    S = len(TH)
    th = DeviceBuffer.from_numpy(np.ascontiguousarray(TH, np.float64))
    info = DeviceBuffer.from_numpy(np.ascontiguousarray(info0, np.int32))
    w, q = DeviceBuffer(S * eng.r * 8), DeviceBuffer(S * eng.n_obs * 8)
    if name == "solve":
        A, B = (DeviceBuffer(S * eng.r * eng.r * 8), DeviceBuffer(S * eng.r * 8)) if want_state else (None, None)
        check(lib().finrom_rom_solve(eng._h, th.ptr, S, w.ptr if want_w else None, q.ptr, A.ptr if A else None, B.ptr if B else None,
                                     info.ptr, None), "finrom_rom_solve")
    else:
        d = DeviceBuffer.from_numpy(np.ascontiguousarray(data, np.float64))
        J, g = DeviceBuffer(S * 8), DeviceBuffer(S * eng.P * 8)
        check(lib().finrom_rom_grad(eng._h, th.ptr, d.ptr, int(np.ndim(data) == 2), S, J.ptr, g.ptr, w.ptr, q.ptr, info.ptr, None),
              "finrom_rom_grad")
    return info.to_numpy((S,), np.int32)


def _no_residue(label, eng, TH, dirty_TH, bad, S, first, kw=None, data=None):
    """Items 4 and 5, once per kernel family.  kw: finrom_rom_solve with these options, data: finrom_rom_grad with this data (per-sample
    data is cut to the batch).  `first` = the clean call that came before the poisoned one on this handle.  A clean call after the
    poisoned one returns the same bits, and so does one four samples (a workgroup) shorter -- the per-sample bits of every form here
    do not depend on S within the form's range -- in the same form.  Then the poisoned batch with 0x40 prefilled in info at a clean row
    (5) and at a poisoned one (9): 0x40 and 0x42 come back, every other row as from a zeroed info -- this family's reporting sites OR
    and nothing in front of them clears."""
    def call(th):
        return eng.solve(th, **kw) if data is None else eng.grad(th, data[:len(th)] if np.ndim(data) == 2 else data)
    keys = _keys(first)
    call(dirty_TH)
    f0 = _form(eng)
    F.same_bits(f"{label}: clean after poisoned", first, call(TH[:S]), keys)
    assert _form(eng) == f0
    F.same_bits(f"{label}: S - 4 after poisoned", first, call(TH[:S - 4]), keys, rows=S - 4)
    assert _form(eng) == f0, (label, f0, _form(eng))
    assert 9 in bad and 5 not in bad
    pre = np.zeros(S, np.int32)
    pre[[5, 9]] = 0x40
    want = pre.copy()
    want[bad] |= F.ROM_FLAG
    got = _raw(eng, "solve", dirty_TH, pre, **kw) if data is None else _raw(eng, "grad", dirty_TH, pre, data=data)
    assert _form(eng) == f0
    assert got[5] == 0x40 and got[9] == 0x42 and np.array_equal(got, want), (label, got.tolist())
    print(f"{label}: clean, poisoned, clean at S = {S} and clean at S = {S - 4}: the first call's bits, form {f0}; "
          f"0x40 prefilled in rows 5, 9 -> {got[5]:#x}, {got[9]:#x}")


# ---- finrom_rom_solve ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 64])
@pytest.mark.parametrize("r", [33, 96])
def test_solve_one_sample_kernels(models, r, S):
    """rom_small_proj_kernel + rom_small_solve_kernel (batches of <= 64 without the state), with w_r and QoI-only."""
    rom, c = models(12, r)
    for i, (name, kw) in enumerate(VARIANTS[:2]):
        clean, dirty_TH, bad = _solve_pair(f"solve, one-sample kernels, r = {r}, {name}", rom, c.TH, S, 2 * (r == 96) + i, kw)
        if (r, S, i) == (33, 64, 0):                      # (`clean` came before this test's first poisoned call)
            _no_residue("solve, one-sample kernels, r = 33", rom._rom, c.TH, dirty_TH, bad, S, clean, kw=kw)


@pytest.mark.parametrize("r", [64, 96])
def test_solve_split_k_with_the_state(models, r):
    """rom_proj_splitk_kernel + rom_solve_kernel: S = 64 with the state."""
    rom, c = models(12, r)
    S, kw = 64, {"want_state": True}
    clean, dirty_TH, bad = _solve_pair(f"solve, split-K with the state, r = {r}", rom, c.TH, S, r // 32, kw)
    assert set(clean) == {"qoi_r", "w_r", "A_r", "B_r", "info"}
    if r == 64:
        _no_residue("solve, split-K with the state, r = 64", rom._rom, c.TH, dirty_TH, bad, S, clean, kw=kw)


@pytest.mark.parametrize("m,r,env", [(4, 16, None), (12, 80, None), (4, 16, "FINROM_PROJ_UNGROUPED")])
def test_solve_grouped_one_wave_kernel(models, m, r, env):
    """rom_proj_single_kernel at S = 65 (grouped k-steps; the FINROM_PROJ_UNGROUPED handle in table order): the fused solve,
    QoI-only, and with the state (rom_solve_kernel)."""
    rom, c = models(m, r, env=env)
    for i, (name, kw) in enumerate(VARIANTS):
        _solve_pair(f"solve, {'ungrouped' if env else 'grouped'} one-wave, (m, r) = ({m}, {r}), {name}", rom, c.TH, 65, i + m, kw)
    if (m, r, env) == (12, 80, None):
        S = 70
        first, dirty_TH, bad = _solve_pair("solve, grouped one-wave, (12, 80), w_r", rom, c.TH, S, 3, {})
        _no_residue("solve, grouped one-wave, (12, 80)", rom._rom, c.TH, dirty_TH, bad, S, first, kw={})


def test_solve_in_register_factor_six_blocks(models):
    """r = 96, S = 65: rom_proj_kernel<6, 1> factors in registers, rom_subst_blocked_kernel substitutes; with the state
    rom_solve_kernel."""
    rom, c = models(12, 96)
    for i, (name, kw) in enumerate(VARIANTS):
        _solve_pair(f"solve, in-register six blocks, r = 96, {name}", rom, c.TH, 65, i + 1, kw)
    S = 70
    first, dirty_TH, bad = _solve_pair("solve, in-register six blocks, r = 96, w_r", rom, c.TH, S, 0, {})
    _no_residue("solve, in-register six blocks, r = 96", rom._rom, c.TH, dirty_TH, bad, S, first, kw={})


@pytest.mark.parametrize("r", [120, 128, 200])
def test_solve_wide_bases(models, r):
    """S = 70: r = 120 the HalfCover projection, 128 the aligned one, 200 the factor in global memory; want_w: rom_chol_blocked_kernel
    + rom_subst_blocked_kernel, QoI-only: fused_solve_mw, with the state: rom_solve_kernel."""
    rom, c = models(12, r)
    S = 70
    for i, (name, kw) in enumerate(VARIANTS):
        clean, dirty_TH, bad = _solve_pair(f"solve, wide, r = {r}, {name}", rom, c.TH, S, i + r // 8, kw)
        # r = 120: the blocked Cholesky family and the factor in the projection's registers; r = 128: the aligned projection;
        # r = 200 with the state: rom_solve_kernel with the factor in global memory
        if (r == 120 and name != "state") or (r == 128 and name == "QoI-only") or (r == 200 and name == "state"):
            _no_residue(f"solve, wide, r = {r}, {name}", rom._rom, c.TH, dirty_TH, bad, S, clean, kw=kw)


def test_solve_half_and_short_lists(models):
    """The benchmark-recipe basis at (4, 16), S = 65, the clean batch mirror-symmetric: the default handle's samples walk the short
    list, a FINROM_ROM_KEEP_ROWS handle's the half list with all rows; a poisoned sample fails the mirror test (or not: the whole
    row 1e200 is mirror-symmetric) and walks another list, which changes nothing in what is asserted."""
    rom, c = models(4, 16, "bench")
    keep, _ = models(4, 16, "bench", env="FINROM_ROM_KEEP_ROWS")
    assert rom._rom.mirror and keep._rom.mirror and rom._rom.mirror_dropped > 0 and keep._rom.mirror_dropped == 0
    for which, h in (("short list", rom), ("half list", keep)):
        for i, (name, kw) in enumerate(VARIANTS):
            _solve_pair(f"solve, {which}, (4, 16), {name}", h, c.TH, 65, i + (which == "half list"), kw, form="half")
    S = 70
    for which, h in (("short list", rom), ("half list", keep)):
        first, dirty_TH, bad = _solve_pair(f"solve, {which}, (4, 16), w_r", h, c.TH, S, 2, {}, form="half")
        _no_residue(f"solve, {which}, (4, 16)", h._rom, c.TH, dirty_TH, bad, S, first, kw={})


@pytest.mark.parametrize("S", [65, 70])
@pytest.mark.parametrize("m,r", [(4, 8), (12, 80), (12, 120)])
def test_solve_offline_online(models, m, r, S):
    """projection='offline_online': rom_gram_kernel (two samples per wave: a poisoned sample's partner is among the neighbours) at
    r = 8 and 80, rom_gram_store_kernel + the blocked Cholesky and substitution kernels at r = 120."""
    rom, c = models(m, r, projection="offline_online")
    assert rom.projection == "offline_online"
    for i, (name, kw) in enumerate(VARIANTS):
        clean, dirty_TH, bad = _solve_pair(f"solve, offline/online, (m, r) = ({m}, {r}), {name}", rom, c.TH, S, i + S + r, kw)
        if S == 70 and m == 12 and name == "w_r":
            _no_residue(f"solve, offline/online, r = {r}", rom._rom, c.TH, dirty_TH, bad, S, clean, kw=kw)


# ---- finrom_rom_grad -------------------------------------------------------------------------------------------------------------
GRAD_KEYS = ("J", "g", "w_r", "qoi_r")


def _grad_case(label, rom, c, S, case_id, residue=False):
    """Shared data and per-sample data on one handle, each clean and with poisoned theta; per-sample data also with a NaN in the
    data rows at the same positions and a clean theta.  residue: item 4 with per-sample data (the third call is also the check that
    the arrival counters of the small contraction went back to zero: the summing workgroup is chosen by count)."""
    rom._ensure_gradient()
    eng = rom._rom
    TH, D = c.TH, c.D
    for per_sample, data in ((False, c.data), (True, D[:S])):
        kind = "per-sample data" if per_sample else "shared data"
        clean = eng.grad(TH[:S], data)
        f0 = _form(eng)
        assert f0 == ("full", "standard") and set(clean) == set(GRAD_KEYS) | {"info"}
        dirty_TH, bad = F.poisoned(TH, S, case_id + per_sample)
        dirty = eng.grad(dirty_TH, data)
        assert _form(eng) == f0
        kinds = F.kinds_at(S, case_id + per_sample)
        F.check_contract(f"{label}, S = {S}, {kind}, form {f0}, poisons {dict(zip(bad, kinds))}", clean, dirty, bad, GRAD_KEYS, F.ROM_FLAG)
        if not per_sample:
            continue
        rows = F.positions(S)
        Dn = D[:S].copy()
        for i, s in enumerate(rows):
            Dn[s, (case_id + 2 * i) % Dn.shape[1]] = np.nan
        dirty = eng.grad(TH[:S], Dn)
        assert _form(eng) == f0
        F.check_contract(f"{label}, S = {S}, form {f0}, NaN in the data rows {rows}", clean, dirty, [], GRAD_KEYS, F.ROM_FLAG, data_bad=rows)
        if residue:
            _no_residue(f"{label}, per-sample data", eng, TH, dirty_TH, bad, S, clean, data=D[:S])


@pytest.mark.parametrize("S", [3, 64])
@pytest.mark.parametrize("r", [33, 81])
def test_gradient_one_sample_kernels(models, r, S):
    """rom_small_proj_kernel + rom_small_solve_kernel + rom_grad_contract_small_kernel (36 workgroups per sample, arrival counters)."""
    rom, c = models(12, r)
    _grad_case(f"gradient, one-sample kernels, r = {r}", rom, c, S, (r == 81) + 2 * (S == 64), residue=(r, S) == (81, 64))


def test_gradient_split_k_form_with_forty_observations(models):
    """The 40 point observations (no one-sample kernels): the adjoint gradient in rom_proj_splitk_kernel (factor 4) +
    rom_grad_contract_small_kernel, S = 64."""
    (m, r), _ = Y.GRAD40
    rom, c = models(m, r, external_obs=True)
    assert rom.n_obs == 40
    _grad_case(f"gradient, split-K form, 40 observations, r = {r}", rom, c, 64, 1, residue=True)


@pytest.mark.parametrize("projection", ["direct", "offline_online"])
@pytest.mark.parametrize("r", [80, 120])
def test_gradient_batched_contraction(models, r, projection):
    """S = 70: the projection writes the factor, rom_subst_blocked_kernel does both solves, rom_grad_contract_kernel contracts 16
    samples per MFMA tile: row 21 sits in the middle of the second tile, row 69 in the ragged fifth."""
    rom, c = models(12, r, projection=None if projection == "direct" else projection)
    assert rom.projection == projection
    _grad_case(f"gradient, batched contraction, {projection}, r = {r}", rom, c, 70, r // 40 + (projection == "direct"),
               residue=True)


# ---- a prefilled info ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 70])
def test_a_prefilled_info_is_ored_into(models, S):
    """finrom_rom_solve and finrom_rom_grad OR bit 2 into the info they are given and clear nothing (include/finrom.h): 0x40 in a
    clean row (5) and in a poisoned one (9) comes back as 0x40 and 0x42; every other row as from a zeroed info.  S = 64: the
    one-sample kernels, S = 70: the grouped one-wave kernel / the batched contraction."""
    rom, c = models(12, 80)
    rom._ensure_gradient()
    eng = rom._rom
    TH, bad = F.poisoned(c.TH, S, 1)
    pre = np.zeros(S, np.int32)
    pre[[5, 9]] = 0x40
    want = pre.copy()
    want[bad] |= F.ROM_FLAG
    assert want[9] == 0x42 and want[5] == 0x40
    for name, data in (("solve", None), ("grad", c.data), ("grad", c.D[:S])):
        got = _raw(eng, name, TH, pre, data)
        print(f"prefilled info, finrom_rom_{name}, S = {S}: rows 5, 9 -> {got[5]:#x}, {got[9]:#x}")
        assert np.array_equal(got, want), (name, got.tolist())


def test_a_prefilled_info_on_the_pair_path_is_ored_into(spaces):
    """finrom_solve_pairs ORs bit 1 (FOM half) and bit 2 (ROM half) into the info it is given: m = 4, r = 16, nine fin conductivities,
    S = 70, a NaN conductivity in rows 9 and 69: 0x40 in row 5 stays 0x40, in row 9 it comes back as 0x43."""
    from bayesianinferencedl_amd._ffi import DeviceBuffer, check, lib
    from bayesianinferencedl_amd.pairs import FinPairSolver
    c = Y.case(4, 16)
    ps = FinPairSolver(spaces(4), c.phi, params="nine")
    S = 70
    X = np.random.default_rng(5).uniform(0.5, 2.0, (S, 9))
    X[9, 2] = np.nan
    X[69, 7] = np.nan
    plain = np.asarray(ps.solve_pairs(X)["info"])
    assert np.nonzero(plain)[0].tolist() == [9, 69] and plain[9] == plain[69] == 3
    pre = np.zeros(S, np.int32)
    pre[[5, 9]] = 0x40
    fom, rom = ps.solver._engine("nine"), ps.solver_r._rom
    x, info = DeviceBuffer.from_numpy(X), DeviceBuffer.from_numpy(pre)
    q, qr, err = (DeviceBuffer(8 * S * ps.n_obs) for _ in range(3))
    check(lib().finrom_solve_pairs(fom._h, rom._h, ps._avg._S.ptr, x.ptr, S, q.ptr, qr.ptr, err.ptr, None, None, None, info.ptr, None),
          "finrom_solve_pairs")
    got = info.to_numpy((S,), np.int32)
    print(f"prefilled info, finrom_solve_pairs: rows 5, 9 -> {got[5]:#x}, {got[9]:#x}")
    assert got[5] == 0x40 and got[9] == 0x43 and np.array_equal(got, pre | plain)


@pytest.mark.parametrize("name", ["one-staged-w16", "b1-ref-S65"])
def test_a_prefilled_info_is_overwritten_by_romml_grad(spaces, name):
    """finrom_romml_grad is the one entry point that OVERWRITES info (the one-sample form stores 0 or 2, the batched forms clear it in
    front of their kernels): 0x40 in a clean row (0) comes back as 0, in a poisoned row (1: a NaN in the field) as the flag alone --
    which is why engine.romml_grad may hand it an uninitialised info (zero=False)."""
    import mlp_cases as K
    from bayesianinferencedl_amd._ffi import DeviceBuffer, check, lib
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    c = K.FUSED_BY_NAME[name]
    assert c.P == 9 and c.projection == "direct" and not c.per_sample
    _, phi, _ = K.oracle_rig(c.m, c.r, c.n_obs)
    rom = AffineROMFin(spaces(c.m), None, phi, external_obs=(c.n_obs == 40))
    rom._ensure_gradient()
    mlp = DeviceErrorModel(K.fused_model(c))
    S, n = c.S, K.MESH_N[c.m]
    Kf, data = K.rom_inputs(n, S, seed=3), K.fused_data(c)
    Kf[1, 7] = np.nan
    k, d = DeviceBuffer.from_numpy(Kf), DeviceBuffer.from_numpy(np.ascontiguousarray(data, np.float64))
    grad, loss, q, e = DeviceBuffer(8 * S * n), DeviceBuffer(8 * S), DeviceBuffer(8 * S * c.n_obs), DeviceBuffer(8 * S * c.n_obs)
    got = {}
    for fill in (0, 0x40):
        pre = np.zeros(S, np.int32)
        pre[[0, 1]] = fill
        info = DeviceBuffer.from_numpy(pre)
        check(lib().finrom_romml_grad(rom._rom._h, mlp._h, rom._avg._S.ptr, k.ptr, d.ptr, 0, S, grad.ptr, loss.ptr, q.ptr, e.ptr, info.ptr,
                                      None), "finrom_romml_grad")
        got[fill] = info.to_numpy((S,), np.int32)
    print(f"prefilled info, finrom_romml_grad, {name}: rows 0, 1 -> {got[0x40][0]:#x}, {got[0x40][1]:#x}")
    assert np.nonzero(got[0])[0].tolist() == [1] and got[0][1] == F.ROM_FLAG
    assert np.array_equal(got[0x40], got[0])


# ---- pieces ----------------------------------------------------------------------------------------------------------------------


def _pieces(S, bound, per_sample, equal):
    """The piece loop of rom_solve_impl (equal pieces) / finrom_rom_grad (whole pieces, then the rest) as csrc/api_rom.hip cuts it."""
    chunk = max(4, bound // per_sample // 4 * 4)
    if equal and S > chunk:
        n = -(-S // chunk)
        chunk = (-(-S // n) + 3) // 4 * 4
    return [(s0, min(s0 + chunk, S)) for s0 in range(0, S, chunk)]


@pytest.mark.parametrize("row", [64, 44])
def test_solve_in_pieces(models, row):
    """finrom_rom_solve with the state, r = 80, S = 130, FINROM_ROM_WORKSPACE_BYTES at 64 samples' worth: rom_solve_impl makes equal
    pieces, 44 + 44 + 42 (finrom_rom_grad, below, cuts 64 + 64 + 2), so theta, w_r, qoi_r, A_r, B_r and info are offset with
    s0 = 44 and 88.  One poisoned sample: row 64 (inside the second piece) and row 44 (its first sample).  A piece chooses its form by
    its own size -- 44 samples with the state take the split-K projection, 130 the grouped one-wave kernel -- so every piece is
    compared bit for bit with a separate call on its slice, never with the one-piece call, whose bits must differ."""
    rom, c = models(12, 80)
    eng, S = rom._rom, 130
    cuts = _pieces(S, 64 * _per_sample_bytes(80), _per_sample_bytes(80), equal=True)
    assert cuts == [(0, 44), (44, 88), (88, 130)]
    case_id = {64: 2, 44: 1}[row]                          # 1e200 in one entry; +inf
    TH, bad = F.poisoned(c.TH, S, case_id, rows=[row])
    whole = eng.solve(TH, want_state=True)
    with _env(FINROM_ROM_WORKSPACE_BYTES=str(64 * _per_sample_bytes(80))):
        dirty = eng.solve(TH, want_state=True)
        clean = eng.solve(c.TH[:S], want_state=True)
    keys = _keys(dirty)
    assert set(keys) == {"qoi_r", "w_r", "A_r", "B_r"}
    F.check_contract(f"solve in pieces {cuts}, poison {F.kind_of(case_id, 0)} at row {row}", clean, dirty, bad, keys, F.ROM_FLAG)
    for s0, s1 in cuts:
        alone = eng.solve(TH[s0:s1], want_state=True)
        F.same_bits(f"solve in pieces, piece {s0}:{s1}", {k: np.asarray(v)[s0:s1] for k, v in dirty.items()}, alone, keys)
    assert not np.array_equal(np.asarray(whole["qoi_r"])[:44], np.asarray(dirty["qoi_r"])[:44]), "the batch was not cut"
    assert np.array_equal(np.asarray(whole["info"]), np.asarray(dirty["info"]))


def _per_sample_bytes(r):
    rp = (r + 15) // 16 * 16
    return (rp * (rp + 1) // 2 + rp) * 8


@pytest.mark.parametrize("branch,r,obs40,S,piece,differs", [("one-sample kernels", 80, False, 130, 64, True),
                                                           ("batched contraction", 80, False, 200, 128, False),
                                                           ("split-K form, 40 observations", 81, True, 64, 32, False)])
def test_gradient_in_pieces(models, branch, r, obs40, S, piece, differs):
    """finrom_rom_grad with per-sample data in pieces (whole pieces, then the rest), once per branch of its piece loop, so that each
    branch's offsets of theta, data, J, g, w_r, qoi_r and info (and its use of vw and the arrival counters piece after piece) run
    with s0 > 0: r = 80, S = 130 as 64 + 64 + 2 (the one-sample kernels; the one-piece call takes the batched contraction: other
    bits); r = 80, S = 200 as 128 + 72 (rom_subst_blocked_kernel + rom_grad_contract_kernel in both pieces); r = 81 with 40
    observations, S = 64 as 32 + 32 (rom_proj_splitk_kernel with factor 4).  The first row of the second piece is poisoned; a second
    call has a NaN in its data row instead.  Every piece is compared bit for bit with a call on its slice."""
    rom, c = models(12, r, external_obs=obs40)
    rom._ensure_gradient()
    eng = rom._rom
    bound = piece * _per_sample_bytes(r)
    cuts = _pieces(S, bound, _per_sample_bytes(r), equal=False)
    assert cuts[0] == (0, piece) and len(cuts) >= 2 and cuts[-1][1] == S
    row = piece
    D = c.D[:S]
    assert not np.array_equal(D[row], D[0])
    TH, bad = F.poisoned(c.TH, S, 2, rows=[row])
    Dn = D.copy()
    Dn[row, 3] = np.nan
    whole = eng.grad(TH, D)
    with _env(FINROM_ROM_WORKSPACE_BYTES=str(bound)):
        clean = eng.grad(c.TH[:S], D)
        dirty = eng.grad(TH, D)
        dirty_data = eng.grad(c.TH[:S], Dn)
    label = f"gradient in pieces {cuts}, {branch}"
    F.check_contract(f"{label}, poison {F.kind_of(2, 0)} at row {row}", clean, dirty, bad, GRAD_KEYS, F.ROM_FLAG)
    F.check_contract(f"{label}, NaN in data row {row}", clean, dirty_data, [], GRAD_KEYS, F.ROM_FLAG, data_bad=[row])
    for s0, s1 in cuts:
        alone = eng.grad(TH[s0:s1], D[s0:s1])
        F.same_bits(f"{label}, piece {s0}:{s1}", {k: np.asarray(v)[s0:s1] for k, v in dirty.items()}, alone, GRAD_KEYS)
    if differs:
        assert not np.array_equal(np.asarray(whole["g"])[:piece], np.asarray(dirty["g"])[:piece]), "the batch was not cut"
    assert np.array_equal(np.asarray(whole["info"]), np.asarray(dirty["info"]))
