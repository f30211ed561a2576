"""Host logic of the COMPACT list (DESIGN 4b'', finrom_rom_compact_rows, RomEngine.mirror_compact_rows), no GPU: the rotation of the
short list's pattern classes onto their singular directions, the gate that picks the threshold, the builder's counts and tables
for the compact descriptor, its solution against the short list's in 80-bit arithmetic, and the switches."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

import rom_lspg_cases as Y
from test_rom_mirror_host import _tables
from test_rom_short_scale_free_host import _thetas, _walk
from test_rom_skip_rows_host import _noisy_tables

SIZES = [(4, 16), (12, 80)]
SWITCHES = ("FINROM_ROM_NO_COMPACT", "FINROM_ROM_KEEP_ROWS", "FINROM_ROM_SHORT_GROUPED")


@functools.lru_cache(maxsize=None)
def _form(m, r):
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    ops, phi, tables = _tables(m, r)
    return ops, tables, AffineROMFin.mirror_form(ops, tables)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


def _desc_tables(d, keep, P):
    """The descriptor's rows as tables [P + 1][n, r] (rows without terms are zero)."""
    row_ptr, term_p, tv = np.asarray(keep[0][0]), np.asarray(keep[1][0]), np.asarray(keep[2][0])
    T = np.zeros((P + 1, d.n, d.r))
    T[term_p, np.repeat(np.arange(d.n), np.diff(row_ptr))] = tv
    return T


def _psi(T, theta):
    return np.tensordot(np.concatenate([[1.0], theta]), T, axes=1)


def _counts(d, keep):
    from bayesianinferencedl_amd import _ffi
    o = [C.c_int32() for _ in range(3)]
    _ffi.check(_ffi.lib().finrom_rom_mirror_counts(C.byref(d), keep[5][1], *[C.byref(x) for x in o]))
    return tuple(x.value for x in o)


def _load(d, keep, r):
    """The builder's tables of a descriptor (finrom_rom_mirror_tables): nkg, ext_final, records, rows, factor definitions."""
    from bayesianinferencedl_amd import _ffi
    L, wp = _ffi.lib(), keep[5][1]
    o = [C.c_int32() for _ in range(3)] + [C.c_int64()]
    _ffi.check(L.finrom_rom_mirror_tables(C.byref(d), wp, *[C.byref(x) for x in o], None, None, None))
    nkg, n_ext, ext_final, n_slots = [x.value for x in o]
    rp = (r + 15) // 16 * 16
    assert nkg > 0 and nkg % 3 == 0 and 0 < n_ext <= 64 and 0 < ext_final < n_ext
    kmg = np.zeros((nkg + 8) * 8, np.int32); tvg = np.zeros(n_slots * 4 * rp); ext_def = np.zeros(n_ext * 3, np.int32)
    _ffi.check(L.finrom_rom_mirror_tables(C.byref(d), wp, *[C.byref(x) for x in o], kmg.ctypes.data_as(_ffi.c_i32p),
                                          tvg.ctypes.data_as(_ffi.c_f64p), ext_def.ctypes.data_as(_ffi.c_i32p)))
    return nkg, ext_final, kmg.reshape(-1, 8), tvg.reshape(n_slots, 4, rp), ext_def.reshape(n_ext, 3)


def _eps_at(form, tables, theta, T_kept, T_trunc):
    """The gate's combined value at one theta, as RomEngine.mirror_probe_eps forms it: lambda_max(D, A) with A the kept compact rows'
    sum and D = psi_a^T psi_a + the short list's dropped rows + the truncated rotated rows."""
    import scipy.linalg as sla
    perm, rows, twin = form["perm"], form["rows"], form["twin"]
    Ts = form["Ts"]
    th1 = np.concatenate([[1.0], theta])
    ps = sum(th1[p] * Ts[p] for p in range(len(Ts))); pa = sum(th1[p] * (np.asarray(tables[p]) - Ts[p]) for p in range(len(Ts)))
    drop = np.zeros(len(perm), bool)
    drop[rows[form["dropped_rows"]]] = True; drop[perm[rows[form["dropped_rows"]]]] = True
    pk, pt = _psi(T_kept, theta), _psi(T_trunc, theta)
    D = pa.T @ pa + ps[drop].T @ ps[drop] + pt.T @ pt
    L = np.linalg.cholesky(pk.T @ pk)
    M = sla.solve_triangular(L, sla.solve_triangular(L, D, lower=True).T, lower=True)
    return float(np.linalg.eigvalsh(0.5 * (M + M.T)).max())


@pytest.mark.parametrize("m,r", SIZES)
def test_rotation(m, r):
    """Every rotated class: Q^T Q = I to 1e-13 (Q is a product of a few hundred plane rotations per row, one rounding of 2^-53 each:
    10 sweeps x 62 partners x 1.1e-16 = 7e-14 if they all added up), the rotated rows are Q times the weighted rows, the singular
    values come largest first, and the class's sum over ALL rotated rows -- the truncated ones included -- equals the sum over its
    own weighted rows to 1e-14 max|A_r| at the gate's 16 probes and the 32 corners of [0.1, 10]."""
    from bayesianinferencedl_amd.engine import RomEngine
    ops, tables, form = _form(m, r)
    d, keep = form["desc_short"], form["keep_short"]
    P = d.P
    out = RomEngine.compact_rows(d, keep, form["tau_compact"], with_q=True)
    assert np.array_equal(out["tv"], form["compact_out"]["tv"]) and np.array_equal(out["keep"], form["compact_out"]["keep"])
    weight = np.asarray(keep[5][0])
    T_short = _desc_tables(d, keep, P) * np.sqrt(weight)[None, :, None]
    T_rot = RomEngine.compact_tables(d, keep, dict(out, keep=np.ones(d.n, np.int32)), P)[0]       # every row, truncated ones too
    loaded = np.asarray(keep[3][0]) != 0.0
    assert (out["cls"][loaded] == -1).all() and np.array_equal(T_rot[:, loaded], T_short[:, loaded])
    assert np.allclose(out["rhs"][loaded] * np.sqrt(weight[loaded]), np.asarray(keep[3][0])[loaded], rtol=1e-15)
    probes, corners = _thetas(form["twin"])
    assert len(probes) == 16 and len(corners) == 32
    A_max = [np.abs(_psi(T_rot, th).T @ _psi(T_rot, th)).max() for th in probes + corners]
    rotated = 0
    print(f"m = {m}, r = {r}: tau = {form['tau_compact']:g}, largest singular value {out['sigma_max']:.3e}")
    for c in range(out["cls"].max() + 1):
        mem = np.nonzero(out["cls"] == c)[0]
        sig = out["sigma"][mem]
        pattern = np.nonzero(np.abs(T_short[:, mem]).sum(axis=(1, 2)))[0]
        is_rot = bool((out["keep"][mem] == 0).any())
        print(f"    class {c} {list(pattern)}: {len(mem)} rows, singular values >= 1e-5 / 1e-7 / tau of the largest: "
              f"{(sig >= 1e-5 * out['sigma_max']).sum()} / {(sig >= 1e-7 * out['sigma_max']).sum()} / "
              f"{(sig >= form['tau_compact'] * out['sigma_max']).sum()}{', rotated' if is_rot else ''}")
        assert (np.diff(sig) <= 0).all() and sig[0] <= out["sigma_max"]
        if not is_rot:
            assert np.array_equal(T_rot[:, mem], T_short[:, mem]) and not out["Q"][mem].any()
            continue
        rotated += 1
        assert np.array_equal(out["keep"][mem] != 0, sig >= form["tau_compact"] * out["sigma_max"])
        assert (out["keep"][mem] != 0).sum() // -4 > len(mem) // -4                   # it saves a k-step
        Q = out["Q"][mem][:, :len(mem)]
        assert not out["Q"][mem][:, len(mem):].any()
        qerr = np.abs(Q.T @ Q - np.eye(len(mem))).max()
        rerr = np.abs(np.einsum("ij,pjk->pik", Q, T_short[:, mem]) - T_rot[:, mem]).max() / np.abs(T_short[:, mem]).max()
        gerr = 0.0
        for th, amax in zip(probes + corners, A_max):
            a, b = _psi(T_rot[:, mem], th), _psi(T_short[:, mem], th)
            gerr = max(gerr, np.abs(a.T @ a - b.T @ b).max() / amax)
        print(f"        |Q^T Q - I| {qerr:.2e}, |Q rows - rotated rows| {rerr:.2e}, class sum {gerr:.2e} max|A_r|")
        assert qerr <= 1e-13 and rerr <= 1e-13 and gerr <= 1e-14
    assert rotated >= 4


@pytest.mark.parametrize("m,r", SIZES)
def test_gate(m, r):
    """The combined value -- psi_a^T psi_a, the short list's dropped rows and the truncated rotated rows in D -- is at most 1e-9 at the
    gate's probes and at the 32 corners of [0.1, 10]; the installed tau is the first of the ladder that passes."""
    from bayesianinferencedl_amd.engine import RomEngine
    ops, tables, form = _form(m, r)
    assert RomEngine.MIRROR_COMPACT_TAUS == (1e-8, 1e-9, 1e-10) and RomEngine.MIRROR_EPS_GATE == 1e-9
    d, keep = form["desc_short"], form["keep_short"]
    T_kept, T_trunc = RomEngine.compact_tables(d, keep, form["compact_out"], d.P)
    probes, corners = _thetas(form["twin"])
    e_probe = max(_eps_at(form, tables, th, T_kept, T_trunc) for th in probes)
    e_corner = max(_eps_at(form, tables, th, T_kept, T_trunc) for th in corners)
    print(f"m = {m}, r = {r}: tau {form['tau_compact']:g}, eps at the probes {e_probe:.3e} (the form's {form['eps_compact']:.3e}; "
          f"short list {form['eps']:.3e}), at the corners {e_corner:.3e}")
    assert form["eps_compact"] <= 1e-9 and e_probe <= 1e-9 and e_corner <= 1e-9
    assert abs(e_probe - form["eps_compact"]) <= 1e-6 * form["eps_compact"] + 1e-30
    assert form["eps_compact"] >= form["eps"] * (1 - 1e-6)            # more rows in D, fewer in A: never better than the short list
    drop = np.zeros(len(form["perm"]), bool)
    drop[form["rows"][form["dropped_rows"]]] = True; drop[form["perm"][form["rows"][form["dropped_rows"]]]] = True
    for tau in RomEngine.MIRROR_COMPACT_TAUS:
        out = RomEngine.compact_rows(d, keep, tau)
        if (out["keep"] != 0).all():
            continue
        eps = RomEngine.mirror_probe_eps(tables, form["perm"], form["twin"], nprobe=16, drop=drop,
                                         rotated=RomEngine.compact_tables(d, keep, out, d.P))[0]
        if eps <= 1e-9:
            assert tau == form["tau_compact"] and eps == form["eps_compact"]
            break
    else:
        raise AssertionError("no tau of the ladder passes")


@pytest.mark.parametrize("m,r", SIZES)
def test_noisy_basis_gets_no_compact_list(m, r):
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    ops, tables = _noisy_tables(m, r, symmetric=False)
    form = AffineROMFin.mirror_form(ops, tables)
    assert "desc_compact" not in form and "desc_short" not in form


@pytest.mark.parametrize("m,r", SIZES)
def test_counts(m, r):
    """finrom_rom_mirror_counts on desc_compact: fewer rows than the short list (317 at m = 12) and at most (rows + 3) // 4 + 12
    k-steps; expected at (12, 80): about 139 rows and 42 k-steps."""
    ops, tables, form = _form(m, r)
    rows_c, k_c, fma_c = _counts(form["desc_compact"], form["keep_compact"])
    rows_s, k_s, fma_s = _counts(form["desc_short"], form["keep_short"])
    print(f"m = {m}, r = {r}: compact list {rows_c} rows, {k_c} k-steps ({fma_c} with vector arithmetic); "
          f"short list {rows_s} rows, {k_s} k-steps ({fma_s})")
    if (m, r) == (12, 80):
        assert rows_s == 317
    assert rows_c == form["compact_rows"] == rows_s - form["compact_truncated"] < rows_s
    assert (rows_c + 3) // 4 <= k_c <= (rows_c + 3) // 4 + 12 and k_c < k_s and fma_c <= k_c
    assert (np.asarray(form["keep_compact"][5][0]) == 1.0).all() and form["desc_compact"].n == form["desc_short"].n


@pytest.mark.parametrize("m,r", SIZES)
def test_walk(m, r):
    """The NumPy walk of the builder's tables for desc_compact, as proj_main_grouped walks them, reproduces the compact rows' psi^T psi
    to 1e-14 max|A_r| at the gate's 16 probes and the 32 corners; no factor of the list doubles."""
    ops, tables, form = _form(m, r)
    d, keep = form["desc_compact"], form["keep_compact"]
    tb = _load(d, keep, r)
    assert not (tb[4][:, 2] & 2).any()
    T = _desc_tables(d, keep, d.P)
    probes, corners = _thetas(form["twin"])
    worst = 0.0
    for th in probes + corners:
        want = _psi(T, th).T @ _psi(T, th)
        worst = max(worst, np.abs(_walk(tb, r, th) - want).max() / np.abs(want).max())
    print(f"m = {m}, r = {r}: walk vs the compact rows, 16 probes + 32 corners: {worst:.2e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("m,r", SIZES)
def test_solution(m, r):
    """The compact list's 80-bit LSPG against the short list's 80-bit LSPG on the checked samples of the bench case's batch: within
    the allowance of host64's own deviation from the short list's yardstick there (what the short list itself is held to)."""
    case = Y.case(m, r, "bench")
    form = case.form
    d, keep = form["desc_compact"], form["keep_compact"]
    Tc = _desc_tables(d, keep, d.P)
    Tc = Tc[:, np.diff(np.asarray(keep[0][0])) > 0]
    full = np.zeros((10,) + Tc.shape[1:])
    full[:Tc.shape[0]] = Tc                                  # (merged under the smaller index: the twins' tables are zero)
    rows, ones = np.arange(Tc.shape[1]), np.ones(Tc.shape[1])
    res = {}
    for k in ("qoi_r", "Phi_w"):
        dd = dh = 0.0
        for s in Y.checked_samples(case.SMAX):
            ref = case.ld(s, "short")
            got = Y.lspg_ld(case.tables, case.F, case.C, case.TH[s], phi=case.phi, row_tables=list(full), rows=rows, weight=ones)
            dd, dh = max(dd, Y.dev(got[k], ref[k])), max(dh, Y.dev(case.h64(s, "short")[k], ref[k]))
        res[k] = (dd, dh)
    assert Y.report(f"m = {m}, r = {r}, compact vs short, 80-bit", res)


@pytest.mark.parametrize("m,r", SIZES)
def test_switches(m, r, monkeypatch):
    """FINROM_ROM_NO_COMPACT=1 and FINROM_ROM_KEEP_ROWS=1 give forms without desc_compact; the half tables keep the sha256 of DESIGN
    4b'' and the short tables are the same bytes with and without the compact list beside them."""
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    ops, tables, form = _form(m, r)
    assert "desc_compact" in form
    sha = lambda tb: tuple(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:12] for a in (tb[3], tb[2], tb[4]))
    half, short = sha(_load(form["desc"], form["keep"], r)), sha(_load(form["desc_short"], form["keep_short"], r))
    print(f"m = {m}, r = {r}: half {half}, short {short}")
    assert half == {(4, 16): ("395ce7abbcad", "7107de23a447", "1ff6acad96d3"), (12, 80): ("f97de4d4a419", "4b98d14a2717", "1ff6acad96d3")}[(m, r)]
    assert short == SHORT_SHA[(m, r)]
    monkeypatch.setenv("FINROM_ROM_NO_COMPACT", "1")
    f2 = AffineROMFin.mirror_form(ops, tables)
    monkeypatch.delenv("FINROM_ROM_NO_COMPACT")
    assert "desc_compact" not in f2 and "desc_short" in f2 and f2["eps"] == form["eps"] and f2["dropped"] == form["dropped"]
    assert sha(_load(f2["desc"], f2["keep"], r)) == half and sha(_load(f2["desc_short"], f2["keep_short"], r)) == short
    monkeypatch.setenv("FINROM_ROM_KEEP_ROWS", "1")
    f3 = AffineROMFin.mirror_form(ops, tables)
    monkeypatch.delenv("FINROM_ROM_KEEP_ROWS")
    assert "desc_compact" not in f3 and "desc_short" not in f3 and sha(_load(f3["desc"], f3["keep"], r)) == half


# tvg / kmg / ext_def of the short list as the builder made them before the compact list existed (first 12 digits of the sha256)
SHORT_SHA = {(4, 16): ("c3ebc2ce1233", "d04bf16aaf1f", "a97ca3adcb8a"), (12, 80): ("f47a7d69efeb", "5c251515a04a", "a97ca3adcb8a")}
