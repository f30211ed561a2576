"""Host logic of the SHORT half list (DESIGN 4b'', RomEngine.mirror_skip_rows), no GPU: which rows of the half list the gate lets
go, that a basis whose rows are not small keeps them all, the builder's tables walked in NumPy as proj_main_grouped walks them, and
the builder's own counts (finrom_rom_mirror_counts)."""
import ctypes as C

import numpy as np
import pytest

from test_rom_mirror_host import _symmetric_theta, _tables

CASES = [(4, 16, 30, 131), (12, 80, 506, 823)]


def _form(m, r, monkeypatch=None, keep_rows=False):
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    ops, phi, tables = _tables(m, r)
    if keep_rows:
        monkeypatch.setenv("FINROM_ROM_KEEP_ROWS", "1")
    try:
        return ops, AffineROMFin.mirror_form(ops, tables)
    finally:
        if keep_rows:
            monkeypatch.delenv("FINROM_ROM_KEEP_ROWS")


def _counts(form, short=False):
    from bayesianinferencedl_amd import _ffi
    o = [C.c_int32() for _ in range(3)]
    d, keep = (form["desc_short"], form["keep_short"]) if short else (form["desc"], form["keep"])
    _ffi.check(_ffi.lib().finrom_rom_mirror_counts(C.byref(d), keep[5][1], *[C.byref(x) for x in o]))
    return tuple(x.value for x in o)


def _walk(form, r, theta):
    """A_r of the builder's short list per theta, accumulated as the kernel accumulates it (test_rom_mirror_host)."""
    from bayesianinferencedl_amd import _ffi
    d, keep = form["desc_short"], form["keep_short"]
    L = _ffi.lib()
    wp = keep[5][1]
    o = [C.c_int32() for _ in range(3)] + [C.c_int64()]
    _ffi.check(L.finrom_rom_mirror_tables(C.byref(d), wp, *[C.byref(x) for x in o], None, None, None))
    nkg, n_ext, ext_final, n_slots = [x.value for x in o]
    rp = (r + 15) // 16 * 16
    assert nkg > 0 and nkg % 3 == 0 and 0 < n_ext <= 64 and 0 < ext_final < n_ext
    kmg = np.zeros((nkg + 8) * 8, np.int32); tvg = np.zeros(n_slots * 4 * rp); ext_def = np.zeros(n_ext * 3, np.int32)
    _ffi.check(L.finrom_rom_mirror_tables(C.byref(d), wp, *[C.byref(x) for x in o], kmg.ctypes.data_as(_ffi.c_i32p),
                                          tvg.ctypes.data_as(_ffi.c_f64p), ext_def.ctypes.data_as(_ffi.c_i32p)))
    kmg = kmg.reshape(-1, 8); tvg = tvg.reshape(n_slots, 4, rp); ext_def = ext_def.reshape(n_ext, 3)
    assert (kmg[nkg:, 1] == 1).all() and (kmg[nkg:, 2] == 1).all() and not tvg[kmg[nkg, 0]].any()
    assert ((ext_def[:, 2] & 2) != 0).sum() == 1
    live = int(np.count_nonzero([tvg[s:s + nt].any() for s, nt in kmg[:nkg, :2]]))

    def A_r(theta):
        th1 = np.concatenate([[1.0], theta])
        ext = np.array([(th1[a] / th1[b]) ** (2 if f & 1 else 1) * (2.0 if f & 2 else 1.0) for a, b, f in ext_def])
        acc = np.zeros((rp, rp))
        for slot, nt, flags, fidx, *cf in kmg[:nkg]:
            if flags & 2:
                acc *= ext[fidx]
            slab = tvg[slot].copy() if flags & 1 else ext[cf[0]] * tvg[slot]
            for t in range(1, nt):
                slab += ext[cf[t]] * tvg[slot + t]
            acc += slab.T @ slab
        acc *= ext[ext_final]
        assert not acc[r:].any() and not acc[:, r:].any()
        return acc[:r, :r]
    return [A_r(th) for th in theta], live, nkg


@pytest.mark.parametrize("m,r,ndrop,nhalf", CASES)
def test_selection_and_gate(m, r, ndrop, nhalf):
    """30 of 131 (m = 4, r = 16) and 506 of 823 (m = 12, r = 80) half rows are dropped, at the first threshold tried; the combined
    probe value stays below the gate and is not smaller than the value without dropped rows; no row with load is dropped; in the
    short descriptor a dropped row keeps node and weight and has no terms, every other row has some; the half descriptor beside it
    (what samples outside the probes' range walk) keeps every row."""
    from bayesianinferencedl_amd.engine import RomEngine
    ops, form = _form(m, r)
    assert form["installs"] and len(form["rows"]) == nhalf
    print(f"m = {m}, r = {r}: dropped {form['dropped']} of {nhalf} rows at tau = {form['tau']:g}, "
          f"eps combined {form['eps']:.3e}, eps all rows {form['eps_all_rows']:.3e}")
    assert form["dropped"] == ndrop == int(form["dropped_rows"].sum()) and form["tau"] == 1e-6
    assert form["eps_all_rows"] <= form["eps"] <= RomEngine.MIRROR_EPS_GATE == 1e-9
    assert not (ops.F[form["rows"]][form["dropped_rows"]] != 0).any() and (ops.F != 0).any()
    assert form["desc"].n == nhalf and (np.diff(form["keep"][0][0]) > 0).all()
    d, keep = form["desc_short"], form["keep_short"]
    row_ptr = keep[0][0]
    assert d.n == nhalf and np.array_equal(keep[4][0], form["rows"]) and np.array_equal(keep[5][0], form["weight"])
    assert np.array_equal(np.diff(row_ptr) == 0, form["dropped_rows"])
    # the gap: any threshold between 1e-7 and 1e-5 selects the same rows
    rn = np.sqrt(sum((T[form["rows"]] ** 2).sum(1) for T in form["Ts"])); rn /= rn.max()
    print(f"    largest dropped row {rn[form['dropped_rows']].max():.1e}, smallest kept row {rn[~form['dropped_rows']].min():.1e}")
    assert rn[form["dropped_rows"]].max() < 1e-7 and rn[~form["dropped_rows"]].min() > 1e-5


def _noisy_tables(m, r, symmetric):
    """The basis plus 1e-4 x random noise (unit columns), re-orthonormalised; symmetric: the noise mirrored onto itself."""
    from bayesianinferencedl_amd.bandplan import mirror_permutation
    ops, phi, _ = _tables(m, r)
    N = np.random.default_rng(5).standard_normal(phi.shape)
    if symmetric:
        N = 0.5 * (N + N[mirror_permutation(ops.mesh)])
    phi = np.linalg.qr(phi + 1e-4 * N / np.linalg.norm(N, axis=0))[0]
    return ops, [ops.csr(ops.robin_vals) @ phi] + [ops.csr(ops.sub_vals[i]) @ phi for i in range(9)]


@pytest.mark.parametrize("m,r", [(4, 16), (12, 80)])
def test_noisy_basis_keeps_its_rows(m, r, monkeypatch):
    """1e-4 x random noise on the basis: no row is small any more, nothing is dropped.  Plain noise also breaks the mirror symmetry,
    so that form does not install at all (as before); with the noise mirrored onto itself the form installs, drops nothing and is
    the one FINROM_ROM_KEEP_ROWS=1 gives, down to the builder's k-steps.  The switch on the clean basis: today's rows, all of them."""
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    ops, tables = _noisy_tables(m, r, symmetric=False)
    form = AffineROMFin.mirror_form(ops, tables)
    assert form["dropped"] == 0 and not form["dropped_rows"].any() and form["eps"] == form["eps_all_rows"] and "desc_short" not in form
    ops, tables = _noisy_tables(m, r, symmetric=True)
    form = AffineROMFin.mirror_form(ops, tables)
    print(f"m = {m}, r = {r}, symmetric noise: eps {form['eps']:.3e}, dropped {form['dropped']}")
    assert form["installs"] and form["dropped"] == 0 and form["tau"] is None and form["eps"] == form["eps_all_rows"]
    assert "desc_short" not in form
    monkeypatch.setenv("FINROM_ROM_KEEP_ROWS", "1")
    keep_form = AffineROMFin.mirror_form(ops, tables)
    counts_keep = _counts(keep_form)
    monkeypatch.delenv("FINROM_ROM_KEEP_ROWS")
    assert keep_form["eps"] == form["eps"] and keep_form["dropped"] == 0
    for a, b in zip(form["keep"], keep_form["keep"]):
        assert np.array_equal(a[0], b[0])
    assert _counts(form) == counts_keep and counts_keep[0] == form["desc"].n
    _, clean_keep = _form(m, r, monkeypatch, keep_rows=True)
    assert clean_keep["installs"] and clean_keep["dropped"] == 0 and "desc_short" not in clean_keep
    assert (np.diff(clean_keep["keep"][0][0]) > 0).all()
    for a, b in zip(clean_keep["keep"], _form(m, r)[1]["keep"]):      # ... and the half descriptor is the same with or without the switch
        assert np.array_equal(a[0], b[0])
    assert clean_keep["eps"] == clean_keep["eps_all_rows"] == _form(m, r)[1]["eps_all_rows"]


@pytest.mark.parametrize("m,r,ndrop,nhalf", CASES)
def test_short_list_walk_and_counts(m, r, ndrop, nhalf, monkeypatch):
    """For eight mirror-symmetric theta in [0.1, 10] the short list's sum reproduces psi_s[kept]^T W psi_s[kept] to 1e-12 max|A_r|
    and differs from the all-rows sum psi_s^T psi_s by at most 1e-12 max|A_r| (the tolerance of the all-rows walk; measured 2e-14);
    B_r of the descriptor equals psi_s^T F to 1e-12.  The builder's counts: the kept rows, at most (kept + 3) // 4 + 12 k-steps,
    fewer than the list with all rows, and the same numbers as the tables show."""
    ops, form = _form(m, r)
    d, keep, Ts, twin = form["desc_short"], form["keep_short"], form["Ts"], form["twin"]
    rows, weight, dropped = form["rows"], form["weight"], form["dropped_rows"]
    rng = np.random.default_rng(11)
    thetas = [_symmetric_theta(rng, twin) for _ in range(8)]
    got, live, nkg = _walk(form, r, thetas)
    row_ptr, term_p, tv, rhs_half = keep[0][0], keep[1][0], keep[2][0], keep[3][0]
    worst_kept = worst_all = 0.0
    for theta, A in zip(thetas, got):
        th1 = np.concatenate([[1.0], theta])
        psi_s = sum(th1[p] * Ts[p] for p in range(10))
        ph = psi_s[rows]
        kept = (ph[~dropped].T * weight[~dropped]) @ ph[~dropped]
        full = psi_s.T @ psi_s
        worst_kept = max(worst_kept, np.max(np.abs(A - kept)) / np.abs(kept).max())
        worst_all = max(worst_all, np.max(np.abs(A - full)) / np.abs(full).max())
        psi_half = np.zeros((d.n, r))
        for i in range(d.n):
            for t in range(row_ptr[i], row_ptr[i + 1]):
                psi_half[i] += th1[term_p[t]] * tv[t]
        Br, Br_want = psi_half.T @ rhs_half, psi_s.T @ ops.F
        assert np.max(np.abs(Br - Br_want)) <= 1e-12 * np.abs(Br_want).max()
    live_rows, ksteps, fma_ksteps = _counts(form, short=True)
    assert _counts(form) == _counts(_form(m, r, monkeypatch, keep_rows=True)[1])      # the half list beside it: as ever
    _, keep_form = _form(m, r, monkeypatch, keep_rows=True)
    monkeypatch.setenv("FINROM_ROM_KEEP_ROWS", "1")
    all_rows, all_ksteps, all_fma = _counts(keep_form)
    monkeypatch.delenv("FINROM_ROM_KEEP_ROWS")
    print(f"m = {m}, r = {r}: short list {ksteps} k-steps ({fma_ksteps} with vector arithmetic, {nkg} with padding) for {live_rows} rows; "
          f"all rows: {all_ksteps} k-steps ({all_fma}) for {all_rows} rows; walk vs kept rows {worst_kept:.2e}, vs all rows {worst_all:.2e}")
    assert worst_kept <= 1e-12 and worst_all <= 1e-12
    assert live_rows == nhalf - ndrop and all_rows == nhalf
    assert ksteps == live and nkg - 2 <= ksteps <= nkg
    assert (live_rows + 3) // 4 <= ksteps <= (live_rows + 3) // 4 + 12
    assert ksteps < all_ksteps and fma_ksteps <= ksteps
