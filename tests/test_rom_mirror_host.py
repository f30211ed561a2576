"""Host logic of the half form of the projection for mirror-symmetric reduced models (DESIGN 4b', finrom_rom_set_mirror), no GPU:
the half list's tables walked in NumPy as proj_main_grouped walks them, the gate that decides whether a basis gets the form, and
the half descriptor's validator."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import fin_oracle as O


@functools.lru_cache(maxsize=None)
def _tables(m, r, kind="five", noise=0.0):
    """Per (mesh, basis), once: the operators, the POD basis of oracle snapshots by bench.py's recipe (400 five- or nine-parameter
    samples of U(0.1, 10), seed 1) and the tables A_p Phi.  noise: antisymmetric noise of that column 2-norm, re-orthonormalised."""
    from bayesianinferencedl_amd.bandplan import mirror_permutation
    from bayesianinferencedl_amd.fom.thermal_fin import get_space
    prob = O.FinProblem(m)
    fo = O.FinOracle(prob)
    rng = np.random.default_rng(1)
    lift = fo.five_param_to_function if kind == "five" else fo.nine_param_to_function
    Y = np.array([fo.forward(lift(rng.uniform(0.1, 10.0, 5 if kind == "five" else 9))) for _ in range(400)])
    phi = O.pod_basis(Y, r)
    V = get_space(None, m=m); ops = V.operators()
    if noise:
        perm = mirror_permutation(ops.mesh)
        N = np.random.default_rng(2).standard_normal(phi.shape)
        N = 0.5 * (N - N[perm])
        phi = np.linalg.qr(phi + noise * N / np.linalg.norm(N, axis=0))[0]
    tables = [ops.csr(ops.robin_vals) @ phi] + [ops.csr(ops.sub_vals[i]) @ phi for i in range(9)]
    return ops, phi, tables


def _symmetric_theta(rng, twin, low=0.1, high=10.0):
    th = np.exp(rng.uniform(np.log(low), np.log(high), len(twin)))
    return th[np.minimum(np.arange(len(twin)), twin)]


@pytest.mark.parametrize("m,r", [(4, 16), (12, 80)])
def test_half_list_reproduces_the_symmetric_part(m, r):
    """The tables of finrom_rom_mirror_tables, walked as the kernel walks them (slab = first term's rows as loaded where the record
    says so, multiply-adds for the others, accumulators rescaled where a record opens a segment and behind the last k-step -- the
    factor between the rows that count twice and the rows that count once carries the 2), give psi_s^T psi_s over ALL rows,
    psi_s = A(theta) Phi_s, for 8 mirror-symmetric theta in [0.1, 10], to 1e-12 max|A_r|; the descriptor's rows with its load
    (weight F) give B_r = psi_s^T F."""
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    ops, phi, tables = _tables(m, r)
    form = AffineROMFin.mirror_form(ops, tables)
    assert form is not None and form["installs"], form and form["eps"]
    d, keep, Ts, twin = form["desc"], form["keep"], form["Ts"], form["twin"]
    L = _ffi.lib()
    wp = keep[5][1]
    nkg, n_ext, ext_final, n_slots = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    _ffi.check(L.finrom_rom_mirror_tables(C.byref(d), wp, C.byref(nkg), C.byref(n_ext), C.byref(ext_final), C.byref(n_slots), None, None, None))
    nkg, n_ext, ext_final, n_slots = nkg.value, n_ext.value, ext_final.value, n_slots.value
    rp = (r + 15) // 16 * 16
    assert nkg > 0 and nkg % 3 == 0 and 0 < n_ext <= 64 and 0 < ext_final < n_ext
    kmg = np.zeros((nkg + 8) * 8, np.int32); tvg = np.zeros(n_slots * 4 * rp); ext_def = np.zeros(n_ext * 3, np.int32)
    o = [C.c_int32() for _ in range(3)] + [C.c_int64()]
    _ffi.check(L.finrom_rom_mirror_tables(C.byref(d), wp, *[C.byref(x) for x in o], kmg.ctypes.data_as(_ffi.c_i32p),
                                          tvg.ctypes.data_as(_ffi.c_f64p), ext_def.ctypes.data_as(_ffi.c_i32p)))
    kmg = kmg.reshape(-1, 8); tvg = tvg.reshape(n_slots, 4, rp); ext_def = ext_def.reshape(n_ext, 3)
    assert (kmg[nkg:, 1] == 1).all() and (kmg[nkg:, 2] == 1).all() and not tvg[kmg[nkg, 0]].any()      # zero k-steps behind the list
    assert ((ext_def[:, 2] & 2) != 0).sum() == 1            # exactly one factor doubles
    # about half the k-steps of the full list (m = 12: 400)
    live = int(np.count_nonzero([tvg[s:s + nt].any() for s, nt in kmg[:nkg, :2]]))
    full_rows, half_rows = ops.n, d.n
    print(f"m = {m}, r = {r}: half list {live} k-steps for {half_rows} of {full_rows} rows, eps_probe = {form['eps']:.3e}")
    assert live <= (half_rows + 3) // 4 + 12
    # the half descriptor as plain arrays
    row_ptr, term_p, tv = keep[0][0], keep[1][0], keep[2][0]
    rhs_half = keep[3][0]
    rng = np.random.default_rng(11)
    for trial in range(8):
        theta = _symmetric_theta(rng, twin)
        th1 = np.concatenate([[1.0], theta])
        ext = np.array([(th1[a] / th1[b]) ** (2 if f & 1 else 1) * (2.0 if f & 2 else 1.0) for a, b, f in ext_def])
        assert ext[0] == 1.0
        acc = np.zeros((rp, rp))
        for slot, nt, flags, fidx, *cf in kmg[:nkg]:
            if flags & 2:
                acc *= ext[fidx]
            slab = tvg[slot].copy() if flags & 1 else ext[cf[0]] * tvg[slot]
            for t in range(1, nt):
                slab += ext[cf[t]] * tvg[slot + t]
            acc += slab.T @ slab
        acc *= ext[ext_final]
        psi_s = sum(th1[p] * Ts[p] for p in range(10))
        want = psi_s.T @ psi_s
        assert np.max(np.abs(acc[:r, :r] - want)) <= 1e-12 * np.abs(want).max()
        assert not acc[r:].any() and not acc[:, r:].any()
        psi_half = np.zeros((d.n, r))
        for i in range(d.n):
            for t in range(row_ptr[i], row_ptr[i + 1]):
                psi_half[i] += th1[term_p[t]] * tv[t]
        Br, Br_want = psi_half.T @ rhs_half, psi_s.T @ ops.F
        assert np.max(np.abs(Br - Br_want)) <= 1e-12 * np.abs(Br_want).max()


def test_gate_installs_and_refuses(monkeypatch):
    """(c) of the gate at m = 12, r = 80: the five-parameter basis installs (eps_probe printed; 5.7e-11 on the CPU), the
    nine-parameter basis is refused, and so is the five-parameter basis plus antisymmetric noise of column norm 1e-7 (eps 2e-5: an
    entrywise test would have let it through); (d): with FINROM_ROM_NO_MIRROR set nothing installs."""
    from bayesianinferencedl_amd.engine import RomEngine
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    ops, _, tables = _tables(12, 80)
    form = AffineROMFin.mirror_form(ops, tables)
    print(f"eps_probe, five-parameter basis, m = 12, r = 80: {form['eps']:.3e}")
    assert form["installs"] and form["eps"] < 1e-9
    assert RomEngine.MIRROR_EPS_GATE == 1e-9 and RomEngine.MIRROR_PROBES >= 16
    ops9, _, tables9 = _tables(12, 80, "nine")
    form9 = AffineROMFin.mirror_form(ops9, tables9)
    print(f"eps_probe, nine-parameter basis: {form9['eps']:.3e}")
    assert not form9["installs"] and form9["eps"] > 1e-3 and "desc" not in form9
    opsn, _, tablesn = _tables(12, 80, "five", 1e-7)
    formn = AffineROMFin.mirror_form(opsn, tablesn)
    print(f"eps_probe, five-parameter basis + 1e-7 antisymmetric noise: {formn['eps']:.3e}")
    assert not formn["installs"] and 1e-9 < formn["eps"] < 1e-3
    monkeypatch.setenv("FINROM_ROM_NO_MIRROR", "1")
    assert AffineROMFin.mirror_form(ops, tables) is None


def test_validator_refuses_corrupt_half_descriptors():
    """finrom_rom_mirror_validate: the descriptor of the m = 4 form passes; a wrong weight, a row listed twice and a twin that is
    not an involution each come back as FINROM_ERR_ARG."""
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    ops, _, tables = _tables(4, 16)
    form = AffineROMFin.mirror_form(ops, tables)
    d, keep = form["desc"], form["keep"]
    node, weight, twin = keep[4][0], keep[5][0], keep[6][0]
    L = _ffi.lib()
    call = lambda: L.finrom_rom_mirror_validate(C.byref(d), ops.n, keep[4][1], keep[5][1], keep[6][1])
    assert call() == 0, L.finrom_last_error()

    def refused(arr, idx, value, what):
        old = arr[idx]
        arr[idx] = value
        try:
            assert call() == -1 and what in L.finrom_last_error(), (what, L.finrom_last_error())
        finally:
            arr[idx] = old
    refused(weight, 0, 1.5, b"neither 1 nor 2")
    refused(weight, 0, 1.0, b"do not add up")
    refused(node, 1, node[0], b"listed twice")
    refused(twin, 0, 0 if twin[0] != 0 else 1, b"involution")
    assert call() == 0
