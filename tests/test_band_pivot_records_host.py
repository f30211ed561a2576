"""Pivot records of the half plan's functional form (include/finrom.h finrom_fom_band_mirror_records, csrc/fom_band_tables.hip,
DESIGN 4c'), on the host: one fixed-size record per entering node gathers what the sweeps read per pivot from nine tables.  The
records against the tables entry by entry (prologue and tail records included), the harmless slot of a pivot that is no interface
node, the validator against one changed field at a time, and a descriptor the functional form does not fit."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

MS = [4, 8, 12]
WINDOWS = {4: (3, 4), 8: (4, 6), 12: (5, 8)}
NF = 5


def _five(ops):
    return sp.csr_matrix(ops.W_field @ sp.csr_matrix(ops.N9 @ ops.E59))


def _form(spaces, m):
    from bayesianinferencedl_amd.engine import FomEngine
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    V = spaces(m)
    ops = V.operators()
    fin = Fin(V)
    form = FomEngine.mirror_form(ops, 5, ops.robin_vals, _five(ops), ops.F, fin.B_obs)
    assert form is not None
    return form


def _args(d, bp, n_rows, out_ptr, out_col, n_obs=9):
    from bayesianinferencedl_amd import _ffi
    op, oc = np.array(out_ptr, np.int32), np.array(out_col, np.int32)
    return (C.byref(d), bp.n, 5, n_rows, n_obs, op.ctypes.data_as(_ffi.c_i32p), oc.ctypes.data_as(_ffi.c_i32p)), (op, oc)


def _records(lib, d, bp, n_rows, out_ptr, out_col, n_obs=9):
    from bayesianinferencedl_amd import _ffi
    fr = np.zeros(d.nfins * (d.npf + d.nif), _ffi.BAND_FIN_REC)
    pr = np.zeros(d.npost + d.NSP, _ffi.BAND_POST_REC)
    fr["pad0"], pr["pad0"] = -7, -7                       # (the library writes whole records: the sentinels go)
    fits = C.c_int32(-1)
    args, keep = _args(d, bp, n_rows, out_ptr, out_col, n_obs)
    rc = lib.finrom_fom_band_mirror_records(*args, C.byref(fits), fr.ctypes.data, pr.ctypes.data)
    return rc, fits.value, fr, pr


def _functionals(lib, d, bp, n_rows, out_ptr, out_col):
    from bayesianinferencedl_amd import _ffi
    fits = C.c_int32(-1)
    cw = np.zeros(d.npost * NF); prow = np.zeros(d.npost, np.int32); poff = np.zeros(d.npost, np.int32)
    args, keep = _args(d, bp, n_rows, out_ptr, out_col)
    rc = lib.finrom_fom_band_mirror_functionals(*args, C.byref(fits), cw.ctypes.data_as(_ffi.c_f64p), prow.ctypes.data_as(_ffi.c_i32p),
                                                poff.ctypes.data_as(_ffi.c_i32p))
    assert rc == 0 and fits.value == 1
    return cw.reshape(d.npost, NF), prow, poff


def test_record_types_have_the_header_sizes():
    from bayesianinferencedl_amd import _ffi
    assert _ffi.BAND_FIN_REC.itemsize == 32 and _ffi.BAND_POST_REC.itemsize == 96


@pytest.mark.parametrize("m", MS)
def test_records_reproduce_the_tables(spaces, m):
    """abmap << 9, FgQ, act, ent_extra, the ecp ranges, piv_row, piv_off + offY and cw, entry by entry; the prologue's records
    (the first NSP nodes, whose act is 0) and the tail's (act of the last NSP pivots, nothing else) included; the slot of a pivot
    that is no interface node lies inside the workspace of the form (nAB value slots + nfins x nif slots of g)."""
    from bayesianinferencedl_amd import _ffi
    lib = _ffi.lib()
    bp, d, keep, _, out_ptr, out_col = _form(spaces, m)
    assert (d.NSF, d.NSP) == WINDOWS[m]
    n_rows = len(out_ptr) - 1
    rc, fits, fr, pr = _records(lib, d, bp, n_rows, out_ptr, out_col)
    assert rc == 0 and fits == 1, lib.finrom_last_error()
    cw, prow, poff = _functionals(lib, d, bp, n_rows, out_ptr, out_col)
    ntot, npost, NSP, nAB = d.npf + d.nif, d.npost, d.NSP, d.nAB
    gfin = d.nfins * ntot
    abmap = np.array(d.abmap[:3 * (gfin + npost)], np.int64).reshape(-1, 3)
    FgQ = np.array(d.qoi_FgQ[:gfin + npost])
    assert np.array_equal(fr["off"], abmap[:gfin] << 9) and np.array_equal(fr["fg"], FgQ[:gfin])
    assert not fr["pad0"].any() and not fr["pad1"].any() and not pr["pad0"].any() and not pr["pad1"].any()
    act = np.array(d.act[:npost])
    assert np.array_equal(pr["act"][NSP:], act) and not pr["act"][:NSP].any()
    body, tail = pr[:npost], pr[npost:]
    assert np.array_equal(body["off"], abmap[gfin:] << 9) and np.array_equal(body["fg"], FgQ[gfin:])
    assert np.array_equal(body["ex"], np.array(d.ent_extra[:npost]))
    ecp = np.array(d.ecp_ptr[:npost + 1])
    assert np.array_equal(body["c0"], ecp[:-1]) and np.array_equal(body["c1"], ecp[1:])
    assert np.array_equal(body["row"], prow) and np.array_equal(body["cw"], cw)
    iface = prow >= 0
    assert iface.any() and (~iface).any()
    assert np.array_equal(body["gv"][iface], (nAB + poff[iface]) << 9)
    dummy = body["gv"][~iface].astype(np.int64)
    assert (dummy >= 0).all() and (dummy % 512 == 0).all() and (dummy < (nAB + d.nfins * d.nif) * 512).all()
    for name in ("off", "gv", "ex", "c0", "c1", "row", "fg", "cw"):
        assert not tail[name].any(), name
    args, keep_ = _args(d, bp, n_rows, out_ptr, out_col)
    assert lib.finrom_fom_band_records_check(*args, fr.ctypes.data, pr.ctypes.data) == 0, lib.finrom_last_error()


@pytest.mark.parametrize("m", MS)
def test_validator_refuses_one_changed_field(spaces, m):
    """finrom_fom_band_records_check -- the check finrom_fom_set_band_mirror applies before it uploads the records -- rebuilds the
    source tables from the records: one field of one record changed, one case per field, is refused and named."""
    from bayesianinferencedl_amd import _ffi
    lib = _ffi.lib()
    bp, d, keep, _, out_ptr, out_col = _form(spaces, m)
    n_rows = len(out_ptr) - 1
    rc, fits, fr, pr = _records(lib, d, bp, n_rows, out_ptr, out_col)
    assert rc == 0 and fits == 1
    args, keep_ = _args(d, bp, n_rows, out_ptr, out_col)

    def check(f, p):
        return lib.finrom_fom_band_records_check(*args, f.ctypes.data, p.ctypes.data)
    assert check(fr, pr) == 0
    npost, NSP = d.npost, d.NSP
    t_if = int(np.nonzero(pr["row"][:npost] >= 0)[0][0])
    t_no = int(np.nonzero(pr["row"][:npost] < 0)[0][0])
    post_cases = [("off", npost // 2, 1, 512), ("off", 0, 0, 512), ("fg", 3, None, 1.0), ("act", NSP + 1, None, 1), ("act", 0, None, 1),
                  ("act", npost + NSP - 1, None, 1), ("ex", NSP + 2, None, 1), ("c0", 5, None, 1), ("c1", 5, None, 1),
                  ("row", t_if, None, 1), ("row", t_no, None, 1), ("gv", t_if, None, 512), ("gv", t_no, None, 4),
                  ("gv", t_no, None, (d.nAB + d.nfins * d.nif) * 512 - int(pr["gv"][t_no])), ("cw", 7, 4, 0.5), ("cw", t_if, 0, -0.25),
                  ("off", npost, 2, 512), ("row", npost + 1, None, -1)]
    for name, t, e, delta in post_cases:
        bad = pr.copy()
        if e is None:
            bad[name][t] += delta
        else:
            bad[name][t, e] += delta
        assert check(fr, bad) != 0, (name, t)
        assert b"pivot record" in lib.finrom_last_error()
    for name, t, e, delta in [("off", 0, 0, 512), ("off", len(fr) - 1, 2, -512), ("fg", len(fr) // 2, None, 2.0)]:
        bad = fr.copy()
        if e is None:
            bad[name][t] += delta
        else:
            bad[name][t, e] += delta
        assert check(bad, pr) != 0, (name, t)
    assert check(fr, pr) == 0


@pytest.mark.parametrize("m", MS)
def test_a_descriptor_the_form_does_not_fit_yields_no_records(spaces, m):
    """Six distinct rows (a post-only row once more, as a row of its own with an output column of its own): the descriptor is valid,
    keeps the stored-factor form, and no record is written; the check of handed-in records refuses it."""
    from bayesianinferencedl_amd import _ffi
    lib = _ffi.lib()
    bp, d, keep, _, out_ptr, out_col = _form(spaces, m)
    n_rows = len(out_ptr) - 1
    nq = d.qoi_obs_ptr[n_rows]
    o_post = [o for o in range(n_rows) if d.qoi_row_fin[o] < 0][0]
    t0, t1 = d.obs_ptr[o_post], d.obs_ptr[o_post + 1]
    nz = d.obs_ptr[n_rows]
    optr = np.array(list(d.obs_ptr[:n_rows + 1]) + [nz + (t1 - t0)], np.int32)
    oidx = np.array(list(d.obs_idx[:nz]) + list(d.obs_idx[t0:t1]), np.int32)
    ow = np.array(list(d.obs_w[:nz]) + list(d.obs_w[t0:t1]), np.float64)
    rf = np.array(list(d.qoi_row_fin[:n_rows]) + [-1], np.int32)
    qptr = np.array(list(d.qoi_obs_ptr[:n_rows + 1]) + [nq + (t1 - t0)], np.int32)
    qidx = np.array(list(d.qoi_obs_idx[:nq]) + list(d.obs_idx[t0:t1]), np.int32)
    qw = np.array(list(d.qoi_obs_w[:nq]) + list(d.obs_w[t0:t1]), np.float64)
    saved = (d.obs_ptr, d.obs_idx, d.obs_w, d.qoi_row_fin, d.qoi_obs_ptr, d.qoi_obs_idx, d.qoi_obs_w)
    P32, P64 = _ffi.c_i32p, _ffi.c_f64p
    try:
        d.obs_ptr, d.obs_idx, d.obs_w = optr.ctypes.data_as(P32), oidx.ctypes.data_as(P32), ow.ctypes.data_as(P64)
        d.qoi_row_fin, d.qoi_obs_ptr, d.qoi_obs_idx, d.qoi_obs_w = (rf.ctypes.data_as(P32), qptr.ctypes.data_as(P32),
                                                                    qidx.ctypes.data_as(P32), qw.ctypes.data_as(P64))
        op6, oc6 = list(out_ptr) + [10], list(out_col) + [9]
        rc, fits, fr, pr = _records(lib, d, bp, n_rows + 1, op6, oc6, n_obs=10)
        assert rc == 0 and fits == 0, lib.finrom_last_error()
        assert (fr["pad0"] == -7).all() and (pr["pad0"] == -7).all() and not fr["off"].any() and not pr["off"].any()
        args, keep_ = _args(d, bp, n_rows + 1, op6, oc6, n_obs=10)
        assert lib.finrom_fom_band_records_check(*args, fr.ctypes.data, pr.ctypes.data) != 0
    finally:
        d.obs_ptr, d.obs_idx, d.obs_w, d.qoi_row_fin, d.qoi_obs_ptr, d.qoi_obs_idx, d.qoi_obs_w = saved
    rc, fits, fr, pr = _records(lib, d, bp, n_rows, out_ptr, out_col)
    assert rc == 0 and fits == 1
