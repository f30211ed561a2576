"""Host logic of the SCALE-FREE short half list (DESIGN 4b'', build_grouped_tables' group_pays), no GPU.  The short list has lost the
interior rows whose k-steps carry {theta_d} alone, so no leading parameter pays for the rescale a group costs: its k-steps sit in
segment 0 with their usual coefficients (theta_d T_d + T_0), no record names a 1/theta scalar, and the only factors left are the
exact 2 where the weight class changes and the final one.  FINROM_ROM_SHORT_GROUPED=1 brings the grouped short list back; the
all-rows half list is the same list either way."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_rom_skip_rows_host import _counts, _form

CASES = [(4, 16, 30), (12, 80, 506)]
SWITCH = "FINROM_ROM_SHORT_GROUPED"


def _load(form, r, short=True):
    """The builder's tables of the short (or the all-rows half) descriptor: nkg, ext_final, records, rows, factor definitions."""
    from bayesianinferencedl_amd import _ffi
    d, keep = (form["desc_short"], form["keep_short"]) if short else (form["desc"], form["keep"])
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


def _live(kmg, tvg, nkg):
    """The records in front of the padding (their rows are not all zero)."""
    return [rec for rec in kmg[:nkg] if tvg[rec[0]:rec[0] + rec[1]].any()]


def _walk(tables, r, theta):
    """A_r accumulated as proj_main_grouped accumulates it (test_rom_skip_rows_host._walk)."""
    nkg, ext_final, kmg, tvg, ext_def = tables
    rp = tvg.shape[2]
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


def _thetas(twin):
    """The gate's 16 seeded probes (RomEngine.mirror_probe_eps: seed 0, log-uniform per mirror pair) and the corners of [0.1, 10]."""
    from bayesianinferencedl_amd.engine import RomEngine
    lo, hi = RomEngine.MIRROR_PROBE_RANGE
    P = len(twin)
    rep = np.minimum(np.arange(P), np.asarray(twin))
    rng = np.random.default_rng(0)
    probes = [np.exp(rng.uniform(np.log(lo), np.log(hi), P))[rep] for _ in range(RomEngine.MIRROR_PROBES)]
    free = np.unique(rep)
    corners = []
    for bits in itertools.product((lo, hi), repeat=len(free)):
        th = np.zeros(P)
        th[free] = bits
        corners.append(th[rep])
    return probes, corners


@pytest.mark.parametrize("m,r,ndrop", CASES)
def test_short_list_is_scale_free(m, r, ndrop, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    ops, form = _form(m, r)
    assert form["dropped"] == ndrop
    P = form["desc_short"].P
    tables = _load(form, r)
    nkg, ext_final, kmg, tvg, ext_def = tables
    live = _live(kmg, tvg, nkg)
    # one rescale in the list, the weight-class change: an exact 2, no conductivity in it; the final factor exists and is 1
    opens = [rec for rec in live if rec[2] & 2]
    assert len(opens) == 1 and tuple(ext_def[opens[0][3]]) == (0, 0, 3)
    assert ((ext_def[:, 2] & 2) != 0).sum() == 1 and tuple(ext_def[ext_final]) == (0, 0, 1)
    assert len(ext_def) == 1 + 2 * P + 2
    # no live record names a 1/theta scalar (ext[P + 1 .. 2 P]); a two-term record is T_0 + theta_d T_d
    for slot, nt, flags, fidx, *cf in live:
        assert all(not (P < cf[t] <= 2 * P) for t in range(nt)), (slot, nt, cf)
        if nt == 2 and cf[0] == 0:
            assert flags & 1 and 1 <= cf[1] <= P
    # the counts are those of the grouped short list -- the same k-steps, elsewhere in the list: live, with padding, and with a
    # multiply-add (two or more terms).  The builder's own count of k-steps with ANY vector arithmetic is larger by the k-steps
    # {theta_d} alone, which the grouped list loads as they are and this one multiplies (one at m = 12: 80 against 79).
    counts = _counts(form, short=True)
    monkeypatch.setenv(SWITCH, "1")
    old = _load(form, r)
    counts_old = _counts(form, short=True)
    monkeypatch.delenv(SWITCH)
    old_live = _live(old[2], old[3], old[0])
    fma = sum(1 for rec in live if rec[1] >= 2)
    lone = sum(1 for rec in live if rec[1] == 1 and rec[4] != 0)
    assert counts[:2] == counts_old[:2] and old[0] == nkg and len(old_live) == len(live) == counts[1]
    assert fma == sum(1 for rec in old_live if rec[1] >= 2) == counts_old[2] and counts[2] == fma + lone
    print(f"m = {m}, r = {r}: {counts[1]} live k-steps, {nkg} with padding, {fma} with a multiply-add, {lone} with a lone multiply; "
          f"factors {len(ext_def) - 1 - 2 * P} (grouped: {len(old[4]) - 1 - 2 * P})")
    if m == 12:
        assert (counts[1], nkg, fma) == (80, 81, 79)
    # with the switch the old structure is back: a rescale per group, 1/theta in the records
    assert sum(1 for rec in old_live if rec[2] & 2) > 1
    assert any(P < rec[4 + t] <= 2 * P for rec in old_live for t in range(rec[1]))
    assert len(old[4]) > len(ext_def)


@pytest.mark.parametrize("m,r,ndrop", CASES)
def test_scale_free_walk(m, r, ndrop, monkeypatch):
    """The NumPy walk of the scale-free tables equals psi_s[kept]^T W psi_s[kept] to 1e-12 max|A_r| at the gate's 16 probes and at the
    32 corners of [0.1, 10]^5 (1e-12: the bound of the grouped lists' walks; both are sums of the same ~n r^2 products in fp64)."""
    monkeypatch.delenv(SWITCH, raising=False)
    ops, form = _form(m, r)
    Ts, rows, weight, dropped = form["Ts"], form["rows"], form["weight"], form["dropped_rows"]
    tables = _load(form, r)
    probes, corners = _thetas(form["twin"])
    assert len(probes) == 16 and len(corners) == 32
    worst = 0.0
    for theta in probes + corners:
        th1 = np.concatenate([[1.0], theta])
        ph = sum(th1[p] * Ts[p] for p in range(len(Ts)))[rows][~dropped]
        want = (ph.T * weight[~dropped]) @ ph
        worst = max(worst, np.max(np.abs(_walk(tables, r, theta) - want)) / np.abs(want).max())
    print(f"m = {m}, r = {r}: walk vs kept rows, 16 probes + 32 corners: {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("m,r,ndrop", CASES)
def test_all_rows_half_list_keeps_its_groups(m, r, ndrop, monkeypatch):
    """The half descriptor with every row is not a short list: a group per leading parameter, and the same tables with the switch."""
    monkeypatch.delenv(SWITCH, raising=False)
    ops, form = _form(m, r)
    P = form["desc"].P
    a = _load(form, r, short=False)
    monkeypatch.setenv(SWITCH, "1")
    b = _load(form, r, short=False)
    monkeypatch.delenv(SWITCH)
    assert a[0] == b[0] and a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))
    live = _live(a[2], a[3], a[0])
    assert sum(1 for rec in live if rec[2] & 2) > 1 and any(P < rec[4 + t] <= 2 * P for rec in live for t in range(rec[1]))
