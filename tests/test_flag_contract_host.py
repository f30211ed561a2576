"""The checker of the flagged-sample contract (tests/flag_cases.py) on synthetic outputs, no GPU: it accepts a conforming set and
rejects, each for its own reason, the seven ways a kernel can break the contract that the device tests rely on it to see."""
import numpy as np
import pytest

import flag_cases as F

S, R, NOBS, P = 70, 5, 9, 9
KEYS = ("qoi_r", "w_r", "J", "g")


def _outputs(bad=(), data_bad=(), flag=F.ROM_FLAG):
    rng = np.random.default_rng(7)
    out = {"qoi_r": rng.uniform(0.1, 1.0, (S, NOBS)), "w_r": rng.standard_normal((S, R)), "J": rng.uniform(0.1, 1.0, S),
           "g": rng.standard_normal((S, P)), "info": np.zeros(S, np.int32)}
    for s in bad:
        out["info"][s] = flag
        for k in KEYS:
            out[k][s] = np.nan
    for s in data_bad:
        out["J"][s] = np.nan; out["g"][s] = np.nan
    return out


BAD = F.positions(S)


def _flip_low_bit(a, idx):
    a.view(np.uint64)[idx] ^= np.uint64(1)


def test_the_poison_table():
    """Positions as the table of DESIGN.md section 2 has them, four rows at most; every kind of poison meets every form within four consecutive
    case ids (FOM: five); a poisoned batch differs from the clean one in exactly the bad rows, and every bad row is bad."""
    assert F.positions(3) == [1] and F.positions(64) == [4, 9, 63]
    for n in (65, 70, 200, 301):
        assert F.positions(n) == [4, 9, 21, n - 1]
    for kinds in (F.ROM_KINDS, F.FOM_KINDS):
        for n in (3, 64, 70):
            assert {k for c in range(len(kinds)) for k in F.kinds_at(n, c, kinds)} == set(kinds)
        assert set(F.kinds_at(70, 0, kinds)) == set(kinds[:4])
    TH = np.random.default_rng(0).uniform(0.1, 10.0, (301, 9))
    for case_id in range(8):
        for n in (3, 64, 65, 301):
            out, bad = F.poisoned(TH, n, case_id)
            assert bad == F.positions(n) and out.shape == (n, 9)
            assert F.rows_with_other_bits(out, TH[:n]) == bad
            for s, kind in zip(bad, F.kinds_at(n, case_id)):
                row = out[s]
                assert {"nan": np.isnan(row).sum() == 1, "inf": np.isposinf(row).sum() == 1, "big": (row == 1e200).sum() == 1,
                        "bigrow": (row == 1e200).all()}[kind], (kind, row)
    out, bad = F.poisoned(TH, 70, 1, F.FOM_KINDS)
    assert F.kinds_at(70, 1, F.FOM_KINDS) == ["inf", "big", "bigrow", "neg"] and (out[69] < 0).sum() == 1
    assert TH[4, 0] != 1e200                                 # (the input is not written)


def test_a_conforming_set_is_accepted():
    n = F.check_contract("conforming", _outputs(), _outputs(BAD), BAD, KEYS, F.ROM_FLAG)
    assert n == {k: S - 4 for k in KEYS}
    # a partly NaN w_r in a flagged row is allowed
    d = _outputs(BAD)
    d["w_r"][BAD[0], 1:] = 0.5
    F.check_contract("partly NaN w_r", _outputs(), d, BAD, KEYS, F.ROM_FLAG)
    # a NaN in a data row: info 0, J and g NaN, qoi_r and w_r with the clean bits and compared
    n = F.check_contract("data row", _outputs(), _outputs(BAD[:3], data_bad=[BAD[3]]), BAD[:3], KEYS, F.ROM_FLAG, data_bad=[BAD[3]])
    assert n == {"qoi_r": S - 3, "w_r": S - 3, "J": S - 4, "g": S - 4}
    F.check_contract("FOM", _outputs(), _outputs(BAD, flag=F.FOM_FLAG), BAD, KEYS, F.FOM_FLAG)


def _rejected(match, dirty, clean=None, bad=BAD, keys=KEYS, **kw):
    with pytest.raises(AssertionError, match=match):
        F.check_contract("control", clean or _outputs(), dirty, bad, keys, F.ROM_FLAG, **kw)


def test_a_neighbour_with_one_changed_low_bit_is_rejected():
    for k, s in (("qoi_r", 5), ("w_r", 8), ("J", 20), ("g", 68)):
        d = _outputs(BAD)
        _flip_low_bit(d[k].reshape(S, -1)[s], 0)
        _rejected(rf"{k}: rows \[{s}\] do not have the clean batch's bits", d)


def test_a_nan_leaked_into_a_neighbours_g_is_rejected():
    d = _outputs(BAD)
    d["g"][22, 3] = np.nan                                   # the tile neighbour of row 21
    _rejected(r"g: rows \[22\] are not finite with info == 0", d)


def test_a_flagged_row_with_one_finite_qoi_entry_is_rejected():
    d = _outputs(BAD)
    d["qoi_r"][9, 8] = 0.25
    _rejected(r"qoi_r: flagged rows \[9\] hold entries that are not NaN", d)
    d = _outputs(BAD)
    d["w_r"][9] = 0.25
    _rejected(r"w_r: flagged rows \[9\] are all finite", d)


def test_a_nan_row_with_info_zero_is_rejected():
    d = _outputs(BAD)
    d["info"][21] = 0
    _rejected(r"poisoned rows \[21\] are not flagged", d)
    d = _outputs(BAD)
    d["qoi_r"][30] = np.nan                                  # nobody poisoned row 30
    _rejected(r"qoi_r: rows \[30\] are not finite with info == 0", d)


def test_a_flag_on_the_wrong_row_is_rejected():
    d = _outputs(BAD)
    d["info"][21], d["info"][22] = 0, F.ROM_FLAG             # the flag one row off, the NaNs in place
    _rejected(r"poisoned rows \[21\] are not flagged", d)
    d = _outputs(BAD)
    d["info"][4] = 1                                         # the other path's bit
    _rejected(r"flagged rows \[4\] carry info \[1\], not the bit 2", d)


def test_a_clean_row_whose_info_was_set_is_rejected():
    d = _outputs(BAD)
    d["info"][0] = F.ROM_FLAG
    _rejected(r"rows \[0\] are flagged and were not poisoned", d)
    c = _outputs()
    c["info"][3] = F.ROM_FLAG
    _rejected(r"the clean batch is flagged at \[3\]", _outputs(BAD), clean=c)


def test_a_silently_skipped_key_is_rejected():
    d = _outputs(BAD)
    del d["g"]
    _rejected(r"key skipped: \['g'\] not in the poisoned outputs", d)
    _rejected(r"key skipped: the clean call returned \['g'\], which nobody compares", _outputs(BAD), keys=("qoi_r", "w_r", "J"))
    # too many rows left out of the comparison
    with pytest.raises(AssertionError):
        F.check_contract("control", _outputs(), _outputs(BAD + [30]), BAD + [30], KEYS, F.ROM_FLAG)


def test_a_data_row_poison_must_leave_the_solve_alone_and_j_g_nan():
    d = _outputs(BAD[:3], data_bad=[BAD[3]])
    d["g"][BAD[3], 2] = 0.0
    _rejected(r"g: rows \[69\] with a NaN in their data hold entries that are not NaN", d, bad=BAD[:3], data_bad=[BAD[3]])
    d = _outputs(BAD[:3], data_bad=[BAD[3]])
    _flip_low_bit(d["qoi_r"][BAD[3]], 0)
    _rejected(r"qoi_r: rows \[69\] do not have the clean batch's bits", d, bad=BAD[:3], data_bad=[BAD[3]])
    d = _outputs(BAD[:3], data_bad=[BAD[3]])
    d["info"][BAD[3]] = F.ROM_FLAG
    _rejected(r"rows \[69\] are flagged and were not poisoned", d, bad=BAD[:3], data_bad=[BAD[3]])


def test_a_valid_extreme_row_is_solved_or_flagged_and_nothing_in_between():
    """`either` (the FOM at 1e200): flagged with NaN outputs, or info == 0 with finite ones of whatever value; not compared."""
    d = _outputs(BAD)                                        # row 21 flagged and NaN like a poisoned one
    n = F.check_contract("flagged", _outputs(), d, [4, 9, 69], KEYS, F.ROM_FLAG, either=[21])
    assert n == {k: S - 4 for k in KEYS}
    d = _outputs([4, 9, 69])
    d["g"][21] *= 3.0                                        # solved: other numbers than the clean row's, finite, info 0
    F.check_contract("solved", _outputs(), d, [4, 9, 69], KEYS, F.ROM_FLAG, either=[21])
    d["g"][21, 0] = np.inf
    _rejected(r"g: rows \[21\] are not finite with info == 0", d, bad=[4, 9, 69], either=[21])
    d = _outputs([4, 9, 69])
    d["info"][21] = F.ROM_FLAG                               # flagged, and numbers came back
    _rejected(r"qoi_r: flagged rows \[21\] hold entries that are not NaN", d, bad=[4, 9, 69], either=[21])
    with pytest.raises(AssertionError):                      # counted against the cap of four
        F.check_contract("cap", _outputs(), _outputs(BAD), BAD, KEYS, F.ROM_FLAG, either=[30])


def test_same_bits_sees_one_bit():
    a, b = _outputs(), _outputs()
    F.same_bits("same", a, b, KEYS)
    F.same_bits("leading rows", a, {k: v[:66] for k, v in b.items()}, KEYS, rows=66)
    _flip_low_bit(b["g"][40], 1)
    with pytest.raises(AssertionError, match=r"g: rows \[40\] differ"):
        F.same_bits("one bit", a, b, KEYS)
    b = _outputs()
    b["info"][2] = 2
    with pytest.raises(AssertionError, match=r"info: rows \[2\] differ"):
        F.same_bits("info", a, b, KEYS)
