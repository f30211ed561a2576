"""The flagged-sample contract of DESIGN 1 / DESIGN 2 ("What a flagged sample is held to") as data and one checker, for
tests/test_gpu_rom_flags.py and tests/test_gpu_fom_flags.py; tests/test_flag_contract_host.py holds the checker itself to its controls.

A batched call fails per sample: a sample that cannot be factored gets info[s] != 0 and NaN outputs, and no other sample is touched.
  1. exactly flagged      info[s] == flag_bit for every poisoned sample, info[s] == 0 for every other
  2. flagged rows are not numbers: every entry of a flagged sample's qoi_r / qoi, J, g / grad is NaN, its w_r not all finite
  3. neighbours keep their bits: every output of every other sample equals, bit for bit, the same sample's of the clean batch
A NaN in a sample's DATA row (gradient entry points, per-sample data) is not a flagged sample: info stays 0, qoi_r and w_r keep the
clean bits, J and every entry of g are NaN.

Poisons (one sample's row of theta, FOM: x): one entry NaN, one entry +inf, one entry 1e200 (finite, A_r overflows), the whole row
1e200; for the FOM also one negative conductivity (an indefinite operator whatever the rounding).  Positions: the first sample of a
four-sample workgroup (4), a middle wave of another (9), the middle of the second 16-sample tile (21), the last sample of the batch
(the ragged tail).  Kinds are dealt over the positions and rotated by case_id: every kind meets every form, not every position."""
import numpy as np

ROM_KINDS = ("nan", "inf", "big", "bigrow")
FOM_KINDS = ("nan", "inf", "big", "bigrow", "neg")
ROM_FLAG, FOM_FLAG = 2, 1
FOM_VALID_KINDS = ("big", "bigrow")                         # x = 1e200 is a positive definite FOM operator with finite entries: see check_contract's `either`
MAX_BAD = 4
DATA_KEYS = ("J", "g", "grad")                              # what a NaN in a sample's data row turns into NaN, and nothing else
NAN_KEYS = ("qoi_r", "qoi", "J", "g", "grad")              # every entry of a flagged row is NaN
STATE_KEYS = ("w_r",)                                       # not all finite in a flagged row (some forms leave a part of it finite)


def positions(S):
    """The poisoned rows of a batch of S samples (the table of DESIGN.md section 2, "What a flagged sample is held to")."""
    if S < 64:
        assert S >= 2
        return [1]
    if S == 64:
        return [4, 9, 63]
    return [4, 9, 21, S - 1]


def kind_of(case_id, i, kinds=ROM_KINDS):
    """The kind of poison of the i-th poisoned row of case `case_id`: the kinds dealt over the rows and rotated by case."""
    return kinds[(case_id + i) % len(kinds)]


def kinds_at(S, case_id, kinds=ROM_KINDS):
    """The kind of poison at each position of `positions(S)`."""
    return [kind_of(case_id, i, kinds) for i in range(len(positions(S)))]


def poison_row(row, kind, entry):
    """One row with one poison; `entry` picks the column (modulo the row's length)."""
    row = np.array(row, np.float64)
    e = entry % row.size
    if kind == "nan":
        row[e] = np.nan
    elif kind == "inf":
        row[e] = np.inf
    elif kind == "big":
        row[e] = 1e200
    elif kind == "bigrow":
        row[:] = 1e200
    elif kind == "neg":
        row[e] = -5.0 if row.size <= 9 else -50.0           # a nodal field: the elements around the node get a negative mean
    else:
        raise ValueError(kind)
    return row


def poisoned(TH, S, case_id, kinds=ROM_KINDS, rows=None):
    """-> (a copy of TH[:S] with positions(S) (or `rows`) poisoned, the list of bad rows).  kinds_at(S, case_id, kinds) says with what."""
    out = np.array(np.asarray(TH)[:S], np.float64)
    bad = positions(S) if rows is None else list(rows)
    assert len(bad) <= MAX_BAD and max(bad) < S
    for i, s in enumerate(bad):
        out[s] = poison_row(out[s], kind_of(case_id, i, kinds), 3 * case_id + 2 * i)
    return out, bad


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1) if len(a) else np.zeros((0, 0), np.uint8)


def rows_with_other_bits(a, b):
    """The rows in which two [S, ...] arrays of one shape and dtype differ in a bit."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return np.nonzero((_bits(a) != _bits(b)).any(axis=1))[0].tolist()


def check_contract(label, clean, dirty, bad, keys, flag_bit, data_bad=(), either=()):
    """clean / dirty: the output dictionaries of the same call on the clean and on the poisoned batch; bad: the poisoned rows;
    keys: EVERY output array of the call but info; data_bad: rows with a NaN in their data row only; either: rows with an extreme
    but valid input (the FOM at 1e200), which a form may solve or flag: flagged with every entry NaN, or info == 0 with every entry
    finite -- nothing in between; they count as poisoned and are not compared.  Asserts items 1 to 3, prints
    and returns per key how many rows it compared bit for bit, and fails if that is fewer than S - 4 for any key."""
    bad, data_bad, either = sorted(int(s) for s in bad), sorted(int(s) for s in data_bad), sorted(int(s) for s in either)
    assert len(bad) + len(data_bad) + len(either) <= MAX_BAD and len(set(bad) | set(data_bad) | set(either)) == len(bad) + len(data_bad) + len(either), (label, bad, data_bad, either)
    info_c, info_d = np.asarray(clean["info"]), np.asarray(dirty["info"])
    bad = sorted(bad + [s for s in either if info_d[s] != 0])      # a flagged `either` row is held to everything a poisoned row is
    solved = [s for s in either if s not in bad]
    S = info_d.shape[0]
    for out, name in ((clean, "clean"), (dirty, "poisoned")):
        missing = [k for k in keys if k not in out or out[k] is None]
        assert not missing, f"{label}: key skipped: {missing} not in the {name} outputs"
        extra = [k for k in out if k != "info" and out[k] is not None and k not in keys]
        assert not extra, f"{label}: key skipped: the {name} call returned {extra}, which nobody compares"
    assert info_c.shape == (S,) and not info_c.any(), f"{label}: the clean batch is flagged at {np.nonzero(info_c)[0].tolist()}"
    for k in keys:
        assert np.isfinite(np.asarray(clean[k])).all(), f"{label}: the clean batch's {k} is not finite"
    # 1. exactly flagged
    missed = [s for s in bad if info_d[s] == 0]
    assert not missed, f"{label}: poisoned rows {missed} are not flagged (info == 0)"
    wrong = [s for s in range(S) if s not in bad and info_d[s] != 0]
    assert not wrong, f"{label}: rows {wrong} are flagged and were not poisoned (info {info_d[wrong].tolist()})"
    other = [s for s in bad if info_d[s] != flag_bit]
    assert not other, f"{label}: flagged rows {other} carry info {info_d[other].tolist()}, not the bit {flag_bit}"
    good = np.array([s for s in range(S) if s not in bad and s not in data_bad and s not in solved], dtype=np.int64)
    compared = {}
    for k in keys:
        a, c = np.asarray(dirty[k]), np.asarray(clean[k])
        assert a.shape == c.shape and a.shape[0] == S, (label, k, a.shape, c.shape)
        rows = a.reshape(S, -1)
        # a row that is not a number and not flagged
        loose = [s for s in range(S) if s not in bad and not (s in data_bad and k in DATA_KEYS) and not np.isfinite(rows[s]).all()]
        assert not loose, f"{label}: {k}: rows {loose} are not finite with info == 0"
        # 2. flagged rows are not numbers
        if k in NAN_KEYS:
            finite = [s for s in bad if not np.isnan(rows[s]).all()]
            assert not finite, f"{label}: {k}: flagged rows {finite} hold entries that are not NaN"
        elif k in STATE_KEYS:
            finite = [s for s in bad if np.isfinite(rows[s]).all()]
            assert not finite, f"{label}: {k}: flagged rows {finite} are all finite"
            partly = [s for s in bad if np.isfinite(rows[s]).any()]
            if partly:
                print(f"{label}: {k}: flagged rows {partly} are only partly not finite")
        if k in DATA_KEYS:
            finite = [s for s in data_bad if not np.isnan(rows[s]).all()]
            assert not finite, f"{label}: {k}: rows {finite} with a NaN in their data hold entries that are not NaN"
        # 3. neighbours keep their bits (a row with poisoned data keeps the bits of everything but J and g)
        cmp_rows = good if k in DATA_KEYS else np.array(sorted(good.tolist() + data_bad), dtype=np.int64)
        moved = [int(cmp_rows[i]) for i in rows_with_other_bits(a[cmp_rows], c[cmp_rows])]
        assert not moved, f"{label}: {k}: rows {moved} do not have the clean batch's bits"
        compared[k] = len(cmp_rows)
        assert compared[k] >= S - MAX_BAD, f"{label}: {k}: only {compared[k]} of {S} rows compared"
    print(f"{label}: flagged {bad}" + (f", solved unflagged and finite {solved}" if solved else "") + (f", data poisoned {data_bad}" if data_bad else "") + ", rows compared bit for bit: " +
          ", ".join(f"{k} {n}" for k, n in compared.items()))
    return compared


def same_bits(label, a, b, keys, rows=None):
    """Every key (and info) of two calls' outputs bit for bit, on the leading `rows` rows of both."""
    for k in tuple(keys) + ("info",):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if rows is not None:
            x, y = x[:rows], y[:rows]
        moved = rows_with_other_bits(x, y)
        assert not moved, f"{label}: {k}: rows {moved} differ"
