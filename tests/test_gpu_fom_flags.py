"""finrom_fom_gradient on its three paths (band adjoint, small-batch kernel, interpreter) and the Hessian action with poisoned samples,
held to the flagged-sample contract of tests/flag_cases.py ("What a flagged sample is held to"): exactly the poisoned
samples flagged with the FOM's bit 1, their grad, J and qoi NaN in every entry, every other sample's outputs the bits of the same
call on the clean batch (same handle, same S, same finrom_fom_last_path), and no residue on the handle afterwards.  No yardstick
here: tests/test_gpu_fom_ld.py holds the clean batches' accuracy; handles and batches are its (tests/fom_ld_cases.py).

S = 70 (a full block of 64 lanes and six live lanes of a second); poisoned: lanes 0, 37 and 63 of the first block and the last
sample of the second.  Poisons of x: one entry NaN, one entry +inf, one negative conductivity (an indefinite operator whatever the
rounding) -- these must be flagged.  One entry 1e200 and the whole row 1e200 leave the full-order operator positive definite with
finite entries (A is linear in x; nothing is squared as in the reduced A_r = psi^T psi): a path may solve such a sample or flag it,
and is held to "flagged and NaN, or info == 0 and finite -- nothing in between" (check_contract's `either`); what each path did is
printed.  With per-sample data also a NaN in a sample's data row: info 0, qoi with the clean bits, J and grad NaN.
Measured on the MI355X: every NaN, +inf and negative row flagged and NaN on every path, every neighbour's bits kept; of the 26 rows
at 1e200 in the 16 gradient calls 16 came back solved and finite, 10 flagged and NaN (the Robin term is 200 digits below such a
sub-domain's stiffness: what is factored there is singular to rounding, and its last pivot is rounding noise)."""
import numpy as np
import pytest

import flag_cases as F
import fom_ld_cases as Y

pytestmark = pytest.mark.gpu
S = Y.S_BATCH
ROWS = [0, 37, 63, S - 1]
KEYS = ("grad", "J", "qoi")
PATHS = [("band adjoint", 4, True, False, "band_registers"), ("band adjoint", 16, True, False, "band_lds_4wave"),
         ("small-batch kernel", 4, True, True, "small_lds"), ("interpreter", 4, False, False, "interpreter")]


@pytest.fixture(scope="module")
def handles(spaces):
    """(Fin, FomEngine, Case) per (m, kind, band plan or not), made once (the pattern of tests/test_gpu_fom_ld.py)."""
    import bayesianinferencedl_amd.engine as E
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    fins = {}

    def get(m, kind, band=True):
        c = Y.case(m, kind)
        old = E.USE_BAND
        try:
            E.USE_BAND = band
            if (m, band) not in fins:
                fins[(m, band)] = Fin(spaces(m))
            fin = fins[(m, band)]
            eng = fin._engine(kind)
        finally:
            E.USE_BAND = old
        assert (eng.band is not None) == band
        return fin, eng, c
    return get


def _small(eng, on):
    import bayesianinferencedl_amd.engine as E
    in_lds = (eng.plan.nnzL + 3 * eng.plan.n + eng.xdim) * 8 <= 156 * 1024
    eng.set_small_max((E.SMALL_MAX if in_lds else E.SMALL_MAX_GLOBAL) if on else 0)


def _split(case_id):
    """The poisoned batch's rows by what the contract asks of them: (must be flagged, valid at 1e200), and the kinds by row."""
    kinds = [F.kind_of(case_id, i, F.FOM_KINDS) for i in range(len(ROWS))]
    bad = [s for s, k in zip(ROWS, kinds) if k not in F.FOM_VALID_KINDS]
    return bad, [s for s in ROWS if s not in bad], dict(zip(ROWS, kinds))


@pytest.mark.parametrize("kind", ["field", "five"])
@pytest.mark.parametrize("name,m,band,small,path", PATHS, ids=[f"{p[0]}-m{p[1]}" for p in PATHS])
def test_gradient_with_poisoned_samples(handles, name, m, band, small, path, kind):
    """Items 1 to 4 on grad, J, qoi and info, with shared and with per-sample data.  The smaller batch of item 4 is S minus one
    workgroup: six samples for the 64-lane blocks of the band adjoint and the interpreter (the small-batch threshold is out of the
    way, so they keep their path), 69 for the small-batch kernel (one workgroup per sample)."""
    fin, eng, c = handles(m, kind, band=band)
    _small(eng, small)
    X = c.X[:S]
    base = 2 * PATHS.index((name, m, band, small, path)) + (kind == "five")
    for per_sample, data in ((False, c.data), (True, c.D[:S])):
        case_id = base + 3 * per_sample
        label = f"FOM gradient, {name}, m = {m}, {kind}, {'per-sample' if per_sample else 'shared'} data"
        clean = eng.gradient(X, data)
        assert eng.last_path() == path, eng.last_path()
        Xd, rows = F.poisoned(X, S, case_id, F.FOM_KINDS, rows=ROWS)
        bad, either, kinds = _split(case_id)
        dirty = eng.gradient(Xd, data)
        assert eng.last_path() == path
        F.check_contract(f"{label}, path {path}, poisons {kinds}", clean, dirty, bad, KEYS, F.FOM_FLAG, either=either)
        # a row at 1e200 that came back solved: its J is the misfit of the qoi it returned for its own data (fp64 sum of n_obs squares)
        for s in either:
            if np.asarray(dirty["info"])[s] == 0:
                res = np.asarray(dirty["qoi"])[s] - (data[s] if per_sample else data)
                assert abs(np.asarray(dirty["J"])[s] - 0.5 * res @ res) <= 1e-12 * 0.5 * res @ res, (label, s)
        # 4. no residue: clean again, and a smaller clean batch on the same path
        F.same_bits(f"{label}: clean after poisoned", clean, eng.gradient(X, data), KEYS)
        n = S - 1 if small else S - 64
        less = eng.gradient(X[:n], data[:n] if per_sample else data)
        assert eng.last_path() == path
        F.same_bits(f"{label}: S = {n} after poisoned", clean, less, KEYS, rows=n)
        if per_sample:
            Dn = np.array(data)
            for i, s in enumerate(ROWS):
                Dn[s, (case_id + 2 * i) % Dn.shape[1]] = np.nan
            dirty = eng.gradient(X, Dn)
            assert eng.last_path() == path
            F.check_contract(f"{label}, path {path}, NaN in the data rows {ROWS}", clean, dirty, [], KEYS, F.FOM_FLAG, data_bad=ROWS)


def test_hessian_action_with_an_indefinite_sample(handles):
    """Fin.hessian_action_batch at m = 4, six samples, sample 3 with one negative nodal conductivity: the forward solve flags it and
    the routine reports through an exception on the Python side (np.linalg.LinAlgError) -- it returns nothing for the batch, so items
    2 and 3 have no outputs to hold; item 1 is held on the forward solve it runs (info == 1 at sample 3 only, w and qoi NaN there,
    the five neighbours' bits kept), and the clean action after the refused one returns the bits of the one before (item 4)."""
    fin, eng, c = handles(4, "field")
    n = Y.HESSIAN[(4, "field", False)]
    assert n == 6
    first = fin.hessian_action_batch(c.X[:n], c.U[:n], c.data)
    assert eng.last_path() == "band_registers" and np.isfinite(first).all()
    X = c.X[:n].copy()
    X[3] = F.poison_row(X[3], "neg", 11)
    with pytest.raises(np.linalg.LinAlgError):
        fin.hessian_action_batch(X, c.U[:n], c.data)
    clean, dirty = eng.solve(c.X[:n], want_w=True), eng.solve(X, want_w=True)
    info = np.asarray(dirty["info"])
    assert info.tolist() == [0, 0, 0, F.FOM_FLAG, 0, 0]
    assert np.isnan(np.asarray(dirty["w"])[3]).all() and np.isnan(np.asarray(dirty["qoi"])[3]).all()
    good = [0, 1, 2, 4, 5]
    for k in ("w", "qoi"):
        assert not F.rows_with_other_bits(np.asarray(dirty[k])[good], np.asarray(clean[k])[good]), k
    again = fin.hessian_action_batch(c.X[:n], c.U[:n], c.data)
    assert not F.rows_with_other_bits(again, first)
    print("Hessian action, m = 4, one indefinite sample among six: reported by np.linalg.LinAlgError for the whole batch, no outputs; "
          "its forward solve flags sample 3 alone with info 1; the clean action afterwards has the first one's bits")


# ---- a prefilled info ------------------------------------------------------------------------------------------------------------
def test_a_prefilled_info_is_ored_into(handles):
    """finrom_fom_solve, finrom_fom_gradient and finrom_fom_solve_rhs OR bit 1 into the info they are given and clear nothing
    (include/finrom.h): 0x40 in a clean row (5) and in a poisoned one (37) comes back as 0x40 and 0x41, every other row as from a
    zeroed info.  m = 4, five fin conductivities, S = 70: the band sweep and the band adjoint."""
    from bayesianinferencedl_amd._ffi import DeviceBuffer, check, lib
    fin, eng, c = handles(4, "five")
    _small(eng, False)
    eng._enable_gradient()
    X, bad = F.poisoned(c.X[:S], S, 0, ("neg", "nan", "inf"), rows=ROWS[:3])
    assert 37 in bad and 5 not in bad
    pre = np.zeros(S, np.int32)
    pre[[5, 37]] = 0x40
    plain = np.asarray(eng.solve(X)["info"])                # what a zeroed info comes back as
    assert all(plain[s] == F.FOM_FLAG for s in bad) and not plain[[s for s in range(S) if s not in bad]].any()
    want = pre | plain

    def dev(a):
        return DeviceBuffer.from_numpy(np.ascontiguousarray(a))
    x, rhs, data = dev(X), dev(Y.case(4, "field").R[:S]), dev(c.D[:S])
    nrhs = Y.NRHS
    q, g, J, out = (DeviceBuffer(8 * S * k) for k in (eng.n_obs, eng.xdim, 1, nrhs * eng.n))
    calls = {
        "finrom_fom_solve": lambda i: lib().finrom_fom_solve(eng._h, x.ptr, S, q.ptr, None, i.ptr, None),
        "finrom_fom_gradient": lambda i: lib().finrom_fom_gradient(eng._h, x.ptr, data.ptr, 1, S, g.ptr, J.ptr, q.ptr, i.ptr, None),
        "finrom_fom_solve_rhs": lambda i: lib().finrom_fom_solve_rhs(eng._h, x.ptr, S, rhs.ptr, nrhs, out.ptr, i.ptr, None),
    }
    for name, call in calls.items():
        info = dev(pre)
        check(call(info), name)
        got = info.to_numpy((S,), np.int32)
        print(f"prefilled info, {name}: rows 5, 37 -> {got[5]:#x}, {got[37]:#x}")
        assert got[5] == 0x40 and got[37] == 0x41
        assert np.array_equal(got, want), (name, got.tolist())
