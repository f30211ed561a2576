"""CPU tests of the trainer's edge cases (tests/train_cases.py): that the cases are sound -- the host statement in fp32 stays close
to the fp64 yardstick, so the allowance of the GPU tests stays tight -- and that they discriminate: a kernel that dropped a row,
skipped an input column or read its rows one off would leave the allowance by more than a factor of ten."""
import numpy as np
import pytest

import train_cases as T
from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel


# ---- the table covers what it says it covers -----------------------------------------------------------------------------------------
def test_the_table_covers_the_listed_values():
    col = lambda i: {c[i] for c in T.CASES}
    assert {1, 2, 3, 5, 7, 16, 31, 33} <= col(1)
    assert {2, 15, 17, 31, 32, 33, 63, 65, 97} <= col(2)
    assert {0, 1, 8} <= col(4) and any(0 < l < 8 and l % 2 for l in col(4)) and any(0 < l < 8 and not l % 2 for l in col(4))
    assert {(1, 1), (64, 64), (3, 40), (50, 9)} <= set(T.WIDTHS)
    assert any(c[6] == c[2] for c in T.CASES) and any(c[6] == c[2] + 37 for c in T.CASES)
    assert any(c[7] == "repeat" for c in T.CASES)
    assert all(c[4] <= 1 for c in T.CASES if c[2] == 2)                 # (batch normalisation over two rows: L <= 1, see (a))
    for name in T.CASE_IDS:
        c = T.case(name)
        assert c.rows.min() >= 1 and c.rows.max() + 1 < c.S and len(c.rows) == c.B
        assert (len(set(c.rows.tolist())) < c.B) == (c.rows_kind == "repeat")
        assert not np.array_equal(c.rows, np.sort(c.rows))              # (a non-trivial index array)
        assert np.array_equal(c.X.astype(np.float32).astype(np.float64), c.X)


def test_the_value_cases_hold_the_values_they_name():
    z = T.case("zeros")
    neg = lambda a: int((np.signbit(a) & (a == 0)).sum())
    assert neg(z.model.W0) == 50 and int((z.model.W0 == 0).sum()) == 125
    assert neg(z.model.units[1]["W"]) == 50 and int((z.model.units[1]["W"] == 0).sum()) == 150
    share = (z.Y[z.rows] == 0).mean()
    assert 0.15 < share < 0.25
    o = T.case("offset")
    y0 = o.X[o.rows] @ o.model.W0.astype(np.float64) + o.model.b0
    ratio = np.abs(y0.mean(axis=0)) / y0.std(axis=0)
    print("offset case: column mean / spread of y0, smallest, median, largest:", ratio.min(), np.median(ratio), ratio.max())
    assert 100 < np.median(ratio) < 250 and abs(y0.std(axis=0).mean() - T.OFFSET_SPREAD) < 1e-3


# ---- (a) the host-fp32 deviation is small ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.CASE_IDS)
def test_host_fp32_stays_close_to_the_yardstick(name):
    """Every compared quantity of the host statement in fp32 within 1e-5 of the fp64 yardstick (the allowance of the GPU test is
    then at most 1.6e-4); in the offset case, whose y0 carries its own fp32 rounding at mean / std = 160, within 2e-5.
    Measured (largest quantity per case): min 1.2e-6 (l0_beta), b2_l1 2.1e-6, b15_wide_out 9.1e-6 (W0), b17_full_width 6.1e-7,
    b31_l3 9.3e-7, b32_l0 1.1e-6, b33_l8 1.7e-6, b33_w1 4.5e-6 (l0_W), b63 6.8e-7, b64_narrow 1.7e-6, b65 1.1e-6, b97_repeat 9.0e-7,
    k165 2.2e-6, zeros 9.7e-7; offset 1.3e-5 (W0; l0_var 1.2e-6) at the suggested scales (b0 = 8 + 0.1 randn, W0 scaled to a mean
    column spread of 0.05: mean / std between 125 and 210, median 160) -- no tuning was needed."""
    c = T.case(name)
    nm = max(c.dev32, key=c.dev32.get)
    print(f"{name}: host fp32 against fp64, largest {nm} {c.dev32[nm]:.3g}; l0_var {c.dev32['l0_var']:.3g}")
    for q, v in c.dev32.items():
        assert v <= T.host32_bound(name), (q, v)


def test_two_rows_through_eight_units_are_degenerate():
    """Why the B = 2 cases have L <= 1: (3, 2, 64, 8, 64) leaves the bound by two orders (batch normalisation over two rows maps
    every column to +-1 and amplifies the rounding of a small difference through eight units)."""
    m = T.perturbed(3, 64, 8, 64)
    X, Y = T.probe(3, 2, 64)
    ref = m.train_gradients(X, Y, np.float64)
    d = T.step_deviations(m.train_gradients(X, Y, np.float32), ref)
    print("(3, 2, 64, 8, 64): host fp32 against fp64, largest", max(d.values()))
    assert max(d.values()) > 10 * T.HOST32_BOUND


# ---- (b) the cases discriminate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.CASE_IDS)
def test_planted_faults_leave_the_allowance(name):
    """Each planted fault, computed with the unmodified fp64 statement on altered inputs, moves at least one compared quantity by
    more than 10 x that quantity's allowance."""
    c = T.case(name)
    allow = T.allowance(c.dev32)
    for fault, res in c.planted().items():
        d = T.step_deviations(res, c.ref64)
        over = {q: d[q] / allow[q] for q in d}
        q = max(over, key=over.get)
        print(f"{name}, {fault}: {q} moves by {d[q]:.3g}, {over[q]:.3g} x its allowance {allow[q]:.3g}")
        assert over[q] > 10, (fault, q, over[q])


def test_a_one_pass_fp32_variance_fails_the_offset_case():
    """E[y^2] - mean^2 in float32 on the offset case's y0 misses the fp64 variance by more than 10 x the allowance of l0_var: the
    case tells Chan's update from the cancellation it avoids."""
    c = T.case("offset")
    ref = np.asarray(c.ref64[2]["layers"][0]["var"])
    miss = np.abs(T.one_pass_variance32(c).astype(np.float64) - ref).max() / ref.max()
    allow = T.allowance(c.dev32)["l0_var"]
    print(f"offset: one-pass fp32 variance misses by {miss:.3g}; allowance {allow:.3g}; two-pass host fp32 {c.dev32['l0_var']:.3g}")
    assert miss > 10 * allow


# ---- (c) the helpers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_w,n_out", T.WIDTHS)
def test_flatten_unflatten_round_trip_is_exact(n_w, n_out):
    rng = np.random.default_rng(n_w * 100 + n_out)
    for L in (0, 2):
        m = ResBnFcModel(5, n_out, L, n_w, seed=1)
        flat = rng.standard_normal(ResBnFcModel.flatten(m._tree()).size).astype(np.float32)
        flat[::7] = -0.0
        tree = m.unflatten(flat)
        assert T.bits(ResBnFcModel.flatten(tree)).tolist() == T.bits(flat).tolist()
        assert tree["W0"].shape == (5, n_w) and tree["layers"][-1]["W"].shape == (n_w, n_out) and tree["layers"][-1]["b"].shape == (n_out,)
        assert flat.size == 5 * n_w + n_w + L * (5 * n_w + n_w * n_w) + 4 * n_w + n_w * n_out + n_out


def test_embedding_keeps_the_statement():
    """The (50, 9) model inside width 64: the fp64 statement gives the same common block (the added columns are zero in every
    layer) and zero gradients on everything added -- what the device's padding test relies on."""
    c = T.case("b65")
    big = T.embedded(c.model, 64, c.n_out)
    l, p, g = big.train_gradients(c.X[c.rows], c.Y[c.rows], np.float64)
    assert abs(l - c.ref64[0]) <= 1e-14 * c.ref64[0] and abs(p - c.ref64[1]) <= 1e-14 * c.ref64[1]
    d = T.deviations(T.cut(g, c.model), c.ref64[2])
    assert max(d.values()) <= 1e-13, d
    assert T.outside_is_zero(g, c.model)


def test_the_short_run_is_sound():
    """Section 5's sequence on the host: per step the fp32 statement's loss and batch variances within 1e-5 of the fp64 run's.
    The batch means carry b0 and the units' b, which move on rounding noise by up to lr per step: they are printed."""
    s64, m64, start = T.run_host(np.float64)
    s32, m32, _ = T.run_host(np.float32)
    for i, (a, b) in enumerate(zip(s32, s64)):
        d = T.stat_deviations(a, b)
        print(f"step {i} (B = {T.RUN_B[i]}): host fp32 against fp64, largest {max(d, key=d.get)} {max(d.values()):.3g}")
        assert max(v for q, v in d.items() if not q.endswith("mean")) <= T.HOST32_BOUND
        assert max(d.values()) <= (i + 1) * T.RUN_LR
    d = T.param_deviations(m32, m64, start)
    print("parameters after the run:", {k: f"{v:.2g}" for k, v in d.items()})
    assert m64.opt["t"] == 6
