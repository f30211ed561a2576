"""GPU tests of the trainer's kernels at their edges (csrc/mlp_train.hip through engine.DeviceTrainer and the C ABI): the cases of
tests/train_cases.py, which tests/test_train_edges_host.py shows to be sound and to discriminate.
Yardstick: ResBnFcModel.train_gradients / evaluate / adam_apply in float64.  Allowance: per compared quantity 16 x the deviation of
the same host statement in float32 on the same inputs, floor 4 ulp of fp32 (train_cases.allowance).  Properties of section 3 are
compared bit for bit."""
import copy

import numpy as np
import pytest

import train_cases as T
from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel

pytestmark = pytest.mark.gpu


def cuda_rows(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()


class Handle:
    """A DeviceTrainer on a private copy of the model, with the data resident; closed on exit."""

    def __init__(self, model, X, Y, max_batch):
        from bayesianinferencedl_amd.engine import DeviceTrainer
        self.model = copy.deepcopy(model)
        self.tr = DeviceTrainer(self.model, max_batch=max_batch)
        self.X, self.Y = self.tr.to_device(X, model.n_in), self.tr.to_device(Y, model.n_out)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.tr.close()

    def grad(self, rows):
        """One finrom_mlp_train_grad on the rows -> (loss, MAPE, tree) of get_grads."""
        self.tr.grad(self.X, self.Y, cuda_rows(rows))
        return self.tr.get_grads()

    def state(self):
        """pull -> the bits of every parameter, moving statistic, m, v, and t."""
        self.tr.pull()
        m = self.model
        return T.bits(m.flatten(m._tree()), m.flatten(m.opt["m"]), m.flatten(m.opt["v"])), m.opt["t"]


def step_bits(res):
    return T.bits(np.float64(res[0]), np.float64(res[1]), ResBnFcModel.flatten(res[2]))


def device_step(c, max_batch=None, rows=None, X=None, Y=None):
    with Handle(c.model, c.X if X is None else X, c.Y if Y is None else Y, max_batch or c.max_batch) as h:
        return h.grad(c.rows if rows is None else rows)


# ---- 1. edge cases of one step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.CASE_IDS)
def test_one_step_at_the_edges_matches_the_fp64_statement(name):
    """Every gradient tensor, every layer's batch mean and variance, loss and MAPE of finrom_mlp_train_grad -> get_grads under the
    rule.  The measured factor (device deviation over host-fp32 deviation, worst quantity; 16 allowed) is printed per case.
    Recorded on an MI355X (worst quantity, factor): min mape 1.2; b2_l1 l0_b 3.3; b15_wide_out l1_beta 2.4; b17_full_width l1_W 1.7;
    b31_l3 l0_W 1.6; b32_l0 mape 2.3; b33_l8 l3_W 2.8; b33_w1 loss 4.0 (1.2e-7 against the quarter-ulp floor); b63 l0_mean 2.8;
    b64_narrow l1_W 5.9 (1.6e-6 / 2.7e-7); b65 l5_b 1.7; b97_repeat l3_b 1.5; k165 loss 1.6; zeros l0_var 1.0; offset mape 3.6.
    The largest device deviation of any quantity: 1.1e-5 (W0 of b15_wide_out, host fp32 9.1e-6)."""
    c = T.case(name)
    devd = T.step_deviations(device_step(c), c.ref64)
    allow = T.allowance(c.dev32)
    nm, f = T.worst(devd, c.dev32)
    big = max(devd, key=devd.get)
    print(f"{name} ({c.n_in}, {c.B}, {c.n_w}, {c.L}, {c.n_out}, max_batch {c.max_batch}): worst {nm} factor {f:.2f} "
          f"({devd[nm]:.3g} / {c.dev32[nm]:.3g}); largest device deviation {big} {devd[big]:.3g}; loss {devd['loss']:.3g} "
          f"(fp32 {c.dev32['loss']:.3g}); MAPE {devd['mape']:.3g} (fp32 {c.dev32['mape']:.3g})")
    for q in devd:
        assert devd[q] <= allow[q], (q, devd[q], c.dev32[q])


def test_the_offset_case_holds_the_first_variance_where_one_pass_would_not():
    """The device's variance of y0 at mean / std = 160 against the fp64 statement's, beside what E[y^2] - mean^2 in fp32 gives.
    Recorded on an MI355X: device 1.3e-6, host fp32 (two passes) 1.2e-6, one pass in fp32 1.2e-2."""
    c = T.case("offset")
    ref = np.asarray(c.ref64[2]["layers"][0]["var"])
    dev = np.asarray(device_step(c)[2]["layers"][0]["var"], dtype=np.float64)
    d = np.abs(dev - ref).max() / ref.max()
    miss = np.abs(T.one_pass_variance32(c).astype(np.float64) - ref).max() / ref.max()
    print(f"offset: l0_var device {d:.3g}, host fp32 {c.dev32['l0_var']:.3g}, one-pass fp32 {miss:.3g}")
    assert d <= T.allowance(c.dev32)["l0_var"] < miss / 10


# ---- 3. bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B2", [33, 2])
def test_stale_tiles_of_a_larger_batch_are_never_read(B2):
    """grad at B = 97, then grad at B2 on other rows, on one handle of max_batch 97, against a fresh handle at B2."""
    c = T.case("b97_repeat")
    model = T.perturbed(c.n_in, c.n_w, 1, c.n_out)                       # (L = 1: B = 2 stays well-conditioned)
    other = np.random.default_rng(9).permutation(c.S)[:B2]
    assert other.max() < c.S
    with Handle(model, c.X, c.Y, 97) as h:
        h.grad(c.rows)
        used = h.grad(other)
    with Handle(model, c.X, c.Y, 97) as h:
        fresh = h.grad(other)
    assert np.array_equal(step_bits(used), step_bits(fresh))
    assert np.isfinite(fresh[0]) and fresh[0] > 0


@pytest.mark.parametrize("name", ["b65", "b15_wide_out", "b33_l8"])
def test_strides_by_max_batch_change_no_bit(name):
    c = T.case(name)
    assert np.array_equal(step_bits(device_step(c, max_batch=c.B)), step_bits(device_step(c, max_batch=c.B + T.EXTRA)))


@pytest.mark.parametrize("name", ["b97_repeat", "b63"])
def test_rows_through_the_index_array_against_gathered_rows(name):
    """Rows r into X against identity rows into the pre-gathered X[r], Y[r]."""
    c = T.case(name)
    direct = device_step(c)
    gathered = device_step(c, rows=np.arange(c.B), X=c.X[c.rows], Y=c.Y[c.rows])
    assert np.array_equal(step_bits(direct), step_bits(gathered))


def test_padding_width_50_inside_width_64():
    """(n_w, n_out) = (50, 9) against the same model embedded in n_w = 64 (added weights, gammas, betas, biases zero), n_out
    unchanged: loss, MAPE and the common block bit for bit, everything added exactly zero.  The device layouts coincide; what
    differs is pack / unpack at another width."""
    c = T.case("b65")
    small = device_step(c)
    with Handle(T.embedded(c.model, 64, c.n_out), c.X, c.Y, c.max_batch) as h:
        big = h.grad(c.rows)
    assert np.array_equal(step_bits(small), step_bits((big[0], big[1], T.cut(big[2], c.model))))
    assert T.outside_is_zero(big[2], c.model)


def test_padding_outputs_16_inside_64_scales_by_four():
    """(50, 16) against the same model embedded in (64, 64) with the added targets zero: d loss / d out is 2 diff / (B n_out), so
    every data gradient of the common block is the small model's divided by exactly 4 (a power of two commutes with every
    rounding; no value is near the subnormals).  Bit for bit: batch means and variances as they are, the gradients of gamma,
    beta, b, b0 and the head's W times 4.  W0's and the units' W's gradients add the regulariser's term r after the scaling, so
    there (a - r) against 4 (b - r): each side is an fp32 result (half an ulp) of a sum whose term r was itself rounded (half an
    ulp of r, on the wide side times 4) -- within 4 ulp of fp32 at the larger of max |a| and 4 max |b|."""
    model = T.perturbed(33, 50, 2, 16)
    X, Y = T.probe(33, 80, 16, seed=5)
    rows = 3 + np.random.default_rng(6).permutation(70)[:65]
    Ybig = np.zeros((80, 64)); Ybig[:, :16] = Y
    with Handle(model, X, Y, 65) as h:
        small = h.grad(rows)
    with Handle(T.embedded(model, 64, 64), X, Ybig, 65) as h:
        big = h.grad(rows)
    assert T.outside_is_zero(big[2], model)
    for (nm, a, _), (_, b, _) in zip(T.leaves(small[2]), T.leaves(T.cut(big[2], model))):
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        if nm.endswith(("mean", "var")):
            assert np.array_equal(T.bits(a32), T.bits(b32)), nm
        elif nm == "W0" or (nm.endswith("_W") and nm != "l2_W"):
            w = np.asarray(model.W0 if nm == "W0" else model.units[int(nm[1])]["W"], dtype=np.float64)
            r = 1e-4 * np.sign(w) + 2e-4 * w
            assert np.abs((a - r) - 4 * (b - r)).max() <= 4 * T.ULP32 * max(np.abs(a).max(), 4 * np.abs(b).max()), nm
        else:
            assert np.array_equal(T.bits(a32), T.bits(np.float32(4) * b32)), nm


def test_lr_zero_moves_no_parameter_but_the_optimiser_state():
    """grad; apply at lr = 0: every parameter's bits unchanged; m, v, the moving statistics and t move (fit's graph warm-up)."""
    c = T.case("b65")
    with Handle(c.model, c.X, c.Y, c.max_batch) as h:
        before = copy.deepcopy(h.model)
        h.tr.set_lr(0.0)
        h.grad(c.rows)
        h.tr.apply()
        h.tr.pull()
        after = h.model
    moving = lambda nm: nm.endswith(("mean", "var"))
    for (nm, a, _), (_, b, _) in zip(T.leaves(after._tree()), T.leaves(before._tree())):
        same = np.array_equal(T.bits(a.astype(np.float32)), T.bits(b.astype(np.float32)))
        assert same != moving(nm), nm
    assert after.opt["t"] == 1
    for k in ("m", "v"):
        for nm, a, _ in T.leaves(after.opt[k]):
            assert np.any(a != 0) != moving(nm), (k, nm)


def test_evaluation_touches_no_training_state():
    """grad; evaluate; apply gives the bits of grad; apply."""
    c = T.case("b65")
    out = []
    for with_eval in (False, True):
        with Handle(c.model, c.X, c.Y, c.max_batch) as h:
            h.tr.set_lr(1e-3)
            h.grad(c.rows)
            if with_eval:
                h.tr.evaluate(h.X, h.Y)                                   # (S = 138 rows: three chunks over the tape)
            h.tr.apply()
            out.append((h.state(), h.tr.epoch_stats()))
    (sa, ta), ea = out[0]
    (sb, tb), eb = out[1]
    assert np.array_equal(sa, sb) and ta == tb == 1 and ea == eb and ea[2] == 65


def test_epoch_stats_are_the_row_weighted_means():
    """Two steps at B = 65 and B = 2: loss and MAPE are (65 a + 2 b) / 67 in double, formed as the device forms them, bit for bit;
    the MSE against single-step handles' to 1e-14 (x 65 / 65 is not an identity in the last bit); rows 67; zeros after the reset."""
    c = T.case("b65")
    model = T.perturbed(c.n_in, c.n_w, 1, c.n_out)
    r2 = np.array([12, 4])
    with Handle(model, c.X, c.Y, 65) as h:
        h.tr.set_lr(1e-3)
        a = h.grad(c.rows); h.tr.apply()
        b = h.grad(r2); h.tr.apply()
        loss, mape, rows = h.tr.epoch_stats()
        mse = h.tr.last_mse
        again = h.tr.epoch_stats()
    assert rows == 67 and again == (0.0, 0.0, 0)
    assert loss == (a[0] * 65.0 + b[0] * 2.0) / 67.0 and mape == (a[1] * 65.0 + b[1] * 2.0) / 67.0
    singles = []
    with Handle(model, c.X, c.Y, 65) as h:
        h.tr.set_lr(1e-3)
        for r in (c.rows, r2):
            h.grad(r); h.tr.apply()
            h.tr.epoch_stats()
            singles.append(h.tr.last_mse)
    assert 0 < singles[0] < a[0] and 0 < singles[1] < b[0]
    assert mse == pytest.approx((singles[0] * 65 + singles[1] * 2) / 67, rel=1e-14)


@pytest.mark.parametrize("n_w,n_out", T.WIDTHS)
def test_parameters_round_trip_exactly(n_w, n_out):
    """set_params / get_params at every (n_w, n_out) of the table: bits kept (-0.0 included); m = v = None gives zeros; t carried."""
    from bayesianinferencedl_amd.engine import DeviceTrainer
    from bayesianinferencedl_amd.deep_learning.dl_model import tree_map
    rng = np.random.default_rng(n_w * 100 + n_out)
    m = T.perturbed(5, n_w, 2, n_out)
    for u in m.units + [m.head]:
        u["mean"] = rng.normal(0, 0.3, n_w).astype(np.float32)
        u["var"] = rng.uniform(0.5, 1.5, n_w).astype(np.float32)
    m.W0[0, 0] = -0.0
    m.opt["t"] = 5
    want = T.tree_bits(m._tree())
    tr = DeviceTrainer(m, max_batch=2)
    try:
        tr.pull()
        assert np.array_equal(T.tree_bits(m._tree()), want) and m.opt["t"] == 5
        assert not np.any(ResBnFcModel.flatten(m.opt["m"])) and not np.any(ResBnFcModel.flatten(m.opt["v"]))
        def state(a):
            return rng.standard_normal(a.shape).astype(np.float32)
        m.opt["m"], m.opt["v"] = tree_map(state, m._tree()), tree_map(lambda a: np.abs(state(a)), m._tree())
        for tree in (m.opt["m"], m.opt["v"]):                             # (unused slots of the layout: they come back as zeros)
            for u in tree["layers"]:
                u["mean"][...] = 0; u["var"][...] = 0
        m.opt["t"] = 123456789012
        wm, wv = T.tree_bits(m.opt["m"]), T.tree_bits(m.opt["v"])
        tr.push()
        m.opt["m"] = m.opt["v"] = None; m.opt["t"] = 0
        tr.pull()
        assert np.array_equal(T.tree_bits(m._tree()), want) and m.opt["t"] == 123456789012
        assert np.array_equal(T.tree_bits(m.opt["m"]), wm) and np.array_equal(T.tree_bits(m.opt["v"]), wv)
    finally:
        tr.close()


# ---- 4. evaluation in inference form -----------------------------------------------------------------------------------------------
def test_evaluation_in_chunks_matches_the_fp64_statement():
    """S = 150 on handles of max_batch 150 (one chunk), 64 (64 + 64 + 22), 149 (a tail chunk of one row), 37 (four chunks + 2), and
    S = 1: loss and MAPE against evaluate in float64 under the rule, evaluate in float32 as the fp32 side; the chunkings among
    themselves to 1e-12 (the sums are in double and only their grouping differs).  Recorded on an MI355X: S = 150 loss 6.2e-8
    (fp32 5.6e-8), MAPE 5.6e-8 (fp32 2.1e-7), the same digits at every chunking; S = 1 loss 4.9e-8 (6.7e-9), MAPE 2.4e-8 (1.0e-7)."""
    m, X, Y = T.eval_model()
    got = {}
    for S in (T.EVAL_S, 1):
        l64, p64 = (float(v) for v in m.evaluate(X[:S], Y[:S], np.float64))
        l32, p32 = (float(v) for v in m.evaluate(X[:S], Y[:S], np.float32))
        for mb, what in (T.EVAL_MAX_BATCH if S > 1 else [(2, "one row")]):
            with Handle(m, X[:S], Y[:S], mb) as h:
                ld, pd = h.tr.evaluate(h.X, h.Y)
            got[(S, mb)] = (ld, pd)
            print(f"S = {S}, max_batch {mb} ({what}): loss {abs(ld - l64) / l64:.3g} (fp32 {abs(l32 - l64) / l64:.3g}), "
                  f"MAPE {abs(pd - p64) / p64:.3g} (fp32 {abs(p32 - p64) / p64:.3g})")
            assert abs(ld - l64) <= max(T.FACTOR * abs(l32 - l64), 4 * T.ULP32 * l64)
            assert abs(pd - p64) <= max(T.FACTOR * abs(p32 - p64), 4 * T.ULP32 * p64)
    l0, p0 = got[(T.EVAL_S, 150)]
    for mb, _ in T.EVAL_MAX_BATCH[1:]:
        l, p = got[(T.EVAL_S, mb)]
        assert abs(l - l0) <= 1e-12 * l0 and abs(p - p0) <= 1e-12 * p0, mb


# ---- 5. a short run with changing batch sizes on one handle ------------------------------------------------------------------------
def test_a_run_of_changing_batch_sizes_follows_the_fp64_run():
    """Six steps of grad; apply with B = 65, 2, 33, 64, 31, 65 on one handle (max_batch 65, lr 1e-3, L = 1).  Per step: loss and
    every layer's batch mean and variance under the rule against the same sequence of train_gradients / adam_apply in float64,
    the float32 host sequence as the fp32 side.  Afterwards: every parameter and moving statistic under the rule, except b0 and
    the unit's b.  Those move on rounding noise: a parameter moves by at most about lr per step under Adam, so either
    run's bias stays within the run's largest parameter change and the two runs within twice that; that is their bound.
    Recorded on an MI355X: per-step factors 1.4, 0.9, 1.2, 1.1, 1.0, 1.1 (loss up to 4.8e-6 at the B = 2 step, host fp32 5.5e-6);
    parameters: worst l0_beta 2.8e-6 against 7.3e-7 (3.8), W0 9.6e-6 against 2.1e-5; b0 0.23 and l0_b 0.16 of the largest change."""
    s64, m64, start = T.run_host(np.float64)
    s32, m32, _ = T.run_host(np.float32)
    m, X, Y, rows = T.run_setup()
    with Handle(m, X, Y, T.RUN_MAX_BATCH) as h:
        h.tr.set_lr(T.RUN_LR)
        for i, r in enumerate(rows):
            res = h.grad(r)
            h.tr.apply()
            devd, dev32 = T.stat_deviations(res, s64[i]), T.stat_deviations(s32[i], s64[i])
            nm, f = T.worst(devd, dev32)
            print(f"step {i} (B = {len(r)}): worst {nm} factor {f:.2f} ({devd[nm]:.3g} / {dev32[nm]:.3g}); loss {devd['loss']:.3g}")
            allow = T.allowance(dev32)
            for q in devd:
                assert devd[q] <= allow[q], (i, q, devd[q], dev32[q])
        h.tr.pull()
        dev = h.model
    assert dev.opt["t"] == 6
    devd, dev32 = T.param_deviations(dev, m64, start), T.param_deviations(m32, m64, start)
    print("parameters after the run, device / host fp32:", {k: f"{devd[k]:.2g} / {dev32[k]:.2g}" for k in devd})
    for q in devd:
        if T.NOISE_BIASES(q, dev.n_layers):
            assert devd[q] <= 2.0, (q, devd[q])
        else:
            assert devd[q] <= max(T.FACTOR * dev32[q], 4 * T.ULP32), (q, devd[q], dev32[q])
