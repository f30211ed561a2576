"""The fused chains under the pure deep-learning surrogate on the device (finrom_hmc_leapfrog_ml / finrom_hmc_trajectory_ml,
csrc/hmc_ml.hip; hmc.py model="ml" with ml_form="steps" | "trajectory").

Kernels, through the C ABI (shapes and statements: tests/hmc_ml_cases.py): the whole trajectory in one launch leaves the bits of
the composed steps; a step is the exact position update, the bits of finrom_mlp_misfit_grad at the new point and the exact kick on
them; a chain with a NaN in its position is flagged after every step, gets no force, keeps its momentum's bits and disturbs no other
chain; everything the entry points refuse is refused before a launch.  Chains: both forms against the host recursion over the same
device calls (tests/test_gpu_surrogate.py's closeness), against each other bit for bit, under the Gaussian-field prior against the
host chain on the whitened surrogate, with stats= and with delayed acceptance."""
import ctypes
import functools

import numpy as np
import pytest

import hmc_cases as H
import hmc_ml_cases as MC
import mlp_cases as K
import surrogate_cases as SC

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -1, -4
MOVED = ("P", "dUq", "loss", "info")


def _id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _rig(shape):
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    model = MC.kernel_model(shape)
    return model, DeviceErrorModel(model)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from bayesianinferencedl_amd import _ffi
    return _ffi.lib()


def _data(shape, C, per_sample):
    import torch
    return torch.from_numpy(MC.kernel_data(shape, C, per_sample)).cuda()


def _step(mlp, dev, step, data_t, per_sample, grad_t=None, out_t=None):
    return _lib().finrom_hmc_leapfrog_ml(mlp._h, ctypes.byref(dev.st), step, data_t.data_ptr(), int(per_sample),
                                         grad_t.data_ptr() if grad_t is not None else None,
                                         out_t.data_ptr() if out_t is not None else None, _stream())


def _trajectory(mlp, dev, n_steps, data_t, per_sample):
    return _lib().finrom_hmc_trajectory_ml(mlp._h, ctypes.byref(dev.st), n_steps, data_t.data_ptr(), int(per_sample), _stream())


def _run(case, mlp, n_steps, data_t, per_sample, form):
    """The download after n_steps steps from `case` in the given form, and the DeviceState."""
    dev = H.DeviceState(case)
    if form == "trajectory":
        assert _trajectory(mlp, dev, n_steps, data_t, per_sample) == 0
    else:
        for s in range(n_steps):
            assert _step(mlp, dev, s, data_t, per_sample) == 0
    return dev.download(), dev


def _assert_same_end(got_t, got_s, dev, n_steps, tag):
    """Kq[n_steps & 1], P, dUq, loss, info: equal bytes, padding included; everything else but the other position buffer: as uploaded."""
    end, other = "Kq%d" % (n_steps & 1), "Kq%d" % ((n_steps + 1) & 1)
    for name in (end,) + MOVED:
        assert H.same_bits(got_t[name], got_s[name]), (tag, name)
    for got in (got_t, got_s):
        dev.assert_bits(got, {}, skip=(end, other) + MOVED)
        for name in (end, other) + MOVED:
            assert H.same_bits(got[name][-H.PAD:], dev.up[name][-H.PAD:]), (tag, name, "written behind its end")


# ---- 1. the trajectory is the composed steps, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C", MC.CHAINS)
@pytest.mark.parametrize("shape", MC.SHAPES, ids=_id)
def test_the_trajectory_leaves_the_bits_of_the_composed_steps(shape, C):
    model, mlp = _rig(shape)
    for per_sample in (False, True):
        data_t = _data(shape, C, per_sample)
        for n_steps in MC.STEPS:
            case = MC.state_case(shape, C)
            got_s, dev = _run(case, mlp, n_steps, data_t, per_sample, "steps")
            got_t, _ = _run(case, mlp, n_steps, data_t, per_sample, "trajectory")
            tag = (shape, C, n_steps, per_sample)
            _assert_same_end(got_t, got_s, dev, n_steps, tag)
            assert np.isfinite(dev.body(got_s, "loss")).all() and not dev.body(got_s, "info").any(), tag
            assert np.isfinite(dev.body(got_s, "Kq%d" % (n_steps & 1))).all() and np.isfinite(dev.body(got_s, "P")).all(), tag
            assert np.any(dev.body(got_s, "P") != case["P"]), tag                  # (the trajectory did move)


# ---- 2. a step is what is already tested, bit for bit ---------------------------------------------------------------------------------------
STEP_CASES = [(s, C) for s in MC.SHAPES for C in (1, 4)] + [(MC.SHAPES[0], 80), (MC.SHAPES[1], 80)]


@pytest.mark.parametrize("shape,C", STEP_CASES, ids=_id)
def test_a_step_is_the_exact_drift_the_misfit_calls_bits_and_the_exact_kick(shape, C):
    """k' = fma(eps, P, k); loss and grad_out are finrom_mlp_misfit_grad's bits at k' (per-sample form); info = 0; dUq and P are the
    NumPy kick on those bits.  Both parities of step, eps = 0 included, data shared and per chain, out given and left out."""
    import torch
    model, mlp = _rig(shape)
    n = shape[0]
    for step, eps, per_sample in ((0, None, False), (1, None, True), (0, 0.0, True)):
        case = MC.state_case(shape, C, eps=eps, seed=step)
        if step & 1:
            case["Kq1"], case["Kq0"] = case["Kq0"], case["Kq1"]
        k = case["Kq%d" % (step & 1)]
        data_t = _data(shape, C, per_sample)
        dev = H.DeviceState(case)
        grad_t = torch.full((C, n), float("nan"), dtype=torch.float64, device="cuda")
        out_t = torch.full((C, shape[3]), float("nan"), dtype=torch.float64, device="cuda") if step == 0 else None
        assert _step(mlp, dev, step, data_t, per_sample, grad_t, out_t) == 0
        got = dev.download()
        kq = MC.ref_drift(case, k)
        if eps == 0.0:
            assert H.same_bits(kq, k)
        ref = mlp.misfit_grad(torch.from_numpy(kq).cuda(), data_t)
        assert mlp.last_form() == 1
        loss, grad = ref["loss"].cpu().numpy(), ref["grad"].cpu().numpy()
        assert np.isfinite(loss).all() and np.isfinite(grad).all() and np.abs(grad).max() > 0
        dU, Pn = MC.ref_kick(case, kq, case["P"], np.zeros(C, np.int32), grad)
        tag = (shape, C, step, eps, per_sample)
        dev.assert_bits(got, {"Kq%d" % ((step + 1) & 1): kq, "loss": loss, "info": np.zeros(C, np.int32), "dUq": dU, "P": Pn})
        assert H.same_bits(grad_t.cpu().numpy(), grad), tag
        if out_t is not None:
            assert H.same_bits(out_t.cpu().numpy(), ref["out"].cpu().numpy()), tag
        # the same step without grad_out: the handle's own buffer, the same bits
        dev2 = H.DeviceState(case)
        assert _step(mlp, dev2, step, data_t, per_sample) == 0
        got2 = dev2.download()
        assert [name for name in got if not H.same_bits(got[name], got2[name])] == [], tag


# ---- 3. a flagged chain -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [MC.SHAPES[1], MC.SHAPES[3]], ids=_id)
def test_a_chain_with_a_nan_is_flagged_gets_no_force_and_disturbs_nobody(shape):
    model, mlp = _rig(shape)
    C, bad, n_steps = 4, 2, 3
    data_t = _data(shape, C, True)
    clean = MC.state_case(shape, C)
    case = MC.state_case(shape, C)
    case["Kq0"][bad, shape[0] // 3] = np.nan                         # a value, not a fault
    dev = H.DeviceState(case)
    for s in range(n_steps):                                         # after every step
        assert _step(mlp, dev, s, data_t, True) == 0
        got = dev.download()
        assert list(dev.body(got, "info")) == [0, 0, 1, 0], s
        assert not np.isfinite(dev.body(got, "loss")[bad]) and np.isfinite(np.delete(dev.body(got, "loss"), bad)).all()
        assert not dev.body(got, "dUq")[bad].any() and not np.signbit(dev.body(got, "dUq")[bad]).any(), s
        assert H.same_bits(dev.body(got, "P")[bad], case["P"][bad]), s
    got_s = got
    got_t, _ = _run(case, mlp, n_steps, data_t, True, "trajectory")
    _assert_same_end(got_t, got_s, dev, n_steps, (shape, "flagged"))
    good = [c for c in range(C) if c != bad]
    for form, flagged in (("steps", got_s), ("trajectory", got_t)):
        ref, rdev = _run(clean, mlp, n_steps, data_t, True, form)
        for name in ("Kq%d" % (n_steps & 1),) + MOVED:
            assert H.same_bits(dev.body(flagged, name)[good], rdev.body(ref, name)[good]), (form, name)


# ---- 4. checks before any device call -------------------------------------------------------------------------------------------------------
def test_the_entry_points_refuse_before_any_launch():
    import torch
    L = _lib()
    err = L.finrom_last_error
    shape = MC.SHAPES[0]
    model, mlp = _rig(shape)
    data_t = _data(shape, 3, False)
    dev = H.DeviceState(MC.state_case(shape, 3))
    st, d, s = ctypes.byref(dev.st), data_t.data_ptr(), _stream()
    assert L.finrom_hmc_leapfrog_ml(None, st, 0, d, 0, None, None, s) == ERR_ARG and b"hmc_leapfrog_ml: null mlp handle or data" in err()
    assert L.finrom_hmc_leapfrog_ml(mlp._h, st, 0, None, 0, None, None, s) == ERR_ARG and b"null mlp handle or data" in err()
    assert L.finrom_hmc_leapfrog_ml(mlp._h, None, 0, d, 0, None, None, s) == ERR_ARG and b"hmc_leapfrog_ml: null field" in err()
    assert L.finrom_hmc_leapfrog_ml(mlp._h, st, -1, d, 0, None, None, s) == ERR_ARG and b"hmc_leapfrog_ml: step < 0" in err()
    assert L.finrom_hmc_trajectory_ml(None, st, 3, d, 0, s) == ERR_ARG and b"hmc_trajectory_ml: null mlp handle or data" in err()
    assert L.finrom_hmc_trajectory_ml(mlp._h, st, 3, None, 0, s) == ERR_ARG and b"null mlp handle or data" in err()
    assert L.finrom_hmc_trajectory_ml(mlp._h, None, 3, d, 0, s) == ERR_ARG and b"hmc_trajectory_ml: null field" in err()
    assert L.finrom_hmc_trajectory_ml(mlp._h, st, -1, d, 0, s) == ERR_ARG and b"hmc_trajectory_ml: n_steps < 0" in err()
    # a state of another size than the network's input
    other = H.DeviceState(MC.state_case((shape[0] - 1,) + shape[1:], 3))
    assert _step(mlp, other, 0, data_t, False) == ERR_ARG and b"n = 36 is not the network's input size (37)" in err()
    assert _trajectory(mlp, other, 3, data_t, False) == ERR_ARG and b"n = 36 is not the network's input size (37)" in err()
    other.assert_bits(other.download(), {})
    # c_pri = 0
    zero = MC.state_case(shape, 3)
    zero["c_pri"] = 0.0
    zdev = H.DeviceState(zero)
    assert _step(mlp, zdev, 0, data_t, False) == ERR_ARG and b"hmc_leapfrog_ml: c_pri = 0" in err()
    assert _trajectory(mlp, zdev, 3, data_t, False) == ERR_ARG and b"hmc_trajectory_ml: c_pri = 0" in err()
    # no chains: 0, nothing touched
    none = H.DeviceState(MC.state_case(shape, 0))
    assert _step(mlp, none, 0, data_t, False) == 0 and _trajectory(mlp, none, 3, data_t, False) == 0
    none.assert_bits(none.download(), {})
    # no steps: 0, nothing touched
    assert _trajectory(mlp, dev, 0, data_t, False) == 0
    dev.assert_bits(dev.download(), {})
    for t in (other, zdev):
        t.assert_bits(t.download(), {})


def test_an_input_wider_than_the_forward_kernels_lds_is_refused():
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    L = _lib()
    shape = (K.FORWARD_MAX_IN + 3, 17, 1, 9)
    assert L.finrom_mlp_forward_max_in() == K.FORWARD_MAX_IN
    mlp = DeviceErrorModel(K.make_model(*shape, seed=3))
    data_t = _data(shape, 1, False)
    dev = H.DeviceState(MC.state_case(shape, 1))
    assert _step(mlp, dev, 0, data_t, False) == ERR_UNSUPPORTED and b"exceeds %d" % K.FORWARD_MAX_IN in L.finrom_last_error()
    assert _trajectory(mlp, dev, 2, data_t, False) == ERR_UNSUPPORTED and b"exceeds %d" % K.FORWARD_MAX_IN in L.finrom_last_error()
    dev.assert_bits(dev.download(), {})


def test_a_data_width_other_than_n_out_is_refused(chains):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    c = chains
    for form in hmc.ML_FORMS:
        with pytest.raises(ValueError, match=r"data must be \[9\]"):
            hmc.run_chains_fused(None, SC.hmc_starts(), MC.HMC_EVALS, model="ml", surrogate=c["sur"], data=np.ones(10), ml_form=form,
                                 **MC.chain_kw(False))


@pytest.mark.parametrize("form", ["steps", "trajectory"])
def test_the_first_call_with_a_new_c_inside_a_capture_is_refused_with_a_message(form):
    import torch
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    L = _lib()
    shape = MC.SHAPES[0]
    mlp = DeviceErrorModel(MC.kernel_model(shape))                   # a fresh handle: no workspace yet
    data_t = _data(shape, 5, False)
    dev = H.DeviceState(MC.state_case(shape, 5))
    x = torch.ones(8, device="cuda")
    call = (lambda: _step(mlp, dev, 0, data_t, False)) if form == "steps" else (lambda: _trajectory(mlp, dev, 2, data_t, False))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        twice = x * 2.0                                              # (the capture is not empty)
        rc = call()
        msg = L.finrom_last_error()
    torch.cuda.synchronize()
    assert rc == ERR_UNSUPPORTED and b"capture" in msg, (rc, msg)
    dev.assert_bits(dev.download(), {})
    assert call() == 0                                               # outside the capture the same call goes through
    assert np.isfinite(dev.body(dev.download(), "loss")).all()


# ---- chains ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chains(spaces):
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    model = SC.hmc_model()
    prior = MC.prior4(spaces(4))
    sur = Surrogate(model)
    return dict(model=model, sur=sur, data=SC.hmc_data(model), prior=prior, wsur=sur.whitened(prior), hosts={})


@pytest.fixture(scope="module")
def fin4(spaces):
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    return Fin(spaces(4))


def _close(dev, host):
    """tests/test_gpu_surrogate.py::_close."""
    assert dev.proposals == host.proposals and np.array_equal(dev.accept, host.accept), (dev.accept, host.accept)
    if host.trace is not None:
        assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    assert np.linalg.norm(dev.K - host.K) <= 1e-9 * np.linalg.norm(host.K)
    if host.get("V") is not None:
        assert np.linalg.norm(dev.V - host.V) <= 1e-9 * np.linalg.norm(host.V)


def _host(c, field, rng, **more):
    """The host recursion over the same device calls, once per (prior, rng): under the prior on the WHITENED surrogate with mean 0
    and tau 1, its states v mapped through prior.field."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    key = (field, rng) + tuple(sorted(more))
    if key not in c["hosts"]:
        kw = MC.chain_kw(field, rng=rng, keep_trace=True, record=MC.RECORD, **more)
        if field:
            kw.update(mean=0.0, tau=1.0)
        res = hmc.run_chains(hmc.ml_value_and_grad(c["wsur" if field else "sur"], c["data"]), SC.hmc_starts(field=field), MC.HMC_EVALS, **kw)
        assert 0 < res.accept.sum() < 4 * MC.HMC_PROPOSALS, res.accept
        if field:
            res = hmc.HmcResult(res, V=res.K, K=c["prior"].field(res.K), trace=c["prior"].field(res.trace))
        c["hosts"][key] = res
    return c["hosts"][key]


def _device(c, field, form, **more):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    kw = MC.chain_kw(field, **more)
    res = hmc.run_chains_device(None, SC.hmc_starts(field=field), MC.HMC_EVALS, model="ml", surrogate=c["sur"], data=c["data"], ml_form=form,
                                prior=c["prior"] if field else None, **kw)
    assert res.fused is True and res.ml_form == form and res.model == "ml"
    return res


# ---- 5., 6. both forms against the host recursion, both priors ---------------------------------------------------------------------------
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "stream"])
@pytest.mark.parametrize("form", ["steps", "trajectory"])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_both_forms_follow_the_host_recursion_over_the_same_device_calls(chains, field, form, graph, rng):
    c = chains
    host = _host(c, field, rng)
    dev = _device(c, field, form, graph=graph, rng=rng, keep_trace=True, record=MC.RECORD)
    assert dev.graph == graph
    _close(dev, host)
    assert [e for e, *_ in dev.recorded] == [e for e, *_ in host.recorded] == sorted(MC.RECORD)
    model = c["wsur"].model if field else c["model"]                 # under the prior the records are (v, loss, gradient in v)
    for (ev, Xr, loss, grad), (_, Xh, _, _) in zip(dev.recorded, host.recorded):
        assert np.max(np.abs(Xr - Xh)) <= 1e-9 * np.max(np.abs(Xh))
        ref, h32 = SC.misfit_refs(model, Xr, c["data"])
        print(f"RATIO form=hmc-ml/{form}/{'field' if field else 'iid'}/ev{ev} loss {K.ratio(loss, h32['loss'], ref['loss']):.3f} "
              f"grad {K.ratio(grad, h32['grad'], ref['grad']):.3f}")
        assert np.max(np.abs(loss - ref["loss"])) <= K.bound(h32["loss"], ref["loss"])
        assert np.max(np.abs(grad - ref["grad"])) <= K.bound(h32["grad"], ref["grad"])


@pytest.mark.parametrize("record", [None, MC.RECORD], ids=["plain", "recorded"])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_the_trajectory_form_is_the_step_form_bit_for_bit(chains, field, record):
    a = _device(chains, field, "steps", keep_trace=True, record=record, rng="philox")
    b = _device(chains, field, "trajectory", keep_trace=True, record=record, rng="philox")
    assert np.array_equal(a.K, b.K) and np.array_equal(a.trace, b.trace) and np.array_equal(a.accept, b.accept)
    assert 0 < a.accept.sum() < 4 * MC.HMC_PROPOSALS
    if field:
        assert np.array_equal(a.V, b.V)
    for (ea, *ra), (eb, *rb) in zip(a.recorded, b.recorded):
        assert ea == eb and all(np.array_equal(x, y) for x, y in zip(ra, rb))
    # and neither depends on the block of proposals drawn ahead
    d = _device(chains, field, "trajectory", keep_trace=True, record=record, rng="philox", block=3)
    assert np.array_equal(d.K, b.K) and np.array_equal(d.trace, b.trace)


# ---- 7. stats= -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["steps", "trajectory"])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_device_stats_are_the_recursion_over_the_kept_trace(chains, field, form):
    """ChainStats(burn=1, batch=1): to the standard of tests/test_gpu_hmc_stats.py -- under the i.i.d. prior bit for bit; under the
    Gaussian-field prior the stats see the end point's field from one launch per proposal and the trace is mapped after the run in one
    launch over all rows: mean 1e-12 absolute, m2 1e-12 t."""
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats, stats_from_trace
    plain = _device(chains, field, form, keep_trace=True, rng="philox")
    res = _device(chains, field, form, keep_trace=True, rng="philox", stats=ChainStats(burn=1, batch=1))
    assert np.array_equal(res.K, plain.K) and np.array_equal(res.accept, plain.accept) and np.array_equal(res.trace, plain.trace)
    s, ref = res.stats, stats_from_trace(res.trace, 1, 1)
    assert (s.t, s.n_batches, s.first, s.next) == (ref.t, ref.n_batches, ref.first, ref.next) == (3, 3, 0, 4)
    assert np.array_equal(s.accepted, ref.accepted) and np.array_equal(s.accepted.sum(0), res.accept)
    if field:
        assert np.max(np.abs(s.mean - ref.mean)) <= 1e-12 and np.max(np.abs(s.m2 - ref.m2)) <= 1e-12 * s.t
        assert np.max(np.abs(s.bm_mean - ref.bm_mean)) <= 1e-12 and np.max(np.abs(s.bm_m2 - ref.bm_m2)) <= 1e-12 * s.n_batches
        assert np.max(np.abs(s.cur - ref.cur)) <= 1e-12 and np.max(np.abs(s.mean - 1.0)) < 1.0       # fields, not whitened states
    else:
        for name in ChainStats.SUMS + ("cur",):
            assert np.array_equal(getattr(s, name), getattr(ref, name)), name
    assert np.isfinite(s.misfit).all()
    stay = s.accepted[1:] == 0
    assert np.array_equal(s.misfit[1:][stay], s.misfit[:-1][stay]) and np.all(s.misfit[1:][~stay] != s.misfit[:-1][~stay])


# ---- 8. correct= ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["steps", "trajectory"])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_delayed_acceptance_with_the_fom_deciding(chains, fin4, field, form):
    """The wide-sigma setup of tests/test_gpu_surrogate.py (the network is no model of the fin); under the prior against the
    whitened host statement, whose correcting model sees the field of the whitened state."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    c = chains
    prior = c["prior"]
    data = np.asarray(fin4.qoi_operator(fin4.forward(np.exp(0.25 * np.random.default_rng(11).standard_normal(SC.N4)))[0]))
    kw = dict(seeds=MC.HMC_SEEDS, eps=MC.DA_EPS["field" if field else "iid"], n_leapfrog=MC.HMC_LEAPFROG, sigma=MC.DA_SIGMA, tau=MC.HMC_TAU,
              rng="philox", keep_trace=True)
    x0 = SC.hmc_starts(field=field)
    fv = hmc.fom_value(fin4, data)
    if field:
        host = hmc.run_chains(hmc.ml_value_and_grad(c["wsur"], data), x0, MC.HMC_EVALS, correct=lambda V: fv(prior.field(V)),
                              **dict(kw, mean=0.0, tau=1.0))
        host = hmc.HmcResult(host, V=host.K, K=prior.field(host.K), trace=prior.field(host.trace))
    else:
        host = hmc.run_chains(hmc.ml_value_and_grad(c["sur"], data), x0, MC.HMC_EVALS, correct=fv, **kw)
    dev = hmc.run_chains_device(None, x0, MC.HMC_EVALS, model="ml", surrogate=c["sur"], data=data, correct=fin4, ml_form=form,
                                prior=prior if field else None, **kw)
    assert dev.fused is True and dev.ml_form == form and dev.n_fom == MC.HMC_PROPOSALS + 1
    _close(dev, host)
    assert np.array_equal(dev.accept1, host.accept1) and np.all(dev.accept1 >= dev.accept)
    assert np.allclose(dev.correction, host.correction, rtol=1e-9, atol=1e-9 * np.nanmax(np.abs(host.correction)), equal_nan=True)


# ---- 9. eighty chains ------------------------------------------------------------------------------------------------------------------------
def test_eighty_chains_in_both_forms_are_the_same_bits(chains):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    c = chains
    kw = dict(seeds=list(range(400, 400 + MC.WIDE_C)), eps=MC.HMC_EPS_WIDE, n_leapfrog=MC.HMC_LEAPFROG, sigma=MC.HMC_SIGMA, tau=MC.HMC_TAU,
              rng="philox", keep_trace=True, model="ml", surrogate=c["sur"], data=c["data"])
    x0 = SC.hmc_starts(MC.WIDE_C)
    a = hmc.run_chains_device(None, x0, MC.HMC_EVALS, ml_form="steps", **kw)
    b = hmc.run_chains_device(None, x0, MC.HMC_EVALS, ml_form="trajectory", **kw)
    assert a.ml_form == "steps" and b.ml_form == "trajectory" and a.graph and b.graph
    assert np.array_equal(a.K, b.K) and np.array_equal(a.trace, b.trace) and np.array_equal(a.accept, b.accept)
    assert 0 < a.accept.sum() < MC.WIDE_C * MC.HMC_PROPOSALS


def test_without_ml_form_everything_is_as_it_was(chains):
    """The fused form is still refused for model="ml" and fused=None still takes the torch-op form."""
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc
    c = chains
    kw = dict(model="ml", surrogate=c["sur"], data=c["data"], **MC.chain_kw(False))
    with pytest.raises(_ffi.FinromError, match="status %d" % _ffi.ERR_UNSUPPORTED):
        hmc.run_chains_device(None, SC.hmc_starts(), MC.HMC_EVALS, fused=True, **kw)
    res = hmc.run_chains_device(None, SC.hmc_starts(), MC.HMC_EVALS, fused=None, **kw)
    assert res.get("fused") is False and res.model == "ml" and "ml_form" not in res
