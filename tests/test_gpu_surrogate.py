"""The pure deep-learning surrogate on the device (finrom_mlp_misfit_grad, csrc/mlp_surrogate.hip; model="ml" in estimate_MAP, hmc
and laplace): both forms of the call against the float64 reference of tests/mlp_cases.py under its tolerance rule (A = 16), the exact
layout case, row independence and NaN containment of the tile form bit for bit, capture and replay, the _Batch convention, the
Jacobian, MAP and the HMC chains against the host recursion over the same device calls.

Reference of the misfit (tests/surrogate_cases.py): out = forward64, loss = 1/2 |d - out|^2, grad = -vjp64(d - out); host32:
ResBnFcModel.predict / .vjp."""
import functools

import numpy as np
import pytest

import mlp_cases as K
import surrogate_cases as SC

pytestmark = pytest.mark.gpu

PINNED = (130, 64, 5, 9)
ERR_ARG = -1                                       # FINROM_ERR_ARG (include/finrom.h)
MODELS = {"ref40": (1597, 50, 3, 40, False), "ref9-L5": (1597, 50, 5, 9, False), "tiny": (37, 17, 0, 1, False), "pins": PINNED + (True,)}


@functools.lru_cache(maxsize=None)
def _rig(shape, smax=200):
    """(model, device model, X [smax, n_in], shared data, per-sample data, ref64 / host32 for both kinds of data): computed once."""
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    n_in, n_w, L, n_out, pins = shape
    model = K.make_model(n_in, n_w, L, n_out, seed=17, pins=pins)
    X = K.forward_inputs(n_in, smax, seed=4) if n_in < 100 else K.rom_inputs(n_in, smax, seed=4)
    rng = np.random.default_rng([n_in, n_w, n_out])
    d1, dS = rng.uniform(0.2, 1.0, n_out), rng.uniform(0.2, 1.0, (smax, n_out))
    return model, DeviceErrorModel(model), X, {False: d1, True: dS}, {ps: SC.misfit_refs(model, X, d) for ps, d in ((False, d1), (True, dS))}


def _compare(tag, got, refs, rows):
    ref, host = refs
    for name in ("out", "loss", "grad"):
        if got.get(name) is None:
            continue
        r64, h32 = ref[name][rows], host[name][rows]
        print(f"RATIO form={tag} {name} {K.ratio(got[name], h32, r64):.3f}")
        assert got[name].shape == r64.shape and got[name].dtype == np.float64
        assert np.max(np.abs(got[name] - r64)) <= K.bound(h32, r64), (tag, name)


def _call(dev, X, data, per_sample, rows, **kw):
    return dev.misfit_grad(X[rows], data[per_sample][rows] if per_sample else data[per_sample], **kw)


# ---- per-sample form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 64])
@pytest.mark.parametrize("name", list(MODELS))
def test_per_sample_form_matches_the_reference(name, S):
    model, dev, X, data, refs = _rig(MODELS[name])
    dev.set_tile_min(65)
    rows = slice(5, 5 + S)
    for ps in (False, True):
        got = _call(dev, X, data, ps, rows)
        assert dev.last_form() == 1
        _compare(f"per-sample/{name}/S{S}/{'rows' if ps else 'shared'}", got, refs[ps], rows)
    value = _call(dev, X, data, True, rows, want_grad=False)
    assert value["grad"] is None and np.array_equal(value["loss"], got["loss"]) and np.array_equal(value["out"], got["out"])
    pred = dev.misfit_grad(X[rows], None, want_grad=False)
    assert pred["loss"] is None and pred["grad"] is None and np.array_equal(pred["out"], got["out"])


# ---- tile form ---------------------------------------------------------------------------------------------------------------------------
# (shape, S, forced with set_tile_min(1)): the four models at every S of the issue, the K tails n_in mod 4 = 1, 3, 0, 1, 3, the widths
# around the 16-column blocks, the output counts; forced: the tile's own row counts below 65
TILE = [(MODELS["ref40"], 65, False), (MODELS["ref40"], 200, False), (MODELS["ref9-L5"], 79, False), (MODELS["ref9-L5"], 128, False),
        (MODELS["tiny"], 80, False), (MODELS["tiny"], 81, False), (MODELS["pins"], 65, False), (MODELS["pins"], 200, False),
        ((1, 1, 1, 1, False), 65, False), ((3, 15, 2, 40, False), 79, False), ((4, 16, 1, 64, False), 80, False),
        ((5, 17, 3, 1, False), 81, False), ((7, 64, 2, 40, False), 128, False), ((64, 16, 0, 64, False), 200, False),
        ((65, 15, 1, 1, False), 65, False),
        (MODELS["ref40"], 1, True), (MODELS["tiny"], 15, True), (MODELS["pins"], 16, True), ((5, 17, 3, 1, False), 17, True),
        (MODELS["ref9-L5"], 63, True), ((7, 64, 2, 40, False), 1, True)]


@pytest.mark.parametrize("shape,S,forced", TILE, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tile_form_matches_the_reference(shape, S, forced):
    model, dev, X, data, refs = _rig(shape)
    dev.set_tile_min(1 if forced else 65)                                # (the library's default is the measured crossover, 4096)
    rows = slice(0, S)
    for ps in (False, True):
        got = _call(dev, X, data, ps, rows)
        assert dev.last_form() == 2
        _compare(f"tile/{'-'.join(map(str, shape[:4]))}/S{S}/{'rows' if ps else 'shared'}", got, refs[ps], rows)
    value = _call(dev, X, data, True, rows, want_grad=False)
    assert value["grad"] is None and np.array_equal(value["loss"], got["loss"]) and np.array_equal(value["out"], got["out"])
    pred = dev.misfit_grad(X[rows], None, want_grad=False)
    assert pred["loss"] is None and np.array_equal(pred["out"], got["out"])
    dev.set_tile_min(65)


def test_the_default_threshold_is_the_measured_crossover():
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    model = K.make_model(20, 8, 1, 3, seed=2)
    dev = DeviceErrorModel(model)
    X = K.rom_inputs(20, 4096, seed=1)
    dev.misfit_grad(X[:4095], np.ones(3), want_grad=False)
    assert dev.last_form() == 1
    dev.misfit_grad(X, np.ones(3), want_grad=False)
    assert dev.last_form() == 2


def test_the_tile_form_takes_inputs_beyond_the_per_sample_forms_lds():
    """n_in above finrom_mlp_forward_max_in: the per-sample form refuses, the tile form streams k in chunks."""
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    n_in = K.FORWARD_MAX_IN + 3
    model = K.make_model(n_in, 17, 1, 9, seed=3)
    dev = DeviceErrorModel(model)
    dev.set_tile_min(65)
    X, d = K.rom_inputs(n_in, 66, seed=2), np.linspace(0.2, 1.0, 9)
    with pytest.raises(_ffi.FinromError):
        dev.misfit_grad(X[:2], d)
    got = dev.misfit_grad(X, d)
    assert dev.last_form() == 2
    _compare("tile/wide-input", got, SC.misfit_refs(model, X, d), slice(None))


# ---- exact layout ------------------------------------------------------------------------------------------------------------------------
def test_both_forms_give_the_exact_integers_of_the_layout_case():
    """An asymmetric integer W0 and Wh: a transposed fragment or the f64 row map of the matrix cores gives other integers."""
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    model, X, data, out, loss, grad = SC.exact_case()
    dev = DeviceErrorModel(model)
    for tile_min, rows, form in ((65, slice(None), 2), (1, slice(0, 17), 2), (1000, slice(None), 1), (1000, slice(3, 67), 1)):
        dev.set_tile_min(tile_min)
        got = dev.misfit_grad(X[rows], data[rows])
        assert dev.last_form() == form
        for name, want in (("out", out), ("loss", loss), ("grad", grad)):
            assert np.array_equal(got[name], want[rows]), (form, rows, name, np.max(np.abs(got[name] - want[rows])))


# ---- row independence of the tile form ---------------------------------------------------------------------------------------------------
def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_a_tile_rows_bits_do_not_depend_on_its_place_or_its_neighbours():
    model, dev, X, data, _ = _rig(MODELS["ref40"])
    dev.set_tile_min(65)
    D = data[True]
    base = dev.misfit_grad(X, D)
    assert dev.last_form() == 2 and np.isfinite(base["grad"]).all()
    perm = np.random.default_rng(0).permutation(200)
    got = dev.misfit_grad(X[perm], D[perm])
    for name in ("out", "loss", "grad"):
        assert _bits(got[name], base[name][perm]), ("permuted", name)
    for off in (0, 1, 135):
        got = dev.misfit_grad(X[off:off + 65], D[off:off + 65])
        assert dev.last_form() == 2
        for name in ("out", "loss", "grad"):
            assert _bits(got[name], base[name][off:off + 65]), ("window", off, name)


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_row_that_is_not_finite_is_nan_and_every_other_row_keeps_its_bits(value):
    model, dev, X, data, _ = _rig(MODELS["ref40"])
    dev.set_tile_min(65)
    D = data[True]
    base = dev.misfit_grad(X, D)
    bad = [0, 15, 16, 64, 199]
    Xb = X.copy()
    for i, s in enumerate(bad):
        Xb[s, (0, 3, 700, 1595, 1596)[i]] = value if i % 2 == 0 else -value
    got = dev.misfit_grad(Xb, D)
    good = np.setdiff1d(np.arange(200), bad)
    for name in ("out", "loss", "grad"):
        assert np.isnan(got[name][bad]).all(), name
        assert _bits(got[name][good], base[name][good]), name


# ---- capture -----------------------------------------------------------------------------------------------------------------------------
def test_captured_calls_replay_the_bits_of_stream_order():
    import torch
    model, dev, X, data, _ = _rig(MODELS["ref9-L5"])
    dev.set_tile_min(65)
    Xt = torch.from_numpy(X).cuda()
    dt = torch.from_numpy(data[False]).cuda()
    want = [dev.misfit_grad(Xt[:S], dt) for S in (4, 80)]                 # the warm-up: workspaces and padded weights exist
    forms = []
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for S in (4, 80):
            dev.misfit_grad(Xt[:S], dt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = []
        for S in (4, 80):
            got.append(dev.misfit_grad(Xt[:S], dt))
            forms.append(dev.last_form())
    assert forms == [1, 2]
    for _ in range(2):
        for r in got:
            for t in r.values():
                t.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        for r, w in zip(got, want):
            for name in ("out", "loss", "grad"):
                assert torch.equal(r[name], w[name]), name


def test_the_first_tile_call_inside_a_capture_is_refused_with_a_message():
    import torch
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    model = K.make_model(20, 8, 1, 3, seed=2)
    dev = DeviceErrorModel(model)
    dev.set_tile_min(65)
    Xt, dt = torch.ones(70, 20, dtype=torch.float64, device="cuda"), torch.ones(3, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        twice = Xt * 2.0                                                  # (the capture is not empty)
        with pytest.raises(_ffi.FinromError, match="capture"):
            dev.misfit_grad(Xt, dt)
    torch.cuda.synchronize()
    assert dev.last_form() == 0
    assert np.isfinite(dev.misfit_grad(Xt, dt)["loss"].cpu().numpy()).all() and dev.last_form() == 2


# ---- surface -----------------------------------------------------------------------------------------------------------------------------
def test_numpy_in_numpy_out_and_torch_in_torch_out_agree_bit_for_bit():
    import torch
    model, dev, X, data, _ = _rig(MODELS["pins"])
    dev.set_tile_min(65)
    for S in (3, 70):
        a = dev.misfit_grad(X[:S], data[True][:S])
        b = dev.misfit_grad(torch.from_numpy(X[:S]).cuda(), torch.from_numpy(data[True][:S]).cuda())
        c = dev.misfit_grad(torch.from_numpy(X[:S]).cuda(), data[True][:S])          # (mixed: NumPy data beside a torch batch)
        for name in ("out", "loss", "grad"):
            assert isinstance(a[name], np.ndarray) and b[name].is_cuda and b[name].dtype == torch.float64
            assert _bits(a[name], b[name].cpu().numpy()) and _bits(a[name], c[name].cpu().numpy()), (S, name)


def test_argument_errors_of_the_entry_point():
    import ctypes as C
    from bayesianinferencedl_amd import _ffi
    model, dev, X, data, _ = _rig(MODELS["tiny"])
    L = _ffi.lib()
    p = C.c_void_p(8)                                                     # (never dereferenced: every call below is refused first)
    assert L.finrom_mlp_misfit_grad(None, p, p, 0, 1, p, p, p, None) == ERR_ARG
    assert L.finrom_mlp_misfit_grad(dev._h, p, p, 0, -1, p, p, p, None) == ERR_ARG
    assert L.finrom_mlp_misfit_grad(dev._h, None, p, 0, 1, p, p, p, None) == ERR_ARG
    assert L.finrom_mlp_misfit_grad(dev._h, p, p, 0, 1, p, None, p, None) == ERR_ARG       # data without loss
    assert L.finrom_mlp_misfit_grad(dev._h, p, None, 0, 1, None, p, p, None) == ERR_ARG    # loss without data
    assert L.finrom_mlp_misfit_grad(dev._h, p, None, 0, 1, p, None, p, None) == ERR_ARG    # gradient without data
    assert L.finrom_mlp_misfit_grad(dev._h, p, None, 0, 1, None, None, None, None) == ERR_ARG
    assert L.finrom_mlp_misfit_grad(dev._h, None, p, 0, 0, p, p, p, None) == 0                  # S = 0: nothing to do
    assert L.finrom_mlp_set_tile_min(dev._h, 0) == ERR_ARG and L.finrom_mlp_set_tile_min(None, 5) == ERR_ARG
    with pytest.raises(ValueError):
        dev.misfit_grad(X[:3], np.ones((2, 1)))
    with pytest.raises(ValueError):
        dev.misfit_grad(X[:3], None)


@pytest.mark.parametrize("n_obs,form", [(40, 1), (64, 2)])
def test_misfit_jacobian_ml(n_obs, form):
    from bayesianinferencedl_amd.bayesian_inference.laplace import misfit_jacobian
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    model = K.make_model(SC.N4, 50, 3, n_obs, seed=8)
    k = K.rom_inputs(SC.N4, 1, seed=9)[0]
    sur = Surrogate(model)
    sur.set_tile_min(65)
    J = misfit_jacobian("ml", k, surrogate=sur)
    assert sur.last_form() == form and J.shape == (n_obs, SC.N4)
    ref = K.vjp64(model, np.broadcast_to(k, (n_obs, SC.N4)), np.eye(n_obs))
    host = misfit_jacobian("ml", k, surrogate=Surrogate(model, device=False))
    print(f"RATIO form=jacobian/{n_obs} {K.ratio(J, host, ref):.3f}")
    assert np.max(np.abs(J - ref)) <= K.bound(host, ref)


# ---- MAP ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fin4(spaces):
    from bayesianinferencedl_amd.fom.forward_solve import Fin
    return Fin(spaces(4))


def test_objective_ml_device_against_host_at_six_starts(fin4):
    import torch
    from bayesianinferencedl_amd.bayesian_inference import lbfgs
    from bayesianinferencedl_amd.bayesian_inference.estimate_MAP import objective, starting_points, unit_stiffness
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    model = SC.hmc_model()
    data = SC.hmc_data(model)
    X = starting_points(fin4.V, 6, seed=3)
    f, g, bad = objective("ml", data, surrogate=Surrogate(model), solver=fin4, gamma=1e-6).device(torch.from_numpy(X).cuda())
    assert not bad.any().item()
    tik = (1e-6, unit_stiffness(fin4.ops))
    ref, host = SC.misfit_refs(model, X, data)
    fd, gd = lbfgs.library_terms(X, f.cpu().numpy(), g.cpu().numpy(), None, tik)
    fh, gh = objective("ml", data, surrogate=Surrogate(model, device=False), solver=fin4, gamma=1e-6).host(X)[:2]
    fr, gr = lbfgs.library_terms(X, ref["loss"], ref["grad"], None, tik)
    print(f"RATIO form=objective f {K.ratio(fd, fh, fr):.3f} g {K.ratio(gd, gh, gr):.3f}")
    assert np.max(np.abs(fd - fr)) <= K.bound(fh, fr) and np.max(np.abs(gd - gr)) <= K.bound(gh, gr)


def test_estimate_map_with_a_fitted_surrogate(fin4, tmp_path):
    from bayesianinferencedl_amd.bayesian_inference import lbfgs
    from bayesianinferencedl_amd.bayesian_inference.estimate_MAP import estimate_map, objective, starting_points, unit_stiffness
    from bayesianinferencedl_amd.deep_learning.dl_model import SURROGATE_LAYERS, SURROGATE_WIDTH, ResBnFcModel, Surrogate
    Z = starting_points(fin4.V, 200, seed=5)
    Q = np.asarray(fin4.forward_batch(Z, want_w=False)["qoi"])                      # the targets: FOM observables from the device
    model = ResBnFcModel(SC.N4, Q.shape[1], SURROGATE_LAYERS, SURROGATE_WIDTH, seed=0)
    model.fit(Z, Q, epochs=4, batch_size=50, lr=3e-4, seed=0)
    sur = Surrogate(model)
    k_true = Z[7]
    res = estimate_map(fin4, None, k_true, models=("ml",), surrogate=sur, seed=2, out_dir=str(tmp_path), maxiter=25)
    r = res["ml"]
    X0, x = res["starts"], r["x"]
    assert x.shape == X0.shape == (6, SC.N4)
    tik = (1e-6, unit_stiffness(fin4.ops))
    start = objective("ml", res["data"], surrogate=Surrogate(model, device=False), solver=fin4, gamma=1e-6)
    f0 = start.host(np.clip(X0, *res["bounds"]))[0]
    fh = start.host(x)[0]
    ref = SC.misfit_refs(model, x, res["data"])[0]
    fr = lbfgs.library_terms(x, ref["loss"], ref["grad"], None, tik)[0]
    print(f"RATIO form=map fun {K.ratio(r['fun'], fh, fr):.3f}; fun {r['fun']} from {f0}")
    assert np.max(np.abs(r["fun"] - fr)) <= K.bound(fh, fr)
    assert np.all(r["fun"] < f0)
    assert np.array_equal(np.load(tmp_path / "res_ML.npy"), x[r["best"]])


# ---- HMC ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chains(spaces):
    from bayesianinferencedl_amd.bayesian_inference.gaussian_field import GaussianFieldPrior
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    model = SC.hmc_model()
    return dict(model=model, sur=Surrogate(model), data=SC.hmc_data(model), prior=GaussianFieldPrior(spaces(4), amplitude=0.1, mean=1.0))


def _kw(field, **more):
    return dict(seeds=SC.HMC_SEEDS, eps=SC.HMC_EPS["field" if field else "iid"], n_leapfrog=SC.HMC_LEAPFROG, sigma=SC.HMC_SIGMA,
                tau=SC.HMC_TAU, **more)


def _close(dev, host, field=False):
    assert dev.proposals == host.proposals and np.array_equal(dev.accept, host.accept), (dev.accept, host.accept)
    if host.trace is not None:
        assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    assert np.linalg.norm(dev.K - host.K) <= 1e-9 * np.linalg.norm(host.K)
    if field:
        assert np.linalg.norm(dev.V - host.V) <= 1e-9 * np.linalg.norm(host.V)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "stream"])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_device_chains_follow_the_host_recursion_over_the_same_device_calls(chains, field, graph):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    c = chains
    prior = c["prior"] if field else None
    x0 = SC.hmc_starts(field=field)
    want = {0, 4, 11}
    host = hmc.run_chains(hmc.ml_value_and_grad(c["sur"], c["data"]), x0, SC.HMC_EVALS, keep_trace=True, record=want, prior=prior, **_kw(field))
    assert 0 < host.accept.sum() < 4 * SC.HMC_PROPOSALS, host.accept
    dev = hmc.run_chains_device(None, x0, SC.HMC_EVALS, model="ml", surrogate=c["sur"], data=c["data"], keep_trace=True, record=want,
                                prior=prior, graph=graph, **_kw(field))
    assert dev.model == "ml" and dev.get("fused") is False
    _close(dev, host, field)
    assert [e for e, *_ in dev.recorded] == [e for e, *_ in host.recorded] == sorted(want)
    for ev, Kr, loss, grad in dev.recorded:                                          # recorded evaluations: the float64 reference
        ref, h32 = SC.misfit_refs(c["model"], Kr, c["data"])
        print(f"RATIO form=hmc/{'field' if field else 'iid'}/ev{ev} loss {K.ratio(loss, h32['loss'], ref['loss']):.3f} "
              f"grad {K.ratio(grad, h32['grad'], ref['grad']):.3f}")
        assert np.max(np.abs(loss - ref["loss"])) <= K.bound(h32["loss"], ref["loss"])
        assert np.max(np.abs(grad - ref["grad"])) <= K.bound(h32["grad"], ref["grad"])


def test_the_fused_form_is_refused_and_fused_none_falls_back(chains):
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import hmc
    c = chains
    kw = dict(model="ml", surrogate=c["sur"], data=c["data"], **_kw(False))
    with pytest.raises(_ffi.FinromError, match="status %d" % _ffi.ERR_UNSUPPORTED):
        hmc.run_chains_device(None, SC.hmc_starts(), SC.HMC_EVALS, fused=True, **kw)
    res = hmc.run_chains_device(None, SC.hmc_starts(), SC.HMC_EVALS, fused=None, **kw)
    assert res.get("fused") is False and res.model == "ml"


def test_delayed_acceptance_under_the_surrogate_with_the_fom_deciding(chains, fin4):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    c = chains
    data = np.asarray(fin4.qoi_operator(fin4.forward(np.exp(0.25 * np.random.default_rng(11).standard_normal(SC.N4)))[0]))
    # the network is no model of the fin: a wide sigma keeps the second stage from rejecting everything
    kw = dict(seeds=SC.HMC_SEEDS, eps=0.05, n_leapfrog=SC.HMC_LEAPFROG, sigma=5.0, tau=SC.HMC_TAU, rng="philox")
    sur9 = c["sur"]
    host = hmc.run_chains(hmc.ml_value_and_grad(sur9, data), SC.hmc_starts(), SC.HMC_EVALS, correct=hmc.fom_value(fin4, data), keep_trace=True, **kw)
    dev = hmc.run_chains_device(None, SC.hmc_starts(), SC.HMC_EVALS, model="ml", surrogate=sur9, data=data, correct=fin4, keep_trace=True, **kw)
    _close(dev, host)
    assert np.array_equal(dev.accept1, host.accept1) and np.all(dev.accept1 >= dev.accept)
    assert np.allclose(dev.correction, host.correction, rtol=1e-9, atol=1e-9 * np.nanmax(np.abs(host.correction)), equal_nan=True)


def test_a_metric_is_accepted(chains):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    from bayesianinferencedl_amd.bayesian_inference.laplace import LowRankMetric
    c = chains
    Vt = np.linalg.qr(np.random.default_rng(1).standard_normal((SC.N4, 3)))[0].T
    metric = LowRankMetric(Vt, np.array([4.0, 2.0, 0.5]))
    x0 = SC.hmc_starts(field=True)
    host = hmc.run_chains(hmc.ml_value_and_grad(c["sur"], c["data"]), x0, SC.HMC_EVALS, prior=c["prior"], metric=metric, **_kw(True))
    dev = hmc.run_chains_device(None, x0, SC.HMC_EVALS, model="ml", surrogate=c["sur"], data=c["data"], prior=c["prior"], metric=metric, **_kw(True))
    _close(dev, host, True)


def test_eighty_chains_take_the_tile_form_inside_a_proposal(chains):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    c = chains
    kw = dict(seeds=list(range(400, 400 + SC.WIDE_C)), eps=SC.HMC_EPS_WIDE, n_leapfrog=SC.HMC_LEAPFROG, sigma=SC.HMC_SIGMA, tau=SC.HMC_TAU,
              rng="philox")
    x0 = SC.hmc_starts(SC.WIDE_C)
    c["sur"].set_tile_min(65)
    host = hmc.run_chains(hmc.ml_value_and_grad(c["sur"], c["data"]), x0, SC.HMC_EVALS, **kw)
    assert c["sur"].last_form() == 2
    assert 0 < host.accept.sum() < SC.WIDE_C * SC.HMC_PROPOSALS
    dev = hmc.run_chains_device(None, x0, SC.HMC_EVALS, model="ml", surrogate=c["sur"], data=c["data"], **kw)
    assert c["sur"].last_form() == 2
    c["sur"].set_tile_min(4096)
    _close(dev, host)
