"""The learned error model's inference kernels on the device (csrc/mlp_kernels.hip, csrc/mlp_device.h, the pieces inside
csrc/rom_onesample.hip and the walk back inside rom_kernels.hip's gradient contraction) against the float64 network of
tests/mlp_cases.py, at every width, depth, output count, input size and batch size class that selects code, in every call form:

    forward alone        finrom_mlp_predict: mlp_forward_kernel (mlp_forward_body<1024>)
    "one"                finrom_romml_grad's one-sample form: mlp_first_layer_part<256> in four spare workgroups of the contraction,
                         mlp_forward_tail_wave<staged?> in a spare wave of the solve kernel, mlp_backward_hidden_wave in a spare
                         workgroup of the gradient contraction, mlp_backward_kernel<8> from its hand-over
    "b8" / "b1"          the batched form: mlp_forward_kernel with the fused sub-fin averages, mlp_backward_kernel<8> (S <= 64) or
                         <1> (S > 64) walking back in its own wave 0
    leapfrog             finrom_hmc_leapfrog: "one" with the position update in front and the momentum update and the next step's
                         averages behind

The tolerance is the rule of mlp_cases.bound: max|dev - ref64| <= 16 max(max|host32 - ref64|, 2^-24 max|ref64|), host32 the fp32
NumPy model (for the fused call: the oracle's dense reduced model with it).  Every comparison prints a line "RATIO form=... "
with max|dev - ref64| over max(max|host32 - ref64|, floor); DESIGN.md records the worst per form.  Which branch a row takes is
asserted on the CPU (tests/test_mlp_host.py); nothing here is skipped at run time."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import mlp_cases as K

pytestmark = pytest.mark.gpu


def _check(form, name, qty, dev, host32, ref64):
    dev, ref64 = np.asarray(dev, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert dev.shape == ref64.shape and np.isfinite(dev).all(), (form, name, qty, dev.shape, ref64.shape)
    err, b = float(np.max(np.abs(dev - ref64))), K.bound(host32, ref64)
    print(f"RATIO form={form} case={name} qty={qty} ratio={err / (b / K.A):.3f} dev={err:.3e} host32={np.max(np.abs(np.asarray(host32) - ref64)):.3e} "
          f"scale={np.max(np.abs(ref64)):.3e}")
    assert err <= b, (form, name, qty, err, b)


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


# ---- forward alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.FWD_CASES, ids=K.fwd_id)
def test_forward_against_the_float64_network(c):
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    model, X = K.fwd_model(c), K.forward_inputs(c.n_in, c.S)
    e = DeviceErrorModel(model).predict(X)
    assert e.shape == (c.S, c.n_out)
    _check("forward", K.fwd_id(c), "e", e, model.predict(X), K.forward64(model, X)[0])


@pytest.mark.parametrize("c", K.FWD_BITWISE, ids=K.fwd_id)
def test_forward_sample_alone_is_the_sample_in_its_batch_and_two_runs_agree(c):
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    model, X = K.fwd_model(c), K.forward_inputs(c.n_in, c.S)
    dev = DeviceErrorModel(model)
    e = _np(dev.predict(_dev(X)))
    assert np.array_equal(e, _np(dev.predict(_dev(X)))) and np.array_equal(e, dev.predict(X))      # again; and through the NumPy door
    for s in sorted({0, c.S // 2, c.S - 1}):
        assert np.array_equal(dev.predict(X[s:s + 1])[0], e[s]), s


def test_an_input_wider_than_the_forward_kernels_lds_is_an_error_code_not_a_failed_launch():
    """n_in = 15 200 runs (a row of the ladder); 15 201 is refused with FINROM_ERR_UNSUPPORTED before any launch, and the call behind
    it finds nothing left over."""
    import torch
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    c = K.FWD_TOO_WIDE
    assert c.n_in == _ffi.lib().finrom_mlp_forward_max_in() + 1
    wide = DeviceErrorModel(K.fwd_model(c))                 # (finrom_mlp_create takes it: the one-sample form has room for 24 576)
    with pytest.raises(_ffi.FinromError, match=r"status -4\).*n_in = 15201 exceeds 15200"):
        wide.predict(K.forward_inputs(c.n_in, c.S))
    with pytest.raises(_ffi.FinromError, match=r"status -4\)"):
        wide.predict(_dev(K.forward_inputs(c.n_in, c.S)))
    torch.cuda.synchronize()
    ok = K.FWD_CASES[0]
    model, X = K.fwd_model(ok), K.forward_inputs(ok.n_in, ok.S)
    _check("forward", "after-the-refusal", "e", DeviceErrorModel(model).predict(X), model.predict(X), K.forward64(model, X)[0])
    torch.cuda.synchronize()


# ---- value and gradient: finrom_romml_grad ------------------------------------------------------------------------------------------
_ROMS, _FIVE = {}, {}


def _rom(spaces, c):
    """The device model of a row's mesh, basis and observation operator (one per (m, r, n_obs): the projection is a switch)."""
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    key = (c.m, c.r, c.n_obs)
    if key not in _ROMS:
        prob, phi, ro = K.oracle_rig(*key)
        rom = AffineROMFin(spaces(c.m), None, phi, external_obs=(c.n_obs == 40))
        rom._ensure_gradient()
        assert rom.n == K.MESH_N[c.m] and np.max(np.abs(np.asarray(rom.ops.S) - ro.dsigma_dk)) <= 1e-12 * np.max(np.abs(ro.dsigma_dk))
        assert np.max(np.abs(rom.B_obs_phi - ro.B_obs_phi)) <= 1e-12 * np.max(np.abs(ro.B_obs_phi))
        _ROMS[key] = rom
    return _ROMS[key]


def _five(spaces, c):
    """The reduced model driven by five parameters (mlp_cases.five_parameters): a RomEngine of its own over the same psi tables."""
    from bayesianinferencedl_amd._ffi import DeviceBuffer
    from bayesianinferencedl_amd.engine import RomEngine
    key = (c.m, c.r, c.n_obs)
    if key not in _FIVE:
        rom = _rom(spaces, c)
        E, S5 = K.five_parameters(np.asarray(rom.ops.S))
        dA5 = [sum(E[i, j] * rom.dA_dsigmak_phi[i] for i in range(9)) for j in range(5)]
        tables = [rom._psi_tables[0]] + dA5
        eng = RomEngine(rom.n, rom.n_r, 5, [(p, tables[p]) for p in range(6)], rom.ops.F, rom.B_obs_phi)
        pairs = [(p, i) for p in range(6) for i in range(5) if np.any(tables[p].T @ dA5[i])]
        eng.set_gradient_blocks(pairs, np.stack([tables[p].T @ dA5[i] for p, i in pairs]))
        gp = [(p, q) for p in range(6) for q in range(p, 6) if p == q or np.any(tables[p].T @ tables[q])]
        eng.set_gram_blocks(gp, np.stack([tables[p].T @ tables[q] if p == q else tables[p].T @ tables[q] + tables[q].T @ tables[p] for p, q in gp]))
        _FIVE[key] = (eng, DeviceBuffer.from_numpy(np.ascontiguousarray(S5)))
    return _FIVE[key]


def _caller(spaces, c, model=None):
    """-> (call(K, data) -> dict of NumPy arrays, the rom handle, the error model's handle, the averaging operator's buffer); every
    call runs on device tensors.  A fresh DeviceErrorModel per caller."""
    from bayesianinferencedl_amd.engine import DeviceErrorModel, romml_grad
    rom = _rom(spaces, c)
    mlp = DeviceErrorModel(K.fused_model(c) if model is None else model)
    if c.P == 5:
        eng, sop = _five(spaces, c)
        eng.set_projection(c.projection)
    else:
        rom.set_projection(c.projection)
        eng, sop = rom._rom, rom._avg._S

    def call(Kf, data):
        (eng if c.P == 5 else rom).set_projection(c.projection)
        return {k: _np(v) for k, v in romml_grad(eng, mlp, sop, _dev(Kf), _dev(data)).items()}
    return call, eng, mlp, sop


@pytest.mark.parametrize("c", K.FUSED_CASES, ids=lambda c: c.name)
def test_value_and_gradient_against_the_float64_reference(spaces, c):
    idx = K.compared_samples(c.S)
    Kf, data, r64, r32 = K.fused_refs(c, idx)
    res = _caller(spaces, c)[0](Kf, data)
    assert (res["info"] == 0).all() and res["grad"].shape == Kf.shape and res["e_NN"].shape == (c.S, c.n_obs)
    for qty, key in (("e_nn", "e_NN"), ("loss", "loss"), ("grad", "grad")):
        _check(c.form, c.name, qty, res[key][idx], r32[qty], r64[qty])
    assert np.max(np.abs(res["qoi_r"][idx] - r64["qoi_r"])) <= 1e-8 * np.max(np.abs(r64["qoi_r"]))
    # the value is 1/2 |r|^2 of the pieces the call returns, for EVERY sample (the kernels subtract in another order: data - e - q)
    r = np.broadcast_to(data, res["e_NN"].shape) - (res["qoi_r"] + res["e_NN"])
    assert np.max(np.abs(res["loss"] - 0.5 * np.sum(r * r, axis=1))) <= 1e-13 * np.max(res["loss"])


def _same(a, b, keys=("grad", "loss", "e_NN", "qoi_r", "info")):
    return [k for k in keys if not np.array_equal(a[k], b[k])]


@pytest.mark.parametrize("name", K.FUSED_BITWISE)
def test_a_sample_does_not_depend_on_its_batch_and_two_runs_agree(spaces, name):
    """Bit for bit.  One-sample form: the sample alone (S = 1 takes the same form).  Batched forms: the network's output for the
    sample alone where a batch of one takes the same form (b8), and every output for the sample at its own place among OTHER
    neighbours (the reduced model's batched kernels are not claimed to be independent of a sample's place in its block)."""
    c = K.FUSED_BY_NAME[name]
    call = _caller(spaces, c)[0]
    Kf, data = K.rom_inputs(K.MESH_N[c.m], c.S, seed=3), K.fused_data(c)
    res = call(Kf, data)
    assert (res["info"] == 0).all() and _same(res, call(Kf, data)) == []
    other = K.rom_inputs(K.MESH_N[c.m], c.S, seed=4)
    for s in sorted({0, c.S // 2, c.S - 1}):
        d1 = data[s:s + 1] if c.per_sample else data
        if c.form == "one":
            one = call(Kf[s:s + 1], d1)
            assert all(np.array_equal(one[k][0], res[k][s]) for k in ("grad", "loss", "e_NN", "qoi_r")), (name, s)
            continue
        if c.form == "b8":
            assert np.array_equal(call(Kf[s:s + 1], d1)["e_NN"][0], res["e_NN"][s]), (name, s)
        K2 = other.copy(); K2[s] = Kf[s]
        n2 = c.S if c.form == "b1" else s + 1                # (b1: the batch stays beyond 64 samples; b8: the sample comes last)
        mix = call(K2[:n2], data[:n2] if c.per_sample else data)
        assert all(np.array_equal(mix[k][s], res[k][s]) for k in ("grad", "loss", "e_NN", "qoi_r")), (name, s)
        if s > 0:                                            # (the neighbours did change)
            assert not np.array_equal(mix["grad"][s - 1], res["grad"][s - 1])


def test_the_forms_agree_with_each_other_to_tolerance(spaces):
    """The same four fields through the one-sample form, the batched form with NP = 8 and (inside a batch of 65) with NP = 1: each
    within the rule of the float64 reference, hence within twice the bound of each other."""
    one, b8, b1 = (K.FUSED_BY_NAME[n] for n in ("one-staged-ref", "b8-ref", "b1-ref-S65"))
    assert (one.m, one.r, one.n_w, one.n_layers) == (b8.m, b8.r, b8.n_w, b8.n_layers) == (b1.m, b1.r, b1.n_w, b1.n_layers)
    Kf, data, r64, r32 = K.fused_refs(one)
    pad = np.concatenate([Kf, K.rom_inputs(K.MESH_N[b1.m], b1.S - one.S, seed=5)])
    out = {"one": _caller(spaces, one)[0](Kf, data), "b8": _caller(spaces, b8)[0](Kf, data), "b1": _caller(spaces, b1)[0](pad, data)}
    for qty, key in (("e_nn", "e_NN"), ("loss", "loss"), ("grad", "grad")):
        b = K.bound(r32[qty], r64[qty])
        for f in out:
            _check(f, "cross-form", qty, out[f][key][:one.S], r32[qty], r64[qty])
        for f, g in (("one", "b8"), ("one", "b1"), ("b8", "b1")):
            assert np.max(np.abs(out[f][key][:one.S] - out[g][key][:one.S])) <= 2 * b, (f, g, qty)


@pytest.mark.parametrize("name", K.FUSED_NAN)
def test_a_nan_field_stays_in_its_sample(spaces, name):
    c = K.FUSED_BY_NAME[name]
    call = _caller(spaces, c)[0]
    Kf, data = K.rom_inputs(K.MESH_N[c.m], c.S, seed=3), K.fused_data(c)
    clean = call(Kf, data)
    assert (clean["info"] == 0).all() and np.isfinite(clean["grad"]).all()
    for j in sorted({1, c.S - 1}):
        Kb = Kf.copy(); Kb[j, 7 % Kf.shape[1]] = np.nan
        dirty = call(Kb, data)
        keep = np.arange(c.S) != j
        assert dirty["info"][j] != 0 and (dirty["info"][keep] == 0).all(), (name, j, dirty["info"])
        for k in ("e_NN", "loss", "grad", "qoi_r"):
            assert np.array_equal(dirty[k][keep], clean[k][keep]), (name, j, k)
        assert not np.isfinite(dirty["grad"][j]).all()
    assert _same(call(Kf, data), clean) == []


# ---- the leapfrog form --------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl(a b + c) in double, elementwise, by exact rational arithmetic (float(Fraction) rounds to nearest even)."""
    f = np.frompyfunc(lambda x, y, z: float(Fraction(x) * Fraction(y) + Fraction(z)) if np.isfinite(x) and np.isfinite(y) and np.isfinite(z) else x * y + z, 3, 1)
    return f(a, b, c).astype(np.float64)


class _Leap:
    """finrom_hmc_leapfrog on a state of its own: three steps from (K0, P0), in stream order or captured in one graph and replayed."""
    EPS, C_LIK, C_PRI, STEPS = 0.0123, 400.0, 4.0, 3

    def __init__(self, spaces, c, seed=6):
        import torch
        from bayesianinferencedl_amd import _ffi
        self.c, self.L, self.ffi = c, _ffi.lib(), _ffi
        self.call, self.eng, self.mlp, self.sop = _caller(spaces, c)
        n, S = K.MESH_N[c.m], c.S
        rng = np.random.default_rng([seed, n, S])
        self.K0, self.P0 = K.rom_inputs(n, S, seed=3), 0.05 * rng.standard_normal((S, n))
        self.mean_np = 1.0 + 0.1 * rng.standard_normal((S, n))
        self.data_np = K.fused_data(c)
        z = lambda *sh, dt=torch.float64: torch.zeros(*sh, dtype=dt, device="cuda")
        self.Kq, self.P, self.dUq = [z(S, n), z(S, n)], z(S, n), z(S, n)
        self.mean, self.data = _dev(self.mean_np), _dev(self.data_np)
        self.loss, self.info = z(S), z(S, dt=torch.int32)
        self.grad = [z(S, n) for _ in range(self.STEPS)]
        self.e = [z(S, c.n_obs) for _ in range(self.STEPS)]
        self.q = [z(S, c.n_obs) for _ in range(self.STEPS)]
        self._pad = [z(S, n), z(S), z(S, n), z(S), z(1, S, n), z(1, S), z(1, dt=torch.int64), z(1, dt=torch.int64), z(S, dt=torch.int64)]
        p = self._pad
        self.st = _ffi.HmcState(C=S, n=n, eps=self.EPS, c_lik=self.C_LIK, c_pri=self.C_PRI, mean=self.mean.data_ptr(), K=p[0].data_ptr(),
                                U=p[1].data_ptr(), dU=p[2].data_ptr(), Kq=(C.c_void_p * 2)(self.Kq[0].data_ptr(), self.Kq[1].data_ptr()),
                                P=self.P.data_ptr(), dUq=self.dUq.data_ptr(), H0=p[3].data_ptr(), P_block=p[4].data_ptr(),
                                lu_block=p[5].data_ptr(), jt=p[6].data_ptr(), pt=p[7].data_ptr(), accept=p[8].data_ptr(), trace=None,
                                loss=self.loss.data_ptr(), info=self.info.data_ptr())

    def reset(self):
        self.Kq[0].copy_(_dev(self.K0)); self.Kq[1].zero_(); self.P.copy_(_dev(self.P0)); self.dUq.zero_()

    def step(self, i, state=None):
        import torch
        rc = self.L.finrom_hmc_leapfrog(self.eng._h, self.mlp._h, self.sop.ptr, C.byref(self.st if state is None else state), i, self.data.data_ptr(),
                                        1 if self.c.per_sample else 0, self.grad[i].data_ptr(), self.q[i].data_ptr(), self.e[i].data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
        self.ffi.check(rc, "finrom_hmc_leapfrog")
        self.sop.used_on(torch.cuda.current_stream().cuda_stream)

    def snapshot(self):
        return {"Kq0": _np(self.Kq[0]), "Kq1": _np(self.Kq[1]), "P": _np(self.P), "dUq": _np(self.dUq), "loss": _np(self.loss), "info": _np(self.info),
                "grad": [_np(g) for g in self.grad], "e": [_np(e) for e in self.e], "q": [_np(q) for q in self.q]}

    def stream_order(self, watch=None):
        import torch
        self.reset()
        for i in range(self.STEPS):
            before = (_np(self.Kq[i & 1]), _np(self.P)) if watch else None
            self.step(i)
            if watch:
                torch.cuda.synchronize()
                watch(i, before, _np(self.Kq[(i + 1) & 1]), _np(self.P), _np(self.dUq), _np(self.grad[i]), _np(self.info), _np(self.loss), _np(self.e[i]), _np(self.q[i]))
        torch.cuda.synchronize()
        return self.snapshot()

    def replayed(self):
        import torch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                        # the library's workspaces are sized before the capture
            self.reset()
            for i in range(self.STEPS):
                self.step(i)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(self.STEPS):
                self.step(i)
        out = []
        for _ in range(2):
            self.reset()
            for t in self.grad + self.e + self.q:
                t.zero_()
            g.replay()
            torch.cuda.synchronize()
            out.append(self.snapshot())
        return out


def _flat_equal(a, b):
    bad = []
    for k in a:
        for x, y in zip(a[k], b[k]) if isinstance(a[k], list) else [(a[k], b[k])]:
            if not np.array_equal(x, y, equal_nan=True):
                bad.append(k)
    return bad


@pytest.mark.parametrize("name", K.LEAP_CASES)
def test_leapfrog_steps_are_exact_where_they_are_fma_and_replay_bit_for_bit(spaces, name):
    """Three steps: step 0 forms the averages itself, steps 1 and 2 take them from the step before (the theta carry).
    k_out = fma(eps, p, k), dU = fma(c_lik / c_pri, grad, k_out - mean) and p' = fma(-eps c_pri, dU, p) are checked for EQUALITY
    against exact arithmetic on the inputs the test knows (grad: the call's own output); value, gradient and network output at the
    moved field follow the rule of the float64 reference at steps 0 (no carry) and 2 (carry); one graph of the three steps,
    replayed twice, gives the bits of stream order."""
    c = K.FUSED_BY_NAME[name]
    lf = _Leap(spaces, c)
    rows = K.compared_samples(c.S) if c.S > 8 else list(range(c.S))
    prob, phi, ro = K.oracle_rig(c.m, c.r, c.n_obs)
    kw = dict(zip(("E", "Sop"), K.five_parameters(ro.dsigma_dk))) if c.P == 5 else {}
    model = K.fused_model(c)
    coef, eps_cpri = lf.C_LIK / lf.C_PRI, lf.EPS * lf.C_PRI
    seen = []

    def watch(i, before, k_out, p_new, dUq, grad, info, loss, e, q):
        k_in, p_in = before
        assert (info == 0).all() and np.isfinite(grad).all()
        assert np.array_equal(k_out[rows], _fma(lf.EPS, p_in[rows], k_in[rows])), (name, i, "k_out")
        du = _fma(coef, grad[rows], k_out[rows] - lf.mean_np[rows])
        assert np.array_equal(dUq[rows], du), (name, i, "dU")
        assert np.array_equal(p_new[rows], _fma(-eps_cpri, du, p_in[rows])), (name, i, "momentum")
        if len(rows) < c.S:                                  # the rest of a large batch: the same formulas in NumPy's two roundings
            assert np.max(np.abs(k_out - (k_in + lf.EPS * p_in))) <= 1e-15 * np.max(np.abs(k_in))
        if i in (0, 2):
            idx = rows[:4]
            refs = {net: [K.romml_ref(ro, model, k_out[s], lf.data_np[s] if c.per_sample else lf.data_np, net, **kw) for s in idx] for net in ("f64", "f32")}
            for qty, got in (("e_nn", e), ("loss", loss), ("grad", grad)):
                _check("leapfrog", f"{name}-step{i}", qty, got[idx], np.array([r[qty] for r in refs["f32"]]), np.array([r[qty] for r in refs["f64"]]))
        seen.append((k_in.copy(), p_in.copy(), grad.copy(), e.copy(), loss.copy()))
    first = lf.stream_order(watch)
    assert _flat_equal(first, lf.stream_order()) == []       # two runs
    for snap in lf.replayed():
        assert _flat_equal(first, snap) == [], name
    # the carry is an order of summation, not another number: step 1 again from its inputs on a handle that carries nothing --
    # the same moved field and network output bit for bit, value and gradient within the rule of the reference on both sides
    import torch
    fresh = _Leap(spaces, c)
    k1, p1, g1, e1, l1 = seen[1]
    fresh.reset(); fresh.Kq[1].copy_(_dev(k1)); fresh.P.copy_(_dev(p1))
    fresh.step(1)
    torch.cuda.synchronize()
    assert np.array_equal(_np(fresh.Kq[0]), seen[2][0]) and np.array_equal(_np(fresh.e[1]), e1)
    idx = rows[:4]
    refs = {net: [K.romml_ref(ro, model, seen[2][0][s], lf.data_np[s] if c.per_sample else lf.data_np, net, **kw) for s in idx] for net in ("f64", "f32")}
    for qty, a, b in (("grad", _np(fresh.grad[1]), g1), ("loss", _np(fresh.loss), l1)):
        r64, r32 = np.array([r[qty] for r in refs["f64"]]), np.array([r[qty] for r in refs["f32"]])
        _check("leapfrog", f"{name}-step1-no-carry", qty, a[idx], r32, r64)
        _check("leapfrog", f"{name}-step1-carry", qty, b[idx], r32, r64)
        assert np.max(np.abs(a[idx] - b[idx])) <= 2 * K.bound(r32, r64)


@pytest.mark.parametrize("poison", ["finite", "nan"])
@pytest.mark.parametrize("name", ["one-staged-ref", "one-unstaged-size-50x7"])
def test_a_flagged_chain_keeps_its_momentum_through_the_leapfrog_form(spaces, name, poison):
    """Chain 1 starts at a field the reduced model cannot factor -- finite: -1e200 times its positive field (A_r = psi^T psi cannot
    be indefinite; at this size it is beyond the largest double, tests/leap_field_cases.py); nan: one NaN entry -- and stays
    flagged through three steps, the two that take the carried averages included: info != 0 for it alone, dU = 0 exactly, its
    momentum's bits kept, its position still moved by the rule; every other chain bitwise as in the clean run."""
    c = K.FUSED_BY_NAME[name]
    j, steps = 1, {"clean": [], "dirty": []}

    def recorder(tag):
        def watch(i, before, k_out, p_new, dUq, grad, info, loss, e, q):
            steps[tag].append(dict(k_in=before[0], p_in=before[1], k_out=k_out, P=p_new, dUq=dUq, grad=grad, info=info, loss=loss, e=e, q=q))
        return watch
    _Leap(spaces, c).stream_order(recorder("clean"))
    dirty = _Leap(spaces, c)
    if poison == "finite":
        dirty.K0[j] = -1e200 * dirty.K0[j]
    else:
        dirty.K0[j, 7] = np.nan
    dirty.stream_order(recorder("dirty"))
    keep = np.arange(c.S) != j
    assert len(steps["dirty"]) == len(steps["clean"]) == _Leap.STEPS
    for i, (a, b) in enumerate(zip(steps["dirty"], steps["clean"])):
        assert a["info"][j] != 0 and (a["info"][keep] == 0).all() and (b["info"] == 0).all(), (name, poison, i, a["info"])
        assert np.array_equal(a["dUq"][j], np.zeros_like(a["dUq"][j])), (name, poison, i, "dU of the flagged chain")
        assert np.array_equal(a["P"][j].view(np.uint64), a["p_in"][j].view(np.uint64)), (name, poison, i, "the flagged chain's momentum moved")
        assert np.array_equal(a["k_out"][j], _fma(dirty.EPS, a["p_in"][j], a["k_in"][j]), equal_nan=True), (name, poison, i, "position")
        assert np.isnan(a["k_out"][j]).sum() == (1 if poison == "nan" else 0)
        for k in ("k_out", "P", "dUq", "grad", "loss", "e", "q"):
            assert np.isfinite(a[k][keep]).all() and np.array_equal(a[k][keep], b[k][keep]), (name, poison, i, k)


def test_the_leapfrog_form_refuses_a_batched_model(spaces):
    """The probe behind the table's "one" column: a model the one-sample form does not take is FINROM_ERR_UNSUPPORTED for
    finrom_hmc_leapfrog, and the rows named "one" above were taken (their steps ran)."""
    from bayesianinferencedl_amd import _ffi
    c = K.FUSED_BY_NAME["b8-ref"]
    lf = _Leap(spaces, c)
    lf.reset()
    with pytest.raises(_ffi.FinromError, match=r"status -4\).*one-sample form"):
        lf.step(0)


def test_the_leapfrog_form_refuses_a_null_reduced_model(spaces):
    """finrom_hmc_leapfrog with a valid state, a valid error-model handle and rom = NULL: FINROM_ERR_ARG (-1) and an error text, from
    the argument check in front of every launch (the call used to read rom->d.P first) -- the state keeps its bits."""
    import torch
    c = K.FUSED_BY_NAME["one-staged-w16"]
    lf = _Leap(spaces, c)
    lf.reset()
    torch.cuda.synchronize()
    before = lf.snapshot()
    rc = lf.L.finrom_hmc_leapfrog(None, lf.mlp._h, lf.sop.ptr, C.byref(lf.st), 0, lf.data.data_ptr(), 1 if c.per_sample else 0,
                                  lf.grad[0].data_ptr(), lf.q[0].data_ptr(), lf.e[0].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    assert b"hmc_leapfrog: bad argument" in lf.L.finrom_last_error()
    torch.cuda.synchronize()
    after = lf.snapshot()
    for k in ("Kq0", "Kq1", "P", "dUq", "loss", "info"):
        assert np.array_equal(before[k], after[k]), k
