"""The leapfrog step in whitened coordinates, driven directly on hand-made state (finrom_hmc_leapfrog_field / _field_metric,
csrc/api_hmc.hip: hmc_velocity_kernel, field_prior_kernel<false> with the fused operand w = fma(eps, q, v) and its write-back,
the plain finrom_romml_grad launches, field_prior_kernel<true> with its momentum tail) against the reference of
tests/leap_field_cases.py (checked against hmc.run_chains in tests/test_hmc_leapfrog_field_host.py).  Three steps per case; after
each one: the position update, the momentum update and its dU bit for bit against exact fused multiply-adds; the field bitwise the
plain finrom_sampler_field on the written-back w and within 2e-13 of its scale of the extended-precision product; value and
gradient bitwise a plain finrom_romml_grad at the device's field and within the rule of tests/mlp_cases.py of the float64
reference; the velocity bitwise finrom_metric_apply(INV) and within 2e-13 of its scale; flagged chains (a finite poison and a NaN,
at a first, a middle and a last chain, behind index 64 too) with dU = 0 and their momentum's bits kept on all three steps while
every other chain has the bits of the clean run; everything the step may not touch, PAD sentinel elements behind every buffer
included; a chain's independence of its batch; two runs and a replayed graph bit for bit.

Worst error / allowance observed on an MI355X (each test prints its own): field 1.1e-3 and dU 2.8e-3 of 2e-13 * scale, the
velocity 1.1e-3 of 2e-13 * scale.

The suite found one defect: finrom_romml_grad's batched forms (more than 64 chains, or the offline-online projection) cleared info
with hipMemsetAsync, and inside a captured graph that node did its work in the first replay only -- the second replay of m4-C65,
m4-C70, m4-C65-rho17 and m12-C4-oo kept the 5 the state starts with in info, so every chain counted as flagged
("assert ['Kq0', 'Kq1', 'P', 'dUq', 'loss', 'info', 'x_field', 'x_grad_field'] == []" between replay 1 and replay 2, while
replay 1 had the bits of stream order).  info is now cleared by a kernel; the runtime's behaviour is reproduced without the
library by tools/memset_node_probe.py.

Not visible to any value check: v_out written by every super-tile of a row strip instead of the diagonal one alone -- each of
them stores the same fma(eps, p, v), since x and p are not written during the launch."""
import ctypes as C

import numpy as np
import pytest

import hmc_cases as H
import leap_field_cases as F
import mlp_cases as K
import test_gpu_mlp_kernels as M

pytestmark = pytest.mark.gpu
WORST = {}
OUTPUTS = ("P", "dUq", "loss", "info")               # of the state, beside Kq[(step + 1) & 1]


def _note(what, err, bound):
    """Keep and print the worst error / allowance ratio per quantity; -> whether every element is inside its allowance."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size:
        ratio = float(np.max(err / bound))
        if not ratio <= WORST.get(what, 0.0):
            WORST[what] = ratio
            print("worst error / allowance so far:", WORST)
    return bool(np.all(err <= bound))


def _abs_ld(got, ref):
    return np.abs(np.asarray(got).astype(H.LD) - ref).astype(np.float64)


def _eq(a, b):
    """Bit for bit where the numbers are numbers, NaN where the other is NaN."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and H.same_bits(np.where(na, 0.0, a), np.where(nb, 0.0, b))


class _Shared:
    """What this module's cases share on the device, made on first use and dropped with the module: the reduced model's handles and
    one error-model handle per mesh and projection (every case puts the projection back in its reset), the prior's factor per n,
    the metric per (n, rho), and the downloads of a clean case's three steps (computed once, never written to)."""

    def __init__(self, spaces):
        self.spaces, self._rigs, self._samplers, self._metrics, self._clean = spaces, {}, {}, {}, {}

    def rig(self, lc):
        """(rom model, call, engine, error model, averaging operator)."""
        key = (lc.m, lc.projection)
        if key not in self._rigs:
            row = F.fused_row(lc)
            self._rigs[key] = (M._rom(self.spaces, row),) + tuple(M._caller(self.spaces, row))
        return self._rigs[key]

    def sampler(self, n):
        from bayesianinferencedl_amd.engine import FieldSampler
        if n not in self._samplers:
            self._samplers[n] = FieldSampler(F.factor(n))
        return self._samplers[n]

    def metric(self, n, rho):
        from bayesianinferencedl_amd.engine import MetricHandle
        if (n, rho) not in self._metrics:
            self._metrics[n, rho] = MetricHandle(*H.metric_case(n, rho))
        return self._metrics[n, rho]

    def clean_run(self, lc, run=None):
        if run is not None:
            self._clean[lc.name] = run
        elif lc.name not in self._clean:
            self._clean[lc.name] = _Run(self, lc).stream_order()
        return self._clean[lc.name]


@pytest.fixture(scope="module")
def shared(spaces):
    return _Shared(spaces)


class _Run:
    """A case on the device: the finrom_hmc_state of hmc_cases.DeviceState and the call's own buffers (field mean, data, field,
    grad_field, vel, qoi_r, e_nn), every one with PAD sentinel elements behind its end."""

    def __init__(self, shared, lc, case=None, chain=None):
        import torch
        from bayesianinferencedl_amd import _ffi
        self.lc, self.pr, self.L = lc, F.problem(lc), _ffi.lib()
        pr = self.pr
        self.case = F.state(lc, pr) if case is None else case
        data = pr["data"]
        if chain is not None:
            self.case = H.chain_subset(self.case, chain)
            data = data[chain:chain + 1] if lc.per_sample else data
        self.data = data
        self.dev = H.DeviceState(self.case)
        Cn, n = self.case["C"], self.case["n"]
        self.rom, self.call, self.eng, self.mlp, self.sop = shared.rig(lc)
        self.fs, self.mh = shared.sampler(n), shared.metric(n, lc.rho) if lc.rho else None
        nan = lambda *sh: np.full(sh, np.nan)
        self.shape = {"fmean": (n,), "data": np.shape(data), "field": (Cn, n), "grad_field": (Cn, n), "vel": (Cn, n), "qoi_r": (Cn, 9), "e_nn": (Cn, 9)}
        init = {"fmean": pr["mean"], "data": data}
        self.up = {k: np.concatenate([np.asarray(init.get(k, nan(*sh)), dtype=np.float64).reshape(-1), nan(H.PAD)]) for k, sh in self.shape.items()}
        self.t = {k: torch.from_numpy(a.copy()).cuda() for k, a in self.up.items()}

    def reset(self):
        import torch
        for up, t in ((self.dev.up, self.dev.t), (self.up, self.t)):
            for k in t:
                t[k].copy_(torch.from_numpy(up[k]))
        self.rom.set_projection(self.lc.projection)

    def step(self, i):
        import torch
        x, st = self.t, torch.cuda.current_stream().cuda_stream
        q, e = (x["qoi_r"].data_ptr(), x["e_nn"].data_ptr()) if self.lc.outputs else (None, None)
        args = (self.eng._h, self.mlp._h, self.sop.ptr, self.fs._h, x["fmean"].data_ptr(), x["field"].data_ptr(), x["grad_field"].data_ptr(),
                C.byref(self.dev.st), i, x["data"].data_ptr(), 1 if self.lc.per_sample else 0, q, e)
        if self.mh is None:
            rc = self.L.finrom_hmc_leapfrog_field(*args, st)
        else:
            rc = self.L.finrom_hmc_leapfrog_field_metric(*args, self.mh._h, x["vel"].data_ptr(), st)
        self.sop.used_on(st)
        return rc

    def download(self):
        got = self.dev.download()
        got.update({"x_" + k: t.cpu().numpy() for k, t in self.t.items()})
        return got

    def body(self, got, name):
        if "x_" + name in got:
            return got["x_" + name][:-H.PAD].reshape(self.shape[name])
        return self.dev.body(got, name)

    def stream_order(self, watch=None):
        """Three steps from the case's start -> the download after each."""
        self.reset()
        out = []
        for i in range(F.STEPS):
            before = self.download() if watch else None
            assert self.step(i) == 0, self.L.finrom_last_error()
            out.append(self.download())
            if watch:
                watch(self, i, before, out[-1])
        return out

    def replayed(self):
        """One graph of the three steps, replayed twice after a reset -> the two downloads."""
        import torch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                        # the library's workspaces are sized before the capture
            self.reset()
            for i in range(F.STEPS):
                assert self.step(i) == 0
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(F.STEPS):
                assert self.step(i) == 0
        out = []
        for _ in range(2):
            self.reset()
            g.replay()
            out.append(self.download())
        return out


def _same_download(a, b):
    return [k for k in a if not _eq(a[k], b[k])] if a.keys() == b.keys() else ["keys"]


def _check_step(r, i, before, after):
    """Everything the module docstring lists for one step, from the downloads around it."""
    lc, pr, dev = r.lc, r.pr, r.dev
    Cn, n, U, mean = r.case["C"], r.case["n"], pr["U"], pr["mean"]
    where = (lc.name, "step", i)
    src, dst = "Kq%d" % (i & 1), "Kq%d" % ((i + 1) & 1)
    v, p = dev.body(before, src), dev.body(before, "P")
    w, p_new, dUq = dev.body(after, dst), dev.body(after, "P"), dev.body(after, "dUq")
    info, loss = dev.body(after, "info"), dev.body(after, "loss")
    field, grad = r.body(after, "field"), r.body(after, "grad_field")
    flagged = info != 0
    assert np.flatnonzero(flagged).tolist() == pr["chains"], (where, "flagged chains", info)
    ok = ~flagged
    # velocity: the longdouble M^-1 p, and the bits of finrom_metric_apply(INV) (the same row routine, the same coefficients)
    q = p
    if r.mh is not None:
        q = r.body(after, "vel")
        ref, scale = F.velocity(p, pr["metric"])
        assert _note("vel", _abs_ld(q, ref), H.METRIC_TOL * scale), where
        assert H.same_bits(q, r.mh.apply(p, "inv")), (where, "vel is not finrom_metric_apply's")
    # position: one fused multiply-add, flagged chains included (NaN where the poison is NaN)
    assert _eq(w, H.fma(F.EPS, q, v)), (where, "position update")
    if lc.poison == "nan":
        assert [np.flatnonzero(np.isnan(w[c])).tolist() for c in pr["chains"]] == [[F.nan_column(n, c)] for c in pr["chains"]], where
    # field: the plain kernel's bits on the written-back w; the longdouble product element by element
    assert _eq(field, r.fs.field(w, mean=mean)), (where, "field is not finrom_sampler_field's on the written-back w")
    fin = np.isfinite(w).all(axis=1)
    ref, scale = F.field_of(w[fin], U, mean)
    assert _note("field", _abs_ld(field[fin], ref), F.FIELD_TOL * scale), where
    assert np.isfinite(field[ok]).all() and field[ok].min() > 0
    # value and gradient: a plain finrom_romml_grad at the device's field, bit for bit; the float64 reference by the rule
    plain = r.call(field, r.data)
    assert np.array_equal(plain["info"], info), (where, plain["info"], info)
    pairs = [("loss", loss, plain["loss"]), ("grad_field", grad, plain["grad"])]
    if lc.outputs:
        pairs += [("qoi_r", r.body(after, "qoi_r"), plain["qoi_r"]), ("e_nn", r.body(after, "e_nn"), plain["e_NN"])]
    else:
        assert all(H.same_bits(after["x_" + k], r.up[k]) for k in ("qoi_r", "e_nn")), (where, "a NULL output's neighbour was written")
    for name, got, want in pairs:
        assert H.same_bits(got[ok], want[ok]), (where, name, "is not the plain call's")
    idx = [s for s in K.compared_samples(Cn) if ok[s]]
    idx = idx if len(idx) <= 4 else idx[:2] + idx[-2:]               # (both ends: beyond 64 chains, two of the second launch)
    row = F.fused_row(lc)
    prob, phi, ro = K.oracle_rig(row.m, row.r, row.n_obs)
    model = K.fused_model(row)
    refs = {net: [K.romml_ref(ro, model, field[s], r.data[s] if lc.per_sample else r.data, net) for s in idx] for net in ("f64", "f32")}
    for qty, got in [("loss", loss), ("grad", grad)] + ([("e_nn", r.body(after, "e_nn"))] if lc.outputs else []):
        M._check("leapfrog-field", f"{lc.name}-step{i}", qty, got[idx], np.array([x[qty] for x in refs["f32"]]), np.array([x[qty] for x in refs["f64"]]))
    # momentum, unflagged chains: dU = fma(c_lik, g_v, w) on the plain pullback's g_v, p' = fma(-eps, dU, p)
    assert np.isfinite(grad[ok]).all()
    g_v = r.fs.pullback(np.where(ok[:, None], grad, 0.0))
    assert H.same_bits(dUq[ok], H.fma(F.C_LIK, g_v[ok], w[ok])), (where, "dU")
    ref, gscale = F.pullback_of(grad[ok], U)
    assert _note("dU", _abs_ld(dUq[ok], w[ok].astype(H.LD) + H.LD(F.C_LIK) * ref), F.FIELD_TOL * (np.abs(w[ok]) + F.C_LIK * gscale)), where
    assert H.same_bits(p_new[ok], H.fma(-F.EPS, dUq[ok], p[ok])), (where, "momentum update")
    # flagged chains: dU exactly zero, the momentum's bits kept
    assert not dUq[flagged].any() and not np.isnan(dUq[flagged]).any(), (where, "a flagged chain's dU")
    assert H.same_bits(p_new[flagged], p[flagged]), (where, "a flagged chain's momentum moved")
    # what the step may not touch, and every buffer's sentinels
    written = {dst, "x_field", "x_grad_field"} | set(OUTPUTS) | ({"x_vel"} if r.mh is not None else set()) | \
              ({"x_qoi_r", "x_e_nn"} if lc.outputs else set())
    for name in after:
        if name not in written:
            assert H.same_bits(after[name], before[name]), (where, name, "changed")
        else:
            up = r.up[name[2:]] if name.startswith("x_") else dev.up[name]
            assert H.same_bits(after[name][-H.PAD:], up[-H.PAD:]), (where, name, "padding")


@pytest.mark.parametrize("lc", F.CLEAN, ids=lambda c: c.name)
def test_three_steps_against_the_reference_and_replay_bit_for_bit(shared, lc):
    """Every clean case of the table: the checks of _check_step after each of three steps (no chain flagged), a second run in
    stream order with the same bits, and one captured graph of the three steps, replayed twice after a reset, with the bits of
    stream order (the arrival counters are back at zero after every launch)."""
    r = _Run(shared, lc)
    first = shared.clean_run(lc, r.stream_order(_check_step))
    assert _same_download(first[-1], r.stream_order()[-1]) == [], lc.name
    for snap in r.replayed():
        assert _same_download(first[-1], snap) == [], lc.name
    print("worst error / allowance:", WORST)


@pytest.mark.parametrize("lc", F.POISONED, ids=lambda c: c.name)
def test_flagged_chains_keep_their_momentum_and_stay_in_their_rows(shared, lc):
    """A first, a middle and a last chain poisoned (C = 65, 70: the last behind index 64, in the second launch with its re-based
    tail pointers): info != 0 for exactly these on all three steps, dU = 0, the momentum's bits kept, the position still moved by
    the rule (_check_step); every other chain's position, momentum, dU, loss, field, gradient and velocity bitwise those of the
    clean case, so nothing of the NaN reaches another chain; the replayed graph gives the bits of stream order."""
    r = _Run(shared, lc)
    dirty, clean = r.stream_order(_check_step), shared.clean_run(F.clean_of(lc))
    keep = r.pr["clean"]
    names = ["Kq0", "Kq1", "P", "dUq", "loss", "info", "field", "grad_field"] + (["vel"] if lc.rho else []) + (["qoi_r", "e_nn"] if lc.outputs else [])
    for i in range(F.STEPS):
        for name in names:
            a, b = r.body(dirty[i], name)[keep], r.body(clean[i], name)[keep]
            assert np.isfinite(a).all() and H.same_bits(a, b), (lc.name, "step", i, name, "of a clean chain differs from the clean run")
    for snap in r.replayed():
        assert _same_download(dirty[-1], snap) == [], lc.name


def _among_others(lc, keep):
    """The case with every chain but `keep` started elsewhere."""
    case = F.state(lc)
    rng = np.random.default_rng([lc.C, 99])
    other = np.ones(lc.C, bool)
    other[keep] = False
    case["Kq0"][other] = 0.3 * rng.standard_normal((int(other.sum()), case["n"]))
    case["P"][other] = rng.standard_normal((int(other.sum()), case["n"]))
    return case


@pytest.mark.parametrize("name,chains", [("m12-C8", (3,)), ("m4-C70", (3, 66)), ("m4-C65-rho17", (2, 64))])
def test_a_chain_does_not_depend_on_its_batch(shared, name, chains):
    """Stepped alone (C = 1), a chain has the bits it has inside its batch: for m12-C8 (finrom_romml_grad's one-sample form either
    way) every output of all three steps.  Beyond 64 chains the batch takes finrom_romml_grad's batched form and a chain alone the
    other one, whose value and gradient agree only to tolerance, so for a chain of the first launch (RT = 4) and one behind index 64
    (RT = 2, RT = 1) the step is taken apart at that call: alone, the position, the velocity and the field of step 0 are the
    batch's; on every step the plain pullback of the chain's row of the BATCH's grad_field, launched alone (RT = 1), gives the
    batch's dU and momentum through the two exact fused multiply-adds; and every output of all three steps is the same at its own
    place among OTHER neighbours."""
    lc = F.BY_NAME[name]
    batch = shared.clean_run(lc)
    full = _Run(shared, lc)
    per_chain = ["Kq0", "Kq1", "P", "dUq", "loss", "info", "field", "grad_field"] + (["vel"] if lc.rho else [])
    for c in chains:
        one = _Run(shared, lc, chain=c)
        alone = one.stream_order()
        for i in range(F.STEPS if lc.C <= 64 else 1):
            for k in per_chain if lc.C <= 64 else ["Kq1", "field"] + (["vel"] if lc.rho else []):
                assert H.same_bits(one.body(alone[i], k)[0], full.body(batch[i], k)[c]), (name, c, "step", i, k)
        if lc.C > 64:
            p = full.pr["p0"][c]
            for i in range(F.STEPS):
                w, dUq = full.body(batch[i], "Kq%d" % ((i + 1) & 1))[c], full.body(batch[i], "dUq")[c]
                g_v = full.fs.pullback(full.body(batch[i], "grad_field")[c:c + 1])[0]
                assert H.same_bits(dUq, H.fma(F.C_LIK, g_v, w)), (name, c, "step", i, "dU from the pullback of the chain alone")
                assert H.same_bits(full.body(batch[i], "P")[c], H.fma(-F.EPS, dUq, p)), (name, c, "step", i, "momentum")
                p = full.body(batch[i], "P")[c]
    if lc.C > 64:
        mixed_run = _Run(shared, lc, case=_among_others(lc, list(chains)))
        mixed = mixed_run.stream_order()
        for i in range(F.STEPS):
            for k in per_chain:
                a, b = mixed_run.body(mixed[i], k), full.body(batch[i], k)
                assert H.same_bits(a[list(chains)], b[list(chains)]), (name, "step", i, k)
            assert not H.same_bits(mixed_run.body(mixed[i], "P")[1], full.body(batch[i], "P")[1])        # (the neighbours did change)


def test_the_theta_carry_does_not_survive_a_whitened_step(spaces, shared):
    """On ONE error-model handle: plain step 0 (finrom_hmc_leapfrog leaves its theta carry), one finrom_hmc_leapfrog_field step on
    the same buffers through a second finrom_hmc_state with c_pri = 1 (it moves Kq[1] and P, so the carried averages are stale),
    then plain step 1: its moved field and network output are bitwise those of a fresh handle at the same inputs, value and
    gradient within the rule of the float64 reference on both sides."""
    import torch
    from bayesianinferencedl_amd import _ffi
    c = K.FUSED_BY_NAME["one-staged-ref"]
    n = K.MESH_N[c.m]
    lf = M._Leap(spaces, c)
    lf.reset()
    lf.step(0)
    torch.cuda.synchronize()
    p0 = M._np(lf.P)
    st2 = _ffi.HmcState.from_buffer_copy(lf.st)
    st2.c_pri = 1.0                                  # (c_lik stays the plain form's 400: the momentum moves as far as a plain step moves it)
    fs, fmean = shared.sampler(n), M._dev(F.field_mean(n) + 1.0)
    field, grad_field = torch.zeros_like(lf.P), torch.zeros_like(lf.P)
    stream = torch.cuda.current_stream().cuda_stream
    rc = lf.L.finrom_hmc_leapfrog_field(lf.eng._h, lf.mlp._h, lf.sop.ptr, fs._h, fmean.data_ptr(), field.data_ptr(), grad_field.data_ptr(),
                                        C.byref(st2), 0, lf.data.data_ptr(), 1 if c.per_sample else 0, None, None, stream)
    _ffi.check(rc, "finrom_hmc_leapfrog_field")
    lf.sop.used_on(stream)
    torch.cuda.synchronize()
    k1, p1 = M._np(lf.Kq[1]), M._np(lf.P)
    assert (M._np(lf.info) == 0).all() and M._np(field).min() > 0 and np.isfinite(p1).all()
    assert np.max(np.abs(p1 - p0)) > 1e-3 * np.max(np.abs(p0)), "the whitened step did not move the momentum"
    lf.step(1)
    torch.cuda.synchronize()
    fresh = M._Leap(spaces, c)
    fresh.reset(); fresh.Kq[1].copy_(M._dev(k1)); fresh.P.copy_(M._dev(p1))
    fresh.step(1)
    torch.cuda.synchronize()
    moved = M._np(lf.Kq[0])
    assert np.array_equal(moved, M._fma(lf.EPS, p1, k1)) and np.array_equal(moved, M._np(fresh.Kq[0]))
    assert np.array_equal(M._np(lf.e[1]), M._np(fresh.e[1])) and (M._np(lf.info) == 0).all()
    prob, phi, ro = K.oracle_rig(c.m, c.r, c.n_obs)
    model = K.fused_model(c)
    idx = list(range(c.S))
    refs = {net: [K.romml_ref(ro, model, moved[s], lf.data_np[s] if c.per_sample else lf.data_np, net) for s in idx] for net in ("f64", "f32")}
    for qty, a, b in (("grad", M._np(lf.grad[1]), M._np(fresh.grad[1])), ("loss", M._np(lf.loss), M._np(fresh.loss))):
        r64, r32 = np.array([r[qty] for r in refs["f64"]]), np.array([r[qty] for r in refs["f32"]])
        M._check("leapfrog", "after-a-whitened-step", qty, a[idx], r32, r64)
        M._check("leapfrog", "after-a-whitened-step-fresh", qty, b[idx], r32, r64)


# ---- the edges of the entry points -----------------------------------------------------------------------------------------------
def test_no_chains_no_launch(shared):
    """C = 0: both forms return 0 and touch nothing."""
    lc = F.BY_NAME["m4-C5-rho1"]
    n = K.MESH_N[lc.m]
    case = H.begin_case(n, 0, 1)
    case["c_pri"] = 1.0
    r = _Run(shared, lc, case=case)
    r.reset()
    before = r.download()
    assert r.step(0) == 0
    r.mh = None
    assert r.step(1) == 0
    assert _same_download(before, r.download()) == []


def test_entry_points_check_their_handles_sizes(shared):
    """A metric of another n, a prior of another n: FINROM_ERR_ARG with the documented text, the state untouched."""
    lc = F.BY_NAME["m4-C5-rho1"]
    r = _Run(shared, lc)
    r.reset()
    before = r.download()
    mine, r.mh = r.mh, shared.metric(777, 3)
    assert r.step(0) == -1 and b"hmc_leapfrog_field_metric: n = 245 is not the metric's (777)" in r.L.finrom_last_error()
    r.mh, r.fs = mine, shared.sampler(777)
    assert r.step(0) == -1 and b"hmc_leapfrog_field: n = 245 is not the prior's (777) or the error model's input size (245)" in r.L.finrom_last_error()
    r.mh = None
    assert r.step(0) == -1 and b"hmc_leapfrog_field: n = 245 is not the prior's (777)" in r.L.finrom_last_error()
    r.dev.st.c_pri = 2.0
    r.fs = shared.sampler(245)
    assert r.step(0) == -1 and b"hmc_leapfrog_field: c_pri must be 1" in r.L.finrom_last_error()
    assert _same_download(before, r.download()) == []
