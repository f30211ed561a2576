"""finrom_hmc_drift and finrom_hmc_kick (csrc/hmc_model.hip) through the C ABI against the NumPy statement of
tests/hmc_model_cases.py (which tests/test_hmc_model_host.py walks against hmc.run_chains): the position update and, with a
field-space gradient, dUq and the momentum bit for bit against exact fused multiply-adds; theta and the gradient through a map A
within the bounds of their documented summation orders; flagged chains; everything the calls may not touch, PAD sentinel elements
behind every buffer included; a chain's independence of its batch; a replayed graph against stream order; the edges of the entry
points.  Shapes: n below, at and above one workgroup's 256 threads and at several blocks, C = 1, 3, 13, P = 1, 9, 16, both
parities of `step`.

Worst error / allowance observed on an MI355X (each test prints its own): theta 0.10, the mapped gradient 0.50, dUq 0.97 and the
momentum 0.99 -- the last two allowances are one rounding of the result where the gradient's share is small, which a correctly
rounded fused multiply-add may use in full and cannot exceed."""
import numpy as np
import pytest

import hmc_cases as H
import hmc_model_cases as M

pytestmark = pytest.mark.gpu
SIZES = (1, 255, 256, 257, 600)
CHAINS = (1, 3, 13)
MAPS = (1, 9, 16)


def _pad(a, dtype=np.float64):
    """(device tensor of a with PAD sentinels behind it, what was uploaded)."""
    import torch
    up = np.concatenate([np.asarray(a, dtype=dtype).reshape(-1), np.full(H.PAD, np.nan)])
    return torch.from_numpy(up.copy()).cuda(), up


def _body(t, shape):
    return t.cpu().numpy()[:-H.PAD].reshape(shape)


def _kept(t, up):
    return H.same_bits(t.cpu().numpy(), up)


def _flags(C):
    return ((1, 2), (2, -1)) if C >= 3 else ()


def _note(what, err, tol):
    with np.errstate(all="ignore"):
        worst = float(np.nanmax(np.where(tol > 0, np.abs(err) / tol, 0.0)))
    print(f"{what}: worst error / allowance {worst:.3g}")
    return bool(np.all(np.abs(err) <= tol))


@pytest.mark.parametrize("C", CHAINS)
@pytest.mark.parametrize("n", SIZES)
def test_drift(n, C):
    """k' = fma(eps, p, k) bit for bit into the buffer `step` chooses, the other one and every other array untouched; with a map
    (P = 1, 9, 16; theta0 NULL and given) theta within sum_tol(n) of |theta0| + |A| |k'|; A, theta0 and the padding keep their bits."""
    import torch
    for step in (0, 1):
        for P in (None,) + MAPS:
            for with_t0 in ((False,) if P is None else (False, True)):
                case = M.step_case(n, C, step)
                dev = H.DeviceState(case)
                k, out = case["Kq%d" % (step & 1)], "Kq%d" % ((step + 1) & 1)
                if P is None:
                    assert dev.call("hmc_drift", step, None, None, 0, None) == 0
                    kq, theta, scale = M.ref_drift(k, case["P"], case["eps"])
                else:
                    A, t0 = M.map_case(n, C, P)[:2]
                    (A_t, A_up), (t0_t, t0_up), (th_t, _) = _pad(A), _pad(t0), _pad(np.full((C, P), np.nan))
                    assert dev.call("hmc_drift", step, A_t.data_ptr(), t0_t.data_ptr() if with_t0 else None, P, th_t.data_ptr()) == 0
                    kq, theta, scale = M.ref_drift(k, case["P"], case["eps"], A, t0 if with_t0 else None)
                got = dev.download()
                dev.assert_bits(got, {out: kq})
                if P is not None:
                    torch.cuda.synchronize()
                    assert _kept(A_t, A_up) and _kept(t0_t, t0_up) and np.isnan(th_t.cpu().numpy()[-H.PAD:]).all()
                    err = (_body(th_t, (C, P)).astype(H.LD) - theta).astype(np.float64)
                    assert _note(f"theta n={n} C={C} P={P} step={step} theta0={with_t0}", err, H.sum_tol(n) * scale), (n, C, P, step)


@pytest.mark.parametrize("C", CHAINS)
@pytest.mark.parametrize("n", SIZES)
def test_kick_with_a_field_space_gradient(n, C):
    """dUq = fma(c_lik / c_pri, g, k' - mean) and P = fma(-(eps c_pri), dUq, P) bit for bit; chains flagged 2 and -1 (C >= 3; C = 1:
    a run of its own) get dUq = 0 exactly and keep their momentum's bits; a NaN in an unflagged chain's gradient reaches dUq and P;
    grad_out, when given, is the gradient's bits; nothing else moves, both position buffers included."""
    import torch
    runs = [_flags(C)] + ([((0, 2),)] if C == 1 else [])
    for step in (0, 1):
        for flags in runs:
            for want_out in (False, True):
                case = M.step_case(n, C, step, flags=flags)
                kq = case["Kq%d" % ((step + 1) & 1)] = 1.0 + 0.3 * np.random.default_rng([n, C, step]).standard_normal((C, n))
                g = M.map_case(n, C, 9)[3]
                if case["info"][0] == 0:
                    g[0, n // 2] = np.nan
                dev = H.DeviceState(case)
                (g_t, g_up), (o_t, _) = _pad(g), _pad(np.full((C, n), np.nan))
                assert dev.call("hmc_kick", step, g_t.data_ptr(), None, None, 0, o_t.data_ptr() if want_out else None) == 0
                dU, Pn = M.ref_kick(kq, case["mean"], case["P"], case["info"], case["eps"], case["c_lik"], case["c_pri"], g)
                got = dev.download()
                dev.assert_bits(got, {"dUq": dU, "P": Pn})
                for c, _ in flags:
                    assert not dev.body(got, "dUq")[c].any() and H.same_bits(dev.body(got, "P")[c], case["P"][c])
                if case["info"][0] == 0:
                    assert np.isnan(dev.body(got, "dUq")[0, n // 2]) and np.isnan(dev.body(got, "P")[0, n // 2])
                    assert np.isnan(dev.body(got, "dUq")[0]).sum() == 1
                torch.cuda.synchronize()
                assert _kept(g_t, g_up) and np.isnan(o_t.cpu().numpy()[-H.PAD:]).all()
                assert H.same_bits(_body(o_t, (C, n)), g) if want_out else np.isnan(o_t.cpu().numpy()).all()


@pytest.mark.parametrize("C", CHAINS)
@pytest.mark.parametrize("n", SIZES)
def test_kick_with_a_mapped_gradient(n, C):
    """The gradient as sum_p g_theta[c, p] A[p, i] (P = 1, 9, 16) within (P + 1) 2^-53 of sum_p |g_theta A| (read from grad_out), dUq
    and P within that allowance carried through their two fused multiply-adds (hmc_model_cases.kick_bounds); flagged chains exact;
    nothing else moves."""
    import torch
    for step in (0, 1):
        for P in MAPS:
            flags = _flags(C)
            case = M.step_case(n, C, step, flags=flags)
            kq = case["Kq%d" % ((step + 1) & 1)] = 1.0 + 0.3 * np.random.default_rng([n, C, step]).standard_normal((C, n))
            A, _, g_theta, _ = M.map_case(n, C, P)
            dev = H.DeviceState(case)
            (A_t, A_up), (gt_t, gt_up), (o_t, _) = _pad(A), _pad(g_theta), _pad(np.full((C, n), np.nan))
            assert dev.call("hmc_kick", step, None, gt_t.data_ptr(), A_t.data_ptr(), P, o_t.data_ptr()) == 0
            gL, scale = M.map_gradient(g_theta, A)
            coef, ec = case["c_lik"] / case["c_pri"], case["eps"] * case["c_pri"]
            flagged = (case["info"] != 0)[:, None]
            dU_ref = np.where(flagged, 0, (kq - case["mean"]).astype(H.LD) + H.LD(coef) * gL)      # (k' - mean rounded to double first, as documented)
            P_ref = np.where(flagged, case["P"].astype(H.LD), case["P"].astype(H.LD) - H.LD(ec) * dU_ref)
            tol_g, tol_dU, tol_P = M.kick_bounds(P, scale, dU_ref.astype(np.float64), P_ref.astype(np.float64), case["eps"], case["c_lik"], case["c_pri"])
            got = dev.download()
            dev.assert_bits(got, {}, skip=("dUq", "P"))
            torch.cuda.synchronize()
            tag = f"n={n} C={C} P={P} step={step}"
            assert _note("gradient " + tag, (_body(o_t, (C, n)).astype(H.LD) - gL).astype(np.float64), tol_g), tag
            assert _note("dUq " + tag, (dev.body(got, "dUq").astype(H.LD) - dU_ref).astype(np.float64), tol_dU), tag
            assert _note("P " + tag, (dev.body(got, "P").astype(H.LD) - P_ref).astype(np.float64), tol_P), tag
            for c, _ in flags:
                assert not dev.body(got, "dUq")[c].any() and H.same_bits(dev.body(got, "P")[c], case["P"][c])
            ok = case["info"] == 0                                           # the momentum from the device's own dUq: one fma, bit for bit
            assert H.same_bits(dev.body(got, "P")[ok], H.fma(-ec, dev.body(got, "dUq")[ok], case["P"][ok])), tag
            for name in ("dUq", "P"):
                assert H.same_bits(got[name][-H.PAD:], dev.up[name][-H.PAD:]), name
            assert _kept(A_t, A_up) and _kept(gt_t, gt_up) and np.isnan(o_t.cpu().numpy()[-H.PAD:]).all()


def _one_step(case, step, A, t0, g_theta, grad):
    """Drift (with the map) and both kicks' outputs of one state -> dict of downloads: Kq', theta, and (dUq, P) of the kick with
    grad, then -- from the same momentum -- of the kick with (g_theta, A)."""
    C, n, P = case["C"], case["n"], A.shape[0]
    out = {}
    dev = H.DeviceState(case)
    (A_t, _), (t0_t, _), (th_t, _), (g_t, _), (gt_t, _) = _pad(A), _pad(t0), _pad(np.full((C, P), np.nan)), _pad(grad), _pad(g_theta)
    assert dev.call("hmc_drift", step, A_t.data_ptr(), t0_t.data_ptr(), P, th_t.data_ptr()) == 0
    assert dev.call("hmc_kick", step, g_t.data_ptr(), None, None, 0, None) == 0
    got = dev.download()
    out.update(kq=dev.body(got, "Kq%d" % ((step + 1) & 1)), theta=_body(th_t, (C, P)), dU1=dev.body(got, "dUq"), P1=dev.body(got, "P"))
    assert dev.call("hmc_kick", step, None, gt_t.data_ptr(), A_t.data_ptr(), P, None) == 0
    got = dev.download()
    out.update(dU2=dev.body(got, "dUq"), P2=dev.body(got, "P"))
    return out


@pytest.mark.parametrize("n,C,P", [(257, 13, 9), (600, 3, 16)])
def test_a_chain_alone_has_the_bits_it_has_in_the_batch(n, C, P):
    """Row independence: every output row of a chain run alone (C = 1) is bitwise its row inside the batch -- theta's fixed
    summation order depends on n alone."""
    case = M.step_case(n, C, 1, flags=_flags(C))
    A, t0, g_theta, grad = M.map_case(n, C, P)
    full = _one_step(case, 1, A, t0, g_theta, grad)
    for c in (0, 1, C - 1):
        solo = _one_step(H.chain_subset(case, c), 1, A, t0, g_theta[c:c + 1], grad[c:c + 1])
        for name, a in full.items():
            assert H.same_bits(solo[name][0], a[c]), (name, c)


def test_a_replayed_graph_gives_the_bits_of_stream_order():
    """Drift with a map, kick with the mapped gradient, two steps (both parities), captured once and replayed twice from the
    restored state: the downloads of stream order bit for bit.  Neither call allocates, so the capture needs no warm-up of theirs."""
    import torch
    n, C, P = 600, 13, 9
    case = M.step_case(n, C, 0, flags=_flags(C))
    A, t0, g_theta, _ = M.map_case(n, C, P)
    dev = H.DeviceState(case)
    (A_t, _), (t0_t, _), (th_t, th_up), (gt_t, _) = _pad(A), _pad(t0), _pad(np.full((C, P), np.nan)), _pad(g_theta)
    start = {k: t.clone() for k, t in dev.t.items()}

    def reset():
        for k, t in dev.t.items():
            t.copy_(start[k])
        th_t.copy_(torch.from_numpy(th_up).cuda())

    def steps():
        for step in (0, 1):
            assert dev.call("hmc_drift", step, A_t.data_ptr(), t0_t.data_ptr(), P, th_t.data_ptr()) == 0
            assert dev.call("hmc_kick", step, None, gt_t.data_ptr(), A_t.data_ptr(), P, None) == 0

    def snap():
        d = dev.download()
        d["theta"] = th_t.cpu().numpy()
        return d
    steps()
    want = snap()
    assert not np.isnan(dev.body(want, "Kq0")).any() and not np.isnan(want["theta"][:-H.PAD]).any()
    reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        steps()
    for _ in range(2):
        reset()
        g.replay()
        got = snap()
        assert [k for k in want if not H.same_bits(got[k], want[k])] == []


def test_no_chains_no_launch():
    """C = 0: both calls return 0 and touch nothing."""
    case = M.step_case(65, 0, 0)
    dev = H.DeviceState(case)
    (A_t, A_up), (th_t, th_up) = _pad(np.ones((9, 65))), _pad(np.zeros(0))
    assert dev.call("hmc_drift", 0, A_t.data_ptr(), None, 9, th_t.data_ptr()) == 0
    assert dev.call("hmc_kick", 0, None, th_t.data_ptr(), A_t.data_ptr(), 9, None) == 0
    dev.assert_bits(dev.download(), {})
    assert _kept(A_t, A_up) and _kept(th_t, th_up)


def test_entry_points_check_their_arguments():
    """Null state, P = 0, P = 17, both or neither of grad and g_theta, g_theta without A, a map without theta_out, step < 0:
    FINROM_ERR_ARG with a message, nothing launched (every buffer keeps its bits)."""
    from bayesianinferencedl_amd import _ffi
    lib = _ffi.lib()
    err = lib.finrom_last_error
    case = M.step_case(65, 3, 0)
    dev = H.DeviceState(case)
    (A_t, A_up), (x_t, x_up) = _pad(np.ones((16, 65))), _pad(np.ones((3, 65)))
    a, x = A_t.data_ptr(), x_t.data_ptr()
    assert lib.finrom_hmc_drift(None, 0, None, None, 0, None, None) == -1 and b"hmc_drift: null field" in err()
    assert lib.finrom_hmc_kick(None, 0, x, None, None, 0, None, None) == -1 and b"hmc_kick: null field" in err()
    for P in (0, 17):
        assert dev.call("hmc_drift", 0, a, None, P, x) == -1 and b"hmc_drift: P = %d is outside 1 .. 16" % P in err()
        assert dev.call("hmc_kick", 0, None, x, a, P, None) == -1 and b"hmc_kick: P = %d is outside 1 .. 16" % P in err()
    assert dev.call("hmc_drift", 0, a, None, 9, None) == -1 and b"hmc_drift: A without theta_out" in err()
    assert dev.call("hmc_drift", -1, None, None, 0, None) == -1 and b"hmc_drift: step < 0" in err()
    assert dev.call("hmc_kick", -1, x, None, None, 0, None) == -1 and b"hmc_kick: step < 0" in err()
    assert dev.call("hmc_kick", 0, x, x, a, 9, None) == -1 and b"exactly one of grad and g_theta" in err()
    assert dev.call("hmc_kick", 0, None, None, a, 9, None) == -1 and b"exactly one of grad and g_theta" in err()
    assert dev.call("hmc_kick", 0, None, x, None, 9, None) == -1 and b"hmc_kick: g_theta without A" in err()
    dev.assert_bits(dev.download(), {})
    assert _kept(A_t, A_up) and _kept(x_t, x_up)
