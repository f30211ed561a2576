"""The kernels of delayed-acceptance HMC driven directly through the C ABI on hand-made state: finrom_hmc_end_stage1 (csrc/hmc_kernels.hip)
against hmc_cases.ref_end -- the decision of finrom_hmc_end and nothing else; finrom_hmc_end_stage2 (csrc/hmc_da.hip) against
hmc_da_cases.ref_stage2, bit for bit, eleven roles per launch; finrom_hmc_draw_stage2 against philox.draw_block_stage2.  Every buffer a
kernel must not touch is compared bit for bit, the PAD sentinel elements behind every buffer included."""
import ctypes

import numpy as np
import pytest

import hmc_cases as H
import hmc_da_cases as D

pytestmark = pytest.mark.gpu


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _padded(a, dt):
    import torch
    up = np.concatenate([np.asarray(a, dtype=dt).reshape(-1), np.full(H.PAD, np.nan if dt is np.float64 else H.SENTINEL, dtype=dt)])
    return up, torch.from_numpy(up.copy()).cuda()


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 12, 64])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1597])
def test_stage1_is_the_decision_of_hmc_end_and_writes_nothing_else(n, C):
    """hmc_cases.end_base (chain c plays role c % 12), both parities of n_steps, *jt in 0, B - 1: ok1 is the reference's decision for
    every role; Uq within sum_tol(n) of its scale, +inf where the chain is flagged; every array of the state keeps its uploaded
    bits, padding included; finrom_hmc_end on the same state afterwards accepts exactly the chains ok1 names."""
    import torch
    base = H.end_base(n, C)
    ref = base["ref"]
    flagged = (base["info"] != 0) | ~(np.abs(ref["Uq"]) <= H.U_LIMIT)
    for n_steps, jt in ((3, 0), (4, H.B_BLOCK - 1), (4, 0), (3, H.B_BLOCK - 1)):
        case, _ = H.end_variant(base, n_steps, jt, 2, H.TRACE_ROWS)
        dev = H.DeviceState(case)
        up1, ok1_t = _padded(np.full(C, 77), np.int32)
        upq, Uq_t = _padded(np.full(C, np.nan), np.float64)
        assert dev.call("hmc_end_stage1", n_steps, ok1_t.data_ptr(), Uq_t.data_ptr()) == 0
        got = dev.download()
        dev.assert_bits(got, {})                                    # K, U, dU, accept, trace, jt, pt, every input, all padding
        ok1, Uq = ok1_t.cpu().numpy(), Uq_t.cpu().numpy()
        assert np.array_equal(ok1[-H.PAD:], up1[-H.PAD:]) and np.isnan(Uq[-H.PAD:]).all()
        ok1, Uq = ok1[:C], Uq[:C]
        where = (n, C, n_steps, jt)
        assert np.array_equal(ok1, ref["ok"].astype(np.int32)), (where, ok1, ref["ok"])
        assert np.all(Uq[flagged] == np.inf), (where, Uq[flagged])
        err = np.abs(Uq[~flagged].astype(H.LD) - ref["Uq"][~flagged]).astype(np.float64)
        assert np.all(err <= H.sum_tol(n) * ref["U_scale"][~flagged].astype(np.float64)), (where, err)
        assert dev.call("hmc_end", n_steps) == 0
        after = dev.download()
        assert np.array_equal(dev.body(after, "accept") - case["accept"], ok1.astype(np.int64)), where
        U = dev.body(after, "U")
        assert H.same_bits(U[ok1 != 0], Uq[ok1 != 0]) and H.same_bits(U[ok1 == 0], case["U"][ok1 == 0]), where
    torch.cuda.synchronize()


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------------
# n_obs, data per sample, n_steps, *jt, *pt, trace rows (0: NULL), correction given
VARIANTS = [(9, False, 3, 0, 6, H.TRACE_ROWS, True), (40, True, 4, 2, 2, 0, False), (9, True, 4, 1, 1, H.TRACE_ROWS, False),
            (40, False, 3, 2, 7, 0, True)]


def _canonical_nan(got):
    for name in ("cand_loss_f", "correction"):                       # NaN compared as NaN
        if name in got:
            got[name] = np.where(np.isnan(got[name]), np.nan, got[name])
    return got


@pytest.mark.parametrize("C", [1, 11, 22, 64])
@pytest.mark.parametrize("n", [1, 256, 257, 1597])
def test_stage2_has_the_bits_of_its_statement(n, C):
    """Chain c plays role c % 11 of hmc_da_cases.ROLES (all eleven at C >= 11): clear accepts and rejects, log u2 one ulp below the
    threshold D - Dq (accept) and on it (reject: the comparison is strict), a chain stage 1 stopped with a log u2 that would
    accept, a flagged solve, NaN / +inf / an overflowing value among the observables, a stopped chain whose solve is flagged, a
    stopped chain with Uq = +inf.  n_obs in 9, 40; shared and per-sample data; trace and correction given and NULL; both
    parities of n_steps; *pt > 0.  K, U, dU, D, loss_f, cand_loss_f, the correction row, accept, accept1, the trace row, jt and pt
    have the bits of ref_stage2; everything else, padding included, its uploaded bits."""
    for n_obs, per_sample, n_steps, jt, pt, rows, corr in VARIANTS:
        s, a, want, want_da, ref = D.stage2_case(n, C, n_obs, per_sample, n_steps, jt, pt, rows, corr)
        dev, da = H.DeviceState(s), D.DeviceDA(a)
        assert dev.call("hmc_end_stage2", n_steps, ctypes.byref(da.desc)) == 0
        got, got_da = dev.download(), _canonical_nan(da.download())
        where = (n, C, n_obs, per_sample, n_steps, jt, pt, rows, corr)
        assert np.array_equal(dev.body(got, "accept") - s["accept"], ref["ok"].astype(np.int64)), (where, "decisions")
        try:
            dev.assert_bits(got, want)
            da.assert_bits(got_da, want_da)
        except AssertionError as exc:
            raise AssertionError(f"{where}: {exc}") from None


def test_stage2_checks_its_arguments_and_does_nothing_without_chains():
    """FINROM_ERR_ARG with a message, nothing launched: a null descriptor, n_obs < 1, n_steps < 0, each required pointer of the
    descriptor NULL in turn (correction may be).  C == 0: 0, and no counter moves."""
    from bayesianinferencedl_amd import _ffi
    lib = _ffi.lib()
    s, a, *_ = D.stage2_case(65, 3, 9, False, 3, 0, 2, H.TRACE_ROWS, True)
    dev, da = H.DeviceState(s), D.DeviceDA(a)
    assert dev.call("hmc_end_stage2", 3, None) == -1 and b"hmc_end_stage2: null descriptor" in lib.finrom_last_error()
    assert dev.call("hmc_end_stage2", -1, ctypes.byref(da.desc)) == -1 and b"hmc_end_stage2: n_steps < 0" in lib.finrom_last_error()
    assert dev.call("hmc_end_stage1", -1, da.t["ok1"].data_ptr(), da.t["Uq"].data_ptr()) == -1
    assert b"hmc_end_stage1: n_steps < 0" in lib.finrom_last_error()
    assert dev.call("hmc_end_stage1", 3, None, da.t["Uq"].data_ptr()) == -1 and b"null ok1 or Uq" in lib.finrom_last_error()
    assert dev.call("hmc_end_stage1", 3, da.t["ok1"].data_ptr(), None) == -1
    bad = _ffi.HmcDa.from_buffer_copy(da.desc)
    bad.n_obs = 0
    assert dev.call("hmc_end_stage2", 3, ctypes.byref(bad)) == -1 and b"n_obs < 1" in lib.finrom_last_error()
    for name, _ in D.DA_ARRAYS:
        bad = _ffi.HmcDa.from_buffer_copy(da.desc)
        setattr(bad, name, None)
        rc = dev.call("hmc_end_stage2", 3, ctypes.byref(bad))
        if name == "correction":
            continue                                                # (legal: checked after the loop, it ran)
        assert rc == -1 and b"null pointer in finrom_hmc_da" in lib.finrom_last_error(), name
    got = dev.download()
    assert dev.body(got, "jt") == 1 and dev.body(got, "pt") == 3     # the one legal call above, without a correction table
    # no chains
    s0 = H.begin_case(65, 0, 2)
    dev0 = H.DeviceState(s0)
    assert dev0.call("hmc_end_stage2", 3, ctypes.byref(da.desc)) == 0
    assert dev0.call("hmc_end_stage1", 3, None, None) == 0
    got0 = dev0.download()
    dev0.assert_bits(got0, {})
    assert dev0.body(got0, "jt") == 2 and dev0.body(got0, "pt") == 4


# ---- the second uniform ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 2 ** 33 + 5])
@pytest.mark.parametrize("B,C", [(3, 5), (7, 64), (1, 1)])
def test_draw_stage2_matches_its_numpy_statement(B, C, first):
    """lu2 within 1e-13 absolute of philox.draw_block_stage2 (tests/test_gpu_hmc_rng.py's bound for lu), a seed above 2^32 among the
    chains, first_proposal beyond 2^33; finite and <= 0; the padding intact; B = 0 launches nothing."""
    import torch
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.bayesian_inference import philox
    lib = _ffi.lib()
    seeds = np.array([(2 ** 32 + 11) * (c + 1) + 3 for c in range(C)], dtype=np.uint64)
    seeds_t = torch.from_numpy(seeds.view(np.int64).copy()).cuda()
    up, lu2_t = _padded(np.full((B, C), 5.0), np.float64)
    assert lib.finrom_hmc_draw_stage2(seeds_t.data_ptr(), C, first, B, lu2_t.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got = lu2_t.cpu().numpy()
    assert np.isnan(got[-H.PAD:]).all()
    lu2 = got[:-H.PAD].reshape(B, C)
    want = philox.draw_block_stage2(seeds, first, B)
    assert np.isfinite(lu2).all() and (lu2 <= 0).all()
    assert np.max(np.abs(lu2 - want)) <= 1e-13, np.max(np.abs(lu2 - want))
    assert lib.finrom_hmc_draw_stage2(seeds_t.data_ptr(), C, first, 0, lu2_t.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert H.same_bits(lu2_t.cpu().numpy(), got)
