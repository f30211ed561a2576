"""The reduced LSPG solve (finrom_rom_solve) and its adjoint gradient (finrom_rom_grad) on the device against the extended-precision
yardstick of tests/rom_lspg_cases.py, form by form as csrc/api_rom.hip dispatches them (rom_solve_impl, rom_project,
launch_rom_proj; finrom_rom_grad).

Allowance, per batch and per quantity (qoi_r, Phi w_r, J, g): d_host = the largest relative deviation of host64 (plain fp64 normal
equations, cho_factor / cho_solve) from the yardstick over the checked samples; the device must be within max(8 d_host, 1e-12).
Device and host are two fp64 evaluations of the same normal equations: their errors scale alike with cond(A_r) (1e5 .. 2e8 here)
and differ by the order of sums.  8 d_host <= 1e-10 is a condition on the inputs, held on the host by tests/test_rom_lspg_host.py
for exactly these batches.  Yardsticks: the 80-bit normal equations on 8 samples of a batch (first and last of a workgroup of four,
one per wave of a workgroup in the middle, the ragged tail), fp64 Householder QR on EVERY sample.  With the state returned, the solve
kernels are also held to the backward error of w_r on the device's own A_r, B_r -- independent of conditioning -- against
cho_solve's on the same matrices: 8 x, floor r 2^-53.
Every device deviation also stays under 1e-10.

Inputs: the existing tests' -- the parity basis (U(0.1, 3.5) snapshots), log-uniform theta in [0.1, 10]^9, narrowed to [0.2, 5]^9
for the cases whose host deviation leaves less than half of the 1e-10 free (rom_lspg_cases.Case.NARROW); the benchmark-recipe basis
with mirror-symmetric theta in [0.1, 10] for the half and short lists; m = 12 wherever a form needs 64 k-steps, m = 4 for r <= 16.
Every test prints its measured device and host deviations and records them in its docstring."""
import contextlib
import os

import numpy as np
import pytest
import scipy.linalg as sla

import rom_lspg_cases as Y

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def models(spaces):
    """(AffineROMFin, Case) per (m, r, basis, creation switches, observations, projection), made once; the Case's inputs are the
    handle's own tables (Case.adopt)."""
    from bayesianinferencedl_amd.rom.averaged_affine_ROM import AffineROMFin
    made = {}

    def get(m, r, kind="parity", env=None, external_obs=False, projection=None):
        key = (m, r, kind, env, external_obs, projection)
        c = Y.case(m, r, kind, external_obs)
        if key not in made:
            with _env(**({env: "1"} if env else {})):
                made[key] = AffineROMFin(spaces(m), None, c.phi, external_obs=external_obs, projection=projection)
            c.adopt(made[key])
        return made[key], c
    return get


def _check(label, c, out, S, form="full", all_samples=True, skip=(), walk=False):
    """info clean; qoi_r (and Phi w_r where w_r came back) within the allowance of the 80-bit yardstick on the checked samples and,
    for a full list, of the QR yardstick on every sample."""
    assert not np.asarray(out["info"]).any(), label
    keys = ("qoi_r", "Phi_w") if "w_r" in out else ("qoi_r",)
    ss = [s for s in Y.checked_samples(S) if s not in skip]
    ok = Y.report(f"{label}, 80-bit on {len(ss)} samples", c.against_ld(out, ss, keys, form, walk=walk))
    if all_samples and form == "full":
        ok = Y.report(f"{label}, QR on all {S}", c.against_qr(out, S, keys, skip, walk=walk)) and ok
    assert ok, label


def _check_state(label, c, out, S, form="full", skip=()):
    """With the state: A_r, B_r against the 80-bit ones (1e-12, as everywhere), and the backward error of the device's w_r ON THE
    DEVICE'S OWN A_r, B_r against cho_solve's on the same matrices: margin 8, floor r 2^-53."""
    worst = (0.0, 0.0)
    for s in [s for s in Y.checked_samples(S) if s not in skip]:
        A, b, w = (np.asarray(out[k])[s] for k in ("A_r", "B_r", "w_r"))
        ref = c.ld(s, form)
        assert Y.dev(A.ravel(), ref["A_r"].ravel()) <= 1e-12 and Y.dev(b, ref["B_r"]) <= 1e-12, (label, s)
        assert np.array_equal(A, A.T), (label, s)
        be_d = Y.backward_error(A, b, w)
        be_h = Y.backward_error(A, b, sla.cho_solve(sla.cho_factor(A, lower=True), b))
        assert be_d <= max(8.0 * be_h, c.r * 2.0 ** -53), (label, s, be_d, be_h)
        worst = max(worst, (be_d, be_h))
    print(f"{label}: backward error of w_r on the device's A_r, B_r: device {worst[0]:.2e}, cho_solve {worst[1]:.2e}")


@pytest.mark.parametrize("S", [1, 3, 64])
@pytest.mark.parametrize("r", [33, 80, 96])
def test_one_sample_kernels(models, r, S):
    """Batches of <= 64 samples without the state, m = 12: rom_small_proj_kernel (the contraction over several workgroups per sample)
    + rom_small_solve_kernel (MFMA-form factorisation and substitutions), with w_r and QoI-only.
    Measured, largest over S and both forms (qoi_r, device / host64, relative to the yardstick): r = 33: 2.4e-13 / 8.3e-13, r = 80:
    6.1e-13 / 2.3e-12, r = 96: 5.7e-13 / 1.8e-12; device / host64 per batch at most 2.5."""
    rom, c = models(12, r)
    for want_w in (True, False):
        out = rom._rom.solve(c.TH[:S], want_w=want_w)
        assert rom._rom.last_form() == "full" and rom._rom.last_epilogue() == "standard"
        assert ("w_r" in out) == want_w
        _check(f"one-sample kernels, r = {r}, S = {S}, want_w = {want_w}", c, out, S)


@pytest.mark.parametrize("S", [3, 64])
@pytest.mark.parametrize("r", [33, 64, 96])
def test_small_batches_with_the_state(models, r, S):
    """want_state=True keeps small batches off the one-sample kernels: r = 64, 96 take rom_proj_splitk_kernel (a sample's k-steps
    over four waves, A_r written) + rom_solve_kernel (left-looking Cholesky in LDS); r = 33 (three blocks: no split-K) takes
    rom_proj_single_kernel with the grouped loop + rom_solve_kernel.
    Measured (qoi_r, device / host64): r = 64: 1.8e-12 / 2.3e-12, r = 96: 1.1e-12 / 1.8e-12 (per batch up to 2.2); r = 33, S = 64:
    3.2e-12 / 8.3e-13 (factor 4.2).  r = 33, S = 3: device 1.39e-12, host64 7.6e-14 on these three samples -- 18 x, and over the
    floor of 1e-12: the one cell found outside 8 x BLAS's host64.  host64 on A_r from the grouped k-step tables walked in fp64
    (rom_lspg_cases.grouped_walk, the kernel's own order of sums; the same matrix to 9e-16) gives 1.61e-12 on the same samples,
    so that walk is this cell's second comparator (Y.WALK_CELL; tests/test_rom_lspg_host.py holds it to the cap).  Backward
    error of w_r on the device's own A_r, B_r: 1e-19 .. 4e-19, cho_solve's the same (|A_r|_F |w_r| is 1e5 x |B_r| here: the floor
    r 2^-53 decides, the check catches a gross slip only)."""
    rom, c = models(12, r)
    out = rom._rom.solve(c.TH[:S], want_state=True)
    assert rom._rom.last_form() == "full" and rom._rom.last_epilogue() == "standard"
    label = f"state, r = {r}, S = {S}"
    _check(label, c, out, S, walk=(12, r, S) == Y.WALK_CELL)
    _check_state(label, c, out, S)
    plain = rom._rom.solve(c.TH[:S])                       # the one-sample kernels: another contraction, other bits
    assert not np.array_equal(np.asarray(plain["qoi_r"]), np.asarray(out["qoi_r"]))


@pytest.mark.parametrize("S", [65, 301])
@pytest.mark.parametrize("m,r", [(4, 16), (12, 33), (12, 80)])
def test_grouped_one_wave_kernel(models, m, r, S):
    """Batches of more than 64 samples at r <= 80: rom_proj_single_kernel, k-steps grouped by sub-domain with the accumulators
    rescaled where the group changes (proj_main_grouped), against a handle created with FINROM_PROJ_UNGROUPED=1 (table order) --
    each within its allowance of the yardstick, and not the same bits.  Three variants: the fused solve (Cholesky, substitutions
    and QoI in the kernel's registers; w_r returned), QoI-only, and with the state (A_r written, rom_solve_kernel).
    Measured (qoi_r against QR on all 301, device / host64, the three variants alike): grouped (4, 16): 3.2e-12 / 4.2e-12, (12, 33):
    3.8e-12 / 2.1e-12 (factor 1.8), (12, 80): 4.2e-12 / 2.3e-12 (1.8); ungrouped: 1.4e-12, 1.3e-12 (0.6), 2.4e-12 (1.1).  On the 8
    samples of the 80-bit yardstick the grouped loop reaches factor 5.2 at (12, 80) (2.3e-12 / 4.5e-13), the largest of the solve."""
    rom_g, c = models(m, r)
    rom_u, _ = models(m, r, env="FINROM_PROJ_UNGROUPED")
    TH = c.TH[:S]
    for name, kw in (("fused solve", {}), ("QoI-only", {"want_w": False}), ("state", {"want_state": True})):
        g, u = rom_g._rom.solve(TH, **kw), rom_u._rom.solve(TH, **kw)
        assert rom_g._rom.last_form() == rom_u._rom.last_form() == "full" and rom_g._rom.last_epilogue() == "standard"
        _check(f"grouped, {name}, m = {m}, r = {r}, S = {S}", c, g, S)
        _check(f"ungrouped, {name}, m = {m}, r = {r}, S = {S}", c, u, S)
        assert not np.array_equal(np.asarray(g["qoi_r"]), np.asarray(u["qoi_r"])), "the grouped loop did not run"
        if name == "state":
            _check_state(f"grouped, state, m = {m}, r = {r}, S = {S}", c, g, S)
            _check_state(f"ungrouped, state, m = {m}, r = {r}, S = {S}", c, u, S)
    if m == 12 and S == 65:                                # the first 64 alone take the one-sample kernels: other bits
        assert not np.array_equal(np.asarray(rom_g._rom.solve(TH[:64])["qoi_r"]), np.asarray(rom_g._rom.solve(TH)["qoi_r"])[:64])


@pytest.mark.parametrize("r", [81, 96])
def test_in_register_factor_and_substitution_kernel(models, r):
    """S = 301, six blocks (r = 81 .. 96): rom_proj_kernel<6, 1> factors A_r in registers and writes the packed factor,
    rom_subst_blocked_kernel does both substitutions and the QoI; QoI-only takes the same pair; with the state rom_proj_kernel
    writes A_r and rom_solve_kernel factors it.
    Measured (qoi_r, device / host64): r = 81: 2.1e-12 / 2.5e-12 (factor 0.8); r = 96: 3.1e-12 / 2.7e-12 (1.1); the three variants
    within 5 % of each other."""
    rom, c = models(12, r)
    S = 301
    for name, kw in (("w_r", {}), ("QoI-only", {"want_w": False}), ("state", {"want_state": True})):
        out = rom._rom.solve(c.TH[:S], **kw)
        assert rom._rom.last_form() == "full" and rom._rom.last_epilogue() == "standard"
        _check(f"in-register factor, {name}, r = {r}, S = {S}", c, out, S)
        if name == "state":
            _check_state(f"in-register factor, state, r = {r}", c, out, S)
            assert not np.array_equal(np.asarray(out["w_r"]), np.asarray(rom._rom.solve(c.TH[:S])["w_r"]))


@pytest.mark.parametrize("r", [120, 128, 136, 200])
def test_wide_bases(models, r):
    """S = 70, more than six blocks, four or eight waves per sample: r = 120, 136, 200 take the HalfCover projection
    (launch_rom_proj_half: the last block at most half full), r = 128 the aligned rom_proj_kernel<8, 4>.  want_w: A_r written,
    rom_chol_blocked_kernel + rom_subst_blocked_kernel; QoI-only: factorisation and QoI in the projection kernel's registers
    (fused_solve_mw), other bits; with the state: rom_solve_kernel (r = 200: the factor in global memory).
    Measured (qoi_r, device / host64, largest per-batch factor): r = 120: 2.3e-12 / 1.2e-12 (1.8), r = 128: 1.5e-12 / 1.9e-12 (1.9),
    r = 136: 2.0e-12 / 1.5e-12 (1.4), r = 200: 5.3e-12 / 4.9e-12 (1.2).  (Which of the two projections ran the library does not
    report, and they return the same bits: test_half_block_cover_gives_the_aligned_kernels_bits.)"""
    rom, c = models(12, r)
    S = 70
    outs = {}
    for name, kw in (("w_r", {}), ("QoI-only", {"want_w": False}), ("state", {"want_state": True})):
        outs[name] = out = rom._rom.solve(c.TH[:S], **kw)
        assert rom._rom.last_form() == "full" and rom._rom.last_epilogue() == "standard"
        _check(f"wide basis, {name}, r = {r}, S = {S}", c, out, S)
        if name == "state":
            _check_state(f"wide basis, state, r = {r}", c, out, S)
    assert not np.array_equal(np.asarray(outs["w_r"]["qoi_r"]), np.asarray(outs["QoI-only"]["qoi_r"]))


@pytest.mark.parametrize("m,r", [(4, 16), (12, 33), (12, 80)])
def test_half_list_and_short_list_against_their_own_lspg(models, m, r):
    """The benchmark-recipe basis, mirror-symmetric theta, S = 301, rom_proj_single_kernel on the half list: the default handle's
    in-range samples walk the SHORT list and are held to the short list's own LSPG (A_r from its rows, B_r and B_obs Phi from the
    full tables); a handle created with FINROM_ROM_KEEP_ROWS=1 walks the half list with all rows and is held to that list's; one
    sample outside [0.1, 10] (12 in a mirror pair) must walk the half list with all rows on both handles: the same bits, within
    the allowance of the half list's statement for it.  Fused solve, QoI-only and with the state.
    Measured (qoi_r, device / host64 against the list's own 80-bit LSPG): short list (4, 16): 6.0e-14 / 1.1e-13, (12, 33): 2.8e-12 /
    3.2e-12, (12, 80): 1.9e-12 / 6.3e-12; half list with all rows: 3.6e-14, 2.7e-12, 6.2e-12 / 4.5e-12 (factor 1.4; Phi w_r 1.6)."""
    rom, c = models(m, r, "bench")
    keep, _ = models(m, r, "bench", env="FINROM_ROM_KEEP_ROWS")
    assert rom._rom.mirror and keep._rom.mirror and rom._rom.mirror_dropped > 0 and keep._rom.mirror_dropped == 0
    S, out_of_range = 301, 5
    assert out_of_range not in Y.checked_samples(S)
    TH = c.TH[:S].copy()
    TH[out_of_range, [0, 8]] = 12.0
    for name, kw in (("fused solve", {}), ("QoI-only", {"want_w": False}), ("state", {"want_state": True})):
        a, b = rom._rom.solve(TH, **kw), keep._rom.solve(TH, **kw)
        assert rom._rom.last_form() == keep._rom.last_form() == "half"
        _check(f"short list, {name}, m = {m}, r = {r}", c, a, S, form="short", skip=(out_of_range,))
        _check(f"half list, {name}, m = {m}, r = {r}", c, b, S, form="half", skip=(out_of_range,))
        if name == "state":
            _check_state(f"short list, state, m = {m}, r = {r}", c, a, S, form="short", skip=(out_of_range,))
            _check_state(f"half list, state, m = {m}, r = {r}", c, b, S, form="half", skip=(out_of_range,))
        for key in a:
            assert np.array_equal(np.asarray(a[key])[out_of_range], np.asarray(b[key])[out_of_range]), (name, key)
        if rom._rom.mirror_dropped_max ** 2 >= 2.0 ** -53:
            assert not np.array_equal(np.asarray(a["qoi_r"]), np.asarray(b["qoi_r"]))
        rows = dict(zip(("row_tables", "rows", "weight"), Y.half_rows(c.form, False)))
        ref = Y.lspg_ld(c.tables, c.F, c.C, TH[out_of_range], **rows)
        h = Y.host64(c.tables, c.F, c.C, TH[out_of_range], **rows)
        dd, dh = Y.dev(np.asarray(a["qoi_r"])[out_of_range], ref["qoi_r"]), Y.dev(h["qoi_r"], ref["qoi_r"])
        print(f"the sample outside the range, {name}, m = {m}, r = {r}: qoi_r device {dd:.2e}, host64 {dh:.2e}")
        assert dd <= Y.allowance(dh) <= Y.CAP


@pytest.mark.parametrize("m,r,S", [(4, 8, 301), (12, 80, 301), (12, 120, 70)])
def test_offline_online_projection(models, m, r, S):
    """projection='offline_online': A_r = sum theta_p theta_q G_pq from the precomputed blocks -- rom_gram_kernel (r <= 96, tile
    images, factor and solve in registers) at r = 8 and 80, rom_gram_store_kernel (packed triangle) + the blocked Cholesky and
    substitution kernels at r = 120.  With w_r, QoI-only, with the state.
    Measured (qoi_r, device / host64): (4, 8): 2.3e-13 / 5.3e-13, (12, 80): 1.0e-12 / 2.3e-12, (12, 120): 7.8e-13 / 1.2e-12."""
    rom, c = models(m, r, projection="offline_online")
    assert rom.projection == "offline_online"
    direct, _ = models(m, r)
    for name, kw in (("w_r", {}), ("QoI-only", {"want_w": False}), ("state", {"want_state": True})):
        out = rom._rom.solve(c.TH[:S], **kw)
        assert rom._rom.last_form() == "full" and rom._rom.last_epilogue() == "standard"
        _check(f"offline/online, {name}, m = {m}, r = {r}, S = {S}", c, out, S)
        if name == "state":
            _check_state(f"offline/online, state, m = {m}, r = {r}", c, out, S)
            assert not np.array_equal(np.asarray(out["A_r"]), np.asarray(direct._rom.solve(c.TH[:S], **kw)["A_r"]))


def _check_grad(label, rom, c, S):
    """J, g (and qoi_r) with shared and with per-sample data against grad_ld on the checked samples."""
    ss = Y.checked_samples(S)
    for per_sample, data in ((False, c.data), (True, c.D[:S])):
        out = rom.grad_reduced_batch(None, data=data, theta=c.TH[:S])
        out["g"] = out["g_theta"]
        assert not np.asarray(out["info"]).any(), label
        kind = "per-sample data" if per_sample else "shared data"
        ok = Y.report(f"{label}, {kind}, 80-bit on {len(ss)} samples", c.against_ld(out, ss, ("J", "g"), per_sample=per_sample))
        ok = Y.report(f"{label}, {kind}, the solve", c.against_ld(out, ss, ("qoi_r", "Phi_w"))) and ok
        assert ok, (label, kind)


@pytest.mark.parametrize("S", [3, 64])
@pytest.mark.parametrize("r", [33, 81])
def test_gradient_one_sample_kernels(models, r, S):
    """finrom_rom_grad, batches of <= 64 samples, m = 12, nine observations: rom_small_proj_kernel + rom_small_solve_kernel (forward
    and adjoint solves) + rom_grad_contract_small_kernel (v_r^T G_pi w_r dealt over 36 workgroups per sample).
    Measured (device / host64): r = 33: J 1.8e-13 / 5.8e-13, g 9.2e-13 / 2.4e-12 (per batch up to 1.3); r = 81: J 3.9e-13 / 2.3e-12,
    g 4.5e-12 / 2.1e-12 (3.2)."""
    rom, c = models(12, r)
    _check_grad(f"gradient, one-sample kernels, r = {r}, S = {S}", rom, c, S)


@pytest.mark.parametrize("projection", ["direct", "offline_online"])
@pytest.mark.parametrize("S", [70, 200])
@pytest.mark.parametrize("r", [80, 120])
def test_gradient_batched_contraction(models, r, S, projection):
    """finrom_rom_grad, batches of >= 64 samples: the projection writes the factor (r = 80: rom_proj_single_kernel, grouped; r = 120:
    HalfCover projection + rom_chol_blocked_kernel; offline/online: rom_gram_kernel / rom_gram_store_kernel),
    rom_subst_blocked_kernel does both solves, rom_grad_contract_kernel contracts v_r^T G_pi w_r on the matrix cores, 16 samples
    per wave (S = 70, 200: ragged last waves).
    Measured (device / host64, largest per-batch factor): direct r = 80: g 1.3e-11 / 4.3e-12 (3.3), J 1.3e-12 / 7.7e-13; direct
    r = 120: g 4.8e-12 / 2.6e-12 (2.5), J 4.3e-13 / 1.5e-13 (3.5), qoi_r 7.9e-13 / 4.9e-13 (4.0); offline/online: g 4.0e-12 (1.2)
    and 1.5e-12 (1.0).  The direct form's A_r carries about three times BLAS's rounding error and g amplifies it most."""
    rom, c = models(12, r, projection=None if projection == "direct" else projection)
    assert rom.projection == projection
    _check_grad(f"gradient, batched contraction, {projection}, r = {r}, S = {S}", rom, c, S)


@pytest.mark.parametrize("S", [3, 64])
def test_gradient_split_k_form_with_forty_observations(models, S):
    """finrom_rom_grad with the 40 point observations of external_obs=True (n_obs > 15: no one-sample kernels), r = 81, batches of
    <= 64: the whole adjoint gradient in rom_proj_splitk_kernel (factor 4) + rom_grad_contract_small_kernel.
    Measured (device / host64): J 1.2e-12 / 1.6e-12, g 4.6e-12 / 3.9e-12 (factor 1.2), qoi_r 1.3e-12 / 1.8e-12."""
    (m, r), _ = Y.GRAD40
    rom, c = models(m, r, external_obs=True)
    assert rom.n_obs == 40 and c.C.shape[0] == 40
    _check_grad(f"gradient, split-K form, 40 observations, r = {r}, S = {S}", rom, c, S)
