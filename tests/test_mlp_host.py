"""CPU tests of the error model's inference suite: the float64 reference of tests/mlp_cases.py against torch autograd, the library's
staging predicate against the furthest index the staged loops read, and -- row by row -- the branch of the device code each case of
tests/test_gpu_mlp_kernels.py is meant to take (no GPU: nothing here reaches a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mlp_cases as K

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bayesianinferencedl_amd", "csrc")


# ---- the reference is the network ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 12, 0, 9), (245, 17, 3, 9), (64, 50, 9, 40)], ids=str)
def test_forward64_and_vjp64_match_torch_autograd_in_float64(shape):
    """The same folded fp32 arrays, widened, through torch ops and torch.autograd: an independent statement of the formula."""
    import torch
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    n_in, n_w, L, n_out = shape
    model = K.make_model(n_in, n_w, L, n_out, seed=5, pins=(L == 3))
    a = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in DeviceErrorModel.fold(model).items()}
    X = K.forward_inputs(n_in, 6, seed=1).astype(np.float32).astype(np.float64)
    up = np.random.default_rng(2).standard_normal((6, n_out))
    x = torch.from_numpy(X).requires_grad_(True)
    y = x @ a["W0"] + a["b0"]
    zs = []
    for l in range(L + 1):
        z = y * a["scale"][l] + a["shift"][l]
        zs.append(z)
        act = torch.nn.functional.elu(z)
        y = y + act @ a["W"][l] + a["b"][l] if l < L else act @ a["Wh"] + a["bh"]
    (y * torch.from_numpy(up)).sum().backward()
    out, z64 = K.forward64(model, X)
    g = K.vjp64(model, X, up)
    assert z64.shape == (L + 1, 6, n_w)
    assert np.max(np.abs(out - y.detach().numpy())) <= 1e-13 * np.max(np.abs(out))
    assert np.max(np.abs(z64 - torch.stack(zs).detach().numpy())) <= 1e-13 * np.max(np.abs(z64))
    assert np.max(np.abs(g - x.grad.numpy())) <= 1e-13 * np.max(np.abs(g))
    # and the fp32 host model is the same network: its deviation is fp32 rounding, not a different formula
    assert np.max(np.abs(model.predict(X) - out)) <= 1e-4 * np.max(np.abs(out))
    assert np.max(np.abs(model.vjp(X, up) - g)) <= 1e-4 * np.max(np.abs(g))


def test_the_reference_rounds_the_input_to_fp32_and_nothing_else():
    model = K.make_model(40, 8, 2, 3, seed=1)
    X = K.forward_inputs(40, 3)
    assert np.array_equal(K.forward64(model, X)[0], K.forward64(model, X.astype(np.float32))[0])
    assert not np.array_equal(K.forward64(model, X)[0], K.forward64(model, X + 1e-6)[0])
    assert K.forward64(model, X)[0].dtype == np.float64 and K.vjp64(model, X, np.ones((3, 3))).dtype == np.float64


def test_romml_ref_with_the_fp32_model_is_the_oracles_grad_romml():
    from oracle import fin_oracle as O
    c = K.FUSED_BY_NAME["b8-pins"]
    prob, phi, ro = K.oracle_rig(c.m, c.r, c.n_obs)
    model, k, data = K.fused_model(c), K.rom_inputs(prob.n, 1, seed=3)[0], K.fused_data(c)
    ro.set_data(data)
    go, lo = O.grad_romml_oracle(ro, model, k)
    ref = K.romml_ref(ro, model, k, data, "f32")
    assert np.array_equal(ref["grad"], go) and ref["loss"] == lo
    r64 = K.romml64(ro, model, k)
    assert 0 < np.max(np.abs(r64["grad"] - go)) <= 1e-4 * np.max(np.abs(go))
    # five parameters: the nine-parameter model driven through the 9 x n operator E Sop5 is the same function with the same
    # gradient (the reference's reduced gradient is its own formula, not the derivative of the value: no difference quotient here)
    E, S5 = K.five_parameters(ro.dsigma_dk)
    assert E.shape == (9, 5) and S5.shape == (5, prob.n) and np.all(E.sum(1) == 1) and np.all(E @ (S5 @ k) > 0)
    five, nine = K.romml64(ro, model, k, E=E, Sop=S5), K.romml64(ro, model, k, Sop=E @ S5)
    assert five["loss"] == nine["loss"] and np.max(np.abs(five["grad"] - nine["grad"])) <= 1e-13 * np.max(np.abs(nine["grad"]))
    assert np.max(np.abs(five["grad"] - r64["grad"])) > 1e-3 * np.max(np.abs(r64["grad"]))


# ---- the staging predicate bounds what the staged loops read ----------------------------------------------------------------------
def _furthest_index(n_layers, n_w, n_out):
    """mlp_forward_tail_wave<true>, spelled out: W = wl + l n_w^2 + tid; wv[u] = W[(i0 + u) * ld] for i0 + u < 64, every lane."""
    far = 0
    for l in range(n_layers + 1):
        ld = n_out if l == n_layers else n_w
        far = max(far, l * n_w * n_w + 63 + 63 * ld)
    return far


def test_the_staging_predicate_bounds_the_furthest_index_read():
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    stg, fl = C.c_int32(), C.c_int32()
    assert L.finrom_mlp_stage_reach(5, 50, 9, C.byref(stg), C.byref(fl)) == K.stage_reach(5, 50, 9) and stg.value == 1
    assert fl.value == K.MLP_STAGE_FLOATS == 16384
    n_staged = n_moved = 0
    for nl in range(0, 65):
        for nw in range(1, 65):
            for no in (1, 9, 15, 40, 64):
                reach = L.finrom_mlp_stage_reach(nl, nw, no, C.byref(stg), None)
                assert reach == K.stage_reach(nl, nw, no) == _furthest_index(nl, nw, no) + 1
                assert bool(stg.value) == K.staged(nl, nw, no)
                if stg.value:                                # everything the unguarded loops touch is weights or zero fill
                    n_staged += 1
                    assert reach <= fl.value and nl * nw * nw + nw * no <= reach and (nl * nw * nw) % 4 == 0
                n_moved += K.staged_before_the_fix(nl, nw, no) and not stg.value
    assert n_staged > 1000 and n_moved > 0
    # the shape of the finding: 15 876 floats of weights, lane 63 of layer 11 reads index 16 587
    assert 12 * 36 * 36 + 36 * 9 == 15876 and K.stage_reach(12, 36, 9) == 16588
    assert K.staged_before_the_fix(12, 36, 9) and not K.staged(12, 36, 9)
    assert K.staged(5, 50, 9) and K.staged(6, 50, 9)         # the reference's shapes keep the staged wave
    assert L.finrom_mlp_stage_reach(65, 50, 9, None, None) == -1 and L.finrom_mlp_stage_reach(5, 0, 9, None, None) == -1
    assert L.finrom_deferred_count() == 0


def test_the_kernel_takes_its_predicate_and_its_lds_from_the_shared_header():
    one = open(os.path.join(CSRC, "rom_onesample.hip")).read()
    hdr = open(os.path.join(CSRC, "finrom_internal.h")).read()
    assert re.search(r"const bool staged = fm\.on && mlp_tail_staged\(fm\.m\.n_layers, fm\.m\.n_w, fm\.m\.n_out\);", one)
    assert "MLP_STAGE_FLOATS" not in re.sub(r"mlp \? MLP_STAGE_FLOATS / 2|\[MLP_STAGE_FLOATS\]", "", one).replace("n_stage <= MLP_STAGE_FLOATS", "!")
    assert re.search(r"MLP_STAGE_FLOATS = 16 \* 256 \* 4;", hdr) and re.search(r"constexpr int LMAX = 8;", open(os.path.join(CSRC, "mlp_device.h")).read())
    assert re.search(r"mlp_stage_reach\(n_layers, n_w, n_out\) <= MLP_STAGE_FLOATS && \(\(n_layers \* n_w \* n_w\) & 3\) == 0", hdr)
    mk = open(os.path.join(CSRC, "mlp_kernels.hip")).read()
    assert re.search(r"MLP_SPLIT_MAX_S = 64;", mk) and re.search(r"if \(S <= MLP_SPLIT_MAX_S\)\s*\n\s*hipLaunchKernelGGL\(mlp_backward_kernel<MLP_SPLIT>", mk)
    assert re.search(r"HMC_THETA_PARTS = 8;", hdr) and re.search(r"MLP_SPLIT = HMC_THETA_PARTS;", mk)


def test_forward_input_limit_is_the_kernels_lds(tmp_path):
    """MLP_FORWARD_MAX_IN = what 64 KB leave beside mlp_forward_kernel's static LDS, read from the build."""
    import subprocess
    from bayesianinferencedl_amd import _build, _ffi
    assert _ffi.lib().finrom_mlp_forward_max_in() == K.FORWARD_MAX_IN == 15200
    try:
        hipcc = _build._hipcc()
        subprocess.run([hipcc, "--version"], capture_output=True, check=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError) as exc:
        pytest.skip(f"hipcc not found ({exc})")
    asm = tmp_path / "mlp_kernels.s"
    r = subprocess.run([hipcc, *_build.FLAGS, "-O3", "--cuda-device-only", "-S", os.path.join(_build.CSRC, "mlp_kernels.hip"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = asm.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    blk = [b for b in re.split(r"\n  - (?=\.)", meta)[1:] if re.search(r"\.name:\s*\S*mlp_forward_kernel", b)]
    assert len(blk) == 1
    assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", blk[0]).group(1)) == K.FORWARD_STATIC_LDS == 4736
    assert (K.FORWARD_STATIC_LDS + 4 * K.FORWARD_MAX_IN) <= 64 * 1024 < K.FORWARD_STATIC_LDS + 4 * (K.FORWARD_MAX_IN + 1)
    assert K.M28_N <= K.FORWARD_MAX_IN and K.FWD_TOO_WIDE.n_in == K.FORWARD_MAX_IN + 1


# ---- the forward ladder: one axis at a time around (1597, 50, 5, 9), every branch claimed -------------------------------------------
def test_the_forward_ladder_has_every_value_the_issue_lists_and_the_corners():
    rows = K.FWD_CASES
    ref = K.REF
    assert len(rows) == len(set(rows)) and 50 <= len(rows) <= 80
    assert {c.n_w for c in rows if (c.n_in, c.n_layers, c.n_out) == (ref[0], ref[2], ref[3])} >= set(K.FWD_W) == {1, 15, 16, 17, 31, 32, 33, 48, 50, 63, 64}
    assert {c.n_layers for c in rows if (c.n_in, c.n_w, c.n_out) == (ref[0], ref[1], ref[3])} >= set(K.FWD_L) == {0, 1, 2, 5, 8, 9, 12}
    assert {c.n_out for c in rows if (c.n_in, c.n_w, c.n_layers) == (ref[0], ref[1], ref[2])} >= set(K.FWD_OUT) == {1, 9, 40, 64}
    assert {c.n_in for c in rows if (c.n_w, c.n_layers, c.n_out) == ref[1:]} >= set(K.FWD_IN) == {1, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 1597, 4101, 7757}
    assert {c.S for c in rows if (c.n_in, c.n_w, c.n_layers, c.n_out) == ref} >= set(K.FWD_S) == {1, 2, 64, 65, 300}
    from oracle import fin_oracle as O
    assert O.FinProblem(28).n == K.M28_N and [O.FinProblem(m).n for m in (4, 8, 12)] == [K.MESH_N[m] for m in (4, 8, 12)]
    # corners: both ends of every axis together
    assert any((c.n_in, c.n_w, c.n_layers, c.n_out) == (1, 1, 0, 1) for c in rows)
    assert any((c.n_in, c.n_w, c.n_layers, c.n_out) == (K.M28_N, 64, 12, 64) for c in rows)
    assert any(c.n_in == K.FORWARD_MAX_IN for c in rows) and all(c.n_in <= K.FORWARD_MAX_IN for c in rows)
    assert sum(c.pins for c in rows) >= 3 and len(K.FWD_BITWISE) >= 10 and all(c.S > 1 for c in K.FWD_BITWISE)


def test_the_forward_ladder_claims_every_loop_form():
    """mlp_forward_body<1024>: sixteen parts of the first layer in batches of 32 rows, then of 16, then one by one; the hidden layers
    16 inputs at a time, then one by one."""
    rows = K.FWD_CASES
    parts = [p for c in rows for p in K.forward_chunks(c.n_in)]
    assert K.forward_chunks(1597)[0] == (3, 0, 3) and K.forward_chunks(1597)[4] == (3, 0, 4)
    assert K.forward_chunks(15).count((0, 0, 0)) == 1 and K.forward_chunks(1).count((0, 0, 0)) == 15      # parts without rows
    assert K.forward_chunks(512) == [(1, 0, 0)] * 16 and K.forward_chunks(16) == [(0, 0, 1)] * 16
    assert (0, 1, 0) in K.forward_chunks(256) and (1, 1, 15) in K.forward_chunks(1023) and (15, 0, 4) in K.forward_chunks(K.M28_N)
    for want in [(0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0), (1, 1, 15)]:
        assert want in parts, want
    assert any(f > 0 and m == 0 and t > 0 for f, m, t in parts) and any(f == 0 and m == 1 and t > 0 for f, m, t in parts)
    loops = {K.layer_loops(c.n_w) for c in rows if c.n_layers > 0}
    assert {(0, 1), (0, 15), (1, 0), (1, 1), (1, 15), (2, 0), (2, 1), (3, 0), (3, 2), (3, 15), (4, 0)} <= loops
    assert {c.n_layers for c in rows} >= {0, 1, 8, 9, 12}
    assert any(c.n_out > c.n_w for c in rows) and any(c.n_out == 64 and c.n_w == 64 for c in rows)      # head lanes beyond the hidden width


@pytest.mark.parametrize("c", K.FWD_CASES, ids=K.fwd_id)
def test_forward_rows_are_not_degenerate(c):
    """Pre-activations on both sides of zero in every layer, the pins where they are asked for, and an fp32 host deviation that is a
    rounding error: finite, not zero beyond the smallest shapes, small."""
    if c.n_in * c.S > 2_000_000:
        X = K.forward_inputs(c.n_in, c.S)[:8]
    else:
        X = K.forward_inputs(c.n_in, c.S)
    model = K.fwd_model(c)
    out, zs = K.forward64(model, X)
    assert zs.shape[0] == c.n_layers + 1 and np.isfinite(out).all()
    free = zs[:, :, 3:] if c.pins else zs
    if free[0].size >= 16 and c.n_w > 1:                     # (one unit: both signs somewhere in the network)
        for l in range(c.n_layers + 1):
            assert (free[l] > 0).any() and (free[l] < 0).any(), l
    elif free.size > 1:
        assert (free > 0).any() and (free < 0).any()
    if c.pins:
        assert (zs[:, :, 0] == 0.0).all() and (zs[:, :, 1] < -30).all() and (zs[:, :, 2] > 20).all()
        m32 = model._forward(X.astype(np.float32))[1]
        assert all((z[:, 0] == 0).all() for z, _ in m32)
    d32 = np.max(np.abs(model.predict(X) - out))
    assert np.isfinite(d32) and d32 <= 1e-4 * max(np.max(np.abs(out)), 1.0)
    if c.n_in >= 15 and c.n_w >= 15:
        assert d32 > 0.0


# ---- value and gradient: every form claimed ----------------------------------------------------------------------------------------
def test_fused_rows_take_the_form_they_are_named_for():
    rows = K.FUSED_CASES
    assert len({c.name for c in rows}) == len(rows)
    for c in rows:
        n = K.MESH_N[c.m]
        one = K.one_sample_form(n, c.r, c.n_obs, c.S, c.projection, c.P)
        assert one is (c.form == "one"), c.name              # (never None: no row leaves its form to an unknown number of k-steps)
        if c.form != "one":
            assert K.backward_np(c.S) == {"b8": 8, "b1": 1}[c.form], c.name
            assert c.staged is None and c.pre is None
        else:
            assert c.staged == K.staged(c.n_layers, c.n_w, c.n_obs) and c.pre == K.pre(c.n_layers) and c.name.startswith("one-" + ("staged" if c.staged else "unstaged")) or c.name == "one-P5"
        assert c.n_obs in (9, 40) and c.P in (5, 9) and c.r <= 33
    assert all(K.FUSED_BY_NAME[nm].n_obs == 40 and K.FUSED_BY_NAME[nm].form != "one" for nm in ("b8-obs40", "b8-obs40-w15", "b1-obs40"))
    assert K.one_sample_form(1597, 16, 40, 3) is False and K.one_sample_form(245, 8, 9, 3) is None
    one = [c for c in rows if c.form == "one"]
    forms = {(c.staged, c.pre) for c in one}
    assert forms == {(True, True), (True, False), (False, True), (False, False)}
    why = lambda c: ("size" if c.n_layers * c.n_w ** 2 + c.n_w * c.n_obs > K.MLP_STAGE_FLOATS else
                     "align" if (c.n_layers * c.n_w ** 2) % 4 else "reach")
    assert {why(c) for c in one if not c.staged} == {"size", "align", "reach"}
    c = K.FUSED_BY_NAME["one-unstaged-reach-36x12"]
    assert (c.n_w, c.n_layers, c.staged, c.pre) == (36, 12, False, False) and K.staged_before_the_fix(12, 36, 9)
    assert any(c.n_layers == 0 for c in one) and any(c.n_layers == 8 and c.staged for c in one) and any(c.n_layers == 9 for c in one)
    # the unstaged wave's and the walk back's loops: 16 at a time with and without a scalar tail, and a tail alone
    assert {K.layer_loops(c.n_w) for c in one if not c.staged} >= {(0, 15), (2, 1), (3, 2), (3, 15), (1, 1), (2, 4)}
    assert {K.layer_loops(c.n_w) for c in rows} >= {(0, 1), (0, 15), (1, 0), (1, 1), (2, 0), (3, 0), (3, 2), (4, 0)}
    # the first layer over four spare workgroups x four parts: batches of 32 and a scalar tail
    assert (3, 0, 3) in K.one_sample_chunks(1597) and (3, 0, 4) in K.one_sample_chunks(1597) and (1, 0, 16) in K.one_sample_chunks(777)
    # the first layer's transpose: NP = 8 leaves a workgroup fewer rows than threads, NP = 1 more (a second pass) or fewer
    assert max(K.backward_rows(1597, 8)) == 200 and K.backward_rows(1597, 1) == [1597] and min(K.backward_rows(245, 8)) == 30
    by = lambda f: [c for c in rows if c.form == f]
    assert {c.m for c in by("b1")} == {4, 12} and {c.S for c in by("b1")} >= {65, 130} and {c.S for c in by("b8")} >= {2, 64}
    for f in ("one", "b8", "b1"):
        assert any(c.per_sample for c in by(f)) and any(not c.per_sample for c in by(f)) and any(c.pins for c in by(f)), f
    assert {c.P for c in by("one")} == {5, 9} == {c.P for c in by("b8")}
    for names in (K.FUSED_BITWISE, K.FUSED_NAN):
        assert {K.FUSED_BY_NAME[nm].form for nm in names} == {"one", "b8", "b1"}
        assert {K.FUSED_BY_NAME[nm].staged for nm in names} >= {True, False}
        assert all(K.FUSED_BY_NAME[nm].S >= 3 for nm in names)
    leap = [K.FUSED_BY_NAME[nm] for nm in K.LEAP_CASES]
    assert all(c.form == "one" and c.n_obs == 9 for c in leap) and {(c.staged, c.pre) for c in leap} >= {(True, True), (True, False), (False, True), (False, False)}
    assert {c.P for c in leap} == {5, 9} and any(c.per_sample for c in leap) and {c.m for c in leap} == {8, 12}


def _qr_romml64(ro, model, k, data, E=None, Sop=None):
    """romml64 with the reduced solves through a QR factorisation of psi instead of the normal equations: the same numbers in
    exact arithmetic, another rounding -- the distance between the two is the float64 ROM's own noise."""
    k = np.asarray(k, dtype=np.float64)
    Sop = ro.dsigma_dk if Sop is None else Sop
    E = np.eye(9) if E is None else E
    psi = ro.prob.assemble_affine(E @ (Sop @ k)) @ ro.phi
    Q, R = np.linalg.qr(psi)
    w_r = np.linalg.solve(R, Q.T @ ro.B)
    e = K.forward64(model, k[None])[0][0]
    resid = data - (ro.B_obs_phi @ w_r + e)
    v_r = np.linalg.solve(R, np.linalg.solve(R.T, ro.B_obs_phi.T @ resid))
    g9 = (psi @ v_r) @ np.dot(ro.dA_dsigmak_phi, w_r).T
    return (g9 @ E) @ Sop - K.vjp64(model, k[None], resid[None])[0], 0.5 * float(resid @ resid)


@pytest.mark.parametrize("c", K.FUSED_CASES, ids=lambda c: c.name)
def test_fused_rows_are_not_degenerate(c):
    """Per row, at two samples: the fp32 host model's deviation from the float64 reference is a rounding error of the NETWORK (not
    zero, small) and stands well above the float64 reduced model's own rounding, so that the rule's right-hand side measures fp32
    summation order and nothing else; pre-activations on both sides of zero; the pins."""
    idx = [0, c.S - 1]
    Kf, data, r64, r32 = K.fused_refs(c, idx)
    prob, phi, ro = K.oracle_rig(c.m, c.r, c.n_obs)
    model = K.fused_model(c)
    zs = K.forward64(model, Kf[idx])[1]
    if c.n_w > 3:
        free = zs[:, :, 3:] if c.pins else zs
        assert all((z > 0).any() and (z < 0).any() for z in free)
    if c.pins:
        assert (zs[:, :, 0] == 0.0).all() and (zs[:, :, 1] < -30).all() and (zs[:, :, 2] > 20).all()
    kw = dict(zip(("E", "Sop"), K.five_parameters(ro.dsigma_dk))) if c.P == 5 else {}
    for j, s in enumerate(idx):
        g_qr, l_qr = _qr_romml64(ro, model, Kf[s], data[s] if c.per_sample else data, **kw)
        noise_g, noise_l = np.max(np.abs(g_qr - r64["grad"][j])), abs(l_qr - r64["loss"][j])
        d_g = np.max(np.abs(r32["grad"][j] - r64["grad"][j]))
        assert 64 * noise_g < max(d_g, K.U32 * np.max(np.abs(r64["grad"][j]))), (c.name, s, noise_g, d_g)
        assert 64 * noise_l < K.U32 * r64["loss"][j], (c.name, s, noise_l)
        assert 0 < d_g <= 1e-4 * np.max(np.abs(r64["grad"][j]))
    d_e = np.max(np.abs(r32["e_nn"] - r64["e_nn"]))
    assert d_e <= 1e-4 * np.max(np.abs(r64["e_nn"])) and (d_e > 0 or c.n_w < 15)
    assert np.all(r64["loss"] > 1e-3)                         # a residual of the observables' size: no cancellation in the loss
