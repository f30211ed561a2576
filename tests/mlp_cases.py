"""The learned error model's inference kernels (csrc/mlp_kernels.hip, csrc/mlp_device.h and the pieces inside csrc/rom_onesample.hip):
a plain float64 reference of the network and its vector-Jacobian product, the predicates that choose the device code, and the case
table of tests/test_gpu_mlp_kernels.py.  No GPU here: tests/test_mlp_host.py ties the reference to torch autograd and asserts, row by
row, the branch each case is meant to take.

The network (mlp_kernels.hip, top):
    y0 = W0^T x + b0;   y_{i+1} = y_i + W_i^T elu(s_i y_i + t_i) + b_i  (i < L);   out = W_h^T elu(s_h y_L + t_h) + b_h
The reference evaluates it in float64 on the fp32 arrays exactly as DeviceErrorModel.fold hands them to the library (scale and shift
formed in fp32, then widened) and on the fp32-rounded input (the device rounds k to float before the first layer): what is compared
is the kernels' arithmetic, not the rounding of their operands.

The tolerance rule of the GPU suite (`bound`): with dev the device result, ref64 this reference and host32 the fp32 NumPy model
(ResBnFcModel.predict / .vjp; for the fused call the oracle's dense ROM with that model),
    max|dev - ref64| <= A max(max|host32 - ref64|, u32 max|ref64|),   A = 16, u32 = 2^-24
-- the allowance tests/test_gpu_train.py gives fp32 device arithmetic over NumPy's own fp32 deviation (another summation order at
the same precision); the floor guards a case where NumPy happens to be exact."""
import functools
from collections import namedtuple

import numpy as np

from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel
from bayesianinferencedl_amd.engine import DeviceErrorModel

A = 16.0
U32 = 2.0 ** -24


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _wide(model):
    return {k: np.asarray(v, dtype=np.float64) for k, v in DeviceErrorModel.fold(model).items()}


def _round32(K, n_in):
    return np.asarray(K, dtype=np.float64).reshape(-1, n_in).astype(np.float32).astype(np.float64)


def _elu64(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def _elu_grad64(z):
    return np.where(z > 0, 1.0, np.exp(np.minimum(z, 0.0)))


def forward64(model, K):
    """K [S, n_in] -> (out [S, n_out], pre-activations [L + 1, S, n_w]) in float64."""
    a = _wide(model)
    y = _round32(K, model.n_in) @ a["W0"] + a["b0"]
    L = model.n_layers
    zs = []
    for l in range(L + 1):
        z = y * a["scale"][l] + a["shift"][l]
        zs.append(z)
        act = _elu64(z)
        if l < L:
            y = y + act @ a["W"][l] + a["b"][l]
        else:
            out = act @ a["Wh"] + a["bh"]
    return out, np.stack(zs)


def vjp64(model, K, upstream):
    """upstream [S, n_out] = d loss / d out (float64, as given) -> d loss / d input [S, n_in]."""
    a = _wide(model)
    _, zs = forward64(model, K)
    L = model.n_layers
    g = (np.asarray(upstream, dtype=np.float64).reshape(-1, model.n_out) @ a["Wh"].T) * _elu_grad64(zs[L]) * a["scale"][L]
    for l in range(L - 1, -1, -1):
        g = g + (g @ a["W"][l].T) * _elu_grad64(zs[l]) * a["scale"][l]
    return g @ a["W0"].T


def romml_ref(ro, model, k, data, net="f64", E=None, Sop=None):
    """Value and gradient of the ROM + learned-error misfit at one field k (rom/averaged_affine_ROM.py:358-396): the oracle's dense
    float64 reduced model (oracle.fin_oracle.AffineROMOracle `ro`) with the network in float64 (net="f64": forward64 / vjp64) or as
    the fp32 NumPy model (net="f32": predict / vjp -- then, with the default parameters, oracle.grad_romml_oracle's own numbers).
    E [9, P], Sop [P, n]: the reduced model is driven by P parameters theta = Sop k through the nine sub-fin conductivities E theta
    (default: the nine averages themselves, Sop = the averaging operator).
    -> dict(grad [n], loss, qoi_r [n_obs], e_nn [n_obs])."""
    k = np.asarray(k, dtype=np.float64)
    Sop = ro.dsigma_dk if Sop is None else np.asarray(Sop, dtype=np.float64)
    E = np.eye(9) if E is None else np.asarray(E, dtype=np.float64)
    w_r, A_r, B_r, psi = ro.forward_nine_param_reduced(E @ (Sop @ k), True)
    if net == "f64":
        e_nn = forward64(model, k[None])[0][0]
    else:
        e_nn = np.asarray(model.predict(k[None, :])[0], dtype=np.float64)
    obs = ro.B_obs_phi @ w_r
    resid = np.asarray(data, dtype=np.float64) - (obs + e_nn)
    v_r = np.linalg.solve(A_r.T, ro.B_obs_phi.T @ resid)
    g9 = (psi @ v_r) @ np.dot(ro.dA_dsigmak_phi, w_r).T
    f_x = (g9 @ E) @ Sop
    if net == "f64":
        nn = -vjp64(model, k[None], resid[None])[0]
    else:
        nn = -np.asarray(model.vjp(k[None, :], resid[None, :])[0], dtype=np.float64)
    return {"grad": f_x + nn, "loss": 0.5 * float(resid @ resid), "qoi_r": obs, "e_nn": e_nn}


def romml64(ro, model, k, data=None, **kw):
    return romml_ref(ro, model, k, ro.data if data is None else data, "f64", **kw)


def bound(host32, ref64):
    """The right-hand side of the tolerance rule (module docstring)."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    return A * max(float(np.max(np.abs(np.asarray(host32, dtype=np.float64) - ref64))), U32 * float(np.max(np.abs(ref64))))


def ratio(dev, host32, ref64):
    """max|dev - ref64| over max(max|host32 - ref64|, the floor): what DESIGN.md records per form; the rule asks <= A."""
    return float(np.max(np.abs(np.asarray(dev, dtype=np.float64) - ref64))) / (bound(host32, ref64) / A)


# ---- models and inputs ----------------------------------------------------------------------------------------------------------------
PINS = ("zero", "neg", "pos")


def make_model(n_in, n_w, n_layers, n_out, seed=0, pins=False):
    """Random weights, non-zero biases and non-trivial batch-norm statistics (as bench.hmc_error_model).  pins: in every layer
    (the head's included) unit 0 has gamma = beta = 0, so that its pre-activation is exactly 0; unit 1 (where there is one) has
    beta = -40 (ELU saturated at -1, its derivative ~ 4e-18) and unit 2 beta = +30 (the linear side, far out), both with gamma =
    1e-3: a scale that is small, so that the residual stream cannot move them back, and not zero, so that the walk back passes them."""
    rng = np.random.default_rng([seed, n_in, n_w, n_layers, n_out])
    model = ResBnFcModel(n_in, n_out, n_layers, n_w, seed=seed + 1)
    f32 = np.float32
    model.b0 = rng.normal(0, 0.3, n_w).astype(f32)
    for u in model.units + [model.head]:
        u["gamma"] = rng.uniform(0.5, 1.5, n_w).astype(f32)
        u["beta"] = rng.normal(0, 0.2, n_w).astype(f32)
        u["mean"] = rng.normal(0, 0.2, n_w).astype(f32)
        u["var"] = rng.uniform(0.5, 2.0, n_w).astype(f32)
        u["b"] = rng.normal(0, 0.1, u["b"].shape).astype(f32)
        if n_w == 1:                                         # (one unit: no offsets, so that the sign of the input decides its side)
            u["beta"][:] = 0; u["mean"][:] = 0; model.b0[:] = 0
        if pins:
            u["gamma"][0] = 0; u["beta"][0] = 0
            if n_w > 1:
                u["gamma"][1] = 1e-3; u["beta"][1] = -40
            if n_w > 2:
                u["gamma"][2] = 1e-3; u["beta"][2] = 30
    return model


def forward_inputs(n_in, S, seed=0):
    """Fields for the forward pass alone (any real numbers will do): a_s (1 + 0.6 N(0, 1)) with a_s = +1, -1.125, +1.25, ... so that
    even a network of one unit sees both signs."""
    a = (1.0 + np.arange(S) / 8.0) * np.where(np.arange(S) % 2, -1.0, 1.0)
    return a[:, None] * (1.0 + 0.6 * np.random.default_rng([seed, n_in, S]).standard_normal((S, n_in)))


def rom_inputs(n_in, S, seed=0):
    """Positive fields for the reduced model: exp(0.3 N(0, 1))."""
    return np.exp(0.3 * np.random.default_rng([seed, n_in, S, 1]).standard_normal((S, n_in)))


# ---- the predicates of the device code, restated --------------------------------------------------------------------------------------
MLP_STAGE_FLOATS = 16 * 256 * 4          # rom_onesample.hip stages 256 threads x 16 four-float loads
MLP_MAX_W = 64
LMAX = 8                                 # mlp_forward_tail_wave: scale / shift / bias of <= 8 hidden layers preloaded into registers
SPLIT_MAX_S = 64                         # MLP_SPLIT_MAX_S: the backward kernel's NP = 8 form; also ROM_SPLITK_MAX_S of the one-sample form
FORWARD_STATIC_LDS = (16 * 64 + 2 * 64) * 4 + 16 * 8     # mlp_forward_body<1024>: part, y, a, tred
FORWARD_MAX_IN = (64 * 1024 - FORWARD_STATIC_LDS) // 4   # 15 200


def stage_reach(n_layers, n_w, n_out):
    """One past the furthest staged index mlp_forward_tail_wave<true> reads: all 64 lanes, 64 inputs per layer, unguarded -- lane t
    reads l n_w^2 + t + i n_w (hidden layer l) and L n_w^2 + t + i n_out (head) for i < 64."""
    reach = n_layers * n_w * n_w + 63 * n_out + 63
    if n_layers > 0:
        reach = max(reach, (n_layers - 1) * n_w * n_w + 63 * n_w + 63)
    return reach + 1


def staged(n_layers, n_w, n_out):
    return stage_reach(n_layers, n_w, n_out) <= MLP_STAGE_FLOATS and (n_layers * n_w * n_w) % 4 == 0


def staged_before_the_fix(n_layers, n_w, n_out):
    """The predicate the kernel used to evaluate: it bounded the weights' count, not what the loops read."""
    return n_layers * n_w * n_w + n_w * n_out <= MLP_STAGE_FLOATS and (n_layers * n_w * n_w) % 4 == 0


def pre(n_layers):
    return n_layers <= LMAX


def one_sample_form(n, r, n_obs, S, projection="direct", P=9):
    """finrom_romml_grad's one-sample form (romml_grad_impl: `one && P <= 16`; rom_onesample_applies).  The reduced model's number
    of k-steps nku is at least n / 4 (a k-step holds four rows of psi), so n >= 256 is enough for nku >= 64; smaller meshes are not
    claimed either way (None)."""
    if projection != "direct" or S > SPLIT_MAX_S or r > 96 or n_obs > 15 or P > 16:
        return False
    return True if (n + 3) // 4 >= 64 else None


def backward_np(S):
    return 8 if S <= SPLIT_MAX_S else 1


def layer_loops(n_w):
    """(passes of the "16 at a time" body, scalar tail length) of the hidden-layer loops (forward, unstaged tail wave, backward walk,
    and the first layer's transpose over its n_w columns)."""
    return n_w // 16, n_w % 16


def first_layer_chunks(n_in, parts, ch, mid16):
    """Per part p of the first layer (rows [n_in p / parts, n_in (p + 1) / parts)): (batches of `ch`, batches of 16 where the kernel
    has them, scalar tail) -- mlp_forward_body<1024>: parts = 16, ch = 32, mid16 = True."""
    out = []
    for p in range(parts):
        n = n_in * (p + 1) // parts - n_in * p // parts
        full, n = divmod(n, ch)
        mid, n = divmod(n, 16) if mid16 else (0, n)
        out.append((full, mid, n))
    return out


def forward_chunks(n_in):
    return first_layer_chunks(n_in, 16, 32, True)


def one_sample_chunks(n_in, nw0=4):
    """mlp_first_layer_part<256>: nw0 workgroups take n_in / nw0 rows each, four parts per workgroup, batches of 32, scalar tail."""
    out = []
    for w in range(nw0):
        r0, r1 = n_in * w // nw0, n_in * (w + 1) // nw0
        for p in range(4):
            n = (r1 - r0) * (p + 1) // 4 - (r1 - r0) * p // 4
            out.append((n // 32, 0, n % 32))
    return out


def backward_rows(n_in, np_):
    """Rows of the first layer's transpose per workgroup of mlp_backward_kernel<NP>."""
    return [n_in * (w + 1) // np_ - n_in * w // np_ for w in range(np_)]


# ---- the case table: forward alone ----------------------------------------------------------------------------------------------------
Fwd = namedtuple("Fwd", "n_in n_w n_layers n_out S pins")
REF = (1597, 50, 5, 9)
M28_N = 7757                             # nodes of the m = 28 mesh, the largest with a band plan


def _fwd(n_in=REF[0], n_w=REF[1], n_layers=REF[2], n_out=REF[3], S=3, pins=False):
    return Fwd(n_in, n_w, n_layers, n_out, S, pins)


FWD_W = (1, 15, 16, 17, 31, 32, 33, 48, 50, 63, 64)
FWD_L = (0, 1, 2, 5, 8, 9, 12)
FWD_OUT = (1, 9, 40, 64)
FWD_IN = (1, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 1597, 4101, M28_N)
FWD_S = (1, 2, 64, 65, 300)
FWD_CORNERS = (
    _fwd(1, 1, 0, 1), _fwd(1, 1, 12, 1), _fwd(1, 1, 0, 1, S=16), _fwd(1, 1, 12, 1, S=16), _fwd(n_w=1, S=16), _fwd(1, 64, 12, 64, S=2), _fwd(M28_N, 64, 12, 64, S=2), _fwd(M28_N, 1, 0, 1, S=6),
    _fwd(4101, 1, 0, 64, S=6), _fwd(17, 17, 9, 40), _fwd(513, 63, 1, 1), _fwd(1025, 33, 8, 64), _fwd(15, 15, 2, 9, S=65),
    _fwd(16, 64, 0, 1, S=300), _fwd(511, 31, 9, 9, S=1), _fwd(255, 48, 1, 40), _fwd(256, 16, 8, 9), _fwd(FORWARD_MAX_IN, 17, 1, 9, S=2),
)
FWD_PINNED = (_fwd(pins=True), _fwd(245, 17, 2, 9, pins=True), _fwd(513, 3, 9, 3, S=65, pins=True), _fwd(64, 64, 1, 64, pins=True))


def _ladder():
    rows = [_fwd()]
    rows += [_fwd(n_w=w) for w in FWD_W if w != REF[1]]
    rows += [_fwd(n_layers=l) for l in FWD_L if l != REF[2]]
    rows += [_fwd(n_out=o) for o in FWD_OUT if o != REF[3]]
    rows += [_fwd(n_in=n) for n in FWD_IN if n != REF[0]]
    rows += [_fwd(S=s) for s in FWD_S]
    return rows + list(FWD_CORNERS) + list(FWD_PINNED)


FWD_CASES = _ladder()
FWD_BITWISE = [c for c in FWD_CASES if c.S > 1][::4]       # a sample alone = the sample inside its batch; two runs: every fourth row
FWD_TOO_WIDE = _fwd(FORWARD_MAX_IN + 1, 17, 1, 9, S=2)     # refused by the library


def fwd_id(c):
    return f"in{c.n_in}-w{c.n_w}-L{c.n_layers}-out{c.n_out}-S{c.S}" + ("-pins" if c.pins else "")


def fwd_model(c):
    return make_model(c.n_in, c.n_w, c.n_layers, c.n_out, seed=11, pins=c.pins)


# ---- the case table: value and gradient (finrom_romml_grad) ---------------------------------------------------------------------------
# form: "one" (the ROM's contraction + solve kernels carry the forward pass: mlp_first_layer_part, mlp_forward_tail_wave, the walk back
# in the gradient contraction, mlp_backward_kernel<8> from g0_in), "b8" (mlp_forward_kernel with the fused averages, mlp_backward_kernel<8>
# walking back itself), "b1" (the same with mlp_backward_kernel<1>).  projection "offline_online" keeps a small batch out of "one".
Fused = namedtuple("Fused", "name m r projection n_obs P n_w n_layers S per_sample pins form staged pre")
MESH_N = {4: 245, 8: 777, 12: 1597}


def _fused(name, form, n_w, n_layers, S, *, m=12, r=16, projection="direct", n_obs=9, P=9, per_sample=False, pins=False):
    return Fused(name, m, r, projection, n_obs, P, n_w, n_layers, S, per_sample, pins, form,
                 staged(n_layers, n_w, n_obs) if form == "one" else None, pre(n_layers) if form == "one" else None)


FUSED_CASES = (
    # one-sample form, staged
    _fused("one-staged-ref", "one", 50, 5, 4, r=33),
    _fused("one-staged-w16", "one", 16, 2, 3),
    _fused("one-staged-w17-tail1", "one", 17, 4, 3, per_sample=True),
    _fused("one-staged-w33", "one", 33, 4, 2),
    _fused("one-staged-w64", "one", 64, 3, 3),
    _fused("one-staged-L0", "one", 50, 0, 3),
    _fused("one-staged-w1", "one", 1, 4, 3),
    _fused("one-staged-L8-pre-edge", "one", 32, 8, 3),
    _fused("one-staged-pins", "one", 48, 2, 3, pins=True),
    _fused("one-staged-m8-S64", "one", 31, 4, 64, m=8, r=8),
    # one-sample form, unstaged
    _fused("one-unstaged-size-50x7", "one", 50, 7, 3),
    _fused("one-unstaged-align-15x3", "one", 15, 3, 3),
    _fused("one-unstaged-align-33x1", "one", 33, 1, 3, per_sample=True),
    _fused("one-unstaged-w63", "one", 63, 5, 2),
    # more than eight hidden layers: no register preload
    _fused("one-staged-L12-w32", "one", 32, 12, 3),
    _fused("one-staged-L9-w16", "one", 16, 9, 3, m=8, r=8),
    _fused("one-unstaged-reach-36x12", "one", 36, 12, 3),
    _fused("one-unstaged-L9-w50", "one", 50, 9, 3),
    _fused("one-unstaged-L9-w17-align", "one", 17, 9, 2),
    # five parameters
    _fused("one-P5", "one", 50, 5, 3, P=5),
    _fused("b8-P5", "b8", 17, 2, 5, P=5, projection="offline_online", per_sample=True),
    # batched, fused averages: S <= 64 (offline-online projection or a basis wider than 96) and S > 64
    _fused("b8-ref", "b8", 50, 5, 4, r=33, projection="offline_online"),
    _fused("b8-m8-w33", "b8", 33, 2, 3, m=8, r=16, projection="offline_online"),
    _fused("b8-m4-w17-S64", "b8", 17, 9, 64, m=4, r=8, projection="offline_online", per_sample=True),
    _fused("b8-pins", "b8", 64, 1, 2, m=4, r=8, projection="offline_online", pins=True),
    _fused("b1-ref-S65", "b1", 50, 5, 65, r=33),
    _fused("b1-S130-w31", "b1", 31, 12, 130, m=4, r=8, per_sample=True),
    _fused("b1-S130-w1-L0", "b1", 1, 0, 130, m=4, r=8),
    _fused("b1-pins-S65", "b1", 48, 2, 65, m=4, r=8, projection="offline_online", pins=True),
    # forty point observations: n_obs > 15 has no one-sample form
    _fused("b8-obs40", "b8", 50, 5, 3, n_obs=40, r=33),
    _fused("b8-obs40-w15", "b8", 15, 1, 64, m=4, r=8, n_obs=40, per_sample=True),
    _fused("b1-obs40", "b1", 33, 2, 70, m=4, r=8, n_obs=40),
)
FUSED_BY_NAME = {c.name: c for c in FUSED_CASES}
# a sample alone = the same sample in a batch of the same form; two runs; NaN containment: one row per form and staging
FUSED_BITWISE = ("one-staged-ref", "one-unstaged-size-50x7", "one-unstaged-reach-36x12", "one-P5", "b8-ref", "b8-obs40", "b1-ref-S65",
                 "b1-S130-w31")
FUSED_NAN = ("one-staged-ref", "one-unstaged-align-15x3", "one-staged-L12-w32", "b8-ref", "b8-obs40", "b1-ref-S65", "b1-obs40")
# the leapfrog form (finrom_hmc_leapfrog: one-sample form only): position update in front, momentum update and theta carry behind
LEAP_CASES = ("one-staged-ref", "one-staged-w17-tail1", "one-unstaged-size-50x7", "one-unstaged-reach-36x12", "one-staged-L12-w32",
              "one-staged-m8-S64", "one-P5")


@functools.lru_cache(maxsize=None)
def oracle_rig(m, r, n_obs):
    """(problem, POD basis of r columns from max(3 r, 40) nine-parameter snapshots, AffineROMOracle) -- the basis every fused row of
    this mesh and width shares with the device model.  Narrow bases (r <= 33) keep the reduced normal equations well conditioned,
    so that the float64 ROM's own rounding stays far below the fp32 network's (tests/test_mlp_host.py checks it row by row)."""
    from oracle import fin_oracle as O
    prob = O.FinProblem(m)
    fo = O.FinOracle(prob, external_obs=(n_obs == 40))
    rng = np.random.default_rng(1)
    Y = np.array([fo.forward(fo.nine_param_to_function(rng.uniform(0.1, 3.5, 9))) for _ in range(max(3 * r, 40))])
    phi = O.pod_basis(Y, r)
    return prob, phi, O.AffineROMOracle(prob, phi, B_obs=fo.B_obs if n_obs == 40 else None)


def fused_refs(c, idx=None):
    """ref64 and host32 of a fused row at the samples idx (default: all) -> (K, data, {name: [len(idx), ...]}, same for host32)."""
    prob, phi, ro = oracle_rig(c.m, c.r, c.n_obs)
    model, K, data = fused_model(c), rom_inputs(MESH_N[c.m], c.S, seed=3), fused_data(c)
    kw = {}
    if c.P == 5:
        kw["E"], kw["Sop"] = five_parameters(ro.dsigma_dk)
    idx = range(c.S) if idx is None else idx
    out = {}
    for net in ("f64", "f32"):
        rows = [romml_ref(ro, model, K[s], data[s] if c.per_sample else data, net, **kw) for s in idx]
        out[net] = {k: np.array([r_[k] for r_ in rows]) for k in ("grad", "loss", "qoi_r", "e_nn")}
    return K, data, out["f64"], out["f32"]


def compared_samples(S):
    """The samples a fused row is compared at: all of a small batch; of a large one both ends and the neighbours of 64."""
    return list(range(S)) if S <= 8 else sorted({0, 1, S // 2, 62, 63, 64, S - 2, S - 1} & set(range(S)))


def fused_model(c):
    model = make_model(MESH_N[c.m], c.n_w, c.n_layers, c.n_obs, seed=23, pins=c.pins)
    model.head["W"] *= np.float32(0.1)                       # errors of a tenth of the observables' size
    model.head["b"] *= np.float32(0.1)
    return model


def fused_data(c, seed=0):
    rng = np.random.default_rng([seed, c.n_obs, c.S])
    return rng.uniform(0.2, 1.0, (c.S, c.n_obs) if c.per_sample else c.n_obs)


def five_parameters(S9):
    """A five-parameter drive of the nine sub-fin conductivities for the P = 5 rows: E [9, 5] ties the sub-fins in five groups
    (0-1, 2-3, 4-5, 6-7, 8) and Sop5 = the groups' mean averages, so that E Sop5 k stays positive for a positive field."""
    E = np.zeros((9, 5))
    for i in range(9):
        E[i, i // 2] = 1.0
    Sop5 = np.stack([S9[[i for i in range(9) if i // 2 == j]].mean(axis=0) for j in range(5)])
    return E, Sop5
