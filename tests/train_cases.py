"""Shared cases and helpers of the trainer's tests (csrc/mlp_train.hip): tests/test_gpu_train.py at workload shapes,
tests/test_gpu_train_edges.py at the kernels' edges, tests/test_train_edges_host.py for the soundness of the edge cases.

Yardstick: ResBnFcModel.train_gradients / evaluate / adam_apply in float64 (tests/test_train_host.py ties them to torch autograd).
Allowance (the project's rule): per compared quantity the device may deviate from the yardstick by at most
16 x what the same host statement in float32 deviates on the same inputs, with a floor of 4 ulp of fp32; deviations are relative
to the tensor's largest entry, for the biases whose exact gradient is zero to the step's largest gradient.

Every case's inputs (X, Y) are rounded to fp32 first, so yardstick, host-fp32 statement and device see the same numbers."""
import copy

import numpy as np

from bayesianinferencedl_amd.deep_learning.dl_model import ResBnFcModel, TREE_KEYS

ULP32 = float(np.finfo(np.float32).eps)
FACTOR = 16                                                        # sqrt(K) ceiling between two fp32 orders of a sum
EXTRA = 37                                                         # max_batch = B + EXTRA: strides that are not the batch


def probe(n_in, S, n_out=9, seed=0):
    """Seeded synthetic pairs: fields exp(0.3 xi), targets 0.05 tanh(20 log(x) T), T = randn(n_in, n_out) / n_in."""
    rng = np.random.default_rng(seed)
    X = np.exp(0.3 * rng.standard_normal((S, n_in)))
    T = rng.standard_normal((n_in, n_out)) / n_in
    return X, 0.05 * np.tanh(20 * np.log(X) @ T)


def perturbed(n_in, n_w, L, n_out, seed=1):
    m = ResBnFcModel(n_in, n_out, L, n_w, seed)
    rng = np.random.default_rng(seed + 100)
    for u in m.units + [m.head]:
        u["gamma"] = rng.uniform(0.5, 1.5, u["gamma"].shape).astype(np.float32)
        u["beta"] = rng.normal(0, 0.3, u["beta"].shape).astype(np.float32)
        u["b"] = rng.normal(0, 0.1, u["b"].shape).astype(np.float32)
    m.b0 = rng.normal(0, 0.1, m.b0.shape).astype(np.float32)
    return m


def leaves(tree):
    """[(name, array, gradient zero in exact arithmetic?)]: gradients and, under mean / var, the batch statistics."""
    n = len(tree["layers"])
    out = [("W0", tree["W0"], False), ("b0", tree["b0"], True)]
    for i, u in enumerate(tree["layers"]):
        out += [(f"l{i}_{k}", u[k], k == "b" and i < n - 1) for k in TREE_KEYS]
    return [(nm, np.asarray(a, dtype=np.float64), z) for nm, a, z in out]


def deviations(tree, ref):
    """name -> max |a - ref| over the tensor, relative to the yardstick tensor's largest entry; for the biases whose gradient is
    zero in exact arithmetic, to the largest gradient of the step."""
    R = leaves(ref)
    gmax = max(np.abs(b).max() for nm, b, _ in R if not nm.endswith(("mean", "var")))
    return {nm: np.abs(a - b).max() / (gmax if z or np.abs(b).max() == 0 else np.abs(b).max())
            for (nm, a, z), (_, b, _) in zip(leaves(tree), R)}


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def step_deviations(res, ref):
    """(loss, MAPE, tree) against the yardstick's -> name -> relative deviation of every compared quantity: every gradient tensor,
    every layer's batch mean and variance, loss, MAPE."""
    d = deviations(res[2], ref[2])
    d["loss"] = abs(float(res[0]) - float(ref[0])) / abs(float(ref[0]))
    d["mape"] = abs(float(res[1]) - float(ref[1])) / abs(float(ref[1]))
    return d


def allowance(dev32):
    return {nm: max(FACTOR * v, 4 * ULP32) for nm, v in dev32.items()}


def factors(devd, dev32):
    """name -> the device's deviation as a multiple of the fp32 statement's (floored at a quarter ulp, where 16 x meets the 4 ulp
    floor); the rule allows FACTOR."""
    return {nm: devd[nm] / max(dev32[nm], ULP32 / 4) for nm in devd}


def worst(devd, dev32):
    f = factors(devd, dev32)
    nm = max(f, key=f.get)
    return nm, f[nm]


def bits(*arrays):
    """The uint32 / uint64 views of fp32 / fp64 arrays and scalars, concatenated as uint64: equal iff every bit is equal."""
    out = []
    for a in arrays:
        a = np.atleast_1d(np.asarray(a))
        assert a.dtype in (np.float32, np.float64), a.dtype
        out.append(np.ascontiguousarray(a).ravel().view(np.uint32 if a.dtype == np.float32 else np.uint64).astype(np.uint64))
    return np.concatenate(out)


def tree_bits(tree):
    return bits(ResBnFcModel.flatten(tree))


# ---- 1. the edge cases of one step -------------------------------------------------------------------------------------------------
# (name, n_in, B, n_w, L, n_out, max_batch, rows, the edges the row carries).  rows: "perm" B distinct rows of a pool of 2 B behind
# an offset of 7, in permuted order; "repeat" the same with every fifth index repeated.
# fwd0_kernel cuts K into 8 pieces of ceil(n_in / 4) steps: with nsteps < 8 (n_in < 29) pieces are empty; a piece's step count is
# 0, 1 or 2 up to n_in = 33 (the unroll-by-4 tail guard in the first pass), 5 or 6 at n_in = 165 (a second pass with a tail).
SHAPE_CASES = [
    ("min", 1, 2, 1, 0, 1, 2, "perm",
     "n_in = 1: seven empty K pieces, k < n_in guard, dw0 clamps 15 of 16 inputs; B = 2 the declared minimum (fwd0 clamps 14 rows "
     "of the wave); (n_w, n_out) = (1, 1); L = 0: the head is the only layer, gy0 takes the head's sums, dbpart has two slots"),
    ("b2_l1", 7, 2, 50, 1, 9, 2 + EXTRA, "perm",
     "B = 2 through one unit (batch normalisation over two rows, L <= 1); n_in = 7 (n_in % 4 = 3, n_in < 16); max_batch = B + 37"),
    ("b15_wide_out", 2, 15, 3, 1, 40, 15 + EXTRA, "perm",
     "B < 16: one wave, one clamped row; n_in = 2; (n_w, n_out) = (3, 40): n_out > n_w, the two row lengths of pack / unpack; "
     "L = 1; max_batch = B + 37: part0, tape, dWpart, dbpart strided by max_batch / max_tiles"),
    ("b17_full_width", 3, 17, 64, 2, 64, 17, "perm",
     "(n_w, n_out) = (64, 64): no padding at all; B = 17: B % 16 = 1, a wave with one valid row; n_in = 3; L = 2 (even)"),
    ("b31_l3", 5, 31, 50, 3, 9, 31 + EXTRA, "perm",
     "B = 31: one tile of 31 rows, nt = 1; dw0's b + 4u < B guard ends inside the first pass; n_in = 5; L = 3 (odd)"),
    ("b32_l0", 7, 32, 50, 0, 9, 32, "perm",
     "B = 32: exactly one full tile, nt = 1; L = 0 at full width (50, 9)"),
    ("b33_l8", 16, 33, 50, 8, 9, 33, "perm",
     "B = 33: nt = 2 and a last tile of ONE row (M2 = 0 in Chan's update); L = 8 = TRAIN_MAX_L; n_in = 16: dw0 without a clamp, "
     "fwd0 with four empty pieces"),
    ("b33_w1", 33, 33, 1, 1, 1, 33, "perm",
     "n_w = 1 under a full first layer (n_in = 33: nsteps = 9, no empty piece, k guard in the last step, dw0's third block holds "
     "one input)"),
    ("b63", 31, 63, 37, 3, 2, 63 + EXTRA, "perm",
     "B = 63: last tile of 31, last wave of 15 rows; n_in = 31: n_in % 4 = 3, n_in % 16 = 15; widths (37, 2)"),
    ("b64_narrow", 2, 64, 2, 2, 1, 64 + EXTRA, "perm",
     "B = 64: two full tiles, dw0 exactly two passes; n_out = 1 with n_w = 2"),
    ("b65", 33, 65, 50, 5, 9, 65, "perm",
     "B = 65: nt = 3, last tile of one row, dw0 a third pass of one row; the workload's widths and depth (50, 5, 9)"),
    ("b97_repeat", 33, 97, 50, 4, 9, 97 + EXTRA, "repeat",
     "B = 97: nt = 4, last tile of one row; repeated row indices; L = 4 (even); max_batch = B + 37: max_tiles 5 against nt 4"),
    ("k165", 165, 40, 50, 5, 9, 40, "perm",
     "n_in = 165: nsteps = 42, K pieces of 5 and 6 steps (the unroll's second pass with its s + u < s1 tail), n_in % 4 = 1; B = 40: "
     "dw0's second pass holds 8 rows"),
]
# One case perturbs values instead of shape, in two models on the shape (33, 97, 50, 2, 9):
#   "zeros":  rows 3 and 4 of W0 and a stripe of unit 1's W are 0.0 and -0.0 (the regulariser's sign term), a fifth of the targets
#             are exactly 0 (the max(|y|, 1e-7) clamp of MAPE);
#   "offset": b0 = 8 + 0.1 randn and W0 scaled so that the columns of y0 spread by OFFSET_SPREAD: mean / std = 160, what Chan's
#             update is for.  y0 is itself fp32, so its rounding (8 x 2^-24 against a spread of 0.05: 1e-5) sits in the first
#             layer's variance and in what depends on it; VALUE_BOUND instead of HOST32_BOUND holds there.
VALUE_CASES = [
    ("zeros", 33, 97, 50, 2, 9, 97, "perm", "exact zeros and -0.0 in regularised weights; targets exactly 0"),
    ("offset", 33, 97, 50, 2, 9, 97, "perm", "first layer's column mean 160 x its spread"),
]
CASES = SHAPE_CASES + VALUE_CASES
# Two rows whose y0 nearly agree in some column make the normalisation amplify that column's rounding: of the six pairs of b2_l1's
# pool the host statement in fp32 deviates by 2.1e-6 on this one and by up to 1.3e-5 on the others (HOST32_BOUND, condition (a)).
CHOSEN_ROWS = {"b2_l1": [10, 7]}
CASE_IDS = [c[0] for c in CASES]
OFFSET_MEAN, OFFSET_SPREAD = 8.0, 0.05
HOST32_BOUND, VALUE_BOUND = 1e-5, 2e-5
WIDTHS = sorted({(c[3], c[5]) for c in CASES})                      # every (n_w, n_out) of the table


class Case:
    """One row of the table, built: model (fp32 arrays), X [S, n_in] and Y [S, n_out] (fp32 values held in float64), rows [B]."""

    def __init__(self, row):
        self.name, self.n_in, self.B, self.n_w, self.L, self.n_out, self.max_batch, self.rows_kind, self.edges = row
        n_in, B = self.n_in, self.B
        self.S = 2 * B + 8
        rng = np.random.default_rng(1000 + CASE_IDS.index(self.name))
        self.model = perturbed(n_in, self.n_w, self.L, self.n_out)
        X, Y = probe(n_in, self.S, self.n_out)
        rows = 7 + rng.permutation(2 * B)[:B]                       # (rows - 1 and rows + 1 stay inside [0, S))
        if np.all(np.diff(rows) > 0):                               # (B = 2: a draw in ascending order is turned round)
            rows = rows[::-1].copy()
        rows = np.array(CHOSEN_ROWS.get(self.name, rows))
        if self.rows_kind == "repeat":
            rows[::5] = rows[1::5][:len(rows[::5])]
        self.rows = rows.astype(np.int64)
        if self.name == "zeros":
            m = self.model
            m.W0[3] = 0.0; m.W0[4] = -0.0; m.W0[10, ::2] = 0.0
            m.units[1]["W"][:, 5:8] = np.array([0.0, -0.0, 0.0], np.float32)
            Y = np.where(rng.random(Y.shape) < 0.2, 0.0, Y)
        if self.name == "offset":
            m = self.model
            scale = OFFSET_SPREAD / (X[self.rows] @ m.W0.astype(np.float64)).std(axis=0).mean()
            m.W0 = (m.W0 * scale).astype(np.float32)
            m.b0 = (OFFSET_MEAN + 0.1 * rng.standard_normal(self.n_w)).astype(np.float32)
        self.X = X.astype(np.float32).astype(np.float64)
        self.Y = Y.astype(np.float32).astype(np.float64)

    def statement(self, dtype, rows=None, X=None):
        """(loss, MAPE, tree) of the host statement in `dtype` on the case's batch (or on planted rows / inputs)."""
        rows = self.rows if rows is None else rows
        X = self.X if X is None else X
        l, p, g = self.model.train_gradients(X[rows], self.Y[rows], dtype)
        return float(l), float(p), g

    def planted(self):
        """name -> the unmodified fp64 statement on altered inputs: what a kernel that dropped the last row, skipped the last
        input column or read its rows one off would compute.  At B = 2 the statement has no batch of one row; there the fault is
        the last row read as a copy of the first (what a clamp to a valid row one too early gives)."""
        X0 = self.X.copy(); X0[:, -1] = 0.0
        short = self.rows[:-1] if self.B > 2 else np.array([self.rows[0], self.rows[0]])
        return {"last row dropped": self.statement(np.float64, rows=short),
                "last input column zeroed": self.statement(np.float64, X=X0),
                "rows shifted by one": self.statement(np.float64, rows=self.rows - 1)}


_built = {}


def case(name):
    """The built case, with its fp64 and host-fp32 statements computed once and shared (read-only)."""
    if name not in _built:
        c = Case(CASES[CASE_IDS.index(name)])
        c.ref64, c.ref32 = c.statement(np.float64), c.statement(np.float32)
        c.dev32 = step_deviations(c.ref32, c.ref64)
        _built[name] = c
    return _built[name]


def host32_bound(name):
    """What the host-fp32 deviation of every compared quantity of the case must stay under.  In the offset case every compared
    quantity sits behind the first normalisation, so all of them carry VALUE_BOUND."""
    return VALUE_BOUND if name == "offset" else HOST32_BOUND


def one_pass_variance32(c):
    """The offset case's y0 in fp32 and its biased variance as E[y^2] - mean^2 in float32: the planted fault Chan's update avoids."""
    y = c.X[c.rows].astype(np.float32) @ c.model.W0 + c.model.b0
    return (y * y).mean(axis=0, dtype=np.float32) - y.mean(axis=0, dtype=np.float32) ** 2


def embedded(model, n_w, n_out):
    """The same network inside widths (n_w, n_out): every added weight, gamma, beta and bias is zero (added moving variances are
    one, as created).  The added columns of y are then zero in every layer and every added gradient is zero."""
    big = ResBnFcModel(model.n_in, n_out, model.n_layers, n_w, seed=0)
    small, tree = model._tree(), big._tree()
    w, o = model.n_weights, model.n_out
    tree["W0"][...] = 0; tree["W0"][:, :w] = small["W0"]
    tree["b0"][...] = 0; tree["b0"][:w] = small["b0"]
    for i, (u, s) in enumerate(zip(tree["layers"], small["layers"])):
        cols = o if i == model.n_layers else w
        for k in ("gamma", "beta"):
            u[k][...] = 0; u[k][:w] = s[k]
        u["W"][...] = 0; u["W"][:w, :cols] = s["W"]
        u["b"][...] = 0; u["b"][:cols] = s["b"]
    return big


def cut(tree, model):
    """The block of a (wider) tree that the model's own tree occupies."""
    w, o, L = model.n_weights, model.n_out, model.n_layers
    out = {"W0": tree["W0"][:, :w], "b0": tree["b0"][:w], "layers": []}
    for i, u in enumerate(tree["layers"]):
        cols = o if i == L else w
        out["layers"].append({"gamma": u["gamma"][:w], "beta": u["beta"][:w], "mean": u["mean"][:w], "var": u["var"][:w],
                              "W": u["W"][:w, :cols], "b": u["b"][:cols]})
    return out


def outside_is_zero(tree, model):
    """Every entry of the (wider) tree outside the model's own block is zero."""
    rest = {"W0": np.array(tree["W0"]), "b0": np.array(tree["b0"]), "layers": [{k: np.array(u[k]) for k in TREE_KEYS} for u in tree["layers"]]}
    own = cut(rest, model)                                          # (views)
    own["W0"][...] = 0; own["b0"][...] = 0
    for u in own["layers"]:
        for k in TREE_KEYS:
            u[k][...] = 0
    return all(not np.any(a) for _, a, _ in leaves(rest))


# ---- 4. evaluation in inference form -----------------------------------------------------------------------------------------------
EVAL_S = 150
EVAL_MAX_BATCH = [(150, "one chunk"), (64, "64 + 64 + 22"), (149, "a tail chunk of one row"), (37, "four chunks + 2")]


def eval_model():
    """(33, 50, 3, 9) with moving statistics set directly: means N(0, 0.3), variances U(0.5, 1.5)."""
    m = perturbed(33, 50, 3, 9, seed=2)
    rng = np.random.default_rng(7)
    for u in m.units + [m.head]:
        u["mean"] = rng.normal(0, 0.3, u["mean"].shape).astype(np.float32)
        u["var"] = rng.uniform(0.5, 1.5, u["var"].shape).astype(np.float32)
    X, Y = probe(33, EVAL_S, 9, seed=3)
    return m, X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)


# ---- 5. a short run with changing batch sizes --------------------------------------------------------------------------------------
RUN_B, RUN_LR, RUN_MAX_BATCH = [65, 2, 33, 64, 31, 65], 1e-3, 65


def run_setup():
    """Model (33, 50, L = 1, 9), data, and each step's rows (a fresh draw from the pool per step)."""
    m = perturbed(33, 50, 1, 9, seed=3)
    X, Y = probe(33, 140, 9, seed=4)
    rng = np.random.default_rng(11)
    rows = [rng.permutation(140)[:B].astype(np.int64) for B in RUN_B]
    return m, X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64), rows


def run_host(dtype):
    """The run as train_gradients / adam_apply in `dtype` -> (per-step (loss, MAPE, tree), the model afterwards, the start)."""
    m, X, Y, rows = run_setup()
    start = copy.deepcopy(m)
    m._cast(np.dtype(dtype).type)
    steps = []
    for i, r in enumerate(rows):
        l, p, g = m.train_gradients(X[r], Y[r], dtype)
        steps.append((float(l), float(p), g))
        m.adam_apply(g, i + 1, RUN_LR)
    return steps, m, start


def stat_deviations(res, ref):
    """Loss and every layer's batch mean and variance of one step against the yardstick's."""
    d = {nm: v for nm, v in deviations(res[2], ref[2]).items() if nm.endswith(("mean", "var"))}
    d["loss"] = abs(res[0] - ref[0]) / abs(ref[0])
    return d


NOISE_BIASES = lambda name, L: name == "b0" or (name.endswith("_b") and int(name[1:name.index("_")]) < L)


def param_deviations(model, ref, start):
    """After the run: name -> deviation of every parameter and moving statistic from the fp64 run's, relative to the tensor's
    largest entry; for b0 and the units' b (they move on rounding noise by design) to the run's largest parameter change."""
    R, S0 = leaves(ref._tree()), leaves(start._tree())
    moved = max(np.abs(b - s).max() for (nm, b, _), (_, s, _) in zip(R, S0) if not nm.endswith(("mean", "var")))
    L = model.n_layers
    return {nm: np.abs(a - b).max() / (moved if NOISE_BIASES(nm, L) else np.abs(b).max())
            for (nm, a, _), (_, b, _) in zip(leaves(model._tree()), R)}
