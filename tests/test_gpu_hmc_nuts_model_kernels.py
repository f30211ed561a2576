"""The leaf-at-a-time No-U-turn kernels through the C ABI (finrom_hmc_nuts_begin / _leaf / _end, csrc/hmc_nuts_model.hip).

The model is a NumPy function on the host between two launches: it reads Kq[0] (or theta_out), writes loss, info and grad (or g_theta).
The statement is nuts.LeafMachine in the kernels' arithmetic (nuts_cases.fma, block_dot_1024), fed the same evaluations: after EVERY
leaf Kq[0] and active are compared, after finrom_hmc_nuts_end the raw bytes of K, dU, U, state_loss, Kq[0], the tree row, accept_stat,
accept and the trace row.  Every compared transition decides none of its comparisons closer than nuts_cases.MARGIN (a condition on
the inputs, asserted for every case; the statement runs without a device, so the cases were chosen on the CPU).
Second: with finrom_mlp_misfit_grad as the model the three calls leave finrom_hmc_nuts_ml's bytes."""
import ctypes
import functools

import numpy as np
import pytest

import hmc_cases as H
import hmc_ml_cases as MC
import hmc_model_cases as M
import nuts_cases as NC

pytestmark = pytest.mark.gpu
ROWS = 6                                              # rows of tree / accept_stat: pt = 4 writes row 4
STATE = ("K", "U", "dU", "Kq0", "accept", "loss", "info")     # what the calls or the host model move, beside trace, jt and pt
FIXED = 13                                            # arrays [C x n] of the workspace beside the 2 max_depth checkpoint arrays


def _lib():
    from bayesianinferencedl_amd import _ffi
    return _ffi.lib()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- the host model ------------------------------------------------------------------------------------------------------------------------
def stiffness(n):
    return np.logspace(np.log10(0.5), np.log10(50.0), n) if n > 1 else np.array([5.0])


def toy(n):
    """loss = 1/2 sum s_i k_i^2, grad = s k: rows independent."""
    s = stiffness(n)
    return lambda X: (0.5 * np.sum(s * X * X, axis=1), s * X)


INJECT = {"info": lambda ls: (ls, 3), "nan": lambda ls: (np.nan, 0), "huge": lambda ls: (ls + 2000.0, 0)}


def build_case(n, C, eps, seed=0):
    """The state before a transition (hmc_cases.begin_case's conventions: mean != 0, c_pri != 1, jt = 1, pt = 4) with c_lik = 1 and
    a position of the toy's own scale; U and dU belong to K in the kernels' arithmetic; the evaluation's loss and info not yet written.
    -> (case for hmc_cases.DeviceState, state_loss [C])."""
    s = H.begin_case(n, C, 1, seed=seed)
    rng = np.random.default_rng([n, C, seed, 31])
    s.update(eps=eps, c_lik=1.0, mean=0.1 * rng.standard_normal((C, n)), P=rng.standard_normal((C, n)), dUq=rng.standard_normal((C, n)),
             H0=rng.standard_normal(C), loss=np.full(C, np.nan), info=np.full(C, 7, np.int32))
    s["K"] = s["mean"] + rng.standard_normal((C, n)) / np.sqrt(stiffness(n) + s["c_pri"])
    loss, grad = toy(n)(s["K"])
    s = NC.with_potential(s, loss, grad)
    state_loss = s["loss"]
    return dict(s, loss=np.full(C, np.nan)), state_loss


class Rig:
    """A case on the device with the tree's descriptor: every buffer with hmc_cases.PAD sentinels behind its end."""

    def __init__(self, case, state_loss, seeds, proposal0, depth, P=0):
        import torch
        from bayesianinferencedl_amd import _ffi
        self.L, self.case, self.C, self.n, self.depth, self.P = _lib(), case, case["C"], case["n"], depth, P
        C, n = self.C, self.n
        self.dev = H.DeviceState(case)
        self.ws_doubles = self.L.finrom_hmc_nuts_ws_bytes(C, n, depth) // 8
        assert self.ws_doubles * 8 == (FIXED + 2 * depth) * C * n * 8 + C * 64 + C * 32
        nan_pad = np.full(H.PAD, np.nan)
        self.up = dict(ws=np.full(self.ws_doubles + H.PAD, np.nan), tree=np.full(ROWS * C * 4 + H.PAD, H.SENTINEL, np.int32),
                       stat=np.full(ROWS * C + H.PAD, np.nan), active=np.full(C + H.PAD, H.SENTINEL, np.int32),
                       state_loss=np.concatenate([state_loss, nan_pad]), grad=np.full(C * n + H.PAD, np.nan),
                       gth=np.full(C * max(P, 1) + H.PAD, np.nan), theta=np.full(C * max(P, 1) + H.PAD, np.nan),
                       seeds=np.asarray(seeds, dtype=np.uint64).view(np.int64).copy())
        self.t = {k: torch.from_numpy(v.copy()).cuda() for k, v in self.up.items()}
        p = {k: t.data_ptr() for k, t in self.t.items()}
        self.tr = _ffi.HmcNutsTree(ws=p["ws"], seeds=p["seeds"], proposal0=proposal0, max_depth=depth, state_loss=p["state_loss"],
                                   tree=p["tree"], accept_stat=p["stat"], active=p["active"])
        self.map = (None, None, 0, None)

    def set_map(self, A, theta0):
        import torch
        self.A_t = torch.from_numpy(np.ascontiguousarray(A)).cuda()
        self.th0_t = torch.from_numpy(np.ascontiguousarray(theta0)).cuda() if theta0 is not None else None
        self.map = (self.A_t.data_ptr(), self.th0_t.data_ptr() if theta0 is not None else None, A.shape[0], self.t["theta"].data_ptr())

    def begin(self):
        rc = self.L.finrom_hmc_nuts_begin(ctypes.byref(self.dev.st), ctypes.byref(self.tr), *self.map, _stream())
        assert rc == 0, self.L.finrom_last_error()

    def leaf(self, loss, info, grad=None, gth=None):
        """The host model's evaluation goes up, then ONE finrom_hmc_nuts_leaf."""
        import torch
        C = self.C
        self.dev.t["loss"][:C].copy_(torch.from_numpy(np.ascontiguousarray(loss, dtype=np.float64)))
        self.dev.t["info"][:C].copy_(torch.from_numpy(np.ascontiguousarray(info, dtype=np.int32)))
        if grad is not None:
            self.t["grad"][:C * self.n].copy_(torch.from_numpy(np.ascontiguousarray(grad, dtype=np.float64).reshape(-1)))
        else:
            self.t["gth"][:C * self.P].copy_(torch.from_numpy(np.ascontiguousarray(gth, dtype=np.float64).reshape(-1)))
        rc = self.L.finrom_hmc_nuts_leaf(ctypes.byref(self.dev.st), ctypes.byref(self.tr), self.t["grad"].data_ptr() if grad is not None else None,
                                         self.t["gth"].data_ptr() if grad is None else None, *self.map, _stream())
        assert rc == 0, self.L.finrom_last_error()

    def end(self):
        rc = self.L.finrom_hmc_nuts_end(ctypes.byref(self.dev.st), ctypes.byref(self.tr), _stream())
        assert rc == 0, self.L.finrom_last_error()

    def get(self, name):
        """A buffer now, without its padding, in its shape."""
        C, n = self.C, self.n
        if name in self.t:
            shape = dict(tree=(ROWS, C, 4), stat=(ROWS, C), active=(C,), state_loss=(C,), theta=(C, max(self.P, 1)), ws=(self.ws_doubles,))[name]
            return self.t[name].cpu().numpy()[:-H.PAD].reshape(shape)
        return self.dev.t[name].cpu().numpy()[:-H.PAD].reshape(np.shape(self.case[name]))

    def chain_ws(self, c):
        """Chain c's part of the workspace, as bytes."""
        C, n, A = self.C, self.n, FIXED + 2 * self.depth
        ws = self.get("ws")
        ints = ws[A * C * n + 8 * C:].view(np.int32).reshape(C, 8)
        return ws[:A * C * n].reshape(A, C, n)[:, c].tobytes() + ws[A * C * n:A * C * n + 8 * C].reshape(C, 8)[c].tobytes() + ints[c].tobytes()

    def assert_padding(self):
        for name, up in self.up.items():
            if name != "seeds":
                assert H.same_bits(self.t[name].cpu().numpy()[-H.PAD:], up[-H.PAD:]), (name, "written behind its end")


def transition(spec, chains=None, subset=None, freeze=False):
    """ONE transition on the device under the host model, leaf by leaf beside the statement.  spec: dict(n, C, eps, depth, proposal0,
    seed, inject {(chain, leaf): kind}, map (P, with theta0) or None).  chains: which chains the statement restates (None: all).
    subset: run this one chain ALONE (C = 1) with its own row of everything.  freeze: ended chains' bytes are compared across every
    later leaf call.  -> (rig after finrom_hmc_nuts_end, {chain: the statement's result}, rounds)."""
    from bayesianinferencedl_amd.bayesian_inference import nuts as N
    n, C, eps, depth, proposal0 = spec["n"], spec["C"], spec["eps"], spec["depth"], spec["proposal0"]
    case, state_loss = build_case(n, C, eps, spec.get("seed", 0))
    seeds = np.array([NC.KERNEL_SEEDS0 + c for c in range(C)], dtype=np.uint64)
    ids = list(range(C))                                             # the chains' names in the spec (inject's keys)
    if subset is not None:
        case, state_loss, seeds, ids, C = H.chain_subset(case, subset), state_loss[subset:subset + 1], seeds[subset:subset + 1], [subset], 1
    f, amap = toy(n), spec.get("map")
    if amap is not None:                                             # a model that sees the field through theta = theta0 + A k alone
        A, theta0, _, _ = M.map_case(n, spec["C"], amap[0], seed=3)
        A = A / np.sqrt(n)
        theta0 = theta0 if amap[1] else None
        rq = np.random.default_rng([amap[0], 17])                    # loss = 1/2 |B theta - d|^2, g_theta = B^T (B theta - d)
        Bq, dq = rq.standard_normal((amap[0], amap[0])) / np.sqrt(amap[0]), rq.standard_normal(amap[0])
    rig = Rig(case, state_loss, seeds, proposal0, depth, P=amap[0] if amap else 0)
    if amap is not None:
        rig.set_map(A, theta0)
    restate = range(C) if chains is None or subset is not None else chains
    pt, jt = case["pt"], case["jt"]
    ms = {}
    for c in restate:
        ms[c] = N.LeafMachine(seed=int(seeds[c]), proposal=proposal0 + pt, eps=eps, c_lik=case["c_lik"], c_pri=case["c_pri"],
                              mean=case["mean"][c], max_depth=depth, fma=NC.fma, dot=NC.block_dot_1024)
        ms[c].begin(case["K"][c], case["U"][c], case["dU"][c], state_loss[c], case["P_block"][jt, c])
    rig.begin()
    assert np.all(rig.get("active") == 1)
    rounds, frozen = 0, {}
    while True:
        X, active = rig.get("Kq0"), rig.get("active")
        for c, m in ms.items():
            assert active[c] == int(m.active) and H.same_bits(X[c], m.position), (spec, c, rounds)
        if freeze:
            for c in range(C):
                if not active[c]:
                    now = rig.chain_ws(c) + b"".join(rig.get(k)[c].tobytes() for k in ("K", "dU", "U", "Kq0", "state_loss"))
                    assert frozen.setdefault(c, now) == now, (spec, c, rounds, "an ended chain's bytes moved")
        if not active.any():
            break
        rounds += 1
        assert rounds <= 2 ** depth - 1
        if amap is None:
            loss, grad = f(X)
        else:
            theta = rig.get("theta")
            for c, m in ms.items():                                  # finrom_hmc_drift's contract in the 1024-thread order, ONE rounded addition
                want = np.array([(0.0 if theta0 is None else theta0[q]) + NC.block_dot_1024(A[q], m.position) for q in range(amap[0])])
                assert H.same_bits(theta[c], want), (spec, c, rounds)
            r = theta @ Bq.T - dq
            loss, gth = 0.5 * np.einsum("co,co->c", r, r), r @ Bq
        info = np.zeros(C, np.int32)
        for (c, leaf), kind in spec.get("inject", {}).items():
            if leaf == rounds and c in ids:
                i = ids.index(c)
                loss[i], info[i] = INJECT[kind](loss[i])
        if amap is None:
            rig.leaf(loss, info, grad=grad)
        else:
            rig.leaf(loss, info, gth=gth)
        for c, m in ms.items():
            if not m.active:
                continue
            if amap is None:
                g = grad[c]
            else:                                                    # fma-chained from 0 over p ascending, as finrom_hmc_kick maps it
                g = np.zeros(n)
                for q in range(amap[0]):
                    g = NC.fma(gth[c, q], A[q], g)
                ref, scale = M.map_gradient(gth[c:c + 1], A)
                assert np.all(np.abs(g - ref[0]) <= (amap[0] + 1) * H.U53 * scale[0])
            m.leaf(loss[c], g, info[c] != 0)
    rig.end()
    return rig, {c: m.result() for c, m in ms.items()}, rounds


def compare(rig, results, spec, first_leaf=()):
    """After finrom_hmc_nuts_end: the raw bytes against the statement, everything else as uploaded."""
    case = rig.case
    pt, C = case["pt"], rig.C
    got = {k: rig.get(k) for k in ("K", "dU", "U", "Kq0", "state_loss", "accept", "trace", "tree", "stat", "jt", "pt")}
    margin = np.inf
    for c, r in results.items():
        tag = (spec, c, r.tree.tolist())
        assert np.array_equal(got["tree"][pt, c], r.tree), (tag, got["tree"][pt, c])
        for name, want in (("K", r.k), ("dU", r.dU), ("U", r.U), ("state_loss", r.loss), ("Kq0", r.k), ("accept", case["accept"][c] + r.moved)):
            assert H.same_bits(got[name][c], np.asarray(want, dtype=got[name].dtype)), (tag, name)
        assert H.same_bits(got["trace"][pt + 1, c], r.k), tag
        assert H.same_bits(got["stat"][pt, c], np.float64(r.accept_stat)), (tag, got["stat"][pt, c], r.accept_stat)
        margin = min(margin, r.margin)
    assert margin >= NC.MARGIN, (spec, margin)                       # the condition on the inputs, for this case
    assert int(got["jt"]) == case["jt"] + 1 and int(got["pt"]) == pt + 1
    down = rig.dev.download()
    rig.dev.assert_bits(down, {}, skip=STATE + ("trace", "jt", "pt"))      # mean, Kq1, P, dUq, H0, the draws: as uploaded
    for name in STATE + ("trace",):
        assert H.same_bits(down[name][-H.PAD:], rig.dev.up[name][-H.PAD:]), (name, "written behind its end")
    rig.assert_padding()
    keep = np.ones(H.TRACE_ROWS, bool)
    keep[pt + 1] = False
    assert H.same_bits(got["trace"][keep], case["trace"][keep])
    keep = np.ones(ROWS, bool)
    keep[pt] = False
    assert np.all(got["tree"][keep] == H.SENTINEL) and np.all(np.isnan(got["stat"][keep])) and np.all(rig.get("active") == 0)
    return margin


# n: one element, a partial pass, exactly one and one-plus-one passes of 1024 threads, more; max_depth <= 5 at n = 37 and <= 3 above
CASES = {
    "n37-C4-deep": dict(n=37, C=4, eps=0.08, depth=5, proposal0=0),
    "n37-C4-turns": dict(n=37, C=4, eps=0.2, depth=5, proposal0=0, seed=1),
    "n37-C4-unstable": dict(n=37, C=4, eps=0.3, depth=5, proposal0=0),
    "n37-C4-injected": dict(n=37, C=4, eps=0.05, depth=4, proposal0=1 << 40, inject={(1, 1): "info", (2, 2): "nan", (3, 3): "huge", (0, 1): "nan"},
                            seed=2),
    "n1-C1": dict(n=1, C=1, eps=0.4, depth=3, proposal0=0),
    "n1024-C4": dict(n=1024, C=4, eps=0.1, depth=3, proposal0=0),
    "n1025-C1": dict(n=1025, C=1, eps=0.05, depth=3, proposal0=1 << 40),
    "n1597-C4": dict(n=1597, C=4, eps=0.12, depth=3, proposal0=1 << 40),
    "n37-P9-theta0": dict(n=37, C=4, eps=0.1, depth=4, proposal0=0, map=(9, True)),
    "n1025-P16": dict(n=1025, C=4, eps=0.1, depth=3, proposal0=1 << 40, map=(16, False)),
}
WIDE = {"n37-C80": (dict(n=37, C=80, eps=0.12, depth=3, proposal0=1 << 40), (0, 41, 79)),
        "n1025-C80": (dict(n=1025, C=80, eps=0.1, depth=2, proposal0=0), (0, 41, 79))}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Runs CASES[name] with every assertion -> [(reason, moved, first-leaf divergence, turn levels, leaves)] of its chains, rounds."""
    spec = CASES[name]
    rig, results, rounds = transition(spec, freeze=spec["n"] == 37)
    margin = compare(rig, results, spec)
    seen = tuple((int(r.reason), int(r.moved), r.steps, r.turn_levels) for r in results.values())
    print(f"NUTS leaf kernels {name}: rounds {rounds}, smallest decision margin {margin:.3e}, (reason, moved, leaves, turn levels) {seen}")
    return seen, rounds, results, rig


@pytest.mark.parametrize("name", list(CASES))
def test_a_transition_leaf_by_leaf_is_the_leaf_machine_bit_for_bit(name):
    seen, rounds, results, rig = _case(name)
    assert rounds == max(s[2] for s in seen)
    spec = CASES[name]
    for (c, leaf), kind in spec.get("inject", {}).items():           # an injected divergence ends the chain at that leaf, reason 3
        if all(not (c2 == c and l2 < leaf) for (c2, l2) in spec["inject"]):
            assert results[c].reason == 3 and results[c].steps == leaf, (c, leaf, kind, results[c].tree)
    for c, r in results.items():
        if r.reason == 3 and r.steps == 1:                           # a divergence at the very first leaf: the state's bytes are unchanged
            for k in ("K", "dU", "U"):
                assert H.same_bits(rig.get(k)[c], np.asarray(rig.case[k])[c]), (name, c, k)
            assert r.moved == 0 and rig.get("tree")[rig.case["pt"], c].tolist() == [0, 1, 3, 0] and rig.get("stat")[rig.case["pt"], c] == 0.0


def test_the_cases_cover_every_branch():
    seen = [s for name in CASES for s in _case(name)[0]]
    assert {s[0] for s in seen} == {0, 1, 2, 3} and {s[1] for s in seen} == {0, 1}, sorted(set(seen))
    assert max(s[3] for s in seen) >= 2                              # a sub-tree's turn spanning more than two leaves
    assert any(s[0] == 3 and s[2] == 1 for s in seen)                # a divergence at the very first leaf
    kinds = {kind for name in CASES for kind in CASES[name].get("inject", {}).values()}
    assert kinds == {"info", "nan", "huge"}
    assert any(len({s[2] for s in _case(name)[0]}) > 1 for name in CASES if CASES[name]["n"] == 37)      # chains ending at different rounds


@pytest.mark.parametrize("name", list(WIDE))
def test_eighty_chains_three_restated_and_every_one_equal_to_itself_run_alone(name):
    spec, chains = WIDE[name]
    rig, results, rounds = transition(spec, chains=chains)
    compare(rig, results, spec)
    pt = rig.case["pt"]
    names = ("K", "dU", "U", "Kq0", "state_loss", "accept")
    wide = {k: rig.get(k) for k in names + ("tree", "stat", "trace")}
    for c in range(spec["C"]):
        one, _, _ = transition(spec, subset=c)
        for k in names:
            assert H.same_bits(wide[k][c], one.get(k)[0]), (name, c, k)
        assert H.same_bits(wide["tree"][pt, c], one.get("tree")[pt, 0]) and H.same_bits(wide["stat"][pt, c], one.get("stat")[pt, 0]), (name, c)
        assert H.same_bits(wide["trace"][pt + 1, c], one.get("trace")[pt + 1, 0]), (name, c)


# ---- with finrom_mlp_misfit_grad as the model: finrom_hmc_nuts_ml's bytes ------------------------------------------------------------------
@pytest.mark.parametrize("shape", MC.SHAPES[:2], ids=lambda s: "-".join(map(str, s)))
def test_with_the_surrogate_as_the_model_the_three_calls_leave_the_one_launch_kernels_bytes(shape):
    import torch
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    C, eps, depth, transitions = 4, 0.2, 4, 3
    mlp = DeviceErrorModel(MC.kernel_model(shape))
    data_t = torch.from_numpy(MC.kernel_data(shape, C, True)).cuda()
    s = NC.kernel_state(shape, C, eps)
    r0 = mlp.misfit_grad(torch.from_numpy(s["K"]).cuda(), data_t)
    assert mlp.last_form() == 1
    s = NC.with_potential(s, r0["loss"].cpu().numpy(), r0["grad"].cpu().numpy())
    s["jt"], s["pt"] = 0, 0
    seeds = [NC.KERNEL_SEEDS0 + c for c in range(C)]
    L = _lib()
    # the one-launch kernel: `transitions` calls
    ref = H.DeviceState(s)
    seeds_t = torch.from_numpy(np.asarray(seeds, dtype=np.uint64).view(np.int64).copy()).cuda()
    tree_r, stat_r = torch.zeros(ROWS, C, 4, dtype=torch.int32, device="cuda"), torch.zeros(ROWS, C, dtype=torch.float64, device="cuda")
    # the three calls: the state's misfit apart from the evaluation's
    rig = Rig(dict(s, loss=np.full(C, np.nan)), s["loss"], seeds, 5, depth)
    n = shape[0]
    for q in range(transitions):
        assert L.finrom_hmc_nuts_ml(mlp._h, ctypes.byref(ref.st), seeds_t.data_ptr(), 5, depth, data_t.data_ptr(), 1, tree_r.data_ptr(),
                                    stat_r.data_ptr(), _stream()) == 0, L.finrom_last_error()
        rig.begin()
        rounds = 0
        while rig.get("active").any():
            rounds += 1
            assert rounds <= 2 ** depth - 1
            r = mlp.misfit_grad(rig.dev.t["Kq0"][:C * n].reshape(C, n), data_t)
            assert mlp.last_form() == 1
            loss = r["loss"].cpu().numpy()
            rig.leaf(loss, (~np.isfinite(loss)).astype(np.int32), grad=r["grad"].cpu().numpy())
        rig.end()
        want = ref.download()
        for name in ("K", "U", "dU"):
            assert H.same_bits(rig.get(name), ref.body(want, name)), (shape, q, name)
        assert H.same_bits(rig.get("state_loss"), ref.body(want, "loss")), (shape, q)
        assert H.same_bits(rig.get("tree")[q], tree_r[q].cpu().numpy()) and H.same_bits(rig.get("stat")[q], stat_r[q].cpu().numpy()), (shape, q)
        assert H.same_bits(rig.get("accept"), ref.body(want, "accept")) and H.same_bits(rig.get("Kq0"), ref.body(want, "Kq0"))
    assert tree_r[:transitions, :, 1].max() > 1
