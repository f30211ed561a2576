"""The No-U-turn transition on the device (finrom_hmc_nuts_ml, csrc/hmc_nuts.hip; hmc.py model="ml" with nuts=).

Kernel, through the C ABI (cases and arithmetic: tests/nuts_cases.py): a transition is nuts.transition_iterative bit for bit when the
statement takes each leaf's loss and gradient from the device's own finrom_mlp_misfit_grad, its fused multiply-adds exactly and its sums
in block_sum_1024's order; a chain's bits do not depend on its neighbours; a chain with a NaN diverges at its first leaf, keeps its
state and disturbs nobody; what the entry point refuses it refuses before a launch, a first call with a new C inside a capture included.
Chains: run_chains_device(nuts=) against run_chains(nuts=) over the same device calls, both priors, graph and stream order, any block,
with stats=."""
import ctypes
import functools

import numpy as np
import pytest

import hmc_cases as H
import hmc_ml_cases as MC
import nuts_cases as NC
import surrogate_cases as SC

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -1, -4
ROWS = 6                                              # rows of tree / accept_stat: state_case's pt = 4 writes row 4
STATE = ("K", "U", "dU", "loss", "Kq0", "accept")     # what a transition moves, beside the trace row, the counters and its records


def _id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _rig(shape):
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    model = MC.kernel_model(shape)
    return model, DeviceErrorModel(model)


def _lib():
    from bayesianinferencedl_amd import _ffi
    return _ffi.lib()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _evaluator(mlp, data_row):
    """value_and_grad(K [1, n]) from the device's own finrom_mlp_misfit_grad in its per-sample form."""
    import torch

    def f(K):
        r = mlp.misfit_grad(torch.from_numpy(np.ascontiguousarray(K)).cuda(), data_row)
        assert mlp.last_form() == 1
        loss = r["loss"].cpu().numpy()
        return loss, r["grad"].cpu().numpy(), ~np.isfinite(loss)
    return f


def _case(shape, C, eps, mlp, data_t, seed=0):
    """The state before a transition, its potential and gradient the device's own at K (row by row: the per-sample form)."""
    s = NC.kernel_state(shape, C, eps, seed=seed)
    ev = [_evaluator(mlp, data_t[c])(s["K"][c:c + 1]) for c in range(C)]
    return NC.with_potential(s, np.array([e[0][0] for e in ev]), np.stack([e[1][0] for e in ev]))


class _Run:
    """One finrom_hmc_nuts_ml call on a case: the download, tree [ROWS, C, 4] and accept_stat [ROWS, C] with their padding."""

    def __init__(self, case, mlp, data_t, seeds, proposal0, depth, expect=0):
        import torch
        C = case["C"]
        self.dev = H.DeviceState(case)
        self.tree_up = np.full(ROWS * C * 4 + H.PAD, H.SENTINEL, np.int32)
        self.stat_up = np.full(ROWS * C + H.PAD, np.nan)
        tree_t, stat_t = torch.from_numpy(self.tree_up.copy()).cuda(), torch.from_numpy(self.stat_up.copy()).cuda()
        seeds_t = torch.from_numpy(np.asarray(seeds, dtype=np.uint64).view(np.int64).copy()).cuda()
        self.rc = _lib().finrom_hmc_nuts_ml(mlp._h, ctypes.byref(self.dev.st), seeds_t.data_ptr(), proposal0, depth, data_t.data_ptr(),
                                            1 if data_t.ndim == 2 else 0, tree_t.data_ptr(), stat_t.data_ptr(), _stream())
        assert self.rc == expect, (self.rc, _lib().finrom_last_error())
        self.got = self.dev.download()
        self.tree_all, self.stat_all = tree_t.cpu().numpy(), stat_t.cpu().numpy()
        self.tree, self.stat = self.tree_all[:-H.PAD].reshape(ROWS, C, 4), self.stat_all[:-H.PAD].reshape(ROWS, C)

    def body(self, name):
        return self.dev.body(self.got, name)


def _assert_nothing_else_moved(run, case):
    """Everything a transition does not write is as uploaded, and nothing is written behind any buffer's end or in another row."""
    pt = case["pt"]
    run.dev.assert_bits(run.got, {"jt": np.array(case["jt"] + 1), "pt": np.array(pt + 1)}, skip=STATE + ("trace",))
    for name in STATE + ("trace",):
        assert H.same_bits(run.got[name][-H.PAD:], run.dev.up[name][-H.PAD:]), (name, "written behind its end")
    keep = np.ones(H.TRACE_ROWS, bool)
    keep[pt + 1] = False
    assert H.same_bits(run.body("trace")[keep], case["trace"][keep])
    assert H.same_bits(run.tree_all[-H.PAD:], run.tree_up[-H.PAD:]) and H.same_bits(run.stat_all[-H.PAD:], run.stat_up[-H.PAD:])
    keep = np.ones(ROWS, bool)
    keep[pt] = False
    assert np.all(run.tree[keep] == H.SENTINEL) and np.all(np.isnan(run.stat[keep]))


# ---- 8. a transition is its statement, bit for bit ------------------------------------------------------------------------------------------
def _assert_same_chain(run, c, one, pt, tag):
    """Chain c of `run` has the bytes of the same chain run alone (C = 1): state, trace row, tree, accept_stat."""
    for name in STATE:
        assert H.same_bits(run.body(name)[c], one.body(name)[0]), (tag, c, name)
    assert H.same_bits(run.body("trace")[pt + 1, c], one.body("trace")[pt + 1, 0]), (tag, c)
    assert H.same_bits(run.tree[pt, c], one.tree[pt, 0]) and H.same_bits(run.stat[pt, c], one.stat[pt, 0]), (tag, c)


@functools.lru_cache(maxsize=None)
def _kernel_case(index):
    """Runs case `index` of NC.KERNEL_CASES with every assertion of test 8 -> [(stop reason, moved)] of the restated chains.  Cached: the
    coverage test below reads the same runs, and makes them itself when it is selected alone."""
    import torch
    from bayesianinferencedl_amd.bayesian_inference import nuts as N
    shape, C, eps, depth, proposal0, chains = NC.KERNEL_CASES[index]
    model, mlp = _rig(shape)
    data = MC.kernel_data(shape, C, True)
    data_t = torch.from_numpy(data).cuda()
    case = _case(shape, C, eps, mlp, data_t)
    seeds = [NC.KERNEL_SEEDS0 + c for c in range(C)]
    run = _Run(case, mlp, data_t, seeds, proposal0, depth)
    _assert_nothing_else_moved(run, case)
    pt, margin, seen = case["pt"], np.inf, []
    for c in (range(C) if chains is None else chains):
        r = N.transition_iterative(_evaluator(mlp, data_t[c]), case["K"][c], case["U"][c], case["dU"][c], case["loss"][c],
                                   case["P_block"][case["jt"], c], seed=seeds[c], proposal=proposal0 + pt, eps=eps, c_lik=case["c_lik"],
                                   c_pri=case["c_pri"], mean=case["mean"][c], max_depth=depth, fma=NC.fma, dot=NC.block_dot_1024)
        margin = min(margin, r.margin)
        seen.append((int(r.reason), int(r.moved)))
        tag = (shape, C, c, r.tree.tolist())
        assert np.array_equal(run.tree[pt, c], r.tree), (tag, run.tree[pt, c])
        for name, want in (("K", r.k), ("U", r.U), ("dU", r.dU), ("loss", r.loss), ("Kq0", r.k), ("accept", case["accept"][c] + r.moved)):
            assert H.same_bits(run.body(name)[c], np.asarray(want, dtype=run.body(name).dtype)), (tag, name)
        assert H.same_bits(run.body("trace")[pt + 1, c], r.k), tag
        assert abs(run.stat[pt, c] - r.accept_stat) <= 1e-12 * abs(r.accept_stat), (tag, run.stat[pt, c], r.accept_stat)
        assert 1 <= r.steps <= 2 ** depth - 1
    if chains is not None:                                           # EVERY chain of the eighty against its own C = 1 run, on the device
        for c in range(C):
            one = _Run(H.chain_subset(case, c), mlp, torch.from_numpy(data[c:c + 1].copy()).cuda(), seeds[c:c + 1], proposal0, depth)
            _assert_same_chain(run, c, one, pt, (shape, C))
        seen += [(int(t[2]), int(t[3])) for t in run.tree[pt]]     # (what those runs confirm of the other chains' trees)
    print(f"NUTS kernel case {_id(shape)} C={C}: smallest decision margin {margin:.3e}, (reason, moved) {sorted(set(seen))}")
    assert margin >= NC.MARGIN                                       # the condition of test_nuts_host.py's test 3, on this run
    return tuple(seen)


@pytest.mark.parametrize("index", range(len(NC.KERNEL_CASES)), ids=[_id(k[:4]) for k in NC.KERNEL_CASES])
def test_a_transition_is_its_statement_bit_for_bit(index):
    """Per shape and C.  With C = 1 and 4 every chain is restated on the host; with C = 80 three chains are restated and ALL eighty are
    compared, on the raw bytes, with the same chain run alone (C = 1, the same seed, proposal and data row)."""
    assert len(_kernel_case(index)) >= 1


def test_the_kernel_cases_cover_every_stop_reason_and_both_values_of_moved():
    """Over the cases above: their cached runs, or its own when this test is selected alone.  Only restated chains count for the stop
    reasons' coverage."""
    seen = []
    for index, k in enumerate(NC.KERNEL_CASES):
        n_restated = k[1] if k[5] is None else len(k[5])
        seen += list(_kernel_case(index))[:n_restated]
    assert {r for r, _ in seen} == {0, 1, 2, 3} and {m for _, m in seen} == {0, 1}, sorted(set(seen))


# ---- 9. chains are independent --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,C,eps,depth", [(MC.SHAPES[1], 4, 0.2, 4), (MC.SHAPES[0], 80, 0.2, 3), (MC.SHAPES[3], 4, 0.12, 3)], ids=_id)
def test_a_chains_bits_do_not_depend_on_its_neighbours(shape, C, eps, depth):
    import torch
    model, mlp = _rig(shape)
    data = MC.kernel_data(shape, C, True)
    data_t = torch.from_numpy(data).cuda()
    case = _case(shape, C, eps, mlp, data_t)
    seeds = [NC.KERNEL_SEEDS0 + c for c in range(C)]
    run = _Run(case, mlp, data_t, seeds, 11, depth)
    pt = case["pt"]
    for c in range(C):                                               # every chain
        alone = H.chain_subset(case, c)
        one = _Run(alone, mlp, torch.from_numpy(data[c:c + 1].copy()).cuda(), seeds[c:c + 1], 11, depth)
        _assert_nothing_else_moved(one, alone)
        _assert_same_chain(run, c, one, pt, (shape, C))


@pytest.mark.parametrize("shape", [MC.SHAPES[1], MC.SHAPES[3]], ids=_id)
def test_a_chain_with_a_nan_diverges_at_its_first_leaf_keeps_its_state_and_disturbs_nobody(shape):
    import torch
    model, mlp = _rig(shape)
    C, bad, eps, depth = 4, 2, 0.12, 3
    data_t = torch.from_numpy(MC.kernel_data(shape, C, True)).cuda()
    clean = _case(shape, C, eps, mlp, data_t)
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clean.items()}
    case["K"][bad, shape[0] // 3] = np.nan                           # a value, not a fault
    seeds = [NC.KERNEL_SEEDS0 + c for c in range(C)]
    ref, run = _Run(clean, mlp, data_t, seeds, 0, depth), _Run(case, mlp, data_t, seeds, 0, depth)
    _assert_nothing_else_moved(run, case)
    pt = case["pt"]
    assert run.tree[pt, bad].tolist() == [0, 1, 3, 0] and run.stat[pt, bad] == 0.0
    for name in ("K", "U", "dU", "loss", "accept"):                  # the flagged chain keeps its state's bits
        assert H.same_bits(run.body(name)[bad], np.asarray(case[name])[bad]), name
    assert H.same_bits(run.body("Kq0")[bad], case["K"][bad]) and H.same_bits(run.body("trace")[pt + 1, bad], case["K"][bad])
    good = [c for c in range(C) if c != bad]
    for name in STATE:
        assert H.same_bits(run.body(name)[good], ref.body(name)[good]), name
    assert H.same_bits(run.tree[pt, good], ref.tree[pt, good]) and H.same_bits(run.stat[pt, good], ref.stat[pt, good])
    assert H.same_bits(run.body("trace")[pt + 1, good], ref.body("trace")[pt + 1, good])


# ---- checks before any device call, and the capture refusal ------------------------------------------------------------------------------------
def test_the_entry_point_refuses_before_any_launch():
    import torch
    L = _lib()
    err = L.finrom_last_error
    shape = MC.SHAPES[0]
    model, mlp = _rig(shape)
    data_t = torch.from_numpy(MC.kernel_data(shape, 3, False)).cuda()
    seeds_t = torch.arange(3, dtype=torch.int64, device="cuda")
    d, sd, s = data_t.data_ptr(), seeds_t.data_ptr(), _stream()

    def call(dev, mlp_h=mlp._h, seeds=sd, p0=0, depth=3, data=d):
        return L.finrom_hmc_nuts_ml(mlp_h, ctypes.byref(dev.st) if dev is not None else None, seeds, p0, depth, data, 0, None, None, s)
    dev = H.DeviceState(NC.kernel_state(shape, 3, 0.05))
    assert call(None) == ERR_ARG and b"hmc_nuts_ml: null field" in err()
    assert call(dev, mlp_h=None) == ERR_ARG and b"hmc_nuts_ml: null mlp handle or data" in err()
    assert call(dev, data=None) == ERR_ARG and b"null mlp handle or data" in err()
    assert call(dev, seeds=None) == ERR_ARG and b"hmc_nuts_ml: null seeds" in err()
    assert call(dev, p0=-1) == ERR_ARG and b"proposal0 < 0" in err()
    for depth in (0, 11):
        assert call(dev, depth=depth) == ERR_ARG and b"max_depth = %d is outside 1 .. 10" % depth in err()
    other = H.DeviceState(NC.kernel_state((shape[0] - 1,) + shape[1:], 3, 0.05))
    assert call(other) == ERR_ARG and b"n = 36 is not the network's input size (37)" in err()
    zero = NC.kernel_state(shape, 3, 0.05)
    zero["c_pri"] = 0.0
    zdev = H.DeviceState(zero)
    assert call(zdev) == ERR_ARG and b"hmc_nuts_ml: c_pri = 0" in err()
    many = H.DeviceState(NC.kernel_state(shape, 3, 0.05))
    many.st.C = 65536                                                # (refused before anything is read)
    assert call(many) == ERR_UNSUPPORTED and b"C > 65535" in err()
    none = H.DeviceState(NC.kernel_state(shape, 0, 0.05))
    assert call(none) == 0
    for t in (dev, other, zdev, many, none):
        t.assert_bits(t.download(), {})


def test_the_first_call_with_a_new_c_inside_a_capture_is_refused_with_a_message():
    import torch
    from bayesianinferencedl_amd.engine import DeviceErrorModel
    L = _lib()
    shape = MC.SHAPES[0]
    mlp = DeviceErrorModel(MC.kernel_model(shape))                   # a fresh handle: no workspace yet
    data_t = torch.from_numpy(MC.kernel_data(shape, 5, False)).cuda()
    seeds_t = torch.arange(5, dtype=torch.int64, device="cuda")
    case = _case(shape, 5, 0.05, _rig(shape)[1], torch.from_numpy(MC.kernel_data(shape, 5, True)).cuda())
    dev = H.DeviceState(case)
    x = torch.ones(8, device="cuda")
    call = lambda: L.finrom_hmc_nuts_ml(mlp._h, ctypes.byref(dev.st), seeds_t.data_ptr(), 0, 3, data_t.data_ptr(), 0, None, None, _stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        twice = x * 2.0                                              # (the capture is not empty)
        rc = call()
        msg = L.finrom_last_error()
    torch.cuda.synchronize()
    assert rc == ERR_UNSUPPORTED and b"capture" in msg, (rc, msg)
    dev.assert_bits(dev.download(), {})
    assert call() == 0                                               # outside the capture the same call goes through
    got = dev.download()
    assert int(dev.body(got, "pt")) == case["pt"] + 1 and np.isfinite(dev.body(got, "K")).all()


# ---- 10. device chains against the host -------------------------------------------------------------------------------------------------------
DEPTH = 4


@pytest.fixture(scope="module")
def chains(spaces):
    from bayesianinferencedl_amd.deep_learning.dl_model import Surrogate
    model = SC.hmc_model()
    prior = MC.prior4(spaces(4))
    sur = Surrogate(model)
    return dict(model=model, sur=sur, data=SC.hmc_data(model), prior=prior, wsur=sur.whitened(prior), hosts={}, devs={})


def _kw(field, **more):
    from bayesianinferencedl_amd.bayesian_inference.nuts import Nuts
    return MC.chain_kw(field, rng="philox", nuts=Nuts(DEPTH), keep_trace=True, **more)


def _host(c, field):
    """run_chains(nuts=) over the same device calls: under the prior on the WHITENED surrogate with mean 0 and tau 1."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    if field not in c["hosts"]:
        kw = _kw(field)
        if field:
            kw.update(mean=0.0, tau=1.0)
        res = hmc.run_chains(hmc.ml_value_and_grad(c["wsur" if field else "sur"], c["data"]), SC.hmc_starts(field=field), MC.HMC_EVALS, **kw)
        if field:
            res = hmc.HmcResult(res, V=res.K, K=c["prior"].field(res.K), trace=c["prior"].field(res.trace))
        c["hosts"][field] = res
    return c["hosts"][field]


def _device(c, field, **more):
    from bayesianinferencedl_amd.bayesian_inference import hmc
    key = (field,) + tuple(sorted((k, str(v)) for k, v in more.items()))
    if key not in c["devs"]:
        res = hmc.run_chains_device(None, SC.hmc_starts(field=field), MC.HMC_EVALS, model="ml", surrogate=c["sur"], data=c["data"],
                                    prior=c["prior"] if field else None, **_kw(field, **more))
        assert res.fused is True and res.model == "ml" and res.nuts == DEPTH
        c["devs"][key] = res
    return c["devs"][key]


def _close(dev, host):
    """tests/test_gpu_hmc_ml.py::_close."""
    assert dev.proposals == host.proposals and np.array_equal(dev.accept, host.accept), (dev.accept, host.accept)
    assert np.max(np.abs(dev.trace - host.trace)) <= 1e-9 * np.max(np.abs(host.trace))
    assert np.linalg.norm(dev.K - host.K) <= 1e-9 * np.linalg.norm(host.K)
    if host.get("V") is not None:
        assert np.linalg.norm(dev.V - host.V) <= 1e-9 * np.linalg.norm(host.V)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "stream"])
@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_the_device_chains_follow_the_host_statement_over_the_same_device_calls(chains, field, graph):
    host = _host(chains, field)
    print(f"NUTS chains {'field' if field else 'iid'}: host margin {host.margin:.3e}, tree rows {host.tree.reshape(-1, 4).tolist()}")
    assert host.margin >= NC.MARGIN
    dev = _device(chains, field, graph=graph)
    assert dev.graph == graph and dev.proposals == MC.HMC_PROPOSALS
    assert np.array_equal(dev.tree, host.tree), (dev.tree.tolist(), host.tree.tolist())
    _close(dev, host)
    assert np.array_equal(dev.accept, dev.tree[:, :, 3].sum(axis=0)) and dev.n_evals == host.n_evals
    assert np.max(np.abs(dev.accept_stat - host.accept_stat)) <= 1e-9
    assert dev.tree[:, :, 1].max() > 1                               # (trees, not single steps)


@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_graph_stream_and_block_give_the_same_bits(chains, field):
    a, b, d = _device(chains, field, graph=True), _device(chains, field, graph=False), _device(chains, field, graph=True, block=3)
    for x in (b, d):
        assert np.array_equal(a.K, x.K) and np.array_equal(a.trace, x.trace) and np.array_equal(a.accept, x.accept)
        assert np.array_equal(a.tree, x.tree) and np.array_equal(a.accept_stat, x.accept_stat)
        if field:
            assert np.array_equal(a.V, x.V)


@pytest.mark.parametrize("field", [False, True], ids=["iid", "field"])
def test_device_stats_are_the_recursion_over_the_kept_trace(chains, field):
    """ChainStats(burn=1, batch=1), to the standard of tests/test_gpu_hmc_ml.py's stats test: under the i.i.d. prior bit for bit, under
    the Gaussian-field prior mean 1e-12 absolute, m2 1e-12 t."""
    from bayesianinferencedl_amd.bayesian_inference.hmc import ChainStats, stats_from_trace
    plain = _device(chains, field, graph=True)
    res = _device(chains, field, graph=True, stats=ChainStats(burn=1, batch=1))
    assert np.array_equal(res.K, plain.K) and np.array_equal(res.tree, plain.tree) and np.array_equal(res.trace, plain.trace)
    s, ref = res.stats, stats_from_trace(res.trace, 1, 1)
    assert (s.t, s.n_batches, s.first, s.next) == (ref.t, ref.n_batches, ref.first, ref.next) == (3, 3, 0, 4)
    assert np.array_equal(s.accepted, ref.accepted) and np.array_equal(s.accepted.sum(0), res.accept)
    assert np.array_equal(s.accepted[1:], res.tree[:, :, 3])
    if field:
        assert np.max(np.abs(s.mean - ref.mean)) <= 1e-12 and np.max(np.abs(s.m2 - ref.m2)) <= 1e-12 * s.t
        assert np.max(np.abs(s.bm_mean - ref.bm_mean)) <= 1e-12 and np.max(np.abs(s.bm_m2 - ref.bm_m2)) <= 1e-12 * s.n_batches
        assert np.max(np.abs(s.cur - ref.cur)) <= 1e-12
    else:
        for name in ChainStats.SUMS + ("cur",):
            assert np.array_equal(getattr(s, name), getattr(ref, name)), name
    assert np.isfinite(s.misfit).all()
    stay = s.accepted[1:] == 0
    assert np.array_equal(s.misfit[1:][stay], s.misfit[:-1][stay]) and np.all(s.misfit[1:][~stay] != s.misfit[:-1][~stay])


def test_with_nuts_none_the_trajectory_form_is_as_before(chains):
    """The keyword's default changes nothing: the trajectory form's result carries no tree."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    c = chains
    res = hmc.run_chains_device(None, SC.hmc_starts(), MC.HMC_EVALS, model="ml", surrogate=c["sur"], data=c["data"], ml_form="trajectory",
                                **MC.chain_kw(False, rng="philox"))
    assert res.ml_form == "trajectory" and "tree" not in res and "nuts" not in res
