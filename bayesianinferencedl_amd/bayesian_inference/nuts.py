"""The No-U-turn sampler's transition (hmc.py nuts=Nuts(max_depth)), in NumPy: multinomial NUTS with the generalised U-turn criterion
(Betancourt 2017, "A Conceptual Introduction to Hamiltonian Monte Carlo", A.4), the sampler the reference runs
(bayesian_inference/inference.py:165-166 `pm.NUTS(scaling=G_INV, max_treedepth=7, target_accept=0.98)`), with an identity mass and a
step size that is the caller's.  The statement finrom_hmc_nuts_ml (csrc/hmc_nuts.hip) is tested against.

The chain state's conventions are hmc.py's: dU holds grad U / c_pri and U = fma(c_lik, loss, 0.5 c_pri |k - mean|^2).

A LEAPFROG STEP in direction d = +-1, h = 0.5 eps c_pri formed once:
    p1/2 = fma(-d h, dU, p);  k' = fma(d eps, p1/2, k);  evaluate at k';  dU' = fma(c_lik / c_pri, grad, k' - mean);  p' = fma(-d h, dU', p1/2)
(full-step momenta at every leaf).

START: p0 the proposal's momentum, H0 = U + |p0|^2 / 2, both edges the start, rho = p0, W = 1, the candidate the start.
DOUBLING j = 0 .. max_depth - 1: philox.nuts_top gives the direction and u_top; 2^j leaves from that direction's edge.  Leaf m = 1, 2, ...
(counted over the whole transition): H = U + |p|^2 / 2, dE = H - H0; flagged, dE not finite or dE > 1000 (PyMC3's Emax): the sub-tree is
discarded and the transition ends (stop reason 3).  Else w = exp(-dE), W_sub += w, u_m = philox.nuts_leaf, the sub-tree's candidate becomes
this leaf when u_m W_sub < w, rho_sub += p.  U-turn inside the sub-tree with O(depth) checkpoints: leaf i (0-based inside the sub-tree),
i_max = popcount(i >> 1), i_min = i_max - (trailing one bits of i) + 1; an even i stores (p, rho_sub) at i_max; an odd i tests the
checkpoints c = i_max .. i_min with rho_s = rho_sub - rho_ckpt[c] + p_ckpt[c]: turning when rho_s . p_ckpt[c] <= 0 or rho_s . p <= 0 --
the sub-tree is discarded and the transition ends (2).  A finished sub-tree is adopted: the candidate is replaced when u_top W < W_sub;
W += W_sub, rho += rho_sub, the edge moves, depth = j + 1; the transition ends when rho . p_left <= 0 or rho . p_right <= 0 (1), or at
max_depth (0).  No logarithm anywhere, one exp per leaf.

Two forms that are given the same draws and return the same tree: transition_recursive builds a sub-tree by the textbook recursion
(two halves, their rho added, the criterion on the union); transition_iterative walks the leaves in order with the checkpoints above --
the form the kernel executes.  Both report `margin`: the smallest relative gap between the two sides of any comparison made (a U-turn
product relative to |rho| |p|, a selection test relative to its larger side), so that a test can require its inputs to decide clearly.

LeafMachine is transition_iterative cut at the model call -- begin() returns the first point to evaluate, leaf(loss, grad, bad) takes
its evaluation and returns the next, result() the same namespace --, with all of its state named: the statement of finrom_hmc_nuts_begin /
_leaf / _end (csrc/hmc_nuts_model.hip), which make one leaf per launch so that any model's launches can sit between two leaves.
transition_lockstep advances C machines together with one batched call per round: the statement of hmc.py's device form for "fom",
"rom" and "romml".

`fma(a, x, y)` and `dot(x, y)` may be given: the defaults are the plain NumPy expressions; tests/hmc_cases.fma and the emulated
block_sum_1024 make the iterative form the kernel's arithmetic bit for bit.

UNDER A METRIC (Nuts(max_depth, metric=LowRankMetric), the reference's `scaling`: M = I + V diag(lambda) V^T, laplace.py; the statement
finrom_hmc_nuts_ml_metric is tested against).  metric None or of rank zero: every line and bit above.  Otherwise, with the velocity
    v(x) = M^-1 x = x + sum_j a_j V_j,   a_j = c_inv[j] dot_metric(V_j, x),   c_inv = -lambda / (1 + lambda)   (laplace._coef's forms),
the terms added j ascending, one fma(a_j, V_j, .) each:
START: the proposal's standard normals xi (the same Philox words), p0 = M^(1/2) xi by the same map with c_sqrt = lambda / (sqrt(1 +
lambda) + 1), v0 = v(p0), H0 = U + dot(p0, v0) / 2, both edges (k, p0, v0, dU), rho = p0.
LEAF: p1/2 = fma(-d h, dU, p); k' = fma(d eps, v(p1/2), k); evaluate at k', dU' as above; p' = fma(-d h, dU', p1/2); v' = v(p');
dE = (U' + dot(p', v') / 2) - H0; divergence, weight, streamed selection and rho_sub += p' as above.
U-TURNS, the generalised criterion with p# = M^-1 p (Betancourt 2017, A.4.2): a checkpoint stores (p, v, rho_sub), rho_s = (rho_sub -
rho_ckpt) + p_ckpt; a sub-tree is turning when dot(rho_s, v_ckpt) <= 0 or dot(rho_s, v') <= 0, the tree when dot(rho, v_left) <= 0 or
dot(rho, v_right) <= 0; `margin` takes these products relative to |rho| |v|.
`dot_metric(V_j, x)` may be given like `dot`: the default is np.dot; the kernel's is one wave's (tests/nuts_metric_cases.py).

THE STEP SIZE (Nuts(max_depth, adapt=StepAdapt(target_accept, tune)), the reference's `tune` and `target_accept`): dual averaging on the
accept_stat a transition reports, per chain, behind each of the first `tune` transitions: StepAdapt below, the statement
finrom_hmc_step_adapt_update is tested against.  The transition itself is the one above with that chain's eps."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import philox

E_MAX = 1000.0
MAX_DEPTH_LIMIT = 10
STOP_DEPTH, STOP_TREE_TURNED, STOP_SUBTREE_TURNED, STOP_DIVERGED = 0, 1, 2, 3


class StepAdapt:
    """Nuts(adapt=StepAdapt(target_accept, tune)): the dual-averaging warm-up of the step size (Hoffman & Gelman 2014, Algorithm 5;
    the reference's `tune=100, target_accept=0.98`, bayesian_inference/inference.py:145,165-166), per chain as PyMC3 has it.  The
    specification handed to a chain function and, started, the result `res.adapt`; the statement of finrom_hmc_step_adapt_update
    (csrc/hmc_nuts_model.hip).

    A started StepAdapt holds per chain [C] eps (the step the next transition takes), hbar and xbar (the log-domain state), and mu =
    log(10 eps0) of the caller's eps=, formed once; `next`: the global index of the next transition.  It starts at (eps0, 0, 0).
    update(a, p) behind the transition with global index p, a [C] its accept_stat, t = p + 1, ONLY WHILE t <= tune:
        w    = 1 / (t + t0)
        hbar = (1 - w) * hbar + w * (target - a)
        s    = sqrt(t)
        x    = mu - hbar * s / gamma
        eta  = 1 / (s * sqrt(s))                    (t^-kappa, kappa = 0.75, without pow)
        xbar = eta * x + (1 - eta) * xbar
        eps  = exp(x) if t < tune, exp(xbar) if t == tune: the step every later transition takes
    every operation as written, nothing contracted: +, -, *, / and sqrt are correctly rounded here and on the device, so hbar and xbar
    are the device's bits and only exp can differ.  tune = 0 never moves eps.
    target_accept, tune: None stands for 0.8 and 100.  resume: the `adapt` of the run this one continues (its target_accept and tune
    are taken over, and values given beside it that differ from them are refused; the run must start at proposal0 = resume.next, the
    continuation rule of ChainStats(resume=))."""
    GAMMA, T0, KAPPA = 0.05, 10.0, 0.75

    def __init__(self, target_accept=None, tune=None, resume=None):
        if resume is not None:
            if not isinstance(resume, StepAdapt) or not resume.started:
                raise ValueError("StepAdapt: resume= takes the adapt a run returned")
            if target_accept not in (None, resume.target_accept) or tune not in (None, resume.tune):
                raise ValueError(f"StepAdapt: target_accept = {target_accept}, tune = {tune} differ from the resumed run's "
                                 f"{resume.target_accept}, {resume.tune}")
            target_accept, tune = resume.target_accept, resume.tune
        target_accept, tune = 0.8 if target_accept is None else target_accept, 100 if tune is None else tune
        if not 0.0 < target_accept < 1.0:
            raise ValueError(f"StepAdapt: target_accept = {target_accept} is outside (0, 1)")
        if int(tune) != tune or tune < 0:
            raise ValueError(f"StepAdapt: tune = {tune} is not a number of transitions >= 0")
        self.target_accept, self.tune, self.resume = float(target_accept), int(tune), resume
        self.next = None

    started = property(lambda self: self.next is not None)

    def begin(self, eps0, C, proposal0):
        """-> a started StepAdapt for C chains whose first transition has global index proposal0: (eps0, 0, 0) with mu = log(10
        eps0), or a copy of resume's state."""
        s, r = StepAdapt(self.target_accept, self.tune), self.resume
        if r is None:
            if not eps0 > 0.0:
                raise ValueError(f"StepAdapt: eps = {eps0} is not a step size > 0")
            s.mu = float(np.log(10.0 * eps0))
            s.eps, s.hbar, s.xbar = np.full(C, float(eps0)), np.zeros(C), np.zeros(C)
        else:
            if proposal0 != r.next:
                raise ValueError(f"StepAdapt: the resumed run ended before transition {r.next}; this one starts at proposal0 = {proposal0}")
            if len(r.eps) != C:
                raise ValueError(f"StepAdapt: the resumed run had {len(r.eps)} chains, this one {C}")
            s.mu, s.eps, s.hbar, s.xbar = r.mu, r.eps.copy(), r.hbar.copy(), r.xbar.copy()
        s.next = int(proposal0)
        return s

    def update(self, a, p):
        """Behind the transition with global index p: a [C] its accept_stat."""
        if p != self.next:
            raise ValueError(f"StepAdapt.update: transition {p} after transition {self.next - 1}")
        self.next = p + 1
        if p + 1 > self.tune:
            return
        t = float(p + 1)
        w = 1.0 / (t + self.T0)
        self.hbar = (1.0 - w) * self.hbar + w * (self.target_accept - np.asarray(a, dtype=np.float64))
        s = np.sqrt(t)
        x = self.mu - self.hbar * s / self.GAMMA
        eta = 1.0 / (s * np.sqrt(s))
        self.xbar = eta * x + (1.0 - eta) * self.xbar
        self.eps = np.exp(x if p + 1 < self.tune else self.xbar)


class Nuts:
    """nuts=Nuts(max_depth, metric=None, adapt=None): at most 2^max_depth - 1 leapfrog steps per transition (the reference: 7);
    metric: a laplace.LowRankMetric in the chain's own coordinates (whitened ones under prior=), the reference's `scaling`; adapt: a
    StepAdapt, the reference's `tune` and `target_accept` (None: the caller's eps throughout)."""

    def __init__(self, max_depth=7, metric=None, adapt=None):
        if int(max_depth) != max_depth or not 1 <= max_depth <= MAX_DEPTH_LIMIT:
            raise ValueError(f"Nuts: max_depth = {max_depth} is outside 1 .. {MAX_DEPTH_LIMIT}")
        if metric is not None and not all(hasattr(metric, a) for a in ("rho", "n", "Vt", "lam")):
            raise ValueError("Nuts: metric= takes a laplace.LowRankMetric (Vt [rho, n], lam [rho])")
        if adapt is not None and not isinstance(adapt, StepAdapt):
            raise ValueError("Nuts: adapt= takes a StepAdapt(target_accept, tune)")
        self.max_depth = int(max_depth)
        self.metric = metric
        self.adapt = adapt

    def metric_for(self, n, who="Nuts"):
        """The metric of chains with n coordinates, where n is first known: None for no metric or one of rank zero (the identity:
        the plain transition, bit for bit)."""
        metric = getattr(self, "metric", None)
        if metric is None or metric.rho == 0:
            return None
        if metric.n != n:
            raise ValueError(f"{who}: Nuts(metric=): the metric has n = {metric.n}, the chains have {n} coordinates")
        return metric


def _plain_fma(a, x, y):
    return a * x + y


def _rel(a, b):
    """|a - b| relative to the larger side."""
    big = max(abs(a), abs(b))
    return abs(a - b) / big if big > 0 else np.inf


class _Transition:
    """What both forms share: the start, the leaf (one leapfrog step, its energy, the streamed selection), the adoption."""

    def __init__(self, value_and_grad, k, U, dU, loss, p0, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma, dot, metric=None,
                 dot_metric=None):
        self.metric = Nuts(max_depth, metric).metric_for(np.shape(k)[-1], "nuts.transition")
        self.f, self.fma, self.dot, self.dot_metric = value_and_grad, fma or _plain_fma, dot or np.dot, dot_metric or np.dot
        self.seed, self.proposal, self.eps, self.c_lik, self.c_pri, self.max_depth = seed, int(proposal), eps, c_lik, c_pri, max_depth
        self.mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), np.shape(k))
        self.h, self.coef = 0.5 * eps * c_pri, c_lik / c_pri
        p0 = np.array(p0, dtype=np.float64)
        if self.metric is not None:                                  # p0 holds the standard normals xi: p0 = M^(1/2) xi
            from .laplace import _coef
            self.c_inv = _coef(self.metric.lam, "inv")
            p0 = self.low_rank(p0, _coef(self.metric.lam, "sqrt"))
        v0 = self.velocity(p0)
        self.H0 = U + self.kinetic(p0, v0)
        start = (np.array(k, dtype=np.float64), p0, np.array(dU, dtype=np.float64), v0)
        self.edge = {-1: start, 1: start}
        self.rho, self.W = p0.copy(), 1.0
        self.cand = (start[0], start[2], U, loss)
        self.m, self.sum_acc, self.margin = 0, 0.0, np.inf
        self.depth, self.moved, self.reason, self.directions = 0, 0, STOP_DEPTH, []

    def low_rank(self, x, coef):
        """x + sum_j a_j V_j, a_j = coef[j] dot_metric(V_j, x), j ascending, one fma per term."""
        Vt = self.metric.Vt
        a = [coef[j] * self.dot_metric(Vt[j], x) for j in range(len(coef))]
        y = x
        for j in range(len(coef)):
            y = self.fma(a[j], Vt[j], y)
        return y

    def velocity(self, p):
        """M^-1 p (p itself without a metric)."""
        return p if self.metric is None else self.low_rank(p, self.c_inv)

    def kinetic(self, p, v):
        """p . M^-1 p / 2"""
        return 0.5 * self.dot(p, v)

    def note(self, a, b):
        self.margin = min(self.margin, _rel(a, b))

    def turning(self, rho, pa, pb):
        """rho . pa <= 0 or rho . pb <= 0, each product's gap from zero relative to |rho| |p| noted (pa, pb: velocities under a metric)."""
        out = False
        nr = np.sqrt(np.dot(rho, rho))
        for p in (pa, pb):
            v = self.dot(rho, p)
            scale = nr * np.sqrt(np.dot(p, p))
            self.margin = min(self.margin, abs(v) / scale if scale > 0 else np.inf)
            out = out or bool(v <= 0)
        return out

    def begin_subtree(self, j):
        fwd, self.u_top = philox.nuts_top(self.seed, self.proposal, j)
        self.d = 1 if fwd else -1
        self.directions.append(self.d)
        self.walker = self.edge[self.d]
        self.W_sub, self.rho_sub, self.sub_cand = 0.0, np.zeros_like(self.rho), None

    def drift(self):
        """The walker's first half kick and its drift -> the point to evaluate (leaf m of the transition)."""
        k, p, dU, _ = self.walker
        d, fma = self.d, self.fma
        self.m += 1
        self.ph = fma(-d * self.h, dU, p)
        self.kn = fma(d * self.eps, self.velocity(self.ph), k)
        return self.kn

    def arrive(self, loss, grad, bad):
        """The evaluation of drift()'s point: the second half kick, the energy, the streamed selection -> the leaf's (momentum,
        velocity), or None: diverged."""
        kn, ph, d, fma = self.kn, self.ph, self.d, self.fma
        with np.errstate(all="ignore"):
            dk = kn - self.mean
            dUn = fma(self.coef, grad, dk)
            pn = fma(-d * self.h, dUn, ph)
            vn = self.velocity(pn)
            Un = float(fma(self.c_lik, loss, 0.5 * self.c_pri * self.dot(dk, dk)))
            dE = (Un + self.kinetic(pn, vn)) - self.H0
        if bad or not np.isfinite(loss) or not np.isfinite(dE) or dE > E_MAX:
            return None
        with np.errstate(over="ignore"):
            w = float(np.exp(-dE))
        self.W_sub += w
        self.sum_acc += min(1.0, w)
        u = philox.nuts_leaf(self.seed, self.proposal, self.m)
        self.note(u * self.W_sub, w)
        if u * self.W_sub < w:
            self.sub_cand = (kn, dUn, Un, loss)
        self.rho_sub = self.rho_sub + pn
        self.walker = (kn, pn, dUn, vn)
        return pn, vn

    def leaf(self):
        """One leapfrog step of the walker -> its (momentum, velocity), or None: diverged."""
        kn = self.drift()
        loss, grad, bad = self.f(kn[None])
        loss, grad, bad = float(np.asarray(loss)[0]), np.asarray(grad, dtype=np.float64)[0], bool(np.asarray(bad)[0])
        return self.arrive(loss, grad, bad)

    def adopt(self, j):
        """The finished sub-tree joins the tree -> whether the tree has turned."""
        self.note(self.u_top * self.W, self.W_sub)
        if self.u_top * self.W < self.W_sub:
            self.cand, self.moved = self.sub_cand, 1
        self.W += self.W_sub
        self.rho = self.rho + self.rho_sub
        self.edge[self.d] = self.walker
        self.depth = j + 1
        return self.turning(self.rho, self.edge[-1][3], self.edge[1][3])

    def run(self, subtree):
        """subtree(j) -> 0, or the stop reason with which building it ended the transition."""
        for j in range(self.max_depth):
            self.begin_subtree(j)
            self.reason = subtree(j)
            if self.reason:
                break
            if self.adopt(j):
                self.reason = STOP_TREE_TURNED
                break
        return self.result()

    def result(self):
        k, dU, U, loss = self.cand
        return SimpleNamespace(k=k, dU=dU, U=U, loss=loss, depth=self.depth, steps=self.m, reason=self.reason, moved=self.moved,
                               accept_stat=self.sum_acc / self.m, margin=self.margin, directions=self.directions,
                               tree=np.array([self.depth, self.m, self.reason, self.moved], np.int32))


def _trailing_ones(i):
    t = 0
    while i & 1:
        i >>= 1
        t += 1
    return t


def transition_iterative(value_and_grad, k, U, dU, loss, p0, *, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma=None, dot=None,
                         metric=None, dot_metric=None):
    """One transition of ONE chain from the state (k [n], U, dU [n] = grad U / c_pri, loss) with the momentum p0 [n]; the other draws
    are philox.nuts_top / nuts_leaf of (seed, proposal).  value_and_grad(K [1, n]) -> (loss [1], grad [1, n], bad [1]) as run_chains
    takes it.  The leaves in order, U-turns by checkpoints.  metric: a LowRankMetric (p0 then holds the standard normals: the module's
    text).  -> a namespace: k, dU, U, loss (the draw), depth, steps, reason, moved,
    tree (those four, int32), accept_stat, margin, directions."""
    t = _Transition(value_and_grad, k, U, dU, loss, p0, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma, dot, metric, dot_metric)
    ck_p, ck_v, ck_rho = [None] * max_depth, [None] * max_depth, [None] * max_depth
    t.max_span = 0

    def subtree(j):
        for i in range(1 << j):
            pv = t.leaf()
            if pv is None:
                return STOP_DIVERGED
            p, v = pv
            i_max = bin(i >> 1).count("1")
            if not i & 1:
                ck_p[i_max], ck_v[i_max], ck_rho[i_max] = p, v, t.rho_sub
                continue
            i_min = i_max - _trailing_ones(i) + 1
            for c in range(i_max, i_min - 1, -1):
                rho_s = (t.rho_sub - ck_rho[c]) + ck_p[c]
                if t.turning(rho_s, ck_v[c], v):
                    t.max_span = max(t.max_span, i_max - c + 1)      # levels the turning span covers: 1 = two leaves
                    return STOP_SUBTREE_TURNED
        return 0
    out = t.run(subtree)
    out.turn_levels = t.max_span
    return out


class LeafMachine:
    """transition_iterative cut at the model call (identity mass): the statement of finrom_hmc_nuts_begin / _leaf / _end
    (csrc/hmc_nuts_model.hip), where any model's launches sit between two leaves.
        begin(k, U, dU, loss, p0)  START, begin_subtree(0) and the first drift -> the point to evaluate;
        leaf(loss, grad, bad)      the evaluation of that point -> the next point, or None: the transition has ended;
        result()                   the namespace transition_iterative returns.
    Every operation of transition_iterative in its order (fma=, dot= passed through): driven over a callable, the same bits.  ALL of its
    state is named here -- what the kernel keeps in memory between two launches: j the doubling, i the leaf inside the sub-tree, the
    leaf count m, the direction d and u_top, the walker (k, p, dU) with the half-kicked p1/2 and the drifted k', both edges, rho and
    rho_sub, the checkpoints (p, rho_sub) per level, H0, W, W_sub, the sum of min(1, w), the sub-tree's candidate and the tree's (the
    chain's state itself), depth, moved, reason, active.  `position`: the point of the next evaluation while active, then the draw."""

    def __init__(self, *, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma=None, dot=None):
        self.kw = dict(seed=seed, proposal=proposal, eps=eps, c_lik=c_lik, c_pri=c_pri, mean=mean, max_depth=max_depth, fma=fma, dot=dot)
        self.max_depth, self.active, self.t = max_depth, False, None

    def begin(self, k, U, dU, loss, p0):
        kw = self.kw
        t = self.t = _Transition(None, k, U, dU, loss, p0, kw["seed"], kw["proposal"], kw["eps"], kw["c_lik"], kw["c_pri"], kw["mean"],
                                 self.max_depth, kw["fma"], kw["dot"])
        t.max_span = 0
        self.ck_p, self.ck_rho = [None] * self.max_depth, [None] * self.max_depth
        self.j, self.i, self.active = 0, 0, True
        t.begin_subtree(0)
        self.position = t.drift()
        return self.position

    # the explicit state, by the names of the text above
    m = property(lambda self: self.t.m)
    d = property(lambda self: self.t.d)
    depth = property(lambda self: self.t.depth)
    moved = property(lambda self: self.t.moved)
    reason = property(lambda self: self.t.reason)

    def _end(self, reason):
        self.t.reason, self.active = reason, False
        self.position = self.t.cand[0]
        return None

    def leaf(self, loss, grad, bad):
        if not self.active:
            raise ValueError("LeafMachine.leaf: the transition has ended (or has not begun)")
        t, i = self.t, self.i
        pv = t.arrive(float(loss), np.asarray(grad, dtype=np.float64), bool(bad))
        if pv is None:
            return self._end(STOP_DIVERGED)
        p, v = pv
        i_max = bin(i >> 1).count("1")
        if not i & 1:
            self.ck_p[i_max], self.ck_rho[i_max] = p, t.rho_sub
        else:
            i_min = i_max - _trailing_ones(i) + 1
            for c in range(i_max, i_min - 1, -1):
                rho_s = (t.rho_sub - self.ck_rho[c]) + self.ck_p[c]
                if t.turning(rho_s, self.ck_p[c], v):
                    t.max_span = max(t.max_span, i_max - c + 1)
                    return self._end(STOP_SUBTREE_TURNED)
        self.i += 1
        if self.i == 1 << self.j:                                    # the sub-tree is finished: adoption, the tree's test, the next draw
            if t.adopt(self.j):
                return self._end(STOP_TREE_TURNED)
            if self.j + 1 == self.max_depth:
                return self._end(STOP_DEPTH)
            self.j, self.i = self.j + 1, 0
            t.begin_subtree(self.j)
        self.position = t.drift()
        return self.position

    def result(self):
        if self.active or self.t is None:
            raise ValueError("LeafMachine.result: the transition has not ended")
        out = self.t.result()
        out.turn_levels = self.t.max_span
        return out


def transition_lockstep(value_and_grad, K, U, dU, loss, P0, *, seeds, proposal, eps, c_lik, c_pri, mean, max_depth, fma=None, dot=None):
    """One transition of C chains TOGETHER, the statement of the device form for models whose bits depend on the batch: C LeafMachines,
    ONE call value_and_grad(X [C, n]) -> (loss [C], grad [C, n], bad [C]) per round.  A chain that has ended sits at its draw: its row
    of X is the draw's position and its evaluation is ignored.  K, dU, P0 [C, n], U, loss [C], seeds [C], mean [C, n] (or what
    broadcasts to it).  -> the list of the C namespaces transition_iterative returns, each with `rounds`: the rounds the batch made
    (at most 2^max_depth - 1)."""
    K = np.asarray(K, dtype=np.float64)
    C = len(K)
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), K.shape)
    ms = [LeafMachine(seed=seeds[c], proposal=proposal, eps=eps, c_lik=c_lik, c_pri=c_pri, mean=mean[c], max_depth=max_depth, fma=fma,
                      dot=dot) for c in range(C)]
    for c, mc in enumerate(ms):
        mc.begin(K[c], U[c], dU[c], loss[c], P0[c])
    rounds = 0
    while any(mc.active for mc in ms):
        ls, gr, bad = value_and_grad(np.stack([mc.position for mc in ms]))
        ls, gr, bad = np.asarray(ls, dtype=np.float64), np.asarray(gr, dtype=np.float64), np.asarray(bad, dtype=bool)
        rounds += 1
        for c, mc in enumerate(ms):
            if mc.active:
                mc.leaf(ls[c], gr[c], bad[c])
    out = [mc.result() for mc in ms]
    for r in out:
        r.rounds = rounds
    return out


def transition_recursive(value_and_grad, k, U, dU, loss, p0, *, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma=None, dot=None,
                         metric=None, dot_metric=None):
    """transition_iterative's transition with the sub-tree built by the textbook recursion: two halves, rho their sum, the criterion on
    the union's first and last velocity (momentum, without a metric)."""
    t = _Transition(value_and_grad, k, U, dU, loss, p0, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma, dot, metric, dot_metric)

    def build(depth):
        """-> (reason, first velocity, last velocity, rho)"""
        if depth == 0:
            pv = t.leaf()
            return (STOP_DIVERGED, None, None, None) if pv is None else (0, pv[1], pv[1], pv[0])
        r1, a, _, rho1 = build(depth - 1)
        if r1:
            return r1, None, None, None
        r2, _, b, rho2 = build(depth - 1)
        if r2:
            return r2, None, None, None
        rho = rho1 + rho2
        return (STOP_SUBTREE_TURNED if t.turning(rho, a, b) else 0), a, b, rho
    return t.run(lambda j: build(j)[0])
