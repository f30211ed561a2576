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

`fma(a, x, y)` and `dot(x, y)` may be given: the defaults are the plain NumPy expressions; tests/hmc_cases.fma and the emulated
block_sum_1024 make the iterative form the kernel's arithmetic bit for bit."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import philox

E_MAX = 1000.0
MAX_DEPTH_LIMIT = 10
STOP_DEPTH, STOP_TREE_TURNED, STOP_SUBTREE_TURNED, STOP_DIVERGED = 0, 1, 2, 3


class Nuts:
    """nuts=Nuts(max_depth): at most 2^max_depth - 1 leapfrog steps per transition (the reference: 7)."""

    def __init__(self, max_depth=7):
        if int(max_depth) != max_depth or not 1 <= max_depth <= MAX_DEPTH_LIMIT:
            raise ValueError(f"Nuts: max_depth = {max_depth} is outside 1 .. {MAX_DEPTH_LIMIT}")
        self.max_depth = int(max_depth)


def _plain_fma(a, x, y):
    return a * x + y


def _rel(a, b):
    """|a - b| relative to the larger side."""
    big = max(abs(a), abs(b))
    return abs(a - b) / big if big > 0 else np.inf


class _Transition:
    """What both forms share: the start, the leaf (one leapfrog step, its energy, the streamed selection), the adoption."""

    def __init__(self, value_and_grad, k, U, dU, loss, p0, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma, dot):
        Nuts(max_depth)
        self.f, self.fma, self.dot = value_and_grad, fma or _plain_fma, dot or np.dot
        self.seed, self.proposal, self.eps, self.c_lik, self.c_pri, self.max_depth = seed, int(proposal), eps, c_lik, c_pri, max_depth
        self.mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), np.shape(k))
        self.h, self.coef = 0.5 * eps * c_pri, c_lik / c_pri
        p0 = np.array(p0, dtype=np.float64)
        self.H0 = U + 0.5 * self.dot(p0, p0)
        start = (np.array(k, dtype=np.float64), p0, np.array(dU, dtype=np.float64))
        self.edge = {-1: start, 1: start}
        self.rho, self.W = p0.copy(), 1.0
        self.cand = (start[0], start[2], U, loss)
        self.m, self.sum_acc, self.margin = 0, 0.0, np.inf
        self.depth, self.moved, self.reason, self.directions = 0, 0, STOP_DEPTH, []

    def note(self, a, b):
        self.margin = min(self.margin, _rel(a, b))

    def turning(self, rho, pa, pb):
        """rho . pa <= 0 or rho . pb <= 0, each product's gap from zero relative to |rho| |p| noted."""
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

    def leaf(self):
        """One leapfrog step of the walker -> its momentum, or None: diverged."""
        k, p, dU = self.walker
        d, fma = self.d, self.fma
        self.m += 1
        ph = fma(-d * self.h, dU, p)
        kn = fma(d * self.eps, ph, k)
        loss, grad, bad = self.f(kn[None])
        loss, grad, bad = float(np.asarray(loss)[0]), np.asarray(grad, dtype=np.float64)[0], bool(np.asarray(bad)[0])
        with np.errstate(all="ignore"):
            dk = kn - self.mean
            dUn = fma(self.coef, grad, dk)
            pn = fma(-d * self.h, dUn, ph)
            Un = float(fma(self.c_lik, loss, 0.5 * self.c_pri * self.dot(dk, dk)))
            dE = (Un + 0.5 * self.dot(pn, pn)) - self.H0
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
        self.walker = (kn, pn, dUn)
        return pn

    def adopt(self, j):
        """The finished sub-tree joins the tree -> whether the tree has turned."""
        self.note(self.u_top * self.W, self.W_sub)
        if self.u_top * self.W < self.W_sub:
            self.cand, self.moved = self.sub_cand, 1
        self.W += self.W_sub
        self.rho = self.rho + self.rho_sub
        self.edge[self.d] = self.walker
        self.depth = j + 1
        return self.turning(self.rho, self.edge[-1][1], self.edge[1][1])

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


def transition_iterative(value_and_grad, k, U, dU, loss, p0, *, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma=None, dot=None):
    """One transition of ONE chain from the state (k [n], U, dU [n] = grad U / c_pri, loss) with the momentum p0 [n]; the other draws
    are philox.nuts_top / nuts_leaf of (seed, proposal).  value_and_grad(K [1, n]) -> (loss [1], grad [1, n], bad [1]) as run_chains
    takes it.  The leaves in order, U-turns by checkpoints.  -> a namespace: k, dU, U, loss (the draw), depth, steps, reason, moved,
    tree (those four, int32), accept_stat, margin, directions."""
    t = _Transition(value_and_grad, k, U, dU, loss, p0, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma, dot)
    ck_p, ck_rho = [None] * max_depth, [None] * max_depth
    t.max_span = 0

    def subtree(j):
        for i in range(1 << j):
            p = t.leaf()
            if p is None:
                return STOP_DIVERGED
            i_max = bin(i >> 1).count("1")
            if not i & 1:
                ck_p[i_max], ck_rho[i_max] = p, t.rho_sub
                continue
            i_min = i_max - _trailing_ones(i) + 1
            for c in range(i_max, i_min - 1, -1):
                rho_s = (t.rho_sub - ck_rho[c]) + ck_p[c]
                if t.turning(rho_s, ck_p[c], p):
                    t.max_span = max(t.max_span, i_max - c + 1)      # levels the turning span covers: 1 = two leaves
                    return STOP_SUBTREE_TURNED
        return 0
    out = t.run(subtree)
    out.turn_levels = t.max_span
    return out


def transition_recursive(value_and_grad, k, U, dU, loss, p0, *, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma=None, dot=None):
    """transition_iterative's transition with the sub-tree built by the textbook recursion: two halves, rho their sum, the criterion on
    the union's first and last momentum."""
    t = _Transition(value_and_grad, k, U, dU, loss, p0, seed, proposal, eps, c_lik, c_pri, mean, max_depth, fma, dot)

    def build(depth):
        """-> (reason, first momentum, last momentum, rho)"""
        if depth == 0:
            p = t.leaf()
            return (STOP_DIVERGED, None, None, None) if p is None else (0, p, p, p)
        r1, a, _, rho1 = build(depth - 1)
        if r1:
            return r1, None, None, None
        r2, _, b, rho2 = build(depth - 1)
        if r2:
            return r2, None, None, None
        rho = rho1 + rho2
        return (STOP_SUBTREE_TURNED if t.turning(rho, a, b) else 0), a, b, rho
    return t.run(lambda j: build(j)[0])
