"""Minimal Hamiltonian Monte Carlo driver for BASELINE configs[4]: chains of sequential, DEPENDENT one-sample
value-and-gradient calls of the ROM + learned-error misfit (`AffineROMFin.grad_romml`), the call pattern PyMC3's NUTS
drives through the reference's Theano op (bayesian_inference/pymc_func_bayes_inverse.py:92-104 `err_grad_ROMML`,
:148-167 `SqErrorOpROMML.perform`, model :186-203: potential = misfit / sigma^2 on a latent Gaussian field).

PyMC3 / Theano are control plane and out of scope; what the hot path needs from them is the leapfrog recursion
that makes every evaluation's input depend on the previous evaluation's gradient.  This module is that recursion and
nothing more: fixed-length leapfrog trajectories with a Metropolis test, in independent chains.  Chains are independent, so C
chains advance in LOCKSTEP: one device call evaluates the current leapfrog point of every chain (a batch of C samples), each
chain keeping its own momentum, random stream and accept/reject decision.  On N GPUs a rank owns chains `rank, rank + N, ...` (one
chain per GPU at N = C) and there is no communication until the traces are gathered.

Three chain functions walk the same chains:
  run_chains         the host recursion in NumPy over a callable value_and_grad(K) -> (loss, grad, bad): the statement the other
                     two are tested against (callables: romml_ / fom_ / rom_ / ml_value_and_grad);
  run_chains_device  the chains resident on the device, a proposal captured once as a HIP graph and replayed; its torch-op form
                     is a few elementwise kernels around one model call per step and serves every combination below;
  run_chains_fused   the same with the trajectory's arithmetic inside the library, one step form per (model, prior, metric)
                     (_fused_form); run_chains_device takes it where the library has the form (fused=None) or is told to (fused=True).
The two device functions share one scaffold (_DeviceChains) and differ in evaluation 0 and in what a proposal launches.

The keywords, on all three functions unless said otherwise:

`prior=` None: an i.i.d. Gaussian prior N(mean, tau^2) per node (the form BASELINE configs[4] measures; mean=None: the start
points).  `GaussianFieldPrior(V)` (gaussian_field.py): the reference's own prior, a latent Matern-5/2 Gaussian field
(`pm.gp.Latent(Matern52(2, ls=1.2)).prior`, :191-201), sampled as PyMC3 samples it -- non-centred, in whitened coordinates: the
chains move v ~ N(0, I), the field is k = mean + U^T v (U the upper Cholesky factor of the covariance), the potential is
misfit(k) / sigma^2 + |v|^2 / 2 and its gradient v + U grad_k / sigma^2.  K0 then holds whitened start points, mean must be None
(the prior carries it) and tau is unused; the value-and-gradient call still receives fields and returns field-space gradients (on
the device the two triangular products around it are finrom_sampler_field / _pullback); K and trace of the result are fields, V
the whitened end states.

`metric=LowRankMetric` (laplace.py): a constant mass matrix M = I + V diag(lambda) V^T in the chain's own coordinates (under a
prior the whitened ones), the Gauss-Newton Hessian of the potential at the MAP point (the `scaling` the reference's sampler hands to
NUTS, bayesian_inference/inference.py:102-140,165).  The random stream is the same: the standard normals xi become momenta p =
M^(1/2) xi, the position moves by eps M^-1 p and the kinetic energy is p^T M^-1 p / 2 (= |xi|^2 / 2 at the start).  A metric of rank
zero is the identity and takes the plain paths.

`rng=`, `seeds=`, `proposal0=`: "numpy" (the default) -- chain c draws from np.random.default_rng(seeds[c]), per proposal n normals
for the momentum, then one uniform (_HostDraws); on the device the draws are made `block` proposals ahead and uploaded.  "philox" --
a counter-based stream (philox.py; on the device finrom_hmc_draw, one launch per block of proposals, no host draw and no upload):
Philox4x32-10 with key = seed and counter = (proposal, pair index, 0) for the Box-Muller pairs of the momentum, (proposal, 0, 1)
for the uniform; seeds in [0, 2^64).  The draw of proposal p of the chain with seed s depends on (s, p) alone, so a chain is the
same for any `block` and any deal of the chains over ranks.  THE CONTINUATION RULE: a run of p1 proposals followed by a run from
its end state (K; V under a prior) with proposal0=p1 and an explicit mean= (the first run's; under a prior the prior carries it)
walks the path of one uninterrupted run.  It needs rng="philox": a NumPy generator cannot be advanced to a proposal.

`stats=ChainStats(burn, batch)`: what the reference's drivers take from the trace after the run (bayesian_inference/inference.py:
175-214 `np.mean(trace, 0)`, `np.std(trace, 0)`, the misfit per draw; pymc_func_bayes_inverse.py:212-220) accumulated WHILE the
chains run, so that no trace is kept: per chain and node the Welford mean and sum of squared deviations of the FIELD (under a prior
the field, not the whitened state: its variance needs Cov(v) in full) and the Welford moments of the means of batches of `batch`
consecutive draws, per chain the misfit and the accept flag after every proposal.  On the device that is one launch per proposal
(finrom_hmc_stats_update, behind the Metropolis test, inside the replayed graph); ChainStats.update is the same recursion in NumPy,
operation for operation, and the device's sums are its bits.  `res.stats.summarize()` forms the pooled mean, standard deviation,
R-hat, batch-means effective sample size and Monte-Carlo standard error on the host.  Draws are the states after the proposals with
GLOBAL index >= burn; everything is indexed by the global proposal index, so the sums do not depend on `block`, on graph or stream
order, or on where a run was interrupted: `stats=ChainStats(resume=first.stats)` with the continuation rule continues every sum.

`model=`, `solver=`, `surrogate=`, `data=` (device functions): which of the inverse problem's models the chains evaluate (the
reference's driver instantiates the full-order operator, pymc_func_bayes_inverse.py:174; the reduced ones are the alternatives
beside it, :175-176).  "romml" (the default): solver_r with a device error model.  "rom": solver_r, the plain reduced model without
the learned correction; it sees the field only through its sub-fin averages, so under a prior its fused step stays in whitened
coordinates: theta = Sop m + (Sop U^T) v, grad_v = (Sop U^T)^T g_theta, no triangular product and no field during a trajectory.
"fom": solver=Fin and data=.  "ml": surrogate=Surrogate and data=, the pure deep-learning surrogate (the reference's
MLSolverWrapper); an evaluation is finrom_mlp_misfit_grad.  solver_r may be None for "fom" and "ml".

`ml_form=` (device functions, model="ml" only): None -- the torch-op form.  "steps" | "trajectory" -- the trajectory inside the
library (csrc/hmc_ml.hip): a step as three launches (finrom_hmc_leapfrog_ml), or all n_leapfrog steps in ONE launch with a
1024-thread workgroup per chain (finrom_hmc_trajectory_ml), which leaves the bits of the composed steps.  Under a prior the field
is folded into the first layer (dl_model.whiten_first_layer, Surrogate.whitened: W0' = U W0, b0' = b0 + W0^T mean) and the chain is
the i.i.d. chain of that network with mean 0 and tau 1.  With an ml_form nothing falls back to the torch-op form.

`nuts=Nuts(max_depth)` (nuts.py): the No-U-turn sampler the reference runs (bayesian_inference/inference.py:165-166 `pm.NUTS(scaling=G_INV,
max_treedepth=7, target_accept=0.98)`) in the place of the fixed-length trajectory and its Metropolis test: multinomial NUTS with the
generalised U-turn criterion, identity mass, eps the caller's (or adapted: `adapt=` below).  A call makes (n_evals - 1) // n_leapfrog transitions,
the draws the same call makes without nuts=.  run_chains: nuts.transition_iterative over any callable, chain by chain.  Device
functions, two library forms (fused=False is refused).  model="ml": a transition is ONE finrom_hmc_nuts_ml call (the tree's kernel, one
1024-thread workgroup per chain, and the counters' advance behind it: csrc/hmc_nuts.hip); it implies the library form (ml_form None or
"trajectory").  model="romml" | "rom" | "fom", both priors: ONE LEAF PER ROUND (csrc/hmc_nuts_model.hip; the statement nuts.LeafMachine /
transition_lockstep) -- a transition is finrom_hmc_nuts_begin, for j = 0, 1, ... the 2^j rounds of doubling j, finrom_hmc_nuts_end; a
round clears info, runs the model's own launches at Kq[0] (finrom_fom_gradient; finrom_romml_grad's plain launches; finrom_rom_grad at
theta_out, which begin and leaf write themselves; under a prior finrom_sampler_field / _pullback around the first two, the plain ROM
whitened through A = Sop U^T) and finrom_hmc_nuts_leaf, which keeps the tree's state in a workspace.  Every chain's doubling j covers
the same rounds, so the host reads active [C] back once per doubling, at most max_depth small read-backs per transition; a chain that
has ended sits at its draw.  graph=True captures begin, ONE round and end once each and replays them; the start point's evaluation is
a round too (_run_nuts_rounds), so a run continued with proposal0= is the uninterrupted one to the byte.  The result gains nuts_rounds
and nuts_readbacks.  Nuts(metric=) is refused with these three models.  Either form needs rng="philox" (momenta as before, the tree's direction bits and
uniforms from counter words 3 and 4, philox.nuts_top / nuts_leaf).  The result gains tree [proposals, C, 4] int32 (depth, leapfrog
steps, stop reason: 0 depth limit, 1 tree turned, 2 sub-tree turned, 3 diverged; moved) and accept_stat [proposals, C], the mean of
min(1, exp(H0 - H)) over the leaves: what dual averaging consumes.  accept counts the transitions whose draw is not the point
they started from.  Not with metric=, correct= or record=.
`Nuts(max_depth, metric=LowRankMetric)`: the transition under the Laplace metric -- the reference's `scaling`, on the sampler object as
it is there (the metric= keyword beside nuts= stays refused) -- in the chain's own coordinates: under prior= the whitened ones
(LowRankMetric.from_jacobian(J, prior, sigma)), under the i.i.d. prior the field's.  The momenta are M^(1/2) xi of the same standard
normals, the position moves by eps M^-1 p, the kinetic energy is p . M^-1 p / 2 and the U-turn criterion takes M^-1 p (nuts.py).  On the
device a transition is ONE finrom_hmc_nuts_ml_metric call with metric.device(); a metric of rank zero or None is the call above, bit
for bit.  A metric whose n is not the chains' is refused with both numbers.  The result gains metric_rho.
`Nuts(max_depth, adapt=StepAdapt(target_accept, tune))`: the dual-averaging warm-up of the step size (nuts.StepAdapt; Hoffman & Gelman
2014, Algorithm 5), the reference's `tune=100, target_accept=0.98`.  Every chain adapts its OWN step on its own accept_stat: the
transitions with global index < tune adapt, the later ones take exp(xbar); eps= is the starting point, mu = log(10 eps).  run_chains:
StepAdapt.update behind each transition.  Device functions, all four models, both priors, with or without Nuts(metric=), graph and stream
order: the transition's kernels read their chain's step from eps [C] on the device (finrom_hmc_nuts_ml_adapt / _ml_metric_adapt;
finrom_hmc_nuts_begin_adapt / _leaf_adapt) and ONE finrom_hmc_step_adapt_update launch follows the transition (inside the captured
transition; in the leaf-per-round form inside the `end` graph), which reads its row from the device's counter.  The result gains
step_size [proposals, C], the step each transition took, and adapt, the started StepAdapt at the end; StepAdapt(resume=res.adapt) with
proposal0=res.adapt.next continues the recursion.  stats= with a burn < tune is refused: the tuning draws are not draws of the target.
adapt=None: every path, launch and byte as before.

`correct=`: delayed acceptance (two-stage Metropolis, Christen & Fox 2005).  The trajectory runs under a surrogate -- model "romml",
"rom" or "ml" -- and the full-order model decides: stage 1 is the Metropolis test the chains make anyway, under the surrogate's
Hamiltonian; the end point then gets ONE full-order forward solve (QoI only: no adjoint, no gradient), and stage 2 accepts a
candidate that passed stage 1 with probability min(1, w(k') / w(k)), w = exp(-D), D = c_lik (loss_FOM - loss_surrogate).  The
priors cancel in w; stage 1 is reversible for the surrogate's posterior, so the two stages together are reversible for the
full-order posterior (the one the reference samples, pymc_func_bayes_inverse.py:174) at one forward solve per proposal instead of
n_leapfrog value-and-gradient calls.  run_chains takes a callable (fom_value(Fin, data)) and is the NumPy statement of
finrom_hmc_end_stage2; the device functions take the Fin.  Lockstep solves all C end points, also those stage 1 stopped.  The second
uniform is one more draw of the chain's generator per proposal, behind the first and whatever stage 1 said (rng="numpy"), or Philox
counter word 2 (philox.draw_block_stage2, finrom_hmc_draw_stage2).  The result gains accept1 [C] (proposals past stage 1; accept
is the final count), correction [proposals + 1, C] (row 0 the start's D, row q the candidate's: the surrogate's log-likelihood error
along the chain) and n_fom = proposals + 1; stats= records the full-order misfit.  Not with model="fom" (nothing to correct), not
with ChainStats(resume=...); the fused form has no metric form.

`record=`: a set of evaluation indices whose (input, loss, gradient) are kept in `recorded` for parity checks; on the device the
proposals that hold one run in stream order.  `keep_trace=`: the states after every proposal, row 0 the start.  `graph=`, `block=`
(device functions): replay a captured proposal or launch in stream order; how many proposals' draws a block holds."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np


class HmcResult(dict):
    __getattr__ = dict.__getitem__


class ChainStats:
    """Streaming posterior summaries of C chains in lockstep: the specification handed to a chain function (`stats=ChainStats(burn,
    batch)` or `ChainStats(resume=earlier.stats)`) and, started, the result `res.stats`.

    burn: draws are the states after the proposals with GLOBAL index >= burn (a rejected proposal repeats the state: a draw as well).
    batch: length of the batches whose means give the effective sample size (>= 1); a trailing partial batch stays in `bsum`.
    resume: the `stats` of the run this one continues (its burn and batch are taken over; the run must start at proposal0 =
    resume.next, the existing continuation rule).
    A started ChainStats holds, per chain and node [C, n]: mean, m2 (sum of squared deviations from the mean), bsum (sum of the open
    batch), bm_mean, bm_m2 (the same two moments of the closed batches' means), cur (field of the current state); per chain [C]:
    cur_loss; per proposal [proposals + 1, C] (row 0: the start point): misfit, accepted (int32 0 / 1); and first, next (global index
    of the first proposal covered, of the next one), t (draws) and n_batches (closed batches).  After a device run also `chain`:
    the end state with its potential and gradient, from which a run given resume= restarts to the bit (_restore_chain)."""
    SUMS = ("mean", "m2", "bsum", "bm_mean", "bm_m2")

    def __init__(self, burn=0, batch=32, resume=None):
        if resume is not None:
            if not isinstance(resume, ChainStats) or not resume.started:
                raise ValueError("ChainStats: resume= takes the stats a run returned")
            if (burn, batch) not in ((0, 32), (resume.burn, resume.batch)):
                raise ValueError(f"ChainStats: burn = {burn}, batch = {batch} differ from the resumed run's {resume.burn}, {resume.batch}")
            burn, batch = resume.burn, resume.batch
        if int(burn) != burn or burn < 0:
            raise ValueError(f"ChainStats: burn = {burn} is not a proposal index >= 0")
        if int(batch) != batch or batch < 1:
            raise ValueError(f"ChainStats: batch = {batch} is not a length >= 1")
        self.burn, self.batch, self.resume = int(burn), int(batch), resume
        self.first = self.next = None
        self.chain = None                                            # device runs: (state, U, dU) at the end, see _restore_chain

    started = property(lambda self: self.next is not None)
    t = property(lambda self: max(0, self.next - self.burn))
    n_batches = property(lambda self: self.t // self.batch)
    C = property(lambda self: self.mean.shape[0])

    def begin(self, field0, loss0, proposal0, proposals=0):
        """-> a started ChainStats for a run from the start point (field0 [C, n], loss0 [C]) whose first proposal has global index
        proposal0: zero sums, or a copy of resume's (then the current field and misfit are resume's too: the same state by the
        continuation rule, refused if field0 is not within 1e-9 of it).  proposals: rows of misfit / accepted to allocate ahead (they grow as needed)."""
        field0, loss0 = np.array(field0, dtype=np.float64, ndmin=2), np.array(loss0, dtype=np.float64, ndmin=1)
        C, r = field0.shape[0], self.resume
        loss0 = np.broadcast_to(loss0, (C,)).copy()
        s = ChainStats(self.burn, self.batch)
        if r is None:
            if proposal0 > self.burn:
                raise ValueError(f"ChainStats: proposal0 = {proposal0} > burn = {self.burn}: the draws of proposals {self.burn} .. "
                                 f"{proposal0 - 1} are not at hand (pass resume=, or a burn >= proposal0)")
            s.first = int(proposal0)
            for name in self.SUMS:
                setattr(s, name, np.zeros_like(field0))
            s.misfit, s.accepted = loss0[None].copy(), np.zeros((1, C), np.int32)
        else:
            if proposal0 != r.next:
                raise ValueError(f"ChainStats: the resumed run ended before proposal {r.next}; this one starts at proposal0 = {proposal0}")
            if r.mean.shape != field0.shape:
                raise ValueError(f"ChainStats: the resumed run had chains x nodes = {r.mean.shape}, this one {field0.shape}")
            s.first = r.first
            for name in self.SUMS:
                setattr(s, name, getattr(r, name).copy())
            s.misfit, s.accepted = r.misfit[:r._row + 1].copy(), r.accepted[:r._row + 1].copy()
            if not np.allclose(field0, r.cur, rtol=1e-9, atol=1e-9 * np.max(np.abs(r.cur))):
                raise ValueError("ChainStats: this run does not start from the resumed run's end state")
            field0, loss0 = r.cur.copy(), r.cur_loss.copy()          # the state the sums have seen, to the bit
        s._row = len(s.misfit) - 1
        s.misfit = np.concatenate([s.misfit, np.full((proposals, C), np.nan)])
        s.accepted = np.concatenate([s.accepted, np.zeros((proposals, C), np.int32)])
        s.next, s.cur, s.cur_loss = int(proposal0), field0, loss0
        return s

    def update(self, field, loss, ok, g):
        """The state after the proposal with global index g: field [C, n] and loss [C] at the trajectory's end point, ok [C] whether
        the chain accepted it.  The NumPy statement of finrom_hmc_stats_update's kernel: the same operations in the same order (no
        fused multiply-add on either side), so that the device's sums are these bits."""
        if g != self.next:
            raise ValueError(f"ChainStats.update: proposal {g} after proposal {self.next - 1}")
        ok = np.asarray(ok, dtype=bool)
        self.cur = np.where(ok[:, None], field, self.cur)
        self.cur_loss = np.where(ok, loss, self.cur_loss)
        self._row += 1
        if self._row == len(self.misfit):
            self.misfit = np.concatenate([self.misfit, self.cur_loss[None]])
            self.accepted = np.concatenate([self.accepted, np.zeros((1, len(ok)), np.int32)])
        self.misfit[self._row], self.accepted[self._row] = self.cur_loss, ok
        self.next = g + 1
        if g < self.burn:
            return
        t, x = g - self.burn + 1, self.cur
        d = x - self.mean
        self.mean = self.mean + d / float(t)
        self.m2 = self.m2 + d * (x - self.mean)
        self.bsum = self.bsum + x
        if t % self.batch == 0:
            b, bm = t // self.batch, self.bsum / float(self.batch)
            d = bm - self.bm_mean
            self.bm_mean = self.bm_mean + d / float(b)
            self.bm_m2 = self.bm_m2 + d * (bm - self.bm_mean)
            self.bsum = np.zeros_like(self.bsum)

    def select(self, chains):
        """The started stats of the listed chains, in that order."""
        s = ChainStats(self.burn, self.batch)
        s.first, s.next, s._row = self.first, self.next, self._row
        for name in self.SUMS + ("cur", "cur_loss"):
            setattr(s, name, getattr(self, name)[chains].copy())
        s.misfit, s.accepted = self.misfit[:, chains].copy(), self.accepted[:, chains].copy()
        return s

    @staticmethod
    def concat(parts):
        """The per-rank results of chains dealt over ranks, joined along the chain axis in the order given."""
        parts = list(parts)
        if not parts or not all(isinstance(p, ChainStats) and p.started for p in parts):
            raise ValueError("ChainStats.concat: needs the stats of finished runs")
        a = parts[0]
        for p in parts[1:]:
            if (p.t, p.burn, p.batch) != (a.t, a.burn, a.batch) or (p.first, p.next) != (a.first, a.next):
                raise ValueError(f"ChainStats.concat: (t, burn, batch, first, next) = {(p.t, p.burn, p.batch, p.first, p.next)} "
                                 f"against {(a.t, a.burn, a.batch, a.first, a.next)}")
            if p.mean.shape[1] != a.mean.shape[1]:
                raise ValueError("ChainStats.concat: different numbers of nodes")
        s = ChainStats(a.burn, a.batch)
        s.first, s.next, s._row = a.first, a.next, a._row
        for name in a.SUMS + ("cur", "cur_loss"):
            setattr(s, name, np.concatenate([getattr(p, name) for p in parts], axis=0))
        rows = a._row + 1
        s.misfit = np.concatenate([p.misfit[:rows] for p in parts], axis=1)
        s.accepted = np.concatenate([p.accepted[:rows] for p in parts], axis=1)
        return s

    def summarize(self):
        """Pooled over the chains, each [n]: mean, std (sqrt of var+), rhat (Gelman-Rubin, not split), ess (batch means) and mcse
        (Monte-Carlo standard error of `mean`):
          W = mean_c(m2 / (t - 1)),  B = t var_c(mean, ddof=1),  var+ = (t - 1) / t W + B / t,  rhat = sqrt(var+ / W),
          s^2 = batch mean_c(bm_m2 / (n_batches - 1)),  ess = C t W / s^2,  mcse = sqrt(s^2 / (C t)).
        One chain: rhat is NaN and var+ = (t - 1) / t W."""
        if not self.started or self.t < 2 or self.n_batches < 2:
            raise ValueError(f"ChainStats.summarize: needs >= 2 draws and >= 2 closed batches of {self.batch} "
                             f"(draws: {self.t if self.started else 0})")
        t, nb, C = self.t, self.n_batches, self.C
        W = np.mean(self.m2 / (t - 1), axis=0)
        Bv = t * np.var(self.mean, axis=0, ddof=1) if C > 1 else np.zeros_like(W)
        varp = (t - 1) / t * W + Bv / t
        s2 = self.batch * np.mean(self.bm_m2 / (nb - 1), axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            rhat = np.sqrt(varp / W) if C > 1 else np.full_like(W, np.nan)
            ess = C * t * W / s2
        return HmcResult(mean=np.mean(self.mean, axis=0), std=np.sqrt(varp), rhat=rhat, ess=ess, mcse=np.sqrt(s2 / (C * t)))


def stats_from_trace(trace, burn, batch, proposal0=0, resume=None, loss=None):
    """ChainStats.update run over a kept trace of FIELDS [P + 1, C, n]: row 0 is the start point, row j + 1 the state after the
    proposal with global index proposal0 + j.  loss [P + 1, C] (optional) fills `misfit` (NaN otherwise); `accepted` is whether the
    row differs from the one before (an accepted proposal moves every node)."""
    trace = np.asarray(trace, dtype=np.float64)
    P, C = trace.shape[0] - 1, trace.shape[1]
    loss = np.full((P + 1, C), np.nan) if loss is None else np.asarray(loss, dtype=np.float64)
    s = ChainStats(burn, batch, resume=resume).begin(trace[0], loss[0], proposal0, P)
    for j in range(P):
        s.update(trace[j + 1], loss[j + 1], np.any(trace[j + 1] != trace[j], axis=1), proposal0 + j)
    return s


def _restore_chain(stats, K, U, dU):
    """A device run given stats=ChainStats(resume=r) that starts from r's end state, to the bit, takes that state's potential U and
    gradient dU from r.chain in place of evaluation 0's.  The fused step forms the sub-fin averages of a trajectory's first point
    directly and those of the later ones from the previous momentum update's partial sums, so evaluation 0 of a continued run
    rounds differently from the evaluation that produced the state inside the first run (the continued chain then agrees with the
    uninterrupted one to 1e-9, tests/test_gpu_hmc_rng.py, not to the bit); with the saved values the continued run is the
    uninterrupted one bit for bit, and so are its sums."""
    import torch
    r = stats.resume if stats is not None else None
    if r is None or r.chain is None:
        return
    K0, U0, dU0 = r.chain
    if K0.shape == tuple(K.shape) and np.array_equal(K0, K.cpu().numpy()):
        U.copy_(torch.as_tensor(U0, dtype=U.dtype, device=U.device))
        dU.copy_(torch.as_tensor(dU0, dtype=dU.dtype, device=dU.device))


class _DeviceStats:
    """The buffers of finrom_hmc_stats_update as torch tensors on `dev`, started from the start point's field and misfit (device
    tensors [C, n], [C]); pt, acc: the chain state's counters (device tensors, acc at its start value)."""

    def __init__(self, spec, field0, loss0, proposal0, n_prop, pt, acc):
        import torch
        from .. import _ffi
        self._ffi, self._L, self.n_prop = _ffi, _ffi.lib(), n_prop
        self.host = spec.begin(field0.cpu().numpy(), loss0.cpu().numpy(), proposal0, n_prop)
        dev, h = field0.device, self.host
        Cn, n = field0.shape
        self.cur, self.cur_loss = (torch.as_tensor(a, dtype=torch.float64, device=dev).contiguous() for a in (h.cur, h.cur_loss))
        self.acc_prev = torch.stack([acc, acc]).contiguous()
        self.sums = [torch.as_tensor(getattr(h, name), dtype=torch.float64, device=dev).contiguous() for name in h.SUMS]
        self.misfit = torch.full((n_prop + 1, Cn), float("nan"), dtype=torch.float64, device=dev)
        self.misfit[0].copy_(self.cur_loss)
        self.accepted = torch.zeros(n_prop + 1, Cn, dtype=torch.int32, device=dev)
        self.desc = _ffi.HmcStats(C=Cn, n=n, proposal0=proposal0, burn=h.burn, batch=h.batch, pt=pt.data_ptr(), accept=acc.data_ptr(),
                                  cur=self.cur.data_ptr(), cur_loss=self.cur_loss.data_ptr(), acc_prev=self.acc_prev.data_ptr(),
                                  misfit=self.misfit.data_ptr(), accepted=self.accepted.data_ptr(),
                                  **{name: t.data_ptr() for name, t in zip(h.SUMS, self.sums)})

    def buffers(self):
        """Everything the launch writes: saved before a warm-up proposal and restored after the capture, with the chain state."""
        return [self.cur, self.cur_loss, self.acc_prev, self.misfit, self.accepted] + self.sums

    def update(self, cand, cand_loss):
        """One launch on torch's current stream: cand [C, n], cand_loss [C] (contiguous float64 device tensors) at the end point."""
        import ctypes as C
        import torch
        assert cand.is_contiguous() and cand.dtype == torch.float64 and cand.shape == self.cur.shape and cand_loss.dtype == torch.float64
        self.desc.cand, self.desc.cand_loss = cand.data_ptr(), cand_loss.data_ptr()
        self._ffi.check(self._L.finrom_hmc_stats_update(C.byref(self.desc), torch.cuda.current_stream().cuda_stream),
                        "finrom_hmc_stats_update")

    def result(self, K, U, dU):
        """The started host ChainStats with the device's sums and the chain's end state K, U, dU (synchronises)."""
        h = self.host
        h.chain = (K.cpu().numpy(), U.cpu().numpy(), dU.cpu().numpy())
        for name, t in zip(h.SUMS, self.sums):
            setattr(h, name, t.cpu().numpy())
        h.cur, h.cur_loss = self.cur.cpu().numpy(), self.cur_loss.cpu().numpy()
        if self.n_prop:
            h.misfit[h._row + 1:] = self.misfit[1:].cpu().numpy()
            h.accepted[h._row + 1:] = self.accepted[1:].cpu().numpy()
        h._row += self.n_prop
        h.next += self.n_prop
        return h


class _DeviceStepAdapt:
    """Nuts(adapt=) on the device: the three [C] arrays of finrom_hmc_step_adapt and step_size [proposals, C] as torch tensors, started
    from the host statement's state (nuts.StepAdapt.begin: the caller's eps, or resume's); pt: the chain state's counter,
    accept_stat [proposals, C]: what the transitions write."""

    def __init__(self, spec, eps0, Cn, proposal0, n_prop, pt, accept_stat):
        import torch
        from .. import _ffi
        self._ffi, self._L, self.C, self.proposal0, self.n_prop, self.pt, self.accept_stat = _ffi, _ffi.lib(), Cn, proposal0, n_prop, pt, accept_stat
        h = self.host = spec.begin(eps0, Cn, proposal0)
        f64 = dict(dtype=torch.float64, device=pt.device)
        self.eps, self.hbar, self.xbar = (torch.as_tensor(x, **f64).contiguous() for x in (h.eps, h.hbar, h.xbar))
        self.step_size = torch.zeros(n_prop, Cn, **f64)
        self.desc = _ffi.HmcStepAdapt(eps=self.eps.data_ptr(), hbar=self.hbar.data_ptr(), xbar=self.xbar.data_ptr(), mu=h.mu,
                                      target=h.target_accept, gamma=h.GAMMA, t0=h.T0, tune=h.tune)

    def buffers(self):
        """Everything the launch writes: saved before a warm-up transition and restored after the capture, with the chain state."""
        return [self.eps, self.hbar, self.xbar, self.step_size]

    def update(self):
        """One launch on torch's current stream, behind a transition and its counters' advance."""
        import ctypes as C
        import torch
        self._ffi.check(self._L.finrom_hmc_step_adapt_update(C.byref(self.desc), self.C, self.proposal0, self.pt.data_ptr(),
                                                             self.accept_stat.data_ptr(), self.step_size.data_ptr(),
                                                             torch.cuda.current_stream().cuda_stream), "finrom_hmc_step_adapt_update")

    def result(self, res):
        """res gains step_size and adapt, the started host StepAdapt with the device's end state (synchronises)."""
        h = self.host
        h.eps, h.hbar, h.xbar = self.eps.cpu().numpy(), self.hbar.cpu().numpy(), self.xbar.cpu().numpy()
        h.next = self.proposal0 + self.n_prop
        res["step_size"], res["adapt"] = self.step_size.cpu().numpy(), h
        return res


class _DeviceDA:
    """The buffers of delayed acceptance (finrom_hmc_end_stage1 / _stage2, finrom_hmc_draw_stage2) as torch tensors on `dev`, and the
    full-order solve between the two stages: `fin`'s "field" engine, QoI only."""

    def __init__(self, fin, Cn, n, data_t, per_sample, B, n_prop, dev):
        import torch
        from .. import _ffi
        self._ffi, self._L, self.C, self.n_prop, self.data_t = _ffi, _ffi.lib(), Cn, n_prop, data_t
        self.fom = fin._engine("field")
        if self.fom.xdim != n:
            raise ValueError(f"correct=: the full-order model takes fields of {self.fom.xdim} nodes, the chains have {n}")
        if data_t.shape[-1] != self.fom.n_obs:
            raise ValueError(f"correct=: the full-order model observes {self.fom.n_obs} values, data has {data_t.shape[-1]}")
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        self.ok1, self.Uq = torch.zeros(Cn, **i32), torch.zeros(Cn, **f64)
        self.qoi, self.info = torch.zeros(Cn, self.fom.n_obs, **f64), torch.zeros(Cn, **i32)
        self.lu2 = torch.zeros(B, Cn, **f64)
        self.D, self.loss_f, self.cand = torch.zeros(Cn, **f64), torch.zeros(Cn, **f64), torch.zeros(Cn, **f64)
        self.accept1 = torch.zeros(Cn, dtype=torch.int64, device=dev)
        self.correction = torch.full((n_prop + 1, Cn), float("nan"), **f64)
        self.desc = _ffi.HmcDa(n_obs=self.fom.n_obs, data_per_sample=per_sample, ok1=self.ok1.data_ptr(), Uq=self.Uq.data_ptr(),
                               qoi_f=self.qoi.data_ptr(), info_f=self.info.data_ptr(), data=data_t.data_ptr(),
                               lu2_block=self.lu2.data_ptr(), D=self.D.data_ptr(), loss_f=self.loss_f.data_ptr(),
                               accept1=self.accept1.data_ptr(), cand_loss_f=self.cand.data_ptr(), correction=self.correction.data_ptr())

    def buffers(self):
        """Everything stage 2 writes: saved before a warm-up proposal and restored after the capture, with the chain state."""
        return [self.D, self.loss_f, self.accept1, self.correction, self.cand]

    def solve(self, field):
        """qoi, info <- the full-order model at field [C, n] (a contiguous float64 device tensor), on torch's current stream: the
        flags cleared (the solve flags into them), then ONE finrom_fom_solve without w."""
        import torch
        assert field.is_contiguous() and field.dtype == torch.float64 and field.shape[0] == self.C
        self.info.zero_()
        self._ffi.check(self._L.finrom_fom_solve(self.fom._h, field.data_ptr(), self.C, self.qoi.data_ptr(), None, self.info.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "finrom_fom_solve")

    def misfit(self):
        r = self.qoi - self.data_t
        return (r * r).sum(dim=1).mul_(0.5)

    def start(self, field, loss_s, c_lik):
        """Evaluation 0 of the correcting model: loss_f, D = c_lik (loss_f - loss_s) and row 0 of `correction` (also warms the
        full-order workspace up before a capture).  ValueError for a flagged or non-finite start."""
        import torch
        self.solve(field)
        lossF = self.misfit()
        D = (lossF - loss_s).mul_(c_lik)
        if bool(self.info.ne(0).any()) or not bool(torch.isfinite(lossF).all()) or not bool(torch.isfinite(D).all()):
            raise ValueError("HMC start point: the correcting model is flagged or not finite there")
        self.loss_f.copy_(lossF); self.D.copy_(D); self.correction[0].copy_(D)

    def result(self):
        return dict(accept1=self.accept1.cpu().numpy(), correction=self.correction.cpu().numpy(), n_fom=self.n_prop + 1)


def potential(loss, grad, K, mean, sigma, tau):
    """U(k) = loss(k) / sigma^2 + |k - mean|^2 / (2 tau^2) and its gradient, row-wise for a batch K [C, n]."""
    d = K - mean
    U = np.asarray(loss, dtype=np.float64) / sigma ** 2 + 0.5 * np.einsum("cn,cn->c", d, d) / tau ** 2
    return U, np.asarray(grad, dtype=np.float64) / sigma ** 2 + d / tau ** 2


def whitened_potential(value_and_grad, prior, sigma):
    """The potential of chains in whitened coordinates under a GaussianFieldPrior, row-wise for a batch V [C, n]:
    U(v) = loss(k) / sigma^2 + |v|^2 / 2 and grad U = v + prior.pullback(grad_k) / sigma^2, k = prior.field(v).
    value_and_grad receives the fields k and returns (loss, field-space gradient, bad) as for run_chains.
    Returns f(V) -> (U, dU, K, loss, grad_k, bad)."""
    def f(V):
        K = prior.field(V)
        loss, grad, bad = value_and_grad(K)
        U, dU = potential(loss, prior.pullback(grad), V, 0.0, sigma, 1.0)
        return U, dU, K, loss, grad, bad
    return f


def _check_prior(prior, mean, who):
    if prior is not None and mean is not None:
        raise ValueError(f"{who}: with a prior the chains start from whitened points and the field's mean is the prior's (mean=None)")


def _check_rng(rng, seeds, proposal0, who):
    """rng="numpy": None.  rng="philox": the seeds as a uint64 array (ValueError for one outside [0, 2^64))."""
    if rng == "numpy":
        if proposal0 != 0:
            raise ValueError(f"{who}: proposal0 = {proposal0} needs rng='philox' (a NumPy generator cannot be advanced to a proposal)")
        return None
    if rng != "philox":
        raise ValueError(f"{who}: rng must be 'numpy' or 'philox', not {rng!r}")
    from . import philox
    if int(proposal0) != proposal0 or not 0 <= proposal0 < 1 << 62:
        raise ValueError(f"{who}: rng='philox': proposal0 = {proposal0} is not an index in [0, 2^62)")
    return philox.check_seeds(seeds)


def _device_draw(seeds64, dev, stage2=False):
    """draw(first, nb, P_dev, lu_dev): one finrom_hmc_draw launch on the current stream -- the draws of proposals first .. first + nb - 1
    of every chain into the head of the block buffers.  The seeds sit in an int64 tensor that holds the uint64 bit patterns.
    stage2: draw2(first, nb, lu2_dev) instead -- one finrom_hmc_draw_stage2 launch, the second log-uniforms (correct=)."""
    import torch
    from .. import _ffi
    L = _ffi.lib()
    seeds_t = torch.as_tensor(seeds64.view(np.int64), dtype=torch.int64, device=dev)
    if stage2:
        def draw2(first, nb, lu2_dev):
            _ffi.check(L.finrom_hmc_draw_stage2(seeds_t.data_ptr(), seeds_t.numel(), first, nb, lu2_dev.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "finrom_hmc_draw_stage2")
        return draw2

    def draw(first, nb, P_dev, lu_dev):
        _ffi.check(L.finrom_hmc_draw(seeds_t.data_ptr(), seeds_t.numel(), P_dev.shape[2], first, nb, P_dev.data_ptr(), lu_dev.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "finrom_hmc_draw")
    return draw


def _check_correct(correct, stats, who, model=None):
    """Delayed acceptance corrects a surrogate, and its sums are not continued."""
    if correct is None:
        return
    if model == "fom":
        raise ValueError(f"{who}: correct= with model='fom': the chains already run under the full-order model, there is nothing to correct")
    if stats is not None and stats.resume is not None:
        raise ValueError(f"{who}: correct= with ChainStats(resume=...) is not supported (start the sums anew, with a burn >= proposal0)")


def _check_metric(metric, n):
    """A rank-zero metric is the identity: the plain paths, bit for bit."""
    if metric is None or metric.rho == 0:
        return None
    if metric.n != n:
        raise ValueError(f"metric: n = {metric.n}, the chains have {n} coordinates")
    return metric


class _HostDraws:
    """rng="numpy": chain c draws from np.random.default_rng(seeds[c]), per proposal n standard normals (the momentum), one uniform
    and, under correct=, a second uniform behind it.  Each chain has its own generator and no draw depends on the state, so a
    proposal's uniforms may be drawn with its momentum, and proposals ahead of the chain."""

    def __init__(self, seeds, n):
        self.rngs, self.n = [np.random.default_rng(s) for s in seeds], n

    def block(self, nb, second=False, rows=None):
        """The next nb proposals -> P [rows, C, n], log u [rows, C], second log u [rows, C] (zeros unless second); rows >= nb
        (default nb), the rows behind nb zero."""
        rows = nb if rows is None else rows
        C = len(self.rngs)
        P, lu, lu2, u = np.zeros((rows, C, self.n)), np.zeros((rows, C)), np.zeros((rows, C)), np.ones((2, C))
        for j in range(nb):
            for c, r in enumerate(self.rngs):
                P[j, c] = r.standard_normal(self.n)
                u[0, c] = r.uniform()
                if second:
                    u[1, c] = r.uniform()
            with np.errstate(divide="ignore"):
                lu[j], lu2[j] = np.log(u[0]), np.log(u[1])
        return P, lu, lu2


def run_chains(value_and_grad, K0, n_evals, *, seeds, eps=2e-3, n_leapfrog=10, sigma=0.05, tau=0.5, mean=None, record=None,
               keep_trace=False, prior=None, metric=None, rng="numpy", proposal0=0, stats=None, correct=None, nuts=None):
    """Advance C = len(K0) chains in lockstep for `n_evals` value-and-gradient evaluations per chain.

    value_and_grad(K [C, n]) -> (loss [C], grad [C, n], bad [C] bool): ONE device call per leapfrog point; `bad` marks
    samples whose reduced operator was not positive definite (treated as infinite potential: the proposal is rejected).
    Under a prior it still receives fields, and `recorded` still holds (field, loss, field gradient).
    Under rng="philox" proposal i of this call takes philox.draw_block's draw of GLOBAL proposal proposal0 + i for seed seeds[c].
    correct: f(K [C, n] fields) -> (loss [C], bad [C]) of the model the chain is to be exact for (fom_value); it evaluates the start
    and every trajectory's end point.
    Returns HmcResult(K [C, n] final states (fields), accept [C] accepted proposals, proposals, n_evals (per chain),
    trace [proposals + 1, C, n] if keep_trace (fields), recorded = list of (eval index, K copy, loss, grad), stats = the started
    ChainStats of this run or None; with a prior also V [C, n], the whitened final states; under correct= also accept1, correction,
    n_fom and stage [proposals, C] (0: stopped at stage 1, 1: stopped at stage 2, 2: accepted)); under nuts= also tree, accept_stat
    and margin (_run_chains_nuts)."""
    _check_nuts(nuts, rng, metric, correct, record, "run_chains", stats)
    seeds64 = _check_rng(rng, seeds, proposal0, "run_chains")
    if nuts is not None:
        _check_prior(prior, mean, "run_chains")
        return _run_chains_nuts(value_and_grad, K0, n_evals, seeds64, eps, n_leapfrog, sigma, tau, mean, keep_trace, prior, proposal0,
                                stats, nuts)
    _check_correct(correct, stats, "run_chains")
    _check_prior(prior, mean, "run_chains")
    metric = _check_metric(metric, np.shape(K0)[-1])
    K = np.array(K0, dtype=np.float64, copy=True)
    C, n = K.shape
    if prior is None:
        mean = K.copy() if mean is None else np.broadcast_to(np.asarray(mean, dtype=np.float64), K.shape)

        def pot(Kq):
            loss, grad, bad = value_and_grad(Kq)
            U, dU = potential(loss, grad, Kq, mean, sigma, tau)
            return U, dU, Kq, loss, grad, bad
    else:
        pot = whitened_potential(value_and_grad, prior, sigma)
    if seeds64 is None:
        draws = _HostDraws(seeds, n)
        assert len(draws.rngs) == C
    else:
        from . import philox
        assert len(seeds64) == C
    recorded = []
    evals = 0
    last = {}                                                        # field and misfit of the last evaluation (stats=)

    def evaluate(Kq):
        nonlocal evals
        U, dU, Fq, loss, grad, bad = pot(Kq)
        last["field"], last["loss"] = Fq, loss
        if record is not None and evals in record:
            recorded.append((evals, Fq.copy(), np.array(loss, copy=True), np.array(grad, copy=True)))
        evals += 1
        bad = np.asarray(bad, dtype=bool) | ~np.isfinite(U)
        U = np.where(bad, np.inf, U)
        dU = np.where(bad[:, None], 0.0, dU)
        return U, dU

    U, dU = evaluate(K)                                              # evaluation 0: the starting point
    if not np.all(np.isfinite(U)):
        raise ValueError("HMC start point has an indefinite reduced operator")
    trace = [K.copy()] if keep_trace else None
    accept = np.zeros(C, np.int64)
    proposals = 0
    if correct is not None:                                          # delayed acceptance: D = c_lik (loss_FOM - loss_surrogate) at the start
        c_lik = 1.0 / sigma ** 2
        loss_f, bad_f = correct(last["field"])
        loss_f = np.array(loss_f, dtype=np.float64)
        with np.errstate(all="ignore"):
            D = c_lik * (loss_f - np.asarray(last["loss"], dtype=np.float64))
        if np.any(bad_f) or not np.all(np.isfinite(loss_f)) or not np.all(np.isfinite(D)):
            raise ValueError("HMC start point: the correcting model is flagged or not finite there")
        accept1, correction, stage = np.zeros(C, np.int64), [D.copy()], []
    cs = None if stats is None else stats.begin(last["field"], last["loss"] if correct is None else loss_f, proposal0,
                                                max(0, (n_evals - 1) // n_leapfrog))
    while evals + n_leapfrog <= n_evals:
        if seeds64 is None:
            Pb, lub, lub2 = draws.block(1, second=correct is not None)
        else:
            Pb, lub = philox.draw_block(seeds64, proposal0 + proposals, 1, n)
            if correct is not None:
                lub2 = philox.draw_block_stage2(seeds64, proposal0 + proposals, 1)
        P, lu = Pb[0], lub[0]
        H0 = U + 0.5 * np.einsum("cn,cn->c", P, P)                  # (under a metric: |xi|^2 / 2 = p^T M^-1 p / 2)
        if metric is not None:
            P = metric.apply(P, "sqrt")
        Kq, Pq, Uq, dUq = K.copy(), P.copy(), U, dU
        for _ in range(n_leapfrog):                                  # each step's input depends on the previous gradient
            Pq = Pq - 0.5 * eps * dUq
            Kq = Kq + eps * (Pq if metric is None else metric.apply(Pq, "inv"))
            Uq, dUq = evaluate(Kq)
            Pq = Pq - 0.5 * eps * dUq
        H1 = Uq + 0.5 * np.einsum("cn,cn->c", Pq, Pq if metric is None else metric.apply(Pq, "inv"))
        with np.errstate(over="ignore", invalid="ignore"):
            ok = np.isfinite(H1) & (lu < H0 - H1)
            if correct is not None:                                  # stage 2 (finrom_hmc_end_stage2's rule)
                lu2, ok1 = lub2[0], ok
                cand_f, bad_f = correct(last["field"])
                cand_f = np.asarray(cand_f, dtype=np.float64)
                Dq = c_lik * (cand_f - np.asarray(last["loss"], dtype=np.float64))
                good = ~np.asarray(bad_f, dtype=bool) & (np.abs(cand_f) <= 1.7e308) & np.isfinite(Dq)
                ok = ok1 & good & (lu2 < D - Dq)
                D, loss_f = np.where(ok, Dq, D), np.where(ok, cand_f, loss_f)
                accept1 += ok1
                correction.append(np.where(good, Dq, np.nan))
                stage.append(ok1.astype(np.int8) + ok)
        K = np.where(ok[:, None], Kq, K); U = np.where(ok, Uq, U); dU = np.where(ok[:, None], dUq, dU)
        accept += ok
        if cs is not None:                                           # (the last evaluation was the end point's)
            cs.update(last["field"], np.asarray(last["loss"], dtype=np.float64) if correct is None else np.where(good, cand_f, np.nan),
                      ok, proposal0 + proposals)
        proposals += 1
        if keep_trace:
            trace.append(K.copy())
    da = {} if correct is None else dict(accept1=accept1, correction=np.stack(correction), n_fom=proposals + 1,
                                         stage=np.array(stage, dtype=np.int8).reshape(proposals, C))
    if prior is not None:                                            # the states are v: report fields, and v beside them
        return HmcResult(K=prior.field(K), V=K, accept=accept, proposals=proposals, n_evals=evals, recorded=recorded,
                         trace=prior.field(np.stack(trace)) if keep_trace else None, stats=cs, **da)
    return HmcResult(K=K, accept=accept, proposals=proposals, n_evals=evals, recorded=recorded,
                     trace=np.stack(trace) if keep_trace else None, stats=cs, **da)


def _check_nuts(nuts, rng, metric, correct, record, who, stats=None):
    """nuts=Nuts(max_depth): what the No-U-turn transition is refused beside, each with its reason."""
    if nuts is None:
        return
    from .nuts import MAX_DEPTH_LIMIT
    depth = getattr(nuts, "max_depth", None)
    if depth is None or int(depth) != depth or not 1 <= depth <= MAX_DEPTH_LIMIT:
        raise ValueError(f"{who}: nuts= takes Nuts(max_depth) with max_depth in 1 .. {MAX_DEPTH_LIMIT}, not {depth!r}")
    if rng != "philox":
        raise ValueError(f"{who}: nuts= needs rng='philox' (a NumPy generator cannot serve a data-dependent number of draws reproducibly)")
    if metric is not None:
        raise ValueError(f"{who}: nuts= with metric=: the No-U-turn transition's metric belongs to the sampler object, pass it as "
                         f"Nuts(max_depth, metric=...) (a rank-zero metric included: pass none beside nuts=)")
    if correct is not None:
        raise ValueError(f"{who}: nuts= with correct=: delayed acceptance is a Metropolis test, the No-U-turn transition has none")
    if record is not None:
        raise ValueError(f"{who}: nuts= with record=: a tree's evaluations have no fixed indices to list")
    adapt = getattr(nuts, "adapt", None)
    if adapt is not None:                                            # (StepAdapt and Nuts refuse everything else where they are built)
        if stats is not None and stats.burn < adapt.tune:
            raise ValueError(f"{who}: Nuts(adapt=StepAdapt(tune={adapt.tune})) with ChainStats(burn={stats.burn}): the tuning draws are "
                             f"not draws of the target (the step size still moves): pass a burn >= tune")


def _run_chains_nuts(value_and_grad, K0, n_evals, seeds64, eps, n_leapfrog, sigma, tau, mean, keep_trace, prior, proposal0, stats, nuts):
    """run_chains under nuts=: (n_evals - 1) // n_leapfrog transitions of nuts.transition_iterative per chain, the momenta
    philox.draw_block's.  Works for any callable; a chain's tree is its own, so the chains are evaluated one row at a time.  Under a
    prior the chains move v with mean 0 and c_pri = 1 and the callable is wrapped in prior.field / prior.pullback.
    The result gains tree [proposals, C, 4] int32 (depth, leapfrog steps, stop reason -- 0 depth limit, 1 tree turned, 2 sub-tree
    turned, 3 diverged --, moved), accept_stat [proposals, C] (the mean of min(1, w) over the leaves) and margin (the smallest decision
    margin of the run); accept counts the transitions whose draw is not the point they started from; n_evals is 1 + the largest
    number of leaves any chain made.  Nuts(max_depth, metric=LowRankMetric): the transition under the metric (nuts.py), in the
    chain's own coordinates -- under a prior the whitened ones, LowRankMetric.from_jacobian's; the result gains metric_rho."""
    from . import nuts as N
    from . import philox
    K = np.array(K0, dtype=np.float64, copy=True)
    C, n = K.shape
    assert len(seeds64) == C
    metric = N.Nuts.metric_for(nuts, n, "run_chains")
    c_lik = 1.0 / sigma ** 2
    if prior is None:
        c_pri, field = 1.0 / tau ** 2, (lambda X: X)
        mean = K.copy() if mean is None else np.broadcast_to(np.asarray(mean, dtype=np.float64), K.shape)
        f = value_and_grad
    else:
        c_pri, field, mean = 1.0, prior.field, np.zeros_like(K)

        def f(V):
            loss, grad, bad = value_and_grad(prior.field(V))
            return loss, prior.pullback(np.asarray(grad, dtype=np.float64)), bad
    loss, grad, bad = f(K)                                           # evaluation 0: the starting point
    loss, d = np.array(loss, dtype=np.float64), K - mean
    dU = (c_lik / c_pri) * np.asarray(grad, dtype=np.float64) + d
    U = c_lik * loss + 0.5 * c_pri * np.einsum("cn,cn->c", d, d)
    if np.any(bad) or not np.all(np.isfinite(U)):
        raise ValueError("HMC start point has an indefinite reduced operator")
    n_prop = max(0, (n_evals - 1) // n_leapfrog)
    trace = [np.array(field(K))] if keep_trace else None
    accept = np.zeros(C, np.int64)
    tree, accept_stat, margin = np.zeros((n_prop, C, 4), np.int32), np.zeros((n_prop, C)), np.inf
    cs = None if stats is None else stats.begin(field(K), loss, proposal0, n_prop)
    ad = None if getattr(nuts, "adapt", None) is None else nuts.adapt.begin(eps, C, proposal0)
    step_size = np.zeros((n_prop, C))
    for q in range(n_prop):
        P = philox.draw_block(seeds64, proposal0 + q, 1, n)[0][0]
        for c in range(C):
            eps_c = eps if ad is None else float(ad.eps[c])
            r = N.transition_iterative(f, K[c], U[c], dU[c], loss[c], P[c], seed=seeds64[c], proposal=proposal0 + q, eps=eps_c, c_lik=c_lik,
                                       c_pri=c_pri, mean=mean[c], max_depth=nuts.max_depth, metric=metric)
            K[c], U[c], dU[c], loss[c] = r.k, r.U, r.dU, r.loss
            tree[q, c], accept_stat[q, c], margin, step_size[q, c] = r.tree, r.accept_stat, min(margin, r.margin), eps_c
        if ad is not None:
            ad.update(accept_stat[q], proposal0 + q)
        accept += tree[q, :, 3]
        if cs is not None:
            cs.update(field(K), loss.copy(), tree[q, :, 3] != 0, proposal0 + q)
        if keep_trace:
            trace.append(np.array(field(K)))
    more = dict(tree=tree, accept_stat=accept_stat, margin=margin, nuts=nuts.max_depth, metric_rho=0 if metric is None else metric.rho)
    if ad is not None:
        more.update(step_size=step_size, adapt=ad)
    evals = 1 + (int(tree[:, :, 1].sum(axis=0).max()) if n_prop else 0)
    return HmcResult(K=field(K).copy(), **({} if prior is None else {"V": K}), accept=accept, proposals=n_prop, n_evals=evals, recorded=[],
                     trace=np.stack(trace) if keep_trace else None, stats=cs, **more)


def romml_value_and_grad(solver_r):
    """The evaluation the reference's SqErrorOpROMML performs, batched over chains: AffineROMFin.grad_romml_batch."""
    def f(K):
        res = solver_r.grad_romml_batch(K)
        return np.asarray(res["loss"]), np.asarray(res["grad"]), np.asarray(res["info"]) != 0
    return f


def fom_value_and_grad(solver, data):
    """The evaluation the reference's SqErrorOpFOM performs (pymc_func_bayes_inverse.py:174), batched over chains: Fin.gradient_batch
    at nodal fields against the observations `data`."""
    data = np.ascontiguousarray(data, dtype=np.float64)

    def f(K):
        res = solver.gradient_batch(np.ascontiguousarray(K, dtype=np.float64), data)
        return np.asarray(res["J"]), np.asarray(res["grad"]), np.asarray(res["info"]) != 0
    return f


def fom_value(solver, data):
    """The full-order misfit alone, batched over chains: f(K [C, n] fields) -> (loss [C], bad [C]) from Fin.forward_batch without w
    (one forward solve, no adjoint).  The callable run_chains(..., correct=) takes."""
    data = np.ascontiguousarray(data, dtype=np.float64)

    def f(K):
        res = solver.forward_batch(np.ascontiguousarray(K, dtype=np.float64), want_w=False)
        r = np.asarray(res["qoi"]) - data
        return 0.5 * np.einsum("co,co->c", r, r), np.asarray(res["info"]) != 0
    return f


def rom_value_and_grad(solver_r, data=None):
    """The plain reduced model's evaluation (SqErrorOpROM), batched over chains: AffineROMFin.grad_reduced_batch and the chain rule
    through the sub-fin averages, dJ/dk = g_theta @ dsigma_dk.  data: None = solver_r.data."""
    def f(K):
        res = solver_r.grad_reduced_batch(np.ascontiguousarray(K, dtype=np.float64), data=data)
        return np.asarray(res["J"]), np.asarray(res["g_theta"]) @ solver_r.dsigma_dk, np.asarray(res["info"]) != 0
    return f


def ml_value_and_grad(surrogate, data):
    """The pure deep-learning surrogate's evaluation (the reference's MLSolverWrapper), batched over chains:
    dl_model.Surrogate.misfit_grad_batch at nodal fields against the observations `data`; flagged where the loss is not finite."""
    data = np.ascontiguousarray(data, dtype=np.float64)

    def f(K):
        res = surrogate.misfit_grad_batch(np.ascontiguousarray(K, dtype=np.float64), data)
        return np.asarray(res["loss"]), np.asarray(res["grad"]), np.asarray(res["info"]) != 0
    return f


MODELS = ("romml", "rom", "fom", "ml")


def _check_model(model, solver_r, solver, data, who, surrogate=None):
    """ValueError for a model the chains do not know and for a model without what it evaluates with."""
    if model not in MODELS:
        raise ValueError(f"{who}: unknown model {model!r} (romml, rom, fom, ml)")
    if surrogate is not None and model != "ml":
        raise ValueError(f"{who}: surrogate= belongs to model='ml'; model={model!r} does not evaluate with it")
    if model == "ml":
        if surrogate is None:
            raise ValueError(f"{who}: model='ml' needs surrogate=Surrogate")
        if data is None:
            raise ValueError(f"{who}: model='ml' needs data= (the observations)")
        if solver is not None:
            raise ValueError(f"{who}: solver= belongs to model='fom'; model='ml' evaluates with surrogate=")
    elif model == "fom":
        if solver is None:
            raise ValueError(f"{who}: model='fom' needs solver=Fin")
        if data is None:
            raise ValueError(f"{who}: model='fom' needs data= (the observations)")
    else:
        if solver is not None:
            raise ValueError(f"{who}: solver= belongs to model='fom'; model={model!r} evaluates with solver_r")
        if solver_r is None:
            raise ValueError(f"{who}: model={model!r} needs solver_r=AffineROMFin")
        if data is None and getattr(solver_r, "data", None) is None:
            raise ValueError(f"{who}: model={model!r} needs data= (or solver_r.data)")
    return model


ML_FORMS = ("steps", "trajectory")


def _check_ml_form(ml_form, model, who, fused=None):
    """ValueError for an ml_form the chains do not know, for one beside another model and for one with fused=False."""
    if ml_form is None:
        return
    if ml_form not in ML_FORMS:
        raise ValueError(f"{who}: unknown ml_form {ml_form!r} (None, 'steps', 'trajectory')")
    if model != "ml":
        raise ValueError(f"{who}: ml_form= belongs to model='ml'; model={model!r} has its own fused step")
    if fused is not None and not fused:
        raise ValueError(f"{who}: ml_form={ml_form!r} is a fused form; fused=False asks for the torch-op form")


def _device_model(model, solver_r, solver, data_t, surrogate=None):
    """f(F [C, n] device tensor) -> dict(loss [C], grad [C, n], info [C]) on torch's current stream: the calls that
    estimate_MAP.objective(kind).device makes, one adapter per model."""
    if model == "ml":
        return lambda Fq: surrogate.misfit_grad_batch(Fq, data_t)
    if model == "romml":
        return lambda Fq: solver_r.grad_romml_batch(Fq, data=data_t)
    if model == "fom":
        def f(Fq):
            r = solver.gradient_batch(Fq, data_t)
            return {"loss": r["J"], "grad": r["grad"], "info": r["info"]}
        return f
    import torch
    S_t = torch.as_tensor(np.ascontiguousarray(solver_r.dsigma_dk, dtype=np.float64), dtype=torch.float64, device=data_t.device)

    def f(Fq):
        r = solver_r.grad_reduced_batch(None, data=data_t, theta=solver_r._avg(Fq))
        # g_theta @ dsigma_dk as one broadcast product and one reduction over the nine averages (no BLAS call inside a captured graph)
        return {"loss": r["J"], "grad": (r["g_theta"][:, :, None] * S_t[None]).sum(dim=1), "info": r["info"]}
    return f


class _DeviceChains:
    """What device-resident chains are in either form: the checks, the state and block tensors, the draws, the capture recipe, the
    block loop with its records, and the result.  `a` holds the chain function's arguments by name.  A form calls, in this order,
    allocate(), start() behind its evaluation 0, start_stats(), capture() and run(); it supplies `proposal(rec)` -- one proposal on
    torch's current stream on the tensors below, with note() behind every evaluation when rec.

    Tensors (static: a captured proposal reads and writes the same buffers at every replay): K [C, n], U [C], dU [C, n] the state with
    its potential and gradient; P_dev [B, C, n], lu_dev [B, C] (da.lu2 under correct=) the draws of a block of B proposals; jt the
    proposal inside the block, pt the proposal of the chain (trace row), acc [C] the accept counters; trace [proposals + 1, C, n] or
    None; mean_t [C, n] (zeros under a prior, with c_pri = 1); data_t; fs, fmean the prior's sampler and mean (None without one);
    da, ds the buffers of correct= and stats= (None without)."""

    def __init__(self, who, a):
        self.a = a
        self.seeds64 = _check_rng(a.rng, a.seeds, a.proposal0, who)
        _check_model(a.model, a.solver_r, a.solver, a.data, who, a.surrogate)
        _check_correct(a.correct, a.stats, who, a.model)
        _check_ml_form(a.ml_form, a.model, who, a.fused)
        _check_nuts(a.nuts, a.rng, a.metric, a.correct, a.record, who, a.stats)
        if a.nuts is not None:                                       # two library forms: one launch per transition ("ml"), one leaf per launch
            if a.fused is not None and not a.fused:
                raise ValueError(f"{who}: nuts= is a library form (finrom_hmc_nuts_ml; finrom_hmc_nuts_begin / _leaf / _end); fused=False "
                                 f"asks for the torch-op form")
            if a.ml_form == "steps":
                raise ValueError(f"{who}: nuts= is one launch per transition; ml_form='steps' asks for three launches per step")
            from .nuts import Nuts
            self.nuts_metric = Nuts.metric_for(a.nuts, np.shape(a.K0)[-1], who)     # (refused here where its n is not the chains')
            if a.model != "ml":
                holder, name, need = {"fom": (a.solver, "solver=Fin", "gradient_batch"), "rom": (a.solver_r, "solver_r=AffineROMFin", "grad_reduced_batch"),
                                      "romml": (a.solver_r, "solver_r=AffineROMFin", "grad_romml_batch")}[a.model]
                if not hasattr(holder, need):
                    raise ValueError(f"{who}: nuts= with model={a.model!r} launches the model's own gradient between two leaves and needs "
                                     f"{name} (the transition in one launch belongs to model='ml' and its surrogate)")
                if self.nuts_metric is not None:
                    raise ValueError(f"{who}: Nuts(metric=...) with model={a.model!r}: the leaf kernel (finrom_hmc_nuts_leaf) has no form under "
                                     f"the Laplace metric; the metric's transition is model='ml' alone (finrom_hmc_nuts_ml_metric)")

    def allocate(self):
        import torch
        a = self.a
        dev = torch.device("cuda", torch.cuda.current_device())
        f64, i64 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int64, device=dev)
        K = self.K = torch.as_tensor(np.ascontiguousarray(a.K0, dtype=np.float64), **f64).clone()
        Cn, n = K.shape
        tau, self.fs, self.fmean = a.tau, None, None
        if a.prior is not None:                                      # whitened: N(0, I), c_pri = 1
            self.mean_t, tau = torch.zeros_like(K), 1.0
            self.fs, self.fmean = a.prior.device(), torch.as_tensor(a.prior.mean, **f64)
        else:
            self.mean_t = K.clone() if a.mean is None else torch.as_tensor(
                np.broadcast_to(np.asarray(a.mean, dtype=np.float64), (Cn, n)).copy(), **f64)
        self.data_t = torch.as_tensor(np.ascontiguousarray(a.solver_r.data if a.data is None else a.data, dtype=np.float64), **f64)
        self.per_sample = 1 if self.data_t.ndim == 2 else 0
        self.c_lik, self.c_pri = 1.0 / a.sigma ** 2, 1.0 / tau ** 2
        self.n_prop = max(0, (a.n_evals - 1) // a.n_leapfrog)
        B = self.B = max(1, min(a.block, self.n_prop))
        self.U, self.dU = torch.zeros(Cn, **f64), torch.zeros_like(K)
        self.P_dev, self.lu_dev = torch.zeros(B, Cn, n, **f64), torch.zeros(B, Cn, **f64)
        self.jt, self.pt, self.acc = torch.zeros(1, **i64), torch.zeros(1, **i64), torch.zeros(Cn, **i64)
        self.trace = torch.zeros(self.n_prop + 1, Cn, n, **f64) if a.keep_trace else None
        self.da = self.ds = None
        if a.correct is not None:
            self.da = _DeviceDA(a.correct, Cn, n, self.data_t, self.per_sample, B, self.n_prop, dev)
        if self.seeds64 is None:
            self.host_draws = _HostDraws(a.seeds, n)
            assert len(self.host_draws.rngs) == Cn
        else:
            assert len(self.seeds64) == Cn
            self.draw = _device_draw(self.seeds64, dev)
            self.draw2 = _device_draw(self.seeds64, dev, stage2=True) if self.da is not None else None
        self.recorded, self.evals, self._moved = [], 0, []

    def note(self, read, *args):
        """Behind an evaluation made in stream order: if `record` lists it, read(*args) -> (input, loss, gradient), device tensors
        or arrays, is copied out."""
        if self.a.record is not None and self.evals in self.a.record:
            self.recorded.append((self.evals,) + tuple(x if isinstance(x, np.ndarray) else x.cpu().numpy().copy() for x in read(*args)))
        self.evals += 1

    def start(self, Uv, dUq):
        """Behind evaluation 0: its potential Uv [C] and gradient dUq [C, n] (/ c_pri) become the state's (ValueError for a start that
        is flagged or not finite), row 0 of the trace, and a resumed chain takes its saved values (_restore_chain)."""
        import torch
        self.U.copy_(Uv)
        if not bool(torch.isfinite(self.U).all()):
            raise ValueError("HMC start point has an indefinite reduced operator")
        self.dU.copy_(dUq)
        if self.trace is not None:
            self.trace[0].copy_(self.K)
        _restore_chain(self.a.stats, self.K, self.U, self.dU)

    def start_stats(self, field0, loss0):
        """stats=: the sums start from the start point's field [C, n] and the misfit [C] they record (the correcting model's under correct=)."""
        if self.a.stats is not None:
            self.ds = _DeviceStats(self.a.stats, field0, loss0, self.a.proposal0, self.n_prop, self.pt, self.acc)

    def capture(self, proposal, extra=()):
        """-> proposal() captured as a torch.cuda.CUDAGraph, or None under graph=False or with no proposal to make.  The warm-up
        torch's recipe asks for moves the state, the counters and the sums of stats= and correct=; they are put back (restore)."""
        import torch
        if not self.a.graph or self.n_prop == 0:
            return None
        moved = [self.K, self.U, self.dU, self.acc, self.jt, self.pt]
        moved += (self.ds.buffers() if self.ds is not None else []) + (self.da.buffers() if self.da is not None else []) + list(extra)
        self._moved = [(t, t.clone()) for t in moved]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                               # warm-up on a side stream
            proposal()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            proposal()
        self.restore()                                              # (the warm-up moved the state; the capture does not run)
        return g

    def restore(self):
        for t, t0 in self._moved:
            t.copy_(t0)

    def run(self, proposal, g, **labels):
        """All proposals, block by block -> the HmcResult (result).  A block's draws are one finrom_hmc_draw launch behind the previous
        block's replays (rng="philox"), or the host chain's, drawn without waiting for the device -- they do not depend on the state,
        so the host draws while the device works on the previous block -- and uploaded.  A proposal that holds an evaluation listed
        in `record` runs in stream order, proposal(True); every other one is a replay of g, or proposal(False) without a graph."""
        import torch
        a, da, L = self.a, self.da, self.a.n_leapfrog
        done = 0
        while done < self.n_prop:
            nb = min(self.B, self.n_prop - done)
            if self.seeds64 is not None:
                self.draw(a.proposal0 + done, nb, self.P_dev, self.lu_dev)
                if da is not None:
                    self.draw2(a.proposal0 + done, nb, da.lu2)
            else:
                P, lu, lu2 = self.host_draws.block(nb, second=da is not None, rows=self.B)
                self.P_dev.copy_(torch.from_numpy(P)); self.lu_dev.copy_(torch.from_numpy(lu))
                if da is not None:
                    da.lu2.copy_(torch.from_numpy(lu2))
            self.jt.zero_()
            for j in range(nb):
                first = 1 + (done + j) * L                          # evaluation indices of this proposal: first .. first + L - 1
                if a.record is not None and any(first <= e < first + L for e in a.record):
                    assert self.evals == first
                    proposal(True)
                else:
                    g.replay() if g is not None else proposal(False)
                    self.evals += L
            done += nb
        return self.result(graph=g is not None, **labels)

    def result(self, graph, fused, **more):
        """Synchronises.  Under a prior the states are v: K and trace are mapped to fields by the library, after the run (outside any
        replayed graph), and V holds the whitened end states."""
        K, V, trace = self.K, None, self.trace
        cs = self.ds.result(K, self.U, self.dU) if self.ds is not None else None
        da = self.da.result() if self.da is not None else {}
        if self.fs is not None:
            V, K = K, self.fs.field(K, mean=self.fmean)
            if trace is not None:
                trace = self.fs.field(trace.reshape(-1, K.shape[1]), mean=self.fmean).reshape(trace.shape)
        return HmcResult(K=K.cpu().numpy(), **({} if V is None else {"V": V.cpu().numpy()}), accept=self.acc.cpu().numpy(),
                         proposals=self.n_prop, n_evals=self.evals, recorded=self.recorded,
                         trace=trace.cpu().numpy() if trace is not None else None, graph=graph, fused=fused, stats=cs,
                         model=self.a.model, **da, **more)


def _fused_form(a):
    """The fused step form of (model, prior, metric), chosen before anything is allocated: raises what the combination is refused
    with -- _ffi.FinromError with status FINROM_ERR_UNSUPPORTED where the library has no such step, so that fused=None falls back --
    or returns bind(ch, Kq, loss) -- ch the allocated _DeviceChains, Kq the state's two position buffers, loss its misfit buffer --
    which acquires the model's handles, allocates the form's own buffers and returns the form:
      step(state, i, want_grad)  leapfrog step i on a finrom_hmc_state, on torch's current stream; want_grad: the raw misfit
                                 gradient is kept for read()
      read(i)                    (input, loss, gradient) of the evaluation step i made, as `recorded` holds it
      field, needs_field         the tensor with the field of the point a step moved to (None: the position buffer is the field);
                                 needs_field: no step forms it, one finrom_sampler_field launch does where stats= or correct= ask
      mh                         the metric's handle (finrom_hmc_begin_metric / _end_metric around the trajectory), or None
      trajectory(state)          all n_leapfrog steps in one launch (ml_form="trajectory"), or None.

      model    prior  metric   step
      romml    -      -        finrom_hmc_leapfrog
      romml    field  -        finrom_hmc_leapfrog_field
      romml    field  M        finrom_hmc_leapfrog_field_metric
      fom      -      -        finrom_hmc_leapfrog_fom
      fom      field  -        finrom_hmc_leapfrog_field_fom
      rom      -      -        finrom_hmc_leapfrog_rom, A = Sop
      rom      field  -        finrom_hmc_leapfrog_rom, A = Sop U^T, theta0 = Sop mean: whitened, no field during a trajectory
      ml       any    -        finrom_hmc_leapfrog_ml (finrom_hmc_trajectory_ml), under a prior on surrogate.whitened(prior):
                               whitened, no field during a trajectory, and read() gives (v, loss, gradient with respect to v)."""
    from .. import _ffi
    model, prior, solver_r, surrogate = a.model, a.prior, a.solver_r, a.surrogate
    n = np.shape(a.K0)[-1]

    def unsupported(what):
        return _ffi.FinromError(f"run_chains_fused failed (status {_ffi.ERR_UNSUPPORTED}): {what}")

    if model == "ml":                                                # everything refused before the device is touched
        if a.ml_form is None and a.nuts is None:
            raise unsupported("model='ml' has no fused leapfrog step (pass fused=False)")
        metric = _check_metric(a.metric, n)
        if metric is not None:
            raise unsupported("the fused leapfrog steps of model='ml' have no metric form (pass fused=False and no ml_form)")
        if np.shape(a.data)[-1] != surrogate.n_out or np.ndim(a.data) not in (1, 2):
            raise ValueError(f"run_chains_fused: data must be [{surrogate.n_out}] or [C, {surrogate.n_out}], got {np.shape(a.data)}")
        if n != surrogate.n_in:
            raise ValueError(f"run_chains_fused: the chains have {n} coordinates, the surrogate {surrogate.n_in} inputs")
        if not surrogate.device:
            raise _ffi.FinromError("run_chains_fused needs the surrogate on the device (Surrogate(model, device=True))")
        _check_prior(prior, a.mean, "run_chains_fused")
    else:
        if model == "romml" and solver_r._dev_model is None:
            raise _ffi.FinromError("run_chains_fused needs the error model on the device (a ResBnFcModel)")
        _check_prior(prior, a.mean, "run_chains_fused")
        metric = _check_metric(a.metric, n)
        if metric is not None and prior is None:
            raise unsupported("the fused leapfrog step under the i.i.d. prior has no metric form (pass prior=, or fused=False)")
        if metric is not None and model != "romml":
            raise unsupported(f"the fused leapfrog steps of model={model!r} have no metric form (pass fused=False)")
        if metric is not None and a.correct is not None:
            raise unsupported("delayed acceptance (correct=) has no metric form of the fused step (pass fused=False)")
        if model == "rom":                                           # theta = theta0 + A x, gradient A^T g_theta (x: k, or v under a prior)
            S_np = np.ascontiguousarray(solver_r.dsigma_dk, dtype=np.float64)
            if not np.array_equal(S_np, solver_r.ops.S):             # (one map serves theta and the chain rule)
                raise unsupported("the reduced model's averaging operator and dsigma_dk differ (pass fused=False)")

    def bind(ch, Kq, loss):                                          # (a step holds, by name, every tensor it passes by address)
        import ctypes as C
        import torch
        L, check = _ffi.lib(), _ffi.check
        K, data_p, per = ch.K, ch.data_t.data_ptr(), ch.per_sample
        f64 = dict(dtype=torch.float64, device=K.device)
        grad_rec = torch.zeros_like(K)                               # raw misfit gradient, written only for recorded evaluations
        form = SimpleNamespace(field=None, needs_field=False, mh=None, trajectory=None, read=lambda i: (Kq[(i + 1) & 1], loss, grad_rec))
        if prior is not None:
            F, grad_f = torch.zeros_like(K), torch.zeros_like(K)     # the step's field and misfit gradient
            form.field, fs_h, fmean_p = F, ch.fs._h, ch.fmean.data_ptr()

        def stream():
            return torch.cuda.current_stream().cuda_stream

        def kept(want_grad):
            return grad_rec.data_ptr() if want_grad else None

        if model == "ml":                                            # under a prior: the field folded into the first layer
            mlp = (surrogate.whitened(prior) if prior is not None else surrogate)._dev
            form.needs_field, form.mlp = prior is not None, mlp

            def step(state, i, want_grad):
                check(L.finrom_hmc_leapfrog_ml(mlp._h, C.byref(state), i, data_p, per, kept(want_grad), None, stream()),
                      "finrom_hmc_leapfrog_ml")
            if a.ml_form == "trajectory":
                def trajectory(state):
                    check(L.finrom_hmc_trajectory_ml(mlp._h, C.byref(state), a.n_leapfrog, data_p, per, stream()),
                          "finrom_hmc_trajectory_ml")
                form.trajectory = trajectory
        elif model == "fom":
            fom = a.solver._engine("field")
            fom._enable_gradient()
            if prior is not None:
                form.read = lambda i: (F, loss, grad_f)

                def step(state, i, want_grad):
                    check(L.finrom_hmc_leapfrog_field_fom(fom._h, fs_h, fmean_p, F.data_ptr(), grad_f.data_ptr(), C.byref(state), i,
                                                          data_p, per, None, stream()), "finrom_hmc_leapfrog_field_fom")
            else:
                def step(state, i, want_grad):                      # (the gradient between the model's launches and the kick: grad_rec)
                    check(L.finrom_hmc_leapfrog_fom(fom._h, C.byref(state), i, data_p, per, grad_rec.data_ptr(), None, stream()),
                          "finrom_hmc_leapfrog_fom")
        elif model == "rom":
            rom = solver_r._rom
            solver_r._ensure_gradient()
            A_t = torch.as_tensor(np.ascontiguousarray(S_np @ prior.U.T) if prior is not None else S_np, **f64)
            th0 = torch.as_tensor(S_np @ prior.mean, **f64) if prior is not None else None
            theta_b, gth_b = torch.zeros(K.shape[0], S_np.shape[0], **f64), torch.zeros(K.shape[0], S_np.shape[0], **f64)
            if prior is not None:                                    # field and field-space gradient, formed for the record alone
                form.needs_field = True
                form.read = lambda i: (ch.fs.field(Kq[(i + 1) & 1], mean=ch.fmean), loss, gth_b.cpu().numpy() @ S_np)

            def step(state, i, want_grad):
                check(L.finrom_hmc_leapfrog_rom(rom._h, A_t.data_ptr(), th0.data_ptr() if th0 is not None else None, C.byref(state), i,
                                                data_p, per, theta_b.data_ptr(), gth_b.data_ptr(), kept(want_grad and prior is None),
                                                None, stream()), "finrom_hmc_leapfrog_rom")
        else:
            rom, mlp, Sop = solver_r._rom, solver_r._dev_model, solver_r._avg._S
            solver_r._ensure_gradient()
            if prior is not None:
                form.read = lambda i: (F, loss, grad_f)
            if metric is not None:
                mh, vel = metric.device(), torch.zeros_like(K)      # the step's velocity M^-1 p
                form.mh = mh

                def step(state, i, want_grad):
                    check(L.finrom_hmc_leapfrog_field_metric(rom._h, mlp._h, Sop.ptr, fs_h, fmean_p, F.data_ptr(), grad_f.data_ptr(),
                                                             C.byref(state), i, data_p, per, None, None, mh._h, vel.data_ptr(),
                                                             stream()), "finrom_hmc_leapfrog_field_metric")
                    Sop.used_on(stream())
            elif prior is not None:
                def step(state, i, want_grad):
                    check(L.finrom_hmc_leapfrog_field(rom._h, mlp._h, Sop.ptr, fs_h, fmean_p, F.data_ptr(), grad_f.data_ptr(),
                                                      C.byref(state), i, data_p, per, None, None, stream()), "finrom_hmc_leapfrog_field")
                    Sop.used_on(stream())
            else:
                def step(state, i, want_grad):
                    check(L.finrom_hmc_leapfrog(rom._h, mlp._h, Sop.ptr, C.byref(state), i, data_p, per, kept(want_grad), None, None,
                                                stream()), "finrom_hmc_leapfrog")
                    Sop.used_on(stream())
        form.step = step
        return form
    return bind


def _run_nuts_rounds(a, ch, st, Kq0, loss, info):
    """run_chains_fused under nuts= for model "fom" | "rom" | "romml": the No-U-turn transition with ONE LEAF PER ROUND of all chains
    (csrc/hmc_nuts_model.hip; the statement: nuts.LeafMachine / transition_lockstep).  ch: the allocated _DeviceChains, st its
    finrom_hmc_state, Kq0 the position every round evaluates, loss / info the evaluation's misfit and flags.
    A transition: finrom_hmc_nuts_begin; for j = 0, 1, ... the 2^j rounds of doubling j; finrom_hmc_nuts_end (finrom_hmc_stats_update
    behind it under stats=).  A round: info cleared, the model's own launches at Kq[0], finrom_hmc_nuts_leaf:
      fom    i.i.d.  finrom_fom_gradient at Kq[0] -> grad
             field   finrom_sampler_field -> finrom_fom_gradient -> finrom_sampler_pullback -> grad (whitened: mean zeros, c_pri = 1)
      romml  the same two with finrom_romml_grad, its plain launches
      rom    theta_out = theta0 + A Kq[0] written by begin / leaf themselves; finrom_rom_grad at it -> g_theta; i.i.d. A = Sop, under a
             prior A = Sop U^T, theta0 = Sop m: no field, no triangular product.
    Every chain's doubling j covers the same rounds, so the host reads active [C] back ONCE per doubling and stops when no chain is
    active: at most max_depth small read-backs per transition.  graph=True: begin, ONE round and end are each captured once; the leaf
    kernel reads j, i, m and d from the workspace, so the round's graph is replayed with no node parameter changed.
    The start point's evaluation is a round too (finrom_hmc_nuts_leaf with active = 2), before any capture: it warms the model's
    workspaces up with the same C and leaves the state's U and dU in a leaf's arithmetic, so a run continued with proposal0= from a
    draw (K, or V under a prior; an explicit mean=) is the uninterrupted run to the byte."""
    import ctypes as C
    import torch
    from .. import _ffi
    L, check = _ffi.lib(), _ffi.check
    model, prior, solver_r, depth = a.model, a.prior, a.solver_r, a.nuts.max_depth
    K = ch.K
    Cn, n = K.shape
    f64, i32 = dict(dtype=torch.float64, device=K.device), dict(dtype=torch.int32, device=K.device)
    data_p, per = ch.data_t.data_ptr(), ch.per_sample

    def stream():
        return torch.cuda.current_stream().cuda_stream

    ws = torch.zeros(L.finrom_hmc_nuts_ws_bytes(Cn, n, depth) // 8, **f64)
    seeds_t = torch.as_tensor(ch.seeds64.view(np.int64), dtype=torch.int64, device=K.device)
    tree, accept_stat = torch.zeros(ch.n_prop, Cn, 4, **i32), torch.zeros(ch.n_prop, Cn, **f64)
    active, state_loss = torch.zeros(Cn, **i32), torch.zeros(Cn, **f64)
    tr = _ffi.HmcNutsTree(ws=ws.data_ptr(), seeds=seeds_t.data_ptr(), proposal0=a.proposal0, max_depth=depth, state_loss=state_loss.data_ptr(),
                          tree=tree.data_ptr(), accept_stat=accept_stat.data_ptr(), active=active.data_ptr())
    ad = None                                                        # Nuts(adapt=): each chain's own step, the update behind `end`
    if a.nuts.adapt is not None:
        ad = _DeviceStepAdapt(a.nuts.adapt, a.eps, Cn, a.proposal0, ch.n_prop, ch.pt, accept_stat)
    grad = gth = A_t = th0 = theta = None                            # (a round holds, by name, every tensor it passes by address)
    P = 0
    if prior is not None:
        F, gF, fs_h, fmean_p = torch.zeros_like(K), torch.zeros_like(K), ch.fs._h, ch.fmean.data_ptr()
    if model == "rom":
        rom = solver_r._rom
        solver_r._ensure_gradient()
        S_np = np.ascontiguousarray(solver_r.dsigma_dk, dtype=np.float64)
        P = S_np.shape[0]
        A_t = torch.as_tensor(np.ascontiguousarray(S_np @ prior.U.T) if prior is not None else S_np, **f64)
        th0 = torch.as_tensor(S_np @ prior.mean, **f64) if prior is not None else None
        theta, gth = torch.zeros(Cn, P, **f64), torch.zeros(Cn, P, **f64)

        def evaluate():
            check(L.finrom_rom_grad(rom._h, theta.data_ptr(), data_p, per, Cn, loss.data_ptr(), gth.data_ptr(), None, None, info.data_ptr(),
                                    stream()), "finrom_rom_grad")
    else:
        grad = torch.zeros_like(K)
        if model == "fom":
            fom = a.solver._engine("field")
            fom._enable_gradient()

            def at(X, g):
                check(L.finrom_fom_gradient(fom._h, X.data_ptr(), data_p, per, Cn, g.data_ptr(), loss.data_ptr(), None, info.data_ptr(),
                                            stream()), "finrom_fom_gradient")
        else:
            rom, mlp, Sop = solver_r._rom, solver_r._dev_model, solver_r._avg._S
            solver_r._ensure_gradient()

            def at(X, g):
                check(L.finrom_romml_grad(rom._h, mlp._h, Sop.ptr, X.data_ptr(), data_p, per, Cn, g.data_ptr(), loss.data_ptr(), None, None,
                                          info.data_ptr(), stream()), "finrom_romml_grad")
                Sop.used_on(stream())
        if prior is None:
            def evaluate():
                at(Kq0, grad)
        else:
            def evaluate():
                check(L.finrom_sampler_field(fs_h, fmean_p, Kq0.data_ptr(), Cn, F.data_ptr(), stream()), "finrom_sampler_field")
                at(F, gF)
                check(L.finrom_sampler_pullback(fs_h, gF.data_ptr(), Cn, grad.data_ptr(), stream()), "finrom_sampler_pullback")
    ptr = lambda t: t.data_ptr() if t is not None else None
    map_args = (ptr(A_t), ptr(th0), P, ptr(theta))

    def begin(state=st):
        if ad is not None and state is st:                           # (the start point's round: the plain begin with eps = 0)
            check(L.finrom_hmc_nuts_begin_adapt(C.byref(state), C.byref(tr), ad.eps.data_ptr(), *map_args, stream()),
                  "finrom_hmc_nuts_begin_adapt")
        else:
            check(L.finrom_hmc_nuts_begin(C.byref(state), C.byref(tr), *map_args, stream()), "finrom_hmc_nuts_begin")

    def round_():
        info.zero_()
        evaluate()
        if ad is not None:
            check(L.finrom_hmc_nuts_leaf_adapt(C.byref(st), C.byref(tr), ad.eps.data_ptr(), ptr(grad), ptr(gth), *map_args, stream()),
                  "finrom_hmc_nuts_leaf_adapt")
        else:
            check(L.finrom_hmc_nuts_leaf(C.byref(st), C.byref(tr), ptr(grad), ptr(gth), *map_args, stream()), "finrom_hmc_nuts_leaf")

    def end():
        check(L.finrom_hmc_nuts_end(C.byref(st), C.byref(tr), stream()), "finrom_hmc_nuts_end")
        if ad is not None:
            ad.update()
        if ch.ds is not None:                                        # (Kq[0] holds the draw: where it moved, the sums take it)
            ch.ds.update(field_of_draw(), state_loss)

    def field_of_draw():
        if prior is None:
            return Kq0
        check(L.finrom_sampler_field(fs_h, fmean_p, Kq0.data_ptr(), Cn, F.data_ptr(), stream()), "finrom_sampler_field")
        return F

    # evaluation 0, a round: Kq[0] = K (and theta_out) by a begin with eps = 0, the model, the leaf call that writes the state
    st0 = _ffi.HmcState.from_buffer_copy(st)
    st0.eps = 0.0
    begin(st0)
    active.fill_(2)
    round_()
    ch.evals += 1
    ch.start(ch.U.clone(), ch.dU.clone())
    ch.start_stats(field_of_draw().clone() if a.stats is not None else None, state_loss)
    counts = dict(rounds=0, readbacks=0)
    graphs = None
    if a.graph and ch.n_prop > 0:
        def captured(fn):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            return g
        torch.cuda.synchronize()
        graphs = tuple(captured(fn) for fn in (begin, round_, end))

    def transition(rec=False):
        g_begin, g_round, g_end = graphs if graphs is not None else (None, None, None)
        g_begin.replay() if graphs else begin()
        for j in range(depth):
            for _ in range(1 << j):
                g_round.replay() if graphs else round_()
            counts["rounds"] += 1 << j
            counts["readbacks"] += 1
            if not bool(active.any()):                               # ONE small read-back per doubling
                break
        g_end.replay() if graphs else end()

    res = ch.run(transition, SimpleNamespace(replay=transition) if graphs else None, fused=True, nuts=depth, metric_rho=0)
    res["nuts_rounds"], res["nuts_readbacks"] = counts["rounds"], counts["readbacks"]
    res["tree"], res["accept_stat"] = tree.cpu().numpy(), accept_stat.cpu().numpy()
    if np.any(res["tree"][:, :, 2] < 0):
        raise _ffi.FinromError(f"run_chains_fused: a chain was still active after 2^{depth} - 1 rounds (tree rows with reason -1)")
    res["n_evals"] = 1 + (int(res["tree"][:, :, 1].sum(axis=0).max()) if ch.n_prop else 0)
    return res if ad is None else ad.result(res)


def run_chains_fused(solver_r, K0, n_evals, *, seeds, eps=2e-3, n_leapfrog=10, sigma=0.05, tau=0.5, mean=None, record=None,
                     keep_trace=False, graph=True, data=None, block=32, prior=None, metric=None, rng="numpy", proposal0=0,
                     stats=None, model="romml", solver=None, correct=None, surrogate=None, ml_form=None, nuts=None):
    """Device-resident chains with the trajectory's arithmetic INSIDE the library (include/finrom.h).  A proposal is finrom_hmc_begin,
    n_leapfrog steps of the form _fused_form chose -- each the model's own launches with the position update in front and the
    momentum update behind -- and finrom_hmc_end; under metric= finrom_hmc_begin_metric, the metric step, finrom_hmc_end_metric;
    under ml_form="trajectory" ONE finrom_hmc_trajectory_ml launch in the place of the steps (the steps' bits; evaluation 0 and the
    proposals with a recorded evaluation run in the step form).  correct=Fin: finrom_hmc_end_stage1 in the place of finrom_hmc_end,
    finrom_fom_solve without w at the end point's field (flags cleared in front), finrom_hmc_end_stage2.  stats=: one
    finrom_hmc_stats_update launch behind that, on the end point's field.  Where the step forms no field (the whitened forms of
    "rom" and "ml"), one finrom_sampler_field launch per proposal forms the end point's for correct= and stats= together.  All of it
    is one linear chain of launches, captured once and replayed; a capture that fails raises.
    nuts=Nuts(max_depth) (model="ml"): a proposal is ONE finrom_hmc_nuts_ml call (the tree's kernel and the counters' advance) -- a whole No-U-turn transition of every chain, the
    statement nuts.transition_iterative -- in the place of begin, steps and end; the momenta are finrom_hmc_draw's, finrom_sampler_field
    and finrom_hmc_stats_update follow where prior= / stats= ask for them, under a prior the chain runs on surrogate.whitened(prior).
    The result gains tree and accept_stat as run_chains has them.
    nuts=Nuts(max_depth) (model="romml" | "rom" | "fom"): one leaf per round, finrom_hmc_nuts_begin / _leaf / _end around the model's
    own launches (_run_nuts_rounds); the same result fields, and nuts_rounds, nuts_readbacks.
    Raises _ffi.FinromError (FINROM_ERR_UNSUPPORTED) where the library has no such step (_fused_form) before anything is allocated:
    run_chains_device(fused=None) then takes the torch-op form.
    Same random numbers, same order of evaluations and the same chains as run_chains up to the rounding of fused multiply-adds; the
    result of run_chains_device with fused=True, and ml_form where one was named.  `recorded` holds (field, loss, field gradient);
    for model="ml" under a prior (v, loss, gradient with respect to v): that chain runs on surrogate.whitened(prior) and knows no
    field-space gradient."""
    a = SimpleNamespace(fused=None, **locals())
    ch = _DeviceChains("run_chains_fused", a)
    bind = _fused_form(a)
    import ctypes as C
    import torch
    from .. import _ffi
    L, check = _ffi.lib(), _ffi.check
    ch.allocate()
    K, da = ch.K, ch.da
    Cn, n = K.shape
    f64 = dict(dtype=torch.float64, device=K.device)
    Kq = [torch.empty_like(K), torch.empty_like(K)]
    P, dUq = torch.zeros_like(K), torch.zeros_like(K)
    H0, loss, info = torch.zeros(Cn, **f64), torch.zeros(Cn, **f64), torch.zeros(Cn, dtype=torch.int32, device=K.device)
    st = _ffi.HmcState(C=Cn, n=n, eps=eps, c_lik=ch.c_lik, c_pri=ch.c_pri, mean=ch.mean_t.data_ptr(), K=K.data_ptr(), U=ch.U.data_ptr(),
                       dU=ch.dU.data_ptr(), Kq=(C.c_void_p * 2)(Kq[0].data_ptr(), Kq[1].data_ptr()), P=P.data_ptr(), dUq=dUq.data_ptr(),
                       H0=H0.data_ptr(), P_block=ch.P_dev.data_ptr(), lu_block=ch.lu_dev.data_ptr(), jt=ch.jt.data_ptr(),
                       pt=ch.pt.data_ptr(), accept=ch.acc.data_ptr(), trace=ch.trace.data_ptr() if ch.trace is not None else None,
                       loss=loss.data_ptr(), info=info.data_ptr())
    st0 = _ffi.HmcState.from_buffer_copy(st)                         # evaluation 0: a "step" of length zero from K itself
    st0.eps = 0.0
    if nuts is not None and model != "ml":
        return _run_nuts_rounds(a, ch, st, Kq[0], loss, info)
    form = bind(ch, Kq, loss)
    step, mh = form.step, form.mh

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def field_at(X):
        """The tensor that holds the field of the point X the last step moved to (or of the start point)."""
        if form.field is None:
            return X
        if form.needs_field:
            check(L.finrom_sampler_field(ch.fs._h, ch.fmean.data_ptr(), X.data_ptr(), Cn, form.field.data_ptr(), stream()),
                  "finrom_sampler_field")
        return form.field

    if nuts is not None:
        seeds_t = torch.as_tensor(ch.seeds64.view(np.int64), dtype=torch.int64, device=K.device)
        tree = torch.zeros(ch.n_prop, Cn, 4, dtype=torch.int32, device=K.device)
        accept_stat = torch.zeros(ch.n_prop, Cn, **f64)
        nmh = ch.nuts_metric.device() if ch.nuts_metric is not None else None      # (a rank-zero or absent metric: the plain tree)
        ad = None                                                    # Nuts(adapt=): each chain's own step, the update behind the tree
        if nuts.adapt is not None:
            ad = _DeviceStepAdapt(nuts.adapt, eps, Cn, proposal0, ch.n_prop, ch.pt, accept_stat)

    def transition(rec=False):
        if ad is not None:
            tail = (seeds_t.data_ptr(), proposal0, nuts.max_depth, ch.data_t.data_ptr(), ch.per_sample, tree.data_ptr(),
                    accept_stat.data_ptr(), stream())
            if nmh is not None:
                check(L.finrom_hmc_nuts_ml_metric_adapt(form.mlp._h, C.byref(st), nmh._h, ad.eps.data_ptr(), *tail),
                      "finrom_hmc_nuts_ml_metric_adapt")
            else:
                check(L.finrom_hmc_nuts_ml_adapt(form.mlp._h, C.byref(st), ad.eps.data_ptr(), *tail), "finrom_hmc_nuts_ml_adapt")
            ad.update()
        elif nmh is not None:
            check(L.finrom_hmc_nuts_ml_metric(form.mlp._h, C.byref(st), nmh._h, seeds_t.data_ptr(), proposal0, nuts.max_depth,
                                              ch.data_t.data_ptr(), ch.per_sample, tree.data_ptr(), accept_stat.data_ptr(), stream()),
                  "finrom_hmc_nuts_ml_metric")
        else:
            check(L.finrom_hmc_nuts_ml(form.mlp._h, C.byref(st), seeds_t.data_ptr(), proposal0, nuts.max_depth, ch.data_t.data_ptr(),
                                       ch.per_sample, tree.data_ptr(), accept_stat.data_ptr(), stream()), "finrom_hmc_nuts_ml")
        if ch.ds is not None:                                        # (Kq[0] and loss hold the draw: where it moved, the sums take it)
            ch.ds.update(field_at(Kq[0]), loss)

    def proposal(rec=False):
        if mh is not None:
            check(L.finrom_hmc_begin_metric(C.byref(st), mh._h, stream()), "finrom_hmc_begin_metric")
        else:
            check(L.finrom_hmc_begin(C.byref(st), stream()), "finrom_hmc_begin")
        if form.trajectory is not None and not rec:
            form.trajectory(st)
        else:
            for i in range(n_leapfrog):                              # each step's input depends on the previous gradient
                step(st, i, rec)
                if rec:
                    ch.note(form.read, i)
        if mh is not None:
            check(L.finrom_hmc_end_metric(C.byref(st), mh._h, n_leapfrog, stream()), "finrom_hmc_end_metric")
        elif da is not None:                                         # the surrogate's test; the full-order model's follows below
            check(L.finrom_hmc_end_stage1(C.byref(st), n_leapfrog, da.ok1.data_ptr(), da.Uq.data_ptr(), stream()), "finrom_hmc_end_stage1")
        else:
            check(L.finrom_hmc_end(C.byref(st), n_leapfrog, stream()), "finrom_hmc_end")
        if da is not None or ch.ds is not None:
            Fq = field_at(Kq[n_leapfrog & 1])                        # the end point's field: one launch at most, shared
        if da is not None:
            da.solve(Fq)
            check(L.finrom_hmc_end_stage2(C.byref(st), n_leapfrog, C.byref(da.desc), stream()), "finrom_hmc_end_stage2")
        if ch.ds is not None:
            ch.ds.update(Fq, loss if da is None else da.cand)

    # evaluation 0: the starting point (also warms the library up: workspaces, function attributes)
    Kq[0].copy_(K)
    step(st0, 0, True)                                               # Kq[1] = K + 0 * P, dUq = grad U / c_pri at K
    ch.note(form.read, 0)
    D = K - ch.mean_t
    Uv = torch.linalg.vecdot(D, D).mul_(0.5 * ch.c_pri).add_(loss, alpha=ch.c_lik)
    ch.start(torch.nan_to_num_(Uv, nan=float("inf"), posinf=float("inf"), neginf=float("inf")).masked_fill_(info.ne(0), float("inf")), dUq)
    F0 = field_at(K) if stats is not None or da is not None else None   # (also warms the field kernel's workspace up, before a capture)
    if da is not None:                                               # evaluation 0 of the full-order model (warms its workspace up)
        da.start(F0, loss, ch.c_lik)
    ch.start_stats(F0, loss if da is None else da.loss_f)
    if nuts is not None:                                             # (loss is the state's misfit here: the warm-up moves it too)
        g = ch.capture(transition, extra=[loss, Kq[0], tree, accept_stat] + (ad.buffers() if ad is not None else []))
        if g is not None and ch.trace is not None:
            ch.trace[1].zero_()
        res = ch.run(transition, g, fused=True, nuts=nuts.max_depth, metric_rho=0 if ch.nuts_metric is None else ch.nuts_metric.rho,
                     **({} if ml_form is None else {"ml_form": ml_form}))
        res["tree"], res["accept_stat"] = tree.cpu().numpy(), accept_stat.cpu().numpy()
        res["n_evals"] = 1 + (int(res["tree"][:, :, 1].sum(axis=0).max()) if ch.n_prop else 0)
        return res if ad is None else ad.result(res)
    g = ch.capture(proposal)
    if g is not None and ch.trace is not None:                       # (the warm-up's row; proposal 0 writes it again)
        ch.trace[1].zero_()
    return ch.run(proposal, g, fused=True, **({} if ml_form is None else {"ml_form": ml_form}))


def run_chains_device(solver_r, K0, n_evals, *, seeds, eps=2e-3, n_leapfrog=10, sigma=0.05, tau=0.5, mean=None, record=None,
                      keep_trace=False, graph=True, data=None, block=32, fused=None, prior=None, metric=None, rng="numpy",
                      proposal0=0, stats=None, model="romml", solver=None, correct=None, surrogate=None, ml_form=None, nuts=None):
    """`run_chains` with the chains RESIDENT ON THE DEVICE (torch tensors on the current CUDA device): positions, momenta,
    potentials, the Metropolis test and the accept counters never visit the host.  A whole PROPOSAL -- momentum in, n_leapfrog
    steps, Hamiltonians, accept / reject, state update -- is captured once in a HIP graph (torch.cuda.CUDAGraph: the library
    launches on torch's capture stream) and replayed: one graph launch per proposal, no synchronisation until the chain ends; the
    graph picks its proposal's draws out of the block by a device-side counter.  graph=False: the same launches in stream order.
    Proposals that contain an evaluation index listed in `record` run in stream order too, step by step, so that the evaluation's
    input, loss and gradient can be copied out.

    fused=True: run_chains_fused.  fused=None (the default): run_chains_fused, and where it refuses the combination
    (_ffi.FinromError) and no ml_form is named, the form below.  fused=False, the torch-op form: a step is a few elementwise torch
    kernels around ONE model call (_device_model; under a prior FieldSampler.field in front of it and FieldSampler.pullback behind),
    the metric's maps are finrom_metric_apply launches (engine.MetricHandle), correct= is the rule of finrom_hmc_end_stage2 in torch
    ops around correct.forward_batch(field, want_w=False), stats= one finrom_hmc_stats_update launch behind the state update.  It
    serves every model, prior and metric.  A capture that fails is warned about and the proposals run in stream order.
    Same chains as run_chains over the model's host callable (romml_value_and_grad(solver_r), fom_value_and_grad(solver, data),
    rom_value_and_grad(solver_r, data), ml_value_and_grad(surrogate, data)) up to the rounding of the elementwise updates.
    Returns HmcResult(K [C, n] (NumPy; fields), V under a prior, accept, proposals, n_evals, recorded, trace, graph: whether a graph
    was replayed, fused, stats, model; under correct= accept1, correction, n_fom; ml_form where one was named)."""
    a = SimpleNamespace(**locals())
    ch = _DeviceChains("run_chains_device", a)
    import torch
    metric = _check_metric(metric, np.shape(K0)[-1])
    if fused is None or fused:
        from .. import _ffi
        kw = dict(vars(a), metric=metric)
        del kw["fused"]
        try:
            return run_chains_fused(**kw)
        except _ffi.FinromError:
            if fused or ml_form is not None or nuts is not None:
                raise
    _check_prior(prior, mean, "run_chains_device")
    ch.allocate()
    K, U, dU, jt, pt, da, fs, fmean, mean_t, c_lik, c_pri = ch.K, ch.U, ch.dU, ch.jt, ch.pt, ch.da, ch.fs, ch.fmean, ch.mean_t, ch.c_lik, ch.c_pri
    C, n = K.shape
    f64 = dict(dtype=torch.float64, device=K.device)
    model_eval = _device_model(model, solver_r, solver, ch.data_t, surrogate)
    mh = metric.device() if metric is not None else None
    # work tensors (static, like the state: the graph's operands)
    Kq, Pq, D, dUq = (torch.empty_like(K) for _ in range(4))
    P0, lu = torch.zeros(1, C, n, **f64), torch.zeros(1, C, **f64)
    out = {}
    if da is not None:                                               # delayed acceptance: finrom_hmc_end_stage2's state and rule in torch ops
        lu2, nan_c = torch.zeros(1, C, **f64), torch.full((C,), float("nan"), **f64)

    def fom_misfit(Fq):
        """(loss_f [C], flagged [C]) of the correcting model at the fields Fq: one forward solve, no adjoint."""
        res = correct.forward_batch(Fq, want_w=False)
        r = res["qoi"] - ch.data_t
        return (r * r).sum(dim=1).mul_(0.5), res["info"].ne(0)

    def evaluate():
        """dUq (= grad U / c_pri), out <- value and gradient at Kq."""
        Fq = fs.field(Kq, mean=fmean) if prior is not None else Kq  # (with a prior, Kq is v and the misfit is taken at its field)
        res = model_eval(Fq)
        gq = fs.pullback(res["grad"]) if prior is not None else res["grad"]
        torch.sub(Kq, mean_t, out=D)
        torch.add(D, gq, alpha=c_lik / c_pri, out=dUq)              # dU / c_pri (one kernel; c_pri rides in the momentum updates' alpha)
        dUq.masked_fill_(res["info"].ne(0)[:, None], 0.0)           # an indefinite reduced operator: no force, rejected below
        out["loss"], out["grad"], out["info"], out["field"] = res["loss"], res["grad"], res["info"], Fq

    def read():
        return out["field"], out["loss"], out["grad"]

    inf = float("inf")

    def potential_now():
        # (as few kernels as possible: each is a node of the proposal's graph, ~1.6 us)
        Uv = torch.add(torch.linalg.vecdot(D, D).mul_(0.5 * c_pri), out["loss"], alpha=c_lik)
        return torch.nan_to_num_(Uv, nan=inf, posinf=inf, neginf=inf).masked_fill_(out["info"].ne(0), inf)

    def proposal(rec=False):
        """One proposal on the static tensors: momentum and log u of slice jt, trajectory, Metropolis test, state update."""
        ds = ch.ds
        torch.index_select(ch.P_dev, 0, jt, out=P0)
        torch.index_select(ch.lu_dev, 0, jt, out=lu)
        H0 = torch.add(U, torch.linalg.vecdot(P0[0], P0[0]), alpha=0.5)
        Kq.copy_(K); dUq.copy_(dU)
        torch.add(P0[0] if mh is None else mh.apply(P0[0], "sqrt"), dUq, alpha=-0.5 * eps * c_pri, out=Pq)     # first half step
        for _ in range(n_leapfrog):                                 # each step's input depends on the previous gradient
            Kq.add_(Pq if mh is None else mh.apply(Pq, "inv"), alpha=eps)
            evaluate()
            Pq.add_(dUq, alpha=-eps * c_pri)                       # two half steps; the ends of a trajectory correct by +- eps/2
            if rec:
                ch.note(read)
        Pq.add_(dUq, alpha=0.5 * eps * c_pri)                       # the last update was a whole step: back to a half
        Uq = potential_now()
        H1 = torch.add(Uq, torch.linalg.vecdot(Pq, Pq) if mh is None else mh.apply(Pq, "inv", want_quad=True)[1], alpha=0.5)
        ok = lu[0] < H0 - H1                                        # (H1 = inf or nan compares false, as on the host: rejected)
        if da is not None:                                          # stage 2: the full-order misfit at the end point decides
            torch.index_select(da.lu2, 0, jt, out=lu2)
            lossF, flagged = fom_misfit(out["field"])
            Dq = (lossF - out["loss"]).mul_(c_lik)
            good = ~flagged & (lossF.abs() <= 1.7e308) & torch.isfinite(Dq)
            da.accept1.add_(ok)
            ok = ok & good & (lu2[0] < da.D - Dq)
            torch.where(ok, Dq, da.D, out=da.D); torch.where(ok, lossF, da.loss_f, out=da.loss_f)
            torch.where(good, lossF, nan_c, out=da.cand)
        torch.where(ok[:, None], Kq, K, out=K); torch.where(ok, Uq, U, out=U); torch.where(ok[:, None], dUq, dU, out=dU)
        ch.acc.add_(ok)
        jt.add_(1); pt.add_(1)
        if ch.trace is not None:
            ch.trace.index_copy_(0, pt, K[None])
        if da is not None:
            da.correction.index_copy_(0, pt, torch.where(good, Dq, nan_c)[None])
        if ds is not None:                                          # (out holds the last evaluation: the end point's)
            ds.update(out["field"], out["loss"] if da is None else da.cand)

    Kq.copy_(K); Pq.zero_()
    evaluate()                                                      # evaluation 0: the starting point (also warms the library up)
    ch.note(read)
    ch.start(potential_now(), dUq)
    if da is not None:                                               # evaluation 0 of the correcting model
        lossF, flagged = fom_misfit(out["field"])
        D0 = (lossF - out["loss"]).mul_(c_lik)
        if bool(flagged.any()) or not bool(torch.isfinite(lossF).all()) or not bool(torch.isfinite(D0).all()):
            raise ValueError("HMC start point: the correcting model is flagged or not finite there")
        da.loss_f.copy_(lossF); da.D.copy_(D0); da.correction[0].copy_(D0)
    ch.start_stats(out["field"], out["loss"] if da is None else da.loss_f)
    try:
        g = ch.capture(proposal)
    except Exception as exc:                                        # no graph support for this sequence: plain stream order
        import warnings
        warnings.warn(f"hmc: HIP graph capture failed ({exc!r}); the proposals are launched kernel by kernel")
        g = None
        ch.restore()
    return ch.run(proposal, g, fused=False)

