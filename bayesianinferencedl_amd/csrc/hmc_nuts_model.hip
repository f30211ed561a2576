// The No-U-turn transition under ANY model (finrom_hmc_nuts_begin / _leaf / _end; hmc.py model="fom" | "rom" | "romml" with nuts=):
// hmc_nuts.hip's tree with ONE LEAF PER LAUNCH and the tree's bookkeeping in memory, so that a model's own launches -- the full-order
// gradient, the reduced one, the reduced one with its learned correction -- can sit between two leaves.  The statement is nuts.py's
// LeafMachine (transition_iterative cut at the model call); the reference runs this sampler under the full-order operator
// (bayesian_inference/inference.py:21-57,165-166).
//
// A round of the chains is: the model's value and gradient at Kq[0] (into st->loss, st->info and grad or g_theta), then the leaf
// kernel, which finishes the leapfrog step at that point (dU', p', the energy, the divergence test, the weight, the streamed
// selection, rho_sub, the checkpoint or the U-turn tests), at a sub-tree's end adopts it (the candidate IS the chain's state), tests
// the tree and draws the next sub-tree, and leaves in Kq[0] either the next leaf's drifted position or, the transition over, the draw.
//
// Layout, shared by the three kernels: one 1024-thread workgroup per chain; element i of every per-chain array belongs to thread
// i % 1024, so an element is read back by the thread that wrote it, in this launch or an earlier one.  Every sum goes through
// block_sum_1024 / block_sum2_1024; every fused multiply-add is written fma(...), nothing else contracts.  Control flow is uniform
// over the workgroup: thread 0 decides and broadcasts through LDS behind a barrier (each broadcast word is written once per launch).
// A workgroup waits on no other: workgroup barriers only.  The Philox counters, both uniforms, the stop reasons, the tree row and
// accept_stat are finrom_hmc_nuts_ml's.
//
// The state in memory (finrom_hmc_nuts_ws_bytes): 13 + 2 max_depth arrays [C x n] -- both edges (k, p, dU), the walker's p', its
// half-kicked p1/2 and dU' (its position is Kq[0] itself), the sub-tree's candidate (k, dU), rho, rho_sub, a checkpoint (p, rho_sub) per
// level --, 8 doubles per chain (H0, W, W_sub, the sum of min(1, w), the sub-tree candidate's U and misfit, u_top) and 8 ints per chain
// (j, i inside the sub-tree, the leaf count m, the direction, depth, moved, reason).
#include "finrom_internal.h"
#include "block_reduce.h"
#include "hmc_nuts_device.h"

#pragma clang fp contract(off)

namespace finrom {

namespace {

constexpr int NT = 1024;
enum { A_LK, A_LP, A_LDU, A_RK, A_RP, A_RDU, A_WP, A_WPH, A_WDU, A_SK, A_SDU, A_RHO, A_RHS, A_CK };
enum { S_H0, S_W, S_WSUB, S_ACC, S_USUB, S_LSUB, S_UTOP };
enum { I_J, I_I, I_M, I_FWD, I_DEPTH, I_MOVED, I_REASON };
static_assert(A_CK == NUTS_TREE_FIXED_ARRAYS, "the workspace holds the kernels' arrays");

// theta_out[c][q] = theta0[q] + sum_i A[q][i] k'[c][i] (finrom_hmc_drift's contract in the 1024-thread order): a thread's chains
struct ThetaSums {
  double s[HMC_MODEL_MAXP];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < HMC_MODEL_MAXP; ++q) s[q] = 0.0;
  }
  __device__ __forceinline__ void add(const NutsMap& tm, int n, int e, double kq) {
#pragma unroll
    for (int q = 0; q < HMC_MODEL_MAXP; ++q)
      if (q < tm.P) s[q] = fma(tm.A[(int64_t)q * n + e], kq, s[q]);
  }
  // (uniform over the workgroup; redt: [HMC_MODEL_MAXP][16] doubles of LDS that nothing else uses)
  __device__ __forceinline__ void store(const NutsMap& tm, int64_t c, double (*redt)[16]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < HMC_MODEL_MAXP; ++q) {
      if (q < tm.P) {
        double v = s[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) redt[q][wave] = v;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < tm.P) {
      const int q = threadIdx.x;
      tm.theta_out[c * tm.P + q] = (tm.theta0 != nullptr ? tm.theta0[q] : 0.0) + wave_sums_16(redt[q]);
    }
  }
};

struct Chain {                                                        // chain c's arrays
  double *Lk, *Lp, *LdU, *Rk, *Rp, *RdU, *wp, *wph, *wdU, *sk, *sdU, *rho, *rhs, *ck;
  int64_t plane;
  __device__ __forceinline__ Chain(const NutsTreeDev& a, int64_t C, int n, int64_t c) {
    plane = C * n;
    double* w = a.ws + c * n;
    Lk = w + A_LK * plane; Lp = w + A_LP * plane; LdU = w + A_LDU * plane; Rk = w + A_RK * plane; Rp = w + A_RP * plane;
    RdU = w + A_RDU * plane; wp = w + A_WP * plane; wph = w + A_WPH * plane; wdU = w + A_WDU * plane; sk = w + A_SK * plane;
    sdU = w + A_SDU * plane; rho = w + A_RHO * plane; rhs = w + A_RHS * plane; ck = w + A_CK * plane;
  }
};

// sub-tree j's draw (thread 0): u_top, W_sub = 0 -> the direction bit
__device__ __forceinline__ int draw_subtree(double* sc, unsigned g0, unsigned g1, int j, unsigned k0, unsigned k1) {
  unsigned ow[4];
  nuts_philox(g0, g1, (unsigned)j, 3u, k0, k1, ow);
  sc[S_UTOP] = nuts_uniform(ow);
  sc[S_WSUB] = 0.0;
  return (int)(ow[2] & 1u);
}

// the walker starts at the edge of its direction with its first half kick made; the first drift goes to kq
__device__ __forceinline__ void start_walker(const Chain& ch, bool fwd, double hh, double eps, int n, double* kq, const NutsMap& tm,
                                             ThetaSums& ts) {
  const double dsgn = fwd ? 1.0 : -1.0, dh = -dsgn * hh, deps = dsgn * eps;
  const double* Ek = fwd ? ch.Rk : ch.Lk;
  const double* Ep = fwd ? ch.Rp : ch.Lp;
  const double* EdU = fwd ? ch.RdU : ch.LdU;
  for (int e = threadIdx.x; e < n; e += NT) {
    const double du = EdU[e], ph = fma(dh, du, Ep[e]), kn = fma(deps, ph, Ek[e]);
    ch.wph[e] = ph; ch.wdU[e] = du; ch.rhs[e] = 0.0; kq[e] = kn;
    if (tm.A != nullptr) ts.add(tm, n, e, kn);
  }
}

__global__ __launch_bounds__(NT) void hmc_nuts_begin_kernel(HmcDev h, NutsTreeDev a, NutsMap tm) {
  __shared__ double red[16];
  __shared__ double redt[HMC_MODEL_MAXP][16];
  __shared__ int bc[1];
  const int64_t c = blockIdx.x, C = h.C;
  const int tid = threadIdx.x, n = h.n;
  const int64_t o = c * n;
  const Chain ch(a, C, n, c);
  const double* __restrict__ p0 = h.P_block + (*h.jt * C + c) * n;
  double s0 = 0.0;
  for (int e = tid; e < n; e += NT) {                                 // the start: both edges the state, rho = p0
    const double p = p0[e], kv = h.K[o + e], du = h.dU[o + e];
    s0 = fma(p, p, s0);
    ch.Lk[e] = kv; ch.Rk[e] = kv; ch.Lp[e] = p; ch.Rp[e] = p; ch.LdU[e] = du; ch.RdU[e] = du; ch.rho[e] = p;
  }
  const double pp0 = block_sum_1024(s0, red);
  if (tid == 0) {
    double* sc = a.scal + c * NUTS_TREE_SCALARS;
    int* it = a.ints + c * NUTS_TREE_INTS;
    const unsigned long long seed = a.seeds[c], gp = (unsigned long long)(a.proposal0 + *h.pt);
    sc[S_H0] = h.U[c] + 0.5 * pp0; sc[S_W] = 1.0; sc[S_ACC] = 0.0;
    const int fwd = draw_subtree(sc, (unsigned)gp, (unsigned)(gp >> 32), 0, (unsigned)seed, (unsigned)(seed >> 32));
    it[I_J] = 0; it[I_I] = 0; it[I_M] = 0; it[I_FWD] = fwd; it[I_DEPTH] = 0; it[I_MOVED] = 0; it[I_REASON] = 0;
    a.active[c] = 1;
    bc[0] = fwd;
  }
  __syncthreads();
  ThetaSums ts;
  ts.clear();
  const double eps = a.eps_c != nullptr ? a.eps_c[c] : h.eps;          // (uniform over the workgroup)
  start_walker(ch, bc[0] != 0, 0.5 * eps * h.c_pri, eps, n, h.Kq0 + o, tm, ts);
  if (tm.A != nullptr) ts.store(tm, c, redt);
}

__global__ __launch_bounds__(NT) void hmc_nuts_leaf_kernel(HmcDev h, NutsTreeDev a, const double* __restrict__ grad,
                                                           const double* __restrict__ g_theta, NutsMap tm) {
  __shared__ double red[32];
  __shared__ double redt[HMC_MODEL_MAXP][16];
  __shared__ int bc[4];                                               // (leaf's stop, selected), adopted, the next direction
  const int64_t c = blockIdx.x, C = h.C;
  const int act = a.active[c];
  if (act == 0) return;                                               // (uniform; an ended chain is left as it is)
  const int tid = threadIdx.x, n = h.n;
  const int64_t o = c * n;
  if (act == 2) {
    // the START POINT's evaluation, a round like any other: Kq[0] holds the state's position and the model has been there.  The
    // state's dU, U and misfit in a leaf's arithmetic, so that a chain continued from a draw starts from the bits the draw had.
    const bool bad = h.info[c] != 0;
    double sd = 0.0;
    for (int e = tid; e < n; e += NT) {
      double g;
      if (grad != nullptr) {
        g = grad[o + e];
      } else {
        g = 0.0;
        for (int q = 0; q < tm.P; ++q) g = fma(g_theta[c * tm.P + q], tm.A[(int64_t)q * n + e], g);
      }
      const double dk = h.Kq0[o + e] - h.mean[o + e];
      h.dU[o + e] = bad ? 0.0 : fma(h.c_lik / h.c_pri, g, dk);
      sd = fma(dk, dk, sd);
    }
    sd = block_sum_1024(sd, red);
    if (tid == 0) {
      const double ls = h.loss[c], U0 = fma(h.c_lik, ls, 0.5 * h.c_pri * sd);
      h.U[c] = (bad || !__builtin_isfinite(U0)) ? __builtin_inf() : U0;
      a.st_loss[c] = ls;
      a.active[c] = 0;
    }
    return;
  }
  const Chain ch(a, C, n, c);
  double* const sc = a.scal + c * NUTS_TREE_SCALARS;
  int* const it = a.ints + c * NUTS_TREE_INTS;
  const int j = it[I_J], i = it[I_I], m = it[I_M] + 1;
  const bool fwd = it[I_FWD] != 0;
  const bool flagged = h.info[c] != 0;
  const unsigned long long seed = a.seeds[c], gp = (unsigned long long)(a.proposal0 + *h.pt);
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), g0 = (unsigned)gp, g1 = (unsigned)(gp >> 32);
  const double eps = a.eps_c != nullptr ? a.eps_c[c] : h.eps;          // (uniform over the workgroup)
  const double hh = 0.5 * eps * h.c_pri, coef = h.c_lik / h.c_pri;
  const double dsgn = fwd ? 1.0 : -1.0, dh = -dsgn * hh, deps = dsgn * eps;
  double* const kn = h.Kq0 + o;                                       // the leaf's position k'
  const double* __restrict__ mean = h.mean + o;
  const int i_max = __popc((unsigned)i >> 1);
  double* const ckp = ch.ck + (int64_t)(2 * i_max) * ch.plane;
  double* const ckr = ckp + ch.plane;

  // the second half kick; and while p' is at hand what does not wait for the decision (a leaf that diverges discards all of it):
  // rho_sub, an even leaf's checkpoint
  double sp = 0.0, sd = 0.0;
  if (!flagged) {
    for (int e = tid; e < n; e += NT) {
      double g;
      if (grad != nullptr) {
        g = grad[o + e];
      } else {
        g = 0.0;
        for (int q = 0; q < tm.P; ++q) g = fma(g_theta[c * tm.P + q], tm.A[(int64_t)q * n + e], g);
      }
      const double dk = kn[e] - mean[e];
      const double du = fma(coef, g, dk);
      const double pe = fma(dh, du, ch.wph[e]);
      const double r = ch.rhs[e] + pe;
      ch.wdU[e] = du; ch.wp[e] = pe; ch.rhs[e] = r;
      if (!(i & 1)) { ckp[e] = pe; ckr[e] = r; }
      sp = fma(pe, pe, sp);
      sd = fma(dk, dk, sd);
    }
  }
  block_sum2_1024(sp, sd, red);
  if (tid == 0) {                                                     // the leaf's energy, divergence, the streamed selection
    const double ls = h.loss[c];
    const double Un = fma(h.c_lik, ls, 0.5 * h.c_pri * sd);
    const double dE = (Un + 0.5 * sp) - sc[S_H0];
    int st = 0, sel = 0;
    if (flagged || !__builtin_isfinite(dE) || dE > 1000.0) {
      st = 3;
    } else {
      const double wt = exp(-dE);
      const double W_sub = sc[S_WSUB] + wt;
      sc[S_WSUB] = W_sub;
      sc[S_ACC] += wt < 1.0 ? wt : 1.0;
      unsigned ow[4];
      nuts_philox(g0, g1, (unsigned)m, 4u, k0, k1, ow);
      sel = nuts_uniform(ow) * W_sub < wt ? 1 : 0;
      if (sel) { sc[S_USUB] = Un; sc[S_LSUB] = ls; }
    }
    bc[0] = st; bc[1] = sel;
  }
  __syncthreads();
  int reason = bc[0];
  bool ended = reason != 0;
  int j_next = j, i_next = i + 1, fwd_next = fwd ? 1 : 0;
  ThetaSums ts;
  ts.clear();
  if (!ended) {
    if (bc[1] != 0) {
      for (int e = tid; e < n; e += NT) { ch.sk[e] = kn[e]; ch.sdU[e] = ch.wdU[e]; }
    }
    if (i & 1) {                                                      // U-turns over the sub-trees that end at this leaf, smallest first
      const int i_min = i_max - (__ffs(~i) - 1) + 1;
      for (int q = i_max; q >= i_min; --q) {
        const double* cp = ch.ck + (int64_t)(2 * q) * ch.plane;
        const double* cr = cp + ch.plane;
        double t1 = 0.0, t2 = 0.0;
        for (int e = tid; e < n; e += NT) {
          const double cpe = cp[e], rs = (ch.rhs[e] - cr[e]) + cpe;
          t1 = fma(rs, cpe, t1); t2 = fma(rs, ch.wp[e], t2);
        }
        block_sum2_1024(t1, t2, red);
        if (t1 <= 0.0 || t2 <= 0.0) { reason = 2; ended = true; break; }       // (every thread holds the same two sums)
      }
    }
  }
  if (!ended && i + 1 == (1 << j)) {                                  // the finished sub-tree joins the tree
    if (tid == 0) {
      const double W = sc[S_W], W_sub = sc[S_WSUB];
      const int rep = sc[S_UTOP] * W < W_sub ? 1 : 0;
      if (rep) { h.U[c] = sc[S_USUB]; a.st_loss[c] = sc[S_LSUB]; it[I_MOVED] = 1; }
      sc[S_W] = W + W_sub;
      it[I_DEPTH] = j + 1;
      bc[2] = rep;
    }
    __syncthreads();
    const bool rep = bc[2] != 0;
    double* const Ek = fwd ? ch.Rk : ch.Lk;
    double* const Ep = fwd ? ch.Rp : ch.Lp;
    double* const EdU = fwd ? ch.RdU : ch.LdU;
    double t1 = 0.0, t2 = 0.0;
    for (int e = tid; e < n; e += NT) {
      const double r = ch.rho[e] + ch.rhs[e];
      ch.rho[e] = r;
      Ek[e] = kn[e]; Ep[e] = ch.wp[e]; EdU[e] = ch.wdU[e];
      if (rep) { h.K[o + e] = ch.sk[e]; h.dU[o + e] = ch.sdU[e]; }
      t1 = fma(r, ch.Lp[e], t1); t2 = fma(r, ch.Rp[e], t2);
    }
    block_sum2_1024(t1, t2, red);
    if (t1 <= 0.0 || t2 <= 0.0) {
      reason = 1; ended = true;
    } else if (j + 1 == a.max_depth) {
      ended = true;                                                   // (reason 0: the depth limit)
    } else {                                                          // the next sub-tree's draw and walker
      j_next = j + 1; i_next = 0;
      if (tid == 0) bc[3] = draw_subtree(sc, g0, g1, j_next, k0, k1);
      __syncthreads();
      fwd_next = bc[3];
      start_walker(ch, fwd_next != 0, hh, eps, n, kn, tm, ts);
    }
  } else if (!ended) {                                                // the next leaf of this sub-tree: its half kick and drift
    for (int e = tid; e < n; e += NT) {
      const double ph = fma(dh, ch.wdU[e], ch.wp[e]), kq = fma(deps, ph, kn[e]);
      ch.wph[e] = ph; kn[e] = kq;
      if (tm.A != nullptr) ts.add(tm, n, e, kq);
    }
  }
  if (ended) {                                                        // Kq[0] is the draw's position: what every later round evaluates
    for (int e = tid; e < n; e += NT) {
      const double kv = h.K[o + e];
      kn[e] = kv;
      if (tm.A != nullptr) ts.add(tm, n, e, kv);
    }
  }
  if (tm.A != nullptr) ts.store(tm, c, redt);
  if (tid == 0) {
    it[I_J] = j_next; it[I_I] = i_next; it[I_M] = m; it[I_FWD] = fwd_next; it[I_REASON] = reason;
    if (ended) a.active[c] = 0;
  }
}

// grid (ceil(n / 256), C): the trace row; block x = 0's thread 0 the chain's records
__global__ __launch_bounds__(256) void hmc_nuts_end_kernel(HmcDev h, NutsTreeDev a) {
  const int64_t c = blockIdx.y, C = h.C, row = *h.pt;
  const int e = (int)(blockIdx.x * 256u + threadIdx.x), n = h.n;
  if (h.trace != nullptr && e < n) h.trace[((row + 1) * C + c) * n + e] = h.K[c * n + e];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int* it = a.ints + c * NUTS_TREE_INTS;
    const double* sc = a.scal + c * NUTS_TREE_SCALARS;
    h.accept[c] += it[I_MOVED];
    if (a.tree != nullptr) {
      int* t = a.tree + (row * C + c) * 4;
      t[0] = it[I_DEPTH]; t[1] = it[I_M]; t[2] = a.active[c] != 0 ? -1 : it[I_REASON]; t[3] = it[I_MOVED];
    }
    if (a.accept_stat != nullptr) a.accept_stat[row * C + c] = sc[S_ACC] / (double)it[I_M];
  }
}

__global__ void hmc_nuts_tree_advance_kernel(long long* jt, long long* pt) { *jt += 1; *pt += 1; }

// The dual-averaging update of every chain's step (nuts.py StepAdapt.update, Hoffman & Gelman 2014, Algorithm 5): one thread per chain,
// behind a transition of either form and its counters' advance.  The transition is row *pt - 1 with global index p = proposal0 + row;
// the step it took goes to step_size first, then, while t = p + 1 <= tune, the recursion in the statement's operations, one rounding
// each (this file contracts nothing).  Everything is read from device memory, so a captured launch is replayed as it is.
__global__ __launch_bounds__(256) void hmc_step_adapt_kernel(StepAdaptDev ad) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const long long row = *ad.pt - 1;
  if (c >= ad.C || row < 0) return;
  const double e = ad.eps[c];
  if (ad.step_size != nullptr) ad.step_size[row * ad.C + c] = e;
  const long long ti = ad.proposal0 + row + 1;
  if (ti > ad.tune) return;
  const double t = (double)ti, acc = ad.accept_stat[row * ad.C + c];
  const double w = 1.0 / (t + ad.t0);
  const double hbar = (1.0 - w) * ad.hbar[c] + w * (ad.target - acc);
  const double s = sqrt(t);
  const double x = ad.mu - hbar * s / ad.gamma;
  const double eta = 1.0 / (s * sqrt(s));
  const double xbar = eta * x + (1.0 - eta) * ad.xbar[c];
  ad.hbar[c] = hbar; ad.xbar[c] = xbar;
  ad.eps[c] = exp(ti < ad.tune ? x : xbar);
}

}  // namespace

int64_t hmc_nuts_tree_ws_bytes(int64_t C, int n, int max_depth) {
  return (int64_t)(NUTS_TREE_FIXED_ARRAYS + 2 * max_depth) * C * n * (int64_t)sizeof(double) + C * NUTS_TREE_SCALARS * (int64_t)sizeof(double) +
         C * NUTS_TREE_INTS * (int64_t)sizeof(int);
}

int launch_hmc_nuts_begin(const HmcDev& h, const NutsTreeDev& a, const NutsMap& tm, hipStream_t st) {
  if (h.C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_nuts_begin_kernel, dim3((unsigned)h.C), dim3(NT), 0, st, h, a, tm);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_hmc_nuts_leaf(const HmcDev& h, const NutsTreeDev& a, const double* grad, const double* g_theta, const NutsMap& tm,
                         hipStream_t st) {
  if (h.C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_nuts_leaf_kernel, dim3((unsigned)h.C), dim3(NT), 0, st, h, a, grad, g_theta, tm);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_hmc_step_adapt(const StepAdaptDev& ad, hipStream_t st) {
  if (ad.C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_step_adapt_kernel, dim3((unsigned)((ad.C + 255) / 256)), dim3(256), 0, st, ad);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_hmc_nuts_end(const HmcDev& h, const NutsTreeDev& a, hipStream_t st) {
  if (h.C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_nuts_end_kernel, dim3((unsigned)((h.n + 255) / 256), (unsigned)h.C), dim3(256), 0, st, h, a);
  FR_HIP(hipGetLastError());
  hipLaunchKernelGGL(hmc_nuts_tree_advance_kernel, dim3(1), dim3(1), 0, st, h.jt, h.pt);      // the counters, as launch_hmc_end advances them
  FR_HIP(hipGetLastError());
  return 0;
}

}  // namespace finrom
