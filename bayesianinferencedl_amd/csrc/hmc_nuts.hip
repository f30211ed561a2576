// The No-U-turn transition of the chains under the pure deep-learning surrogate (finrom_hmc_nuts_ml, hmc.py model="ml" with nuts=):
// ONE kernel (the counters' one-thread advance follows it) is one transition of every chain, one 1024-thread workgroup per chain executing nuts.py's transition_iterative --
// multinomial NUTS with the generalised U-turn criterion, identity mass, the caller's step size.  A tree is hmc_ml_trajectory_kernel's
// loop with a data-dependent trip count and a few fixed-order sums per leaf: the same device functions (hmc_ml_device.h), so a leaf's
// loss and gradient are finrom_mlp_misfit_grad's bits at its position, and the leapfrog step is the four fused multiply-adds of the
// statement, nothing else contracted.
//
// Control flow is uniform over the workgroup: what depends on the data -- the leaf's energy, the divergence test, the streamed
// selection, the adoption -- is decided by thread 0, which draws its own Philox words, and broadcast through LDS behind a barrier; a
// U-turn test compares two block sums that every thread holds in the same bits.  A chain's workgroup waits on no other: workgroup
// barriers only, no flags, spins or atomics, and at most 2^max_depth - 1 leaves whatever the data is.
//
// Who touches what: element i of every per-chain array belongs to thread i % 1024, in mlp_forward_body's drift and here alike, so
// every element is read back by the thread that wrote it and the arrays need no barrier between leaves.  The tree's candidate IS the
// chain's state (K, dU, U, loss): the start is the candidate until a sub-tree's is adopted over it, and a transition that ends
// without an adoption -- a chain flagged at its first leaf -- leaves the state's bits as they are.
//
// LDS is the trajectory kernel's: the block sums' scratch is MlScratch's rr (dead once the loss is summed) and the broadcast words
// lie in its `up` (dead once wave 0 has walked back), both over the dead first-layer input.
//
// The kernel is a template over METRIC.  The `false` instantiation is the identity-mass transition above, from the text it always had
// (finrom_hmc_nuts_ml: every addition is behind `if constexpr`).  The `true` instantiation (finrom_hmc_nuts_ml_metric; nuts.py
// metric=, the reference's `scaling`, bayesian_inference/inference.py:102-140,165-166) runs the transition under M = I + V diag(lambda) V^T:
// p0 = M^(1/2) xi, the drift takes the velocity v(p1/2) = M^-1 p1/2, the energy p' . v' / 2 and the U-turn tests v = M^-1 p at the
// checkpoints and the edges.  Its maps run outside the forward pass, between the leaf's row pass and the leaf's sums.
#include "hmc_ml_device.h"
#include "block_reduce.h"
#include "hmc_nuts_device.h"

namespace finrom {

namespace {

// element e of a per-chain array: the array's address stays a scalar and the element's byte offset one 32-bit register shared by all
// arrays (a 64-bit address per array held across the forward pass does not fit beside it)
__device__ __forceinline__ double& at(double* base, int e) { return *(double*)((char*)base + (unsigned)e * 8u); }
__device__ __forceinline__ const double& at(const double* base, int e) { return *(const double*)((const char*)base + (unsigned)e * 8u); }

// the per-chain arrays of the workspace, [NUTS_ARRAYS][C][n]: the two edges (k, p, dU), the walker (its position ping-pongs as the
// trajectory's does; beside its momentum p the half-kicked p1/2 the next leaf's drift takes), the sub-tree's candidate (k, dU), rho
// and rho_sub, NUTS_MAX_DEPTH checkpoints (p, rho)
enum { A_LK, A_LP, A_LDU, A_RK, A_RP, A_RDU, A_WK0, A_WK1, A_WP, A_WPH, A_WDU, A_SK, A_SDU, A_RHO, A_RHS, A_CK };
// under a metric (finrom_hmc_nuts_ml_metric), behind them: the velocity v = M^-1 p at both edges, the walker's v' and v(p1/2) -- the
// drift's `mom` --, and v per checkpoint
enum { B_LV = NUTS_ARRAYS, B_RV, B_WV, B_WVH, B_CKV, NUTS_METRIC_ARRAYS = B_CKV + NUTS_MAX_DEPTH };

// The metric's part of the transition (hmc_metric.hip's maps for a 1024-thread workgroup).  nuts_metric_dots: dx[j] = scale[j] (V_j . x)
// and with TWO dy[j] = scale[j] (V_j . y) in the same sweep of Vt, j < rho, visible to every thread on return.  Wave w forms the
// products of eigenvectors w, w + 16, w + 32, w + 48 ALONE -- lane l chains fused multiply-adds over elements l, l + 64, ..., then a
// butterfly inside the wave --, so the rho <= 64 sums meet in LDS behind one barrier and need no sum across waves; every sum in its own
// fixed order, with one vector or two.  A wave with no eigenvector (rho < 16) only meets the barriers.  The barrier in front: x and y
// were written element by element by the threads that own them, and the previous dx, dy have been read.
struct NoMetric {};
template <bool METRIC> struct NutsMetricArg { using type = NoMetric; };
template <> struct NutsMetricArg<true> { using type = MetricDev; };

template <bool TWO>
__device__ __forceinline__ void nuts_metric_dots(const MetricDev& mt, const double* __restrict__ scale, const double* x, const double* y,
                                                 double* dx, double* dy) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = mt.n, rho = mt.rho;
  __syncthreads();
  if (wave < rho) {
    const int j1 = wave + 16, j2 = wave + 32, j3 = wave + 48;
    // (an index past the end re-reads the last eigenvector; its sum is dropped)
    const double* __restrict__ v0 = mt.Vt + (size_t)wave * n;
    const double* __restrict__ v1 = mt.Vt + (size_t)min(j1, rho - 1) * n;
    const double* __restrict__ v2 = mt.Vt + (size_t)min(j2, rho - 1) * n;
    const double* __restrict__ v3 = mt.Vt + (size_t)min(j3, rho - 1) * n;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    if (j1 >= rho) {
      // rho <= 16, or a wave with one eigenvector: its sweep alone (no re-read of a clamped row), eight elements' loads in flight.
      // The chain of each sum is the same as below: the same bits
#pragma unroll 8
      for (int i = lane; i < n; i += 64) {
        const double e0 = v0[i], xi = x[i];
        a0 = fma(e0, xi, a0);
        if constexpr (TWO) b0 = fma(e0, y[i], b0);
      }
    } else {
#pragma unroll 2
    for (int i = lane; i < n; i += 64) {
      const double e0 = v0[i], e1 = v1[i], e2 = v2[i], e3 = v3[i], xi = x[i];
      a0 = fma(e0, xi, a0); a1 = fma(e1, xi, a1); a2 = fma(e2, xi, a2); a3 = fma(e3, xi, a3);
      if constexpr (TWO) {
        const double yi = y[i];
        b0 = fma(e0, yi, b0); b1 = fma(e1, yi, b1); b2 = fma(e2, yi, b2); b3 = fma(e3, yi, b3);
      }
    }
    }
    for (int off = 32; off > 0; off >>= 1) {
      a0 += __shfl_xor(a0, off); a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); a3 += __shfl_xor(a3, off);
      if constexpr (TWO) { b0 += __shfl_xor(b0, off); b1 += __shfl_xor(b1, off); b2 += __shfl_xor(b2, off); b3 += __shfl_xor(b3, off); }
    }
    if (lane == 0) {
      dx[wave] = scale[wave] * a0;
      if (j1 < rho) dx[j1] = scale[j1] * a1;
      if (j2 < rho) dx[j2] = scale[j2] * a2;
      if (j3 < rho) dx[j3] = scale[j3] * a3;
      if constexpr (TWO) {
        dy[wave] = scale[wave] * b0;
        if (j1 < rho) dy[j1] = scale[j1] * b1;
        if (j2 < rho) dy[j2] = scale[j2] * b2;
        if (j3 < rho) dy[j3] = scale[j3] * b3;
      }
    }
  }
  __syncthreads();
}
// hmc_metric.hip's metric_update: x(i) + sum_j w[j] Vt[j][i], j in order (w in LDS); two vectors share the read of Vt
__device__ __forceinline__ double nuts_metric_update(const MetricDev& mt, const double* w, int i, double xi) {
  double y = xi;
#pragma unroll 8
  for (int j = 0; j < mt.rho; ++j) y = fma(w[j], mt.Vt[(size_t)j * mt.n + i], y);
  return y;
}
__device__ __forceinline__ void nuts_metric_update2(const MetricDev& mt, const double* wa, const double* wb, int i, double& ya, double& yb) {
#pragma unroll 8
  for (int j = 0; j < mt.rho; ++j) {
    const double e = mt.Vt[(size_t)j * mt.n + i];
    ya = fma(wa[j], e, ya); yb = fma(wb[j], e, yb);
  }
}
// the two sets of METRIC_MAX_RHO sums lie behind the trajectory kernel's dynamic layout, in the metric launch only
__host__ __device__ inline size_t nuts_metric_dots_offset(size_t dyn_bytes) { return (dyn_bytes + 7) & ~(size_t)7; }

template <bool METRIC>
__global__ __launch_bounds__(HMC_ML_THREADS) void hmc_nuts_ml_kernel(MlpDev m, HmcDev h, NutsDev a, const double* __restrict__ data,
                                                                     int64_t data_stride, const double* __restrict__ zero, float* tape,
                                                                     double* out, typename NutsMetricArg<METRIC>::type mt) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const MlScratch s(dyn);
  double* red = s.rr;
  int* bc = (int*)s.up;
  const int64_t c = blockIdx.x, C = h.C;
  const int tid = threadIdx.x, n = m.n_in;
  const int64_t o = c * n, plane = C * n;
  double* const w = a.ws + o;                                         // array q of this chain: w + q * plane
  double* const Lp = w + A_LP * plane;
  double* const Rp = w + A_RP * plane;
  double* const wp = w + A_WP * plane;
  double* const wph = w + A_WPH * plane;
  double* const wdU = w + A_WDU * plane;
  double* const sk = w + A_SK * plane;
  double* const sdU = w + A_SDU * plane;
  double* const rho = w + A_RHO * plane;
  double* const rhs = w + A_RHS * plane;
  const double* __restrict__ mean = h.mean + o;
  const int64_t row = *h.pt;
  const double* __restrict__ p0 = h.P_block + (*h.jt * C + c) * n;
  const unsigned long long seed = a.seeds[c], gp = (unsigned long long)(a.proposal0 + row);
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), g0 = (unsigned)gp, g1 = (unsigned)(gp >> 32);
  const double eps = a.eps_c != nullptr ? a.eps_c[c] : h.eps;          // (uniform over the workgroup: a scalar load)
  const double hh = 0.5 * eps * h.c_pri, coef = h.c_lik / h.c_pri;

  // under a metric: the velocities' arrays, the two sets of sums in LDS, the maps' coefficients
  double *Lv = nullptr, *Rv = nullptr, *wv = nullptr, *wvh = nullptr, *dA = nullptr, *dB = nullptr;
  const double *c_inv = nullptr;
  if constexpr (METRIC) {
    Lv = w + B_LV * plane; Rv = w + B_RV * plane; wv = w + B_WV * plane; wvh = w + B_WVH * plane;
    const size_t in = (size_t)n * sizeof(float);
    dA = (double*)((char*)dyn + nuts_metric_dots_offset(in > (size_t)HMC_ML_SCRATCH ? in : (size_t)HMC_ML_SCRATCH));
    dB = dA + METRIC_MAX_RHO;
    c_inv = mt.coef + (size_t)METRIC_OP_INV * METRIC_MAX_RHO;
  }

  // the start: both edges, rho = p0, H0
  double s0 = 0.0;
  if constexpr (METRIC) {
    // P_block holds the standard normals xi: p0 = M^(1/2) xi, v0 = M^-1 p0, H0 = U + p0 . v0 / 2
    nuts_metric_dots<false>(mt, mt.coef + (size_t)METRIC_OP_SQRT * METRIC_MAX_RHO, p0, nullptr, dA, nullptr);
    for (int e = tid; e < n; e += HMC_ML_THREADS) {
      const double p = nuts_metric_update(mt, dA, e, at(p0, e)), kv = at(h.K + o, e), du = at(h.dU + o, e);
      at(w + A_LK * plane, e) = kv; at(w + A_RK * plane, e) = kv;
      at(Lp, e) = p; at(Rp, e) = p;
      at(w + A_LDU * plane, e) = du; at(w + A_RDU * plane, e) = du;
      at(rho, e) = p;
    }
    nuts_metric_dots<false>(mt, c_inv, Lp, nullptr, dA, nullptr);
    for (int e = tid; e < n; e += HMC_ML_THREADS) {
      const double p = at(Lp, e), v = nuts_metric_update(mt, dA, e, p);
      at(Lv, e) = v; at(Rv, e) = v;
      s0 = fma(p, v, s0);
    }
  } else {
  for (int e = tid; e < n; e += HMC_ML_THREADS) {
    const double p = at(p0, e), kv = at(h.K + o, e), du = at(h.dU + o, e);
    s0 = fma(p, p, s0);
    at(w + A_LK * plane, e) = kv; at(w + A_RK * plane, e) = kv;
    at(Lp, e) = p; at(Rp, e) = p;
    at(w + A_LDU * plane, e) = du; at(w + A_RDU * plane, e) = du;
    at(rho, e) = p;
  }
  }
  const double pp0 = block_sum_1024(s0, red);
  // thread 0's own scalars live in the workspace, not in registers that would have to stay alive through the forward pass (which
  // fills the 128 a 1024-thread workgroup may have): it reads them back where it decides
  double* const sc = a.scal + c * NUTS_SCALARS;
  enum { S_H0, S_W, S_WSUB, S_ACC, S_USUB, S_LSUB, S_UTOP };
  if (tid == 0) { sc[S_H0] = h.U[c] + 0.5 * pp0; sc[S_W] = 1.0; sc[S_ACC] = 0.0; }
  int moved = 0, depth = 0, reason = 0, leaves = 0;

  for (int j = 0; j < a.max_depth; ++j) {                             // (uniform over the workgroup, and so is every barrier below)
    if (tid == 0) {
      unsigned ow[4];
      nuts_philox(g0, g1, (unsigned)j, 3u, k0, k1, ow);
      sc[S_UTOP] = nuts_uniform(ow);
      sc[S_WSUB] = 0.0;
      bc[0] = (int)(ow[2] & 1u);
    }
    __syncthreads();
    const bool fwd = __builtin_amdgcn_readfirstlane(bc[0]) != 0;              // (uniform, and the compiler knows it)
    const double dsgn = fwd ? 1.0 : -1.0, dh = -dsgn * hh, deps = dsgn * eps;
    double* const Ek = w + (fwd ? A_RK : A_LK) * plane;
    double* const Ep = fwd ? Rp : Lp;
    double* const EdU = w + (fwd ? A_RDU : A_LDU) * plane;
    for (int e = tid; e < n; e += HMC_ML_THREADS) {                   // the walker starts at the edge, its first half kick made
      const double du = at(EdU, e);
      at(w + A_WK0 * plane, e) = at(Ek, e); at(wph, e) = fma(dh, du, at(Ep, e)); at(wdU, e) = du; at(rhs, e) = 0.0;
    }
    if constexpr (METRIC) {                                           // the first drift's velocity v(p1/2)
      nuts_metric_dots<false>(mt, c_inv, wph, nullptr, dA, nullptr);
      for (int e = tid; e < n; e += HMC_ML_THREADS) at(wvh, e) = nuts_metric_update(mt, dA, e, at(wph, e));
    }
    int cur = 0, stop = 0;
    __syncthreads();                                                  // the direction has been read: the input may overwrite it
    for (int i = 0; i < (1 << j); ++i) {
      ++leaves;
      const double* kbase = a.ws + (cur ? A_WK1 : A_WK0) * plane;    // [C x n]: mlp_forward_body indexes the chain itself
      double* knbase = a.ws + (cur ? A_WK0 : A_WK1) * plane;
      ml_forward_loss(m, kbase, a.ws + (METRIC ? (int)B_WVH : (int)A_WPH) * plane, deps, knbase, c, data, data_stride, tape, out, a.wloss,
                      a.winfo, dyn, tid);
      if (tid < 64) mlp_backward_hidden_wave(m, c, tape, data, data_stride, zero, out, s.g, s.up, tid);
      __syncthreads();
      const bool flagged = __builtin_amdgcn_readfirstlane(*s.flag) != 0;
      const double* kn = knbase + o;
      const int i_max = __popc((unsigned)i >> 1);
      double* const ckp = w + (A_CK + 2 * i_max) * plane;
      double* const ckr = ckp + plane;
      double sp = 0.0, sd = 0.0;
      if (!flagged) {
        // sur_backward_kernel's row, then the second half kick; and while p' is at hand what does not wait for the decision (a leaf
        // that diverges discards all of it): the next leaf's first half kick, rho_sub, an even leaf's checkpoint
        for (int e = tid; e < n; e += HMC_ML_THREADS) {
          const double gr = ml_grad_row(m, s.g, e);
          const double dk = at(kn, e) - at(mean, e);
          const double du = fma(coef, gr, dk);
          const double pe = fma(dh, du, at(wph, e));
          const double r = at(rhs, e) + pe;
          at(wdU, e) = du; at(wp, e) = pe; at(wph, e) = fma(dh, du, pe); at(rhs, e) = r;
          if (!(i & 1)) { at(ckp, e) = pe; at(ckr, e) = r; }
          if constexpr (!METRIC) sp = fma(pe, pe, sp);
          sd = fma(dk, dk, sd);
        }
      }
      if constexpr (METRIC) {
        // p' and the next leaf's p1/2 are both at hand: their two sets of sums in ONE sweep of Vt, then v' = M^-1 p' (the energy's,
        // the U-turn tests', an even leaf's checkpoint) and v(p1/2), the next drift's.  (`flagged` is uniform: so are the barriers.)
        if (!flagged) {
          nuts_metric_dots<true>(mt, c_inv, wp, wph, dA, dB);
          double* const ckv = w + (B_CKV + i_max) * plane;
          for (int e = tid; e < n; e += HMC_ML_THREADS) {
            const double pe = at(wp, e);
            double vp = pe, vh = at(wph, e);
            nuts_metric_update2(mt, dA, dB, e, vp, vh);
            at(wv, e) = vp; at(wvh, e) = vh;
            if (!(i & 1)) at(ckv, e) = vp;
            sp = fma(pe, vp, sp);
          }
        }
      }
      block_sum2_1024(sp, sd, red);
      if (tid == 0) {                                                 // the leaf's energy, divergence, the streamed selection
        const double ls = a.wloss[c];
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
          nuts_philox(g0, g1, (unsigned)leaves, 4u, k0, k1, ow);
          sel = nuts_uniform(ow) * W_sub < wt ? 1 : 0;
          if (sel) { sc[S_USUB] = Un; sc[S_LSUB] = ls; }
        }
        bc[0] = st; bc[1] = sel;
      }
      __syncthreads();
      stop = __builtin_amdgcn_readfirstlane(bc[0]);
      const bool sel = __builtin_amdgcn_readfirstlane(bc[1]) != 0;
      if (stop) break;                                                // diverged: the sub-tree is discarded, the transition ends
      if (sel) {
        for (int e = tid; e < n; e += HMC_ML_THREADS) { at(sk, e) = at(kn, e); at(sdU, e) = at(wdU, e); }
      }
      cur ^= 1;
      if (i & 1) {                                                    // U-turns over the sub-trees that end at this leaf, smallest first
        const int i_min = i_max - (__ffs(~i) - 1) + 1;
        for (int q = i_max; q >= i_min; --q) {
          const double* cp = w + (A_CK + 2 * q) * plane;
          const double* cr = cp + plane;
          double t1 = 0.0, t2 = 0.0;
          for (int e = tid; e < n; e += HMC_ML_THREADS) {
            const double cpe = at(cp, e), rs = (at(rhs, e) - at(cr, e)) + cpe;
            if constexpr (METRIC) {                                   // the criterion with p# = M^-1 p
              t1 = fma(rs, at(w + (B_CKV + q) * plane, e), t1); t2 = fma(rs, at(wv, e), t2);
            } else {
            t1 = fma(rs, cpe, t1); t2 = fma(rs, at(wp, e), t2);
            }
          }
          block_sum2_1024(t1, t2, red);
          if (__builtin_amdgcn_readfirstlane(t1 <= 0.0 || t2 <= 0.0 ? 1 : 0)) { stop = 2; break; }
        }
      }
      __syncthreads();                                                // the broadcast and the sums have been read: the next input may overwrite them
      if (stop) break;
    }
    if (stop) { reason = stop; break; }
    // the finished sub-tree joins the tree
    if (tid == 0) {
      const double W = sc[S_W], W_sub = sc[S_WSUB];
      const int rep = sc[S_UTOP] * W < W_sub ? 1 : 0;
      if (rep) { h.U[c] = sc[S_USUB]; a.st_loss[c] = sc[S_LSUB]; moved = 1; }
      sc[S_W] = W + W_sub;
      bc[0] = rep;
    }
    depth = j + 1;
    __syncthreads();
    const bool rep = __builtin_amdgcn_readfirstlane(bc[0]) != 0;
    const double* wk = w + (cur ? A_WK1 : A_WK0) * plane;
    double t1 = 0.0, t2 = 0.0;
    for (int e = tid; e < n; e += HMC_ML_THREADS) {
      const double r = at(rho, e) + at(rhs, e);
      at(rho, e) = r;
      at(Ek, e) = at(wk, e); at(Ep, e) = at(wp, e); at(EdU, e) = at(wdU, e);
      if (rep) { at(h.K + o, e) = at(sk, e); at(h.dU + o, e) = at(sdU, e); }
      if constexpr (METRIC) {
        at(fwd ? Rv : Lv, e) = at(wv, e);
        t1 = fma(r, at(Lv, e), t1); t2 = fma(r, at(Rv, e), t2);
      } else {
      t1 = fma(r, at(Lp, e), t1); t2 = fma(r, at(Rp, e), t2);
      }
    }
    block_sum2_1024(t1, t2, red);                                     // (its barriers also stand between this broadcast and the next)
    if (__builtin_amdgcn_readfirstlane(t1 <= 0.0 || t2 <= 0.0 ? 1 : 0)) { reason = 1; break; }
  }

  // commit: the state is the candidate already; the draw's position where finrom_hmc_stats_update reads it, the trace row, the records
  for (int e = tid; e < n; e += HMC_ML_THREADS) {
    const double kv = at(h.K + o, e);
    at(h.Kq0 + o, e) = kv;
    if (h.trace != nullptr) h.trace[((row + 1) * C + c) * n + e] = kv;
  }
  if (tid == 0) {
    h.accept[c] += moved;
    if (a.tree != nullptr) {
      int* t = a.tree + (row * C + c) * 4;
      t[0] = depth; t[1] = leaves; t[2] = reason; t[3] = moved;
    }
    if (a.accept_stat != nullptr) a.accept_stat[row * C + c] = sc[S_ACC] / (double)leaves;
  }
}

__global__ void hmc_nuts_advance_kernel(long long* jt, long long* pt) { *jt += 1; *pt += 1; }

}  // namespace

int64_t hmc_nuts_ws_doubles(int64_t C, int n) { return (int64_t)NUTS_ARRAYS * C * n; }

int launch_hmc_nuts_ml(const MlpDev& m, const HmcDev& h, const NutsDev& a, const double* data, int64_t data_stride, const double* zero,
                       float* tape, double* out, hipStream_t st) {
  static_assert(A_CK + 2 * NUTS_MAX_DEPTH == NUTS_ARRAYS, "the workspace holds the kernel's arrays");
  if (h.C == 0) return 0;
  if (int rc = mlp_forward_fits(m)) return rc;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_nuts_ml_kernel<false>, dim3((unsigned)h.C), dim3(HMC_ML_THREADS), hmc_ml_dyn_bytes(m), st, m, h, a, data, data_stride,
                     zero, tape, out, NoMetric{});
  FR_HIP(hipGetLastError());
  hipLaunchKernelGGL(hmc_nuts_advance_kernel, dim3(1), dim3(1), 0, st, h.jt, h.pt);      // the counters, as launch_hmc_end advances them
  FR_HIP(hipGetLastError());
  return 0;
}

int64_t hmc_nuts_metric_ws_doubles(int64_t C, int n) { return (int64_t)NUTS_METRIC_ARRAYS * C * n; }

// the same launch under a metric: a.ws holds hmc_nuts_metric_ws_doubles, the two sets of sums lie behind the identity launch's LDS
int launch_hmc_nuts_ml_metric(const MlpDev& m, const HmcDev& h, const NutsDev& a, const MetricDev& mt, const double* data,
                              int64_t data_stride, const double* zero, float* tape, double* out, hipStream_t st) {
  if (h.C == 0) return 0;
  if (int rc = mlp_forward_fits(m)) return rc;
  ScopedKernelTimer t(K_MISC, st);
  const size_t dyn = nuts_metric_dots_offset(hmc_ml_dyn_bytes(m)) + 2 * METRIC_MAX_RHO * sizeof(double);
  if (dyn + MLP_FORWARD_STATIC_LDS > 64 * 1024) {                     // (the sums' 1 KB comes out of what the input may take)
    set_error("hmc_nuts_ml_metric: n_in = " + std::to_string(m.n_in) + " leaves no LDS for the metric's sums (at most " +
              std::to_string(MLP_FORWARD_MAX_IN - 2 * METRIC_MAX_RHO * (int)sizeof(double) / 4) + ")");
    return FINROM_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(hmc_nuts_ml_kernel<true>, dim3((unsigned)h.C), dim3(HMC_ML_THREADS), dyn, st, m, h, a, data, data_stride, zero, tape, out,
                     mt);
  FR_HIP(hipGetLastError());
  hipLaunchKernelGGL(hmc_nuts_advance_kernel, dim3(1), dim3(1), 0, st, h.jt, h.pt);
  FR_HIP(hipGetLastError());
  return 0;
}

}  // namespace finrom
