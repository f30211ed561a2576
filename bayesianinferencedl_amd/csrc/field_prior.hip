// The latent Gaussian-field prior of the reference's HMC model (bayesian_inference/pymc_func_bayes_inverse.py:191-201:
// pm.gp.Latent(Matern52).prior on the dof coordinates, non-centred: the sampler moves v ~ N(0, I), the field is k = mean + U^T v
// with U the UPPER Cholesky factor of the covariance).  Every leapfrog step sits between two dense triangular products with the
// factor the sampler handle holds:
//   field     k[c, :]   = mean + U^T w[c, :],  w = v + eps p   (optionally w written back: the whitened position update)
//   pullback  g_v[c, :] = U g[c, :]                            (optionally the momentum update behind it, c_pri = 1)
// Both read the same tiles: k[:, I] += U[J, I]^T w[:, J] and g_v[:, J] += U[J, I] g[:, I] for J <= I, so ONE tiling serves both.
//  * Work unit: a 128 x 128 super-tile (2 x 2 sub-tiles of 64) on or above the diagonal, times up to 16 batch rows.  The
//    super-tile is loaded into registers at once (up to 64 doubles per thread, every load in flight together), then each
//    64 x 64 sub-tile passes through LDS; the operand rows (w over the super-tile's row strip, g over its column strip) sit in LDS.
//  * Its partial sums [rows x 128] go to the handle's workspace; the workgroup that arrives last at an output strip (arrival
//    counter) adds the strip's partials in super-tile order and writes the result (+ mean, or the momentum update).
//  * Deterministic: every output is ONE chain of fused multiply-adds in a fixed order -- within a super-tile over its reduction
//    sub-tiles in order, 64 terms each in order; then the super-tiles' partials in order -- set by n alone: neither the batch size,
//    the row chunking nor the workgroup placement enters, and row c's result does not depend on the other rows of the batch.
//  * Placement (speed only): block b works on super-tile b % T8 (T8 = tile count rounded up to 8) and row chunk b / T8, so a
//    super-tile always lands on the XCD of blocks b % 8 in both products and in every call: each XCD's 1/8 of the triangle
//    (1.3 MB at n = 1597) can stay in its 4 MB L2 from one leapfrog step to the next.
#include "finrom_internal.h"

namespace finrom {

namespace {

constexpr int FP_T = 64;            // sub-tile edge
constexpr int FP_B = 128;           // super-tile edge
constexpr int FP_PIECE = 64;        // batch rows per launch: bounds the partial-sum workspace (more rows: more launches)
constexpr int FP_MAX_RC = FP_PIECE / 4;     // row chunks per launch at most (4 rows per chunk at the least)

struct FpArgs {
  const double* U; int n, NB, T, T8;
  int64_t S;                                    // rows of this launch (<= FP_PIECE)
  const double* x;                              // field: v; pullback: g  [S x n]
  const double* p; double eps;                  // field: w = v + eps p (p may be null)
  const double* mean; double* out; double* v_out;   // field: k = mean + U^T w [S x n]; v_out: w (or null).  pullback: out (or null)
  FieldPriorTail tail;                          // pullback: the momentum update (tail.mom null: none)
  double* part; int* tick;
};

__device__ __forceinline__ int tile_index(int NB, int JB, int IB) { return JB * NB - JB * (JB - 1) / 2 + (IB - JB); }

template <bool PULL, int RT>
__global__ __launch_bounds__(256) void field_prior_kernel(FpArgs a) {
  constexpr int R = 4 * RT;                     // batch rows of the workgroup: four row groups of RT rows
  __shared__ double Us[FP_T][FP_T + 1];
  __shared__ double Xs[R][FP_B];
  const int tid = threadIdx.x;
  const int t = (int)(blockIdx.x % (unsigned)a.T8), rc = (int)(blockIdx.x / (unsigned)a.T8);
  if (t >= a.T) return;
  int JB = 0, rest = t;
  while (rest >= a.NB - JB) { rest -= a.NB - JB; ++JB; }
  const int IB = JB + rest;
  const int n = a.n;
  const int c0 = rc * R;
  const int rows = min(R, (int)(a.S - c0));
  const int j0 = JB * FP_B, i0 = IB * FP_B;

  // the whole super-tile into registers (zero outside the matrix and below the diagonal)
  double ur[4][16];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int JJ = k >> 1, II = k & 1;
    const int r0 = j0 + JJ * FP_T, q0 = i0 + II * FP_T;
    const bool live = !(JB == IB && JJ > II) && r0 < n && q0 < n;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = tid + 256 * q, rr = r0 + (e >> 6), cc = q0 + (e & 63);
      ur[k][q] = (live && rr < n && cc < n) ? a.U[(int64_t)rr * n + cc] : 0.0;
    }
  }
  // operand rows: field w over the row strip (the diagonal super-tile writes w back), pullback g over the column strip
  const int x0 = PULL ? i0 : j0;
  for (int e = tid; e < R * FP_B; e += 256) {
    const int c = e / FP_B, q = e % FP_B, col = x0 + q;
    double w = 0.0;
    if (c < rows && col < n) {
      const int64_t o = (int64_t)(c0 + c) * n + col;
      w = a.x[o];
      if (!PULL && a.p != nullptr) w = fma(a.eps, a.p[o], w);
      if (!PULL && a.v_out != nullptr && JB == IB) a.v_out[o] = w;
    }
    Xs[c][q] = w;
  }

  const int o = tid & 63, cg = tid >> 6;
#pragma unroll
  for (int out = 0; out < 2; ++out) {
    double acc[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q) acc[q] = 0.0;
#pragma unroll
    for (int red = 0; red < 2; ++red) {
      const int JJ = PULL ? out : red, II = PULL ? red : out;
      const int k = JJ * 2 + II;
      const bool live = !(JB == IB && JJ > II) && j0 + JJ * FP_T < n && i0 + II * FP_T < n;     // (uniform)
      if (!live) continue;
      __syncthreads();                          // the previous pass is done with Us (first pass: Xs is staged)
#pragma unroll
      for (int q = 0; q < 16; ++q) { const int e = tid + 256 * q; Us[e >> 6][e & 63] = ur[k][q]; }
      __syncthreads();
      const int xo = red * FP_T;
#pragma unroll 8
      for (int e = 0; e < FP_T; ++e) {
        const double u = PULL ? Us[o][e] : Us[e][o];
#pragma unroll
        for (int q = 0; q < RT; ++q) acc[q] = fma(u, Xs[cg + 4 * q][xo + e], acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int c = cg + 4 * q;
      if (c < rows) a.part[((int64_t)t * a.S + c0 + c) * FP_B + out * FP_T + o] = acc[q];
    }
  }

  // hand-off: partials stored and released at agent scope, then one arrival per workgroup; the last one adds them up
  const int strip = PULL ? JB : IB;
  const int nq = PULL ? a.NB - JB : IB + 1;
  int* tk = a.tick + strip * FP_MAX_RC + rc;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int prev = __hip_atomic_fetch_add(tk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    Xs[0][0] = prev == nq - 1 ? 1.0 : 0.0;      // ("I am last" through the LDS array the workgroup has done with)
  }
  __syncthreads();
  if (Xs[0][0] == 0.0) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  // E outputs per thread; the partials come in groups of G super-tiles, E x G = 32 loads in flight per thread (one at a time, the
  // dependent adds made every partial a round trip of its own: ~1.2 us each), added in super-tile order as they arrive
  constexpr int E = R * FP_B / 256, G = 32 / E;
  double s[E];
#pragma unroll
  for (int i = 0; i < E; ++i) s[i] = 0.0;
  for (int k0 = 0; k0 < nq; k0 += G) {
    double pv[G][E];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int kq = k0 + j;
      const int tq = kq < nq ? (PULL ? tile_index(a.NB, JB, JB + kq) : tile_index(a.NB, kq, IB)) : 0;
#pragma unroll
      for (int i = 0; i < E; ++i) {
        const int e = tid + 256 * i, c = e / FP_B, q = e % FP_B;
        pv[j][i] = (kq < nq && c < rows) ? a.part[((int64_t)tq * a.S + c0 + c) * FP_B + q] : 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
      for (int i = 0; i < E; ++i)
        if (k0 + j < nq) s[i] += pv[j][i];
  }
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const int e = tid + 256 * i, c = e / FP_B, q = e % FP_B, col = strip * FP_B + q;
    if (c >= rows || col >= n) continue;
    const int64_t oi = (int64_t)(c0 + c) * n + col;
    const double sv = s[i];
    if (!PULL) {
      a.out[oi] = a.mean != nullptr ? a.mean[col] + sv : sv;
    } else {
      if (a.out != nullptr) a.out[oi] = sv;
      const FieldPriorTail& tl = a.tail;
      if (tl.mom != nullptr) {                  // dU = v' + c_lik g_v (0 for a flagged sample), p -= eps dU
        const double d = tl.info[c0 + c] != 0 ? 0.0 : fma(tl.c_lik, sv, tl.vq[oi]);
        tl.dU[oi] = d;
        tl.mom[oi] = fma(-tl.eps, d, tl.mom[oi]);
      }
    }
  }
  if (tid == 0) *tk = 0;                        // ready for the next launch
}

int n_super(int n) { return (n + FP_B - 1) / FP_B; }

}  // namespace

size_t field_prior_part_bytes(int n, int64_t S) {
  const int NB = n_super(n);
  return (size_t)NB * (NB + 1) / 2 * (size_t)std::min<int64_t>(std::max<int64_t>(S, 1), FP_PIECE) * FP_B * sizeof(double);
}
size_t field_prior_tick_bytes(int n) { return (size_t)n_super(n) * FP_MAX_RC * sizeof(int); }

int launch_field_prior(const double* U, int n, int pull, const double* x, const double* p, double eps, const double* mean,
                       double* out, double* v_out, const FieldPriorTail* tail, int64_t S, double* part, int* tick, hipStream_t st) {
  if (S == 0) return 0;
  ScopedKernelTimer tm(K_MISC, st);
  FpArgs a{};
  a.U = U; a.n = n; a.NB = n_super(n); a.T = a.NB * (a.NB + 1) / 2; a.T8 = (a.T + 7) / 8 * 8;
  a.part = part; a.tick = tick; a.eps = eps;
  for (int64_t s0 = 0; s0 < S; s0 += FP_PIECE) {
    const int64_t Sp = std::min<int64_t>(FP_PIECE, S - s0);
    const int64_t off = s0 * n;
    a.S = Sp;
    a.x = x + off; a.p = p ? p + off : nullptr; a.mean = mean;
    a.out = out ? out + off : nullptr; a.v_out = v_out ? v_out + off : nullptr;
    a.tail = FieldPriorTail{};
    if (tail != nullptr && tail->mom != nullptr) {
      a.tail = *tail;
      a.tail.vq = tail->vq + off; a.tail.mom = tail->mom + off; a.tail.dU = tail->dU + off; a.tail.info = tail->info + s0;
    }
    const int RT = Sp <= 4 ? 1 : Sp <= 8 ? 2 : 4;
    const unsigned grid = (unsigned)(a.T8 * ((Sp + 4 * RT - 1) / (4 * RT)));
#define FP_LAUNCH(P_, RT_) hipLaunchKernelGGL((field_prior_kernel<P_, RT_>), dim3(grid), dim3(256), 0, st, a)
    if (pull) { if (RT == 1) FP_LAUNCH(true, 1); else if (RT == 2) FP_LAUNCH(true, 2); else FP_LAUNCH(true, 4); }
    else { if (RT == 1) FP_LAUNCH(false, 1); else if (RT == 2) FP_LAUNCH(false, 2); else FP_LAUNCH(false, 4); }
#undef FP_LAUNCH
    FR_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace finrom
