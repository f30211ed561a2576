// Low-rank metric of the Laplace-preconditioned HMC chains (bayesian_inference/laplace.py, hmc.py metric=): the Gauss-Newton
// Hessian of the whitened potential at the MAP point, M = I + V diag(lambda) V^T with rho <= 64 orthonormal columns V_j, as the
// reference hands it to NUTS as `scaling` (bayesian_inference/inference.py:102-140,165).  Every map the chains need is
//   y = x + sum_j c_j V_j (V_j . x)            (M: c = lambda, M^-1: -lambda / (1 + lambda), M^(+-1/2): (1 + lambda)^(+-1/2) - 1)
// One 256-thread workgroup per row.  The eigenvectors are stored as Vt [rho x n] row-major, so lanes read consecutive doubles.
// Pass 1: wave w forms the dot products of eigenvectors w, w + 4, ... ALONE (lane l sums elements l, l + 64, ... in order, then a
// butterfly inside the wave), so the rho sums meet in LDS behind ONE barrier and need no sum across waves.  Pass 2: the update,
// j = 0 .. rho - 1 in order.  All sums run in a fixed order that depends on n and rho alone: the same bits run to run, and a row's
// bits do not depend on the batch it is in.
#include "finrom_internal.h"
#include "block_reduce.h"

namespace finrom {

namespace {

// dots[j] = (scale ? scale[j] : 1) * sum_i Vt[j][i] x(i), j < rho, visible to every thread on return.  dots: METRIC_MAX_RHO doubles
// of LDS.  Four eigenvectors per sweep of the row (independent loads in flight: the pass is latency-bound, Vt sits in L2).
template <class X>
__device__ __forceinline__ void metric_dots(const double* __restrict__ Vt, int n, int rho, const double* __restrict__ scale, X x,
                                            double* dots) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j0 = wave; j0 < rho; j0 += 16) {
    const int j1 = j0 + 4, j2 = j0 + 8, j3 = j0 + 12;
    // (an index past the end re-reads the last eigenvector; its sum is dropped)
    const double* __restrict__ v0 = Vt + (size_t)j0 * n;
    const double* __restrict__ v1 = Vt + (size_t)min(j1, rho - 1) * n;
    const double* __restrict__ v2 = Vt + (size_t)min(j2, rho - 1) * n;
    const double* __restrict__ v3 = Vt + (size_t)min(j3, rho - 1) * n;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int i = lane; i < n; i += 64) {
      const double xi = x(i);
      a0 = fma(v0[i], xi, a0); a1 = fma(v1[i], xi, a1); a2 = fma(v2[i], xi, a2); a3 = fma(v3[i], xi, a3);
    }
    for (int off = 32; off > 0; off >>= 1) {
      a0 += __shfl_xor(a0, off); a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); a3 += __shfl_xor(a3, off);
    }
    if (lane == 0) {
      dots[j0] = scale ? scale[j0] * a0 : a0;
      if (j1 < rho) dots[j1] = scale ? scale[j1] * a1 : a1;
      if (j2 < rho) dots[j2] = scale ? scale[j2] * a2 : a2;
      if (j3 < rho) dots[j3] = scale ? scale[j3] * a3 : a3;
    }
  }
  __syncthreads();
}

// x(i) + sum_j w[j] Vt[j][i], j in order (w in LDS: one broadcast read per term)
__device__ __forceinline__ double metric_update(const double* __restrict__ Vt, int n, int rho, const double* w, int i, double xi) {
  double y = xi;
  for (int j = 0; j < rho; ++j) y = fma(w[j], Vt[(size_t)j * n + i], y);
  return y;
}

// y = x + sum_j c_j V_j (V_j . x) for S rows; quad[s] = x . y (optional)
__device__ __forceinline__ void metric_apply_row(const double* __restrict__ Vt, const double* __restrict__ coef, int n, int rho,
                                                 const double* __restrict__ x, double* __restrict__ y, double* __restrict__ quad,
                                                 double* w, double* red) {
  metric_dots(Vt, n, rho, coef, [&](int i) { return x[i]; }, w);
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double xi = x[i];
    const double yi = metric_update(Vt, n, rho, w, i, xi);
    y[i] = yi;
    s = fma(xi, yi, s);
  }
  if (quad != nullptr) {
    const double q = block_sum_256(s, red);
    if (threadIdx.x == 0) *quad = q;
  }
}

__global__ __launch_bounds__(256) void metric_apply_kernel(const double* __restrict__ Vt, const double* __restrict__ coef, int n, int rho,
                                                           const double* __restrict__ x, double* __restrict__ y,
                                                           double* __restrict__ quad) {
  __shared__ double w[METRIC_MAX_RHO];
  __shared__ double red[4];
  const size_t o = (size_t)blockIdx.x * n;
  metric_apply_row(Vt, coef, n, rho, x + o, y + o, quad ? quad + blockIdx.x : nullptr, w, red);
}

// the velocity of a leapfrog step, Q = M^-1 P, chain by chain (the position update in front of finrom_hmc_leapfrog_field_metric)
__global__ __launch_bounds__(256) void hmc_velocity_kernel(const double* __restrict__ Vt, const double* __restrict__ c_inv, int n, int rho,
                                                           const double* __restrict__ P, double* __restrict__ Q) {
  __shared__ double w[METRIC_MAX_RHO];
  __shared__ double red[4];
  const size_t o = (size_t)blockIdx.x * n;
  metric_apply_row(Vt, c_inv, n, rho, P + o, Q + o, nullptr, w, red);
}

// hmc_begin_kernel under the metric: P_block holds the standard normals xi (the host chain's draws);  p = M^(1/2) xi,
// H0 = U + |xi|^2 / 2 (= U + p^T M^-1 p / 2), then the first half step of p
__global__ __launch_bounds__(256) void hmc_begin_metric_kernel(HmcDev h, const double* __restrict__ Vt, const double* __restrict__ c_sqrt,
                                                               int rho) {
  __shared__ double w[METRIC_MAX_RHO];
  __shared__ double red[4];
  const int64_t c = blockIdx.x, j = *h.jt;
  const double* __restrict__ xi = h.P_block + (j * h.C + c) * h.n;
  const int64_t o = c * h.n;
  metric_dots(Vt, h.n, rho, c_sqrt, [&](int i) { return xi[i]; }, w);
  double s = 0.0;
  for (int i = threadIdx.x; i < h.n; i += 256) {
    const double x = xi[i];
    s = fma(x, x, s);
    const double p = metric_update(Vt, h.n, rho, w, i, x);
    h.Kq0[o + i] = h.K[o + i];
    const double du = h.dU[o + i];
    h.dUq[o + i] = du;
    h.P[o + i] = fma(-0.5 * h.eps * h.c_pri, du, p);
  }
  const double xx = block_sum_256(s, red);
  if (threadIdx.x == 0) h.H0[c] = h.U[c] + 0.5 * xx;
}

// hmc_end_kernel under the metric: kinetic energy p^T M^-1 p / 2 = (|p|^2 - sum_j d_j (V_j . p)^2) / 2, d_j = lambda_j / (1 + lambda_j)
__global__ __launch_bounds__(256) void hmc_end_metric_kernel(HmcDev h, const double* __restrict__ Kq, const double* __restrict__ Vt,
                                                             const double* __restrict__ d, int rho) {
  __shared__ double w[METRIC_MAX_RHO];
  __shared__ double red[4];
  __shared__ int ok_s;
  const int64_t c = blockIdx.x, j = *h.jt, row = *h.pt + 1;
  const int64_t o = c * h.n;
  const double half = 0.5 * h.eps * h.c_pri;
  metric_dots(Vt, h.n, rho, nullptr, [&](int i) { return fma(half, h.dUq[o + i], h.P[o + i]); }, w);
  double sp = 0.0, sd = 0.0;
  for (int i = threadIdx.x; i < h.n; i += 256) {
    const double p = fma(half, h.dUq[o + i], h.P[o + i]);
    const double dk = Kq[o + i] - h.mean[o + i];
    sp = fma(p, p, sp); sd = fma(dk, dk, sd);
  }
  const double pp = block_sum_256(sp, red), dd = block_sum_256(sd, red);
  if (threadIdx.x == 0) {
    double low = 0.0;
    for (int q = 0; q < rho; ++q) low = fma(d[q] * w[q], w[q], low);
    double Uq = fma(h.c_lik, h.loss[c], 0.5 * h.c_pri * dd);
    if (h.info[c] != 0 || !(Uq == Uq) || Uq > 1.7e308 || Uq < -1.7e308) Uq = __builtin_inf();
    const double H1 = Uq + 0.5 * (pp - low);
    const int ok = h.lu_block[j * h.C + c] < h.H0[c] - H1;      // (H1 = inf or nan compares false: rejected)
    if (ok) h.U[c] = Uq;
    h.accept[c] += ok;
    ok_s = ok;
  }
  __syncthreads();
  const bool ok = ok_s != 0;
  for (int i = threadIdx.x; i < h.n; i += 256) {
    if (ok) { h.K[o + i] = Kq[o + i]; h.dU[o + i] = h.dUq[o + i]; }
    if (h.trace != nullptr) h.trace[(row * h.C + c) * h.n + i] = ok ? Kq[o + i] : h.K[o + i];
  }
}

__global__ void hmc_metric_advance_kernel(long long* jt, long long* pt) { *jt += 1; *pt += 1; }

}  // namespace

int launch_metric_apply(const MetricDev& m, int op, const double* x, int64_t S, double* y, double* quad, hipStream_t st) {
  ScopedKernelTimer t(K_MISC, st);
  for (int64_t s0 = 0; s0 < S; s0 += 0x7fffffff) {             // (one workgroup per row: the grid's x extent)
    const int64_t Sc = std::min<int64_t>(S - s0, 0x7fffffff);
    hipLaunchKernelGGL(metric_apply_kernel, dim3((unsigned)Sc), dim3(256), 0, st, m.Vt, m.coef + (size_t)op * METRIC_MAX_RHO, m.n, m.rho,
                       x + s0 * m.n, y + s0 * m.n, quad ? quad + s0 : nullptr);
    FR_HIP(hipGetLastError());
  }
  return 0;
}

int launch_hmc_velocity(const MetricDev& m, const double* P, int64_t C, double* Q, hipStream_t st) {
  if (C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_velocity_kernel, dim3((unsigned)C), dim3(256), 0, st, m.Vt, m.coef + (size_t)METRIC_OP_INV * METRIC_MAX_RHO, m.n,
                     m.rho, P, Q);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_hmc_begin_metric(const HmcDev& h, const MetricDev& m, hipStream_t st) {
  if (h.C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_begin_metric_kernel, dim3((unsigned)h.C), dim3(256), 0, st, h, m.Vt,
                     m.coef + (size_t)METRIC_OP_SQRT * METRIC_MAX_RHO, m.rho);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_hmc_end_metric(const HmcDev& h, const MetricDev& m, const double* Kq, hipStream_t st) {
  if (h.C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_end_metric_kernel, dim3((unsigned)h.C), dim3(256), 0, st, h, Kq, m.Vt, m.coef + (size_t)METRIC_OP_D * METRIC_MAX_RHO,
                     m.rho);
  FR_HIP(hipGetLastError());
  hipLaunchKernelGGL(hmc_metric_advance_kernel, dim3(1), dim3(1), 0, st, h.jt, h.pt);
  FR_HIP(hipGetLastError());
  return 0;
}

}  // namespace finrom
