// The two halves of a leapfrog step that do not depend on the forward model (finrom_hmc_drift / _kick, hmc.py model="fom" | "rom"):
// the position update in front of a value-and-gradient call and the momentum update behind it, as kernels of their own, so that the
// chains of bayesian_inference/hmc.py can run under any model whose gradient the library forms (the reference's sampler instantiates
// the full-order operator, bayesian_inference/pymc_func_bayes_inverse.py:174; the reduced ones are the alternatives beside it,
// :175-176).  finrom_hmc_leapfrog fuses the same two updates into finrom_romml_grad's launches; these are their stand-alone form.
//
// Both take an optional map A [P x n], P <= 16: the drift then also forms theta = theta0 + A k' (the reduced model sees the field
// only through its sub-fin averages; in whitened coordinates A = Sop U^T and theta0 = Sop mean), the kick takes the gradient as
// A^T g_theta.
//
// Arithmetic contract (include/finrom.h states it operation by operation; tests/hmc_model_cases.py is the NumPy statement): no
// contraction beyond what the source writes -- every fused multiply-add is an fma(...) -- and every sum in a fixed order.
#include "finrom_internal.h"
#include "block_reduce.h"

#pragma clang fp contract(off)

namespace finrom {

namespace {

// one workgroup per chain: k' = fma(eps, p, k);  theta[c][q] = theta0[q] + sum_i A[q][i] k'[i], the sum in block_sum_256's order
// (thread t chains i = t, t + 256, ... by fma(A, k', s); butterfly 32 .. 1 in each wave; (w0 + w1) + (w2 + w3))
__global__ __launch_bounds__(256) void hmc_drift_kernel(const double* __restrict__ k, const double* __restrict__ p, double eps,
                                                        double* __restrict__ k_out, int n, const double* __restrict__ A,
                                                        const double* __restrict__ theta0, int P, double* __restrict__ theta_out) {
  __shared__ double red[HMC_MODEL_MAXP][4];
  const int64_t c = blockIdx.x, o = c * n;
  double s[HMC_MODEL_MAXP];
#pragma unroll
  for (int q = 0; q < HMC_MODEL_MAXP; ++q) s[q] = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double kq = fma(eps, p[o + i], k[o + i]);
    k_out[o + i] = kq;
    if (A != nullptr) {
#pragma unroll
      for (int q = 0; q < HMC_MODEL_MAXP; ++q)
        if (q < P) s[q] = fma(A[(int64_t)q * n + i], kq, s[q]);
    }
  }
  if (A == nullptr) return;                                       // (uniform over the workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < HMC_MODEL_MAXP; ++q) {
    if (q < P) {
      double v = s[q];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if (lane == 0) red[q][wave] = v;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < P) {
    const int q = threadIdx.x;
    const double sum = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
    theta_out[c * P + q] = (theta0 != nullptr ? theta0[q] : 0.0) + sum;
  }
}

// one thread per (chain, node): g = grad, or sum_q g_theta[c][q] A[q][i] with q ascending (fma(g_theta, A, g) from 0);
// dUq = fma(coef, g, k' - mean), 0 for a flagged chain;  P = fma(-(eps c_pri), dUq, P), untouched for a flagged chain
__global__ __launch_bounds__(256) void hmc_kick_kernel(const double* __restrict__ kq, const double* __restrict__ mean, double coef,
                                                       double eps_cpri, const int* __restrict__ info, double* __restrict__ mom,
                                                       double* __restrict__ dUq, int n, const double* __restrict__ grad,
                                                       const double* __restrict__ g_theta, const double* __restrict__ A, int P,
                                                       double* __restrict__ grad_out) {
  const int64_t c = blockIdx.y;
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const int64_t o = c * n + i;
  double g;
  if (grad != nullptr) {
    g = grad[o];
  } else {
    g = 0.0;
    for (int q = 0; q < P; ++q) g = fma(g_theta[c * P + q], A[(int64_t)q * n + i], g);
  }
  if (grad_out != nullptr) grad_out[o] = g;
  if (info[c] != 0) { dUq[o] = 0.0; return; }
  const double du = fma(coef, g, kq[o] - mean[o]);
  dUq[o] = du;
  mom[o] = fma(-eps_cpri, du, mom[o]);
}

}  // namespace

int launch_hmc_drift(const HmcDev& h, const double* k, double* k_out, const double* A, const double* theta0, int P, double* theta_out,
                     hipStream_t st) {
  if (h.C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_drift_kernel, dim3((unsigned)h.C), dim3(256), 0, st, k, (const double*)h.P, h.eps, k_out, h.n, A, theta0,
                     A != nullptr ? P : 0, theta_out);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_hmc_kick(const HmcDev& h, const double* kq, const double* grad, const double* g_theta, const double* A, int P,
                    double* grad_out, hipStream_t st) {
  if (h.C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_kick_kernel, dim3((unsigned)((h.n + 255) / 256), (unsigned)h.C), dim3(256), 0, st, kq, h.mean,
                     h.c_lik / h.c_pri, h.eps * h.c_pri, h.info, h.P, h.dUq, h.n, grad, g_theta, A, grad != nullptr ? 0 : P, grad_out);
  FR_HIP(hipGetLastError());
  return 0;
}

}  // namespace finrom
