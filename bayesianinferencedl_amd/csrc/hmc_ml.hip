// The chains under the pure deep-learning surrogate (finrom_hmc_leapfrog_ml / finrom_hmc_trajectory_ml, hmc.py model="ml" with
// ml_form=): the one model whose chain needs nothing from any other workgroup -- a sample of mlp_surrogate.hip's per-sample form is
// ONE 1024-thread workgroup, the first layer's transpose is row by row, the drift and the kick are element by element.
//   step form        forward launch (the position update k' = fma(eps, P, k) in front through mlp_forward_body's `mom` path, then the
//                    misfit and the flag info = !isfinite(loss)), sur_backward_kernel (mlp_surrogate.hip), hmc_kick_kernel
//                    (hmc_model.hip): three launches;
//   trajectory form  all n_steps steps in ONE launch, one workgroup per chain.  A chain's workgroup waits on no other: workgroup
//                    barriers only, under control flow that is uniform over the workgroup; no flags, spins or atomics.
// The trajectory leaves the bits the composed steps leave: the same device functions (mlp_forward_body<1024>,
// mlp_backward_hidden_wave), sur_backward_kernel's row chains (four chains of 16, (a0 + a1) + (a2 + a3)) and hmc_kick_kernel's two
// fused multiply-adds, nothing else contracted in the double arithmetic written here.
//
// Who touches what in the trajectory kernel: element i of a chain's k, k', P and dUq belongs to thread i % 1024 in the drift (inside
// mlp_forward_body) and in the kick alike, so the position and the momentum stay in the state's own rows between steps and every
// element is read back by the thread that wrote it.  tape and out are wave 0's, lane by lane.  What crosses threads goes through
// LDS: the input xs (all waves), g0 and the flag (wave 0 -> all), each behind a workgroup barrier.
//
// LDS: the input's n_in floats are dead once the first layer has been summed (mlp_forward_body's second barrier), so wave 0's
// scratch -- the squared residuals, g, up, the flag: HMC_ML_SCRATCH bytes -- lies over them and the kernels' static LDS is
// mlp_forward_body's alone (MLP_FORWARD_STATIC_LDS): n_in <= MLP_FORWARD_MAX_IN is exactly what fits 64 KB.
#include "hmc_ml_device.h"

namespace finrom {

namespace {

__global__ __launch_bounds__(HMC_ML_THREADS) void hmc_ml_forward_kernel(MlpDev m, const double* k, const double* mom, double eps,
                                                                        double* k_out, const double* __restrict__ data,
                                                                        int64_t data_stride, float* tape, double* out, double* loss,
                                                                        int* info) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];      // [max(n_in, HMC_ML_SCRATCH / 4)]
  ml_forward_loss(m, k, mom, eps, k_out, blockIdx.x, data, data_stride, tape, out, loss, info, dyn, threadIdx.x);
}

__global__ __launch_bounds__(HMC_ML_THREADS) void hmc_ml_trajectory_kernel(MlpDev m, int n_steps, double* kq0, double* kq1, double* mom,
                                                                           const double* __restrict__ mean, double* dUq, double eps,
                                                                           double coef, double eps_cpri, const double* __restrict__ data,
                                                                           int64_t data_stride, const double* __restrict__ zero,
                                                                           float* tape, double* out, double* loss, int* info) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const MlScratch s(dyn);
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x, n = m.n_in;
  for (int step = 0; step < n_steps; ++step) {          // (uniform over the workgroup, and so is every barrier below)
    const double* k = step & 1 ? kq1 : kq0;
    double* kn = step & 1 ? kq0 : kq1;
    ml_forward_loss(m, k, mom, eps, kn, c, data, data_stride, tape, out, loss, info, dyn, tid);
    if (tid < 64) mlp_backward_hidden_wave(m, c, tape, data, data_stride, zero, out, s.g, s.up, tid);
    __syncthreads();
    const bool flagged = *s.flag != 0;
    for (int i = tid; i < n; i += HMC_ML_THREADS) {     // sur_backward_kernel's row, then hmc_kick_kernel's element
      const double gr = ml_grad_row(m, s.g, i);
      const int64_t o = c * n + i;
      if (flagged) { dUq[o] = 0.0; continue; }
      const double du = fma(coef, gr, kn[o] - mean[o]);
      dUq[o] = du;
      mom[o] = fma(-eps_cpri, du, mom[o]);
    }
    __syncthreads();                                    // g and the flag have been read: the next step's input may overwrite them
  }
}

}  // namespace

int launch_hmc_ml_forward(const MlpDev& m, const HmcDev& h, const double* k, double* k_out, const double* data, int64_t data_stride,
                          float* tape, double* out, double* loss, int* info, hipStream_t st) {
  if (h.C == 0) return 0;
  if (int rc = mlp_forward_fits(m)) return rc;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_ml_forward_kernel, dim3((unsigned)h.C), dim3(HMC_ML_THREADS), hmc_ml_dyn_bytes(m), st, m, k, (const double*)h.P, h.eps,
                     k_out, data, data_stride, tape, out, loss, info);
  FR_HIP(hipGetLastError());
  return 0;
}

int launch_hmc_ml_trajectory(const MlpDev& m, const HmcDev& h, int n_steps, double* kq0, double* kq1, const double* data,
                             int64_t data_stride, const double* zero, float* tape, double* out, double* loss, int* info, hipStream_t st) {
  if (h.C == 0 || n_steps == 0) return 0;
  if (int rc = mlp_forward_fits(m)) return rc;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_ml_trajectory_kernel, dim3((unsigned)h.C), dim3(HMC_ML_THREADS), hmc_ml_dyn_bytes(m), st, m, n_steps, kq0, kq1, h.P,
                     h.mean, h.dUq, h.eps, h.c_lik / h.c_pri, h.eps * h.c_pri, data, data_stride, zero, tape, out, loss, info);
  FR_HIP(hipGetLastError());
  return 0;
}

}  // namespace finrom
