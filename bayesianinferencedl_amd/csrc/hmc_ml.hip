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
#include "mlp_device.h"
#include "mlp_surrogate.h"

// (behind the headers: their device functions keep the contraction they have in mlp_surrogate.hip)
#pragma clang fp contract(off)

namespace finrom {

namespace {

constexpr int HMC_ML_THREADS = 1024;
constexpr int HMC_ML_SCRATCH = MLP_MAX_W * 8 + 2 * MLP_MAX_W * 4 + 16;      // rr [64] doubles, g, up [64] floats, the flag

struct MlScratch {
  double* rr; float* g; float* up; int* flag;
  __device__ explicit MlScratch(float* dyn) : rr((double*)dyn), g(dyn + 2 * MLP_MAX_W), up(dyn + 3 * MLP_MAX_W), flag((int*)(dyn + 4 * MLP_MAX_W)) {}
};

// k' = fma(eps, P, k) -> k_out and the network at it (tape, out), then by wave 0: loss[c] = 1/2 |data - out|^2 as sur_forward_kernel
// sums it, info[c] = 1 where that is not finite (Surrogate._pack's rule), else 0; the flag also into LDS.  The waves behind the
// first come back as soon as the first layer is summed.
__device__ __forceinline__ void ml_forward_loss(const MlpDev& m, const double* k, const double* mom, double eps, double* k_out, int64_t c,
                                                const double* __restrict__ data, int64_t data_stride, float* tape, double* out,
                                                double* loss, int* info, float* dyn, int tid) {
  mlp_forward_body<HMC_ML_THREADS>(m, k, c, nullptr, 0, tape, out, nullptr, nullptr, 0, nullptr, dyn, tid, mom, eps, k_out);
  if (tid >= 64) return;
  const MlScratch s(dyn);
  if (tid < m.n_out) {
    const double r = data[(data_stride ? c * data_stride : 0) + tid] - out[c * m.n_out + tid];
    s.rr[tid] = r * r;
  }
  wave_sync();
  if (tid == 0) {
    double t = 0.0;
    for (int o = 0; o < m.n_out; ++o) t += s.rr[o];
    const double l = 0.5 * t;
    const int bad = __builtin_isfinite(l) ? 0 : 1;
    loss[c] = l;
    info[c] = bad;
    *s.flag = bad;
  }
}

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
  const int tid = threadIdx.x, nw = m.n_w, n = m.n_in;
  for (int step = 0; step < n_steps; ++step) {          // (uniform over the workgroup, and so is every barrier below)
    const double* k = step & 1 ? kq1 : kq0;
    double* kn = step & 1 ? kq0 : kq1;
    ml_forward_loss(m, k, mom, eps, kn, c, data, data_stride, tape, out, loss, info, dyn, tid);
    if (tid < 64) mlp_backward_hidden_wave(m, c, tape, data, data_stride, zero, out, s.g, s.up, tid);
    __syncthreads();
    const bool flagged = *s.flag != 0;
    for (int i = tid; i < n; i += HMC_ML_THREADS) {     // sur_backward_kernel's row, then hmc_kick_kernel's element
      const float* __restrict__ wrow = m.W0 + (int64_t)i * nw;
      float a4[4] = {0.f, 0.f, 0.f, 0.f};
      int j = 0;
      for (; j + 16 <= nw; j += 16) {
        float wv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) wv[u] = wrow[j + u];
#pragma unroll
        for (int u = 0; u < 16; ++u) a4[u & 3] = fmaf(s.g[j + u], wv[u], a4[u & 3]);
      }
      for (; j < nw; ++j) a4[0] = fmaf(s.g[j], wrow[j], a4[0]);
      const float acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
      const double gr = -(double)acc;
      const int64_t o = c * n + i;
      if (flagged) { dUq[o] = 0.0; continue; }
      const double du = fma(coef, gr, kn[o] - mean[o]);
      dUq[o] = du;
      mom[o] = fma(-eps_cpri, du, mom[o]);
    }
    __syncthreads();                                    // g and the flag have been read: the next step's input may overwrite them
  }
}

size_t hmc_ml_dyn_bytes(const MlpDev& m) {
  const size_t in = (size_t)m.n_in * sizeof(float);
  return in > (size_t)HMC_ML_SCRATCH ? in : (size_t)HMC_ML_SCRATCH;
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
