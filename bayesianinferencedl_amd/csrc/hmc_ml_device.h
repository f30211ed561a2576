// Device pieces shared by the kernels that run a chain under the pure deep-learning surrogate in one 1024-thread workgroup
// (hmc_ml.hip: the forward launch and the whole trajectory; hmc_nuts.hip: the No-U-turn transition): wave 0's scratch over the dead
// first-layer input, the forward pass with the misfit and the flag, a row of the first layer's transpose.  A leapfrog step built from
// these leaves the bits of finrom_hmc_leapfrog_ml's three launches.
#pragma once
#include "mlp_device.h"
#include "mlp_surrogate.h"

// (behind the headers: their device functions keep the contraction they have in mlp_surrogate.hip)
#pragma clang fp contract(off)

namespace finrom {

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

// row i of the first layer's transpose against g0 (LDS), sur_backward_kernel's chains: four chains of 16, (a0 + a1) + (a2 + a3);
// the misfit's gradient with its sign
__device__ __forceinline__ double ml_grad_row(const MlpDev& m, const float* g, int i) {
  const int nw = m.n_w;
  const float* __restrict__ wrow = m.W0 + (int64_t)i * nw;
  float a4[4] = {0.f, 0.f, 0.f, 0.f};
  int j = 0;
  for (; j + 16 <= nw; j += 16) {
    float wv[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) wv[u] = wrow[j + u];
#pragma unroll
    for (int u = 0; u < 16; ++u) a4[u & 3] = fmaf(g[j + u], wv[u], a4[u & 3]);
  }
  for (; j < nw; ++j) a4[0] = fmaf(g[j], wrow[j], a4[0]);
  const float acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
  return -(double)acc;
}

inline size_t hmc_ml_dyn_bytes(const MlpDev& m) {
  const size_t in = (size_t)m.n_in * sizeof(float);
  return in > (size_t)HMC_ML_SCRATCH ? in : (size_t)HMC_ML_SCRATCH;
}

}  // namespace finrom
