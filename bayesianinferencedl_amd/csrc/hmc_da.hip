// Delayed-acceptance HMC, second stage (finrom_hmc_end_stage2, hmc.py correct=): the trajectory ran under a surrogate and passed, or
// failed, the Metropolis test of finrom_hmc_end_stage1; the full-order model was solved once at the end point (QoI only); this
// kernel forms the full-order misfit, tests the candidate with probability min(1, w(k') / w(k)), w = exp(-c_lik (loss_FOM -
// loss_surrogate)) (Christen & Fox 2005), and commits as finrom_hmc_end commits.  One workgroup per chain.
//
// Arithmetic contract (include/finrom.h states it operation by operation; tests/hmc_da_cases.py::ref_stage2 is the NumPy statement):
// no contraction into fused multiply-adds in this file, the one fma of the misfit written out -- the decision, D, loss_f,
// cand_loss_f and the correction row are the bits of the NumPy statement.
#include "finrom_internal.h"

#pragma clang fp contract(off)

namespace finrom {

namespace {

__global__ __launch_bounds__(256) void hmc_end_stage2_kernel(HmcDev h, const double* __restrict__ Kq, finrom_hmc_da a) {
  __shared__ int ok_s;
  const int64_t c = blockIdx.x, j = *h.jt, row = *h.pt + 1;
  const int64_t o = c * h.n;
  if (threadIdx.x == 0) {
    const double* __restrict__ q = a.qoi_f + c * a.n_obs;
    const double* __restrict__ d = a.data + (a.data_per_sample ? c * a.n_obs : 0);
    double s = 0.0;
    for (int i = 0; i < a.n_obs; ++i) {
      const double r = q[i] - d[i];
      s = fma(r, r, s);
    }
    const double lossF = 0.5 * s;
    const double Dq = h.c_lik * (lossF - h.loss[c]);
    const bool good = a.info_f[c] == 0 && fabs(lossF) <= 1.7e308 && fabs(Dq) <= 1.7976931348623157e308;   // (NaN fails both)
    const bool pass1 = a.ok1[c] != 0;
    const int ok = pass1 && good && a.lu2_block[j * h.C + c] < a.D[c] - Dq;
    const double nan = __builtin_nan("");
    a.cand_loss_f[c] = good ? lossF : nan;
    if (a.correction != nullptr) a.correction[row * h.C + c] = good ? Dq : nan;
    a.accept1[c] += pass1 ? 1 : 0;
    h.accept[c] += ok;
    if (ok) { h.U[c] = a.Uq[c]; a.D[c] = Dq; a.loss_f[c] = lossF; }
    ok_s = ok;
  }
  __syncthreads();
  const bool ok = ok_s != 0;
  for (int i = threadIdx.x; i < h.n; i += 256) {                    // finrom_hmc_end's commit
    if (ok) { h.K[o + i] = Kq[o + i]; h.dU[o + i] = h.dUq[o + i]; }
    if (h.trace != nullptr) h.trace[(row * h.C + c) * h.n + i] = ok ? Kq[o + i] : h.K[o + i];
  }
}

__global__ void hmc_da_advance_kernel(long long* jt, long long* pt) { *jt += 1; *pt += 1; }

}  // namespace

int launch_hmc_end_stage2(const HmcDev& h, const double* Kq, const finrom_hmc_da& da, hipStream_t st) {
  if (h.C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_end_stage2_kernel, dim3((unsigned)h.C), dim3(256), 0, st, h, Kq, da);
  FR_HIP(hipGetLastError());
  hipLaunchKernelGGL(hmc_da_advance_kernel, dim3(1), dim3(1), 0, st, h.jt, h.pt);
  FR_HIP(hipGetLastError());
  return 0;
}

}  // namespace finrom
