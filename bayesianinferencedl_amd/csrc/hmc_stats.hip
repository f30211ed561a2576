// The chains' posterior summaries accumulated on the device (finrom_hmc_stats_update, hmc.py stats=): what the reference's drivers
// compute from a kept trace after the run (bayesian_inference/inference.py:175-214 np.mean / np.std of the trace and the misfit per
// draw) as a streaming update, one launch behind every proposal's Metropolis test.  Per (chain, node): the CURRENT field (the
// candidate where the proposal was accepted), Welford mean and sum of squared deviations of the draws, and Welford moments of the
// means of batches of `batch` consecutive draws; per chain: misfit and accept flag of every proposal.
//
// Arithmetic contract with hmc.py (ChainStats.update): no contraction into fused multiply-adds in this file, IEEE division, the
// counters t and b converted to double exactly, every statement written as ChainStats.update writes it -- the device's sums are the
// bits of the NumPy statement.  One thread per (chain, node); no thread reads what another writes in the same launch: whether the
// proposal was accepted is read from the accept counter against the ping-pong slot the PREVIOUS launch wrote, and the other slot
// is written by the chain's first workgroup alone.
#include "finrom_internal.h"

#pragma clang fp contract(off)

namespace finrom {

namespace {

__global__ __launch_bounds__(256) void hmc_stats_kernel(finrom_hmc_stats s) {
  const int64_t c = blockIdx.y;
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  const int64_t q = *s.pt;                                          // proposals done in this call, this one included
  if (q < 1) return;
  const int64_t a = s.accept[c];
  const bool ok = a != s.acc_prev[((q - 1) & 1) * s.C + c];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    s.acc_prev[(q & 1) * s.C + c] = a;
    const double l = ok ? s.cand_loss[c] : s.cur_loss[c];
    if (ok) s.cur_loss[c] = l;
    if (s.misfit != nullptr) s.misfit[q * s.C + c] = l;
    if (s.accepted != nullptr) s.accepted[q * s.C + c] = ok ? 1 : 0;
  }
  if (i >= s.n) return;
  const int64_t o = c * s.n + i;
  double x;
  if (ok) { x = s.cand[o]; s.cur[o] = x; } else { x = s.cur[o]; }
  const int64_t g = s.proposal0 + q - 1;
  if (g < s.burn) return;
  const int64_t t = g - s.burn + 1;
  double mean = s.mean[o];
  double d = x - mean;
  mean = mean + d / (double)t;
  s.mean[o] = mean;
  s.m2[o] = s.m2[o] + d * (x - mean);
  double bsum = s.bsum[o] + x;
  if (t % s.batch == 0) {
    const int64_t b = t / s.batch;
    const double bm = bsum / (double)s.batch;
    double bm_mean = s.bm_mean[o];
    d = bm - bm_mean;
    bm_mean = bm_mean + d / (double)b;
    s.bm_mean[o] = bm_mean;
    s.bm_m2[o] = s.bm_m2[o] + d * (bm - bm_mean);
    bsum = 0.0;
  }
  s.bsum[o] = bsum;
}

}  // namespace

int launch_hmc_stats(const finrom_hmc_stats& s, hipStream_t st) {
  if (s.C == 0) return 0;
  ScopedKernelTimer t(K_MISC, st);
  hipLaunchKernelGGL(hmc_stats_kernel, dim3((unsigned)((s.n + 255) / 256), (unsigned)s.C), dim3(256), 0, st, s);
  FR_HIP(hipGetLastError());
  return 0;
}

}  // namespace finrom
