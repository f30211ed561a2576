// Workgroup reductions in a FIXED order, shared by the per-row bookkeeping kernels (hmc_kernels.hip, lbfgs_kernels.hip): every
// result is the same bits run to run, and a row's result depends on that row alone.
#pragma once
#include <hip/hip_runtime.h>

namespace finrom {

// 256 threads: a butterfly inside each wave (lane i adds lane i ^ off, off = 32 .. 1: every lane ends with the wave's sum), then
// (w0 + w1) + (w2 + w3).  Every thread gets the sum.  red: 4 doubles of LDS; consecutive calls may share it.
__device__ __forceinline__ double block_sum_256(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// two block_sum_256 at once (each value summed in the same order as alone: the same bits), one LDS exchange.  red: 8 doubles.
__device__ __forceinline__ void block_sum2_256(double& a, double& b, double* red) {
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) { red[wave] = a; red[4 + wave] = b; }
  __syncthreads();
  a = (red[0] + red[1]) + (red[2] + red[3]);
  b = (red[4] + red[5]) + (red[6] + red[7]);
}

// block_sum2_256 and, in the same LDS exchange, whether `flag` is set on any thread (a wave vote: no shuffle).  red: 12 doubles.
__device__ __forceinline__ bool block_sum2_any_256(double& a, double& b, bool flag, double* red) {
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
  const double fl = __any(flag) ? 1.0 : 0.0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) { red[wave] = a; red[4 + wave] = b; red[8 + wave] = fl; }
  __syncthreads();
  a = (red[0] + red[1]) + (red[2] + red[3]);
  b = (red[4] + red[5]) + (red[6] + red[7]);
  return (red[8] + red[9]) + (red[10] + red[11]) != 0.0;
}

// the same pattern for a maximum (exact in any order; NaN-free inputs)
__device__ __forceinline__ double block_max_256(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// 1024 threads (the one-workgroup-per-chain kernels of hmc_nuts.hip): the same butterfly inside each of the 16 waves, then the 16 wave
// sums added pairwise in index order, ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)) and so on up the tree.  Every thread gets the
// sum.  red: 16 doubles of LDS per value; consecutive calls may share it.
__device__ __forceinline__ double wave_sums_16(const double* r) {
  return (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) +
         (((r[8] + r[9]) + (r[10] + r[11])) + ((r[12] + r[13]) + (r[14] + r[15])));
}
__device__ __forceinline__ double block_sum_1024(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return wave_sums_16(red);
}

// two block_sum_1024 at once (each value summed in the same order as alone: the same bits), one LDS exchange.  red: 32 doubles.
__device__ __forceinline__ void block_sum2_1024(double& a, double& b, double* red) {
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) { red[wave] = a; red[16 + wave] = b; }
  __syncthreads();
  a = wave_sums_16(red);
  b = wave_sums_16(red + 16);
}

}  // namespace finrom
