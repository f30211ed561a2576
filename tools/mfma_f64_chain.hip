// Does a v_mfma_f64_16x16x4_f64 that accumulates onto the result of the one before it need a software wait?
// A chain of dependent MFMAs on ONE accumulator, issued from inline asm (hipcc pads nothing around it), with DIST independent
// MFMAs on other accumulators between two links (DIST = 0: back to back) and no s_nop anywhere in the chain; two waves per SIMD
// on every CU, so that the pipe is shared as in the projection kernel.  Operands are small integers: every product and sum is
// exact in fp64, and the result must equal the serial sum formed on the host, bit for bit.  A missing interlock would show as a
// link reading its accumulator before the previous link wrote it.
// Build: hipcc -w --offload-arch=gfx950 -O3 tools/mfma_f64_chain.hip -o tools/mfma_f64_chain      exit status 0 = every chain exact
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int LINKS = 16;      // links per pass (operands of a pass live in registers)

__host__ __device__ inline double opa(int lane, int s) { return (double)((lane * 7 + s * 3) % 5 - 2); }      // A[i = lane & 15][k = lane >> 4] of link s
__host__ __device__ inline double opb(int lane, int s) { return (double)((lane * 5 + s * 11) % 7 - 3); }     // B[k = lane >> 4][j = lane & 15]

template <int DIST>
__global__ __launch_bounds__(512) void chain(double* out, int passes) {
  const int lane = threadIdx.x & 63;
  d4 acc = (d4){0, 0, 0, 0}, side[2] = {(d4){0, 0, 0, 0}, (d4){0, 0, 0, 0}};
  double a[LINKS], b[LINKS];
#pragma unroll
  for (int s = 0; s < LINKS; ++s) { a[s] = opa(lane, s); b[s] = opb(lane, s); }
  asm volatile("s_nop 7" ::: "memory");
#pragma unroll 1
  for (int p = 0; p < passes; ++p) {
#pragma unroll
    for (int s = 0; s < LINKS; ++s) {
      asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(acc) : "v"(a[s]), "v"(b[s]));
#pragma unroll
      for (int d = 0; d < DIST; ++d) asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(side[d & 1]) : "v"(a[s]), "v"(b[(s + 1 + d) % LINKS]));
    }
  }
  // the results are read by ordinary code: wait for the pipe first
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" : "+v"(acc), "+v"(side[0]), "+v"(side[1]));
  double* o = out + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  for (int g = 0; g < 4; ++g) o[g] = acc[g];
  if (side[0][0] + side[1][0] == 12345.678) o[0] = 0.0;      // (keeps the side accumulators alive)
}

template <int DIST>
int run(double* d, int blocks, int threads, int passes, const std::vector<double>& want) {
  const size_t n = (size_t)blocks * threads * 4;
  (void)hipMemset(d, 0xff, n * 8);
  hipLaunchKernelGGL(chain<DIST>, dim3(blocks), dim3(threads), 0, 0, d, passes);
  if (hipDeviceSynchronize() != hipSuccess) { printf("DIST=%d: launch failed\n", DIST); return 1; }
  std::vector<double> got(n);
  (void)hipMemcpy(got.data(), d, n * 8, hipMemcpyDeviceToHost);
  size_t bad = 0;
  for (size_t t = 0; t < (size_t)blocks * threads; ++t)
    for (int g = 0; g < 4; ++g) bad += got[t * 4 + g] != want[(t & 63) * 4 + g] * passes;
  printf("DIST=%d  %d waves/SIMD  %d dependent MFMAs per wave: %zu of %zu entries differ from the serial sum\n", DIST, threads / 256,
         LINKS * passes, bad, n);
  return bad != 0;
}

int main() {
  // serial sum of one pass on the host: D[row][col] = sum_s sum_k A_s[row][k] B_s[k][col]; lane (q, c), register g holds D[q + 4 g][c]
  std::vector<double> want(64 * 4, 0.0);
  for (int lane = 0; lane < 64; ++lane)
    for (int g = 0; g < 4; ++g) {
      const int row = (lane >> 4) + 4 * g, col = lane & 15;
      double sum = 0.0;
      for (int s = 0; s < LINKS; ++s)
        for (int k = 0; k < 4; ++k) sum += opa(row + 16 * k, s) * opb(col + 16 * k, s);
      want[lane * 4 + g] = sum;
    }
  const int blocks = 256, threads = 512, passes = 500;
  double* d;
  (void)hipMalloc(&d, (size_t)blocks * threads * 4 * 8);
  int rc = 0;
  rc |= run<0>(d, blocks, threads, passes, want);
  rc |= run<1>(d, blocks, threads, passes, want);
  rc |= run<2>(d, blocks, threads, passes, want);
  rc |= run<0>(d, blocks, 256, passes, want);
  (void)hipFree(d);
  return rc;
}
