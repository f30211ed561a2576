// The No-U-turn transition's random words, shared by its two kernel files (hmc_nuts.hip: one tree per launch under the pure surrogate;
// hmc_nuts_model.hip: one leaf per launch under any model): Philox4x32-10 and the uniform both take from words (o1 o0).
#pragma once
#include <hip/hip_runtime.h>

namespace finrom {

__device__ __forceinline__ void nuts_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {                                      // Philox4x32-10, as util_kernels.hip has it
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
__device__ __forceinline__ double nuts_uniform(const unsigned (&o)[4]) {      // [0, 1)
  return (double)((((unsigned long long)o[1] << 32) | o[0]) >> 11) * 0x1.0p-53;
}

}  // namespace finrom
