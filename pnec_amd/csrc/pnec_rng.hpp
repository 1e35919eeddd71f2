// pnec_rng.hpp -- the counter-based draws of the RANSAC kernels: a hash of (seed, pair, hypothesis, draw) in place of
// opengv's rand(), so that the CPU oracle, the tests' checker and the device draw the same samples and a pair's draws
// do not depend on the batch around it.  Device code only.  pnec_essential_ransac.hip includes it.  pnec_frontend.hip
// still has the same two functions in its own text: including this header there leaves all 18 of its kernels the same
// machine code, but the file's digest is what the committed work counts of the front stages are tied to
// (profiles/chain_work_latest.json), and those are counted on the device.
#pragma once

#include <hip/hip_runtime.h>

namespace pnec_hip {

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// [0, 1); all 64 bits of `seed` enter
__device__ __forceinline__ double rng_uniform(unsigned long long seed, unsigned long long pair,
                                              unsigned long long hyp, unsigned long long draw) {
  const unsigned long long h =
      splitmix64(splitmix64(splitmix64(seed ^ 0xD1B54A32D192ED03ull) + pair) + (hyp << 20) + draw);
  return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

}  // namespace pnec_hip
