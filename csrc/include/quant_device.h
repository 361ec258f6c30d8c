// Q-GADMM stochastic quantizer on the device: the specification of gadmm_amd/algorithms/quantize.py,
// operation for operation. Every floating-point line below is a separately rounded IEEE f64
// operation: the bodies run under `fp contract(off)`, so no multiply-add is fused, and the sender
// and every receiver of a message go through the SAME q_apply, so their copies of a public model
// stay identical bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace quant {

// bits in {4, 8, 16}: log2 of the codes per 64-bit word (16, 8, 4)
__device__ __host__ __forceinline__ int q_log2_per(int bits) { return bits == 4 ? 4 : (bits == 8 ? 3 : 2); }
// 64-bit code words of one d-coordinate message
__device__ __host__ __forceinline__ int q_words(int d, int bits) {
  const int per = 64 / bits;
  return (d + per - 1) / per;
}

// Counter-based uniform in [0, 1): splitmix64 finaliser of a Weyl sequence indexed by
// (iteration, worker, coordinate); integers mod 2^64.
__device__ __forceinline__ double q_u01(unsigned long long seed, int it, int n, int w, int d, int i) {
  const unsigned long long idx =
      (((unsigned long long)it * (unsigned long long)n + (unsigned long long)w) * (unsigned long long)d +
       (unsigned long long)i) + 1ull;
  unsigned long long z = seed + 0x9e3779b97f4a7c15ull * idx;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (double)(z >> 11) * 0x1p-53;  // both exact: a 53-bit integer, a power of two
}

// The code of one coordinate: clamp(floor((diff + R) / delta + u), 0, L), delta = 2 R / L; 0 at R == 0.
__device__ __forceinline__ unsigned q_code(double diff, double R, double L, double u) {
#pragma clang fp contract(off)
  if (R == 0.0) return 0u;
  const double delta = (2.0 * R) / L;
  const double c = (diff + R) / delta;
  double f = floor(c + u);
  f = f < 0.0 ? 0.0 : (f > L ? L : f);
  return f == f ? (unsigned)f : 0u;
}

// The dequantize line, shared by the sender and every receiver: hat + (q delta - R); hat at R == 0.
__device__ __forceinline__ double q_apply(double hat, double R, double L, unsigned q) {
#pragma clang fp contract(off)
  if (R == 0.0) return hat;
  const double delta = (2.0 * R) / L;
  const double step = (double)q * delta;
  return hat + (step - R);
}

}  // namespace quant
