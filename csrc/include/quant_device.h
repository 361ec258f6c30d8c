// Q-GADMM stochastic quantizer on the device: the specification of gadmm_amd/algorithms/quantize.py,
// operation for operation. Every floating-point line below is a separately rounded IEEE f64
// operation: the bodies run under `fp contract(off)`, so no multiply-add is fused, and the sender
// and every receiver of a message go through the SAME q_apply, so their copies of a public model
// stay identical bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "gadmm_chain.h"
#include "quad_gemv.h"

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

// ------------------------------------------------------------------------------------------------
// The wire format's device helpers, shared by the chain kernels (chain_quant.hip) and the graph kernel
// (graph_quant.hip): the wave maximum that gives R, the OR that packs a group's codes into its word,
// and the raw tagged granule a message travels in.

// A 64-bit value of another lane of the same 16-lane row through DPP (no LDS round trip, unlike
// __shfl_xor's ds_bpermute): 0xB1 / 0x4E = quad_perm [1,0,3,2] / [2,3,0,1], 0x141 = row_half_mirror,
// 0x140 = row_mirror. Applied in that order to a SYMMETRIC reduction (max, or) every lane of a group of
// 2, 4, 8, 16 lanes ends with the group's result.
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, false);
  return ((unsigned long long)hi << 32) | lo;
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  return __longlong_as_double((long long)dpp_u64<CTRL>((unsigned long long)__double_as_longlong(v)));
}

// max is exact, associative and commutative: any reduction order gives the same bits. Four DPP steps
// inside the rows, then the rows meet through the permlane swaps of quad_gemv.h.
__device__ __forceinline__ double wave_max_f64(double v) {
  v = fmax(v, dpp_f64<0xB1>(v));
  v = fmax(v, dpp_f64<0x4E>(v));
  v = fmax(v, dpp_f64<0x141>(v));
  v = fmax(v, dpp_f64<0x140>(v));
  double a = v, b = v;
  swap16_f64(a, b);  // rows (r0, r1, r2, r3) -> a = (r0, r0, r2, r2), b = (r1, r1, r3, r3)
  v = fmax(a, b);
  a = v;
  b = v;
  swap32_f64(a, b);  // a = (m01 x 4), b = (m23 x 4)
  return fmax(a, b);
}

// OR over each aligned group of 2^lp lanes (lp in {2, 3, 4}), the result in every lane of the group
__device__ __forceinline__ unsigned long long group_or_u64(unsigned long long v, int lp) {
  v |= dpp_u64<0xB1>(v);
  v |= dpp_u64<0x4E>(v);
  if (lp >= 3) v |= dpp_u64<0x141>(v);
  if (lp >= 4) v |= dpp_u64<0x140>(v);
  return v;
}

__device__ __forceinline__ void put_raw(bool local, __amdgpu_buffer_rsrc_t rs, int byte_off, unsigned tag,
                                        unsigned long long bits) {
  u32x4 g = {tag, (unsigned)(bits & 0xffffffffull), tag, (unsigned)(bits >> 32)};
  if (local) __builtin_amdgcn_raw_buffer_store_b128(g, rs, byte_off, 0, 0);
  else __builtin_amdgcn_raw_buffer_store_b128(g, rs, byte_off, 0, 16 /* sc1 */);
}
__device__ __forceinline__ unsigned long long raw_bits(const u32x4& g) {
  return ((unsigned long long)g.w << 32) | g.y;
}

}  // namespace quant
