// Device-side helpers shared by the chain-engine kernels (small fused path and large-d path).
#pragma once
#include "gadmm_common.h"
#include "gadmm_chain.h"
#include "stop_rule.h"

namespace chain_dev {

__device__ __forceinline__ void drain_vmem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ double softplus(double t) {  // log(1 + exp(t)), stable
  return t > 30.0 ? t + log1p(exp(-t)) : log1p(exp(t));
}

// Close the phase: release + ticket; the last arriver acquires and runs `finish`.
__device__ __forceinline__ bool phase_arrive(ChainCtl* ctl, int n_slots, int* flag_lds) {
  drain_vmem();
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    drain_vmem();
    const unsigned t = __hip_atomic_fetch_add(&ctl->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = (t == (unsigned)(n_slots - 1));
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      drain_vmem();
    }
    *flag_lds = last;
  }
  __syncthreads();
  return *flag_lds != 0;
}

__device__ __forceinline__ void finish_iteration(const PhaseArgs& a, int it) {
  if (threadIdx.x != 0) return;
  ChainCtl* ctl = a.ctl;
  if (a.tstamp && it - 1 < a.max_iter) a.tstamp[it - 1] = (long long)__builtin_amdgcn_s_memrealtime();
  if (a.flags & PH_LOCAL_STOP) {
    double s = 0.0;
    for (int i = 0; i < a.n_local; ++i) s += a.objw[i];  // fixed order (local order == worker order)
    if (it - 1 < a.max_iter) a.trace[it - 1] = s;
    const int code = stop_code(s, a.obj0, a.tol, it, a.max_iter);
    if (code) {
      ctl->done = code;
      ctl->conv_iter = it;
    }
    ctl->monitored = it;
  } else {
    double* row = a.part + (long)((it - 1) % a.ring) * a.n_total;
    for (int i = 0; i < a.n_local; ++i) row[a.lgid[i]] = a.objw[i];
  }
  ctl->pending = 1;
  ctl->ticket = 0u;
  ctl->iter = it + 1;
}

// out[i] = sum_j M[j*d + i] * x[j]  (M symmetric), for i < d. x, out in LDS; red: NW*64*NC.
// NT: the block size; its NT / 64 waves split the summation index: wave k sums j = k mod NW ascending, the partials
// are added in wave order -- the one summation order of every engine (quad_gemv reproduces it in registers).
template <int NC, int NT>
__device__ __forceinline__ void symv_cols(const double* __restrict__ M, const double* x, double* out,
                                          double* red, int d) {
  constexpr int NW = NT / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  int j = w;
  // 2-way unrolled over j for memory-level parallelism
  for (; j + NW < d; j += 2 * NW) {
    const double x0 = x[j], x1 = x[j + NW];
    const double* r0 = M + (long)j * d;
    const double* r1 = M + (long)(j + NW) * d;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = lane + 64 * c;
      if (i < d) acc[c] = fma(r1[i], x1, fma(r0[i], x0, acc[c]));
    }
  }
  for (; j < d; j += NW) {
    const double x0 = x[j];
    const double* r0 = M + (long)j * d;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = lane + 64 * c;
      if (i < d) acc[c] = fma(r0[i], x0, acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) red[w * 64 * NC + c * 64 + lane] = acc[c];
  __syncthreads();
  for (int i = threadIdx.x; i < d; i += NT) {
    const int c = i >> 6, l = i & 63;
    double s = 0.0;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) s += red[ww * 64 * NC + c * 64 + l];
    out[i] = s;
  }
  __syncthreads();
}

}  // namespace chain_dev
using namespace chain_dev;
