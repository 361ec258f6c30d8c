// The neighbour poll and the LDS layout of the persistent graph kernels that exchange plain theta granules
// (graph_persistent.hip, graph_persistent_logistic.hip): one table row per worker, the values staged in
// LDS at nbv[k * 64 + lane], lane i reading and writing column i only (no barrier).
#pragma once
#include "persist_device.h"
#include "quad_gemv.h"

constexpr int GFLAGS = 2;  // doubles (16 bytes) at the head of dynamic LDS: the placement verdict's word
// dynamic LDS in doubles: [GFLAGS | monitor: n values] or [GFLAGS | QSTAGE | max_degree * 64 | ids]
__host__ __device__ constexpr long graph_lds_doubles(int n, int max_degree) {
  const long mon = n, wk = (long)QSTAGE + (long)max_degree * 64 + (max_degree + 1) / 2;
  return GFLAGS + (mon > wk ? mon : wk);
}

// One poll of neighbours k0 .. k0 + DK - 1 of a worker (those below deg): all loads first, then the tests;
// the values go to the staging column of this lane. off[j]: byte offset of row nb[k0 + j].
template <int DK>
__device__ __forceinline__ bool poll_group(__amdgpu_buffer_rsrc_t rth, const int (&off)[DK], int k0, int deg, int lane,
                                           unsigned tag, double* nbv) {
  u32x4 g[DK];
#pragma unroll
  for (int j = 0; j < DK; ++j) {
    g[j] = u32x4{0u, 0u, 0u, 0u};
    if (k0 + j < deg) g[j] = load_raw<false>(rth, off[j] + lane * 16);
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < DK; ++j)
    if (k0 + j < deg) {
      ok &= granule_ok(g[j], tag);
      nbv[(k0 + j) * 64 + lane] = granule_val(g[j]);
    }
  return ok;
}

// All neighbours of the worker: the first group from the offsets held in registers, the rest (degree
// > DK, only in a unit's widest DK instantiation) from the id table in LDS.
template <int DK>
__device__ __forceinline__ bool poll_all(__amdgpu_buffer_rsrc_t rth, const int (&off0)[DK], const int* ids, int deg,
                                         int d, int lane, unsigned tag, double* nbv) {
  bool ok = poll_group<DK>(rth, off0, 0, deg, lane, tag, nbv);
  for (int k0 = DK; k0 < deg; k0 += DK) {
    int off[DK];
#pragma unroll
    for (int j = 0; j < DK; ++j) off[j] = (k0 + j < deg ? ids[k0 + j] : 0) * d * 16;
    ok &= poll_group<DK>(rth, off, k0, deg, lane, tag, nbv);
  }
  return ok;
}
