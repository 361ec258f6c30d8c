// The stop rule of every engine (group_ADMM_closedForm.m:105-108), decided once per iteration on the
// global objective s = sum_n f_n(theta_n^it). The order of the tests is part of the contract:
// 3 numerical failure (NaN / inf) before 1 converged (|s - obj0| < tol) before 2 max_iter reached;
// 0: go on. Host and device: csrc/tests/native_selftest.cpp checks it without a GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

__host__ __device__ __forceinline__ int stop_code(double s, double obj0, double tol, int it, int max_iter) {
  if (!(s == s) || isinf(s)) return 3;
  if (fabs(s - obj0) < tol) return 1;
  if (it >= max_iter) return 2;
  return 0;
}
