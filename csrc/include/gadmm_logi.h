// Arguments of the persistent logistic kernels beside PersistArgs: one ABI for the inner-GD kernels
// (chain_persistent_logistic.hip) and the exact Newton kernels (chain_persistent_newton.hip).
// ctypes mirror: gadmm_amd/ops/native.py (LogiArgs), checked against gadmm_logi_abi_layout.
#pragma once

struct LogiArgs {
  const double* X;  // [n_local][m][d]
  const double* Y;  // [n_local][m]
  int m, max_inner;
  double lam, step, inner_tol;  // Newton: step = chord threshold (<= 0: a fresh inverse every step)
  int* inner_iters;             // [n_local] optional: GD / Newton steps of the worker's last local solve
  double* scratch;              // Newton pipeline kernel only: [n_local][RSLOTS][4 QB] refresh images (P | B | XP | XB)
};
