// Arguments of the persistent logistic kernels beside PersistArgs: one ABI for the inner-GD kernels
// (chain_persistent_logistic.hip) and the exact Newton kernels (chain_persistent_newton.hip).
// ctypes mirror: gadmm_amd/ops/native.py (LogiArgs), checked against gadmm_logi_abi_layout.
#pragma once
#include "gadmm_chain.h"

struct LogiArgs {
  const double* X;  // [n_local][m][d]
  const double* Y;  // [n_local][m]
  int m, max_inner;
  double lam, step, inner_tol;  // Newton: step = chord threshold (<= 0: a fresh inverse every step)
  int* inner_iters;             // [n_local] optional: GD / Newton steps of the worker's last local solve
  double* scratch;              // Newton pipeline kernel only: [n_local][RSLOTS][4 QB] refresh images (P | B | XP | XB)
};

// One slot of the inner-GD sweep kernel (chain_logistic_sweep.hip: up to eight solves in one launch, slot
// j on the blocks b % 8 == j): the solve's own PersistArgs and LogiArgs. Written by the host before the
// launch and never by a kernel, so the kernel reads it like kernel arguments, through the constant
// address space (LogiSweepSlot: wave-uniform scalar loads). Only X, Y and the plan tables (slots, pos)
// may be shared between slots. ctypes mirror: LogiSweepArgs, checked against gadmm_logi_sweep_abi_layout.
struct LogiSweepArgs {
  PersistArgs p;
  LogiArgs g;
};
#if defined(__HIPCC__) || defined(__clang__)
typedef __attribute__((address_space(4))) LogiSweepArgs LogiSweepSlot;
#endif
