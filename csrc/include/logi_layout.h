// What the single-solve inner-GD logistic kernels (chain_persistent_logistic.hip) and the sweep unit's copy
// of their loops (logi_body.h, chain_logistic_sweep.hip) must agree on: the two-wave worker's block size
// and s ring, the dynamic LDS of either layout and the margins wave's sigmoid.
#pragma once
#include <stddef.h>
#include "quad_gemv.h"
#include "fast_sigm.h"

constexpr int ZR_NT = 128;
constexpr int ZR_SLOTS = 64;  // s ring depth; the margins wave checks it every ZR_CHK steps
// (same-box A/B, E3 bench: 8/4 5.34, 16/4 5.34, 16/8 5.17, 32/8 5.11, 64/8 4.93 ms; 128/8 with an early-end
// check every 8 steps 5.41, 32/16 with one every step 5.43: profiles/r06_logistic)
constexpr int ZR_CHK = 8;

// s = y / (1 + e^{y z}) on the margins wave's critical path: inv1pexp_fast (fast_sigm.h). Measured 5.64 ->
// 5.21 ms on E3, one box (profiles/r05_j/r5jf); the default (GADMM_LOGISTIC_FASTSIGM=0: libm exp and
// the IEEE quotient). The traces stay within 1e-12 of torch.
__device__ __forceinline__ double zr_sigm(double yv, double z) { return yv * inv1pexp_fast(yv * z); }

// Dynamic LDS of a workgroup of either layout (zrec: the two-wave worker): the larger of a worker's and the
// monitor's n * 8. Two-wave worker: [2][QSTAGE] staging | z_0, c [2][64] | s ring [ZR_SLOTS][4 QX] | K [64][64]
// | control ints.
inline size_t logi_lds_bytes(bool zrec, int n) {
  const size_t mon = (size_t)n * 8;
  const size_t wk = zrec ? (size_t)(2 * QSTAGE + 128 + ZR_SLOTS * 4 * QX + 64 * 64) * 8 + 32 : (size_t)QSTAGE * 8;
  return mon > wk ? mon : wk;
}
