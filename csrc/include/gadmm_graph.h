// Shared host/device layout of the persistent GGADMM kernel (csrc/kernels/graph_persistent.hip):
// group ADMM on any connected bipartite graph (Ben Issaid et al., arXiv:2009.06459), one GPU, every
// worker local. The specification is gadmm_amd/algorithms/ggadmm.py.
#pragma once
#include "gadmm_chain.h"

// Arguments of one launch (passed by value; every pointer is a device address). Per-worker arrays are
// indexed by worker id; the launch order (workgroup b runs worker wid[b]) is the heads in ascending
// id, then the tails in ascending id, and the CSR arrays follow that order.
struct GraphArgs {
  int d, n, n_local, start_iter;   // n_local == n: every worker is local
  int max_iter, lag, ring, nranks; // nranks == 1 (the monitor fans its decision out to one ring)
  unsigned epoch;                  // salts every tag: tag = epoch << 20 | iteration (no re-zeroing between solves)
  int max_degree;                  // sizes the neighbour staging in LDS (max_degree * 64 doubles)
  int timeline_iters, pad0;        // (read by monitor_loop; always 0 here)
  double rho, obj0, tol;
  long long timeout_ticks;         // s_memrealtime ticks (100 MHz)
  const int* nb_ptr;               // [n + 1] CSR rows by launch slot
  const int* nb_idx;               // [2 |E|] neighbours as worker ids, ascending inside a row
  const int* wid;                  // [n] worker id of each launch slot
  const int* is_head;              // [n] by launch slot
  const double* Minv;              // [n][d][d]: (A_w + rho deg_w I)^{-1}, each worker's at its own degree
  const double* A;                 // [n][d][d]
  const double* b;                 // [n][d]
  const double* yy;                // [n]
  double* theta;                   // [n][d] in: theta^{start_iter - 1}, out: the last iteration's
  double* mu;                      // [n][d] in/out (out: every worker's dual after the last iteration)
  u32x4* thg;                      // [n][d] theta granules, ONE row per worker
  u32x4* objg;                     // [ring][n] objective ring
  unsigned long long* decg;        // [ring] decision ring
  unsigned long long* const* dec_push;  // [1] -> decg
  double* trace;                   // [max_iter]
  long long* tstamp;               // optional [max_iter] s_memrealtime of each decision
  double* rres;                    // optional K4 primal residual [max_iter][n]: the tails' rows
  ChainCtl* ctl;
  u32x4* xchk;                     // XCD packing: as PersistArgs::xchk / xcd / xtag
  int xcd, xtag;
};

// Q-GGADMM (csrc/kernels/graph_quant.hip): the same launch with a quantized exchange. GraphArgs comes
// first, unchanged (thg is not read); the quantizer's fields follow it.
struct GraphQArgs {
  GraphArgs g;
  u32x4* qg;                       // [n][G] message granules, G = q_words(d, q_bits) + 1: ONE row per worker
  int q_bits, q_pad;               // 4, 8 or 16
  unsigned long long q_seed;
  double* q_true;                  // optional [n][d] out: the TRUE iterates (theta receives the public models)
};
