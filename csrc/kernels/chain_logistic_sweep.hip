// Up to 8 independent inner-GD logistic GADMM solves in ONE launch, one per XCD, on one GPU with a static
// chain: the rho / max_inner / inner_tol sweep of the logistic solve (LogisticRegression_Synthetic.m:88-100).
//
// The single solve (chain_persistent_logistic.hip) is latency-bound -- every inner step is one dependent
// d <= 64 register GEMV, the sigmoid and a ring post -- and is packed onto one XCD by an 8x wider grid
// whose blocks b % 8 != 0 exit at once. Here those blocks work: slot j = blockIdx.x & 7 runs solve j on
// the blocks blockIdx.x >> 3, so a sweep of K <= 8 solves takes about the time of its slowest member.
//
// Work split: a worker is one workgroup, as in the single solve, of either layout (one per launch):
//   ZREC = true   two waves (128 threads): the iterate wave holds X and X^T in VGPRs (quad layout,
//                 quad_gemv.h), the margins wave K = X X^T; s_k crosses through a 64-slot LDS ring. LDS:
//                 two QSTAGE staging areas, z_0 / c, the ring, K and the control words (~76 KB: two
//                 workgroups per CU).
//   ZREC = false  one wave (64 threads, QSTAGE doubles of LDS): bit-identical to the graph engine.
// and of one register class, T = 13 for max(d, m) <= 52 and T = 16 for 53..64. Each slot adds its monitor
// workgroup. The bodies (logi_body.h) are this unit's own copy of the single-solve kernels'
// loops, statement for statement, so a slot computes what its own single launch computes, bit for bit.
// A copy, because the single-solve kernels built on a shared body measured 2.1 % slower (5.100 vs 4.995 ms
// on E3 against the parent's library in one GPU call, at equal register, scratch and LDS figures for that
// instantiation; profiles/logistic_sweep): the kernels of chain_persistent_logistic.hip keep their own text, and
// what the two units must agree on (block size, s ring, LDS size, the fast sigmoid) is logi_layout.h.
//
// A slot's arguments are its LogiSweepArgs {PersistArgs p; LogiArgs g} (gadmm_logi.h), staged by the host
// in one copy ahead of the launch and read through the constant address space. Per slot, its own: rho,
// step, lam, max_inner, inner_tol, obj0, tol, max_iter, theta / mu, the theta granule table, objective
// and decision rings, ctl, trace, tstamp, rres, inner_iters, xchk, tag salt (epoch), deadline and dbg
// bits. Shared read-only: the shards X, Y and the plan tables slots / pos. Nothing assumes WHICH XCD a
// slot gets: with xcd = 2 a slot verifies that its own blocks reported one XCC_ID (xcd_verdict on its own
// xchk under its own xtag) before it publishes with plain stores, else it publishes with sc1 stores;
// readers load with sc1 either way. A block of a slot j >= nb, or past its slot's n_local + 1, returns
// before the placement check, any barrier and any LDS flag.
#include "gadmm_common.h"
#include "gadmm_chain.h"
#include "persist_device.h"
#include "persist_launch.h"
#include "gadmm_logi.h"
#include "logi_body.h"
#include <cstddef>
#include <stdio.h>
#include <stdlib.h>

template <int T, bool ZREC>
__global__ void __launch_bounds__(ZREC ? ZR_NT : 64)
    chain_persistent_logistic_sweep_kernel(const LogiSweepArgs* __restrict__ batch, int nb) {
  const int j = (int)(blockIdx.x & 7u);
  if (j >= nb) return;
  const LogiSweepSlot& s = *(const LogiSweepSlot*)(batch + j);
  if constexpr (ZREC) logi_zrec_body<T>(s.p, s.g);
  else logi_onewave_body<T>(s.p, s.g);
}

#define LOGI_SWEEP_CAPACITY 8

template <>
struct SweepSlot<LogiSweepArgs> {
  static int& xcd(LogiSweepArgs& a) { return a.p.xcd; }
  static int& xtag(LogiSweepArgs& a) { return a.p.xtag; }
  static void set_dbg(LogiSweepArgs&, int) {}  // (the launcher below sets the logistic bits itself)
};

namespace {

bool env_is(const char* name, char c) {
  const char* e = getenv(name);
  return e && e[0] == c;
}

// The sweep bodies take solve `s` (else: the reason in gadmm_set_error, prefixed `who`). No HIP call.
bool logi_entry_ok(const LogiSweepArgs& s, const char* who) {
  const PersistArgs& a = s.p;
  const LogiArgs& g = s.g;
  const int mx = a.d > g.m ? a.d : g.m;
  if (a.d < 1 || g.m < 1 || mx > 64) {
    gadmm_set_error("%s: d=%d, m=%d not eligible (max(d, m) <= 64)", who, a.d, g.m);
    return false;
  }
  if (g.max_inner < 1) {
    gadmm_set_error("%s: max_inner must be >= 1, got %d", who, g.max_inner);
    return false;
  }
  if (a.sys_scope || a.n_epochs > 0 || a.nranks != 1 || !a.has_monitor || a.push || a.n_local != a.n) {
    gadmm_set_error("%s: one GPU, every worker local, a static chain, with its monitor", who);
    return false;
  }
  if (!g.X || !g.Y || !a.slots || !a.pos || !a.thg || !a.objg || !a.decg || !a.dec_push || !a.theta || !a.mu ||
      !a.ctl || !a.trace) {
    gadmm_set_error("%s: a required buffer is null", who);
    return false;
  }
  if (!a.xchk) {
    gadmm_set_error("%s has no placement-check buffer (xchk)", who);
    return false;
  }
  if (a.n_local + 1 > XCHK) {
    gadmm_set_error("%s has %d workgroups, the placement check holds %d", who, a.n_local + 1, XCHK);
    return false;
  }
  return true;
}

}  // namespace

extern "C" {

// ABI self-description of LogiSweepArgs (ctypes mirror in gadmm_amd/ops/native.py; gadmm_abi_layout and
// gadmm_logi_abi_layout cover the two structs in it).
int gadmm_logi_sweep_abi_layout(long long* out, int n) {
  long long v[] = {(long long)sizeof(LogiSweepArgs), (long long)offsetof(LogiSweepArgs, p),
                   (long long)offsetof(LogiSweepArgs, g), (long long)sizeof(PersistArgs), (long long)sizeof(LogiArgs)};
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n && i < k; ++i) out[i] = v[i];
  return k;
}

// Solves one launch of chain_persistent_logistic_sweep_kernel can run side by side (one per XCD).
int gadmm_chain_persistent_logistic_sweep_capacity() { return LOGI_SWEEP_CAPACITY; }

// nb <= 8 independent inner-GD logistic solves (one GPU each, one register class: max(d, m) <= 52 or
// 53..64) in ONE launch, solve j on the blocks b % 8 == j. GADMM_LOGISTIC_ZREC picks the layout for the
// whole launch; the GADMM_LOGISTIC_FASTSIGM / GADMM_LOGISTIC_POSTFENCE bits go to every slot, as the single
// launcher sets them. Each entry must name its own ctl, trace, theta, mu, theta granule table, objective /
// decision rings, xchk and (where it has them) tstamp, rres and inner_iters. Staging buffers and the
// residency refusal (-2): gadmm_sweep_launch_as. -1: refused before any HIP call.
int gadmm_chain_persistent_logistic_sweep_launch(const LogiSweepArgs* batch, int nb, LogiSweepArgs* host_stage,
                                                 LogiSweepArgs* dev_stage, hipStream_t st) {
  const char* name = "persistent logistic sweep";
  if (!gadmm_sweep_batch_ok(name, batch, nb, LOGI_SWEEP_CAPACITY, host_stage, dev_stage)) return -1;
  const bool zrec = !env_is("GADMM_LOGISTIC_ZREC", '0');
  const int dbg = (env_is("GADMM_LOGISTIC_FASTSIGM", '0') ? 32 : 0) | (env_is("GADMM_LOGISTIC_POSTFENCE", '1') ? 1 << 17 : 0);
  LogiSweepArgs mine[LOGI_SWEEP_CAPACITY];
  int blocks[LOGI_SWEEP_CAPACITY], cls[LOGI_SWEEP_CAPACITY];
  size_t shm = 0;
  for (int j = 0; j < nb; ++j) {
    const PersistArgs& a = batch[j].p;
    char who[48];
    snprintf(who, sizeof(who), "%s: solve %d", name, j);
    if (!logi_entry_ok(batch[j], who)) return -1;
    cls[j] = (a.d > batch[j].g.m ? a.d : batch[j].g.m) <= 52;
    if (cls[j] != cls[0]) {
      gadmm_set_error("%s: solves of different register classes (max(d, m) <= 52 or 53..64)", name);
      return -1;
    }
    for (int i = 0; i < j; ++i) {
      const PersistArgs& o = batch[i].p;
      if (gadmm_sweep_shares(a, o) || o.thg == a.thg || o.dec_push == a.dec_push ||
          (batch[j].g.inner_iters && batch[i].g.inner_iters == batch[j].g.inner_iters)) {
        gadmm_set_error("%s: solves %d and %d share a buffer that both write", name, i, j);
        return -1;
      }
    }
    if (gadmm_range_defects(a)) {
      gadmm_set_error("%s: ring/lag/tag range", who);
      return -1;
    }
    blocks[j] = a.n_local + 1;
    const size_t need = logi_lds_bytes(zrec, a.n);
    if (need > shm) shm = need;
    mine[j] = batch[j];
    mine[j].p.dbg |= dbg;
  }
  const void* fn = zrec ? (cls[0] ? (const void*)chain_persistent_logistic_sweep_kernel<13, true>
                                  : (const void*)chain_persistent_logistic_sweep_kernel<16, true>)
                        : (cls[0] ? (const void*)chain_persistent_logistic_sweep_kernel<13, false>
                                  : (const void*)chain_persistent_logistic_sweep_kernel<16, false>);
  return gadmm_sweep_launch_as<LogiSweepArgs>({fn, zrec ? ZR_NT : 64, shm, name, false}, mine, nb, blocks, host_stage,
                                              dev_stage, st);
}

}  // extern "C"
