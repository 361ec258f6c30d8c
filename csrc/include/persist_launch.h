// Host side of the persistent (single-launch) kernels (csrc/runtime/persist_launch.cpp): residency,
// the XCD packing mode, the launch sequence the chain launchers share, and the one the sweep launchers
// share. Device side: persist_device.h.
#pragma once
#include <stddef.h>
#include <hip/hip_runtime.h>
#include "gadmm_chain.h"
#include "gadmm_common.h"
#include "gadmm_graph.h"

extern "C" {

// Workgroups of `fn` (block size, dynamic LDS) that the device can hold resident at once; 0 on error.
long gadmm_resident_capacity(const void* fn, int threads, size_t shm);
// Effective XCD packing mode (0 off, 1 packed, 2 packed + placement check) of `blocks` working workgroups.
int gadmm_xcd_pick(int want, int multi, int blocks, long cap_total, const void* xchk);
int gadmm_xcd_mode(const PersistArgs* a, int blocks, long cap_total);
// PersistArgs::xtag of a launch: fresh per launch in this process.
unsigned gadmm_next_xtag();

}  // extern "C"

// One persistent launch: the variant its launcher chose.
struct PersistLaunch {
  const void* fn;    // kernel
  int threads;       // block size
  size_t shm;        // dynamic LDS bytes
  int blocks;        // working workgroups (workers [+ objective] [+ monitor])
  const char* name;  // prefix of the error texts ("persistent chain kernel")
  bool pack;         // the kernel has the placement prologue: XCD packing allowed
};

// The common launch sequence, after the launcher's own eligibility checks. ka: the launcher's mutable
// copy of the arguments (its xcd / xtag are set here); kargs: the kernel's argument pointers, kargs[0] == ka.
// -1: ring <= lag + 1, or iteration tags past 2^20; -2: the workgroups cannot all be resident.
int gadmm_persist_launch(const PersistLaunch& l, PersistArgs* ka, void** kargs, hipStream_t st);

// What is out of range in an entry's ring / lag / iteration tags (0: nothing): the test of every launcher.
enum { RANGE_LAG = 1, RANGE_RING = 2, RANGE_TAGS = 4 };  // lag < 1, ring <= lag + 1, tags past 2^20
int gadmm_range_defects(const PersistArgs& a);

// One sweep launch (up to eight solves side by side, solve j on the blocks b % 8 == j): the variant
// its launcher chose.
struct SweepLaunch {
  const void* fn;    // kernel (const PersistArgs* batch, int nb)
  int threads;       // block size
  size_t shm;        // dynamic LDS bytes
  const char* name;  // prefix of the error texts ("blocked sweep")
  bool dbg;          // stamp PersistArgs::dbg of every slot from GADMM_BLK_DBG
};

// The checks every sweep launcher opens with: 1..cap solves, a batch and a staging pair. No HIP call.
bool gadmm_sweep_batch_ok(const char* name, const void* batch, int nb, int cap, const void* host_stage,
                          const void* dev_stage);
// Solves a and o share one of the buffers every sweep kernel writes (ctl, trace, theta, mu, objg, decg,
// xchk, and tstamp / rres where a has them): per-XCD L2s are not coherent, two slots never write one
// buffer. A launcher adds the buffers only its kernel writes.
bool gadmm_sweep_shares(const PersistArgs& a, const PersistArgs& o);
// The common tail of a sweep launch, after the launcher's own eligibility checks. blocks[j]: working
// workgroups of solve j. host_stage (pinned) / dev_stage: nb PersistArgs each, owned by the caller and
// left alone until the stream has drained; the entries (with their xcd, xtag and dbg set here) go up in
// one async copy ahead of the kernel. -2: the workgroups cannot all be resident together, or a solve's
// own not on the one XCD that its 8-strided blocks are dealt to.
int gadmm_sweep_launch(const SweepLaunch& l, const PersistArgs* batch, int nb, const int* blocks,
                       PersistArgs* host_stage, PersistArgs* dev_stage, hipStream_t st);

// gadmm_sweep_shares for the graph sweeps (graph_persistent.hip, graph_quant.hip): ctl, trace, theta, mu,
// thg, objg, decg, dec_push, xchk, and tstamp / rres where a has them. A, b, yy, Minv and the CSR arrays
// may be shared. The Q launcher adds qg and q_true.
bool gadmm_graph_sweep_shares(const GraphArgs& a, const GraphArgs& o);
// The graph sweep kernels' third argument: log2 of slot j's degree class dk[j] (2 .. 32) in bits 4 j .. 4 j + 3.
unsigned gadmm_graph_sweep_classes(const int* dk, int nb);

// The same tail over any slot argument type (gadmm_sweep_launch is its PersistArgs instantiation; the
// graph sweeps run it over GraphArgs / GraphQArgs). SweepSlot<Args> names where a slot keeps what the
// tail sets: xcd(), xtag(), and set_dbg() (a no-op where the kernel has no debug word).
template <class Args>
struct SweepSlot;

template <>
struct SweepSlot<PersistArgs> {
  static int& xcd(PersistArgs& a) { return a.xcd; }
  static int& xtag(PersistArgs& a) { return a.xtag; }
  static void set_dbg(PersistArgs& a, int v) { a.dbg = v; }
};

template <>
struct SweepSlot<GraphArgs> {
  static int& xcd(GraphArgs& a) { return a.xcd; }
  static int& xtag(GraphArgs& a) { return a.xtag; }
  static void set_dbg(GraphArgs&, int) {}
};

template <>
struct SweepSlot<GraphQArgs> {
  static int& xcd(GraphQArgs& a) { return a.g.xcd; }
  static int& xtag(GraphQArgs& a) { return a.g.xtag; }
  static void set_dbg(GraphQArgs&, int) {}
};

// The residency half of the tail (no argument type in it): the sum of blocks[] against the resident
// capacity of the kernel, each blocks[j] against the CUs of one XCD, and the dynamic-LDS attribute past
// 64 KiB. *max_blocks: the widest slot. 0, -2 (refused), or a HIP error.
int gadmm_sweep_residency(const SweepLaunch& l, int nb, const int* blocks, int* max_blocks);
// GADMM_BLK_DBG (0 if unset) and GADMM_XCD (-1 if unset), as the tail reads them per launch.
void gadmm_sweep_env(int* dbg, int* xenv);

// extra: nullable pointer to a third kernel argument (after batch and nb), e.g. the graph sweeps' classes.
template <class Args>
int gadmm_sweep_launch_as(const SweepLaunch& l, const Args* batch, int nb, const int* blocks, Args* host_stage,
                          Args* dev_stage, hipStream_t st, void* extra = nullptr) {
  int max_blocks = 0;
  if (const int rc = gadmm_sweep_residency(l, nb, blocks, &max_blocks)) return rc;
  int dbg = 0, xenv = -1;
  gadmm_sweep_env(&dbg, &xenv);
  for (int j = 0; j < nb; ++j) {
    Args& ka = host_stage[j];
    ka = batch[j];
    if (l.dbg) SweepSlot<Args>::set_dbg(ka, dbg);
    // the 8-strided layout is inherent to a sweep: 0 (no packing) maps to 1 (packed, sc1 stores)
    const int x = xenv >= 0 ? xenv : SweepSlot<Args>::xcd(ka);
    SweepSlot<Args>::xcd(ka) = x >= 2 ? 2 : 1;
    // fresh placement-check tag per slot and per launch (a continuation re-runs the check): no memset of xchk
    SweepSlot<Args>::xtag(ka) = (int)gadmm_next_xtag();
  }
  GADMM_CHECK(hipMemcpyAsync(dev_stage, host_stage, (size_t)nb * sizeof(Args), hipMemcpyHostToDevice, st));
  const Args* dbatch = dev_stage;
  void* kargs[] = {&dbatch, &nb, extra};
  GADMM_CHECK(hipLaunchKernel(l.fn, dim3(8 * max_blocks), dim3(l.threads), kargs, l.shm, st));
  GADMM_CHECK(hipGetLastError());
  return 0;
}
