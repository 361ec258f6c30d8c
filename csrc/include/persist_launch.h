// Host side of the persistent (single-launch) kernels (csrc/runtime/persist_launch.cpp): residency,
// the XCD packing mode, the launch sequence the chain launchers share, and the one the sweep launchers
// share. Device side: persist_device.h.
#pragma once
#include <stddef.h>
#include <hip/hip_runtime.h>
#include "gadmm_chain.h"

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
