// Host side of the persistent (single-launch) kernels (csrc/runtime/persist_launch.cpp): residency,
// the XCD packing mode, and the launch sequence the chain launchers share. Device side: persist_device.h.
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
