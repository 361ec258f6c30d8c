// Host side of the persistent (single-launch) kernels: how many workgroups can be resident, the XCD
// packing mode of a launch, the launch sequence the chain launchers share, and the one the sweep
// launchers (up to eight solves in one launch, one per XCD) share (persist_launch.h).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>

#include "gadmm_common.h"
#include "persist_launch.h"

// Occupancy of (kernel, threads, LDS, device), queried once: eligibility checks and launches ask for
// it several times per solve
namespace {
struct OccEntry {
  const void* fn;
  int threads, dev, per_cu;
  size_t shm;
};
std::mutex g_occ_mu;
OccEntry g_occ[128];
int g_occ_n = 0;
}  // namespace

// Workgroups of `fn` (block size, dynamic LDS) that the device can hold resident at once:
// occupancy per CU x CUs. GADMM_CU_BUDGET=<n> replaces the CU count (tests of a partitioned or
// shared device). A persistent launch needs every one of its workgroups resident together: the
// workers spin on each other, so a workgroup that waits for a CU would stall the rest until the
// deadline. 0 on error.
extern "C" long gadmm_resident_capacity(const void* fn, int threads, size_t shm) {
  int dev = 0, per_cu = -1;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  {
    std::lock_guard<std::mutex> lk(g_occ_mu);
    for (int i = 0; i < g_occ_n; ++i)
      if (g_occ[i].fn == fn && g_occ[i].threads == threads && g_occ[i].shm == shm && g_occ[i].dev == dev) {
        per_cu = g_occ[i].per_cu;
        break;
      }
  }
  if (per_cu < 0) {
    per_cu = 0;
    if (shm > 65536 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess)
      return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, shm) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lk(g_occ_mu);
    if (g_occ_n < 128) g_occ[g_occ_n++] = OccEntry{fn, threads, dev, per_cu, shm};
  }
  long cus = gadmm_cu_count();
  if (cus <= 0) return 0;
  if (const char* e = getenv("GADMM_CU_BUDGET")) {
    const long b = atol(e);
    if (b > 0 && b < cus) cus = b;
  }
  return (long)per_cu * cus;
}

// Effective XCD packing mode (PersistArgs::xcd / StarArgs::xcd `want`; env GADMM_XCD overrides it for
// A/B runs) of a launch of `blocks` working workgroups: one GPU only (`multi` = 0), and only when all
// of them fit on one XCD (cap_total / 8 of the `cap_total` resident slots), since packing deals every
// one of them there. Mode 2 needs the placement-check buffer.
extern "C" int gadmm_xcd_pick(int want, int multi, int blocks, long cap_total, const void* xchk) {
  int x = want;
  if (const char* e = getenv("GADMM_XCD")) x = atoi(e);
  if (x < 0) x = 0;
  if (x > 2) x = 2;
  if (multi || blocks > XCHK || (long)blocks > cap_total / 8) x = 0;
  if (x == 2 && !xchk) x = 1;
  return x;
}

extern "C" int gadmm_xcd_mode(const PersistArgs* a, int blocks, long cap_total) {
  return gadmm_xcd_pick(a->xcd, a->sys_scope || a->nranks > 1, blocks, cap_total, a->xchk);
}

// PersistArgs::xtag of a launch: fresh per launch in this process (high bit set, so never XTAG nor a
// zeroed granule), so the placement-check granules an earlier launch left in xchk never match.
extern "C" unsigned gadmm_next_xtag() {
  static std::atomic<unsigned> launches{0};
  return 0x80000000u | ((launches.fetch_add(1, std::memory_order_relaxed) + 1u) & 0x7fffffffu);
}

int gadmm_range_defects(const PersistArgs& a) {
  return (a.lag < 1 ? RANGE_LAG : 0) | (a.ring <= a.lag + 1 ? RANGE_RING : 0) |
         (a.start_iter + a.max_iter + a.lag >= (1 << 20) ? RANGE_TAGS : 0);
}

int gadmm_persist_launch(const PersistLaunch& l, PersistArgs* ka, void** kargs, hipStream_t st) {
  const int bad = gadmm_range_defects(*ka);  // (a launcher whose kernel needs lag >= 1 says so itself)
  if (bad & RANGE_RING) {
    gadmm_set_error("%s: ring must exceed lag + 1", l.name);
    return -1;
  }
  if (bad & RANGE_TAGS) {
    gadmm_set_error("%s: iteration tags limited to 2^20", l.name);
    return -1;
  }
  const long cap = gadmm_resident_capacity(l.fn, l.threads, l.shm);
  if (l.blocks > cap) {  // every workgroup must be resident together (they spin on each other)
    gadmm_set_error("%s: %d workgroups but only %ld can be resident", l.name, l.blocks, cap);
    return -2;
  }
  if (l.shm > 65536) GADMM_CHECK(hipFuncSetAttribute(l.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.shm));
  ka->xcd = l.pack ? gadmm_xcd_mode(ka, l.blocks, cap) : 0;
  ka->xtag = (int)gadmm_next_xtag();  // fresh placement-check tag: no memset of xchk
  GADMM_CHECK(hipLaunchKernel(l.fn, dim3(ka->xcd > 0 ? 8 * l.blocks : l.blocks), dim3(l.threads), kargs, l.shm, st));
  GADMM_CHECK(hipGetLastError());
  return 0;
}

bool gadmm_sweep_batch_ok(const char* name, const void* batch, int nb, int cap, const void* host_stage,
                          const void* dev_stage) {
  if (nb < 1 || nb > cap) {
    gadmm_set_error("%s: %d solves, one launch takes 1..%d", name, nb, cap);
    return false;
  }
  if (!batch || !host_stage || !dev_stage) {
    gadmm_set_error("%s: null batch or staging buffer", name);
    return false;
  }
  return true;
}

bool gadmm_sweep_shares(const PersistArgs& a, const PersistArgs& o) {
  return o.ctl == a.ctl || o.trace == a.trace || o.theta == a.theta || o.mu == a.mu || o.objg == a.objg ||
         o.decg == a.decg || o.xchk == a.xchk || (a.tstamp && o.tstamp == a.tstamp) || (a.rres && o.rres == a.rres);
}

bool gadmm_graph_sweep_shares(const GraphArgs& a, const GraphArgs& o) {
  return o.ctl == a.ctl || o.trace == a.trace || o.theta == a.theta || o.mu == a.mu || (a.thg && o.thg == a.thg) ||
         o.objg == a.objg || o.decg == a.decg || o.dec_push == a.dec_push || o.xchk == a.xchk ||
         (a.tstamp && o.tstamp == a.tstamp) || (a.rres && o.rres == a.rres);
}

unsigned gadmm_graph_sweep_classes(const int* dk, int nb) {
  unsigned c = 0;
  for (int j = 0; j < nb; ++j) {
    unsigned l = 0;
    while ((1 << l) < dk[j]) ++l;
    c |= l << (4 * j);
  }
  return c;
}

int gadmm_sweep_residency(const SweepLaunch& l, int nb, const int* blocks, int* max_blocks_out) {
  int max_blocks = 0, sum_blocks = 0;
  for (int j = 0; j < nb; ++j) {
    sum_blocks += blocks[j];
    if (blocks[j] > max_blocks) max_blocks = blocks[j];
  }
  *max_blocks_out = max_blocks;
  // every workgroup of every solve must be resident together, and a solve's own on the one XCD that
  // its 8-strided blocks are dealt to
  const long cap = gadmm_resident_capacity(l.fn, l.threads, l.shm);
  const long cus_xcd = gadmm_cu_count() / 8;
  if (sum_blocks > cap) {
    gadmm_set_error("%s: %d workgroups but only %ld can be resident", l.name, sum_blocks, cap);
    return -2;
  }
  for (int j = 0; j < nb; ++j)
    if (blocks[j] > cus_xcd) {
      gadmm_set_error("%s: solve %d has %d workgroups but an XCD has %ld CUs", l.name, j, blocks[j], cus_xcd);
      return -2;
    }
  if (l.shm > 65536) GADMM_CHECK(hipFuncSetAttribute(l.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.shm));
  return 0;
}

void gadmm_sweep_env(int* dbg, int* xenv) {
  *dbg = 0;
  *xenv = -1;
  if (const char* e = getenv("GADMM_BLK_DBG")) *dbg = atoi(e);
  if (const char* e = getenv("GADMM_XCD")) *xenv = atoi(e);
}

int gadmm_sweep_launch(const SweepLaunch& l, const PersistArgs* batch, int nb, const int* blocks,
                       PersistArgs* host_stage, PersistArgs* dev_stage, hipStream_t st) {
  return gadmm_sweep_launch_as<PersistArgs>(l, batch, nb, blocks, host_stage, dev_stage, st);
}
