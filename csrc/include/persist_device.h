// Device helpers shared by the persistent (single-launch) kernels: data-is-flag granules
// (cdna_hip_programming.md §6 Guideline 16, R2), wall-clock deadlines, LDS-resident GEMV, and the
// protocol every engine wraps around its worker loop: the placement prologue (place_block), the
// stop-rule monitor (monitor_loop) and, on the worker side, the phase wait and the stop epilogue
// (wait_decision, post_outcome). Host side of the protocol: persist_launch.h.
#pragma once
#include "gadmm_common.h"
#include "stop_rule.h"

// Pause between two polls of a hand-off spin (s_sleep units of 64 clocks; 0 = poll back to back).
#ifndef GADMM_POLL_SLEEP
#define GADMM_POLL_SLEEP 1
#endif
#define GADMM_POLL_PAUSE()                                              \
  do {                                                                  \
    if (GADMM_POLL_SLEEP > 0) __builtin_amdgcn_s_sleep(GADMM_POLL_SLEEP); \
  } while (0)
#include "gadmm_chain.h"
#include "quad_gemv.h"

// The fence-free LDS ring post (lds_post below: the s ring of the two-wave logistic kernel, the pipeline
// rings of the Newton kernel) relies on one hardware property: the LDS instructions of ONE wave are performed in issue order
// (CDNA3 / CDNA4: the property every counted `s_waitcnt lgkmcnt(N)` on a wave's LDS traffic relies on,
// cdna_hip_programming.md §5). The HIP / LLVM memory model does not promise it, so it is enabled only
// for the architectures whose ISA documents it; any other target compiles the fenced (release) post.
// tests/test_gpu.py::test_postfence_stress checks the two posts give bit-identical traces on gfx950.
#if defined(__gfx950__) || defined(__gfx942__)
#define GADMM_LDS_IN_ORDER 1
#else
#define GADMM_LDS_IN_ORDER 0
#endif

namespace persist {

// Hand-offs between the waves of one workgroup through LDS words. LDS-only ordering: the fences name the
// "local" address space, so they wait for LDS operations only (lgkmcnt). A plain workgroup fence would
// also wait for the wave's outstanding GLOBAL stores (vmcnt): the write-through theta granules it has
// just published (~1 us each).
__device__ __forceinline__ int lds_load_acq(const int* p) {
  const int v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  return v;
}
__device__ __forceinline__ void lds_store_rel(int* p, int v) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// A per-step ring post without the release fence: a wave's LDS operations are performed in order
// (GADMM_LDS_IN_ORDER), so a flag written after the ring data it announces (or after the reads of a
// slot it frees) cannot become visible before them; the fence's s_waitcnt only held the flag back by
// one LDS round trip. The compiler barrier keeps the data accesses first. `fenced` (PersistArgs::dbg
// bit 17: GADMM_LOGISTIC_POSTFENCE / GADMM_NEWTON_POSTFENCE = 1) restores the fenced post (A/B).
__device__ __forceinline__ void lds_post(int* p, int v, bool fenced) {
  if (fenced || !GADMM_LDS_IN_ORDER) {  // fence-free only where in-order LDS is documented
    lds_store_rel(p, v);
    return;
  }
  asm volatile("" ::: "memory");
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}


__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}

template <bool SYS>
__device__ __forceinline__ void store_granule(__amdgpu_buffer_rsrc_t rs, int byte_off, unsigned tag, double v) {
  const unsigned long long bits = __double_as_longlong(v);
  u32x4 g = {tag, (unsigned)(bits & 0xffffffffull), tag, (unsigned)(bits >> 32)};
  if (SYS) __builtin_amdgcn_raw_buffer_store_b128(g, rs, byte_off, 0, 17 /* sc0 sc1 */);
  else __builtin_amdgcn_raw_buffer_store_b128(g, rs, byte_off, 0, 16 /* sc1 */);
}

// Plain (write-back) granule store: the line stays in this XCD's L2, so a same-XCD `sc1` reader is
// served from L2 instead of re-fetching it across the fabric (MI355X_MICROARCH.md, price list:
// `sc1` stores DROP the line). Visible ONLY to readers on the same XCD: callers must have verified
// the placement of every reader (xcd_verdict below, through place_block).
__device__ __forceinline__ void store_granule_local(__amdgpu_buffer_rsrc_t rs, int byte_off, unsigned tag, double v) {
  const unsigned long long bits = __double_as_longlong(v);
  u32x4 g = {tag, (unsigned)(bits & 0xffffffffull), tag, (unsigned)(bits >> 32)};
  __builtin_amdgcn_raw_buffer_store_b128(g, rs, byte_off, 0, 0);
}

// store_granule, or (one GPU, placement verified: `local` wave-uniform) store_granule_local
template <bool SYS>
__device__ __forceinline__ void put_granule(bool local, __amdgpu_buffer_rsrc_t rs, int byte_off, unsigned tag, double v) {
  if (!SYS && local) store_granule_local(rs, byte_off, tag, v);
  else store_granule<SYS>(rs, byte_off, tag, v);
}

// This wave's XCD (0-7).
__device__ __forceinline__ unsigned xcc_id() {
  unsigned x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
  return x;
}

template <bool SYS>
__device__ __forceinline__ bool load_granule(__amdgpu_buffer_rsrc_t rs, int byte_off, unsigned tag, double* v) {
  const u32x4 g = SYS ? __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 17)
                      : __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 16);
  *v = __longlong_as_double((long long)(((unsigned long long)g.w << 32) | g.y));
  return g.x == tag && g.z == tag;
}

template <bool SYS>
__device__ __forceinline__ u32x4 load_raw(__amdgpu_buffer_rsrc_t rs, int byte_off) {
  return SYS ? __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 17)
             : __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 16);
}
__device__ __forceinline__ bool granule_ok(const u32x4& g, unsigned tag) { return g.x == tag && g.z == tag; }
__device__ __forceinline__ double granule_val(const u32x4& g) {
  return __longlong_as_double((long long)(((unsigned long long)g.w << 32) | g.y));
}

template <bool SYS>
__device__ __forceinline__ void store_dec(unsigned long long* p, unsigned long long v) {
  if (SYS) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool SYS>
__device__ __forceinline__ unsigned long long load_dec(unsigned long long* p) {
  if (SYS) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long now_ticks() { return __builtin_amdgcn_s_memrealtime(); }

__device__ __forceinline__ unsigned make_tag(unsigned epoch, int it) { return (epoch << 20) | ((unsigned)it & 0xfffffu); }

// Every lane of wave 0 polls the granules of its elements of table row `row` until all carry `tag`.
template <int NC, bool SYS>
__device__ __forceinline__ bool wait_row(__amdgpu_buffer_rsrc_t rs, int row, int d, unsigned tag, double (&out)[NC],
                                         unsigned long long deadline) {
  const int lane = threadIdx.x & 63;
  for (;;) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = lane + 64 * c;
      if (i < d) ok &= load_granule<SYS>(rs, (row * d + i) * 16, tag, &out[c]);
    }
    if (__all(ok)) return true;
    if (now_ticks() > deadline) return false;
    GADMM_POLL_PAUSE();
  }
}

// Poll up to two rows (row < 0: skipped) in ONE loop, so a worker waiting on both chain neighbours
// pays one round trip, not two. Rows may carry different tags. `stopw` (nullable) is a run-wide stop
// word: -1 abort, k > 0 stopped after iteration k (the wait is abandoned once it > k).
// Returns 1 ok, 0 deadline passed, -1 stopped. Wave-uniform.
template <int NC, bool SYS>
__device__ __forceinline__ int wait_pair(__amdgpu_buffer_rsrc_t rs, int d, int ra, unsigned ta, double (&va)[NC],
                                         int rb, unsigned tb, double (&vb)[NC], unsigned long long deadline,
                                         const int* stopw = nullptr, int it = 0) {
  const int lane = threadIdx.x & 63;
  for (int spin = 0;; ++spin) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = lane + 64 * c;
      if (i < d) {
        if (ra >= 0) ok &= load_granule<SYS>(rs, (ra * d + i) * 16, ta, &va[c]);
        if (rb >= 0) ok &= load_granule<SYS>(rs, (rb * d + i) * 16, tb, &vb[c]);
      }
    }
    if (__all(ok)) return 1;
    if ((spin & 7) == 7) {
      if (stopw) {
        const int s = __hip_atomic_load(stopw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s < 0 || (s > 0 && it > s)) return -1;
      }
      if (now_ticks() > deadline) return 0;
    }
    GADMM_POLL_PAUSE();
  }
}

// y[i] = sum_{j < rows} M[j][i] x[j] (M row-major, `cols` wide) with M and x in LDS; lanes own i,
// the block's NW waves split j. Every wave ends with the full y for its lanes' elements; the wave
// partials are combined in fixed order (deterministic, identical in every workgroup).
template <int NC>
__device__ __forceinline__ void gemv_t_lds(const double* M, const double* x, double (&y)[NC], double* red, int rows,
                                           int cols) {
  constexpr int NW = 4;
  const int d = cols;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  // 4 rows of M per batch per wave: the 4 (x NC) LDS loads issue together, one wait per batch
  int j = w;
  for (; j + 3 * NW < rows; j += 4 * NW) {
    double mv[4][NC], xv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      xv[q] = x[j + q * NW];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int i = lane + 64 * c;
        mv[q][c] = i < d ? M[(j + q * NW) * d + i] : 0.0;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = fma(mv[q][c], xv[q], acc[c]);
  }
  for (; j < rows; j += NW) {
    const double xj = x[j];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = lane + 64 * c;
      if (i < d) acc[c] = fma(M[j * d + i], xj, acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) red[(w * NC + c) * 64 + lane] = acc[c];
  lds_barrier();
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double s = 0.0;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) s += red[(ww * NC + c) * 64 + lane];
    y[c] = s;  // every wave holds the full result for its lanes' rows
  }
  lds_barrier();
}

// y = M x for symmetric M (d x d) in LDS.
template <int NC>
__device__ __forceinline__ void symv_lds(const double* M, const double* x, double (&y)[NC], double* red, int d) {
  gemv_t_lds<NC>(M, x, y, red, d, d);
}

constexpr int DREG = 64;  // register-resident variant: d <= 64, one wave per worker

// y_i = sum_j M[i][j] x_j with lane i holding row i of M in registers and x broadcast from LDS
// (zero-padded to DREG); four independent accumulators over j = k mod 4, combined ((a0 + a1) + a2) + a3:
// exactly the summation order of symv_lds / symv_cols (wave k of 4 sums rows j = k mod 4, partials
// added in wave order), so every engine produces bit-identical iterates (M is exactly symmetric).
template <int DB>
__device__ __forceinline__ double reg_gemv(const double (&Mr)[DB], const double* xv) {
  static_assert(DB % 4 == 0, "row length must be a multiple of 4");
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
  for (int j = 0; j < DB; j += 4) {
    const double2 x01 = *reinterpret_cast<const double2*>(xv + j);
    const double2 x23 = *reinterpret_cast<const double2*>(xv + j + 2);
    a0 = fma(Mr[j], x01.x, a0);
    a1 = fma(Mr[j + 1], x01.y, a1);
    a2 = fma(Mr[j + 2], x23.x, a2);
    a3 = fma(Mr[j + 3], x23.y, a3);
  }
  return ((a0 + a1) + a2) + a3;
}

constexpr unsigned XTAG = 0x5a5a0001u;  // placement-check granule tag of launchers that zero xchk first

// XCD packing (PersistArgs::xcd): every working block posts its XCC_ID into xchk[bid] and waits for
// all nb; true iff they are all equal, i.e. every reader of every granule shares this block's L2.
// The verdict is identical in every block (same inputs); false on a deadline (the run then times
// out through its normal path, with sc1 stores). lds_flag: one int of LDS. tag: XTAG behind a memset
// of xchk, or the launch's own PersistArgs::xtag (no memset: earlier launches' granules never match).
__device__ __forceinline__ bool xcd_verdict(u32x4* xchk, int bid, int nb, unsigned long long deadline, int* lds_flag,
                                            unsigned tag = XTAG) {
  const __amdgpu_buffer_rsrc_t rs = rsrc_of(xchk);
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 64) {
    if (lane == 0) store_granule<false>(rs, bid * 16, tag, (double)xcc_id());
    bool ok = true, same = true;
    double first = -1.0;
    for (int i0 = 0; i0 < nb; i0 += 64) {
      const int i = i0 + lane;
      double x = 0.0;
      if (i < nb)
        for (int spin = 0;; ++spin) {
          if (load_granule<false>(rs, i * 16, tag, &x)) break;
          if ((spin & 7) == 7 && now_ticks() > deadline) {
            ok = false;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      if (i0 == 0) first = __shfl(x, 0, 64);  // block 0's XCD
      same &= i >= nb || x == first;
    }
    same = __all(ok && same);
    if (lane == 0) *lds_flag = same ? 1 : 0;
  }
  lds_barrier();
  return __builtin_amdgcn_readfirstlane(*lds_flag) != 0;
}

// Where this block stands in a launch that may be XCD-packed (`xcd`: the launch's PersistArgs::xcd /
// StarArgs::xcd / FoArgs::xcd; packing is one-GPU only, so SYS launches are never packed).
struct Placement {
  bool spacer;  // packed launch, blockIdx.x % 8 != 0: the block has no work and returns at once
  int bid;      // index among the working blocks
  bool local;   // every working block verified on this XCD: publish with plain stores (put_granule)
};

// The opening of a persistent kernel: nb working blocks; xcd > 1 runs xcd_verdict with `tag` and
// `lds_flag` (block-uniform outcome, ends in a workgroup barrier). ctl (nullable): block 0 records the
// placement in ChainCtl::placed.
template <bool SYS>
__device__ __forceinline__ Placement place_block(int xcd, u32x4* xchk, unsigned tag, int nb,
                                                 unsigned long long deadline, int* lds_flag, ChainCtl* ctl = nullptr) {
  const bool packed = !SYS && xcd > 0;
  Placement p;
  p.spacer = packed && (blockIdx.x & 7u);  // only b % 8 == 0 work (one XCD)
  p.bid = packed ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  p.local = false;
  if (p.spacer) return p;
  if (!SYS && xcd > 1) p.local = xcd_verdict(xchk, p.bid, nb, deadline, lds_flag, tag);
  if (!SYS && ctl && p.bid == 0 && threadIdx.x == 0) ctl->placed = xcd > 0 ? (p.local ? 2 : 1) : 0;
  return p;
}

// A sweep slot's PersistArgs (kernels that run up to 8 solves in one launch, slot j on the blocks
// b % 8 == j): written by the host before the launch and never by a kernel, so it is read like kernel
// arguments, through the constant address space (wave-uniform scalar loads).
typedef __attribute__((address_space(4))) PersistArgs SweepArgs;

// place_block for a block of a sweep slot: the layout is always 8-strided (one GPU), the slot's working
// blocks are blockIdx.x >> 3 < nb, and the grid is sized for the widest slot of the launch, so a block
// with bid >= nb belongs to a wider slot: it is returned as a spacer BEFORE the placement check and
// before any barrier (it posts nothing and nobody waits for it). xchk / tag / ctl are the slot's own:
// nothing assumes which XCD a slot gets, and `local` is the verdict on the slot's own blocks.
__device__ __forceinline__ Placement place_block_sweep(int xcd, u32x4* xchk, unsigned tag, int nb,
                                                       unsigned long long deadline, int* lds_flag, ChainCtl* ctl) {
  Placement p;
  p.bid = (int)(blockIdx.x >> 3);
  p.spacer = p.bid >= nb;
  p.local = false;
  if (p.spacer) return p;
  if (xcd > 1) p.local = xcd_verdict(xchk, p.bid, nb, deadline, lds_flag, tag);
  if (ctl && p.bid == 0 && threadIdx.x == 0) ctl->placed = p.local ? 2 : 1;
  return p;
}

// The stop-rule monitor of every persistent engine: one workgroup per run (on the monitor rank), of
// which wave 0 works and the others return (`wave`: the caller's wave index, wave-uniform). Per iteration it polls the tagged objective granules of
// all n workers in ring slot it % ring, sums them in worker order (the order of the graph engine's
// finish: the traces are bit-identical), records the trace, applies stop_code and fans {tag, code}
// out to every rank's decision ring (dec_push[r], r < nranks). A poll that outlives the deadline
// (tested every 8th poll) decides code 4. It returns after the first non-zero code.
// PA: PersistArgs, a sweep slot's copy of it, or StarArgs (the fields read here have one meaning in
// all of them); what differs between engines is passed explicitly:
//   PAUSE       s_sleep units between two polls, 0 = back to back (each engine's measured choice)
//   vals        LDS, n doubles
//   start_iter  first iteration of this launch
//   hard_stop   > 0 (epoch chunks): no iteration beyond it runs; done = 5 if none decided a stop, and a
//               decision is also written to ctl (the workers may stop at hard_stop before they see it)
//   wave        this wave's index in the block, as the kernel already holds it (recomputing it here cost the
//               blocked kernels two VGPRs and the d = 52 paired kernel its zero scratch)
//   tl          nullable: this workgroup's timeline row; iteration start_iter + k is stamped at
//               tl[k * tl_stride] for k < timeline_iters
template <bool SYS, int PAUSE, class PA>
__device__ __forceinline__ void monitor_loop(const PA& a, double* vals, __amdgpu_buffer_rsrc_t rob,
                                             unsigned long long deadline, int start_iter, int hard_stop,
                                             long long* tl, int tl_stride, int wave) {
  if (wave != 0) return;
  const int lane = threadIdx.x & 63, n = a.n;
  for (int it = start_iter;; ++it) {
    if (hard_stop > 0 && it > hard_stop) {  // chunk exhausted without a stop decision
      if (lane == 0) a.ctl->done = 5;
      return;
    }
    const unsigned tag = make_tag(a.epoch, it);
    const int slot = it % a.ring;
    bool okall = true;
    for (int w = lane; w < n; w += 64) {
      double val = 0.0;
      for (int spin = 0;; ++spin) {
        if (load_granule<SYS>(rob, (slot * n + w) * 16, tag, &val)) break;
        if ((spin & 7) == 7 && now_ticks() > deadline) {
          okall = false;
          break;
        }
        if (PAUSE > 0) __builtin_amdgcn_s_sleep(PAUSE);
      }
      vals[w] = val;
    }
    const bool ok = __all(okall);
    unsigned code = 0;
    if (lane == 0) {
      if (!ok) {
        code = 4;
      } else {
        double s = 0.0;
        for (int w = 0; w < n; ++w) s += vals[w];  // worker order: deterministic, == every other engine
        if (it - 1 < a.max_iter) a.trace[it - 1] = s;
        code = (unsigned)stop_code(s, a.obj0, a.tol, it, a.max_iter);
        if (a.tstamp && it - 1 < a.max_iter) a.tstamp[it - 1] = (long long)now_ticks();
      }
      const unsigned long long dv = ((unsigned long long)tag << 32) | code;
      for (int r = 0; r < a.nranks; ++r) store_dec<SYS>(a.dec_push[r] + slot, dv);
      if (code && hard_stop > 0) {
        a.ctl->done = (int)code;
        a.ctl->conv_iter = it;
      }
      const int k = it - start_iter;
      if (tl && k < a.timeline_iters) tl[(long)k * tl_stride] = (long long)now_ticks();
    }
    if (__shfl((int)code, 0, 64)) return;
  }
}

struct NoPollHook {
  __device__ __forceinline__ void operator()(bool, bool) const {}
};

// The worker side of the same protocol: one wave's wait before iteration `it`, for what its neighbours
// publish and for the monitor's decision of iteration it - lag (needed once it - start_iter >= lag), in
// ONE loop, so both cost one round trip. A stop decision abandons the wait (a neighbour that saw it
// publishes no more). Returns 1 go, 2 stop (code / stop_iter: the decision and its iteration it - lag),
// 3 deadline passed (tested every 8th poll). Wave-uniform.
//   poll   () -> bool: issues the site's neighbour loads, this lane's "all arrived" bit
//   dslot  (it - lag) % ring as the site computes it (read only when a decision is needed)
//   PAUSE  s_sleep units between two polls, 0 = back to back (each engine's measured choice)
//   hook   (arrived, decided) after the loads of every poll, before the tests (timeline stamps)
template <bool SYS, int PAUSE, class PA, class Poll, class Hook = NoPollHook>
__device__ __forceinline__ int wait_decision(const PA& a, int it, int start_iter, int dslot, unsigned long long deadline,
                                             Poll poll, int& code, int& stop_iter, Hook hook = Hook()) {
  const int jdec = it - a.lag;
  const unsigned tj = make_tag(a.epoch, jdec);
  bool decided = !(it - start_iter >= a.lag);
  unsigned long long dv = 0;
  for (int spin = 0;; ++spin) {
    const bool nb = poll();
    if (!decided) {
      dv = __shfl(load_dec<SYS>(&a.decg[dslot]), 0, 64);
      decided = (unsigned)(dv >> 32) == tj;
    }
    hook(nb, decided);
    if (decided && (unsigned)(dv & 0xffffffffu) != 0u) {
      code = (int)(unsigned)(dv & 0xffffffffu);
      stop_iter = jdec;
      return 2;
    }
    if (decided && __all(nb)) return 1;
    if ((spin & 7) == 7 && now_ticks() > deadline) return 3;
    if (PAUSE > 0) __builtin_amdgcn_s_sleep(PAUSE);
  }
}

// How a launch ended, into ctl (by one thread of each worker workgroup): done = 4 if this workgroup
// gave up on a deadline, else block 0 records the stop decision the workers left on. CHAIN: the chain
// engines' resume state (pending dual, monitored iteration); the star engine has neither. Returns
// whether anything was recorded.
template <bool CHAIN = true>
__device__ __forceinline__ bool post_outcome(ChainCtl* ctl, int abort, int bid, int stop_code, int stop_iter, int it) {
  if (abort) {
    ctl->done = 4;
    return true;
  }
  if (bid == 0 && stop_code) {
    ctl->done = stop_code;
    ctl->conv_iter = stop_iter;
    ctl->iter = it;
    if (CHAIN) {
      ctl->pending = 1;
      ctl->monitored = stop_iter;
    }
    return true;
  }
  return false;
}

}  // namespace persist
using namespace persist;
