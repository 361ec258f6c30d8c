// GGADMM (Ben Issaid et al., arXiv:2009.06459): group ADMM on any connected bipartite graph, the whole
// solve in one launch on one GPU, d <= 64, one wave per worker (+ the monitor workgroup). The
// specification is gadmm_amd/algorithms/ggadmm.py; schedule, lagged stop rule, deadlines (done = 4)
// and XCD packing are those of chain_persistent_kernel's register variant and of q_persistent_body
// (chain_quant.hip): inverse and Gram sit in VGPRs in the quad layout, lane i owns coordinate i.
//
// Per iteration `it` a head waits for theta^{it-1} of all its tails (nothing at start_iter: the theta
// table has it), a tail for theta^{it} of all its heads. The wait polls ALL the worker's neighbours
// together with the monitor's decision of iteration it - lag in one loop. The granule loads of a spin
// are issued back to back, DK at a time, before any of them is tested: the kernel is instantiated for
// DK = 2, 4, 8, 16 and 32, and the launcher takes the smallest DK >= the graph's maximum degree, so up to
// degree 32 every neighbour of a worker is polled in ONE group; a worker of larger degree goes through
// its neighbours in groups of 32 (a wave that keeps the inverse and the Gram in registers holds 32
// granules in flight without scratch, not more). The neighbours' values go to a staging area of LDS,
// deg * 64 doubles, lane i reading and writing column i only (no barrier), and every sum over
// neighbours runs over that area in CSR order (ascending worker id), whatever order they arrived in.
//
// ONE slot per worker suffices: theta^{it} of worker w overwrites theta^{it-1} in row w of the table.
// A head h publishes it + 1 only after it has left the wait of it + 1, in which every one of its lanes
// read theta^{it} of EVERY tail neighbour. Each of those tails published theta^{it} only after it had
// left the wait of `it`, in which all its lanes read theta^{it} of h (and copied it to LDS). So when h
// overwrites its row, no neighbour still needs the old value. With the roles swapped: a tail t
// publishes it + 1 after reading theta^{it+1} of every head neighbour, and each of those published
// it + 1 after reading theta^{it} of t. A poll that sees one neighbour early reloads it unchanged.
//
// The race this forbids: a tail publishes BEFORE its dual step (that shortens its heads' wait), and once
// it has published a head may overwrite its own row. So a worker never re-reads a neighbour's granule
// after its own publication: the dual step and the K4 residual of a tail, and the lazy dual of a head
// (applied at the start of the next iteration, as in the chain kernels), take the neighbours from the
// staging area, i.e. the very values that fed the right-hand side.
//
// Exit: every worker leaves at the same iteration (the decision of it - lag is read by all of them at
// `it`), after completing iteration `last`. The tails' duals are final; a head still owes its dual
// step of `last`, for which it polls its tails' theta^{last} once more (they have published it and
// publish nothing after it) under the same deadline. theta and mu then go out as after iteration `last`.
#define GADMM_POLL_SLEEP 0  // one hand-off wait per phase on the critical path: poll back to back
#include <stdio.h>
#include <stdlib.h>
#include <cstddef>
#include "gadmm_common.h"
#include "gadmm_graph.h"
#include "persist_device.h"
#include "persist_launch.h"
#include "quad_gemv.h"

namespace {

constexpr int GFLAGS = 2;  // doubles (16 bytes) at the head of dynamic LDS: the placement verdict's word
// dynamic LDS in doubles: [GFLAGS | monitor: n values] or [GFLAGS | QSTAGE | max_degree * 64 | ids]
__host__ __device__ constexpr long graph_lds_doubles(int n, int max_degree) {
  const long mon = n, wk = (long)QSTAGE + (long)max_degree * 64 + (max_degree + 1) / 2;
  return GFLAGS + (mon > wk ? mon : wk);
}

// One poll of neighbours k0 .. k0 + DK - 1 of a worker (those below deg): all loads first, then the tests;
// the values go to the staging column of this lane. off[j]: byte offset of row nb[k0 + j].
template <int DK>
__device__ __forceinline__ bool poll_group(__amdgpu_buffer_rsrc_t rth, const int (&off)[DK], int k0, int deg, int lane,
                                           unsigned tag, double* nbv) {
  u32x4 g[DK];
#pragma unroll
  for (int j = 0; j < DK; ++j) {
    g[j] = u32x4{0u, 0u, 0u, 0u};
    if (k0 + j < deg) g[j] = load_raw<false>(rth, off[j] + lane * 16);
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < DK; ++j)
    if (k0 + j < deg) {
      ok &= granule_ok(g[j], tag);
      nbv[(k0 + j) * 64 + lane] = granule_val(g[j]);
    }
  return ok;
}

// All neighbours of the worker: the first group from the offsets held in registers, the rest (degree
// > DK, only in the DK = 32 instantiation) from the id table in LDS.
template <int DK>
__device__ __forceinline__ bool poll_all(__amdgpu_buffer_rsrc_t rth, const int (&off0)[DK], const int* ids, int deg,
                                         int d, int lane, unsigned tag, double* nbv) {
  bool ok = poll_group<DK>(rth, off0, 0, deg, lane, tag, nbv);
  for (int k0 = DK; k0 < deg; k0 += DK) {
    int off[DK];
#pragma unroll
    for (int j = 0; j < DK; ++j) off[j] = (k0 + j < deg ? ids[k0 + j] : 0) * d * 16;
    ok &= poll_group<DK>(rth, off, k0, deg, lane, tag, nbv);
  }
  return ok;
}

// A sweep slot's GraphArgs (graph_persistent_sweep_kernel below): written by the host before the launch
// and never by a kernel, so it is read like kernel arguments, through the constant address space
// (wave-uniform scalar loads), as SweepArgs of persist_device.h.
typedef __attribute__((address_space(4))) GraphArgs GraphSweepArgs;

// The persistent GGADMM solve (described above) as a body shared by the single-solve and the sweep
// kernel, as q_persistent_body of chain_quant.hip.
// SWEEP: the body runs as one slot of graph_persistent_sweep_kernel: always 8-strided, this slot's
// blocks are blockIdx.x >> 3, and a block past the slot's own n + 1 leaves before the placement check
// and before any barrier (place_block_sweep). Everything the body reads or writes is named by the
// slot's own arguments, and the LDS layout is the slot's own (its n and max_degree) inside a dynamic
// allocation sized for the launch's largest.
// GA: GraphArgs (the kernel's own argument) or GraphSweepArgs (a slot's entry).
template <int QT, int DK, bool SWEEP, class GA>
__device__ __forceinline__ void graph_body(const GA& a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  int* xflag = reinterpret_cast<int*>(lds);  // the placement verdict (xcd_verdict's LDS word)
  const int d = a.d, n = a.n;
  const int lane = threadIdx.x;
  const __amdgpu_buffer_rsrc_t rth = rsrc_of(a.thg);
  const __amdgpu_buffer_rsrc_t rob = rsrc_of(a.objg);
  const unsigned long long deadline = now_ticks() + (unsigned long long)a.timeout_ticks;
  Placement pl;
  if constexpr (SWEEP) pl = place_block_sweep(a.xcd, a.xchk, (unsigned)a.xtag, n + 1, deadline, xflag, a.ctl);
  else pl = place_block<false>(a.xcd, a.xchk, (unsigned)a.xtag, n + 1, deadline, xflag, a.ctl);
  if (pl.spacer) return;
  const int bid = pl.bid;
  const bool local = pl.local;

  if (bid == n) {
    monitor_loop<false, GADMM_POLL_SLEEP>(a, lds + GFLAGS, rob, deadline, a.start_iter, 0, nullptr, 0, 0);
    return;
  }

  // ------------------------------------------------------------------ worker workgroup (one wave)
  const int w = a.wid[bid];
  const bool head = a.is_head[bid] != 0;
  const int p0 = a.nb_ptr[bid];
  int deg = a.nb_ptr[bid + 1] - p0;
  if (deg > a.max_degree) deg = a.max_degree;  // the staging is sized for max_degree (the engine passes the graph's)
  const double rho = a.rho;
  const bool in = lane < d;
  double* st = lds + GFLAGS;             // quad GEMV staging (QSTAGE doubles)
  double* nbv = st + QSTAGE;             // neighbour k's theta at nbv[k * 64 + lane]
  int* ids = reinterpret_cast<int*>(nbv + (long)a.max_degree * 64);  // neighbour ids in CSR order
  for (int k = lane; k < deg; k += 64) ids[k] = a.nb_idx[p0 + k];
  lds_barrier();
  int off0[DK];
#pragma unroll
  for (int j = 0; j < DK; ++j) off0[j] = (j < deg ? a.nb_idx[p0 + j] : 0) * d * 16;  // wave-uniform

  double Mq[4][QT], Aq[4][QT];
  quad_load<QT>(Mq, a.Minv + (long)w * d * d, d, true);
  quad_load<QT>(Aq, a.A + (long)w * d * d, d, true);
  double th = in ? a.theta[(long)w * d + lane] : 0.0;
  double mu = in ? a.mu[(long)w * d + lane] : 0.0;
  const double bb = in ? a.b[(long)w * d + lane] : 0.0;
  const double half_yy = 0.5 * a.yy[w];
  for (int k = 0; k < deg; ++k) nbv[k * 64 + lane] = in ? a.theta[(long)ids[k] * d + lane] : 0.0;
  int pending = 0;  // a head's dual step of the previous iteration is still to apply
  int stop_code = 0, stop_iter = 0;
  int abort = 0;

  int it = a.start_iter;
  int rs = a.start_iter % a.ring;
  for (;; ++it, rs = rs + 1 == a.ring ? 0 : rs + 1) {
    if (it > a.max_iter + a.lag) break;
    // -- the wait: the neighbours' theta and the decision of iteration it - lag in one loop; a stop
    // decision abandons it (a neighbour that saw it publishes no more)
    const bool check = it - a.start_iter >= a.lag;
    const int jdec = it - a.lag;
    const bool need_nb = head ? it > a.start_iter : true;
    const unsigned tnb = make_tag(a.epoch, head ? it - 1 : it);
    int dslot = rs - a.lag;  // == jdec % ring
    if (dslot < 0) dslot += a.ring;
    const unsigned tj = make_tag(a.epoch, jdec);
    bool decided = !check;
    unsigned long long dv = 0;
    int outcome = 0;  // 1 go, 2 stop, 3 timeout
    for (int spin = 0;; ++spin) {
      bool nb = true;
      if (in && need_nb) nb = poll_all<DK>(rth, off0, ids, deg, d, lane, tnb, nbv);
      if (!decided) {
        dv = __shfl(load_dec<false>(&a.decg[dslot]), 0, 64);
        decided = (unsigned)(dv >> 32) == tj;
      }
      if (decided && (unsigned)(dv & 0xffffffffu) != 0u) { outcome = 2; break; }
      if (decided && __all(nb)) { outcome = 1; break; }
      if ((spin & 7) == 7 && now_ticks() > deadline) { outcome = 3; break; }
      GADMM_POLL_PAUSE();
    }
    if (outcome == 3) { abort = 1; break; }
    if (outcome == 2) {
      stop_code = (int)(unsigned)(dv & 0xffffffffu);
      stop_iter = jdec;
      break;
    }
    // -- a head's lazy end-of-iteration dual, then the right-hand side, both over the staged neighbours
    if (head && pending)
      for (int k = 0; k < deg; ++k) mu = mu + rho * (th - nbv[k * 64 + lane]);
    double r = bb - mu;
    for (int k = 0; k < deg; ++k) r = r + rho * nbv[k * 64 + lane];
    // -- solve theta = (A + deg rho I)^{-1} r and publish it
    const double tn = quad_gemv<QT>(Mq, in ? r : 0.0, st);
    const unsigned tag = make_tag(a.epoch, it);
    if (in) put_granule<false>(local, rth, (w * d + lane) * 16, tag, tn);
    if (!head) {  // tails: every neighbour is this iteration's head -> dual step now, from the staged values
      double rp = 0.0;
      for (int k = 0; k < deg; ++k) {
        const double tk = nbv[k * 64 + lane];
        mu = mu + rho * (tn - tk);
        rp = fma(tk - tn, tk - tn, rp);
      }
      if (a.rres) {  // K4 primal residual: the tail's edges (each edge has exactly one tail end)
        const double rsum = wave_sum_f64(in ? rp : 0.0);
        if (lane == 0 && it - 1 < a.max_iter) a.rres[(long)(it - 1) * n + w] = rsum;
      }
    } else {
      pending = 1;
    }
    // -- objective: 1/2 th^T A th - b^T th + 1/2 y^T y
    const double qa = quad_gemv<QT>(Aq, in ? tn : 0.0, st);
    const double part = in ? (0.5 * qa - bb) * tn : 0.0;
    const double f = wave_sum_f64(part) + half_yy;
    if (lane == 0) put_granule<false>(local, rob, (rs * n + w) * 16, tag, f);
    th = tn;
  }

  // a head's dual step of the last iteration: its tails' theta^{last} (published, and final)
  if (head && pending && !abort) {
    const unsigned tl = make_tag(a.epoch, it - 1);
    for (int spin = 0;; ++spin) {
      bool nb = true;
      if (in) nb = poll_all<DK>(rth, off0, ids, deg, d, lane, tl, nbv);
      if (__all(nb)) break;
      if ((spin & 7) == 7 && now_ticks() > deadline) { abort = 1; break; }
      GADMM_POLL_PAUSE();
    }
    if (!abort)
      for (int k = 0; k < deg; ++k) mu = mu + rho * (th - nbv[k * 64 + lane]);
  }
  if (in) {  // final state (plain stores; visible to the host after the kernel)
    a.theta[(long)w * d + lane] = th;
    a.mu[(long)w * d + lane] = mu;
  }
  if (lane == 0) post_outcome<false>(a.ctl, abort, bid, stop_code, stop_iter, it);
}

template <int QT, int DK>
__global__ void __launch_bounds__(64) graph_persistent_kernel(GraphArgs a) {
  graph_body<QT, DK, false>(a);
}

// Up to 8 independent GGADMM solves in one launch, one per XCD: slot j = blockIdx.x & 7 runs solve j on
// the blocks b % 8 == j, i.e. on the blocks that the single-solve launch leaves as exiting spacers.
// batch[j] is solve j's own GraphArgs: its own graph (CSR arrays, launch order), theta / mu, granule
// table, objective and decision rings, ctl, trace, tstamp, rres, xchk, tag salt, rho, stop rule and
// deadline; only the read-only inputs (A, b, yy, Minv, the CSR arrays) may be shared. Slots may differ in
// n, d (within the QT class), graph and degree class: `classes` holds log2 of slot j's own DK (what
// pick_graph_variant gives its single launch) in bits 4 j .. 4 j + 3, and the wave-uniform switch below
// sends the slot into the body of that class, so every slot executes the poll code of its own single
// solve (a chain member does not pay for a star's 32-wide poll group). The kernel's registers are those
// of its widest body. Nothing assumes WHICH XCD a slot gets (place_block_sweep).
template <int QT>
__global__ void __launch_bounds__(64) graph_persistent_sweep_kernel(const GraphArgs* __restrict__ batch, int nb,
                                                                    unsigned classes) {
  const int j = (int)(blockIdx.x & 7u);
  if (j >= nb) return;
  const GraphSweepArgs& a = *(const GraphSweepArgs*)(batch + j);
  switch ((classes >> (4 * j)) & 15u) {
    case 1: graph_body<QT, 2, true>(a); break;
    case 2: graph_body<QT, 4, true>(a); break;
    case 3: graph_body<QT, 8, true>(a); break;
    case 4: graph_body<QT, 16, true>(a); break;
    default: graph_body<QT, 32, true>(a); break;
  }
}

#define GRAPH_SWEEP_CAPACITY 8

struct GVariant {
  const void* fn = nullptr;
  size_t shm = 0;
  int dk = 0;
};

template <int QT>
const void* graph_fn(int dk) {
  if (dk == 2) return (const void*)graph_persistent_kernel<QT, 2>;
  if (dk == 4) return (const void*)graph_persistent_kernel<QT, 4>;
  if (dk == 8) return (const void*)graph_persistent_kernel<QT, 8>;
  if (dk == 16) return (const void*)graph_persistent_kernel<QT, 16>;
  return (const void*)graph_persistent_kernel<QT, 32>;
}

GVariant pick_graph_variant(const GraphArgs& a) {
  GVariant v;
  if (a.d < 1 || a.d > 64 || a.n < 2 || a.max_degree < 1 || a.max_degree >= a.n) return v;
  v.dk = 2;  // the smallest class that polls every neighbour of every worker in one group, at most 32
  while (v.dk < a.max_degree && v.dk < 32) v.dk *= 2;
  // register kernel: QT = 13 covers d <= 52, 16 covers d <= 64 (as chain_persistent_kernel)
  v.fn = a.d <= 52 ? graph_fn<13>(v.dk) : graph_fn<16>(v.dk);
  v.shm = (size_t)graph_lds_doubles(a.n, a.max_degree) * 8;
  return v;
}

// What the launch of one solve asks of its arguments, before residency (`who` prefixes the reason in
// gadmm_set_error): 0 fine, -1 malformed, -2 the staging does not fit in LDS. No HIP call.
int graph_entry_check(const GraphArgs& a, const GVariant& v, const char* who) {
  if (!v.fn) {
    gadmm_set_error("%s: d=%d, n=%d, max_degree=%d not eligible (1 <= d <= 64, n >= 2)", who, a.d, a.n, a.max_degree);
    return -1;
  }
  if (!a.nb_ptr || !a.nb_idx || !a.wid || !a.is_head || !a.Minv || !a.A || !a.b || !a.yy || !a.theta || !a.mu ||
      !a.thg || !a.objg || !a.decg || !a.dec_push || !a.trace || !a.ctl) {
    gadmm_set_error("%s: a required buffer is null", who);
    return -1;
  }
  if (a.n_local != a.n || a.nranks != 1 || a.timeline_iters != 0) {
    gadmm_set_error("%s: one GPU, every worker local", who);
    return -1;
  }
  if (a.lag < 1 || a.ring <= a.lag + 1 || a.start_iter < 1 || a.start_iter + a.max_iter + a.lag >= (1 << 20)) {
    gadmm_set_error("%s: ring must exceed lag + 1, iteration tags are limited to 2^20", who);
    return -1;
  }
  if (v.shm > 65536) {
    gadmm_set_error("%s: max_degree=%d needs %zu bytes of LDS staging, 65536 fit", who, a.max_degree, v.shm);
    return -2;
  }
  return 0;
}

}  // namespace

extern "C" {

// ABI self-description of GraphArgs (ctypes mirror in gadmm_amd/ops/native.py).
int gadmm_graph_abi_layout(long long* out, int n) {
  long long v[] = {(long long)sizeof(GraphArgs),           (long long)offsetof(GraphArgs, epoch),
                   (long long)offsetof(GraphArgs, rho),    (long long)offsetof(GraphArgs, timeout_ticks),
                   (long long)offsetof(GraphArgs, nb_ptr), (long long)offsetof(GraphArgs, Minv),
                   (long long)offsetof(GraphArgs, thg),    (long long)offsetof(GraphArgs, dec_push),
                   (long long)offsetof(GraphArgs, rres),   (long long)offsetof(GraphArgs, ctl),
                   (long long)offsetof(GraphArgs, xchk),   (long long)offsetof(GraphArgs, xtag)};
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n && i < k; ++i) out[i] = v[i];
  return k;
}

// Dynamic LDS bytes of a launch over n workers of maximum degree max_degree.
long gadmm_graph_persistent_lds(int n, int max_degree) { return graph_lds_doubles(n, max_degree) * 8; }

// The degree class (granules polled back to back) the launch of `args` would take; 0: not eligible.
int gadmm_graph_persistent_class(const GraphArgs* args) { return pick_graph_variant(*args).dk; }

// Workgroups the kernel for `args` (d, n, max_degree) can keep resident (0: shape not eligible).
long gadmm_graph_persistent_capacity(const GraphArgs* args) {
  const GVariant v = pick_graph_variant(*args);
  if (!v.fn || v.shm > 65536) return 0;
  return gadmm_resident_capacity(v.fn, 64, v.shm);
}

// -1: malformed arguments; -2: refused (the staging does not fit in LDS, or the n + 1 workgroups cannot
// all be resident) -- either way before anything is launched, the reason in gadmm_set_error.
int gadmm_graph_persistent_launch(const GraphArgs* args, hipStream_t st) {
  const GraphArgs& a = *args;
  const GVariant v = pick_graph_variant(a);
  if (const int rc = graph_entry_check(a, v, "persistent graph kernel")) return rc;
  const int blocks = a.n + 1;
  const long cap = gadmm_resident_capacity(v.fn, 64, v.shm);
  if (blocks > cap) {  // every workgroup must be resident together (they spin on each other)
    gadmm_set_error("persistent graph kernel: %d workgroups but only %ld can be resident", blocks, cap);
    return -2;
  }
  GraphArgs ka = a;
  ka.xcd = gadmm_xcd_pick(a.xcd, 0, blocks, cap, a.xchk);
  ka.xtag = (int)gadmm_next_xtag();  // fresh placement-check tag: no memset of xchk
  void* kargs[] = {&ka};
  GADMM_CHECK(hipLaunchKernel(v.fn, dim3(ka.xcd > 0 ? 8 * blocks : blocks), dim3(64), kargs, v.shm, st));
  GADMM_CHECK(hipGetLastError());
  return 0;
}

// Solves one launch of graph_persistent_sweep_kernel can run side by side (one per XCD).
int gadmm_graph_persistent_sweep_capacity() { return GRAPH_SWEEP_CAPACITY; }

// nb <= 8 independent GGADMM solves (one register class: d <= 52 or 53..64; any graphs, each slot on the
// degree class of its own single launch) in ONE launch, solve j on the blocks b % 8 == j. Every entry
// passes the single launch's checks and names its own written buffers (gadmm_graph_sweep_shares) and a
// placement-check buffer. Dynamic LDS: the largest entry's. Staging buffers and the residency refusal
// (-2: the sum of the workgroups, or one solve's n + 1 past the CUs of an XCD): gadmm_sweep_launch_as.
// -1: refused before any HIP call.
int gadmm_graph_persistent_sweep_launch(const GraphArgs* batch, int nb, GraphArgs* host_stage, GraphArgs* dev_stage,
                                        hipStream_t st) {
  const char* name = "persistent graph sweep";
  if (!gadmm_sweep_batch_ok(name, batch, nb, GRAPH_SWEEP_CAPACITY, host_stage, dev_stage)) return -1;
  int blocks[8], dk[8];
  size_t shm = 0;
  for (int j = 0; j < nb; ++j) {
    const GraphArgs& a = batch[j];
    char who[48];
    snprintf(who, sizeof(who), "%s: solve %d", name, j);
    if ((a.d <= 52) != (batch[0].d <= 52)) {
      gadmm_set_error("%s: solves of different register classes (d = %d and %d; d <= 52 or 53..64)", name, batch[0].d,
                      a.d);
      return -1;
    }
    const GVariant v = pick_graph_variant(a);
    if (const int rc = graph_entry_check(a, v, who)) return rc;
    if (!a.xchk) {
      gadmm_set_error("%s has no placement-check buffer (xchk)", who);
      return -1;
    }
    blocks[j] = a.n + 1;
    if (blocks[j] > XCHK) {
      gadmm_set_error("%s has %d workgroups, the placement check holds %d", who, blocks[j], XCHK);
      return -1;
    }
    for (int i = 0; i < j; ++i)
      if (gadmm_graph_sweep_shares(a, batch[i])) {
        gadmm_set_error("%s: solves %d and %d share a buffer that both write", name, i, j);
        return -1;
      }
    dk[j] = v.dk;
    if (v.shm > shm) shm = v.shm;
  }
  unsigned classes = gadmm_graph_sweep_classes(dk, nb);
  const void* fn = batch[0].d <= 52 ? (const void*)graph_persistent_sweep_kernel<13>
                                    : (const void*)graph_persistent_sweep_kernel<16>;
  return gadmm_sweep_launch_as<GraphArgs>({fn, 64, shm, name, false}, batch, nb, blocks, host_stage, dev_stage, st,
                                          &classes);
}

}  // extern "C"
