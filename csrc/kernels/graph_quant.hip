// Q-GGADMM: GGADMM (graph_persistent.hip) with the quantized exchange of Q-GADMM (chain_quant.hip), the
// whole solve in one launch on one GPU, d <= 64, one wave per worker (+ the monitor workgroup). The
// specification is gadmm_amd/algorithms/ggadmm.py (the quantized recurrence) over the quantizer of
// gadmm_amd/algorithms/quantize.py. Schedule, lagged stop rule, deadlines (done = 4), XCD packing and the
// quad-layout register inverse and Gram are graph_persistent_kernel's; no censoring: every worker
// publishes every iteration, so the wait is that kernel's too (all neighbours at tag `it`, or `it - 1`
// for a head, polled together with the decision of it - lag).
//
// Hand-off: the wire format of chain_persistent_q_kernel. Row w of the message table qg is
// G = q_words(d, bits) + 1 tagged granules, granule 0 the bits of R, granule 1 + k code word k. Per
// neighbour lane i loads the header granule and the one granule that holds its own code: 2 DK loads in
// flight per poll group, so the classes are DK = 2, 4, 8, 16 (32 granules, what a wave that keeps two
// register matrices holds without scratch); a worker of larger degree goes through its neighbours in
// groups of 16. The sender and every receiver move a public model through the same quant::q_apply.
//
// State: the LDS staging nbv[k * 64 + lane] holds this worker's COPY of neighbour k's public model, kept
// from one iteration to the next (lane i reads and writes column i only: no barrier). A message is a
// difference, so it must reach a copy exactly once. The rule:
//
//   * A poll never writes into nbv. A poll group is APPLIED -- nbv[k] <- q_apply(nbv[k], R_k, code_k) for
//     every neighbour k of the group -- in the spin in which every lane saw BOTH granules of EVERY
//     neighbour of the group carry the expected tag (one __all per group: wave-uniform), from the very
//     registers that were tested.
//   * A wave-uniform mask `applied` has one bit per poll group, cleared at the top of every iteration. An
//     applied group sets its bit and is neither polled nor applied again in that wait: a group that is
//     complete while another is not is applied once, not once per spin.
//   * A wait abandoned by a stop decision leaves `applied` as it is, and the head's exit poll (below)
//     goes on from it with the same tag.
//
// Why that is exactly once. (a) Within a wait the mask admits each group once. (b) One slot per worker
// suffices by the argument of graph_persistent.hip: a neighbour overwrites its row with message it + 1
// only after it has left a wait in which it read this worker's NEXT message, which this worker publishes
// only after it has left the present wait, i.e. after every group was applied; so between two spins of
// one wait a neighbour's granules either still miss the tag or hold the one message the wait is for, and
// what is applied is that message whole (both granules tested in the same registers). (c) Nothing
// half-applied survives a stop: a tail abandons the wait of iteration `it` for its heads' message `it`,
// which no head publishes (every head reads the same decision at `it` and leaves), so none of its groups
// was applied and its copies are the heads' public models of `last` = it - 1, consistent with its final
// dual. A head abandons the wait for its tails' message `last`; the groups it applied hold the tails'
// models of `last`, the others those of last - 1. The head owes its dual step of `last`, for which it
// needs exactly message `last` in every copy: the exit poll waits for the groups whose bit is clear --
// the tails have published `last` and publish nothing after it -- and applies each once; the groups
// whose bit is set are skipped, so no copy absorbs the message twice. (When the loop ends at the
// iteration cap without a wait, the mask is clear and the exit poll applies every group.)
//
// The own public model `hat`, the true iterate `th` and the dual `mu` stay in registers; at exit theta
// receives the public models, q_true the true iterates, mu the duals after iteration `last`.
#define GADMM_POLL_SLEEP 0  // one hand-off wait per phase on the critical path: poll back to back
#include <stdio.h>
#include <stdlib.h>
#include <cstddef>
#include "gadmm_common.h"
#include "gadmm_graph.h"
#include "persist_device.h"
#include "persist_launch.h"
#include "quad_gemv.h"
#include "quant_device.h"

using namespace quant;

namespace {

constexpr int GFLAGS = 2;  // doubles (16 bytes) at the head of dynamic LDS: the placement verdict's word
// dynamic LDS in doubles: [GFLAGS | monitor: n values] or [GFLAGS | QSTAGE | max_degree * 64 | ids]
__host__ __device__ constexpr long graph_q_lds_doubles(int n, int max_degree) {
  const long mon = n, wk = (long)QSTAGE + (long)max_degree * 64 + (max_degree + 1) / 2;
  return GFLAGS + (mon > wk ? mon : wk);
}

// What a lane needs to read its code out of a message row.
struct QLane {
  int my_off;      // byte offset, inside a row, of the granule that holds this lane's code
  int my_sh;       // ... and the code's bit position in that word
  unsigned qmask;  // 2^bits - 1
  double L;        // the same as a double
};

// One poll of neighbours k0 .. k0 + DK - 1 (those below deg): all loads first, then the tests; when every
// lane has both granules of every one of them under `tag`, the messages are applied to the copies in nbv
// and the group reports true (wave-uniform; called by the whole wave). off[j]: byte offset of row
// nb[k0 + j] of qg.
template <int DK>
__device__ __forceinline__ bool poll_group_q(__amdgpu_buffer_rsrc_t rq, const int (&off)[DK], int k0, int deg, int lane,
                                             bool in, const QLane& ql, unsigned tag, double* nbv) {
  u32x4 gR[DK], gW[DK];
#pragma unroll
  for (int j = 0; j < DK; ++j) {
    gR[j] = u32x4{0u, 0u, 0u, 0u};
    gW[j] = gR[j];
    if (in && k0 + j < deg) {
      gR[j] = load_raw<false>(rq, off[j]);
      gW[j] = load_raw<false>(rq, off[j] + ql.my_off);
    }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < DK; ++j)
    if (in && k0 + j < deg) ok &= granule_ok(gR[j], tag) && granule_ok(gW[j], tag);
  if (!__all(ok)) return false;
#pragma unroll
  for (int j = 0; j < DK; ++j)
    if (in && k0 + j < deg) {
      double* c = nbv + (k0 + j) * 64 + lane;
      *c = q_apply(*c, __longlong_as_double((long long)raw_bits(gR[j])), ql.L,
                   (unsigned)(raw_bits(gW[j]) >> ql.my_sh) & ql.qmask);
    }
  return true;
}

// Every poll group whose bit in `applied` is clear: the first from the offsets held in registers, the
// rest (degree > DK, only in the DK = 16 instantiation) from the id table in LDS. True when every group
// has been applied. Wave-uniform.
template <int DK>
__device__ __forceinline__ bool poll_all_q(__amdgpu_buffer_rsrc_t rq, const int (&off0)[DK], const int* ids, int deg,
                                           int row_bytes, int lane, bool in, const QLane& ql, unsigned tag, double* nbv,
                                           unsigned& applied) {
  bool all = true;
  if (!(applied & 1u)) {
    if (poll_group_q<DK>(rq, off0, 0, deg, lane, in, ql, tag, nbv)) applied |= 1u;
    else all = false;
  }
  unsigned bit = 2u;
  for (int k0 = DK; k0 < deg; k0 += DK, bit <<= 1) {
    if (applied & bit) continue;
    int off[DK];
#pragma unroll
    for (int j = 0; j < DK; ++j) off[j] = (k0 + j < deg ? ids[k0 + j] : 0) * row_bytes;
    if (poll_group_q<DK>(rq, off, k0, deg, lane, in, ql, tag, nbv)) applied |= bit;
    else all = false;
  }
  return all;
}

// A sweep slot's GraphQArgs (graph_persistent_q_sweep_kernel below), read through the constant address
// space like kernel arguments (as GraphSweepArgs of graph_persistent.hip).
typedef __attribute__((address_space(4))) GraphQArgs GraphQSweepArgs;

// The persistent Q-GGADMM solve (described above) as a body shared by the single-solve and the sweep
// kernel. SWEEP: one slot of graph_persistent_q_sweep_kernel: 8-strided, blocks blockIdx.x >> 3, a block
// past the slot's own n + 1 leaves before the placement check and before any barrier; the LDS layout is
// the slot's own. QA: GraphQArgs (the kernel's own argument) or GraphQSweepArgs (a slot's entry).
template <int QT, int DK, bool SWEEP, class QA>
__device__ __forceinline__ void graph_q_body(const QA& qa) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  int* xflag = reinterpret_cast<int*>(lds);  // the placement verdict (xcd_verdict's LDS word)
  const auto& a = qa.g;
  const int d = a.d, n = a.n;
  const int lane = threadIdx.x;
  const __amdgpu_buffer_rsrc_t rq = rsrc_of(qa.qg);
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
  const int bits = qa.q_bits, lp = q_log2_per(bits);
  const int G = q_words(d, bits) + 1;
  const int row_bytes = G * 16;
  const int my_g = 1 + (lane >> lp);  // the granule that holds this lane's code
  QLane ql;
  ql.my_off = my_g * 16;
  ql.my_sh = bits * (lane & ((1 << lp) - 1));
  ql.qmask = (1u << bits) - 1u;
  ql.L = (double)((1u << bits) - 1u);
  double* st = lds + GFLAGS;             // quad GEMV staging (QSTAGE doubles)
  double* nbv = st + QSTAGE;             // this worker's copy of neighbour k's public model at nbv[k * 64 + lane]
  int* ids = reinterpret_cast<int*>(nbv + (long)a.max_degree * 64);  // neighbour ids in CSR order
  for (int k = lane; k < deg; k += 64) ids[k] = a.nb_idx[p0 + k];
  lds_barrier();
  int off0[DK];
#pragma unroll
  for (int j = 0; j < DK; ++j) off0[j] = (j < deg ? a.nb_idx[p0 + j] : 0) * row_bytes;  // wave-uniform

  double Mq[4][QT], Aq[4][QT];
  quad_load<QT>(Mq, a.Minv + (long)w * d * d, d, true);
  quad_load<QT>(Aq, a.A + (long)w * d * d, d, true);
  // lane i owns coordinate i: the true theta, the worker's own public model (the theta table holds
  // public models) and, in LDS, its copies of the neighbours'
  double th = in ? a.theta[(long)w * d + lane] : 0.0;
  double hat = th;
  double mu = in ? a.mu[(long)w * d + lane] : 0.0;
  const double bb = in ? a.b[(long)w * d + lane] : 0.0;
  const double half_yy = 0.5 * a.yy[w];
  for (int k = 0; k < deg; ++k) nbv[k * 64 + lane] = in ? a.theta[(long)ids[k] * d + lane] : 0.0;
  int pending = 0;  // a head's dual step of the previous iteration is still to apply
  int stop_code = 0, stop_iter = 0;
  int abort = 0;
  unsigned applied = 0u;  // poll groups of the current wait whose messages are in nbv (see the header)

  int it = a.start_iter;
  int rs = a.start_iter % a.ring;
  for (;; ++it, rs = rs + 1 == a.ring ? 0 : rs + 1) {
    applied = 0u;
    if (it > a.max_iter + a.lag) break;
    const double u = q_u01(qa.q_seed, it, n, w, d, lane);  // this iteration's draw: ready before the wait ends
    // -- the wait: the neighbours' messages and the decision of iteration it - lag in one loop; a stop
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
      if (need_nb) nb = poll_all_q<DK>(rq, off0, ids, deg, row_bytes, lane, in, ql, tnb, nbv, applied);
      if (!decided) {
        dv = __shfl(load_dec<false>(&a.decg[dslot]), 0, 64);
        decided = (unsigned)(dv >> 32) == tj;
      }
      if (decided && (unsigned)(dv & 0xffffffffu) != 0u) { outcome = 2; break; }
      if (decided && nb) { outcome = 1; break; }
      if ((spin & 7) == 7 && now_ticks() > deadline) { outcome = 3; break; }
      GADMM_POLL_PAUSE();
    }
    if (outcome == 3) { abort = 1; break; }
    if (outcome == 2) {
      stop_code = (int)(unsigned)(dv & 0xffffffffu);
      stop_iter = jdec;
      break;
    }
    // -- a head's lazy end-of-iteration dual, then the right-hand side, both over the copies (public models)
    if (head && pending)
      for (int k = 0; k < deg; ++k) mu = mu + rho * (hat - nbv[k * 64 + lane]);
    double r = bb - mu;
    for (int k = 0; k < deg; ++k) r = r + rho * nbv[k * 64 + lane];
    // -- solve theta = (A + deg rho I)^{-1} r: the TRUE iterate
    const double tn = quad_gemv<QT>(Mq, in ? r : 0.0, st);
    // -- quantize theta - th_hat and publish the packed message
    const double diff = in ? tn - hat : 0.0;
    const double R = wave_max_f64(fabs(diff));
    const unsigned q = in ? q_code(diff, R, ql.L, u) : 0u;
    const double hat_new = in ? q_apply(hat, R, ql.L, q) : 0.0;
    const unsigned long long word = group_or_u64((unsigned long long)q << ql.my_sh, lp);  // the word of this lane's group
    const unsigned tag = make_tag(a.epoch, it);
    if (in && (lane & ((1 << lp) - 1)) == 0) put_raw(local, rq, w * row_bytes + ql.my_off, tag, word);
    if (lane == 0) put_raw(local, rq, w * row_bytes, tag, (unsigned long long)__double_as_longlong(R));
    if (!head) {  // tails: every neighbour is this iteration's head -> dual step now, from the copies
      double rp = 0.0;
      for (int k = 0; k < deg; ++k) {
        const double tk = nbv[k * 64 + lane];
        mu = mu + rho * (hat_new - tk);
        rp = fma(tk - hat_new, tk - hat_new, rp);
      }
      if (a.rres) {  // K4 primal residual on the public models: the tail's edges (each edge has exactly one tail end)
        const double rsum = wave_sum_f64(in ? rp : 0.0);
        if (lane == 0 && it - 1 < a.max_iter) a.rres[(long)(it - 1) * n + w] = rsum;
      }
    } else {
      pending = 1;
    }
    // -- objective of the TRUE theta: 1/2 th^T A th - b^T th + 1/2 y^T y
    const double qv = quad_gemv<QT>(Aq, in ? tn : 0.0, st);
    const double part = in ? (0.5 * qv - bb) * tn : 0.0;
    const double f = wave_sum_f64(part) + half_yy;
    if (lane == 0) put_granule<false>(local, rob, (rs * n + w) * 16, tag, f);
    th = tn;
    hat = hat_new;
  }

  // a head's dual step of the last iteration: its tails' message `last` (published, and final), applied
  // to the groups the abandoned wait has not applied already
  if (head && pending && !abort) {
    const unsigned tl = make_tag(a.epoch, it - 1);
    for (int spin = 0;; ++spin) {
      if (poll_all_q<DK>(rq, off0, ids, deg, row_bytes, lane, in, ql, tl, nbv, applied)) break;
      if ((spin & 7) == 7 && now_ticks() > deadline) { abort = 1; break; }
      GADMM_POLL_PAUSE();
    }
    if (!abort)
      for (int k = 0; k < deg; ++k) mu = mu + rho * (hat - nbv[k * 64 + lane]);
  }
  if (in) {  // final state (plain stores; visible to the host after the kernel)
    a.theta[(long)w * d + lane] = hat;
    a.mu[(long)w * d + lane] = mu;
    if (qa.q_true) qa.q_true[(long)w * d + lane] = th;
  }
  if (lane == 0) post_outcome<false>(a.ctl, abort, bid, stop_code, stop_iter, it);
}

template <int QT, int DK>
__global__ void __launch_bounds__(64) graph_persistent_q_kernel(GraphQArgs qa) {
  graph_q_body<QT, DK, false>(qa);
}

// Up to 8 independent Q-GGADMM solves in one launch, one per XCD, as graph_persistent_sweep_kernel: slot
// j = blockIdx.x & 7 runs batch[j] on the blocks b % 8 == j, on the body of its own degree class (log2 of
// it in bits 4 j .. 4 j + 3 of `classes`; 2 .. 16 here). Slots may differ in graph, n, d (within the QT
// class), bits and seed; each names its own message table, public models, true iterates, duals, rings,
// ctl, trace and xchk.
template <int QT>
__global__ void __launch_bounds__(64) graph_persistent_q_sweep_kernel(const GraphQArgs* __restrict__ batch, int nb,
                                                                      unsigned classes) {
  const int j = (int)(blockIdx.x & 7u);
  if (j >= nb) return;
  const GraphQSweepArgs& qa = *(const GraphQSweepArgs*)(batch + j);
  switch ((classes >> (4 * j)) & 15u) {
    case 1: graph_q_body<QT, 2, true>(qa); break;
    case 2: graph_q_body<QT, 4, true>(qa); break;
    case 3: graph_q_body<QT, 8, true>(qa); break;
    default: graph_q_body<QT, 16, true>(qa); break;
  }
}

#define GRAPH_Q_SWEEP_CAPACITY 8

struct GQVariant {
  const void* fn = nullptr;
  size_t shm = 0;
  int dk = 0;
};

template <int QT>
const void* graph_q_fn(int dk) {
  if (dk == 2) return (const void*)graph_persistent_q_kernel<QT, 2>;
  if (dk == 4) return (const void*)graph_persistent_q_kernel<QT, 4>;
  if (dk == 8) return (const void*)graph_persistent_q_kernel<QT, 8>;
  return (const void*)graph_persistent_q_kernel<QT, 16>;
}

GQVariant pick_graph_q_variant(const GraphQArgs& qa) {
  const GraphArgs& a = qa.g;
  GQVariant v;
  if (a.d < 1 || a.d > 64 || a.n < 2 || a.max_degree < 1 || a.max_degree >= a.n) return v;
  if (qa.q_bits != 4 && qa.q_bits != 8 && qa.q_bits != 16) return v;
  v.dk = 2;  // the smallest class that polls every neighbour of every worker in one group, at most 16
  while (v.dk < a.max_degree && v.dk < 16) v.dk *= 2;
  // register kernel: QT = 13 covers d <= 52, 16 covers d <= 64 (as graph_persistent_kernel)
  v.fn = a.d <= 52 ? graph_q_fn<13>(v.dk) : graph_q_fn<16>(v.dk);
  v.shm = (size_t)graph_q_lds_doubles(a.n, a.max_degree) * 8;
  return v;
}

// What the launch of one solve asks of its arguments, before residency (`who` prefixes the reason in
// gadmm_set_error): 0 fine, -1 malformed (q_bits outside {4, 8, 16} among them), -2 the staging does not
// fit in LDS. No HIP call.
int graph_q_entry_check(const GraphQArgs& qa, const GQVariant& v, const char* who) {
  const GraphArgs& a = qa.g;
  if (qa.q_bits != 4 && qa.q_bits != 8 && qa.q_bits != 16) {
    gadmm_set_error("%s: q_bits must be 4, 8 or 16, got %d", who, qa.q_bits);
    return -1;
  }
  if (!v.fn) {
    gadmm_set_error("%s: d=%d, n=%d, max_degree=%d not eligible (1 <= d <= 64, n >= 2)", who, a.d, a.n, a.max_degree);
    return -1;
  }
  if (!a.nb_ptr || !a.nb_idx || !a.wid || !a.is_head || !a.Minv || !a.A || !a.b || !a.yy || !a.theta || !a.mu ||
      !qa.qg || !a.objg || !a.decg || !a.dec_push || !a.trace || !a.ctl) {
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

// ABI self-description of GraphQArgs (ctypes mirror in gadmm_amd/ops/native.py; gadmm_graph_abi_layout
// covers the GraphArgs it starts with).
int gadmm_graph_q_abi_layout(long long* out, int n) {
  long long v[] = {(long long)sizeof(GraphQArgs),           (long long)offsetof(GraphQArgs, g),
                   (long long)offsetof(GraphQArgs, qg),     (long long)offsetof(GraphQArgs, q_bits),
                   (long long)offsetof(GraphQArgs, q_seed), (long long)offsetof(GraphQArgs, q_true),
                   (long long)sizeof(GraphArgs)};
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n && i < k; ++i) out[i] = v[i];
  return k;
}

// Dynamic LDS bytes of a launch over n workers of maximum degree max_degree.
long gadmm_graph_persistent_q_lds(int n, int max_degree) { return graph_q_lds_doubles(n, max_degree) * 8; }

// The degree class (neighbours polled back to back, two granules each) the launch of `args` would take;
// 0: not eligible.
int gadmm_graph_persistent_q_class(const GraphQArgs* args) { return pick_graph_q_variant(*args).dk; }

// Workgroups the kernel for `args` (d, n, max_degree, q_bits) can keep resident (0: shape not eligible).
long gadmm_graph_persistent_q_capacity(const GraphQArgs* args) {
  const GQVariant v = pick_graph_q_variant(*args);
  if (!v.fn || v.shm > 65536) return 0;
  return gadmm_resident_capacity(v.fn, 64, v.shm);
}

// -1: malformed arguments (q_bits outside {4, 8, 16} among them); -2: refused (the staging does not fit
// in LDS, or the n + 1 workgroups cannot all be resident) -- either way before anything is launched, the
// reason in gadmm_set_error.
int gadmm_graph_persistent_q_launch(const GraphQArgs* args, hipStream_t st) {
  const GraphQArgs& qa = *args;
  const GraphArgs& a = qa.g;
  const GQVariant v = pick_graph_q_variant(qa);
  if (const int rc = graph_q_entry_check(qa, v, "persistent graph Q kernel")) return rc;
  const int blocks = a.n + 1;
  const long cap = gadmm_resident_capacity(v.fn, 64, v.shm);
  if (blocks > cap) {  // every workgroup must be resident together (they spin on each other)
    gadmm_set_error("persistent graph Q kernel: %d workgroups but only %ld can be resident", blocks, cap);
    return -2;
  }
  GraphQArgs ka = qa;
  ka.g.xcd = gadmm_xcd_pick(a.xcd, 0, blocks, cap, a.xchk);
  ka.g.xtag = (int)gadmm_next_xtag();  // fresh placement-check tag: no memset of xchk
  void* kargs[] = {&ka};
  GADMM_CHECK(hipLaunchKernel(v.fn, dim3(ka.g.xcd > 0 ? 8 * blocks : blocks), dim3(64), kargs, v.shm, st));
  GADMM_CHECK(hipGetLastError());
  return 0;
}

// Solves one launch of graph_persistent_q_sweep_kernel can run side by side (one per XCD).
int gadmm_graph_persistent_q_sweep_capacity() { return GRAPH_Q_SWEEP_CAPACITY; }

// nb <= 8 independent Q-GGADMM solves in ONE launch, as gadmm_graph_persistent_sweep_launch: one register
// class, every entry passes the single launch's checks, no two entries share a written buffer (the graph
// sweep's, plus the message table and the true iterates). -1 / -2 as there.
int gadmm_graph_persistent_q_sweep_launch(const GraphQArgs* batch, int nb, GraphQArgs* host_stage,
                                          GraphQArgs* dev_stage, hipStream_t st) {
  const char* name = "persistent graph Q sweep";
  if (!gadmm_sweep_batch_ok(name, batch, nb, GRAPH_Q_SWEEP_CAPACITY, host_stage, dev_stage)) return -1;
  int blocks[8], dk[8];
  size_t shm = 0;
  for (int j = 0; j < nb; ++j) {
    const GraphQArgs& qa = batch[j];
    const GraphArgs& a = qa.g;
    char who[48];
    snprintf(who, sizeof(who), "%s: solve %d", name, j);
    if ((a.d <= 52) != (batch[0].g.d <= 52)) {
      gadmm_set_error("%s: solves of different register classes (d = %d and %d; d <= 52 or 53..64)", name,
                      batch[0].g.d, a.d);
      return -1;
    }
    const GQVariant v = pick_graph_q_variant(qa);
    if (const int rc = graph_q_entry_check(qa, v, who)) return rc;
    if (!a.xchk) {
      gadmm_set_error("%s has no placement-check buffer (xchk)", who);
      return -1;
    }
    blocks[j] = a.n + 1;
    if (blocks[j] > XCHK) {
      gadmm_set_error("%s has %d workgroups, the placement check holds %d", who, blocks[j], XCHK);
      return -1;
    }
    for (int i = 0; i < j; ++i) {
      const GraphQArgs& o = batch[i];
      if (gadmm_graph_sweep_shares(a, o.g) || o.qg == qa.qg || (qa.q_true && o.q_true == qa.q_true)) {
        gadmm_set_error("%s: solves %d and %d share a buffer that both write", name, i, j);
        return -1;
      }
    }
    dk[j] = v.dk;
    if (v.shm > shm) shm = v.shm;
  }
  unsigned classes = gadmm_graph_sweep_classes(dk, nb);
  const void* fn = batch[0].g.d <= 52 ? (const void*)graph_persistent_q_sweep_kernel<13>
                                      : (const void*)graph_persistent_q_sweep_kernel<16>;
  return gadmm_sweep_launch_as<GraphQArgs>({fn, 64, shm, name, false}, batch, nb, blocks, host_stage, dev_stage, st,
                                           &classes);
}

}  // extern "C"
