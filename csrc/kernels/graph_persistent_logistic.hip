// Logistic GGADMM with the reference's inexact local solver (inner GD, logReg_GD.m) on any connected
// bipartite graph: the whole solve in one launch on one GPU, max(d, m) <= 64, one wave per worker (+ the
// monitor workgroup). The specification is gadmm_amd/algorithms/ggadmm.py (graph_admm_logistic).
//
// Protocol: graph_persistent.hip's, through persist_device.h / graph_poll.h -- one theta-granule row per
// worker, tags salted per launch, the monitor's decision of iteration it - lag read with the neighbours
// in ONE wait (wait_decision), a deadline on every spin (done = 4), XCD packing (place_block). As there,
// a worker never re-reads a neighbour's granule after its own publication: a tail's dual step and K4
// row, and a head's lazy dual (applied at the start of the next iteration), take the neighbours from the
// LDS staging area nbv[k * 64 + lane], i.e. the very values that fed the frozen shift; a head polls its
// tails once more at the exit for the dual step it still owes.
//
// The design is this kernel's own. A worker wave keeps its shard TWICE in VGPRs in the quad layout of
// quad_gemv.h, Xq for the margins z = X x and XTq for the gradient X^T v, as
// chain_persistent_logistic_kernel does: 8 QT doubles per lane, 208 VGPRs at QT = 13 (max(d, m) <= 52)
// and 256 at QT = 16 (53..64), before anything else. The linear graph kernel's 32-granule poll group (128
// more VGPRs in flight) does not fit beside that, so a poll group here is at most 8 neighbours: classes
// DK = 2, 4, 8, the launcher takes the smallest DK >= the graph's maximum degree, and a worker of larger
// degree walks its neighbours in groups of 8 from the id table in LDS. That is the right trade here and
// not in the linear kernel: a phase is max_inner DEPENDENT GEMV pairs, tens of microseconds, against
// about one microsecond for a poll.
//
// Per local solve the frozen shift s = mu + sum_k rho (x0 - theta_k) is formed ONCE from the staging
// area, in CSR order (ascending worker id), and lives in a register; the inner loop touches LDS only
// through the two quad_gemv stagings. Its arithmetic is the one-wave chain kernel's statement for
// statement: z, v with libm exp and the IEEE quotient, -gx + lam x + sh, x - step gr, __all(conv). The
// objective is taken at the new iterate as there (one more quad_gemv with Xq, softplus, two wave sums).
//
// Two-wave workers (the margins recursion of GADMM_LOGISTIC_ZREC) are not built here.
#include <stdio.h>
#include <stdlib.h>
#include <cstddef>
#include "gadmm_common.h"
#include "gadmm_graph.h"
#include "persist_device.h"
#include "persist_launch.h"
#include "quad_gemv.h"
#include "graph_poll.h"
#include "chain_device.h"

namespace {

using chain_dev::softplus;

constexpr int GL_MAX_DK = 8;  // the widest poll group (profiles/glogistic/resource_usage.txt: no scratch at 8)

// A sweep slot's GraphLogiArgs (graph_logistic_sweep_kernel below): written by the host before the launch
// and never by a kernel, so it is read like kernel arguments, through the constant address space
// (wave-uniform scalar loads), as GraphSweepArgs of graph_persistent.hip.
typedef __attribute__((address_space(4))) GraphLogiArgs GraphLogiSweepArgs;

// The persistent logistic GGADMM solve (described above) as a body shared by the single-solve and the
// sweep kernel, as graph_body of graph_persistent.hip.
// SWEEP: the body runs as one slot of graph_logistic_sweep_kernel: always 8-strided, this slot's blocks
// are blockIdx.x >> 3, and a block past the slot's own n + 1 leaves before the placement check, any
// barrier and any LDS flag (place_block_sweep). Everything the body reads or writes is named by the
// slot's own arguments, and the LDS layout is the slot's own (its n and max_degree) inside a dynamic
// allocation sized for the launch's largest.
// GA: GraphLogiArgs (the kernel's own argument) or GraphLogiSweepArgs (a slot's entry).
template <int QT, int DK, bool SWEEP, class GA>
__device__ __forceinline__ void graph_logistic_body(const GA& ga) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const auto& a = ga.g;
  const auto& g = ga.l;
  int* xflag = reinterpret_cast<int*>(lds);  // the placement verdict (xcd_verdict's LDS word)
  const int d = a.d, n = a.n, m = g.m;
  const int lane = threadIdx.x, qi = lane & 15, qc = lane >> 4;
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
  const double rho = a.rho, lam = g.lam, step = g.step;
  const bool inj = lane < d, ini = lane < m;
  double* st = lds + GFLAGS;             // quad GEMV staging (QSTAGE doubles)
  double* nbv = st + QSTAGE;             // neighbour k's theta at nbv[k * 64 + lane]
  int* ids = reinterpret_cast<int*>(nbv + (long)a.max_degree * 64);  // neighbour ids in CSR order
  for (int k = lane; k < deg; k += 64) ids[k] = a.nb_idx[p0 + k];
  lds_barrier();
  int off0[DK];
#pragma unroll
  for (int j = 0; j < DK; ++j) off0[j] = (j < deg ? a.nb_idx[p0 + j] : 0) * d * 16;  // wave-uniform

  const double* Xg = g.X + (long)w * m * d;
  double Xq[4][QT], XTq[4][QT];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const int row = qi + 16 * r, col = qc + 4 * t;
      Xq[r][t] = (row < m && col < d) ? Xg[(long)row * d + col] : 0.0;   // X[row][col]
      XTq[r][t] = (col < m && row < d) ? Xg[(long)col * d + row] : 0.0;  // X^T[row][col]
    }
  const double yv = ini ? g.Y[(long)w * m + lane] : 0.0;
  double th = inj ? a.theta[(long)w * d + lane] : 0.0;  // theta_n^{it-1}
  double mu = inj ? a.mu[(long)w * d + lane] : 0.0;
  for (int k = 0; k < deg; ++k) nbv[k * 64 + lane] = inj ? a.theta[(long)ids[k] * d + lane] : 0.0;
  int pending = 0;  // a head's dual step of the previous iteration is still to apply
  int stop_code = 0, stop_iter = 0, abort = 0, used = 0;

  int it = a.start_iter;
  int rs = a.start_iter % a.ring;
  for (;; ++it, rs = rs + 1 == a.ring ? 0 : rs + 1) {
    if (it > a.max_iter + a.lag) break;
    // -- the wait: the neighbours' theta (heads: tails' theta^{it-1}, nothing at start_iter; tails: heads'
    // theta^it) and the decision of iteration it - lag in one loop
    const bool need_nb = inj && (head ? it > a.start_iter : true);
    const unsigned tnb = make_tag(a.epoch, head ? it - 1 : it);
    int dslot = rs - a.lag;  // == (it - lag) % ring
    if (dslot < 0) dslot += a.ring;
    int code = 0, sj = 0;
    const int outcome = wait_decision<false, GADMM_POLL_SLEEP>(
        a, it, a.start_iter, dslot, deadline,
        [&]() { return need_nb ? poll_all<DK>(rth, off0, ids, deg, d, lane, tnb, nbv) : true; }, code, sj);
    if (outcome == 3) { abort = 1; break; }
    if (outcome == 2) {
      stop_code = code;
      stop_iter = sj;
      break;
    }
    // -- a head's lazy end-of-iteration dual, then the frozen proximal shift, both over the staged neighbours
    double sh = 0.0, x = 0.0;
    if (inj) {
      double mm = mu;
      if (head && pending) {
        for (int k = 0; k < deg; ++k) mm = mm + rho * (th - nbv[k * 64 + lane]);
        mu = mm;
      }
      double s = mm;
      for (int k = 0; k < deg; ++k) s = s + rho * (th - nbv[k * 64 + lane]);
      sh = s;
      x = th;
    }
    // -- inner GD (logReg_GD.m): registers and the two GEMV stagings only
    used = 0;
    for (int k = 0; k < g.max_inner; ++k) {
      const double z = quad_gemv<QT>(Xq, x, st);                // margins z_i = X[i,:] x
      const double sv = ini ? yv / (1.0 + exp(yv * z)) : 0.0;  // y_i / (1 + e^{y_i z_i})
      const double gx = quad_gemv<QT>(XTq, sv, st);            // (X^T s)_j
      bool conv = true;
      if (inj) {
        const double gr = -gx + lam * x + sh;
        const double xn = x - step * gr;
        conv = fabs(xn - x) < g.inner_tol;
        x = xn;
      }
      used = k + 1;
      if (__all(conv)) break;
    }
    // -- publish theta^it
    const unsigned tag = make_tag(a.epoch, it);
    if (inj) put_granule<false>(local, rth, (w * d + lane) * 16, tag, x);
    if (!head) {  // tails: every neighbour is this iteration's head -> dual step now, from the staged values
      double rp = 0.0;
      if (inj) {
        double mm = mu;
        for (int k = 0; k < deg; ++k) {
          const double tk = nbv[k * 64 + lane];
          mm = mm + rho * (x - tk);
          rp = fma(tk - x, tk - x, rp);
        }
        mu = mm;
      }
      if (a.rres) {  // K4 primal residual: the tail's edges (each edge has exactly one tail end)
        const double rsum = wave_sum_f64(rp);
        if (lane == 0 && it - 1 < a.max_iter) a.rres[(long)(it - 1) * n + w] = rsum;
      }
    } else {
      pending = 1;
    }
    th = x;
    // -- f_n(theta^it) = lam/2 |x|^2 + sum softplus(-y z) at the new iterate -> monitor
    const double z = quad_gemv<QT>(Xq, x, st);
    const double part = wave_sum_f64(ini ? softplus(-yv * z) : 0.0);
    const double xx = wave_sum_f64(inj ? x * x : 0.0);
    if (lane == 0) put_granule<false>(local, rob, (rs * n + w) * 16, tag, lam * 0.5 * xx + part);
  }

  // a head's dual step of the last iteration: its tails' theta^{last} (published, and final)
  if (head && pending && !abort) {
    const unsigned tl = make_tag(a.epoch, it - 1);
    for (int spin = 0;; ++spin) {
      bool nb = true;
      if (inj) nb = poll_all<DK>(rth, off0, ids, deg, d, lane, tl, nbv);
      if (__all(nb)) break;
      if ((spin & 7) == 7 && now_ticks() > deadline) { abort = 1; break; }
      GADMM_POLL_PAUSE();
    }
    if (!abort && inj)
      for (int k = 0; k < deg; ++k) mu = mu + rho * (th - nbv[k * 64 + lane]);
  }
  if (inj) {  // final state (plain stores; visible to the host after the kernel)
    a.theta[(long)w * d + lane] = th;
    a.mu[(long)w * d + lane] = mu;
  }
  if (lane == 0) {
    if (g.inner_iters) g.inner_iters[w] = used;
    post_outcome<false>(a.ctl, abort, bid, stop_code, stop_iter, it);
  }
}

template <int QT, int DK>
__global__ void __launch_bounds__(64) graph_logistic_kernel(GraphLogiArgs ga) {
  graph_logistic_body<QT, DK, false>(ga);
}

// Up to 8 independent logistic GGADMM solves in one launch, one per XCD: slot j = blockIdx.x & 7 runs
// solve j on the blocks b % 8 == j, i.e. on the blocks that the single-solve launch leaves as exiting
// spacers. batch[j] is solve j's own GraphLogiArgs: its own graph (CSR arrays, launch order), n, d, m, rho,
// lam, step, max_inner, inner_tol, stop rule, theta / mu, granule table, objective and decision rings, ctl,
// trace, tstamp, rres, inner_iters, xchk, tag salt and deadline; only the shards X, Y and the read-only CSR
// arrays may be shared. Slots may differ in n, d and m (within the QT class), graph and degree class:
// `classes` holds log2 of slot j's own DK (what pick_variant gives its single launch) in bits 4 j ..
// 4 j + 3, and the wave-uniform switch below sends the slot into the body of that class, so every slot
// executes the poll code of its own single solve (a chain member never runs a star's 8-wide poll group).
// The three bodies hold the shard in the same 16 QT VGPRs each; the kernel's registers are those of its
// widest body (profiles/glogistic_sweep/resource_usage.txt: no scratch). Nothing assumes WHICH XCD a
// slot gets (place_block_sweep): a slot publishes with plain stores only after its own blocks reported one
// XCC_ID under its own xtag, else with sc1 stores.
template <int QT>
__global__ void __launch_bounds__(64) graph_logistic_sweep_kernel(const GraphLogiArgs* __restrict__ batch, int nb,
                                                                  unsigned classes) {
  const int j = (int)(blockIdx.x & 7u);
  if (j >= nb) return;
  const GraphLogiSweepArgs& ga = *(const GraphLogiSweepArgs*)(batch + j);
  switch ((classes >> (4 * j)) & 15u) {
    case 1: graph_logistic_body<QT, 2, true>(ga); break;
    case 2: graph_logistic_body<QT, 4, true>(ga); break;
    default: graph_logistic_body<QT, GL_MAX_DK, true>(ga); break;
  }
}

#define GRAPH_LOGISTIC_SWEEP_CAPACITY 8

struct GLVariant {
  const void* fn = nullptr;
  size_t shm = 0;
  int dk = 0;
};

template <int QT>
const void* glogi_fn(int dk) {
  if (dk == 2) return (const void*)graph_logistic_kernel<QT, 2>;
  if (dk == 4) return (const void*)graph_logistic_kernel<QT, 4>;
  return (const void*)graph_logistic_kernel<QT, GL_MAX_DK>;
}

GLVariant pick_variant(const GraphLogiArgs& ga) {
  const GraphArgs& a = ga.g;
  GLVariant v;
  const int mx = a.d > ga.l.m ? a.d : ga.l.m;
  if (a.d < 1 || ga.l.m < 1 || mx > 64 || a.n < 2 || a.max_degree < 1 || a.max_degree >= a.n) return v;
  v.dk = 2;  // the smallest class that polls every neighbour of every worker in one group, at most 8
  while (v.dk < a.max_degree && v.dk < GL_MAX_DK) v.dk *= 2;
  // both copies of the shard in registers: QT = 13 covers max(d, m) <= 52, 16 covers 53..64
  v.fn = mx <= 52 ? glogi_fn<13>(v.dk) : glogi_fn<16>(v.dk);
  v.shm = (size_t)graph_lds_doubles(a.n, a.max_degree) * 8;
  return v;
}

// What the launch asks of its arguments, before residency: 0 fine, -1 malformed, -2 the staging does not
// fit in LDS. No HIP call.
int entry_check(const GraphLogiArgs& ga, const GLVariant& v, const char* who = "persistent graph logistic kernel") {
  const GraphArgs& a = ga.g;
  const LogiArgs& g = ga.l;
  if (!v.fn) {
    gadmm_set_error("%s: d=%d, m=%d, n=%d, max_degree=%d not eligible (1 <= d, m <= 64, n >= 2)", who, a.d, g.m, a.n,
                    a.max_degree);
    return -1;
  }
  if (!a.nb_ptr || !a.nb_idx || !a.wid || !a.is_head || !g.X || !g.Y || !a.theta || !a.mu || !a.thg || !a.objg ||
      !a.decg || !a.dec_push || !a.trace || !a.ctl) {
    gadmm_set_error("%s: a required buffer is null", who);
    return -1;
  }
  if (g.max_inner < 1) {
    gadmm_set_error("%s: max_inner=%d, at least one inner step", who, g.max_inner);
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

template <>
struct SweepSlot<GraphLogiArgs> {
  static int& xcd(GraphLogiArgs& a) { return a.g.xcd; }
  static int& xtag(GraphLogiArgs& a) { return a.g.xtag; }
  static void set_dbg(GraphLogiArgs&, int) {}
};

extern "C" {

// ABI self-description of GraphLogiArgs (ctypes mirror in gadmm_amd/ops/native.py).
int gadmm_graph_logistic_abi_layout(long long* out, int n) {
  long long v[] = {(long long)sizeof(GraphLogiArgs), (long long)offsetof(GraphLogiArgs, g),
                   (long long)offsetof(GraphLogiArgs, l), (long long)sizeof(GraphArgs), (long long)sizeof(LogiArgs)};
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n && i < k; ++i) out[i] = v[i];
  return k;
}

// Dynamic LDS bytes of a launch over n workers of maximum degree max_degree.
long gadmm_graph_logistic_lds(int n, int max_degree) { return graph_lds_doubles(n, max_degree) * 8; }

// The degree class (granules polled back to back: 2, 4 or 8) the launch of `args` would take; 0: not eligible.
int gadmm_graph_logistic_class(const GraphLogiArgs* args) { return pick_variant(*args).dk; }

// Workgroups the kernel for `args` (d, m, n, max_degree) can keep resident (0: shape not eligible).
long gadmm_graph_logistic_capacity(const GraphLogiArgs* args) {
  const GLVariant v = pick_variant(*args);
  if (!v.fn || v.shm > 65536) return 0;
  return gadmm_resident_capacity(v.fn, 64, v.shm);
}

// -1: malformed arguments; -2: refused (the staging does not fit in LDS, or the n + 1 workgroups cannot
// all be resident) -- either way before anything is launched, the reason in gadmm_set_error.
int gadmm_graph_logistic_launch(const GraphLogiArgs* args, hipStream_t st) {
  const GLVariant v = pick_variant(*args);
  if (const int rc = entry_check(*args, v)) return rc;
  const int blocks = args->g.n + 1;
  const long cap = gadmm_resident_capacity(v.fn, 64, v.shm);
  if (blocks > cap) {  // every workgroup must be resident together (they spin on each other)
    gadmm_set_error("persistent graph logistic kernel: %d workgroups but only %ld can be resident", blocks, cap);
    return -2;
  }
  GraphLogiArgs ka = *args;
  ka.g.xcd = gadmm_xcd_pick(args->g.xcd, 0, blocks, cap, args->g.xchk);
  ka.g.xtag = (int)gadmm_next_xtag();  // fresh placement-check tag: no memset of xchk
  void* kargs[] = {&ka};
  GADMM_CHECK(hipLaunchKernel(v.fn, dim3(ka.g.xcd > 0 ? 8 * blocks : blocks), dim3(64), kargs, v.shm, st));
  GADMM_CHECK(hipGetLastError());
  return 0;
}

// Solves one launch of graph_logistic_sweep_kernel can run side by side (one per XCD).
int gadmm_graph_logistic_sweep_capacity() { return GRAPH_LOGISTIC_SWEEP_CAPACITY; }

// nb <= 8 independent logistic GGADMM solves (one register class: max(d, m) <= 52 or 53..64; any graphs,
// each slot on the degree class of its own single launch) in ONE launch, solve j on the blocks b % 8 == j.
// Every entry passes the single launch's checks and names its own written buffers (gadmm_graph_sweep_shares
// on the GraphArgs parts, plus inner_iters) and a placement-check buffer. Dynamic LDS: the largest entry's.
// Staging buffers and the residency refusal (-2: the sum of the workgroups, or one solve's n + 1 past the
// CUs of an XCD): gadmm_sweep_launch_as. -1: refused before any HIP call.
int gadmm_graph_logistic_sweep_launch(const GraphLogiArgs* batch, int nb, GraphLogiArgs* host_stage,
                                      GraphLogiArgs* dev_stage, hipStream_t st) {
  const char* name = "persistent graph logistic sweep";
  if (!gadmm_sweep_batch_ok(name, batch, nb, GRAPH_LOGISTIC_SWEEP_CAPACITY, host_stage, dev_stage)) return -1;
  int blocks[GRAPH_LOGISTIC_SWEEP_CAPACITY], dk[GRAPH_LOGISTIC_SWEEP_CAPACITY];
  size_t shm = 0;
  const auto small = [](const GraphLogiArgs& s) { return (s.g.d > s.l.m ? s.g.d : s.l.m) <= 52; };
  for (int j = 0; j < nb; ++j) {
    const GraphArgs& a = batch[j].g;
    char who[56];
    snprintf(who, sizeof(who), "%s: solve %d", name, j);
    if (small(batch[j]) != small(batch[0])) {
      gadmm_set_error("%s: solves of different register classes (max(d, m) <= 52 or 53..64)", name);
      return -1;
    }
    const GLVariant v = pick_variant(batch[j]);
    if (const int rc = entry_check(batch[j], v, who)) return rc;
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
      if (gadmm_graph_sweep_shares(a, batch[i].g) ||
          (batch[j].l.inner_iters && batch[i].l.inner_iters == batch[j].l.inner_iters)) {
        gadmm_set_error("%s: solves %d and %d share a buffer that both write", name, i, j);
        return -1;
      }
    dk[j] = v.dk;
    if (v.shm > shm) shm = v.shm;
  }
  unsigned classes = gadmm_graph_sweep_classes(dk, nb);
  const void* fn = small(batch[0]) ? (const void*)graph_logistic_sweep_kernel<13>
                                   : (const void*)graph_logistic_sweep_kernel<16>;
  return gadmm_sweep_launch_as<GraphLogiArgs>({fn, 64, shm, name, false}, batch, nb, blocks, host_stage, dev_stage, st,
                                              &classes);
}

}  // extern "C"
