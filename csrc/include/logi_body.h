// The two worker bodies of the persistent inner-GD logistic GADMM solve for a slot of the sweep kernel
// (chain_logistic_sweep.hip: up to eight solves in one launch, one per XCD), templated on the slot's
// argument types. They are the sweep unit's OWN COPY of the loops of chain_persistent_logistic.hip,
// statement for statement, so a slot computes what its single launch computes bit for bit
// (tests/test_gpu_logistic_sweep.py). The single-solve kernels do not call them: built on one text shared
// with the sweep, seven of their eight instantiations kept VGPRs, AGPRs, SGPRs, scratch, LDS and occupancy
// (zrec<16, true>: 170 -> 174 AGPRs), and yet E3's single solve measured 5.100 against 4.995 ms for the
// parent's library in the same GPU call (three alternating rounds, spread 0.1 %), while a sweep of ONE on
// these bodies took 5.00 ms (profiles/logistic_sweep). So the kernels of chain_persistent_logistic.hip
// keep their own text; a change to either loop belongs in both. What the two units must agree on (block
// size, s ring, LDS size, the fast sigmoid) is logi_layout.h. What the kernels compute, the hand-off / stop
// protocol and the margins recursion are described in chain_persistent_logistic.hip. Here:
//   PA / GA  a sweep slot's PersistArgs / LogiArgs, read through the constant address space (SweepArgs
//            and the members of LogiSweepSlot: wave-uniform scalar loads)
//   one GPU, agent scope, every slot with its monitor (the launcher's checks); always 8-strided: this
//   slot's blocks are blockIdx.x >> 3, and a block past the slot's own n_local + 1 leaves before the
//   placement check and before any barrier or LDS flag (place_block_sweep). Everything a body reads or
//   writes is named by the slot's own arguments.
// Barriers of the two-wave body: the placement check's (xcd_verdict) and the one behind the control
// words' reset, both ahead of the monitor / wave split. Past them no wave meets a barrier again, so the
// margins wave may leave (quit, deadline) while the iterate wave works on; a block that leaves as a spacer
// has met none.
#pragma once
#include "gadmm_common.h"
#include "gadmm_chain.h"
#include "persist_device.h"
#include "chain_device.h"
#include "chain_worker.h"
#include "gadmm_logi.h"
#include "logi_layout.h"

// ------------------------------------------------------------------------------------------------
// One wave per worker (64 threads, LDS: QSTAGE doubles): bit-identical to the graph engine.
template <int T, class PA, class GA>
__device__ __forceinline__ void logi_onewave_body(const PA& a, const GA& g) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int d = a.d, n = a.n, m = g.m;
  const int lane = threadIdx.x, qi = lane & 15, qc = lane >> 4;
  const __amdgpu_buffer_rsrc_t rth = rsrc_of(a.thg);
  const __amdgpu_buffer_rsrc_t rob = rsrc_of(a.objg);
  const unsigned long long deadline = now_ticks() + (unsigned long long)a.timeout_ticks;
  __shared__ int xcd_lds;
  const Placement pl = place_block_sweep(a.xcd, a.xchk, (unsigned)a.xtag, a.n_local + 1, deadline, &xcd_lds, a.ctl);
  if (pl.spacer) return;
  const int bid = pl.bid;
  const bool local = pl.local;

  if (bid == a.n_local) {
    monitor_loop<false, 1>(a, lds, rob, deadline, a.start_iter, 0, nullptr, 0, 0);
    return;
  }

  // ------------------------------------------------------------------ worker (one wave)
  const PhaseSlot sl = a.slots[bid];
  const int li = sl.li, w = sl.gid, left = sl.left, right = sl.right;
  const bool head = (a.pos[bid] % 2) == 0;
  const LaneSlot ls = lane_slot(sl, lane, d);
  const double rho = a.rho, lam = g.lam, step = g.step;
  double* st = lds;  // QSTAGE doubles: quad GEMV staging
  const ThetaPush push = push_targets(a, bid);
  const double* Xg = g.X + (long)li * m * d;
  double Xq[4][T], XTq[4][T];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int row = qi + 16 * r, col = qc + 4 * t;
      Xq[r][t] = (row < m && col < d) ? Xg[(long)row * d + col] : 0.0;   // X[row][col]
      XTq[r][t] = (col < m && row < d) ? Xg[(long)col * d + row] : 0.0;  // X^T[row][col]
    }
  const bool inj = lane < d, ini = lane < m;
  const double yv = ini ? g.Y[(long)li * m + lane] : 0.0;
  // The worker's state, wait and dual steps below are load_state / wait_decision / head_lazy_dual /
  // tail_dual_residual (chain_worker.h, persist_device.h) written out: through the helpers this kernel's
  // register allocation changes, and through load_state or head_lazy_dual the compiler contracts one
  // multiply-add of the shift differently, so the trace is no longer the graph engine's bit for bit
  // (profiles/worker_protocol)
  double th = inj ? a.theta[(long)w * d + lane] : 0.0;  // theta_n^{i-1}
  double mu = inj ? a.mu[(long)li * d + lane] : 0.0;
  double tl = (inj && left >= 0) ? a.theta[(long)left * d + lane] : 0.0;
  double tr = (inj && right >= 0) ? a.theta[(long)right * d + lane] : 0.0;
  int pending = a.pending_in;
  int stop_code = 0, stop_iter = 0, abort = 0, used = 0;

  int it = a.start_iter;
  for (;; ++it) {
    if (it > a.max_iter + a.lag) break;
    // -- neighbours' theta (heads: tails' theta^{it-1}; tails: heads' theta^it) and the decision of
    // it - lag, polled in one loop
    const bool check = it - a.start_iter >= a.lag;
    const int jdec = it - a.lag;
    const bool need_nb = head ? it > a.start_iter : true;
    const int jnb = head ? it - 1 : it;
    const unsigned tnb = make_tag(a.epoch, jnb), tj = make_tag(a.epoch, jdec);
    const int ra = need_nb ? left : -1, rb = need_nb ? right : -1;
    bool decided = !check;
    unsigned long long dv = 0;
    int outcome = 0;  // 1 go, 2 stop, 3 timeout
    for (int spin = 0;; ++spin) {
      bool nb = true;
      if (inj) {
        if (ra >= 0) nb &= load_granule<false>(rth, (ra * d + lane) * 16, tnb, &tl);
        if (rb >= 0) nb &= load_granule<false>(rth, (rb * d + lane) * 16, tnb, &tr);
      }
      if (!decided) {
        dv = __shfl(load_dec<false>(&a.decg[jdec % a.ring]), 0, 64);
        decided = (unsigned)(dv >> 32) == tj;
      }
      if (decided && (unsigned)(dv & 0xffffffffu) != 0u) { outcome = 2; break; }
      if (decided && __all(nb)) { outcome = 1; break; }
      if ((spin & 7) == 7 && now_ticks() > deadline) { outcome = 3; break; }
      __builtin_amdgcn_s_sleep(1);
    }
    if (outcome != 1) {
      if (outcome == 2) {
        stop_code = (int)(unsigned)(dv & 0xffffffffu);
        stop_iter = jdec;
      } else {
        abort = 1;
      }
      break;
    }
    // -- lazy dual (heads), frozen proximal shift, inner GD (logReg_GD.m)
    double sh = 0.0, x = 0.0;
    if (inj) {
      double mm = mu;
      if (head && pending) {
        if (left >= 0) mm = mm - rho * (tl - th);
        if (right >= 0) mm = mm + rho * (th - tr);
        mu = mm;
      }
      double s = mm;  // -C1 + C2 (edge form) == mu
      if (left >= 0) s = s + rho * (th - tl);
      if (right >= 0) s = s + rho * (th - tr);
      sh = s;
      x = th;
    }
    used = 0;
    for (int k = 0; k < g.max_inner; ++k) {
      const double z = quad_gemv<T>(Xq, x, st);                 // margins z_i = X[i,:] x
      const double sv = ini ? yv / (1.0 + exp(yv * z)) : 0.0;  // y_i / (1 + e^{y_i z_i})
      const double gx = quad_gemv<T>(XTq, sv, st);             // (X^T s)_j
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
    // -- publish theta^it: own table + the remote neighbours' tables
    const unsigned tag = make_tag(a.epoch, it);
    publish_theta<false>(local, rth, push, ls, tag, x);
    if (!head) {  // tails: both neighbours are this iteration's heads -> dual update now
      double rp = 0.0;
      if (inj) {
        double mm = mu;
        if (left >= 0) mm = mm - rho * (tl - x);
        if (right >= 0) mm = mm + rho * (x - tr);
        mu = mm;
        if (left >= 0) rp = fma(tl - x, tl - x, rp);  // K4 primal residual of the two edges
        if (right >= 0) rp = fma(x - tr, x - tr, rp);
      }
      if (a.rres) {
        const double rs = wave_sum_f64(rp);
        if (lane == 0 && it - 1 < a.max_iter) a.rres[(long)(it - 1) * n + w] = rs;
      }
    } else {
      pending = 1;
    }
    th = x;
    // -- f_n(theta^it) = lam/2 |x|^2 + sum softplus(-y z) at the new iterate -> monitor
    const double z = quad_gemv<T>(Xq, x, st);
    const double part = wave_sum_f64(ini ? softplus(-yv * z) : 0.0);
    const double xx = wave_sum_f64(inj ? x * x : 0.0);
    if (lane == 0) put_granule<false>(local, rob, ((it % a.ring) * n + w) * 16, tag, lam * 0.5 * xx + part);
  }
  store_state(a, ls, th, mu);
  if (lane == 0) {
    if (g.inner_iters) g.inner_iters[li] = used;
    post_outcome(a.ctl, abort, bid, stop_code, stop_iter, it);
  }
}

// ------------------------------------------------------------------------------------------------
// Two waves per worker (ZR_NT threads): the margins recursion (chain_persistent_logistic.hip).
template <int T, class PA, class GA>
__device__ __forceinline__ void logi_zrec_body(const PA& a, const GA& g) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int d = a.d, n = a.n, m = g.m;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, qi = lane & 15, qc = lane >> 4;
  // worker LDS: [2][QSTAGE] per-wave GEMV staging | zc [2][64] (z_0, c) | s ring [8][4 QX] (each slot
  // in quad_gemv's x layout, read by the iterate wave's GEMV in place) | K [64][64] (row-major, built
  // once) | control ints
  double* st = lds + wv * QSTAGE;
  double* zc = lds + 2 * QSTAGE;
  double* sring = zc + 128;
  double* Kb = sring + ZR_SLOTS * 4 * QX;
  int* ctl = (int*)(Kb + 64 * 64);  // [0] start (solve id), [1] s produced, [2] s consumed, [3] solve end, [4] quit,
                                    // [5] c posted (solve id)
  const __amdgpu_buffer_rsrc_t rth = rsrc_of(a.thg);
  const __amdgpu_buffer_rsrc_t rob = rsrc_of(a.objg);
  const unsigned long long deadline = now_ticks() + (unsigned long long)a.timeout_ticks;
  __shared__ int xcd_lds;
  const Placement pl = place_block_sweep(a.xcd, a.xchk, (unsigned)a.xtag, a.n_local + 1, deadline, &xcd_lds, a.ctl);
  if (pl.spacer) return;
  const int bid = pl.bid;
  const bool local = pl.local;

  if (bid == a.n_local) {
    monitor_loop<false, 1>(a, lds, rob, deadline, a.start_iter, 0, nullptr, 0, wv);
    return;
  }

  const PhaseSlot sl = a.slots[bid];
  const int li = sl.li, w = sl.gid, left = sl.left, right = sl.right;
  const bool head = (a.pos[bid] % 2) == 0;
  const LaneSlot ls = lane_slot(sl, lane, d);
  const double rho = a.rho, lam = g.lam, step = g.step;
  const double* Xg = g.X + (long)li * m * d;
  const bool inj = lane < d, ini = lane < m;
  const double yv = ini ? g.Y[(long)li * m + lane] : 0.0;
  const bool post_fence = (a.dbg & (1 << 17)) != 0;
  if (threadIdx.x < 8) ctl[threadIdx.x] = 0;
  __syncthreads();

  if (wv == 1) {
    // ---------------------------------------------------------------- margins wave
    const bool zr_fast = (a.dbg & 32) == 0;  // GADMM_LOGISTIC_FASTSIGM=0: libm exp and IEEE divide (A/B)
    int sid = 0;
    for (;;) {  // one local solve per start
      int s0 = 0;
      for (int spin = 0;; ++spin) {
        s0 = lds_load_acq(&ctl[0]);
        if (s0 > sid || lds_load_acq(&ctl[4])) break;
        if ((spin & 63) == 63 && now_ticks() > deadline) return;
        __builtin_amdgcn_s_sleep(1);
      }
      if (s0 <= sid) return;  // quit
      sid = s0;
      static_assert(T <= 16, "quad layout");
      double Kq[4][T];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < T; ++t) Kq[r][t] = Kb[(qi + 16 * r) * 64 + qc + 4 * t];  // built by wave 0 before start 1
      double z = zc[lane];
      double cc = 0.0;
      const double decay = 1.0 - step * lam;
      bool ended = false;
      for (int k = 0; k < g.max_inner && !ended; ++k) {
        const double sv = ini ? (zr_fast ? zr_sigm(yv, z) : yv / (1.0 + exp(yv * z))) : 0.0;
        // z' = (1 - step lam) z - step c + step (K s): the part without K s is formed while the GEMV runs
        double zpart = fma(decay, z, -step * cc);
        if (k >= ZR_SLOTS - ZR_CHK && k % ZR_CHK == 0) {
          // slots of steps k .. k + ZR_CHK - 1 are free once steps <= k + ZR_CHK - 1 - ZR_SLOTS were read;
          // the iterate wave's end of the solve also ends this run-ahead
          for (int spin = 0;; ++spin) {
            if (lds_load_acq(&ctl[3]) == sid) { ended = true; break; }
            if (lds_load_acq(&ctl[2]) >= sid * 1024 + k + ZR_CHK - ZR_SLOTS) break;
            if ((spin & 63) == 63 && now_ticks() > deadline) return;
          }
          if (ended) break;
        }
        double* slot = sring + (k % ZR_SLOTS) * 4 * QX;
        slot[(lane & 3) * QX + (lane >> 2)] = sv;  // quad_gemv's x layout: both waves' GEMVs read it in place
        lds_post(&ctl[1], sid * 1024 + k + 1, post_fence);
        const double u = quad_gemv_staged<T>(Kq, slot);  // (K s)_i
        if (k == 0) {  // c = X sh arrives after z_0 (the iterate wave posts z_0 first)
          for (int spin = 0;; ++spin) {
            if (lds_load_acq(&ctl[5]) == sid) break;
            if ((spin & 63) == 63 && now_ticks() > deadline) return;
          }
          cc = zc[64 + lane];
          zpart = fma(decay, z, -step * cc);
        }
        z = ini ? fma(step, u, zpart) : 0.0;
      }
    }
  }

  // ------------------------------------------------------------------ iterate wave (wave 0)
  const ThetaPush push = push_targets(a, bid);
  double Xq[4][T], XTq[4][T];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int row = qi + 16 * r, col = qc + 4 * t;
      Xq[r][t] = (row < m && col < d) ? Xg[(long)row * d + col] : 0.0;
      XTq[r][t] = (col < m && row < d) ? Xg[(long)col * d + row] : 0.0;
    }
  // K = X X^T, column j = X (row j of X): m GEMVs into the row-major LDS image the margins wave loads
  for (int j = 0; j < m; ++j) {
    const double xr = inj ? Xg[(long)j * d + lane] : 0.0;
    const double kc = quad_gemv<T>(Xq, xr, st);
    Kb[lane * 64 + j] = ini ? kc : 0.0;
  }
  for (int j = m; j < 64; ++j) Kb[lane * 64 + j] = 0.0;
  // The worker's state, wait and dual steps below are load_state / wait_decision / head_lazy_dual /
  // tail_dual_residual (chain_worker.h, persist_device.h) written out: through any of the helpers this
  // kernel's register allocation changes (20 to 50 more values parked in AGPRs, profiles/worker_protocol)
  double th = inj ? a.theta[(long)w * d + lane] : 0.0;
  double mu = inj ? a.mu[(long)li * d + lane] : 0.0;
  double tl = (inj && left >= 0) ? a.theta[(long)left * d + lane] : 0.0;
  double tr = (inj && right >= 0) ? a.theta[(long)right * d + lane] : 0.0;
  int pending = a.pending_in;
  int stop_code = 0, stop_iter = 0, abort = 0, used = 0, sid = 0;

  int it = a.start_iter;
  for (;; ++it) {
    if (it > a.max_iter + a.lag) break;
    const bool check = it - a.start_iter >= a.lag;
    const int jdec = it - a.lag;
    const bool need_nb = head ? it > a.start_iter : true;
    const int jnb = head ? it - 1 : it;
    const unsigned tnb = make_tag(a.epoch, jnb), tj = make_tag(a.epoch, jdec);
    const int ra = need_nb ? left : -1, rb = need_nb ? right : -1;
    bool decided = !check;
    unsigned long long dv = 0;
    int outcome = 0;
    for (int spin = 0;; ++spin) {
      bool nb = true;
      if (inj) {
        if (ra >= 0) nb &= load_granule<false>(rth, (ra * d + lane) * 16, tnb, &tl);
        if (rb >= 0) nb &= load_granule<false>(rth, (rb * d + lane) * 16, tnb, &tr);
      }
      if (!decided) {
        dv = __shfl(load_dec<false>(&a.decg[jdec % a.ring]), 0, 64);
        decided = (unsigned)(dv >> 32) == tj;
      }
      if (decided && (unsigned)(dv & 0xffffffffu) != 0u) { outcome = 2; break; }
      if (decided && __all(nb)) { outcome = 1; break; }
      if ((spin & 7) == 7 && now_ticks() > deadline) { outcome = 3; break; }
      __builtin_amdgcn_s_sleep(1);
    }
    if (outcome != 1) {
      if (outcome == 2) {
        stop_code = (int)(unsigned)(dv & 0xffffffffu);
        stop_iter = jdec;
      } else {
        abort = 1;
      }
      break;
    }
    double sh = 0.0, x = 0.0;
    if (inj) {
      double mm = mu;
      if (head && pending) {
        if (left >= 0) mm = mm - rho * (tl - th);
        if (right >= 0) mm = mm + rho * (th - tr);
        mu = mm;
      }
      double s = mm;
      if (left >= 0) s = s + rho * (th - tl);
      if (right >= 0) s = s + rho * (th - tr);
      sh = s;
      x = th;
    }
    // margins wave: z_0 = X x_0 and c = X sh, then go
    const double z0 = quad_gemv<T>(Xq, x, st);
    zc[lane] = ini ? z0 : 0.0;
    ++sid;
    lds_store_rel(&ctl[0], sid);  // the margins wave starts from z_0 ...
    const double c0 = quad_gemv<T>(Xq, sh, st);
    zc[64 + lane] = ini ? c0 : 0.0;
    lds_store_rel(&ctl[5], sid);  // ... and needs c only after its first K s
    used = 0;
    for (int k = 0; k < g.max_inner; ++k) {
      const int want = sid * 1024 + k + 1;
      bool got = false;
      for (int spin = 0;; ++spin) {
        if (lds_load_acq(&ctl[1]) >= want) { got = true; break; }
        if ((spin & 63) == 63 && now_ticks() > deadline) break;
      }
      if (!got) { abort = 1; break; }
      const double gx = quad_gemv_staged<T>(XTq, sring + (k % ZR_SLOTS) * 4 * QX);
      lds_post(&ctl[2], want, post_fence);  // (after this GEMV's reads of the slot, LDS in order)
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
    lds_store_rel(&ctl[3], sid);  // this solve is over: the margins wave stops its run-ahead
    if (abort) break;
    const unsigned tag = make_tag(a.epoch, it);
    publish_theta<false>(local, rth, push, ls, tag, x);
    if (!head) {
      double rp = 0.0;
      if (inj) {
        double mm = mu;
        if (left >= 0) mm = mm - rho * (tl - x);
        if (right >= 0) mm = mm + rho * (x - tr);
        mu = mm;
        if (left >= 0) rp = fma(tl - x, tl - x, rp);
        if (right >= 0) rp = fma(x - tr, x - tr, rp);
      }
      if (a.rres) {
        const double rs = wave_sum_f64(rp);
        if (lane == 0 && it - 1 < a.max_iter) a.rres[(long)(it - 1) * n + w] = rs;
      }
    } else {
      pending = 1;
    }
    th = x;
    const double z = quad_gemv<T>(Xq, x, st);
    const double part = wave_sum_f64(ini ? softplus(-yv * z) : 0.0);
    const double xx = wave_sum_f64(inj ? x * x : 0.0);
    if (lane == 0) put_granule<false>(local, rob, ((it % a.ring) * n + w) * 16, tag, lam * 0.5 * xx + part);
  }
  lds_store_rel(&ctl[4], 1);  // the margins wave leaves
  store_state(a, ls, th, mu);
  if (lane == 0) {
    if (g.inner_iters) g.inner_iters[li] = used;
    post_outcome(a.ctl, abort, bid, stop_code, stop_iter, it);
  }
}
