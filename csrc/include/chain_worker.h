// The chain worker of the persistent d <= 64 kernels, one wave with lane i owning coordinate i: its
// state, the two dual steps in the reference's order, the K4 residual row and the publication of
// theta^it. The wait and the stop epilogue around them are wait_decision / post_outcome
// (persist_device.h). Both Newton kernels are built from all of these; the logistic kernels and the
// Q-GADMM body take publish_theta / store_state only and keep the rest written out, because there a
// helper changes the register allocation (profiles/worker_protocol lists every site and its figures).
#pragma once
#include "persist_device.h"

namespace chain_worker {

// Which coordinate of which worker a lane owns: global worker w, local index li, chain neighbours
// left / right (-1: none); inj: lane < d.
struct LaneSlot {
  int lane, d, w, li, left, right;
  bool inj;
};

__device__ __forceinline__ LaneSlot lane_slot(const PhaseSlot& sl, int lane, int d) {
  return LaneSlot{lane, d, sl.gid, sl.li, sl.left, sl.right, lane < d};
}

// theta_n^{start-1}, the dual and the neighbours' theta^{start-1} (0 beyond d or the chain's end)
template <class PA>
__device__ __forceinline__ void load_state(const PA& a, const LaneSlot& k, double& th, double& mu, double& tl,
                                           double& tr) {
  th = k.inj ? a.theta[(long)k.w * k.d + k.lane] : 0.0;
  mu = k.inj ? a.mu[(long)k.li * k.d + k.lane] : 0.0;
  tl = (k.inj && k.left >= 0) ? a.theta[(long)k.left * k.d + k.lane] : 0.0;
  tr = (k.inj && k.right >= 0) ? a.theta[(long)k.right * k.d + k.lane] : 0.0;
}

// final state (plain stores; visible to the host after the kernel)
template <class PA>
__device__ __forceinline__ void store_state(const PA& a, const LaneSlot& k, double th, double mu) {
  if (k.inj) {
    a.theta[(long)k.w * k.d + k.lane] = th;
    a.mu[(long)k.li * k.d + k.lane] = mu;
  }
}

// What a worker waits for before iteration `it`: a head its tails' theta^{it-1} (nothing at the launch's
// first iteration: load_state has it), a tail its heads' theta^it. ra / rb: the table rows, -1: none.
struct NbWait {
  int ra, rb;
  unsigned tnb;
};

template <class PA>
__device__ __forceinline__ NbWait nb_wait(const PA& a, const LaneSlot& k, bool head, int it) {
  const bool need_nb = head ? it > a.start_iter : true;
  const int jnb = head ? it - 1 : it;
  return NbWait{need_nb ? k.left : -1, need_nb ? k.right : -1, make_tag(a.epoch, jnb)};
}

// One poll of both neighbours' granules (wait_decision's `poll`): tl / tr are rewritten by every poll
// and hold the neighbours' theta once all lanes return true.
template <bool SYS>
__device__ __forceinline__ bool load_neighbours(__amdgpu_buffer_rsrc_t rth, const LaneSlot& k, const NbWait& nw,
                                                double& tl, double& tr) {
  bool nb = true;
  if (k.inj) {
    if (nw.ra >= 0) nb &= load_granule<SYS>(rth, (nw.ra * k.d + k.lane) * 16, nw.tnb, &tl);
    if (nw.rb >= 0) nb &= load_granule<SYS>(rth, (nw.rb * k.d + k.lane) * 16, nw.tnb, &tr);
  }
  return nb;
}

// A head's lazy dual: the reference's end-of-iteration step of the previous iteration, applied once the
// tails' theta is known, in the reference's order: - rho (th_l - th), then + rho (th - th_r).
__device__ __forceinline__ void head_lazy_dual(const LaneSlot& k, double rho, double th, double tl, double tr,
                                               double& mu) {
  double mm = mu;
  if (k.left >= 0) mm = mm - rho * (tl - th);
  if (k.right >= 0) mm = mm + rho * (th - tr);
  mu = mm;
}

// A tail's dual step with the fresh heads, and row it - 1 of the K4 primal residual (PersistArgs::rres,
// nullable): the squared norm over the tail's two edges.
template <class PA>
__device__ __forceinline__ void tail_dual_residual(const PA& a, const LaneSlot& k, double rho, int it, double x,
                                                   double tl, double tr, double& mu) {
  double rp = 0.0;
  if (k.inj) {
    double mm = mu;
    if (k.left >= 0) mm = mm - rho * (tl - x);
    if (k.right >= 0) mm = mm + rho * (x - tr);
    mu = mm;
    if (k.left >= 0) rp = fma(tl - x, tl - x, rp);
    if (k.right >= 0) rp = fma(x - tr, x - tr, rp);
  }
  if (a.rres) {
    const double rs = wave_sum_f64(rp);
    if (k.lane == 0 && it - 1 < a.max_iter) a.rres[(long)(it - 1) * a.n + k.w] = rs;
  }
}

// Where theta^it goes besides the rank's own table: the tables of the (at most two) neighbours on
// other GPUs (PersistArgs::push, nullable).
struct ThetaPush {
  u32x4 *p0, *p1;
  __amdgpu_buffer_rsrc_t r0, r1;
};

template <class PA>
__device__ __forceinline__ ThetaPush push_targets(const PA& a, int bid) {
  ThetaPush t;
  t.p0 = a.push ? a.push[2 * bid] : nullptr;
  t.p1 = a.push ? a.push[2 * bid + 1] : nullptr;
  t.r0 = rsrc_of(t.p0 ? (const void*)t.p0 : (const void*)a.thg);
  t.r1 = rsrc_of(t.p1 ? (const void*)t.p1 : (const void*)a.thg);
  return t;
}

// Publish x = theta_w^it [lane]: own table first (the neighbours on this GPU wait for it), then p0, then p1.
template <bool SYS>
__device__ __forceinline__ void publish_theta(bool local, __amdgpu_buffer_rsrc_t rth, const ThetaPush& t,
                                              const LaneSlot& k, unsigned tag, double x) {
  if (!k.inj) return;
  put_granule<SYS>(local, rth, (k.w * k.d + k.lane) * 16, tag, x);
  if (t.p0) store_granule<SYS>(t.r0, (k.w * k.d + k.lane) * 16, tag, x);
  if (t.p1) store_granule<SYS>(t.r1, (k.w * k.d + k.lane) * 16, tag, x);
}

}  // namespace chain_worker
using namespace chain_worker;
