// Q-GADMM (Elgabli et al., arXiv:1910.10453) on the chain engine: quantized neighbour exchange.
//
// Every worker n has a public model th_hat_n that its chain neighbours hold an identical copy of.
// After its solve the worker sends the stochastically quantized difference theta_n - th_hat_n at
// q_bits per coordinate, as (R, codes), and sender and receivers move th_hat_n by the same
// dequantized step (quant_device.h; the specification is gadmm_amd/algorithms/quantize.py). A
// closed-form GADMM solve never reads the worker's own previous theta, so the algorithm is GADMM
// whose theta table holds th_hat: rhs and duals read th_hat of the neighbours (and of the worker
// itself for the duals), the objective and the stop rule read the true theta.
//
// Two kernel families, the same arithmetic in the same order (bit-identical iterates, as the unquantized
// engines: symv_cols / quad_gemv sum in one order):
//   chain_phase_linear_q     one GADMM phase of the graph engine, d <= 256 (body of chain_phase_linear
//                            + the quantize stage): th_hat goes into the theta table.
//   chain_persistent_q_kernel  the whole solve in one launch, d <= 64, one wave per worker, static
//                            chain, one GPU: the hand-off is the packed message itself.
//   chain_persistent_q_sweep_kernel  up to 8 such solves in one launch, one per XCD (the same body).
//
// CQ-GADMM (censoring, Ben Issaid et al., arXiv:2009.06459, on top of the quantizer): a worker transmits
// only when its public model would move by at least a geometrically decaying threshold,
// s = sum_i (cand_i - th_hat_i)^2 >= c_thr2[it] (the table comes from the host: no powers here; s is
// summed in the order of wave_sum_f64 / block_sum_f64, which the specification's sum64 reproduces; the
// persistent kernel runs that butterfly through permlane swaps and DPP, wave_sum_f64_dpp).
// A censored worker keeps its public model and its neighbours keep their copies. Every body below has a
// compile-time CENS parameter; CENS = false are the Q kernels above, their code untouched, CENS = true
// the entry points
//   chain_phase_linear_cq, chain_persistent_cq_kernel, chain_persistent_cq_sweep_kernel
// with their own launchers and capacity functions, instantiated in a translation unit of their own
// (chain_cquant.hip includes this file). With an all-zero threshold table they compute Q-GADMM bit for
// bit (a mixed sweep runs its uncensored members that way).
#define GADMM_POLL_SLEEP 0  // one hand-off wait per phase on the critical path: poll back to back
#include <stdio.h>
#include <stdlib.h>
#include <cstddef>
#include "gadmm_common.h"
#include "gadmm_chain.h"
#include "chain_device.h"
#include "persist_device.h"
#include "chain_worker.h"
#include "persist_launch.h"
#include "quad_gemv.h"
#include "quant_device.h"

using namespace quant;

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;

__device__ __forceinline__ double block_max_f64(double v, double* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = wave_max_f64(v);
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  double t = scratch[0];
  for (int i = 1; i < nw; ++i) t = fmax(t, scratch[i]);
  return t;
}

// One term of the censoring sum: (cand - hat)^2 as two separately rounded operations (the
// specification's step and sq lines; no FMA may form with the additions of the sum that follows).
__device__ __forceinline__ double c_step_sq(double cand, double hat) {
#pragma clang fp contract(off)
  const double step = cand - hat;
  return step * step;
}

// wave_sum_f64's butterfly, x <- x + x[i ^ off] for off = 32, 16, 8, 4, 2, 1 (the specification's sum64;
// an addition gives the same bits with its operands either way round), without its six ds_bpermute round
// trips: the halves and the rows meet through the permlane swaps, lanes inside a row through DPP
// (0x128 = row_ror:8 = i ^ 8; row_half_mirror then quad_perm [3,2,1,0] = i ^ 4; 0x4E, 0xB1 = i ^ 2, i ^ 1).
// Every lane must be active.
__device__ __forceinline__ double wave_sum_f64_dpp(double v) {
  double a = v, b = v;
  swap32_f64(a, b);  // a = (lanes 0-31 twice), b = (lanes 32-63 twice)
  v = a + b;
  a = v;
  b = v;
  swap16_f64(a, b);  // a = (r0, r0, r2, r2), b = (r1, r1, r3, r3)
  v = a + b;
  v = v + dpp_f64<0x128>(v);
  v = v + dpp_f64<0x1B>(dpp_f64<0x141>(v));
  v = v + dpp_f64<0x4E>(v);
  v = v + dpp_f64<0xB1>(v);
  return v;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Graph engine: one GADMM phase with quantized publication. CENS: the censoring decision after the
// quantize stage (chain_phase_linear_cq); false: the Q kernel.
template <int NC, bool CENS>
__device__ __forceinline__ void phase_linear_q_body(const PhaseArgs& a) {
  __shared__ __attribute__((aligned(16))) double sh_r[64 * NC];
  __shared__ __attribute__((aligned(16))) double sh_t[64 * NC];  // the true theta of this solve
  __shared__ __attribute__((aligned(16))) double sh_q[64 * NC];
  __shared__ __attribute__((aligned(16))) double sh_h[64 * NC];  // the new public model th_hat
  __shared__ __attribute__((aligned(16))) double red[NW * 64 * NC];
  __shared__ unsigned sh_c[64 * NC];                             // the codes
  __shared__ double scratch[NW];
  __shared__ int flag_lds;
  ChainCtl* ctl = a.ctl;
  if (ctl->done) return;
  const int it = ctl->iter;
  const int pending = ctl->pending;
  const PhaseSlot sl = a.slots[blockIdx.x];
  const int d = a.d;
  const double rho = a.rho;
  double* th = a.theta;  // rows are th_hat
  const double* thw = th + (long)sl.gid * d;
  const double* thl = sl.left >= 0 ? th + (long)sl.left * d : nullptr;
  const double* thr = sl.right >= 0 ? th + (long)sl.right * d : nullptr;
  double* mu = a.mu + (long)sl.li * d;
  const double* b = a.b + (long)sl.li * d;
  const int deg = (thl != nullptr) + (thr != nullptr);

  for (int j = threadIdx.x; j < d; j += NT) {
    double m = mu[j];
    if ((a.flags & PH_PRE_DUAL) && pending) {
      if (thl) m = m - rho * (thl[j] - thw[j]);
      if (thr) m = m + rho * (thw[j] - thr[j]);
      mu[j] = m;
    }
    double r = b[j] - m;
    if (thl) r = r + rho * thl[j];
    if (thr) r = r + rho * thr[j];
    sh_r[j] = r;
  }
  __syncthreads();
  const double* Mi = a.Minv + ((long)sl.li * a.nvar + a.deg_to_var[deg]) * (long)d * d;
  symv_cols<NC, NT>(Mi, sh_r, sh_t, red, d);

  // -- quantize stage: R = max |theta - th_hat|, then per coordinate draw, code and th_hat update
  const int bits = a.q_bits;
  const double L = (double)((1u << bits) - 1u);
  double dmax = 0.0;
  for (int j = threadIdx.x; j < d; j += NT) dmax = fmax(dmax, fabs(sh_t[j] - thw[j]));
  const double R = block_max_f64(dmax, scratch);
  for (int j = threadIdx.x; j < d; j += NT) {
    const double hat = thw[j];
    const unsigned q = q_code(sh_t[j] - hat, R, L, q_u01(a.q_seed, it, a.n_total, sl.gid, d, j));
    sh_c[j] = q;
    sh_h[j] = q_apply(hat, R, L, q);
  }
  [[maybe_unused]] bool send = true;
  if constexpr (CENS) {
    // d <= 256 = NT: one coordinate per thread, so wave w holds the 64-chunk w of sq and block_sum_f64
    // adds the chunks' butterfly sums in order (the specification's sum64)
    const int j = threadIdx.x;
    const double sq = j < d ? c_step_sq(sh_h[j], thw[j]) : 0.0;
    const double s = block_sum_f64(sq, scratch);
    send = s >= a.c_thr2[it];
    if (!send && j < d) sh_h[j] = thw[j];  // censored: the old public row goes back (own entry, own write)
    if (threadIdx.x == 0 && it - 1 < a.max_iter) a.c_sent[(long)(it - 1) * a.n_total + sl.gid] = send ? 1 : 0;
  }
  __syncthreads();
  if constexpr (CENS) {  // a censored message is its header alone
    if (!send && a.q_msg && threadIdx.x == 0) a.q_msg[(long)sl.gid * (q_words(d, bits) + 1)] = Q_CENSORED;
  }
  if (CENS ? (send && a.q_msg) : (a.q_msg != nullptr)) {  // the message as it would travel: the bits of R, then 64 / bits codes per word
    const int lp = q_log2_per(bits), nw = q_words(d, bits);
    unsigned long long* msg = a.q_msg + (long)sl.gid * (nw + 1);
    if (threadIdx.x == 0) msg[0] = (unsigned long long)__double_as_longlong(R);
    for (int k = threadIdx.x; k < nw; k += NT) {
      unsigned long long wv = 0ull;
      for (int e = 0; e < (1 << lp); ++e) {
        const int i = (k << lp) + e;
        if (i < d) wv |= (unsigned long long)sh_c[i] << (bits * e);
      }
      msg[1 + k] = wv;
    }
  }
  double* thw_out = th + (long)sl.gid * d;
  double rpart = 0.0;
  for (int j = threadIdx.x; j < d; j += NT) {
    const double t = sh_h[j];
    thw_out[j] = t;
    if (a.q_true) a.q_true[(long)sl.li * d + j] = sh_t[j];
    if (a.flags & PH_POST_DUAL) {
      double m = mu[j];
      if (thl) m = m - rho * (thl[j] - t);
      if (thr) m = m + rho * (t - thr[j]);
      mu[j] = m;
      if (a.rres) {  // K4 primal residual of the tail's two edges (public models)
        if (thl) rpart = fma(thl[j] - t, thl[j] - t, rpart);
        if (thr) rpart = fma(t - thr[j], t - thr[j], rpart);
      }
    }
  }
  if (a.rres && (a.flags & PH_POST_DUAL)) {
    const double rs = block_sum_f64(rpart, scratch);
    if (threadIdx.x == 0 && it - 1 < a.max_iter) a.rres[(long)(it - 1) * a.n_total + sl.gid] = rs;
    __syncthreads();  // scratch is reused by the objective's block sum
  }
  if (a.flags & PH_OBJ) {  // the objective of the TRUE theta, still in LDS
    symv_cols<NC, NT>(a.A + (long)sl.li * d * d, sh_t, sh_q, red, d);
    double part = 0.0;
    for (int j = threadIdx.x; j < d; j += NT) part += (0.5 * sh_q[j] - b[j]) * sh_t[j];
    const double f = block_sum_f64(part, scratch) + 0.5 * a.yy[sl.li];
    if (threadIdx.x == 0) a.objw[sl.li] = f;
  }
  if (a.flags & PH_FINISH) {
    if (phase_arrive(ctl, a.n_slots, &flag_lds)) finish_iteration(a, it);
  }
}

template <int NC>
__global__ void __launch_bounds__(NT) chain_phase_linear_q(PhaseArgs a) {
  phase_linear_q_body<NC, false>(a);
}

template <int NC>
__global__ void __launch_bounds__(NT) chain_phase_linear_cq(PhaseArgs a) {
  phase_linear_q_body<NC, true>(a);
}

#ifndef GADMM_CQ_TU
extern "C" int gadmm_chain_phase_cquant(const PhaseArgs* args, hipStream_t st);
extern "C" int gadmm_chain_phase_quant(const PhaseArgs* args, hipStream_t st) {
  const PhaseArgs& a = *args;
  if (a.n_slots <= 0) return 0;
  if (a.model != MODEL_LINEAR || a.d > 256 || a.d < 1) {
    gadmm_set_error("chain_phase (quantized): the linear model with d <= 256 only (model %d, d=%d)", a.model, a.d);
    return -1;
  }
  if (a.q_bits != 4 && a.q_bits != 8 && a.q_bits != 16) {
    gadmm_set_error("chain_phase (quantized): q_bits must be 4, 8 or 16, got %d", a.q_bits);
    return -1;
  }
  if (a.c_thr2) return gadmm_chain_phase_cquant(args, st);  // CQ-GADMM: the censored kernel (chain_cquant.hip)
  const int nc = (a.d + 63) / 64;
  switch (nc) {
    case 1: hipLaunchKernelGGL(chain_phase_linear_q<1>, dim3(a.n_slots), dim3(NT), 0, st, a); break;
    case 2: hipLaunchKernelGGL(chain_phase_linear_q<2>, dim3(a.n_slots), dim3(NT), 0, st, a); break;
    default: hipLaunchKernelGGL(chain_phase_linear_q<4>, dim3(a.n_slots), dim3(NT), 0, st, a); break;
  }
  GADMM_CHECK(hipGetLastError());
  return 0;
}
#else
extern "C" int gadmm_chain_phase_cquant(const PhaseArgs* args, hipStream_t st) {  // checked by gadmm_chain_phase_quant
  const PhaseArgs& a = *args;
  if (!a.c_thr2 || !a.c_sent) {
    gadmm_set_error("chain_phase (censored): needs a threshold table (c_thr2) and a c_sent buffer");
    return -1;
  }
  const int nc = (a.d + 63) / 64;
  switch (nc) {
    case 1: hipLaunchKernelGGL(chain_phase_linear_cq<1>, dim3(a.n_slots), dim3(NT), 0, st, a); break;
    case 2: hipLaunchKernelGGL(chain_phase_linear_cq<2>, dim3(a.n_slots), dim3(NT), 0, st, a); break;
    default: hipLaunchKernelGGL(chain_phase_linear_cq<4>, dim3(a.n_slots), dim3(NT), 0, st, a); break;
  }
  GADMM_CHECK(hipGetLastError());
  return 0;
}
#endif

// ------------------------------------------------------------------------------------------------
// Persistent single-launch Q-GADMM: static chain, one GPU, d <= 64, one wave per worker (+ the
// monitor workgroup). Schedule, lagged stop rule, deadlines (done = 4) and XCD packing are those of
// chain_persistent_kernel (REG variant); inverse and Gram sit in VGPRs in the quad layout.
//
// Hand-off: worker w publishes iteration `it` as G = ceil(d bits / 64) + 1 tagged 16-byte granules
// in row w of the message table qg: granule 0 the bits of R, granule 1 + k code word k (64 / bits
// codes, coordinate i at bit bits (i mod 64/bits) of word i / (64/bits)). Payloads travel as raw bits.
// A receiver keeps th_hat of both neighbours in registers: lane i loads granule 0 and the granule of
// its code and applies q_apply, the function the sender applied to its own th_hat.
//
// The table has ONE slot per worker although a message is a DIFFERENCE that must be consumed exactly
// once: with a static chain a producer cannot publish iteration it + 1 before it has read the
// consumer's next message (a tail needs its heads' theta^{it+1}, a head its tails' theta^{it}), and a
// consumer publishes that message only after it has left the wait in which it read -- and kept in
// registers -- the producer's message `it`. The granules are applied once, after the wait (a poll
// that sees one neighbour's message early reloads it unchanged).
//
// CENS (chain_persistent_cq_kernel): the header granule is published EVERY iteration with that
// iteration's tag; a censored header carries Q_CENSORED (the sign bit: no R >= 0 has it) and the worker
// writes no code granule. A receiver leaves its wait when the header's tag matches AND either the header
// says censored or its code granule's tag matches too: it never waits on a code granule of a censored
// message and never applies one (those granules still hold an older tag and older codes); hl / hr then
// stay as they are. The one-slot argument above still holds, because a header IS a message: a producer
// cannot publish the header of iteration it + 1 before it has read the consumer's next header, which
// the consumer publishes only after it has left the wait in which it read the producer's header `it`
// (and, when that was not censored, the code granules of the same tag). A protocol mistake would end
// at the deadline (outcome 3, done = 4), not in an endless spin.
// (put_raw / raw_bits, the raw tagged granule of this hand-off: quant_device.h.)

// The persistent Q solve (described above) as a body shared by the single-solve and the sweep kernel.
// SWEEP: the body runs as one slot of chain_persistent_q_sweep_kernel (below): always 8-strided, this
// slot's blocks are blockIdx.x >> 3, and a block past the slot's own n_local + 1 leaves before the
// placement check and before any barrier (place_block_sweep). Everything the body reads or writes is
// named by the slot's own arguments.
// PA: PersistArgs (the kernel's own argument) or SweepArgs (a slot's entry, read through the constant
// address space: wave-uniform scalar loads, like the kernarg segment).
__device__ __forceinline__ bool hdr_censored(const u32x4& g) { return (g.w >> 31) != 0u; }

template <int QT, bool SWEEP, bool CENS, class PA>
__device__ __forceinline__ void q_persistent_body(const PA& a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int abort_lds;
  __shared__ int stop_lds;
  __shared__ int xcd_lds;
  const int d = a.d, n = a.n;
  const int lane = threadIdx.x;
  const __amdgpu_buffer_rsrc_t rq = rsrc_of(a.qg);
  const __amdgpu_buffer_rsrc_t rob = rsrc_of(a.objg);
  const unsigned long long deadline = now_ticks() + (unsigned long long)a.timeout_ticks;
  Placement pl;
  if constexpr (SWEEP) pl = place_block_sweep(a.xcd, a.xchk, (unsigned)a.xtag, a.n_local + 1, deadline, &xcd_lds, a.ctl);
  else pl = place_block<false>(a.xcd, a.xchk, (unsigned)a.xtag, a.n_local + 1, deadline, &xcd_lds, a.ctl);
  if (pl.spacer) return;
  const int bid = pl.bid;
  const bool local = pl.local;
  if (lane == 0) {
    abort_lds = 0;
    stop_lds = 0;
  }
  lds_barrier();

  if (bid == a.n_local) {
    monitor_loop<false, GADMM_POLL_SLEEP>(a, lds, rob, deadline, a.start_iter, 0, nullptr, 0, 0);
    return;
  }

  // ------------------------------------------------------------------ worker workgroup (one wave)
  const PhaseSlot sl = a.slots[bid];
  const int pos = a.pos[bid];
  const int li = sl.li, w = sl.gid;
  const int left = sl.left, right = sl.right;
  const bool head = (pos % 2) == 0;
  const LaneSlot ls = lane_slot(sl, lane, d);
  const int deg = (left >= 0) + (right >= 0);
  const double rho = a.rho;
  const int bits = a.q_bits, lp = q_log2_per(bits);
  const int G = q_words(d, bits) + 1;
  const double L = (double)((1u << bits) - 1u);
  const unsigned qmask = (1u << bits) - 1u;
  const int my_g = 1 + (lane >> lp);                 // the granule that holds this lane's code
  const int my_sh = bits * (lane & ((1 << lp) - 1));  // ... at this bit
  const bool in = lane < d;
  double* st = lds;  // quad GEMV staging (QSTAGE doubles)

  double Mq[4][QT], Aq[4][QT];
  quad_load<QT>(Mq, a.Minv + ((long)li * a.nvar + a.deg_to_var[deg]) * (long)d * d, d, true);
  quad_load<QT>(Aq, a.A + (long)li * d * d, d, true);
  // lane i owns coordinate i: the true theta, the worker's own public model and its copies of the
  // neighbours' (the theta table holds public models)
  double th = in ? a.theta[(long)w * d + lane] : 0.0;
  double hat = th;
  double mu = in ? a.mu[(long)li * d + lane] : 0.0;
  const double bb = in ? a.b[(long)li * d + lane] : 0.0;
  double hl = (in && left >= 0) ? a.theta[(long)left * d + lane] : 0.0;
  double hr = (in && right >= 0) ? a.theta[(long)right * d + lane] : 0.0;
  const double half_yy = 0.5 * a.yy[li];
  int pending = (a.pending_in && head) ? 1 : 0;
  int stop_code = 0, stop_iter = 0;
  lds_barrier();

  int it = a.start_iter;
  int rs = a.start_iter % a.ring;
  for (;; ++it, rs = rs + 1 == a.ring ? 0 : rs + 1) {
    if (it > a.max_iter + a.lag) break;
    const double u = q_u01(a.q_seed, it, n, w, d, lane);  // this iteration's draw: ready before the wait ends
    double thr2 = 0.0;
    if constexpr (CENS) thr2 = a.c_thr2[it];  // wave-uniform, issued here: off the dependent chain after the GEMV
    // -- stop rule: the decision of iteration it - lag, polled in the same loop as the neighbours'
    // messages; a stop decision abandons the wait (a neighbour that saw it publishes no more)
    // (wait_decision of persist_device.h written out, as are the dual steps of chain_worker.h below:
    // through the helpers two more values of this kernel are parked in AGPRs, and the single solve
    // measured 2 % slower, profiles/worker_protocol)
    const bool check = it - a.start_iter >= a.lag;
    const int jdec = it - a.lag;
    const bool need_nb = head ? it > a.start_iter : true;
    const int jnb = head ? it - 1 : it;
    const unsigned tnb = make_tag(a.epoch, jnb);
    const int ra = need_nb ? left : -1, rb = need_nb ? right : -1;
    int dslot = rs - a.lag;  // == jdec % ring
    if (dslot < 0) dslot += a.ring;
    const unsigned tj = make_tag(a.epoch, jdec);
    bool decided = !check;
    unsigned long long dv = 0;
    int outcome = 0;  // 1 go, 2 stop, 3 timeout
    u32x4 gRa = {0u, 0u, 0u, 0u}, gWa = gRa, gRb = gRa, gWb = gRa;
    for (int spin = 0;; ++spin) {
      bool nb = true;
      if (in) {
        if (ra >= 0) {
          gRa = load_raw<false>(rq, (ra * G) * 16);
          gWa = load_raw<false>(rq, (ra * G + my_g) * 16);
          if constexpr (CENS) nb &= granule_ok(gRa, tnb) && (hdr_censored(gRa) || granule_ok(gWa, tnb));
          else nb &= granule_ok(gRa, tnb) && granule_ok(gWa, tnb);
        }
        if (rb >= 0) {
          gRb = load_raw<false>(rq, (rb * G) * 16);
          gWb = load_raw<false>(rq, (rb * G + my_g) * 16);
          if constexpr (CENS) nb &= granule_ok(gRb, tnb) && (hdr_censored(gRb) || granule_ok(gWb, tnb));
          else nb &= granule_ok(gRb, tnb) && granule_ok(gWb, tnb);
        }
      }
      if (!decided) {
        dv = __shfl(load_dec<false>(&a.decg[dslot]), 0, 64);
        decided = (unsigned)(dv >> 32) == tj;
      }
      if (decided && (unsigned)(dv & 0xffffffffu) != 0u) { outcome = 2; break; }
      if (decided && __all(nb)) { outcome = 1; break; }
      if ((spin & 7) == 7 && now_ticks() > deadline) { outcome = 3; break; }
      GADMM_POLL_PAUSE();
    }
    if (lane == 0) {
      if (outcome == 3) abort_lds = 1;
      if (outcome == 2) {
        stop_lds = 1;
        stop_code = (int)(unsigned)(dv & 0xffffffffu);
        stop_iter = jdec;
      }
    }
    lds_barrier();
    if (abort_lds || stop_lds) break;
    // -- the neighbours' messages, consumed once: their public models move by the dequantized step
    // (CENS: a censored message moves nothing, and its code granule is an older one: never applied)
    if (in && ra >= 0 && !(CENS && hdr_censored(gRa)))
      hl = q_apply(hl, __longlong_as_double((long long)raw_bits(gRa)), L, (unsigned)(raw_bits(gWa) >> my_sh) & qmask);
    if (in && rb >= 0 && !(CENS && hdr_censored(gRb)))
      hr = q_apply(hr, __longlong_as_double((long long)raw_bits(gRb)), L, (unsigned)(raw_bits(gWb) >> my_sh) & qmask);
    if (head && pending) {  // lazy end-of-iteration dual (reference order), on public models
      double m = mu;
      if (left >= 0) m = m - rho * (hl - hat);
      if (right >= 0) m = m + rho * (hat - hr);
      mu = m;
    }
    double r = bb - mu;
    if (left >= 0) r = r + rho * hl;
    if (right >= 0) r = r + rho * hr;
    const double rv = in ? r : 0.0;

    // -- solve theta = (A + deg rho I)^{-1} r
    const double tn = quad_gemv<QT>(Mq, rv, st);

    // -- quantize theta - th_hat and publish the packed message
    const double diff = in ? tn - hat : 0.0;
    const double R = wave_max_f64(fabs(diff));
    const unsigned q = in ? q_code(diff, R, L, u) : 0u;
    double hat_new = in ? q_apply(hat, R, L, q) : 0.0;
    const unsigned long long word = group_or_u64((unsigned long long)q << my_sh, lp);  // the word of this lane's group
    const unsigned tag = make_tag(a.epoch, it);
    if constexpr (CENS) {
      // the censoring decision: would the public model move by at least this iteration's threshold?
      const bool send = wave_sum_f64_dpp(in ? c_step_sq(hat_new, hat) : 0.0) >= thr2;
      if (send && in && (lane & ((1 << lp) - 1)) == 0) put_raw(local, rq, (w * G + my_g) * 16, tag, word);
      if (lane == 0) {  // the header travels every iteration: R, or the censored notice
        put_raw(local, rq, (w * G) * 16, tag, send ? (unsigned long long)__double_as_longlong(R) : Q_CENSORED);
        if (it - 1 < a.max_iter) a.c_sent[(long)(it - 1) * n + w] = send ? 1 : 0;
      }
      if (!send) hat_new = hat;
    } else {
      if (in && (lane & ((1 << lp) - 1)) == 0) put_raw(local, rq, (w * G + my_g) * 16, tag, word);
      if (lane == 0) put_raw(local, rq, (w * G) * 16, tag, (unsigned long long)__double_as_longlong(R));
    }
    if (!head) {  // tails: both neighbours are this iteration's heads -> dual update now
      double m = mu;
      if (left >= 0) m = m - rho * (hl - hat_new);
      if (right >= 0) m = m + rho * (hat_new - hr);
      mu = m;
      if (a.rres) {  // K4 primal residual of the tail's two edges (public models)
        double rp = 0.0;
        if (in && left >= 0) rp = fma(hl - hat_new, hl - hat_new, rp);
        if (in && right >= 0) rp = fma(hat_new - hr, hat_new - hr, rp);
        const double rsum = wave_sum_f64(rp);
        if (lane == 0 && it - 1 < a.max_iter) a.rres[(long)(it - 1) * n + w] = rsum;
      }
    } else {
      pending = 1;
    }
    // -- objective of the TRUE theta: 1/2 th^T A th - b^T th + 1/2 y^T y
    const double qa = quad_gemv<QT>(Aq, in ? tn : 0.0, st);
    const double part = in ? (0.5 * qa - bb) * tn : 0.0;
    const double f = wave_sum_f64(part) + half_yy;
    if (lane == 0) put_granule<false>(local, rob, (rs * n + w) * 16, tag, f);
    th = tn;
    hat = hat_new;
  }

  // write back the final state (plain stores; visible to the host after the kernel)
  store_state(a, ls, hat, mu);
  if (in && a.q_true) a.q_true[(long)li * d + lane] = th;
  if (lane == 0) post_outcome(a.ctl, abort_lds, bid, stop_code, stop_iter, it);
}

template <int QT>
__global__ void __launch_bounds__(64) chain_persistent_q_kernel(PersistArgs a) {
  q_persistent_body<QT, false, false>(a);
}

template <int QT>
__global__ void __launch_bounds__(64) chain_persistent_cq_kernel(PersistArgs a) {
  q_persistent_body<QT, false, true>(a);
}

// Up to 8 independent Q-GADMM solves in one launch, one per XCD: slot j = blockIdx.x & 7 runs solve j
// on the blocks b % 8 == j, i.e. on the blocks that the single-solve launch leaves as exiting spacers.
// batch[j] is solve j's own PersistArgs: its own message table, theta / mu / true theta, objective and
// decision rings, ctl, trace, tstamp, xchk, tag salt, quantizer (bits, seed), rho, stop rule and
// deadline; only the read-only inputs (A, b, yy, Minv, slots, pos) may be shared. Slots may differ in
// n, d (within the QT class) and bits. Nothing assumes WHICH XCD a slot gets: with xcd = 2 a slot
// verifies that its own blocks share one (xcd_verdict on its own xchk under its own xtag) before it
// publishes with plain stores, else it publishes with sc1 stores; readers load with sc1 either way.
template <int QT>
__global__ void __launch_bounds__(64) chain_persistent_q_sweep_kernel(const PersistArgs* __restrict__ batch, int nb) {
  const int j = (int)(blockIdx.x & 7u);
  if (j >= nb) return;
  q_persistent_body<QT, true, false>(*(const SweepArgs*)(batch + j));
}

// The same launch shape on the censored body: a batch that mixes censored and uncensored members runs
// here, the uncensored ones under an all-zero threshold table (every worker always sends: Q-GADMM bit
// for bit); a batch without a censored member keeps the kernel above.
template <int QT>
__global__ void __launch_bounds__(64) chain_persistent_cq_sweep_kernel(const PersistArgs* __restrict__ batch, int nb) {
  const int j = (int)(blockIdx.x & 7u);
  if (j >= nb) return;
  q_persistent_body<QT, true, true>(*(const SweepArgs*)(batch + j));
}

// The launchers below are compiled once per translation unit: here for the Q kernels, and in
// chain_cquant.hip (which includes this file with GADMM_CQ_TU defined) for the censored ones. Two units,
// so that the Q kernels are compiled exactly as before the censored instantiations existed.
#ifdef GADMM_CQ_TU
#define Q_KERNEL chain_persistent_cq_kernel
#define Q_SWEEP_KERNEL chain_persistent_cq_sweep_kernel
#define Q_NAME "CQ"
constexpr bool CENS_TU = true;
#else
#define Q_KERNEL chain_persistent_q_kernel
#define Q_SWEEP_KERNEL chain_persistent_q_sweep_kernel
#define Q_NAME "Q"
constexpr bool CENS_TU = false;
#endif
#define Q_SWEEP_CAPACITY 8

namespace {

struct QVariant {
  const void* fn = nullptr;
  size_t shm = 0;
};

QVariant pick_q_variant(const PersistArgs& a) {
  QVariant v;
  if (a.d < 1 || a.d > 64) return v;
  // register kernel: QT = 13 covers d <= 52, 16 covers d <= 64 (as chain_persistent_kernel)
  v.fn = a.d <= 52 ? (const void*)Q_KERNEL<13> : (const void*)Q_KERNEL<16>;
  const size_t mon = (size_t)a.n * 8, stg = (size_t)QSTAGE * 8;
  v.shm = mon > stg ? mon : stg;
  return v;
}

// The persistent Q body takes `a` (else: the reason in gadmm_set_error, prefixed `who`). No HIP call.
bool q_entry_ok(const PersistArgs& a, const char* who) {
  const QVariant v = pick_q_variant(a);
  if (!v.fn || v.shm > 65536) {
    gadmm_set_error("%s: d=%d, n=%d not eligible (d <= 64)", who, a.d, a.n);
    return false;
  }
  if (a.q_bits != 4 && a.q_bits != 8 && a.q_bits != 16) {
    gadmm_set_error("%s: q_bits must be 4, 8 or 16, got %d", who, a.q_bits);
    return false;
  }
  if (CENS_TU && (!a.c_thr2 || !a.c_sent)) {
    gadmm_set_error("%s: the censored kernel needs a threshold table (c_thr2) and a c_sent buffer", who);
    return false;
  }
  if (!a.qg || !a.slots || !a.pos || !a.objg || !a.decg || !a.dec_push || !a.theta || !a.mu || !a.Minv || !a.A ||
      !a.ctl) {
    gadmm_set_error("%s: a required buffer is null", who);
    return false;
  }
  if (a.n_epochs > 0 || a.nranks != 1 || a.sys_scope || a.push || a.n_local != a.n || !a.has_monitor ||
      a.hard_stop != 0 || a.cont) {
    gadmm_set_error("%s: one GPU, every worker local, a static chain, one launch per solve", who);
    return false;
  }
  return true;
}

// nb <= 8 independent Q-GADMM solves (one GPU each, one QT class: d <= 52 or 53..64) in ONE launch, solve j
// on the blocks b % 8 == j. Every entry passes the single launch's checks; each must name its own ctl,
// trace, theta, mu, true theta, message table, objective / decision rings and xchk (gadmm_sweep_shares
// and the buffers only these kernels write). Staging buffers and the residency refusal (-2):
// gadmm_sweep_launch. -1: refused before any HIP call.
int q_sweep_launch(const PersistArgs* batch, int nb, PersistArgs* host_stage, PersistArgs* dev_stage, hipStream_t st) {
  const char* name = "persistent " Q_NAME " sweep";
  if (!gadmm_sweep_batch_ok(name, batch, nb, Q_SWEEP_CAPACITY, host_stage, dev_stage)) return -1;
  for (int j = 1; j < nb; ++j)
    if ((batch[j].d <= 52) != (batch[0].d <= 52)) {
      gadmm_set_error("%s: solves of different register classes (d = %d and %d; d <= 52 or 53..64)", name, batch[0].d,
                      batch[j].d);
      return -1;
    }
  int blocks[8];
  size_t shm = 0;
  for (int j = 0; j < nb; ++j) {
    const PersistArgs& a = batch[j];
    char who[48];
    snprintf(who, sizeof(who), "%s: solve %d", name, j);
    if (!q_entry_ok(a, who)) return -1;
    if (!a.trace || !a.b || !a.yy) {  // (the single launch leaves these to its one caller)
      gadmm_set_error("%s: a required buffer is null", who);
      return -1;
    }
    if (!a.xchk) {
      gadmm_set_error("%s has no placement-check buffer (xchk)", who);
      return -1;
    }
    blocks[j] = a.n_local + 1;
    if (blocks[j] > XCHK) {
      gadmm_set_error("%s has %d workgroups, the placement check holds %d", who, blocks[j], XCHK);
      return -1;
    }
    for (int i = 0; i < j; ++i) {
      const PersistArgs& o = batch[i];
      if (gadmm_sweep_shares(a, o) || o.qg == a.qg || (a.q_true && o.q_true == a.q_true) || o.dec_push == a.dec_push ||
          (CENS_TU && o.c_sent == a.c_sent)) {
        gadmm_set_error("%s: solves %d and %d share a buffer that both write", name, i, j);
        return -1;
      }
    }
    if (gadmm_range_defects(a)) {  // last of a slot's checks (tests/test_qsweep_cpu.py builds on that)
      gadmm_set_error("%s: ring/lag/tag range", who);
      return -1;
    }
    const size_t need = pick_q_variant(a).shm;
    if (need > shm) shm = need;
  }
  const void* fn = batch[0].d <= 52 ? (const void*)Q_SWEEP_KERNEL<13> : (const void*)Q_SWEEP_KERNEL<16>;
  return gadmm_sweep_launch({fn, 64, shm, name, false}, batch, nb, blocks, host_stage, dev_stage, st);
}

}  // namespace

#ifndef GADMM_CQ_TU
extern "C" {

// ABI self-description of the Q-GADMM fields appended to PhaseArgs / PersistArgs (ctypes mirrors in
// gadmm_amd/ops/native.py; gadmm_abi_layout covers the rest of both structs).
int gadmm_quant_abi_layout(long long* out, int n) {
  long long v[] = {(long long)offsetof(PhaseArgs, q_true), (long long)offsetof(PhaseArgs, q_msg),
                   (long long)offsetof(PhaseArgs, q_bits), (long long)offsetof(PhaseArgs, q_seed),
                   (long long)sizeof(PhaseArgs),           (long long)offsetof(PersistArgs, qg),
                   (long long)offsetof(PersistArgs, q_true), (long long)offsetof(PersistArgs, q_bits),
                   (long long)offsetof(PersistArgs, q_seed), (long long)sizeof(PersistArgs)};
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n && i < k; ++i) out[i] = v[i];
  return k;
}

// Workgroups the persistent Q kernel for `args` can keep resident (0: shape not eligible).
long gadmm_chain_persistent_q_capacity(const PersistArgs* args) {
  const QVariant v = pick_q_variant(*args);
  if (!v.fn || v.shm > 65536) return 0;
  return gadmm_resident_capacity(v.fn, 64, v.shm);
}

int gadmm_chain_persistent_q_launch(const PersistArgs* args, hipStream_t st) {
  const PersistArgs& a = *args;
  if (!q_entry_ok(a, "persistent Q kernel")) return -1;
  const QVariant v = pick_q_variant(a);
  PersistArgs ka = a;
  void* kargs[] = {&ka};
  return gadmm_persist_launch({v.fn, 64, v.shm, a.n_local + 1, "persistent Q kernel", true}, &ka, kargs, st);
}

// Solves one launch of chain_persistent_q_sweep_kernel can run side by side (one per XCD).
int gadmm_chain_persistent_q_sweep_capacity() { return Q_SWEEP_CAPACITY; }

// The sweep launch (q_sweep_launch above) on chain_persistent_q_sweep_kernel.
int gadmm_chain_persistent_q_sweep_launch(const PersistArgs* batch, int nb, PersistArgs* host_stage,
                                          PersistArgs* dev_stage, hipStream_t st) {
  return q_sweep_launch(batch, nb, host_stage, dev_stage, st);
}

}  // extern "C"
#else
extern "C" {

// ABI self-description of the CQ-GADMM fields of PhaseArgs / PersistArgs (they sit directly in front of
// the Q-GADMM fields; ctypes mirrors in gadmm_amd/ops/native.py).
int gadmm_censor_abi_layout(long long* out, int n) {
  long long v[] = {(long long)offsetof(PhaseArgs, c_thr2),   (long long)offsetof(PhaseArgs, c_sent),
                   (long long)sizeof(PhaseArgs),             (long long)offsetof(PersistArgs, c_thr2),
                   (long long)offsetof(PersistArgs, c_sent), (long long)sizeof(PersistArgs)};
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n && i < k; ++i) out[i] = v[i];
  return k;
}

// Workgroups the persistent CQ kernel for `args` can keep resident (0: shape not eligible).
long gadmm_chain_persistent_cq_capacity(const PersistArgs* args) {
  const QVariant v = pick_q_variant(*args);
  if (!v.fn || v.shm > 65536) return 0;
  return gadmm_resident_capacity(v.fn, 64, v.shm);
}

// CQ-GADMM, the whole solve in one launch: as gadmm_chain_persistent_q_launch, plus c_thr2 / c_sent.
int gadmm_chain_persistent_cq_launch(const PersistArgs* args, hipStream_t st) {
  const PersistArgs& a = *args;
  if (!q_entry_ok(a, "persistent CQ kernel")) return -1;
  const QVariant v = pick_q_variant(a);
  PersistArgs ka = a;
  void* kargs[] = {&ka};
  return gadmm_persist_launch({v.fn, 64, v.shm, a.n_local + 1, "persistent CQ kernel", true}, &ka, kargs, st);
}

// The sweep launch on chain_persistent_cq_sweep_kernel: every entry names a threshold table (all zero
// for an uncensored member, which then computes Q-GADMM bit for bit) and its own c_sent buffer.
int gadmm_chain_persistent_cq_sweep_launch(const PersistArgs* batch, int nb, PersistArgs* host_stage,
                                           PersistArgs* dev_stage, hipStream_t st) {
  return q_sweep_launch(batch, nb, host_stage, dev_stage, st);
}

}  // extern "C"
#endif
