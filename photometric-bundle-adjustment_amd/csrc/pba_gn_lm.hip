// pba_gn_lm.hip — the Levenberg-Marquardt driver of the on-device Gauss-Newton solve (trust_region_minimizer.cc,
// levenberg_marquardt_strategy.cc): the kernels that take a trial's decision on the device where nothing fuses them with
// the elimination, the host side of a trial on one GPU (lm_trial) and on several (dist_trial), and pba_solve /
// pba_solve_distributed*.  Both solves run their trials through run_trials and read the published records through
// read_record (pba_gn_lm_record.h); what they enqueue is pba_gn.hip's stages (pba_gn_lm.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <string>
#include <thread>
#include <utility>

#include "pba_gn_lm.h"
#include "pba_gn_solve.h"

using namespace pba;
using namespace pba::detail;

namespace {

__global__ __launch_bounds__(kDecideThreads) void lm_decide_kernel(const double* __restrict__ red,
                                                                   const double* __restrict__ red2,
                                                                   const double* __restrict__ gmax, int gp, int gq,
                                                                   int gc, const int* __restrict__ status,
                                                                   const DecideOpts o, double* __restrict__ lm,
                                                                   double* __restrict__ host_rec, double seq) {
  // a trial enqueued ahead of the one that ended the solve returns — tested after the sums, so the record's load is in
  // flight with the partials' instead of a round trip of its own before them (the partials are always readable)
  const double done = lm[kLmDone];
  __shared__ double t[kTsCount];
  trial_sums<kDecideThreads>(red, red2, gmax, gp, gq, gc, t);
  if (done != 0.0 || threadIdx.x >= 64) return;  // wave 0 publishes; lane 0 decides
  __shared__ double s_rec[kLmFields];
  if (threadIdx.x == 0) {
    lm_decide(t, *status, o, lm);
    for (int i = 0; i < kLmFields; ++i) s_rec[i] = lm[i];
  }
  if (host_rec) publish_record(s_rec, host_rec, seq);
}

// The LM record of a new solve, on the device: the initial cost and valid blocks summed from the initial linearisation's
// chunk partials (slots [0, gc) of red — the same partials, in the same order, as a trial's candidate cost), the trust
// region, nothing done, buffer set 0, x_norm −1.  The host enqueues the first trials behind it instead of reading the cost
// back first (a host round trip with the GPU idle, once per solve); init[0..1] = the initial cost and valid blocks.
__global__ __launch_bounds__(kDecideThreads) void lm_init_kernel(const double* __restrict__ red, int gc, double radius,
                                                                 double* __restrict__ lm, double* __restrict__ init) {
  __shared__ double t[kTsCount];
  trial_sums<kDecideThreads>(red, red, red, 0, 0, gc, t);
  if (threadIdx.x != 0) return;
  for (int i = 0; i < kLmFields; ++i) lm[i] = 0.0;
  lm[kLmCost] = t[kTsCost];
  lm[kLmValid] = t[kTsValid];
  lm[kLmXNorm] = -1.0;
  lm[kLmRadius] = radius;
  lm[kLmFactor] = 2.0;
  lm[kLmLambda] = 1.0 / radius;
  init[0] = t[kTsCost];
  init[1] = t[kTsValid];
}

// Multi-GPU trial, before the scalar all-reduce: this rank's sums, written to the exchange buffer's kExScalars scalar
// slots Y for the Σ over ranks:
//   Y[0..7]  the point part: [δρ·g, δρ·D·δρ, candidate cost, candidate valid blocks, Σδρ², Σρ_new², points above the
//            gradient tolerance, 0] (the gradient test needs only whether some rank's point gradient exceeds the
//            tolerance: a count sums exactly);
//   Y[8..14] the pose part [g·δ, δ·D·δ, Σδ², Σx_new², max|g|] and the reduced solve's status, from rank 0 only (0 on the
//            other ranks).  Every rank computes them from the same summed system with the same kernels, so they agree
//            bit for bit anyway; summing rank 0's copy makes the decision inputs identical on every rank by construction
//            (a decision that differed between ranks would leave their collective sequences mismatched: a hang).
// rank0 = −1 (a host-callback collective, which does not know the ranks): Y[8..14] stay 0 and the decision reads the
// rank's own pose part from tpose.  tpose: [pose part (5) | this rank's point gradient max-norm | solve status].
__global__ __launch_bounds__(kDecideThreads) void dist_sums_kernel(const double* __restrict__ red,
                                                                   const double* __restrict__ red2,
                                                                   const double* __restrict__ gmax, int gp, int gq, int gc,
                                                                   double gtol, const double* __restrict__ lm,
                                                                   const int* __restrict__ status, int rank0,
                                                                   double* __restrict__ tpose, double* __restrict__ Y) {
  const double done = lm[kLmDone];  // (tested after the sums, as lm_decide_kernel)
  __shared__ double t[kTsCount];
  trial_sums<kDecideThreads>(red, red2, gmax, gp, gq, gc, t);
  if (threadIdx.x != 0) return;
  // the previous decision's word, with its square, and whether it ended the solve on this rank: every rank, done or not
  const double w = decision_word(lm);
  Y[7] = done != 0.0 ? 1.0 : 0.0;
  Y[14] = w;
  Y[15] = w * w;
  if (done != 0.0) {  // (the sums are not used; zeros keep them finite)
    for (int q = 0; q < 7; ++q) Y[q] = 0.0;
    for (int q = 8; q < 14; ++q) Y[q] = 0.0;
    return;
  }
  for (int q = 0; q < 5; ++q) tpose[q] = t[kTsPoseG + q];
  tpose[5] = t[kTsPtGMax];
  tpose[6] = (double)*status;
  Y[0] = t[kTsPtG];
  Y[1] = t[kTsPtD];
  Y[2] = t[kTsCost];
  Y[3] = t[kTsValid];
  Y[4] = t[kTsPtStep2];
  Y[5] = t[kTsPtXNorm2];
  Y[6] = t[kTsPtGMax] > gtol ? 1.0 : 0.0;
  for (int q = 0; q < 5; ++q) Y[8 + q] = rank0 == 1 ? t[kTsPoseG + q] : 0.0;
  Y[13] = rank0 == 1 ? (double)*status : 0.0;
}

// Multi-GPU decision from the summed Y: the same lm_decide on every rank (identical inputs), so every rank takes the
// same decision; the reported gradient norm is this rank's view (the pose part and its own points).  First the check of
// the previous decision (decision_word over the ranks, n_ranks of them): if the ranks' records differed, every rank
// ends the solve here (done = kDoneDesync, kLmDesync = 1 + the number of ranks that had stopped) — the host loops then
// match their remaining collectives (solve_distributed) and report the error instead of hanging.  The record is
// published even when the solve was already done, so a host that stopped can read this check.  perturb_seq (tests,
// PBA_TEST_PERTURB_DECISION): this rank's decision of that trial is overridden (mode 1 flips accept, 2 ends the solve).
__global__ __launch_bounds__(64) void dist_decide_kernel(const double* __restrict__ Y, const double* __restrict__ tpose,
                                                         int local, const DecideOpts o, double* __restrict__ lm,
                                                         double* __restrict__ host_rec, double seq, int n_ranks,
                                                         double perturb_seq, int perturb_mode, int verify_only) {
  __shared__ double s_rec[kLmFields];
  if (threadIdx.x == 0) {
    const bool desync = (double)n_ranks * Y[15] != Y[14] * Y[14];
    if (desync) {
      lm[kLmDone] = kDoneDesync;
      lm[kLmDesync] = Y[7] + 1.0;
      lm[kLmAccept] = 0.0;
    } else if (lm[kLmDone] == 0.0 && !verify_only) {
      const double* pose = local ? tpose : Y + 8;  // [pose part (5) | …, status at 6 resp. 5]
      double t[kTsCount];
      for (int q = 0; q < 5; ++q) t[kTsPoseG + q] = pose[q];
      t[kTsPtG] = Y[0];
      t[kTsPtD] = Y[1];
      t[kTsCost] = Y[2];
      t[kTsValid] = Y[3];
      t[kTsPtStep2] = Y[4];
      t[kTsPtXNorm2] = Y[5];
      // no rank's point gradient above the tolerance: the test then depends on the pose part alone (identical)
      t[kTsPtGMax] = Y[6] > 0.0 ? INFINITY : 0.0;
      lm_decide(t, (int)(local ? tpose[6] : Y[13]), o, lm);
      lm[kLmGradNorm] = fmax(pose[4], tpose[5]);
      if (seq == perturb_seq) {
        if (perturb_mode == 1) lm[kLmAccept] = 1.0 - lm[kLmAccept];
        else lm[kLmDone] = kDoneFunction;
      }
    }
    for (int i = 0; i < kLmFields; ++i) s_rec[i] = lm[i];
  }
  if (host_rec) publish_record(s_rec, host_rec, seq);
}

// The check of the last decision of a multi-GPU solve (no trial follows it): the decision word into Y as dist_sums_kernel
// writes it, every other slot zero.
__global__ void dist_verify_kernel(const double* __restrict__ lm, double* __restrict__ Y) {
  if (threadIdx.x != 0) return;
  const double w = decision_word(lm);
  for (int q = 0; q < kExScalars; ++q) Y[q] = 0.0;
  Y[7] = lm[kLmDone] != 0.0 ? 1.0 : 0.0;
  Y[14] = w;
  Y[15] = w * w;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Wait for trial `seq`'s decision record, published by lm_decide_kernel into host-coherent memory: a poll, not a
// stream event (an event left the GPU idle ~6 µs each) — while the host polls, the GPU runs on into the gated accept
// and linearisation.  The stream is queried now and then so a device error or a record that never comes ends the wait.
constexpr double kDecisionTimeoutMs = 60000.0;  // one trial takes ~0.25 ms at C4

int wait_decision(pba_engine* e, double seq, double* d) {
  volatile double* r = e->gn.lm_h.p + rec_slot(seq);
  // the stream is queried only after 2 ms without the record (a trial takes ~0.23 ms at C4), then every 2 ms: a
  // hipStreamQuery every few hundred spins idled the GPU 5.7 µs before every trial's first kernel
  // (profiles/r2_gn_trial_trace_v7.txt → v9)
  // A device that stops making progress ends the wait after kDecisionTimeoutMs with PBA_ERR_DEVICE.
  const double t0 = now_ms();
  double next_query = t0 + 2.0;
  for (unsigned spins = 1;; ++spins) {
    if (r[kLmFields] == seq) break;
    if ((spins & 255u) == 0u && now_ms() >= next_query) {
      next_query = now_ms() + 2.0;
      const hipError_t q = hipStreamQuery(e->stream);
      if (q == hipSuccess && r[kLmFields] != seq) return fail(PBA_ERR_DEVICE, "LM decision record was not published");
      if (q != hipSuccess && q != hipErrorNotReady) return fail(PBA_ERR_DEVICE, std::string("HIP: ") + hipGetErrorString(q));
      if (next_query - t0 > kDecisionTimeoutMs)
        return fail(PBA_ERR_DEVICE, "LM decision record not published within " + std::to_string(kDecisionTimeoutMs / 1000) + " s");
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  for (int i = 0; i < kLmFields; ++i) d[i] = r[i];
  return PBA_OK;
}

// Levenberg-Marquardt (trust_region_minimizer.cc + levenberg_marquardt_strategy.cc semantics):
// μ = 1/radius, step accepted when (cost − cost_new)/model_decrease > min_relative_decrease (1e-3);
// success: radius /= max(1/3, 1 − (2ρ − 1)³), decrease factor 2; failure: radius /= factor, factor *= 2.
// With a Reducer every cost, model decrease and the reduced system are sums over ranks, so all ranks take
// the same decisions and the same pose steps.
pba_solver_options lm_options(const pba_solver_options* o) {
  pba_solver_options opt{};  // Ceres' defaults (solver.h:278-322), max_num_iterations as map_utils.h:318
  opt.max_iterations = 20;
  opt.max_num_consecutive_invalid_steps = 5;
  opt.initial_trust_region_radius = 1e4;
  opt.function_tolerance = 1e-6;
  opt.parameter_tolerance = 1e-8;
  opt.min_relative_decrease = 1e-3;
  opt.gradient_tolerance = 1e-10;
  opt.max_trust_region_radius = 1e16;
  opt.min_trust_region_radius = 1e-32;
  if (o) opt = *o;
  if (opt.max_num_consecutive_invalid_steps <= 0) opt.max_num_consecutive_invalid_steps = 5;
  return opt;
}

DecideOpts decide_opts(const pba_solver_options& o) {
  return DecideOpts{o.min_relative_decrease, o.function_tolerance, o.parameter_tolerance, o.gradient_tolerance,
                    o.max_trust_region_radius, o.min_trust_region_radius, o.max_num_consecutive_invalid_steps};
}

// After a solve: the last accepted candidate's linearisation is the current one; if it is in buffer set 1, that becomes
// set 0, which the host-driven entry points read.
void current_set_to_0(GnData& G, int set) {
  if (set != 1) return;
  auto swap = [](auto& a, auto& b) {
    std::swap(a.p, b.p);
    std::swap(a.n, b.n);
  };
  swap(G.blk_schur, G.blk_schur1);
  swap(G.pair_rt, G.pair_rt1);
  swap(G.part_lin, G.part_lin1);
}

// One LM trial on a single GPU, enqueued whole and steered by the device LM record G.lm (λ, buffer set, done):
// Schur complement + reduced solve → candidate state (poses, ρ, pair table) and model-decrease partials →
// linearisation AT the candidate into the spare buffer set, whose per-chunk cost partials are the candidate cost →
// the decision on the device (accept, the next trust radius, done; published to the host); the accept itself is applied
// by the next trial's first kernel.  An accepted
// step's linearisation is then already done (a rejected one cost a linearisation instead of a residual-only pass), and
// since every kernel returns at once when the solve is done, the host enqueues the next trial before it has seen this
// one's decision: no host round trip between trials.  The candidate is evaluated even when the solve failed (its
// numbers are then discarded): a garbage state is memory-safe in every evaluation kernel.  ev (phase timing only,
// else nullptr): begin | candidate state | candidate linearisation | decision.
int lm_trial(pba_engine* e, const DecideOpts& dopt, double seq, const hipEvent_t* ev) {
  GnData& G = e->gn;
  const bool fs = lm_free_sets(e);
  if (ev) PBA_HIP(hipEventRecord(ev[0], e->stream));
  if (int rc = enqueue_solve(e, 0.0, G.lm.p, fs)) return rc;
  int gp = 0, gq = 0;
  enqueue_updates(e, 0.0, G.fixed.p, &gp, &gq, G.lm.p, fs);
  if (ev) PBA_HIP(hipEventRecord(ev[1], e->stream));
  if (int rc = linearize(e, nullptr, G.lm.p, G.pairs_new.p, G.rho_new.p, G.red.p + 2 * (gp + gq), nullptr, true, fs))
    return rc;
  if (ev) PBA_HIP(hipEventRecord(ev[2], e->stream));
  if (fs)
    launch_free_decide(e, dopt, seq, gp, gq, false, 0.0);
  else
    lm_decide_kernel<<<1, kDecideThreads, 0, e->stream>>>(G.red.p, G.red2.p, G.gmax.p, gp, gq, G.n_chunks, G.status.p,
                                                          dopt, G.lm.p, G.lm_host_d + rec_slot(seq), seq);
  PBA_HIP(hipGetLastError());
  if (ev) PBA_HIP(hipEventRecord(ev[3], e->stream));
  return PBA_OK;  // an accepted candidate becomes the state in the next trial's first kernel (or after the loop)
}

// Single GPU: every trial is enqueued whole (lm_trial) and the accept/reject decision is taken on the device, so
// the host only reads the decision record back; the breakdown is device time between stream events.
int solve_single(pba_engine* e, const pba_solver_options* o, pba_solver_summary* sum) {
  GnData& G = e->gn;
  const pba_solver_options opt = lm_options(o);
  pba_solver_summary s{};
  struct Events {  // phase timing (pba_set_solver_timing): two sets of 4 (a trial is enqueued ahead)
    hipEvent_t ev[8] = {};
    ~Events() {
      for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    }
  } events;
  const bool timed = G.phase_timing;
  if (timed)
    for (int i = 0; i < 8; ++i) PBA_HIP(hipEventCreate(&events.ev[i]));
  const double t0 = now_ms();
  double cost = 0.0;
  // the initial linearisation (set 0) with its chunk cost partials in red, and the device record formed from them
  // (lm_init_kernel): no host round trip before the first trial
  const bool fs = lm_free_sets(e);
  if (int rc = linearize(e, nullptr, nullptr, nullptr, nullptr, G.red.p, nullptr, false, fs)) return rc;
  if (G.lm_init.n < 2) PBA_HIP(G.lm_init.resize(2));
  const DecideOpts dopt = decide_opts(opt);
  if (fs)  // the record and set 0's λ-free partials in one launch
    launch_free_decide(e, dopt, 0.0, 0, 0, true, opt.initial_trust_region_radius);
  else
    lm_init_kernel<<<1, kDecideThreads, 0, e->stream>>>(G.red.p, G.n_chunks, opt.initial_trust_region_radius, G.lm.p,
                                                         G.lm_init.p);
  PBA_HIP(hipGetLastError());
  for (int r = 0; r < kRecRing; ++r) G.lm_h[r * kRecStride + kLmFields] = 0.0;  // no trial published yet
  // PBA_LM_HOST_DELAY_US (test build only, PBA_TEST_HOOKS): the host thread sleeps this long before each wait, as a
  // descheduled thread would
  const int delay_us = test_hook_int("PBA_LM_HOST_DELAY_US");
  auto events_of = [&](int seq) { return timed ? events.ev + 4 * ((seq - 1) & 1) : nullptr; };
  auto enqueue = [&](int seq) { return lm_trial(e, dopt, (double)seq, events_of(seq)); };
  auto wait = [&](int seq, double* d) -> int {
    if (delay_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(delay_us));
    if (int rc = wait_decision(e, (double)seq, d)) return rc;
    if (const hipEvent_t* ev = events_of(seq)) {
      float ms = 0.0f;
      PBA_HIP(hipEventSynchronize(ev[3]));
      PBA_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
      s.solve_ms += ms;
      PBA_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
      s.linearize_ms += ms;
      PBA_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
      s.cost_ms += ms;
    }
    return PBA_OK;
  };
  Trajectory traj(G.history, opt.initial_trust_region_radius);
  TrialLoop lp;
  if (int rc = run_trials(std::max(0, opt.max_iterations), enqueue, wait, s, traj, cost, lp)) return rc;
  launch_accept(e, G.lm.p);  // the last trial's accept (no trial after it to apply it)
  double init[2] = {0.0, 0.0};
  PBA_HIP(hipMemcpyAsync(init, G.lm_init.p, sizeof init, hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  s.initial_cost = init[0];
  traj.finish(init[0]);
  if (s.successful_steps == 0) cost = init[0];
  current_set_to_0(G, lp.set);
  // a photometric engine's host copy of the (level-0) intrinsics state follows the solved device state
  if (G.nc_sys && s.successful_steps > 0)
    if (int rc = download_intrinsics_state(e)) return rc;
  s.iterations = lp.iter;
  s.final_cost = cost;
  s.total_ms = now_ms() - t0;
  if (sum) *sum = s;
  return PBA_OK;
}

// The collective of the multi-GPU loop: stream-ordered (a pba_comm: RCCL or an in-process group) or a host callback
// that is called once the engine's stream has drained and is complete when it returns.
struct Collective {
  pba_allreduce_fn fn = nullptr;
  void* user = nullptr;
  pba_comm* comm = nullptr;
  int allreduce(pba_engine* e, double* buf, long long n) const {
    if (comm) return comm_allreduce(comm, buf, n, e->stream);
    PBA_HIP(hipStreamSynchronize(e->stream));
    if (int rc = fn(user, buf, n)) return fail(PBA_ERR_DEVICE, "allreduce callback failed (" + std::to_string(rc) + ")");
    return PBA_OK;
  }
  // dist_sums_kernel's rank flag: 1 rank 0, 0 another rank, −1 unknown (a host callback without pba_gn_set_rank)
  int rank0(const pba_engine* e) const {
    const int r = comm ? comm_rank(comm) : e->gn.dist_rank;
    return r < 0 ? -1 : (r == 0 ? 1 : 0);
  }
};

// One multi-GPU LM trial, enqueued whole on the engine stream and steered by the device LM record like lm_trial:
// point elimination for the record's λ (the previous trial's accept applied first) → this rank's banded partial system
// into X → Σ over ranks → damping, constant frames (requested, or observed by no rank), solve → candidate state and the
// update partials → candidate linearisation into the spare buffer set (its chunk partials are this rank's candidate
// cost) → this rank's trial sums, the point part Σ over ranks (kExScalars doubles) → the decision, the same on every
// rank, published to the host.  Two collectives per trial: λ of trial i + 1 depends on the decision of trial i, and the
// point elimination (hence this rank's system) on λ.  With a stream-ordered collective the host enqueues the next trial
// before this one's decision is known, as on one GPU; every rank enqueues the same trials (the decisions agree), so the
// collectives match.
// PBA_TEST_PERTURB_DECISION = "rank:trial:mode" (tests): that rank's decision of that trial is overridden (mode 1: the
// accept flag flipped, 2: the solve ended) — the ranks' records then differ, which the next trial's check must catch.
struct DistCheck {
  int n_ranks = 1;
  double perturb_seq = -1.0;
  int perturb_mode = 0;
};

int dist_trial(pba_engine* e, const Collective& coll, const DecideOpts& dopt, double* X, int K, double seq,
               const DistCheck& chk) {
  GnData& G = e->gn;
  launch_schur_accept(e, G.lm.p);
  const long long nx = ex_scalar_off(e, K);  // the band rows and, with free intrinsics, the border rows
  if (int rc = enqueue_export(e, 0.0, G.lm.p, X, K)) return rc;
  if (int rc = coll.allreduce(e, X, nx)) return rc;
  if (int rc = enqueue_import(e, 0.0, G.lm.p, X, K)) return rc;
  int gp = 0, gq = 0;
  enqueue_updates(e, 0.0, G.fixed_dist.p, &gp, &gq, G.lm.p);
  if (G.n_chunks > 0)
    if (int rc = linearize(e, nullptr, G.lm.p, G.pairs_new.p, G.rho_new.p, G.red.p + 2 * (gp + gq), nullptr, true))
      return rc;  // (at the candidate intrinsics too)
  double* Y = X + nx;
  dist_sums_kernel<<<1, kDecideThreads, 0, e->stream>>>(G.red.p, G.red2.p, G.gmax.p, gp, gq, G.n_chunks, dopt.gtol,
                                                         G.lm.p, G.status.p, coll.rank0(e), G.tpose.p, Y);
  PBA_HIP(hipGetLastError());
  if (int rc = coll.allreduce(e, Y, kExScalars)) return rc;
  dist_decide_kernel<<<1, 64, 0, e->stream>>>(Y, G.tpose.p, coll.rank0(e) < 0 ? 1 : 0, dopt, G.lm.p,
                                              G.lm_host_d + rec_slot(seq), seq, chk.n_ranks, chk.perturb_seq,
                                              chk.perturb_mode, 0);
  PBA_HIP(hipGetLastError());
  return PBA_OK;
}

// The LM loop over all ranks: the initial cost summed over the ranks and the record staged from the host, the trials,
// then the drain that leaves every rank with the same collectives issued and the check of the last decision; after it
// the last accepted candidate becomes the state and the current linearisation is moved to buffer set 0.
int solve_distributed(pba_engine* e, const pba_solver_options* o, const Collective& coll, double* X, int K,
                      pba_solver_summary* sum) {
  GnData& G = e->gn;
  const pba_solver_options opt = lm_options(o);
  pba_solver_summary s{};
  const double t0 = now_ms();
  if (int rc = ensure_exchange_solver(e, K)) return rc;
  double cost = 0.0;
  int n_valid = 0;
  if (int rc = linearize(e, &cost, nullptr, nullptr, nullptr, nullptr, &n_valid)) return rc;
  DistCheck chk;
  {  // Σ over ranks of the initial cost and valid blocks — and of 1: the number of ranks — through the scalar slots
    double v[3] = {cost, (double)n_valid, 1.0};
    double* Y = X + ex_scalar_off(e, K);
    PBA_HIP(hipMemcpyAsync(Y, v, sizeof v, hipMemcpyHostToDevice, e->stream));
    if (int rc = coll.allreduce(e, Y, 3)) return rc;
    PBA_HIP(hipMemcpyAsync(v, Y, sizeof v, hipMemcpyDeviceToHost, e->stream));
    PBA_HIP(hipStreamSynchronize(e->stream));
    cost = v[0];
    n_valid = (int)v[1];
    chk.n_ranks = (int)v[2];
  }
  if (const char* pv = test_hook("PBA_TEST_PERTURB_DECISION")) {  // test build: "rank:trial:mode"
    int pr = -1, pt = -1, pm = 1;
    if (std::sscanf(pv, "%d:%d:%d", &pr, &pt, &pm) >= 2 && pr == (coll.comm ? comm_rank(coll.comm) : G.dist_rank)) {
      chk.perturb_seq = pt;
      chk.perturb_mode = pm;
    }
  }
  s.linearize_ms = now_ms() - t0;
  s.initial_cost = cost;
  for (int i = 0; i < kRecRing * kRecStride; ++i) G.lm_h[i] = 0.0;  // (slot 0 stages the initial record below)
  G.lm_h[kLmCost] = cost;
  G.lm_h[kLmValid] = n_valid;
  G.lm_h[kLmXNorm] = -1.0;
  G.lm_h[kLmRadius] = opt.initial_trust_region_radius;
  G.lm_h[kLmFactor] = 2.0;
  G.lm_h[kLmLambda] = 1.0 / opt.initial_trust_region_radius;
  PBA_HIP(hipMemcpyAsync(G.lm.p, G.lm_h.data(), sizeof(double) * kLmFields, hipMemcpyHostToDevice, e->stream));
  const int n = std::max(0, opt.max_iterations);
  const DecideOpts dopt = decide_opts(opt);
  auto enqueue = [&](int seq) { return dist_trial(e, coll, dopt, X, K, (double)seq, chk); };
  auto wait = [&](int seq, double* d) { return wait_decision(e, (double)seq, d); };
  Trajectory traj(G.history, opt.initial_trust_region_radius);
  TrialLoop lp;  // (last_enq: collectives included)
  if (int rc = run_trials(n, enqueue, wait, s, traj, cost, lp)) return rc;
  // Every rank must leave with the same collectives issued.  Ranks whose records agree stop on the same trial; if they
  // differed at trial k, the next trial's check ends the solve everywhere (kDoneDesync), but a rank whose record k said
  // done has enqueued one trial fewer than a rank that went on (which enqueued k + 2 ahead): it reads record k + 1 (always
  // published) and, when ranks went on, issues trial k + 2 too.  Then the last decision is checked by one more scalar
  // all-reduce on every rank.
  bool desync = lp.stop_done == kDoneDesync;
  int desync_at = desync ? lp.stop_seq - 1 : 0;
  if (!desync && lp.stop_seq > 0 && lp.last_enq > lp.stop_seq) {
    double d2[kLmFields];
    if (int rc = wait(lp.stop_seq + 1, d2)) return rc;
    if (d2[kLmDone] == kDoneDesync) {
      desync = true;
      desync_at = lp.stop_seq;
      const int stopped = (int)d2[kLmDesync] - 1;  // ranks whose record stop_seq ended the solve
      if (stopped < chk.n_ranks && lp.stop_seq + 2 <= n) {
        if (int rc = enqueue(lp.stop_seq + 2)) return rc;
        lp.last_enq = lp.stop_seq + 2;
      }
    }
  }
  {
    double* Y = X + ex_scalar_off(e, K);
    dist_verify_kernel<<<1, 64, 0, e->stream>>>(G.lm.p, Y);
    PBA_HIP(hipGetLastError());
    if (int rc = coll.allreduce(e, Y, kExScalars)) return rc;
    const double vseq = (double)(lp.last_enq + 1);
    dist_decide_kernel<<<1, 64, 0, e->stream>>>(Y, G.tpose.p, 1, dopt, G.lm.p, G.lm_host_d + rec_slot(vseq), vseq,
                                                chk.n_ranks, -1.0, 0, 1);
    PBA_HIP(hipGetLastError());
    double d3[kLmFields];
    if (int rc = wait_decision(e, vseq, d3)) return rc;
    if (!desync && d3[kLmDone] == kDoneDesync) {
      desync = true;
      desync_at = lp.last_enq;
    }
  }
  launch_accept(e, G.lm.p);
  PBA_HIP(hipStreamSynchronize(e->stream));
  if (desync)
    return fail(PBA_ERR_DEVICE, "multi-GPU solve: the ranks' LM decisions differed at trial " + std::to_string(desync_at) +
                                    " (decision-word check); every rank ended the solve");
  traj.finish(s.initial_cost);
  current_set_to_0(G, lp.set);
  s.iterations = lp.iter;
  s.final_cost = cost;
  s.total_ms = now_ms() - t0;
  if (sum) *sum = s;
  return PBA_OK;
}

}  // namespace

extern "C" {

int pba_solve(pba_engine* e, const pba_solver_options* o, pba_solver_summary* sum) {
  if (int rc = ensure_prepared(e)) return rc;
  e->joint.linearized = false;  // (the solve moves the state)
  return solve_single(e, o, sum);
}

int pba_solver_iterations(const pba_engine* e, int32_t capacity, pba_iteration_summary* out, int32_t* count) {
  if (!e || !count || capacity < 0 || (capacity > 0 && !out)) return fail(PBA_ERR_INVALID_ARGUMENT, "bad arguments");
  const std::vector<pba_iteration_summary>& h = e->gn.history;
  const int n = std::min<int>(capacity, (int)h.size());
  for (int i = 0; i < n; ++i) out[i] = h[i];
  *count = (int)h.size();
  return PBA_OK;
}

int pba_set_solver_timing(pba_engine* e, int32_t enable) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  e->gn.phase_timing = enable != 0;
  return PBA_OK;
}

int pba_solve_distributed(pba_engine* e, const pba_solver_options* o, int32_t band, double* d_exchange,
                          pba_allreduce_fn allreduce, void* user, pba_solver_summary* sum) {
  if (int rc = ensure_prepared(e, true)) return rc;
  if (!d_exchange || !allreduce) return fail(PBA_ERR_INVALID_ARGUMENT, "null exchange buffer or allreduce");
  int K;
  if (int rc = exchange_K(e, band, &K)) return rc;
  Collective c;
  c.fn = allreduce;
  c.user = user;
  return solve_distributed(e, o, c, d_exchange, K, sum);
}

int pba_solve_distributed_comm(pba_engine* e, const pba_solver_options* o, int32_t band, pba_comm* comm,
                               pba_solver_summary* sum) {
  if (int rc = ensure_prepared(e, true)) return rc;
  if (!comm) return fail(PBA_ERR_INVALID_ARGUMENT, "null communicator");
  int K;
  if (int rc = exchange_K(e, band, &K)) return rc;
  GnData& G = e->gn;
  PBA_HIP(G.exchange.resize((size_t)exchange_count(e, K)));
  Collective c;
  c.comm = comm;
  return solve_distributed(e, o, c, G.exchange.p, K, sum);
}

}  // extern "C"
