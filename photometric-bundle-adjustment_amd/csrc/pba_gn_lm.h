// pba_gn_lm.h — between the LM driver (pba_gn_lm.hip: the trials, the decision kernels, pba_solve*) and the stages it
// drives (pba_gn.hip): the decision's device code, which both units compile (the driver's decision kernels, and
// schur_free_decide_kernel, which fuses the decision with the λ-free elimination and stays in pba_gn.hip), the record
// ring, and the stage entry points a trial is made of.
#pragma once

#include <cfloat>

#include "pba_gn.h"

namespace pba {
namespace detail {

// A record's decision as a small integer, identical on ranks with identical records: accept, done != 0 and 10 bits of
// the trust-region state (λ's bits folded) — summed with its square over the ranks in the next trial's scalar all-reduce
// (N·Σw² = (Σw)² ⇔ every w equal; exact in fp64 for w < 2^12)
__device__ inline double decision_word(const double* lm) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(lm[kLmLambda]);
  unsigned h = (unsigned)(b ^ (b >> 20) ^ (b >> 40) ^ (b >> 60));
  h = (h ^ (h >> 10) ^ (h >> 20)) & 1023u;
  return (double)((h << 2) | (lm[kLmDone] != 0.0 ? 2u : 0u) | (lm[kLmAccept] != 0.0 ? 1u : 0u));
}
// The published copies of the record (host-coherent page-locked memory): a ring of kRecRing slots of kLmFields fields
// + the trial's sequence number, trial `seq` in slot seq mod kRecRing.  The host enqueues one trial ahead of the record
// it waits for, so two records can be in flight; with a single slot, a host thread descheduled for longer than a trial
// (~0.23 ms at C4) would find the next trial's record over the one it waits for and fail the solve.
#ifndef PBA_REC_RING
#define PBA_REC_RING 4
#endif
constexpr int kRecRing = PBA_REC_RING, kRecStride = kLmFields + 1;  // (-DPBA_REC_RING=1: the one-slot record, tests)
__host__ __device__ inline long long rec_slot(double seq) { return ((long long)seq % kRecRing) * kRecStride; }

// The LM trial's decision on the device (trust_region_minimizer.cc semantics, the same sums and order as the host
// code of the distributed loop): model decrease from the update partials (slots [0, gp + gq)), candidate cost from
// the cost partials (slots [gp + gq, gp + gq + gc)), accepted when the solve succeeded, the model predicts a
// decrease and (cost − cost_new) / model > min_relative_decrease.  On acceptance the record's current cost becomes
// the candidate's.  One workgroup: strided per-thread sums, then a fixed-order tree in LDS (deterministic).
// The record is also published to page-locked, host-coherent memory (host_rec: the kLmFields values, then the trial's
// sequence number after a system-scope fence), so the host learns the decision by polling instead of through a copy
// and a stream event (each of which left the GPU idle ~6 µs).
constexpr int kDecideThreads = 1024;

// Ceres' termination options of the LM loop (solver.h:278-322; pba_solver_options)
struct DecideOpts {
  double min_rel, ftol, ptol, gtol, max_radius, min_radius;
  int max_invalid;
};

// The trial's sums: the pose part (identical on every rank of a distributed solve: same summed system, same step) and
// the point part with the candidate's cost and valid blocks (summed over the ranks).
enum : int {
  kTsPoseG = 0, kTsPoseD, kTsPoseStep2, kTsPoseXNorm2, kTsPoseGMax,
  kTsPtG, kTsPtD, kTsCost, kTsValid, kTsPtStep2, kTsPtXNorm2, kTsPtGMax, kTsCount
};

// The trial's decision (one lane): trust_region_minimizer.cc:85-133 + levenberg_marquardt_strategy.cc:146-160 over the
// summed trial quantities t[kTs*] and the record lm.  In Ceres' order:
//   gradient tolerance at the current state (FinalizeIteration… :336-355, GradientToleranceReached :668-684): checked
//     here, before the step, because this trial is the first to see the current state's gradient; the trial is void
//     (kDoneGradient, not an iteration);
//   invalid step — solver failure or no predicted decrease (:400-439) — HandleInvalidStep (:453-484): the 5th
//     consecutive one ends the solve with FAILURE (kDoneInvalid, not an iteration), earlier ones shrink the radius;
//   candidate cost: infinite (DBL_MAX, :771-778) when a block valid at the current state is invalid at the candidate;
//   parameter tolerance (:706-726, step_norm ≤ ptol (x_norm + ptol) with x_norm = −1 until the first accepted step,
//     :185 / :814) → kDoneParameter;  function tolerance (:729-748) → kDoneFunction (neither step applied);
//   IsStepSuccessful (:781-803) → accept (radius = min(max_radius, radius / max(1/3, 1 − (2ρ − 1)³)), :146-153) or
//     reject (radius /= factor, factor *= 2, :155-160);  MinTrustRegionRadiusReached (:687-703) → kDoneRadius.
__device__ inline void lm_decide(const double* t, int st, const DecideOpts& o, double* lm) {
  const double lambda = lm[kLmLambda];
  const double model = __dadd_rn(__dmul_rn(0.5, __dsub_rn(__dmul_rn(lambda, t[kTsPoseD]), t[kTsPoseG])),
                                 __dmul_rn(0.5, __dsub_rn(__dmul_rn(lambda, t[kTsPtD]), t[kTsPtG])));
  const double cost = lm[kLmCost];
  const double gnorm = fmax(t[kTsPoseGMax], t[kTsPtGMax]);
  double radius = lm[kLmRadius], factor = lm[kLmFactor], done = 0.0, invalid = lm[kLmInvalid];
  bool accept = false, converged = false;
  const bool valid_step = st == 0 && model > 0.0;
  const double c = t[kTsValid] < lm[kLmValid] ? DBL_MAX : t[kTsCost];
  const double step = sqrt(t[kTsPoseStep2] + t[kTsPtStep2]);
  const double rel = (cost - c) / model;
  if (gnorm <= o.gtol) {
    done = kDoneGradient;
  } else if (!valid_step) {
    invalid += 1.0;
    if (invalid >= (double)o.max_invalid) {
      done = kDoneInvalid;
    } else {
      radius /= factor;  // StepIsInvalid = StepRejected(0)
      factor *= 2.0;
      if (radius <= o.min_radius) done = kDoneRadius;
    }
  } else {
    invalid = 0.0;
    if (step <= o.ptol * (lm[kLmXNorm] + o.ptol)) {
      done = kDoneParameter;
      converged = true;
    } else if (fabs(cost - c) <= o.ftol * cost) {
      done = kDoneFunction;
      converged = true;
    } else if (rel > o.min_rel) {
      accept = true;
      const double q = 2.0 * rel - 1.0;
      radius = fmin(o.max_radius, radius / fmax(1.0 / 3.0, 1.0 - q * q * q));
      factor = 2.0;
    } else {
      radius /= factor;
      factor *= 2.0;
      if (radius <= o.min_radius) done = kDoneRadius;
    }
  }
  lm[kLmConverged] = converged ? 1.0 : 0.0;
  lm[kLmCostNew] = c;
  lm[kLmModel] = model;
  lm[kLmRel] = rel;
  lm[kLmAccept] = accept ? 1.0 : 0.0;
  lm[kLmStatus] = (double)st;
  lm[kLmStepNorm] = step;
  lm[kLmGradNorm] = gnorm;
  if (accept) {
    lm[kLmCost] = c;
    lm[kLmValid] = t[kTsValid];
    lm[kLmXNorm] = sqrt(t[kTsPoseXNorm2] + t[kTsPtXNorm2]);
    lm[kLmSet] = 1.0 - lm[kLmSet];  // the candidate's linearisation (the spare set) is now the current one
  }
  lm[kLmInvalid] = invalid;
  lm[kLmRadius] = radius;
  lm[kLmFactor] = factor;
  lm[kLmLambda] = 1.0 / radius;
  lm[kLmDone] = done;
}

// The trial's sums from the update and cost partials (one workgroup; deterministic).  Slots: red [0, gp) poses,
// [gp, gp + gq) points (model decrease parts), [gp + gq, gp + gq + gc) the candidate's (cost, valid) — one slot per
// linearisation chunk, 12.5k at C4; red2 / gmax [0, gp + gq) (update_kernel).  The red2 / gmax slots one per
// thread, then one strided pass over red with U slots per thread in flight, then xor butterflies per wave and the
// waves in order (U loads of three arrays spilled 172 B per lane at 1024 threads: 16 µs per decision).  t: the
// totals, in LDS.
// lo, hi: only the slots [lo, hi) of both passes (a slice of the sums, schur_free_decide_kernel's decision workgroups).
template <int N>
__device__ void trial_sums(const double* __restrict__ red, const double* __restrict__ red2,
                           const double* __restrict__ gmax, int gp, int gq, int gc, double* t, int lo = 0,
                           int hi = 0x7fffffff) {
  constexpr int U = 8;
  __shared__ double part[kTsCount][N / 64];
  double v[kTsCount] = {};
  const int S0 = gp + gq, S = min(S0, hi), E = min(S0 + gc, hi);
  const double2* r1 = reinterpret_cast<const double2*>(red);
  const double2* r2 = reinterpret_cast<const double2*>(red2);
  // the update slots' norms and gradient maxima: one slot per thread, loaded before the red pass so that both are
  // in flight together (S ≤ N unless the problem has > 260k points: a tail loop then)
  const int i_s = lo + (int)threadIdx.x;
  const double2 ys = i_s < S ? r2[i_s] : make_double2(0.0, 0.0);
  const double ms = i_s < S ? gmax[i_s] : 0.0;
  for (int i0 = lo + (int)threadIdx.x; i0 < E; i0 += U * N) {
    double2 x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * N;
      x[u] = i < E ? r1[i] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {  // selects, not a computed index (that put v in scratch memory)
      const int i = i0 + u * N;
      const bool p = i < gp, t = i >= gp && i < S0;
      v[kTsPoseG] += p ? x[u].x : 0.0;
      v[kTsPoseD] += p ? x[u].y : 0.0;
      v[kTsPtG] += t ? x[u].x : 0.0;
      v[kTsPtD] += t ? x[u].y : 0.0;
      v[kTsCost] += i >= S0 ? x[u].x : 0.0;  // (slots past E loaded as zeros)
      v[kTsValid] += i >= S0 ? x[u].y : 0.0;
    }
  }
  auto add_small = [&](int i, const double2& y, double m) {
    if (i < gp) {
      v[kTsPoseStep2] += y.x;
      v[kTsPoseXNorm2] += y.y;
      v[kTsPoseGMax] = fmax(v[kTsPoseGMax], m);
    } else if (i < S) {
      v[kTsPtStep2] += y.x;
      v[kTsPtXNorm2] += y.y;
      v[kTsPtGMax] = fmax(v[kTsPtGMax], m);
    }
  };
  add_small(i_s, ys, ms);
  for (int i = i_s + N; i < S; i += N) add_small(i, r2[i], gmax[i]);
  auto is_max = [](int q) { return q == kTsPoseGMax || q == kTsPtGMax; };
  // a wave past the update slots holds only candidate-cost sums: its other ten are zeros, not butterflied (the same
  // totals: only zeros are left out)
  const bool upd = __builtin_amdgcn_readfirstlane(lo + ((int)threadIdx.x & ~63)) < S;
#pragma unroll
  for (int q = 0; q < kTsCount; ++q) {
    if (!upd && q != kTsCost && q != kTsValid) continue;
    for (int m = 32; m >= 1; m >>= 1) {
      const double o = __shfl_xor(v[q], m, 64);
      v[q] = is_max(q) ? fmax(v[q], o) : v[q] + o;
    }
  }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int q = 0; q < kTsCount; ++q) part[q][threadIdx.x >> 6] = v[q];
  __syncthreads();
  // the waves in order, one thread per sum (one thread summing all twelve, 192 dependent LDS reads, was ~8 µs)
  if (threadIdx.x < kTsCount) {
    const int q = threadIdx.x;
    double w16[N / 64];
#pragma unroll
    for (int w = 0; w < N / 64; ++w) w16[w] = part[q][w];
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < N / 64; ++w) s = is_max(q) ? fmax(s, w16[w]) : s + w16[w];
    t[q] = s;
  }
  __syncthreads();
}

// Publish the record to page-locked, host-coherent memory (wave 0): lane i stores field i, every store completes, then
// lane 0 stores the sequence number the host polls for with a system-scope release.
// Every store is a system-scope relaxed atomic (`sc0 sc1`: written through to memory, whatever the page's cache
// policy), and the sequence number is stored only after every field store has completed (vmcnt(0)).  A release fence
// at system scope instead (`buffer_wbl2`) wrote back every dirty line the candidate linearisation had left in L2: the
// decision launch took 14.5-16.4 µs against 8.6 µs (profiles/r3_gn_trial_trace_*).
__device__ inline void publish_record(const double* s_rec, double* host_rec, double seq) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int l = threadIdx.x;
  if (l < kLmFields) __hip_atomic_store(host_rec + l, s_rec[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every lane's field store has completed
  __builtin_amdgcn_wave_barrier();
  if (l == 0) __hip_atomic_store(host_rec + kLmFields, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// schur_free_decide_kernel's decision part (pba_gn.hip has the kernel and the λ-free elimination it runs beside).
struct DecideArgs {
  const double* red;
  const double* red2;
  const double* gmax;
  int gp, gq, gc;
  const int* status;
  DecideOpts o;
  double* lm;
  double* host_rec;   // the published record slot, or nullptr
  double seq;
  int init;           // 1: a new solve's record (lm_init_kernel), 0: the trial's decision
  double radius;      // init: the initial trust-region radius
  double* init_out;   // init: [initial cost, valid blocks]
  double* ts_part;    // [kDecideWgs][kTsCount]: the decision workgroups' slices of the sums
  int* ts_count;      // their arrivals (0 between launches)
};
// Workgroups of schur_free_decide_kernel that sum the trial's partial slots, a slice each: one workgroup alone took ~20 µs
// for the 13.5k slots at C4 (seven dependent memory rounds), longer than the elimination beside it.
constexpr int kDecideWgs = 16;

// The scalar slots at the end of a multi-GPU exchange buffer (dist_sums_kernel has their layout)
constexpr int kExScalars = 16;

// ---- pba_gn.hip: the stages of a trial, as the driver calls them ----
int ensure_prepared(pba_engine* e, bool distributed = false);  // distributed: a multi-GPU entry point
int linearize(pba_engine* e, double* cost, const double* lm = nullptr, const PairRec* pairs = nullptr,
              const double* rho = nullptr, double* wg_red = nullptr, int* n_valid = nullptr, bool cand_intr = false,
              bool mark_set = false);
int enqueue_solve(pba_engine* e, double lambda, const double* lm = nullptr, bool free_sets = false);
void enqueue_updates(pba_engine* e, double lambda, const uint8_t* fixed, int* gp_out, int* gq_out,
                     const double* lm = nullptr, bool free_sets = false);
void launch_accept(pba_engine* e, const double* lm);
void launch_free_decide(pba_engine* e, const DecideOpts& dopt, double seq, int gp, int gq, bool init, double radius);
bool lm_free_sets(const pba_engine* e);
// multi-GPU: a trial's first launch, then this rank's system into the exchange buffer and the summed one out of it
void launch_schur_accept(pba_engine* e, const double* lm);
int enqueue_export(pba_engine* e, double lambda, const double* lm, double* X, int K);
int enqueue_import(pba_engine* e, double lambda, const double* lm, const double* X, int K);
int exchange_K(pba_engine* e, int band, int* K);
long long ex_scalar_off(const pba_engine* e, int K);
long long exchange_count(pba_engine* e, int K);

}  // namespace detail
}  // namespace pba
