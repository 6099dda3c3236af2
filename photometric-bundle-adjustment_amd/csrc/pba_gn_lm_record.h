// pba_gn_lm_record.h — the LM decision record and how the host reads a solve's records: the record's fields, the done
// reasons the device writes (lm_decide, pba_gn_lm.h), and the mapping from the published records to Ceres' summary and
// iteration history (pba.h) with the loop that applies it, shared by the single- and the multi-GPU solve
// (pba_gn_lm.hip).  No HIP: only pba.h and the standard library, so tests/cpp/lm_record_check.cpp drives the same
// code with hand-written records.
#pragma once

#include <cmath>
#include <vector>

#include "pba.h"

namespace pba {
namespace detail {

// LM decision record kept on the device by the LM loops (lm_decide_kernel).
// The trial's outcome, then the trust-region state the next trial runs with (λ = 1/radius, read by the kernels), the
// done flag (kDone*; every later kernel of the solve returns at once), the index of the linearisation buffer set
// holding the current state's normal-equation pieces (flipped on acceptance), and Ceres' bookkeeping: the current
// state's valid blocks, x_norm (−1 until the first accepted step), consecutive invalid steps, and the trial's step and
// gradient norms.
enum : int {
  kLmCost = 0, kLmCostNew = 1, kLmModel = 2, kLmRel = 3, kLmAccept = 4, kLmStatus = 5, kLmConverged = 6,
  kLmLambda = 7, kLmRadius = 8, kLmFactor = 9, kLmDone = 10, kLmSet = 11, kLmValid = 12, kLmXNorm = 13,
  kLmInvalid = 14, kLmStepNorm = 15, kLmGradNorm = 16, kLmDesync = 17, kLmFields = 18
};

// kLmDone, as Ceres stops (trust_region_minimizer.cc; lm_decide has the order of the tests): function tolerance,
// the limit of consecutive invalid steps, parameter tolerance, gradient tolerance, minimum trust region radius.
// kDoneDesync (multi-GPU): the ranks' decisions of the previous trial differed (kLmDesync = 1 + the number of ranks whose
// record said done then); every rank ends the solve with an error
enum : int { kDoneFunction = 1, kDoneInvalid = 2, kDoneParameter = 3, kDoneGradient = 4, kDoneRadius = 5, kDoneDesync = 6 };

// The summary's outcome from a published decision record (done != 0).  Returns whether the trial counts as an
// iteration (Ceres pushes no IterationSummary for a gradient-tolerance stop, which happens before the step, nor for the
// consecutive-invalid-steps failure).
inline bool finish_summary(double done, pba_solver_summary& s) {
  switch ((int)done) {
    case kDoneFunction: s.termination = PBA_TERMINATION_CONVERGENCE; s.stop_reason = PBA_STOP_FUNCTION_TOLERANCE; return true;
    case kDoneParameter: s.termination = PBA_TERMINATION_CONVERGENCE; s.stop_reason = PBA_STOP_PARAMETER_TOLERANCE; return true;
    case kDoneGradient: s.termination = PBA_TERMINATION_CONVERGENCE; s.stop_reason = PBA_STOP_GRADIENT_TOLERANCE; return false;
    case kDoneRadius: s.termination = PBA_TERMINATION_CONVERGENCE; s.stop_reason = PBA_STOP_MIN_TRUST_REGION_RADIUS; return true;
    default: s.termination = PBA_TERMINATION_FAILURE; s.stop_reason = PBA_STOP_INVALID_STEPS; return false;
  }
}

// The trajectory of a solve, as Ceres' Solver::Summary::iterations (pba.h, pba_iteration_summary): entry 0 the initial
// state, then one entry per trial Ceres pushes.  Filled from the published decision records as the host reads them; the
// costs and cost changes are completed by finish() once the initial cost is known (pba_solve reads it after the loop).
struct Trajectory {
  std::vector<pba_iteration_summary>& it;
  explicit Trajectory(std::vector<pba_iteration_summary>& v, double radius) : it(v) {
    it.clear();
    pba_iteration_summary z{};
    z.step_is_successful = z.step_is_valid = 1;
    z.trust_region_radius = radius;
    z.gradient_max_norm = NAN;
    it.push_back(z);
  }
  // trial record d (kLm* fields): its gradient is the one at the state the trial started from, i.e. the state the last
  // entry ended in, if that entry has none yet (the initial state, an accepted step)
  void trial(const double* d) {
    if (std::isnan(it.back().gradient_max_norm)) it.back().gradient_max_norm = d[kLmGradNorm];
    const double done = d[kLmDone];
    if (done != 0.0 && done != kDoneRadius) return;  // a tolerance or the invalid-step limit: Minimize returns first
    pba_iteration_summary x{};
    x.iteration = (int)it.size();
    x.step_is_valid = d[kLmStatus] == 0.0 && d[kLmModel] > 0.0;
    x.step_is_successful = d[kLmAccept] != 0.0;
    x.cost = d[kLmCostNew];  // (the candidate's; finish() puts the current cost on invalid steps)
    x.relative_decrease = x.step_is_valid ? d[kLmRel] : 0.0;
    x.trust_region_radius = d[kLmRadius];
    x.step_norm = x.step_is_valid ? d[kLmStepNorm] : 0.0;
    x.gradient_max_norm = x.step_is_successful ? NAN : it.back().gradient_max_norm;
    it.push_back(x);
  }
  void finish(double initial_cost) {
    double cur = initial_cost;
    it[0].cost = initial_cost;
    for (size_t k = 1; k < it.size(); ++k) {
      pba_iteration_summary& x = it[k];
      if (!x.step_is_valid) {
        x.cost = cur;
        x.cost_change = 0.0;
        continue;
      }
      x.cost_change = cur - x.cost;
      if (x.step_is_successful) cur = x.cost;
    }
  }
};

// What one published record means for the loop: whether it ends the solve, whether the ending trial counts as an
// iteration, and the done value that ended it (0 while the solve goes on).
struct RecordOutcome {
  bool stop, counts;
  double done;
};

// Record d of the next trial into the summary (gradient norm, step counts, and termination / stop reason when it ends
// the solve), the trajectory and the running cost.  A kDoneDesync record (only a multi-GPU solve writes one) ends the
// loop before the trajectory sees it: the solve fails, and the record is the check's, not a trial's.
inline RecordOutcome read_record(const double* d, pba_solver_summary& s, Trajectory& traj, double& cost) {
  s.gradient_max_norm = d[kLmGradNorm];
  const double done = d[kLmDone];
  if (done == kDoneDesync) return {true, false, done};
  traj.trial(d);
  if (done != 0.0 && done != kDoneRadius)  // a tolerance (the step is not applied) or the invalid-step limit
    return {true, finish_summary(done, s), done};
  if (d[kLmAccept] == 0.0) {  // invalid step (failed solve, no predicted decrease) or too little actual decrease
    ++s.unsuccessful_steps;
    if (done == 0.0) return {false, false, 0.0};
    finish_summary(done, s);  // the trust region collapsed
    return {true, true, done};
  }
  ++s.successful_steps;
  cost = d[kLmCostNew];
  return {false, false, 0.0};
}

// Where a solve's trial loop ended: the trials Ceres counts, the buffer set of the last record read, the last trial
// enqueued, and the trial whose record ended the loop with its done value (0: the iteration limit).
struct TrialLoop {
  int iter = 0, set = 0, last_enq = 0, stop_seq = 0;
  double stop_done = 0.0;
};

// The Ceres-facing loop of every solve, at most n trials: trial seq + 1 is enqueued before the record of trial seq is
// waited for (no host round trip between trials; a trial after the end returns at once on the device), and each record
// goes through read_record.  enqueue(seq) enqueues trial seq whole; wait(seq, d) returns its record's kLmFields values
// — the driver's wait_decision, with whatever the caller does around it per trial (phase timing); both return 0 or an
// error that ends the loop.  s.termination / s.stop_reason are the iteration limit's unless a record sets them.
template <class Enqueue, class Wait>
int run_trials(int n, Enqueue&& enqueue, Wait&& wait, pba_solver_summary& s, Trajectory& traj, double& cost,
               TrialLoop& r) {
  s.termination = PBA_TERMINATION_MAX_ITERATIONS;
  s.stop_reason = PBA_STOP_MAX_ITERATIONS;
  if (n > 0) {
    if (int rc = enqueue(1)) return rc;
    r.last_enq = 1;
  }
  for (; r.iter < n; ++r.iter) {
    const int seq = r.iter + 1;
    if (seq < n) {
      if (int rc = enqueue(seq + 1)) return rc;  // ahead of this trial's decision
      r.last_enq = seq + 1;
    }
    double d[kLmFields];
    if (int rc = wait(seq, d)) return rc;
    r.set = (int)d[kLmSet];
    const RecordOutcome out = read_record(d, s, traj, cost);
    if (!out.stop) continue;
    r.stop_seq = seq;
    r.stop_done = out.done;
    if (out.counts) ++r.iter;
    break;
  }
  return 0;
}

}  // namespace detail
}  // namespace pba
