// pba_host_lm.h — the host-driven trust-region loop of pba_solve_affine (pba_affine.hip) and pba_solve_joint
// (pba_joint.hip): Ceres' loop with the LM strategy (trust_region_minimizer.cc:67-136,
// levenberg_marquardt_strategy.cc) in the order of tests tests/gn_reference.py::lm restates, with the solve's stages as
// callables.  No device code, no engine: tests/cpp/host_lm_check.cpp drives every exit with scripted stages, stand-alone
// under the sanitizers.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "pba.h"

namespace pba {
namespace detail {

// The stages of one solve.  Each returns PBA_OK, or an error that ends the solve at once (no summary is written).
//   linearize(&cost, &gmax, &x_norm)          at the current state: its cost, the gradient max norm and ‖x‖ over the free
//                                              unknowns (‖x‖ is read after an accepted step only)
//   step(lambda, &status, &model, &sq_step)   the damped solve and the candidate state: status ≠ 0 when the factorisation
//                                              failed, the model decrease, ‖step‖²
//   candidate(&cost)                           the candidate's cost; DBL_MAX for a failed evaluation
//   accept()                                   the candidate becomes the state
// After an accept the state is the last step's candidate, so linearize may report a ‖x‖ that its step stage kept from
// that step instead of computing it again (pba_solve_joint does: the step kernel already sums ‖candidate‖²).  The loop
// calls linearize once before any step and then only directly after accept.
template <class Linearize, class Step, class Candidate, class Accept>
struct HostLmStages {
  Linearize linearize;
  Step step;
  Candidate candidate;
  Accept accept;
};
template <class Linearize, class Step, class Candidate, class Accept>
HostLmStages(Linearize, Step, Candidate, Accept) -> HostLmStages<Linearize, Step, Candidate, Accept>;

// o == nullptr: Ceres' defaults.  history gets entry 0 and one entry per trial Ceres would push (pba.h
// pba_iteration_summary); *sum (optional) the summary, total_ms the host wall clock of the call.
template <class Stages>
int host_lm(const pba_solver_options* o, Stages&& stages, std::vector<pba_iteration_summary>& hist,
            pba_solver_summary* sum) {
  pba_solver_options opt{20, 5, 1e4, 1e-6, 1e-8, 1e-3, 1e-10, 1e16, 1e-32};
  if (o) opt = *o;
  if (opt.max_num_consecutive_invalid_steps <= 0) opt.max_num_consecutive_invalid_steps = 5;
  const auto t0 = std::chrono::steady_clock::now();
  pba_solver_summary s{};
  s.termination = PBA_TERMINATION_MAX_ITERATIONS;
  s.stop_reason = PBA_STOP_MAX_ITERATIONS;
  hist.clear();
  double cost = 0.0, gmax = 0.0, x_now = 0.0;
  if (int rc = stages.linearize(&cost, &gmax, &x_now)) return rc;
  s.initial_cost = cost;
  double radius = opt.initial_trust_region_radius, factor = 2.0, x_norm = -1.0;
  int invalid = 0, it = 0;
  hist.push_back({0, 1, 1, 0, cost, 0.0, 0.0, radius, 0.0, gmax});
  auto finish = [&](int term, int reason) {
    s.termination = term;
    s.stop_reason = reason;
  };
  if (gmax <= opt.gradient_tolerance) {
    finish(PBA_TERMINATION_CONVERGENCE, PBA_STOP_GRADIENT_TOLERANCE);
  } else {
    for (it = 1; it <= opt.max_iterations; ++it) {
      double model = 0.0, ss = 0.0, cand = 0.0;
      int st = 0;
      if (int rc = stages.step(1.0 / radius, &st, &model, &ss)) return rc;
      if (st != 0 || !(model > 0.0)) {  // invalid step
        if (++invalid >= opt.max_num_consecutive_invalid_steps) {
          finish(PBA_TERMINATION_FAILURE, PBA_STOP_INVALID_STEPS);
          --it;
          break;
        }
        radius /= factor;
        factor *= 2.0;
        ++s.unsuccessful_steps;
        hist.push_back({it, 0, 0, 0, cost, 0.0, 0.0, radius, 0.0, gmax});
        if (radius <= opt.min_trust_region_radius) {
          finish(PBA_TERMINATION_CONVERGENCE, PBA_STOP_MIN_TRUST_REGION_RADIUS);
          break;
        }
        continue;
      }
      invalid = 0;
      if (int rc = stages.candidate(&cand)) return rc;
      const double step = std::sqrt(ss);
      if (step <= opt.parameter_tolerance * (x_norm + opt.parameter_tolerance)) {
        finish(PBA_TERMINATION_CONVERGENCE, PBA_STOP_PARAMETER_TOLERANCE);
        break;
      }
      if (std::fabs(cost - cand) <= opt.function_tolerance * cost) {
        finish(PBA_TERMINATION_CONVERGENCE, PBA_STOP_FUNCTION_TOLERANCE);
        break;
      }
      const double rel = (cost - cand) / model;
      if (rel > opt.min_relative_decrease) {
        if (int rc = stages.accept()) return rc;
        const double before = cost;
        // (the linearisation's cost is the candidate's: the same rows at the same state)
        if (int rc = stages.linearize(&cost, &gmax, &x_now)) return rc;
        x_norm = x_now;
        radius = std::min(opt.max_trust_region_radius, radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * rel - 1.0, 3)));
        factor = 2.0;
        ++s.successful_steps;
        hist.push_back({it, 1, 1, 0, cost, before - cost, rel, radius, step, gmax});
        if (it < opt.max_iterations && gmax <= opt.gradient_tolerance) {
          finish(PBA_TERMINATION_CONVERGENCE, PBA_STOP_GRADIENT_TOLERANCE);
          break;
        }
      } else {
        radius /= factor;
        factor *= 2.0;
        ++s.unsuccessful_steps;
        hist.push_back({it, 0, 1, 0, cand, cost - cand, rel, radius, step, gmax});
        if (radius <= opt.min_trust_region_radius) {
          finish(PBA_TERMINATION_CONVERGENCE, PBA_STOP_MIN_TRUST_REGION_RADIUS);
          break;
        }
      }
    }
    if (it > opt.max_iterations) it = opt.max_iterations;
  }
  s.iterations = it;
  s.final_cost = cost;
  s.gradient_max_norm = gmax;
  s.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = s;
  return PBA_OK;
}

}  // namespace detail
}  // namespace pba
