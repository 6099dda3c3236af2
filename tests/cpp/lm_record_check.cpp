// lm_record_check — hand-written LM decision records through the host's reading of them (pba_gn_lm_record.h: run_trials,
// read_record, Trajectory, finish_summary), the code both pba_solve and pba_solve_distributed* run.  No GPU and no HIP:
// the records come from the tables below instead of wait_decision.  Prints one JSON object, a member per case: the
// summary, the history, where the loop ended, and the order of the enqueue / wait calls.  tests/test_lm_record.py
// builds this with the address and undefined-behaviour sanitizers and checks the values.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pba_gn_lm_record.h"

using namespace pba::detail;

namespace {

struct Rec {
  double d[kLmFields];
};

// record of trial k (1-based): status 0, model > 0, gradient 10 − k unless changed afterwards
Rec rec(int k, double accept, double cost_new, double done) {
  Rec r{};
  r.d[kLmAccept] = accept;
  r.d[kLmCostNew] = cost_new;
  r.d[kLmDone] = done;
  r.d[kLmModel] = 1.0;
  r.d[kLmRel] = 0.75;
  r.d[kLmStepNorm] = 0.25;
  r.d[kLmRadius] = 1000.0 * k;
  r.d[kLmGradNorm] = 10.0 - k;
  return r;
}

void num(const char* key, double v, const char* sep = ", ") {
  if (std::isnan(v)) std::printf("\"%s\": NaN%s", key, sep);
  else std::printf("\"%s\": %.17g%s", key, v, sep);
}

void run_case(const char* name, int max_iterations, const std::vector<Rec>& recs, bool last) {
  const double initial_cost = 10.0;
  std::vector<pba_iteration_summary> history;
  pba_solver_summary s{};
  Trajectory traj(history, 1e4);
  double cost = initial_cost;
  TrialLoop lp;
  std::string order;
  auto enqueue = [&](int seq) {
    order += "e" + std::to_string(seq) + " ";
    return 0;
  };
  auto wait = [&](int seq, double* d) {
    order += "w" + std::to_string(seq) + " ";
    if (seq < 1 || seq > (int)recs.size()) return 99;  // the loop asked for a record past the one that ends the solve
    for (int i = 0; i < kLmFields; ++i) d[i] = recs[seq - 1].d[i];
    return 0;
  };
  const int rc = run_trials(max_iterations, enqueue, wait, s, traj, cost, lp);
  // as both solves finish: the initial cost into the summary and the trajectory, then the counts
  s.initial_cost = initial_cost;
  traj.finish(initial_cost);
  s.iterations = lp.iter;
  s.final_cost = cost;
  if (!order.empty()) order.pop_back();
  std::printf("\"%s\": {\"rc\": %d, \"order\": \"%s\", ", name, rc, order.c_str());
  std::printf("\"iter\": %d, \"set\": %d, \"last_enq\": %d, \"stop_seq\": %d, ", lp.iter, lp.set, lp.last_enq, lp.stop_seq);
  num("stop_done", lp.stop_done);
  std::printf("\"summary\": {\"iterations\": %d, \"successful_steps\": %d, \"unsuccessful_steps\": %d, "
              "\"termination\": %d, \"stop_reason\": %d, ",
              (int)s.iterations, (int)s.successful_steps, (int)s.unsuccessful_steps, (int)s.termination,
              (int)s.stop_reason);
  num("initial_cost", s.initial_cost);
  num("final_cost", s.final_cost);
  num("gradient_max_norm", s.gradient_max_norm, "}, ");
  std::printf("\"history\": [");
  for (size_t k = 0; k < history.size(); ++k) {
    const pba_iteration_summary& x = history[k];
    std::printf("{\"iteration\": %d, \"step_is_valid\": %d, \"step_is_successful\": %d, ", (int)x.iteration,
                (int)x.step_is_valid, (int)x.step_is_successful);
    num("cost", x.cost);
    num("cost_change", x.cost_change);
    num("relative_decrease", x.relative_decrease);
    num("step_norm", x.step_norm);
    num("trust_region_radius", x.trust_region_radius);
    num("gradient_max_norm", x.gradient_max_norm, "");
    std::printf("}%s", k + 1 < history.size() ? ", " : "");
  }
  std::printf("]}%s", last ? "" : ", ");
}

}  // namespace

int main() {
  std::printf("{\"codes\": {\"convergence\": %d, \"failure\": %d, \"max_iterations\": %d, \"function\": %d, "
              "\"gradient\": %d, \"invalid\": %d, \"radius\": %d, \"stop_max\": %d, \"done_desync\": %d}, ",
              (int)PBA_TERMINATION_CONVERGENCE, (int)PBA_TERMINATION_FAILURE, (int)PBA_TERMINATION_MAX_ITERATIONS,
              (int)PBA_STOP_FUNCTION_TOLERANCE, (int)PBA_STOP_GRADIENT_TOLERANCE, (int)PBA_STOP_INVALID_STEPS,
              (int)PBA_STOP_MIN_TRUST_REGION_RADIUS, (int)PBA_STOP_MAX_ITERATIONS, (int)kDoneDesync);
  // A: accept, reject, accept, then the function tolerance
  run_case("A", 10, {rec(1, 1, 8, 0), rec(2, 0, 9, 0), rec(3, 1, 6, 0), rec(4, 0, 5.999, kDoneFunction)}, false);
  // B: the gradient tolerance at the initial state
  run_case("B", 10, {rec(1, 0, 0, kDoneGradient)}, false);
  // C: a failed solve (status 1, whatever else the record holds), then the invalid-step limit
  Rec c1 = rec(1, 0, 123, 0);
  c1.d[kLmStatus] = 1.0;
  run_case("C", 10, {c1, rec(2, 0, 0, kDoneInvalid)}, false);
  // D: a rejected step that collapses the trust region
  run_case("D", 10, {rec(1, 0, 11, kDoneRadius)}, false);
  // E: the iteration limit
  run_case("E", 2, {rec(1, 1, 8, 0), rec(2, 1, 7, 0)}, false);
  // F (multi-GPU): an accept, then the ranks' decisions differed
  Rec f2 = rec(2, 0, 0, kDoneDesync);
  f2.d[kLmDesync] = 1.0;
  run_case("F", 10, {rec(1, 1, 8, 0), f2}, true);
  std::printf("}\n");
  return 0;
}
