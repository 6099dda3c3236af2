// Stand-alone checker of the host-driven trust-region loop (csrc/pba_host_lm.h): drives it with scripted stages — tables
// of (status, model decrease, ‖step‖², candidate cost, and the gradient norm and ‖x‖ of the linearisation after an
// accept) — one script per exit, and checks the whole summary, every field of every history row, the λ of every step
// and the order of the stage calls.  The expected values are worked out by hand from the rules in the docstring of
// tests/gn_reference.py::lm; the scripts use radii and costs whose arithmetic is exact in binary.  Compiled with
// -fsanitize=address,undefined by tests/test_host_lm.py and run as a program.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pba_host_lm.h"

using pba::detail::host_lm;
using pba::detail::HostLmStages;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

struct Trial {
  int status;
  double model, sq_step, cand;
  double gmax, x_norm;  // of the linearisation after this trial's accept
};

struct Script {
  const char* name;
  double cost0, gmax0;
  std::vector<Trial> trials;
};

struct Row {  // pba_iteration_summary without the padding
  int iteration, successful, valid;
  double cost, cost_change, relative_decrease, radius, step_norm, gmax;
};

struct Expected {
  int iterations, successful, unsuccessful, termination, stop_reason;
  double initial_cost, final_cost, gmax;
  std::vector<Row> rows;
  std::vector<double> lambdas;  // of the step calls, in order
  const char* calls;            // L linearize, S step, C candidate, A accept
};

// Ceres' defaults with the fields a script sets
pba_solver_options options(int max_iterations, int max_invalid, double radius) {
  return pba_solver_options{max_iterations, max_invalid, radius, 1e-6, 1e-8, 1e-3, 1e-10, 1e16, 1e-32};
}

int g_scripts = 0;

void run(const Script& sc, const pba_solver_options* opt, const Expected& ex) {
  std::string calls;
  std::vector<double> lambdas;
  size_t k = 0;           // the trial whose step ran last, + 1
  bool accepted = false;  // the state is trial k − 1's candidate
  HostLmStages stages{
      [&](double* cost, double* gmax, double* x_norm) {
        calls += 'L';
        if (k == 0) {
          *cost = sc.cost0;
          *gmax = sc.gmax0;
          *x_norm = 123.0;  // (not read before the first accept)
        } else {
          CHECK(accepted);  // one linearisation per accept
          accepted = false;
          *cost = sc.trials[k - 1].cand;
          *gmax = sc.trials[k - 1].gmax;
          *x_norm = sc.trials[k - 1].x_norm;
        }
        return 0;
      },
      [&](double lambda, int* status, double* model, double* sq_step) {
        calls += 'S';
        CHECK(k < sc.trials.size());
        lambdas.push_back(lambda);
        *status = sc.trials[k].status;
        *model = sc.trials[k].model;
        *sq_step = sc.trials[k].sq_step;
        ++k;
        return 0;
      },
      [&](double* cost) {
        calls += 'C';
        const Trial& t = sc.trials[k - 1];
        CHECK(t.status == 0 && t.model > 0.0);  // no candidate evaluation after an invalid step
        *cost = t.cand;
        return 0;
      },
      [&]() {
        calls += 'A';
        accepted = true;
        return 0;
      }};
  std::vector<pba_iteration_summary> hist(3);  // (stale entries: the loop clears them)
  pba_solver_summary s;
  s.iterations = -7;
  CHECK(host_lm(opt, stages, hist, &s) == PBA_OK);
  std::fprintf(stderr, "%s: %s\n", sc.name, calls.c_str());
  CHECK(calls == ex.calls);
  CHECK(k == sc.trials.size());  // the script ran to its end
  CHECK(s.iterations == ex.iterations);
  CHECK(s.successful_steps == ex.successful);
  CHECK(s.unsuccessful_steps == ex.unsuccessful);
  CHECK(s.termination == ex.termination);
  CHECK(s.stop_reason == ex.stop_reason);
  CHECK(s.pad_ == 0);
  CHECK(s.initial_cost == ex.initial_cost);
  CHECK(s.final_cost == ex.final_cost);
  CHECK(s.gradient_max_norm == ex.gmax);
  CHECK(std::isfinite(s.total_ms) && s.total_ms >= 0.0);
  CHECK(s.linearize_ms == 0.0 && s.solve_ms == 0.0 && s.cost_ms == 0.0);
  CHECK(hist.size() == ex.rows.size());
  for (size_t i = 0; i < hist.size(); ++i) {
    const pba_iteration_summary& h = hist[i];
    const Row& r = ex.rows[i];
    CHECK(h.iteration == r.iteration);
    CHECK(h.step_is_successful == r.successful);
    CHECK(h.step_is_valid == r.valid);
    CHECK(h.pad_ == 0);
    CHECK(h.cost == r.cost);
    CHECK(h.cost_change == r.cost_change);
    CHECK(h.relative_decrease == r.relative_decrease);
    CHECK(h.trust_region_radius == r.radius);
    CHECK(h.step_norm == r.step_norm);
    CHECK(h.gradient_max_norm == r.gmax);
  }
  CHECK(lambdas.size() == ex.lambdas.size());
  for (size_t i = 0; i < lambdas.size(); ++i) CHECK(lambdas[i] == ex.lambdas[i]);
  ++g_scripts;
}

int main() {
  constexpr int CONV = PBA_TERMINATION_CONVERGENCE, MAXIT = PBA_TERMINATION_MAX_ITERATIONS, FAIL = PBA_TERMINATION_FAILURE;
  // The building blocks, at cost 8: a step of norm ½ with model decrease 4 and …
  const Trial acc75{0, 4.0, 0.25, 5.0, 1.0, 2.0};   // … candidate 5: relative decrease ¾, radius /(1 − (½)³) = /0.875
  const Trial rej{0, 4.0, 0.25, 9.0, 0.0, 0.0};     // … candidate 9: relative decrease −¼, rejected
  const Trial inv_model{0, 0.0, 0.25, 0.0, 0.0, 0.0};   // no predicted decrease
  const Trial inv_neg{0, -1.0, 0.25, 0.0, 0.0, 0.0};    // a predicted increase
  const Trial inv_status{1, 4.0, 0.25, 5.0, 0.0, 0.0};  // the factorisation failed (its model decrease is not read)

  // gradient tolerance at iteration 0 (≤: equality converges), no trial; the default options (nullptr): radius 1e4
  run({"gradient tolerance at 0", 3.0, 1e-10, {}}, nullptr,
      {0, 0, 0, CONV, PBA_STOP_GRADIENT_TOLERANCE, 3.0, 3.0, 1e-10, {{0, 1, 1, 3.0, 0.0, 0.0, 1e4, 0.0, 1e-10}}, {}, "L"});

  // gradient tolerance after an accepted step: radius 7 / 0.875 = 8
  {
    Trial t = acc75;
    t.gmax = 5e-11;
    const pba_solver_options o = options(20, 5, 7.0);
    run({"gradient tolerance after an accept", 8.0, 1.0, {t}}, &o,
        {1, 1, 0, CONV, PBA_STOP_GRADIENT_TOLERANCE, 8.0, 5.0, 5e-11,
         {{0, 1, 1, 8.0, 0.0, 0.0, 7.0, 0.0, 1.0}, {1, 1, 1, 5.0, 3.0, 0.75, 8.0, 0.5, 5e-11}},
         {1.0 / 7.0}, "LSCAL"});
    // … but not when that step is the last allowed iteration (it < max_iterations): the solve ends on max iterations
    const pba_solver_options o1 = options(1, 5, 7.0);
    run({"no gradient test after the last iteration", 8.0, 1.0, {t}}, &o1,
        {1, 1, 0, MAXIT, PBA_STOP_MAX_ITERATIONS, 8.0, 5.0, 5e-11,
         {{0, 1, 1, 8.0, 0.0, 0.0, 7.0, 0.0, 1.0}, {1, 1, 1, 5.0, 3.0, 0.75, 8.0, 0.5, 5e-11}},
         {1.0 / 7.0}, "LSCAL"});
  }

  // five consecutive invalid steps: FAILURE, iterations = the trial index − 1 = 4; the radius 1e4 /2 /4 /8 /16; the
  // fifth pushes no row
  const std::vector<Row> five_rows = {{0, 1, 1, 8.0, 0.0, 0.0, 1e4, 0.0, 1.0},      {1, 0, 0, 8.0, 0.0, 0.0, 5000.0, 0.0, 1.0},
                                      {2, 0, 0, 8.0, 0.0, 0.0, 1250.0, 0.0, 1.0},   {3, 0, 0, 8.0, 0.0, 0.0, 156.25, 0.0, 1.0},
                                      {4, 0, 0, 8.0, 0.0, 0.0, 9.765625, 0.0, 1.0}};
  const std::vector<double> five_lambdas = {1e-4, 2e-4, 8e-4, 0.0064, 0.1024};
  run({"five invalid steps", 8.0, 1.0, {inv_model, inv_neg, inv_model, inv_neg, inv_model}}, nullptr,
      {4, 0, 4, FAIL, PBA_STOP_INVALID_STEPS, 8.0, 8.0, 1.0, five_rows, five_lambdas, "LSSSSS"});
  // the same with max_num_consecutive_invalid_steps = 0, meaning 5, and a solver status ≠ 0 as the invalid step
  {
    const pba_solver_options o = options(20, 0, 1e4);
    run({"invalid-step limit 0 means 5; status != 0 is invalid", 8.0, 1.0,
         {inv_status, inv_status, inv_status, inv_status, inv_status}}, &o,
        {4, 0, 4, FAIL, PBA_STOP_INVALID_STEPS, 8.0, 8.0, 1.0, five_rows, five_lambdas, "LSSSSS"});
  }

  // an invalid run broken by a valid (rejected) step, limit 2: the count starts again, so trial 3 does not fail and
  // trial 4 does; the factor keeps doubling through the rejection: radius 8 /2 /4 /8
  {
    const pba_solver_options o = options(20, 2, 8.0);
    run({"a valid step resets the invalid count", 8.0, 1.0, {inv_neg, rej, inv_status, inv_model}}, &o,
        {3, 0, 3, FAIL, PBA_STOP_INVALID_STEPS, 8.0, 8.0, 1.0,
         {{0, 1, 1, 8.0, 0.0, 0.0, 8.0, 0.0, 1.0},
          {1, 0, 0, 8.0, 0.0, 0.0, 4.0, 0.0, 1.0},
          {2, 0, 1, 9.0, -1.0, -0.25, 1.0, 0.5, 1.0},
          {3, 0, 0, 8.0, 0.0, 0.0, 0.125, 0.0, 1.0}},
         {0.125, 0.25, 1.0, 8.0}, "LSSCSS"});
  }

  // minimum trust-region radius (≤) through rejections and through invalid steps: radius 8 → 4 → 1 with minimum 1
  {
    pba_solver_options o = options(20, 5, 8.0);
    o.min_trust_region_radius = 1.0;
    run({"minimum radius through rejections", 8.0, 1.0, {rej, rej}}, &o,
        {2, 0, 2, CONV, PBA_STOP_MIN_TRUST_REGION_RADIUS, 8.0, 8.0, 1.0,
         {{0, 1, 1, 8.0, 0.0, 0.0, 8.0, 0.0, 1.0},
          {1, 0, 1, 9.0, -1.0, -0.25, 4.0, 0.5, 1.0},
          {2, 0, 1, 9.0, -1.0, -0.25, 1.0, 0.5, 1.0}},
         {0.125, 0.25}, "LSCSC"});
    run({"minimum radius through invalid steps", 8.0, 1.0, {inv_model, inv_status}}, &o,
        {2, 0, 2, CONV, PBA_STOP_MIN_TRUST_REGION_RADIUS, 8.0, 8.0, 1.0,
         {{0, 1, 1, 8.0, 0.0, 0.0, 8.0, 0.0, 1.0}, {1, 0, 0, 8.0, 0.0, 0.0, 4.0, 0.0, 1.0}, {2, 0, 0, 8.0, 0.0, 0.0, 1.0, 0.0, 1.0}},
         {0.125, 0.25}, "LSS"});
  }

  // parameter tolerance before the first accept: ‖x‖ = −1, so with tolerance 2 the bound is 2·(−1 + 2) = 2: a step of
  // norm 3 passes it (with ‖x‖ = 0 it would not: 3 ≤ 4) and is rejected, a step of norm 2 meets it; that trial pushes no
  // row and its candidate is evaluated but not applied
  {
    pba_solver_options o = options(20, 5, 8.0);
    o.parameter_tolerance = 2.0;
    Trial t3 = rej, t2 = rej;
    t3.sq_step = 9.0;
    t2.sq_step = 4.0;
    run({"parameter tolerance with x_norm = -1", 8.0, 1.0, {t3, t2}}, &o,
        {2, 0, 1, CONV, PBA_STOP_PARAMETER_TOLERANCE, 8.0, 8.0, 1.0,
         {{0, 1, 1, 8.0, 0.0, 0.0, 8.0, 0.0, 1.0}, {1, 0, 1, 9.0, -1.0, -0.25, 4.0, 3.0, 1.0}},
         {0.125, 0.25}, "LSCSC"});
  }
  // … and after it: the accepted ‖x‖ = 2 (the linearise stage's) makes the bound 1e-8·(2 + 1e-8); a step of norm 1.5e-8
  // meets it (with ‖x‖ = −1, or ‖x‖ = 1, it would not)
  {
    const pba_solver_options o = options(20, 5, 7.0);
    Trial small = rej;
    small.sq_step = 2.25e-16;
    run({"parameter tolerance with the accepted x_norm", 8.0, 1.0, {acc75, small}}, &o,
        {2, 1, 0, CONV, PBA_STOP_PARAMETER_TOLERANCE, 8.0, 5.0, 1.0,
         {{0, 1, 1, 8.0, 0.0, 0.0, 7.0, 0.0, 1.0}, {1, 1, 1, 5.0, 3.0, 0.75, 8.0, 0.5, 1.0}},
         {1.0 / 7.0, 0.125}, "LSCALSC"});
  }

  // function tolerance: |8 − 5| ≤ ½·8; the step is not applied (no accept), no row
  {
    pba_solver_options o = options(20, 5, 8.0);
    o.function_tolerance = 0.5;
    run({"function tolerance", 8.0, 1.0, {acc75}}, &o,
        {1, 0, 0, CONV, PBA_STOP_FUNCTION_TOLERANCE, 8.0, 8.0, 1.0, {{0, 1, 1, 8.0, 0.0, 0.0, 8.0, 0.0, 1.0}}, {0.125}, "LSC"});
  }

  // accept with the radius update 7 / 0.875 = 8 clamped at max_trust_region_radius = 7.5
  {
    pba_solver_options o = options(1, 5, 7.0);
    o.max_trust_region_radius = 7.5;
    run({"accepted radius clamped", 8.0, 1.0, {acc75}}, &o,
        {1, 1, 0, MAXIT, PBA_STOP_MAX_ITERATIONS, 8.0, 5.0, 1.0,
         {{0, 1, 1, 8.0, 0.0, 0.0, 7.0, 0.0, 1.0}, {1, 1, 1, 5.0, 3.0, 0.75, 7.5, 0.5, 1.0}},
         {1.0 / 7.0}, "LSCAL"});
  }

  // reject: radius /= factor, factor *= 2 (8 → 4 → 1); an accept with relative decrease ½ keeps the radius
  // (1 − 0³ = 1) and puts the factor back to 2: the next rejection halves it (1 → ½, not ⅛).  After the accept the
  // cost is 6, so the last candidate 7 has relative decrease −¼.  Ends on max iterations = 4.
  {
    const pba_solver_options o = options(4, 5, 8.0);
    const Trial acc50{0, 4.0, 0.25, 6.0, 0.5, 2.0};
    Trial last = rej;
    last.cand = 7.0;
    run({"reject, reject, accept, reject; max iterations", 8.0, 1.0, {rej, rej, acc50, last}}, &o,
        {4, 1, 3, MAXIT, PBA_STOP_MAX_ITERATIONS, 8.0, 6.0, 0.5,
         {{0, 1, 1, 8.0, 0.0, 0.0, 8.0, 0.0, 1.0},
          {1, 0, 1, 9.0, -1.0, -0.25, 4.0, 0.5, 1.0},
          {2, 0, 1, 9.0, -1.0, -0.25, 1.0, 0.5, 1.0},
          {3, 1, 1, 6.0, 2.0, 0.5, 1.0, 0.5, 0.5},
          {4, 0, 1, 7.0, -1.0, -0.25, 0.5, 0.5, 0.5}},
         {0.125, 0.25, 1.0, 1.0}, "LSCSCSCALSC"});
  }

  // a DBL_MAX candidate (a failed evaluation) is rejected: 8 − DBL_MAX rounds to −DBL_MAX
  {
    const pba_solver_options o = options(1, 5, 8.0);
    Trial t = rej;
    t.cand = DBL_MAX;
    run({"DBL_MAX candidate", 8.0, 1.0, {t}}, &o,
        {1, 0, 1, MAXIT, PBA_STOP_MAX_ITERATIONS, 8.0, 8.0, 1.0,
         {{0, 1, 1, 8.0, 0.0, 0.0, 8.0, 0.0, 1.0}, {1, 0, 1, DBL_MAX, -DBL_MAX, -DBL_MAX / 4.0, 4.0, 0.5, 1.0}},
         {0.125}, "LSC"});
  }

  // max iterations = 0: the initial linearisation only
  {
    const pba_solver_options o = options(0, 5, 8.0);
    run({"max iterations 0", 8.0, 1.0, {}}, &o,
        {0, 0, 0, MAXIT, PBA_STOP_MAX_ITERATIONS, 8.0, 8.0, 1.0, {{0, 1, 1, 8.0, 0.0, 0.0, 8.0, 0.0, 1.0}}, {}, "L"});
  }

  // a stage's error ends the solve at once: its code is returned and no summary is written
  {
    int steps = 0;
    HostLmStages stages{[](double* cost, double* gmax, double* x_norm) {
                          *cost = 8.0;
                          *gmax = 1.0;
                          *x_norm = 0.0;
                          return 0;
                        },
                        [&](double, int*, double*, double*) {
                          ++steps;
                          return 7;
                        },
                        [](double*) { return 0; }, []() { return 0; }};
    std::vector<pba_iteration_summary> hist;
    pba_solver_summary s;
    s.iterations = -7;
    CHECK(host_lm(nullptr, stages, hist, &s) == 7);
    CHECK(steps == 1 && s.iterations == -7);
    CHECK(host_lm(nullptr, stages, hist, nullptr) == 7);  // (a null summary is allowed)
  }

  std::printf("host lm: ok (%d scripts)\n", g_scripts);
  return 0;
}
