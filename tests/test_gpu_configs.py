"""GPU tests at the sizes of BASELINE.json's configurations:

* C1 (configs[0]) — 20 EuRoC stereo keyframes × 2k landmarks, geometric, double-sphere cameras with the reference's
  EuRoC calibration: records against the oracle; the engine's LM (pba_solve) and the Ceres drop-in (real Ceres 2.0.0
  LM with include/pba_ceres.h over the engine) against the reference's CPU path (real Ceres with AutoDiff).
* C2 (configs[1]) — 50 keyframes of real EuRoC V1 image content, 8-px pattern, 20k blocks, double sphere: the Ceres
  drop-in against real Ceres on the CPU, iteration by iteration, with the evaluation-callback protocol checked on
  every call (evaluation_callback_test.cc:79-160).
* C5 (configs[4]) — the EuRoC V1 sequence is not in the container, so the C5 pieces run at full C4 size on rendered
  images: 21-px disk pattern, I_h,k sampled on the device, 3-level pyramid, fp16 records; sampled oracle parity at
  levels 2 and 0, fp16 within 2⁻¹¹ of fp32, and a coarse-to-fine LM (pba_solve_pyramid) that lowers the cost.
* C4 (configs[3]) — the headline problem, 1000 keyframes × 100k points × 8 px (400k blocks): sampled oracle parity
  over all hosts, full-size properties (validity, finiteness, cost = Σ½ρ(‖r‖²), the state-adopting launch
  bit-identical to set_state + evaluate, fp16 records within 2⁻¹¹), and one Gauss-Newton / LM iteration on rendered
  images (cost decreases; the cyclic-reduction step equals the band-Cholesky step to 1e-7).

Tolerances: records as tests/helpers.compare_records (north star 1e-5 relative).  LM trajectories: the GPU path
computes in fp32 (records) where the CPU path computes in fp64, so per-iteration costs agree to 1e-5 relative while
the accept/reject sequence must be identical.  Final states: the Ceres drop-in (fp32 records, Ceres' fp64 normal
equations) to 1e-5 m in the poses and 1e-4 of the inverse-distance scale; the engine's own solver (fp32 rows, fp64
JᵀJ block products and sums) to 1e-4 m and 1e-3 relative — it stops, like Ceres, at the first step whose cost change is
within the function tolerance, so the stopping state carries the step-size differences of the fp32 rows.
"""
import importlib
import os

import numpy as np
import pytest

import ceres_runner as CR
import gn_reference as GR
import oracle as O
from helpers import compare_records, engine_module, fp16_violations, projected_uv, synth

pytestmark = pytest.mark.gpu
E = engine_module()
THREADS = int(os.environ.get("OMP_NUM_THREADS", "8"))
needs_ceres = pytest.mark.skipif(not CR.available(), reason="oracle/_ref/ceres_lm_driver not built (oracle/ceres.mk)")


def make_engine(pb, huber, fixed=(0, 1)):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array(fixed, np.int32))
    eng.set_state(pb.poses, pb.rho)
    return eng


def assert_same_trajectory(a, b, cost_rtol=1e-5):
    """Two Ceres runs (real Ceres' Solver::Summary): the same accept/reject sequence and per-iteration costs."""
    assert len(a["costs"]) == len(b["costs"]), (a["message"], b["message"])
    assert np.array_equal(a["step_ok"], b["step_ok"])
    np.testing.assert_allclose(a["costs"], b["costs"], rtol=cost_rtol)
    assert a["termination"] == b["termination"]


# ---------------------------------------------------------------------------------------------------- C1
@pytest.fixture(scope="module")
def c1():
    pb = synth.c1_problem()
    pb.poses[:2] = pb.poses_gt[:2]
    return pb


def test_c1_records_match_oracle(c1):
    with make_engine(c1, 1.0) as eng:
        eng.evaluate(True)
        rec, valid = eng.records()
    ref, vref = O.evaluate(c1)
    st = compare_records(1, 2, rec, ref, valid, vref)
    assert valid.all(), st


@needs_ceres
def test_c1_engine_lm_matches_ceres_cpu(c1):
    """pba_solve (on-device Schur GN / LM) against the reference path: real Ceres LM (SPARSE_SCHUR) with AutoDiff."""
    ref = CR.run("cpu", c1, iters=20, huber=1.0, threads=THREADS)
    with make_engine(c1, 1.0) as eng:
        s = eng.solve(max_iterations=20)
        poses, rho = eng.get_state()
        traj = eng.solver_iterations()
    # the trajectory entry by entry (pba_solver_iterations against Solver::Summary::iterations): flags, costs, radii
    assert len(traj["cost"]) == len(ref["costs"]), (len(traj["cost"]), len(ref["costs"]), ref["message"])
    assert np.array_equal(traj["step_is_successful"].astype(bool), ref["step_ok"])
    np.testing.assert_allclose(traj["cost"], ref["costs"], rtol=1e-5)
    np.testing.assert_allclose(traj["trust_region_radius"], ref["radius"], rtol=1e-3)
    # Ceres counts iteration 0 (the initial evaluation) as a successful step
    assert s["successful_steps"] == ref["successful_steps"] - 1, (s, ref["message"])
    assert s["unsuccessful_steps"] == ref["unsuccessful_steps"]
    assert abs(s["initial_cost"] - ref["costs"][0]) <= 1e-6 * ref["costs"][0]
    assert abs(s["final_cost"] - ref["final_cost"]) <= 1e-5 * ref["final_cost"], (s, ref["final_cost"])
    dt, dq = np.abs(poses[:, 4:] - ref["poses"][:, 4:]).max(), np.abs(poses[:, :4] - ref["poses"][:, :4]).max()
    dr = (np.abs(rho - ref["rho"]) / np.abs(ref["rho"])).max()
    print(f"\nC1 engine LM vs Ceres: final cost {abs(s['final_cost'] - ref['final_cost']) / ref['final_cost']:.2e}, "
          f"max |Δt| {dt:.2e} m, max |Δq| {dq:.2e}, max Δρ/ρ {dr:.2e}")
    # measured (round 4): final cost 9.9e-9, |Δt| 2.7e-5 m, |Δq| 2.7e-8, Δρ/ρ 1.2e-5 — bounds ~4-40× above
    np.testing.assert_allclose(poses[:, 4:], ref["poses"][:, 4:], atol=1e-4)
    np.testing.assert_allclose(poses[:, :4], ref["poses"][:, :4], atol=1e-6)
    np.testing.assert_allclose(rho, ref["rho"], rtol=1e-4)


@needs_ceres
@pytest.mark.parametrize("pose_param", ["ref", "tangent"])
def test_c1_ceres_dropin_matches_ceres_cpu(c1, pose_param):
    """The north star's drop-in: the same ceres::Solve with the GPU EvaluationCallback + per-block CostFunctions.
    "ref": bundle_adjustment()'s own Sophus::test::LocalParameterizationSE3 stays registered (map_utils.h:331-333; the
    adapter emits J7 = J6·P⁺); "tangent": the adapter's SE3TangentParameterization."""
    ref = CR.run("cpu", c1, iters=20, huber=1.0, threads=THREADS)
    got = CR.run("gpu", c1, iters=20, huber=1.0, threads=THREADS, pose_param=pose_param)
    assert got["protocol"]["violations"] == 0, got["protocol"]
    assert_same_trajectory(got, ref)
    np.testing.assert_allclose(got["poses"][:, 4:], ref["poses"][:, 4:], atol=1e-5)
    np.testing.assert_allclose(got["rho"], ref["rho"], rtol=1e-4, atol=1e-4 * np.abs(ref["rho"]).max())


@needs_ceres
def test_c1_ceres_dropin_optimize_intrinsics(c1):
    """BundleAdjustmentOptions::optimize_intrinsics (map_utils.h:339-345): the cameras' intrinsics blocks are free, the
    functor differentiates the TARGET camera's intrinsics (reprojection.h:83-86, :108) and unprojects the host pixel with
    the intrinsics captured at problem build.  Real Ceres over the GPU adapter (target-intrinsics Jacobian from the
    engine) takes the CPU AutoDiff run's accept/reject sequence, costs to 1e-5, and moves the intrinsics the same way."""
    pb = synth.Problem(**{**c1.__dict__, "intrinsics": c1.intrinsics * np.array([1.002, 0.998, 1.0, 1.0, 1, 1, 1, 1])})
    ref = CR.run("cpu", pb, iters=20, huber=1.0, threads=THREADS, optimize_intrinsics=1)
    got = CR.run("gpu", pb, iters=20, huber=1.0, threads=THREADS, optimize_intrinsics=1)
    assert got["protocol"]["violations"] == 0, got["protocol"]
    assert_same_trajectory(got, ref)
    moved = np.abs(ref["intrinsics"] - pb.intrinsics).max()
    assert moved > 1e-3, moved  # the intrinsics are optimised, not held
    # the focal lengths trade off against the inverse distances (a weakly observed direction): the final intrinsics
    # agree to ~4e-7 relative, the distortion parameter near 0 to ~2e-7 absolute
    np.testing.assert_allclose(got["intrinsics"], ref["intrinsics"], rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(got["poses"][:, 4:], ref["poses"][:, 4:], atol=1e-5)


@needs_ceres
def test_c1_engine_lm_optimize_intrinsics_matches_ceres_cpu(c1):
    """The engine's own LM (pba_solve, on-device Schur GN) with free intrinsics (optimize_intrinsics, map_utils.h:339-345:
    the cameras' intrinsics blocks free, the functor's target-camera Jacobian, reprojection.h:83-86, :108) against real
    Ceres 2.0.0 on the CPU (AutoDiff, SPARSE_SCHUR with the intrinsics among the f-blocks): the same successful /
    unsuccessful step counts, the final cost to 1e-5, the intrinsics to 2e-6 relative (1e-6 absolute for the distortion
    parameter near 0), as test_c1_ceres_dropin_optimize_intrinsics holds the drop-in."""
    pb = synth.Problem(**{**c1.__dict__, "intrinsics": c1.intrinsics * np.array([1.002, 0.998, 1.0, 1.0, 1, 1, 1, 1])})
    ref = CR.run("cpu", pb, iters=20, huber=1.0, threads=THREADS, optimize_intrinsics=1)
    with make_engine(pb, 1.0) as eng:
        eng.set_optimize_intrinsics(True)
        s = eng.solve(max_iterations=20)
        k = eng.get_intrinsics()
        poses, _ = eng.get_state()
    print(f"\nC1 free intrinsics: engine {s['successful_steps']}/{s['unsuccessful_steps']} final {s['final_cost']:.10g}; "
          f"Ceres {ref['successful_steps'] - 1}/{ref['unsuccessful_steps']} final {ref['final_cost']:.10g} "
          f"({ref['message']}); intrinsics max rel {np.abs(k - ref['intrinsics']).max() / np.abs(ref['intrinsics']).max():.2e}")
    assert np.abs(ref["intrinsics"] - pb.intrinsics).max() > 1e-3  # Ceres moved them
    assert s["successful_steps"] == ref["successful_steps"] - 1, (s, ref["message"])
    assert s["unsuccessful_steps"] == ref["unsuccessful_steps"], (s, ref["message"])
    assert abs(s["initial_cost"] - ref["costs"][0]) <= 1e-6 * ref["costs"][0]
    assert abs(s["final_cost"] - ref["final_cost"]) <= 1e-5 * ref["final_cost"], (s["final_cost"], ref["final_cost"])
    np.testing.assert_allclose(k, ref["intrinsics"], rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(poses[:, 4:], ref["poses"][:, 4:], atol=1e-4)


@needs_ceres
def test_split_border_engine_lm_optimize_intrinsics_matches_ceres_cpu():
    """pba_solve with free intrinsics at the smallest size whose border takes the three-launch branch (128 keyframes ×
    4 cameras = 512 keyframe blocks, 1300 points, 5200 blocks, pinhole; enqueue_border) against real Ceres 2.0.0 on the
    CPU, ten iterations, with the assertions and tolerances of test_c1_engine_lm_optimize_intrinsics_matches_ceres_cpu.
    The rig's cameras differ by 1 % per camera; the intrinsics start 0.3 % / 0.2 % / 0.05 % off them and Ceres moves
    them by up to 0.077 px.
    Measured (MI355X): both 9 successful / 1 unsuccessful steps, initial cost 1.9e-8 and final cost
    1.7e-8 relative, intrinsics 3.8e-9 of their scale."""
    pb0 = synth.make_problem(kind=1, n_frames=128, n_points=1300, width=376, height=240, seed=65, border=12)
    intr = np.stack([pb0.intrinsics[0] * np.array([1 + 0.01 * c, 1 - 0.01 * c, 1, 1, 1, 1, 1, 1]) for c in range(4)])
    pb = synth.make_problem(kind=1, n_frames=128, n_points=1300, width=376, height=240, seed=65, border=12,
                            intrinsics=intr, frame_cam=(np.arange(128) % 4).astype(np.int32), obs_sigma=0.3)
    pb.poses[:2] = pb.poses_gt[:2]
    pb = synth.Problem(**{**pb.__dict__, "intrinsics": intr * np.array([1.003, 0.998, 1.0005, 0.9995, 1, 1, 1, 1])})
    assert pb.n_frames * pb.intrinsics.shape[0] >= 512
    ref = CR.run("cpu", pb, iters=10, huber=1.0, threads=THREADS, optimize_intrinsics=1)
    with make_engine(pb, 1.0) as eng:
        eng.set_optimize_intrinsics(True)
        s = eng.solve(max_iterations=10)
        k = eng.get_intrinsics()
    print(f"\nsplit-border free intrinsics: engine {s['successful_steps']}/{s['unsuccessful_steps']} final "
          f"{s['final_cost']:.10g}; Ceres {ref['successful_steps'] - 1}/{ref['unsuccessful_steps']} final "
          f"{ref['final_cost']:.10g} ({ref['message']}); initial cost rel "
          f"{abs(s['initial_cost'] - ref['costs'][0]) / ref['costs'][0]:.2e}, final cost rel "
          f"{abs(s['final_cost'] - ref['final_cost']) / ref['final_cost']:.2e}, intrinsics max rel "
          f"{np.abs(k - ref['intrinsics']).max() / np.abs(ref['intrinsics']).max():.2e}, Ceres moved them "
          f"{np.abs(ref['intrinsics'] - pb.intrinsics).max():.2e}")
    assert np.abs(ref["intrinsics"] - pb.intrinsics).max() > 1e-3  # Ceres moved them
    assert s["successful_steps"] == ref["successful_steps"] - 1, (s, ref["message"])
    assert s["unsuccessful_steps"] == ref["unsuccessful_steps"], (s, ref["message"])
    assert abs(s["initial_cost"] - ref["costs"][0]) <= 1e-6 * ref["costs"][0]
    assert abs(s["final_cost"] - ref["final_cost"]) <= 1e-5 * ref["final_cost"], (s["final_cost"], ref["final_cost"])
    np.testing.assert_allclose(k, ref["intrinsics"], rtol=2e-6, atol=1e-6)


@needs_ceres
def test_c1_free_intrinsics_without_engine_support_is_refused(c1):
    """Free intrinsics blocks with an evaluator that was not given them: the adapter refuses the Jacobian request
    (Evaluate returns false) and Ceres ends with FAILURE, instead of optimising with a zero intrinsics gradient."""
    got = CR.run("gpu", c1, iters=5, huber=1.0, threads=THREADS, optimize_intrinsics=2)
    assert got["refused_intrinsics"] == 1
    assert got["termination"] == 2, got["message"]  # ceres::FAILURE
    assert not (got["step_ok"][1:]).any()


def _pick_threshold(values, earlier_ratio):
    """first index k ≥ 1 whose value is below every earlier one by the given factor"""
    for k in range(1, len(values)):
        if np.isfinite(values[k]) and values[k] * earlier_ratio < np.min(values[:k]):
            return k
    return None


@needs_ceres
def test_c1_engine_lm_stops_like_ceres_on_parameter_and_gradient_tolerance(c1):
    """pba_solve's ParameterToleranceReached / GradientToleranceReached (trust_region_minimizer.cc:668-728) against
    real Ceres LM on the CPU path: tolerances chosen from Ceres' own per-iteration step and gradient norms (margin
    ≥ 1.5×), then both solvers must stop by the same test with the same step counts and final cost."""
    base = CR.run("cpu", c1, iters=20, huber=1.0, threads=THREADS, ptol=0.0, gtol=0.0, ftol=0.0)
    x_norm = np.sqrt((base["poses"][2:] ** 2).sum() + (base["rho"] ** 2).sum())
    ok = base["step_ok"]
    # parameter tolerance: valid steps (accepted or not; step_norm > 0) after the first accepted one (x_norm is −1
    # before it)
    first = 1 + int(np.argmax(ok[1:]))
    sn = base["step_norm"][first + 1:]
    ratios = sn[sn > 0] / x_norm
    k = _pick_threshold(ratios, 1.5)
    assert k is not None, ratios
    ptol = 1.2 * ratios[k]
    gn = np.where(ok, base["gradient_max_norm"], np.inf)
    kg = _pick_threshold(gn, 2.0)
    assert kg is not None, gn
    gtol = 1.4 * gn[kg]
    for name, kw, reason in (("ptol", {"ptol": ptol}, "parameter_tolerance"),
                             ("gtol", {"gtol": gtol}, "gradient_tolerance")):
        ref = CR.run("cpu", c1, iters=20, huber=1.0, threads=THREADS, **kw)
        assert ref["termination"] == 0 and reason.split("_")[0] in ref["message"].lower(), (name, ref["message"])
        opts = {"parameter_tolerance": ptol} if name == "ptol" else {"gradient_tolerance": gtol}
        with make_engine(c1, 1.0) as eng:
            s = eng.solve(max_iterations=20, **opts)
        assert s["stop_reason"] == reason, (name, s, ref["message"])
        assert s["successful_steps"] == ref["successful_steps"] - 1, (name, s, ref["message"])
        assert s["unsuccessful_steps"] == ref["unsuccessful_steps"], (name, s)
        assert abs(s["final_cost"] - ref["final_cost"]) <= 1e-5 * ref["final_cost"], (name, s, ref["final_cost"])


# ---------------------------------------------------------------------------------------------------- C2
@pytest.fixture(scope="module")
def c2():
    pb = synth.c2_problem()
    pb.poses[:2] = pb.poses_gt[:2]
    return pb


def test_c2_records_match_oracle(c2):
    with make_engine(c2, 9.0) as eng:
        eng.evaluate(True)
        rec, valid = eng.records()
    ref, vref = O.evaluate(c2)
    compare_records(0, 8, rec, ref, valid, vref, projected_uv(c2))


@needs_ceres
def test_c2_ceres_dropin_matches_ceres_cpu(c2):
    """C2 = "Ceres LM + GPU EvaluationCallback": real Ceres' LM over the engine against real Ceres' LM over AutoDiff
    of the restated functor, on real EuRoC image content.  The callback protocol holds on every call, and the
    trust-region sequence has residual-only candidates ("rn") followed, after an accepted step, by a Jacobian
    evaluation at the same point ("Js")."""
    ref = CR.run("cpu", c2, iters=12, huber=9.0, threads=THREADS)
    got = CR.run("gpu", c2, iters=12, huber=9.0, threads=THREADS)
    p = got["protocol"]
    assert p["violations"] == 0, p
    log = [p["log"][i:i + 2] for i in range(0, len(p["log"]), 2)]
    assert log[0] == "Jn" and "rn" in log and "Js" in log, log
    for a, b in zip(log, log[1:]):
        if b == "Js":
            assert a == "rn", log  # an accepted candidate is re-evaluated with Jacobians at the same point
    assert_same_trajectory(got, ref)
    assert got["costs"][-1] < 0.2 * got["costs"][0]
    np.testing.assert_allclose(got["poses"][:, 4:], ref["poses"][:, 4:], atol=1e-5)
    np.testing.assert_allclose(got["rho"], ref["rho"], rtol=1e-4, atol=1e-4 * np.abs(ref["rho"]).max())
    # the end-to-end rate of the drop-in (Ceres' own timers), for the record
    print(f"\nC2 Ceres drop-in: {got['jacobian_evaluations']} J evaluations in {got['jacobian_evaluation_s']:.3f} s "
          f"(CPU AutoDiff {ref['jacobian_evaluation_s']:.3f} s on {ref['threads']} threads)")


@needs_ceres
def test_c2_floor_replays_the_dropin_trajectory(c2):
    """The bench's C2 floor (ceres_lm_driver floor): the drop-in's Solve recorded, then replayed over the recorded
    read-backs.  The replay must make exactly the recorded evaluations (same trajectory, same Jacobian and residual
    evaluation counts, bit-identical costs: the same values reach Ceres), so its timers are the drop-in's own minus the
    device's part."""
    got = CR.run("gpu", c2, iters=10, huber=9.0, threads=THREADS, check=False)
    fl = CR.run("floor", c2, iters=10, huber=9.0, threads=THREADS)
    assert fl["replay_ok"] == 1
    assert fl["jacobian_evaluations"] == got["jacobian_evaluations"]
    assert fl["residual_evaluations"] == got["residual_evaluations"]
    assert np.array_equal(fl["step_ok"], got["step_ok"])
    np.testing.assert_allclose(fl["costs"], got["costs"], rtol=1e-7)  # (two runs: Ceres' threaded sums differ ~1e-9)
    print(f"\nC2 floor: J evaluation {1e3 * fl['jacobian_evaluation_s'] / fl['jacobian_evaluations']:.3f} ms vs drop-in "
          f"{1e3 * got['jacobian_evaluation_s'] / got['jacobian_evaluations']:.3f} ms")


# ---------------------------------------------------------------------------------------------------- C4
@pytest.fixture(scope="module")
def c4():
    import torch
    pb, images = synth.c4_shard(torch.device("cuda", 0))
    return pb, images


def test_c4_full_size_parity_and_properties(c4):
    import torch
    pb, images = c4
    assert pb.n_blocks == 400000 and pb.n_frames == 1004
    rng = np.random.default_rng(3)
    states = []
    for _ in range(2):
        poses = synth.se3_plus(pb.poses, 1e-3 * rng.normal(0, 1, (pb.n_frames, 6)))
        rho = pb.rho * (1 + 0.01 * rng.normal(0, 1, pb.n_points))
        states.append((torch.from_numpy(poses).cuda(), torch.from_numpy(rho).cuda(), poses, rho))
    with E.Engine(0, 0, huber_width=9.0) as eng:
        eng.set_problem(pb, images_device_ptr=images.data_ptr())
        # (1) the one-launch state-adopting evaluation …
        eng.evaluate_state_device(states[1][0].data_ptr(), states[1][1].data_ptr(), True)
        rec_a, valid_a = eng.records()
        cost_a = eng.block_costs()
        # … is bit-identical to set_state_device + evaluate
        eng.set_state_device(states[0][0].data_ptr(), states[0][1].data_ptr())
        eng.evaluate(True)
        eng.set_state_device(states[1][0].data_ptr(), states[1][1].data_ptr())
        eng.evaluate(True)
        rec_b, valid_b = eng.records()
        assert np.array_equal(valid_a, valid_b) and np.array_equal(rec_a.view(np.uint32), rec_b.view(np.uint32))
        # fp16 records: every value within 2⁻¹¹ relative + 2⁻¹⁴ absolute of the fp32 record
        eng.set_record_format(E.RECORD_F16)
        eng.evaluate(True)
        rec_h, valid_h = eng.records()
    assert np.array_equal(valid_h, valid_a)
    at1 = synth.Problem(**{**pb.__dict__, "poses": states[1][2], "rho": states[1][3]})
    bad = fp16_violations(rec_h, rec_a, projected_uv(at1), 8)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        pytest.fail(f"fp16 records: {bad.sum()} values out of bound, max|fp32| {np.abs(rec_a).max():.4g}, "
                    f"columns {np.unique(np.nonzero(bad)[1])[:20]}, e.g. [{i},{j}] {rec_a[i, j]!r} -> {rec_h[i, j]!r}")
    # full size: every block valid (targets are 1-4 keyframes ahead, points well inside), all finite
    assert valid_a.all() and np.isfinite(rec_a).all()
    # per-block cost = ½ρ(Σr²) from the record's residuals (Huber 9, loss_function.cc:48-62)
    r = rec_a[:, :8].astype(np.float64)
    s = (r * r).sum(1)
    c_ref = np.where(s <= 81.0, 0.5 * s, 0.5 * (2 * 9.0 * np.sqrt(s) - 81.0))
    np.testing.assert_allclose(cost_a, c_ref, rtol=2e-6, atol=1e-4)
    # sampled oracle parity: 4096 blocks spread over all 1000 hosts
    sel = np.linspace(0, pb.n_blocks - 1, 4096).astype(np.int64)
    assert len(np.unique(pb.point_host[pb.block_point[sel]])) >= 900
    sub = synth.Problem(**{**pb.__dict__, "images": images.cpu().numpy(), "block_point": pb.block_point[sel],
                           "block_target": pb.block_target[sel], "poses": states[1][2], "rho": states[1][3]})
    ref, vref = O.evaluate(sub)
    compare_records(0, 8, rec_a[sel], ref, valid_a[sel], vref, projected_uv(sub))


def test_c4_gauss_newton_iteration_on_rendered_images(monkeypatch):
    """One LM iteration of the on-device Schur GN at full C4 size on rendered images: the block-cyclic-reduction
    step equals the band-Cholesky step to 1e-7, the reduced system is finite, and the accepted step lowers the cost."""
    import torch
    pb, images = synth.c4_shard(torch.device("cuda", 0), texture="render")
    steps = {}
    for solver in ("cr", "band"):
        monkeypatch.setenv("PBA_SOLVER", solver)
        with E.Engine(0, 0, huber_width=9.0) as eng:
            eng.set_problem(pb, images_device_ptr=images.data_ptr())
            eng.set_fixed_frames(np.array([0, 1], np.int32))
            eng.set_state(pb.poses, pb.rho)
            c0 = eng.gn_linearize()
            m, st = eng.gn_step(1e-4)
            assert st == 0 and m > 0
            steps[solver] = eng.gn_last_step()
            c1 = eng.gn_candidate_cost()
            if solver == "cr":
                eng.set_state(pb.poses, pb.rho)
                s = eng.solve(max_iterations=1)
                assert s["successful_steps"] == 1 and s["final_cost"] < s["initial_cost"], s
        assert np.isfinite(steps[solver][0]).all() and np.isfinite(steps[solver][1]).all()
        assert c1 < c0, (solver, c0, c1)
    for a, b in zip(steps["cr"], steps["band"]):
        assert np.linalg.norm(a - b) <= 1e-7 * np.linalg.norm(b)


@pytest.fixture(scope="module")
def c4_render():
    """The C4 problem on rendered images (the plane every keyframe sees: LM converges), with its images copied to the
    host for the fp64 references."""
    import torch
    pb, images = synth.c4_shard(torch.device("cuda", 0), texture="render")
    pbh = synth.Problem(**{**pb.__dict__, "images": images.cpu().numpy()})
    return pbh, images


def c4_engine(pbh, images):
    eng = E.Engine(0, 0, huber_width=9.0)
    eng.set_problem(pbh, images_device_ptr=images.data_ptr())
    eng.set_fixed_frames(np.array([0, 1], np.int32))
    eng.set_state(pbh.poses, pbh.rho)
    return eng


@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_c4_reduced_system_and_step_against_fp64_reference(c4_render, lam):
    """At full C4 size (1004 keyframes, 400k blocks, rendered images): the device's reduced camera system S, its
    right-hand side and the pose step against the fp64 system built block-sparsely from the oracle's Jacobians
    (gn_reference.reduced_system_sparse: the quantities of schur_complement_solver.cc:138-146) and its dense fp64 solve
    (6024 unknowns).  The device forms the JᵀJ block products of its fp32 rows on the fp64 matrix cores
    (v_mfma_f64_4x4x4f64, round 5) and sums them in fp64.  Measured (MI355X, round 5): cost 1.5e-8; S 5.3e-8 / 5.5e-8 and
    g 6.9e-8 / 6.8e-8 of their scale at λ = 1e-4 / 0.1; the step 3.0e-7 relative at λ = 1e-4 (|δ| = 0.93) and 4.7e-8 at
    λ = 0.1.  (Round 4's fp32 block products gave 3.0e-5 / 1.3e-7: the weakly damped system amplified their rounding.)
    Bounds: cost, S, g 1e-6 of scale; step the north star's 1e-5 (λ = 1e-4) and 1e-6 (λ = 0.1) relative."""
    pbh, images = c4_render
    fixed = (0, 1)
    S_ref, g_ref, c_ref = GR.reduced_system_sparse(pbh, pbh.poses, pbh.rho, 9.0, lam, fixed)
    dp_ref = np.linalg.solve(S_ref, -g_ref)
    with c4_engine(pbh, images) as eng:
        c = eng.gn_linearize()
        _, st = eng.gn_step(lam)
        assert st == 0
        S, g = eng.gn_reduced_system()
        dp, _ = eng.gn_last_step()
    eS = np.abs(S - S_ref).max() / np.abs(S_ref).max()
    eg = np.abs(g - g_ref).max() / np.abs(g_ref).max()
    ep = np.linalg.norm(dp.ravel() - dp_ref) / np.linalg.norm(dp_ref)
    ec = abs(c - c_ref) / c_ref
    print(f"\nC4 λ={lam}: cost {ec:.2e}, S {eS:.2e}, g {eg:.2e}, step {ep:.2e} (|step| {np.linalg.norm(dp_ref):.3e})")
    assert ec <= 1e-6
    assert eS <= 1e-6, eS
    assert eg <= 1e-6, eg
    assert ep <= (1e-5 if lam < 1e-2 else 1e-6), ep


@pytest.fixture(scope="module")
def c4_lm(c4_render):
    """The reference's whole bundle-adjustment solve at full C4 size, both ways, each trajectory from ONE solve:
    pba_solve (pba_solver_iterations) and real Ceres 2.0.0 LM (SPARSE_SCHUR, AutoDiff over the restated photometric
    functor, the reference's LocalParameterizationSE3, 2 constant keyframes; Solver::Summary::iterations), with
    BundleAdjustmentOptions' max_num_iterations = 20 (map_utils.h:318, sfm.cpp:1910) and Ceres' default tolerances.
    Plus the engine's iterates: the state after k = 0 … 19 iterations (pba_solve of k iterations from the same initial
    state — bit-reproducible, so the prefix of the 20-iteration solve) with the trust-region radius it carries."""
    pbh, images = c4_render
    iters = 20
    ref = CR.run("cpu", pbh, iters=iters, huber=9.0, threads=THREADS, timeout=1500)
    states = []
    with c4_engine(pbh, images) as eng:
        summ = eng.solve(max_iterations=iters)
        traj = eng.solver_iterations()
        for k in range(iters):
            eng.set_state(pbh.poses, pbh.rho)
            sk = eng.solve(max_iterations=k)
            tk = eng.solver_iterations()
            # the prefix of the 20-iteration solve, bit for bit
            assert np.array_equal(tk["cost"], traj["cost"][:k + 1]), k
            poses, rho = eng.get_state()
            states.append((poses, rho, traj["trust_region_radius"][k]))
    return pbh, ref, summ, traj, states


@needs_ceres
def test_c4_engine_lm_matches_ceres_cpu_free_running(c4_lm):
    """The two 20-iteration solves side by side.  They take the same steps with the same costs (the north star's 1e-5
    relative) until the trajectories part: once the trust region has grown (radius 2e8 at iteration 10, λ = 5e-9: an
    almost undamped step; the reduced system's condition number is ~1e11) this problem amplifies any difference in the
    iterates by ~×10 per iteration — real Ceres against itself with 16 and 3 threads (fp64, only the summation order
    differs) goes 2e-15 → 1e-8 over the 20 iterations (test_c4_lm_step_sensitivity_and_fp64_products), and the engine's
    rows are fp32 (the north star's precision: records within 1e-5 of the fp64 functor), 1.5e-8 in the initial cost.
    Measured (round 5, fp64 normal equations): costs ≤ 1.6e-6 relative through iteration 9, 0.6-1.5e-5 at 10, 1.3e-4 at
    11; accept flags identical through iteration 15 (round 4's fp32 normal equations: 5.7e-5 at iteration 8).  Asserted:
    iterations 0-9 within 1e-5 and iteration 10 within 1e-4, with identical accept flags, the initial cost within 3e-8.
    Every one of the 20 iterations is pinned from the engine's own iterates in the next test."""
    pbh, ref, summ, traj, _ = c4_lm
    n = min(len(traj["cost"]), len(ref["costs"]))
    rel = np.abs(traj["cost"][:n] - ref["costs"][:n]) / np.abs(ref["costs"][:n])
    rows = [f"{k:2d} {'+' if traj['step_is_successful'][k] else '-'}{'+' if ref['step_ok'][k] else '-'} "
            f"{traj['cost'][k]:.10e} {ref['costs'][k]:.10e} {rel[k]:.2e} radius {traj['trust_region_radius'][k]:.3e} / "
            f"{ref['radius'][k]:.3e} step {traj['step_norm'][k]:.3e} / {ref['step_norm'][k]:.3e}" for k in range(n)]
    print(f"\nC4 LM, 20 iterations: engine {summ['successful_steps']}/{summ['unsuccessful_steps']} "
          f"({summ['stop_reason']}), Ceres {ref['successful_steps'] - 1}/{ref['unsuccessful_steps']} ({ref['message']})\n"
          "it ok(engine,Ceres) engine cost / Ceres cost / relative difference\n" + "\n".join(rows))
    assert len(traj["cost"]) == 21 and len(ref["costs"]) == 21
    assert rel[0] <= 3e-8, rel[0]
    assert np.array_equal(traj["step_is_successful"][:11].astype(bool), ref["step_ok"][:11])
    assert rel[:10].max() <= 1e-5 and rel[10] <= 1e-4, rel[:11]


@needs_ceres
@pytest.mark.timeout(1500)
def test_c4_every_engine_iteration_matches_a_ceres_iteration(c4_lm):
    """Every one of the engine's 20 LM iterations against Ceres' own iteration from the same point: from the engine's
    iterate k (state and trust-region radius), real Ceres runs ONE LM iteration (ceres_lm_driver teacher mode:
    Solver::Options::initial_trust_region_radius = the engine's radius) and must take the engine's decision at iteration
    k + 1 — accept or reject — with the cost at the iterate within 3e-8 (fp32 residuals) and the cost after the iteration
    (the new state's, or the rejected candidate's) within the north star's 1e-5 relative at every iteration, λ down to
    5.6e-10.  Measured (round 5, fp64 normal equations): all 20 decisions identical, step norms to 5 digits; costs after
    the iteration ≤ 2.7e-8 through iteration 10 (λ ≥ 5e-9) and ≤ 4.7e-7 over all 20 (the largest on the rejected
    candidates of the almost undamped iterations 12 and 15)."""
    pbh, ref, summ, traj, states = c4_lm
    t = CR.run("cpu", pbh, iters=1, huber=9.0, threads=THREADS, timeout=2400, teacher=states)["teacher"]
    assert t.shape[0] == len(states)
    cur = traj["cost"][0]
    rows, bad = [], []
    for k in range(len(states)):
        e_ok = bool(traj["step_is_successful"][k + 1])
        c_ok = bool(t[k, 2]) and t[k, 6] == 2
        e_before, e_after = cur, traj["cost"][k + 1]
        r0 = abs(e_before - t[k, 0]) / t[k, 0]
        r1 = abs(e_after - t[k, 1]) / abs(t[k, 1])
        rows.append(f"{k + 1:2d} {'+' if e_ok else '-'}{'+' if c_ok else '-'} at {r0:.1e} after {r1:.2e} "
                    f"(engine {e_after:.10e}, Ceres {t[k, 1]:.10e}) radius {states[k][2]:.3e} λ {1 / states[k][2]:.2e} "
                    f"step {traj['step_norm'][k + 1]:.4e} / {t[k, 5]:.4e}")
        if e_ok != c_ok or r0 > 3e-8 or r1 > 1e-5:
            bad.append(k + 1)
        if e_ok:
            cur = e_after
    print("\nC4 LM, each engine iteration against one Ceres iteration from the engine's iterate:\n" + "\n".join(rows))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- C5
DISK21 = np.array([(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if dx * dx + dy * dy <= 5], np.float32)


def test_c5_style_full_size_pyramid_fp16():
    """C5's configuration on the C4 problem (1004 keyframes, 400k blocks, rendered plane): 21-px pattern with the host
    intensities sampled on the device, a 3-level pyramid, fp16 records.  At levels 2 and 0: 4096 blocks over all hosts
    against the oracle evaluating that level's problem (fp32 records), every block valid and finite, and the fp16
    records within 2⁻¹¹ relative + 2⁻¹⁴ absolute of the fp32 ones; then the coarse-to-fine LM lowers the cost."""
    import torch
    pb, images = synth.c4_shard(torch.device("cuda", 0), texture="render")
    pb5 = synth.Problem(**{**pb.__dict__, "pattern": DISK21, "host_intensity": None})
    P = DISK21.shape[0]
    sel = np.linspace(0, pb.n_blocks - 1, 4096).astype(np.int64)
    imgs = images.cpu().numpy()
    with E.Engine(0, 0, huber_width=9.0) as eng:
        eng.set_problem(pb5, images_device_ptr=images.data_ptr())
        eng.set_fixed_frames(np.array([0, 1], np.int32))
        eng.set_state(pb.poses, pb.rho)
        eng.build_pyramid(3)
        for level in (2, 0):
            eng.set_level(level)
            eng.set_record_format(E.RECORD_F32)
            eng.evaluate(True)
            r32, v32 = eng.records()
            hi = eng.host_intensities()
            eng.set_record_format(E.RECORD_F16)
            eng.evaluate(True)
            r16, v16 = eng.records()
            assert v32.all() and np.array_equal(v16, v32) and np.isfinite(r32).all(), level
            full = synth.Problem(**{**pb5.__dict__, "images": imgs})
            lp = synth.level_problem(full, level, host_intensity=hi)
            bad = fp16_violations(r16, r32, projected_uv(lp), P)
            if bad.any():
                i, j = np.argwhere(bad)[0]
                pytest.fail(f"level {level}: {bad.sum()} fp16 values out of bound, columns "
                            f"{np.unique(np.nonzero(bad)[1])[:20]}, e.g. [{i},{j}] {r32[i, j]!r} -> {r16[i, j]!r}, "
                            f"max|fp32| over them {np.abs(r32[bad]).max():.6g}, non-finite fp16 {(~np.isfinite(r16)).sum()}")
            sub = synth.Problem(**{**lp.__dict__, "block_point": pb.block_point[sel], "block_target": pb.block_target[sel]})
            ref, vref = O.evaluate(sub)
            compare_records(0, P, r32[sel], ref, v32[sel], vref, projected_uv(sub))
        eng.set_record_format(E.RECORD_F32)
        s = eng.solve_pyramid(max_iterations=4)
        assert eng.level()[0] == 0
    assert s["final_cost"] < s["initial_cost"], s


@needs_ceres
@pytest.mark.timeout(1500)
def test_c4_lm_step_sensitivity_and_fp64_products(c4_lm, c4_render):
    """Why the free-running C4 trajectories part (after iteration 10 since round 5; after 7 with round 4's fp32 block
    products), measured at the engine's iterates k (its state and λ = 1/radius):
      * the device step (fp32 rows from the linearisation, fp64 JᵀJ block products on the fp64 matrix cores, fp64
        sums) — step_dev;
      * the same engine's fp32 records with every product and sum in fp64 — step_f64p: what fp64 matrix-core products
        (v_mfma_f64_16x16x4f64) in linearize_kernel would give, since its rows are these fp32 rows;
      * the oracle's fp64 records in fp64 — step_ref (the reference's arithmetic).
    If |step_f64p − step_ref| ≈ |step_dev − step_ref| the fp32 JᵀJ products are not what separates the engine from the
    fp64 reference: the fp32 rows are (the north star's fp32 evaluation), amplified by the weakly damped system.  The
    reference itself is that sensitive: real Ceres against itself with THREADS and 3 threads (fp64, only the summation
    order differs) is printed beside it.  Measured (round 5): with round 4's fp32 products the device step was off by 3e-5,
    2e-3, 0.13, 1.0 at iterates 0, 4, 8, 11 where fp64 products over the same rows gave 1.8e-6, 1.1e-5, 5.1e-5, 2.5e-4 —
    the fp32 JᵀJ rounding was the cause, so the normal equations are fp64 now.  With them (the final round-5 build) the
    device step is 3.0e-7, 1.2e-6, 4.5e-6, 1.7e-6, 4.9e-6 from the reference at iterates 0, 4, 8, 11, 16 — 6-100× closer
    than the fp64-product emulation over the evaluation kernel's rows (1.8e-6 … 1.8e-4): the linearisation's rows are
    the closer ones.  Asserted: the device step within 4× of the emulation's error and 1e-5 of the reference at every
    iterate (the north star's bound)."""
    pbh, images = c4_render
    _, ref, _, traj, states = c4_lm
    rows, ratios, devs = [], [], []
    with c4_engine(pbh, images) as eng:
        for k in (0, 4, 8, 11, 16):
            poses, rho, radius = states[k]
            lam = 1.0 / radius
            eng.set_state(poses, rho)
            eng.gn_linearize()
            _, st = eng.gn_step(lam)
            dp_dev = eng.gn_last_step()[0].ravel() if st == 0 else None
            S_d, g_d = eng.gn_reduced_system()
            eng.set_state(poses, rho)
            eng.evaluate(True)
            rec32, v32 = eng.records()
            at = synth.Problem(**{**pbh.__dict__, "poses": poses, "rho": rho})
            S_a, g_a, _ = GR.reduced_system_from_records(at, rec32, v32, 9.0, lam, (0, 1))
            S_r, g_r, _ = GR.reduced_system_sparse(at, poses, rho, 9.0, lam, (0, 1))
            dp_a = np.linalg.solve(S_a, -g_a)
            dp_r = np.linalg.solve(S_r, -g_r)
            dp_s = np.linalg.solve(S_d, -g_d)  # the device's system, solved in fp64 on the host
            nr = np.linalg.norm(dp_r)
            err = lambda x: np.linalg.norm(x - dp_r) / nr if x is not None else float("nan")
            e_dev, e_a, e_s = err(dp_dev), err(dp_a), err(dp_s)
            eS = np.abs(S_d - S_r).max() / np.abs(S_r).max()
            eSa = np.abs(S_a - S_r).max() / np.abs(S_r).max()
            w = np.linalg.eigvalsh(S_r)
            ratios.append(e_s / max(e_a, 1e-300))
            devs.append(e_dev)
            rows.append(f"iterate {k:2d} λ {lam:.2e} |step| {nr:.3e} cond(S) {w[-1] / w[0]:.2e}: device step−ref "
                        f"{e_dev:.2e} (solver status {st}), device S solved in fp64−ref {e_s:.2e}, fp64 products over the fp32 "
                        f"rows−ref {e_a:.2e}; S error device {eS:.2e}, fp64 products {eSa:.2e}")
    other = CR.run("cpu", pbh, iters=20, huber=9.0, threads=3, timeout=2400)
    m = min(len(other["costs"]), len(ref["costs"]))
    rc = np.abs(other["costs"][:m] - ref["costs"][:m]) / np.abs(ref["costs"][:m])
    print("\nC4 step sensitivity (pose steps, relative to the fp64 reference step):\n" + "\n".join(rows) +
          f"\nCeres {THREADS} vs 3 threads, per-iteration cost: " + " ".join(f"{x:.1e}" for x in rc) +
          f"\n  accept flags equal: {np.array_equal(other['step_ok'][:m], ref['step_ok'][:m])}")
    assert max(ratios) <= 4.0, ratios
    assert max(devs) <= 1e-5, devs
