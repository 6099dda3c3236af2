"""GPU parity of the on-device Gauss-Newton path (normal equations, Schur complement, skyline Cholesky,
LM loop) against the dense double-precision reference in tests/gn_reference.py (oracle Jacobians).

Tolerances: the device accumulates JᵀJ from fp32 rows (fp32 workgroup partials, fp64 across
workgroups), so S and g are compared relative to their scale: max|ΔS| ≤ 1e-4·max|S|, max|Δg| ≤ 1e-4·max|g|;
steps relative to their norm ≤ 1e-3 (the reduced system's conditioning amplifies the fp32 rounding);
LM runs must reach the same final cost within 1e-3 relative and the same poses within 1e-5 m / rad.
"""
import numpy as np
import pytest

import ceres_runner as CR
import gn_reference as GR
from helpers import engine_module, synth

pytestmark = pytest.mark.gpu
E = engine_module()
THREADS = int(__import__("os").environ.get("OMP_NUM_THREADS", "8"))


def make_engine(pb, huber, fixed, library=None):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber, library=library)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array(fixed, np.int32))
    eng.set_state(pb.poses, pb.rho)
    return eng


CASES = [(0, 0, 9.0), (0, 1, 9.0), (0, 2, 0.0), (0, 3, 9.0), (1, 0, 1.0), (1, 1, 1.0), (1, 3, 1.0),
         (0, 6, 9.0)]  # 6 = EUCM (2) + 4 · bicubic: PhotometricError<8>'s residual in the Gauss-Newton path


@pytest.mark.parametrize("kind,model,huber", CASES)
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_reduced_system_and_step(kind, model, huber, lam):
    interp, model = model >> 2, model & 3
    pb = synth.make_problem(kind=kind, model=model, n_frames=8, n_points=60, width=376, height=240, seed=11 + model,
                            border=12)
    pb.interp = interp
    fixed = (0,)
    H, g, cost = GR.linearize(pb, pb.poses, pb.rho, huber, fixed)
    S_ref, gS_ref, dp_ref, dl_ref, model_ref = GR.schur_step(H, g, pb.n_frames, lam, fixed)
    with make_engine(pb, huber, fixed) as eng:
        c = eng.gn_linearize()
        model_dec, st = eng.gn_step(lam)
        assert st == 0
        S, gS = eng.gn_reduced_system()
        dp, dl = eng.gn_last_step()
    assert abs(c - cost) <= 1e-5 * cost + 1e-6
    # S holds λ-damped diagonal; compare as assembled
    assert np.abs(S - S_ref).max() <= 1e-4 * np.abs(S_ref).max(), np.abs(S - S_ref).max()
    assert np.abs(gS - gS_ref).max() <= 1e-4 * np.abs(gS_ref).max() + 1e-9
    assert np.linalg.norm(dp - dp_ref) <= 1e-3 * np.linalg.norm(dp_ref) + 1e-12
    assert np.linalg.norm(dl - dl_ref) <= 1e-3 * np.linalg.norm(dl_ref) + 1e-12
    assert abs(model_dec - model_ref) <= 1e-3 * abs(model_ref) + 1e-9


@pytest.mark.parametrize("P,pm", [(12, 0), (21, 0), (32, 0), (21, 1), (17, 2), (21, 3), (21, 6), (30, 5)])
def test_reduced_system_large_patterns(P, pm):
    """Patterns beyond 8 px (linearize_adj_kernel<·, PPL>: 8 lanes per block, 2-4 rows per lane; the multi-pixel
    candidate-cost kernel) for every camera model and both interpolators (pm = model + 4 · interpolator): reduced
    system, step and candidate cost against the dense reference, same tolerances as above."""
    pat = np.random.default_rng(P).integers(-3, 4, (P, 2)).astype(np.float32)
    interp, model = pm >> 2, pm & 3
    pb = synth.make_problem(model=model, n_frames=8, n_points=60, width=376, height=240, pattern=pat, seed=40 + P + pm,
                            border=12)
    pb.interp = interp
    fixed = (0,)
    lam = 1e-3
    H, g, cost = GR.linearize(pb, pb.poses, pb.rho, 9.0, fixed)
    S_ref, gS_ref, dp_ref, dl_ref, model_ref = GR.schur_step(H, g, pb.n_frames, lam, fixed)
    with make_engine(pb, 9.0, fixed) as eng:
        c = eng.gn_linearize()
        model_dec, st = eng.gn_step(lam)
        assert st == 0
        S, gS = eng.gn_reduced_system()
        dp, dl = eng.gn_last_step()
        c_new = eng.gn_candidate_cost()
    assert abs(c - cost) <= 1e-5 * cost + 1e-6
    assert np.abs(S - S_ref).max() <= 1e-4 * np.abs(S_ref).max()
    assert np.abs(gS - gS_ref).max() <= 1e-4 * np.abs(gS_ref).max() + 1e-9
    assert np.linalg.norm(dp - dp_ref) <= 1e-3 * np.linalg.norm(dp_ref) + 1e-12
    assert abs(model_dec - model_ref) <= 1e-3 * abs(model_ref) + 1e-9
    np_, nr = GR.apply_step(pb.poses, pb.rho, dp, dl)
    _, _, cost_new_ref = GR.linearize(pb, np_, nr, 9.0, fixed)
    assert abs(c_new - cost_new_ref) <= 1e-5 * cost_new_ref + 1e-6


@pytest.mark.parametrize("pm,P", [(0, 8), (1, 8), (2, 8), (3, 8), (6, 8)])
def test_adjoint_linearisation_matches_fourteen_columns(pm, P, monkeypatch):
    """Photometric patterns linearise through the pair's adjoint (linearize_adj_kernel: the matrix cores form the
    8-column target products, the host blocks follow as Adᵀ·H_tt·Ad, −Adᵀ·H_tt, −Adᵀ·g_t and W_h = −W_t·Ad) — against
    the 14-column products of the same rows (linearize_kernel, the one A/B reference lineariser: PBA_LIN_LEGACY in the
    library's test build, libpba_test.so) on the same problem: same cost, reduced system and step to the rounding of the
    fp32 host rows (the host Jacobian's fp32 rounding differs), then the same LM run.  (9…32-px patterns, ⌈P/8⌉ passes of
    the same kernel into fp64 per-block accumulators: test_reduced_system_large_patterns, against the dense reference.)"""
    interp, model = pm >> 2, pm & 3
    pat = None if P == 8 else np.random.default_rng(P).integers(-3, 4, (P, 2)).astype(np.float32)
    pb = synth.make_problem(model=model, n_frames=10, n_points=200, width=376, height=240, seed=70 + pm, border=12,
                            obs_sigma=0.3, pattern=pat)
    pb.interp = interp
    pb.poses[:2] = pb.poses_gt[:2]
    out = {}
    for legacy in (True, False):
        if legacy:
            monkeypatch.setenv("PBA_LIN_LEGACY", "1")
        else:
            monkeypatch.delenv("PBA_LIN_LEGACY")
        with make_engine(pb, 9.0, (0, 1), E.TEST_LIB_PATH if legacy else None) as eng:
            c = eng.gn_linearize()
            _, st = eng.gn_step(1e-3)
            assert st == 0
            S, gS = eng.gn_reduced_system()
            dp, dl = eng.gn_last_step()
            eng.set_state(pb.poses, pb.rho)
            summ = eng.solve(max_iterations=10)
        out[legacy] = (c, S, gS, dp, dl, summ)
    (c0, S0, g0, dp0, dl0, s0), (c1, S1, g1, dp1, dl1, s1) = out[True], out[False]
    eS = np.abs(S1 - S0).max() / np.abs(S0).max()
    eg = np.abs(g1 - g0).max() / np.abs(g0).max()
    ep = np.linalg.norm(dp1 - dp0) / np.linalg.norm(dp0)
    el = np.linalg.norm(dl1 - dl0) / np.linalg.norm(dl0)
    print(f"\nmodel {pm}: S {eS:.1e}, g {eg:.1e}, pose step {ep:.1e}, ρ step {el:.1e}, final cost "
          f"{s1['final_cost']:.10e} / {s0['final_cost']:.10e}")
    assert c1 == c0  # the same rows and weights: the cost does not depend on the products
    tol = 1e-6
    assert eS <= tol and eg <= tol, (eS, eg)
    assert ep <= 10 * tol and el <= 10 * tol, (ep, el)
    for key in ("iterations", "successful_steps", "unsuccessful_steps", "termination"):
        assert s1[key] == s0[key], (key, s1, s0)
    assert abs(s1["final_cost"] - s0["final_cost"]) <= 1e-6 * s0["final_cost"]


def test_candidate_cost_and_accept():
    pb = synth.make_problem(n_frames=8, n_points=80, width=376, height=240, seed=21, border=12)
    with make_engine(pb, 9.0, (0,)) as eng:
        eng.gn_linearize()
        eng.gn_step(1e-3)
        dp, dl = eng.gn_last_step()
        c_new = eng.gn_candidate_cost()
        eng.gn_accept()
        poses, rho = eng.get_state()
    np_, nr = GR.apply_step(pb.poses, pb.rho, dp, dl)
    np.testing.assert_allclose(poses, np_, atol=1e-10)
    np.testing.assert_allclose(rho, nr, rtol=1e-12)
    _, _, c_ref = GR.linearize(pb, np_, nr, 9.0, (0,))
    assert abs(c_new - c_ref) <= 1e-5 * c_ref + 1e-6


LM_CASES = [
    # kind, model, huber, pose σ, ρ σ, min_relative_decrease, iterations
    (0, 0, 9.0, 0.003, 0.02, 1e-3, 15),
    (1, 0, 1.0, 0.003, 0.02, 1e-3, 15),
    (1, 1, 1.0, 0.003, 0.02, 1e-3, 15),
    (1, 0, 1.0, 0.05, 0.3, 1e-3, 15),  # converges (function tolerance) after 9 trials
    # a strict acceptance threshold forces rejected steps: the reference's relative decreases are 1.77 1.92 2.07
    # 1.89 1.23, then 0.896 0.896 0.896 0.897 0.905 0.902 0.919 (all rejected: margin ≥ 0.03), then ≈ 1.0
    (0, 0, 9.0, 0.003, 0.02, 0.95, 15),
]


@pytest.mark.parametrize("kind,model,huber,ps,rs,min_rel,iters", LM_CASES)
def test_lm_matches_reference_lm(kind, model, huber, ps, rs, min_rel, iters):
    """The device LM loop (lm_decide_kernel + gated accept / speculative linearisation) takes the same trust-region
    decisions as the host reference of trust_region_minimizer.cc: same iterations, successful and unsuccessful
    step counts, termination, final cost, poses and inverse distances."""
    pb = synth.make_problem(kind=kind, model=model, n_frames=8, n_points=120, width=376, height=240, seed=31,
                            border=12, obs_sigma=0.3, pose_sigma=ps, rho_sigma=rs)
    pb.poses[:2] = pb.poses_gt[:2]
    fixed = (0, 1)
    p_ref, r_ref, c0_ref, c1_ref, it_ref, info = GR.lm(pb, huber, fixed, max_iterations=iters,
                                                        min_relative_decrease=min_rel, summary=True)
    with make_engine(pb, huber, fixed) as eng:
        summ = eng.solve(max_iterations=iters, min_relative_decrease=min_rel)
        poses, rho = eng.get_state()
    assert abs(summ["initial_cost"] - c0_ref) <= 1e-5 * c0_ref
    assert summ["final_cost"] < summ["initial_cost"]
    assert abs(summ["final_cost"] - c1_ref) <= 1e-3 * c1_ref + 1e-6, (summ, c1_ref)
    assert summ["iterations"] == it_ref, (summ, it_ref, info)
    assert summ["successful_steps"] == info["successful_steps"], (summ, info)
    assert summ["unsuccessful_steps"] == info["unsuccessful_steps"], (summ, info)
    assert (summ["termination"] == 0) == info["converged"], (summ, info)
    assert summ["stop_reason"] == info["stop_reason"], (summ, info)
    np.testing.assert_allclose(poses[:, 4:], p_ref[:, 4:], atol=1e-5)
    np.testing.assert_allclose(poses[:, :4] * np.sign(poses[:, 3:4]), p_ref[:, :4] * np.sign(p_ref[:, 3:4]), atol=1e-5)
    np.testing.assert_allclose(rho, r_ref, rtol=1e-4)


def _same_lm(summ, poses, rho, ref):
    p_ref, r_ref, c0_ref, c1_ref, it_ref, info = ref
    assert abs(summ["initial_cost"] - c0_ref) <= 1e-5 * c0_ref
    assert abs(summ["final_cost"] - c1_ref) <= 1e-3 * c1_ref + 1e-6, (summ, c1_ref)
    assert summ["iterations"] == it_ref, (summ, it_ref, info)
    assert summ["successful_steps"] == info["successful_steps"], (summ, info)
    assert summ["unsuccessful_steps"] == info["unsuccessful_steps"], (summ, info)
    assert summ["stop_reason"] == info["stop_reason"], (summ, info)
    assert (summ["termination"] == 0) == info["converged"], (summ, info)
    np.testing.assert_allclose(poses[:, 4:], p_ref[:, 4:], atol=1e-5)
    np.testing.assert_allclose(rho, r_ref, rtol=1e-4, atol=1e-6)


def forward_problem(seed=31):
    """Keyframes moving 1.2 m per frame along their optical axis: the last targets are close to the points, and with
    a huge initial trust region the Gauss-Newton steps push some points behind a target camera (outside the
    projection domain)."""
    nf = 6
    T = np.zeros((nf, 7))
    T[:, 3] = 1.0
    T[:, 6] = 1.2 * np.arange(nf)
    T[:, 4] = 0.02 * np.arange(nf)
    pb = synth.make_problem(kind=0, model=0, n_frames=nf, n_points=80, width=376, height=240, seed=seed, border=12,
                            obs_sigma=0.3, pose_sigma=0.02, rho_sigma=0.1, poses_gt=T)
    pb.poses[:2] = pb.poses_gt[:2]
    return pb


def test_lm_rejects_candidate_that_invalidates_blocks():
    """A candidate that leaves the projection domain for a block that is valid at the current state has infinite cost
    (Ceres' Evaluate failing, trust_region_minimizer.cc:771-778) and is rejected — it must not count as a cost decrease
    because the block's residual vanished.  Same decisions as the reference loop, which sees 2 such candidates."""
    pb = forward_problem()
    ref = GR.lm(pb, 9.0, (0, 1), max_iterations=6, radius=1e12, summary=True)
    assert ref[5]["invalid_candidates"] >= 1, ref[5]
    with make_engine(pb, 9.0, (0, 1)) as eng:
        summ = eng.solve(max_iterations=6, initial_trust_region_radius=1e12)
        poses, rho = eng.get_state()
    _same_lm(summ, poses, rho, ref)


def _lm_case(seed=31):
    pb = synth.make_problem(kind=0, model=0, n_frames=8, n_points=120, width=376, height=240, seed=seed, border=12,
                            obs_sigma=0.3, pose_sigma=0.003, rho_sigma=0.02)
    pb.poses[:2] = pb.poses_gt[:2]
    return pb


def test_lm_parameter_tolerance_stop():
    """ParameterToleranceReached (trust_region_minimizer.cc:706-726): |x − x_new| ≤ ptol (x_norm + ptol) with x_norm = −1
    until the first accepted step.  ptol is chosen from the reference's own valid steps so that a step in mid-run is the
    first to satisfy it, with ≥ 20 % margin on every step; the engine must stop on the same trial."""
    pb = _lm_case()
    hist = GR.lm(pb, 9.0, (0, 1), max_iterations=15, parameter_tolerance=0.0, summary=True)[5]["history"]
    ratios = [(st / (xn + 0.0)) if xn > 0 else np.inf for _, _, st, xn, _ in hist]
    pick = None
    for k in range(1, len(ratios)):
        earlier = min(ratios[:k])
        if np.isfinite(ratios[k]) and ratios[k] * 1.5 < earlier:
            pick = k
            break
    assert pick is not None, ratios
    ptol = ratios[pick] * 1.2
    ref = GR.lm(pb, 9.0, (0, 1), max_iterations=15, parameter_tolerance=ptol, summary=True)
    assert ref[5]["stop_reason"] == "parameter_tolerance", ref[5]
    with make_engine(pb, 9.0, (0, 1)) as eng:
        summ = eng.solve(max_iterations=15, parameter_tolerance=ptol)
        poses, rho = eng.get_state()
    _same_lm(summ, poses, rho, ref)


def test_lm_gradient_tolerance_stop():
    """GradientToleranceReached (trust_region_minimizer.cc:668-684) after an accepted step: max|x − (x ⊞ −g)| ≤ gtol
    at the new state ends the solve before the next step.  gtol is chosen between the reference's gradient norms (≥ 2×
    margin on both sides)."""
    pb = _lm_case()
    ref0 = GR.lm(pb, 9.0, (0, 1), max_iterations=15, gradient_tolerance=0.0, summary=True)
    g = [h[4] for h in ref0[5]["history"] if h[1]]
    gprev = [ref0[5]["gnorm0"]] + g
    pick = None
    for k in range(1, len(g)):
        if 4.0 * g[k] < min(gprev[:k + 1]):
            pick = k
            break
    assert pick is not None, g
    gtol = 2.0 * g[pick]
    ref = GR.lm(pb, 9.0, (0, 1), max_iterations=15, gradient_tolerance=gtol, summary=True)
    assert ref[5]["stop_reason"] == "gradient_tolerance", ref[5]
    with make_engine(pb, 9.0, (0, 1)) as eng:
        summ = eng.solve(max_iterations=15, gradient_tolerance=gtol)
        poses, rho = eng.get_state()
    _same_lm(summ, poses, rho, ref)
    assert summ["gradient_max_norm"] <= gtol


def test_point_without_blocks_keeps_its_state():
    """A landmark observed only by its host has no residual block (map_utils.h:347-375 adds none; pba_map_load
    keeps it as a point).  Ceres never sees its inverse distance, so solve() must leave it bit-identical."""
    pb = synth.make_problem(kind="geometric", n_frames=8, n_points=100, width=376, height=240, seed=33, border=12)
    keep = pb.block_point != 7
    pb = synth.Problem(**{**pb.__dict__, "block_point": pb.block_point[keep], "block_target": pb.block_target[keep],
                          "u_obs": pb.u_obs[keep]})
    rho0 = pb.rho.copy()
    with make_engine(pb, 1.0, (0,)) as eng:
        summ = eng.solve(max_iterations=5)
        _, rho = eng.get_state()
    assert summ["successful_steps"] > 0
    assert rho[7] == rho0[7]
    assert np.abs(rho - rho0).max() > 0


def test_photometric_lm_converges_towards_ground_truth():
    """Rendered plane scene: LM from a perturbed state recovers the keyframe poses (two frames fixed)."""
    pb = synth.make_problem(n_frames=10, n_points=800, width=376, height=240, seed=41, border=12,
                            pose_sigma=0.002, rho_sigma=0.01)
    pb.poses[:2] = pb.poses_gt[:2]
    with make_engine(pb, 9.0, (0, 1)) as eng:
        summ = eng.solve(max_iterations=30)
        poses, rho = eng.get_state()
    import oracle as O
    out, valid = O.evaluate(pb, poses=pb.poses_gt, rho=pb.rho_gt, want_jac=False)
    cost_gt = sum(O.huber_block(out[b, :pb.R], 9.0)[0] for b in range(pb.n_blocks) if valid[b])
    # reaches (or beats: quantised images, weak gauge over a 0.45 m chain) the ground-truth cost
    assert summ["final_cost"] <= 1.05 * cost_gt, (summ, cost_gt)
    err0 = np.abs(pb.poses[:, 4:] - pb.poses_gt[:, 4:]).max(1)
    err1 = np.abs(poses[:, 4:] - pb.poses_gt[:, 4:]).max(1)
    assert err1[2:].mean() < 0.6 * err0[2:].mean(), (err0, err1)


def test_c3_sized_gn_iteration_runs():
    """200 keyframes × 20k points (C3): one linearise + step; reduced system finite and step decreases cost."""
    pb = synth.make_problem(n_frames=200, n_points=20000, texture="noise", seed=42, pose_sigma=5e-4, rho_sigma=5e-3)
    with make_engine(pb, 9.0, (0, 1)) as eng:
        c = eng.gn_linearize()
        m, st = eng.gn_step(1e-2)
        assert st == 0 and m > 0
        c_new = eng.gn_candidate_cost()
        dp, dl = eng.gn_last_step()
    assert np.isfinite(dp).all() and np.isfinite(dl).all()
    assert np.isfinite(c_new)


@pytest.mark.parametrize("solver", ["cr", "band"])
def test_gn_step_and_solve_are_reproducible(solver, monkeypatch):
    """C3 size: the same linearisation gives the same step bit for bit, twice in one engine and in a second engine
    (fresh buffers), and pba_solve the same final state — every device sum has a fixed order and nothing races.
    (Cyclic reduction's level 0 had each diagonal block entry written by two lanes whose sums can differ in the last
    bit, so the step varied from run to run.)"""
    monkeypatch.setenv("PBA_SOLVER", solver)
    pb = synth.make_problem(n_frames=200, n_points=20000, texture="noise", seed=42, pose_sigma=5e-4, rho_sigma=5e-3)
    runs = []
    for _ in range(2):
        with make_engine(pb, 9.0, (0, 1)) as eng:
            for _ in range(2):
                eng.set_state(pb.poses, pb.rho)
                eng.gn_linearize()
                _, st = eng.gn_step(1e-3)
                assert st == 0
                dp, dl = eng.gn_last_step()
                eng.set_state(pb.poses, pb.rho)
                s = eng.solve(max_iterations=4, function_tolerance=0.0)
                poses, rho = eng.get_state()
                runs.append((dp, dl, np.float64(s["final_cost"]), poses, rho))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b)


def test_solve_survives_a_slow_host_thread(monkeypatch):
    """The device-steered LM loop publishes each trial's decision record while the host already has the next trial
    enqueued.  A host thread that sleeps longer than a trial before each wait (PBA_LM_HOST_DELAY_US, as a descheduled
    thread would) must still read every trial's own record — the records go to a ring of slots by sequence number; with
    one slot the next trial's record overwrote the awaited one and the solve failed.  Same trajectory as without (the
    delayed run loads the library's test build, libpba_test.so, where the hook exists)."""
    pb = synth.make_problem(n_frames=40, n_points=2000, texture="noise", seed=44, pose_sigma=5e-4, rho_sigma=5e-3)
    with make_engine(pb, 9.0, (0, 1)) as eng:
        ref = eng.solve(max_iterations=6, function_tolerance=0.0)
        ref_state = eng.get_state()
    monkeypatch.setenv("PBA_LM_HOST_DELAY_US", "3000")  # ≫ one trial at this size (a hook of the test build)
    with make_engine(pb, 9.0, (0, 1), E.TEST_LIB_PATH) as eng:
        s = eng.solve(max_iterations=6, function_tolerance=0.0)
        state = eng.get_state()
    for k in ("iterations", "successful_steps", "unsuccessful_steps", "final_cost"):
        assert s[k] == ref[k], (k, s, ref)
    assert all(np.array_equal(a, b) for a, b in zip(state, ref_state))


@pytest.mark.parametrize("solver", ["cr", "band", "skyline"])
@pytest.mark.parametrize("n_frames", [12, 13, 6, 37])
def test_reduced_solvers_agree(solver, n_frames, monkeypatch):
    """Block cyclic reduction (default for bandwidth ≤ 8 block rows), the LDS-window band Cholesky and the
    general skyline Cholesky all give the reference step (frame counts that are not multiples of the
    super-row size exercise the identity padding of cyclic reduction)."""
    monkeypatch.setenv("PBA_SOLVER", solver)
    pb = synth.make_problem(n_frames=n_frames, n_points=10 * n_frames, width=376, height=240, seed=51 + n_frames,
                            border=12)
    fixed = (0,)
    H, g, _ = GR.linearize(pb, pb.poses, pb.rho, 9.0, fixed)
    _, gS_ref, dp_ref, dl_ref, _ = GR.schur_step(H, g, pb.n_frames, 1e-3, fixed)
    with make_engine(pb, 9.0, fixed) as eng:
        eng.gn_linearize()
        _, st = eng.gn_step(1e-3)
        dp, dl = eng.gn_last_step()
    assert st == 0
    assert np.linalg.norm(dp - dp_ref) <= 1e-3 * np.linalg.norm(dp_ref)
    assert np.linalg.norm(dl - dl_ref) <= 1e-3 * np.linalg.norm(dl_ref)


@pytest.mark.parametrize("pcr_cap", ["0", "1", "4", "16", "1000"])
@pytest.mark.parametrize("n_frames", [37, 150, 300])
def test_cyclic_reduction_large_levels(n_frames, pcr_cap, monkeypatch):
    """Problems whose top cyclic-reduction levels exceed the single-workgroup tail (> 32 super-rows) take the
    per-level back-substitution launches; parallel cyclic reduction takes over once a level has at most
    PBA_PCR_CAP rows (0: cyclic reduction down to the root; 1000: PCR from level 0, no back-substitution; 4 / 16:
    CR levels, PCR, then back-substitution through the tail and the large levels).  The step must equal the band
    Cholesky's (the PCR levels a launch each, the last one also solving its decoupled rows)."""
    pb = synth.make_problem(n_frames=n_frames, n_points=20 * n_frames, width=376, height=240, seed=7 + n_frames,
                            border=12)
    monkeypatch.setenv("PBA_PCR_CAP", pcr_cap)
    steps = {}
    for solver in ("cr", "band"):
        monkeypatch.setenv("PBA_SOLVER", solver)
        with make_engine(pb, 9.0, (0,)) as eng:
            eng.gn_linearize()
            _, st = eng.gn_step(1e-3)
            assert st == 0
            steps[solver] = eng.gn_last_step()
    for a, b in zip(steps["cr"], steps["band"]):
        assert np.linalg.norm(a - b) <= 1e-7 * np.linalg.norm(b)


def test_loop_closure_structure_uses_skyline():
    pb = synth.make_problem(kind="geometric", n_frames=24, n_points=150, seed=52, obs_sigma=0.2)
    # add loop-closure observations: points of host 0 seen again by the last keyframe
    sel = np.nonzero(pb.point_host == 0)[0][:10]
    extra_t = np.full(len(sel), pb.n_frames - 1, np.int32)
    Th, Tt = pb.poses_gt[0], pb.poses_gt[pb.n_frames - 1]
    b = synth.unproject(pb.model, pb.intrinsics[0], pb.u_ref[sel])
    ph = b / pb.rho_gt[sel, None]
    pw = (synth.quat_to_rot(Th[:4]) @ ph.T).T + Th[4:]
    pt = (synth.quat_to_rot(Tt[:4]).T @ (pw - Tt[4:]).T).T
    uo = synth.project(pb.model, pb.intrinsics[0], pt)
    ok = pt[:, 2] > 0.5
    pb = synth.Problem(**{**pb.__dict__, "block_point": np.concatenate([pb.block_point, sel[ok].astype(np.int32)]),
                          "block_target": np.concatenate([pb.block_target, extra_t[ok]]),
                          "u_obs": np.concatenate([pb.u_obs, uo[ok]])})
    fixed = (0,)
    H, g, _ = GR.linearize(pb, pb.poses, pb.rho, 1.0, fixed)
    _, _, dp_ref, dl_ref, _ = GR.schur_step(H, g, pb.n_frames, 1e-3, fixed)
    with make_engine(pb, 1.0, fixed) as eng:
        eng.gn_linearize()
        _, st = eng.gn_step(1e-3)
        dp, dl = eng.gn_last_step()
    assert st == 0
    assert np.linalg.norm(dp - dp_ref) <= 1e-3 * np.linalg.norm(dp_ref)
    assert np.linalg.norm(dl - dl_ref) <= 1e-3 * np.linalg.norm(dl_ref)


def _intrinsics_problem(n_frames, n_points, seed):
    pb0 = synth.make_problem(kind=1, n_frames=n_frames, n_points=n_points, width=376, height=240, seed=seed, border=12)
    k1 = pb0.intrinsics[0].copy()
    k1[:4] *= np.array([1.01, 0.99, 1.0, 1.0])
    intr = np.stack([pb0.intrinsics[0], k1])
    return synth.make_problem(kind=1, n_frames=n_frames, n_points=n_points, width=376, height=240, seed=seed,
                              border=12, intrinsics=intr, frame_cam=np.arange(n_frames, dtype=np.int32) % 2)


@pytest.mark.parametrize("case", ["band", "loop", "intrinsics"])
def test_front_and_global_skyline_agree(case, monkeypatch):
    """The skyline system's two solvers: front_solve_kernel (the active front — the rows of the current column's profile
    — in LDS, statically slotted rows, fresh blocks prefetched a column ahead) and skyline_solve_kernel (the same
    right-looking factorisation through global memory, PBA_SKYLINE_GLOBAL).  A band forced onto the skyline path, a
    loop-closure profile (row n − 1 reaches column 0) and the free-intrinsics border (two cameras, 2·2 border rows) give
    the same step to fp64 rounding (reciprocal pivots against divisions)."""
    monkeypatch.setenv("PBA_SOLVER", "skyline")
    if case == "band":
        pb, huber = synth.make_problem(n_frames=37, n_points=370, width=376, height=240, seed=88, border=12), 9.0
    elif case == "loop":
        pb = synth.make_problem(kind="geometric", n_frames=24, n_points=150, seed=52, obs_sigma=0.2)
        sel = np.nonzero(pb.point_host == 0)[0][:10]
        Th, Tt = pb.poses_gt[0], pb.poses_gt[pb.n_frames - 1]
        b = synth.unproject(pb.model, pb.intrinsics[0], pb.u_ref[sel])
        pw = (synth.quat_to_rot(Th[:4]) @ (b / pb.rho_gt[sel, None]).T).T + Th[4:]
        pt = (synth.quat_to_rot(Tt[:4]).T @ (pw - Tt[4:]).T).T
        ok = pt[:, 2] > 0.5
        pb = synth.Problem(**{**pb.__dict__,
                              "block_point": np.concatenate([pb.block_point, sel[ok].astype(np.int32)]),
                              "block_target": np.concatenate([pb.block_target,
                                                              np.full(ok.sum(), pb.n_frames - 1, np.int32)]),
                              "u_obs": np.concatenate([pb.u_obs, synth.project(pb.model, pb.intrinsics[0], pt)[ok]])})
        huber = 1.0
    else:
        pb, huber = _intrinsics_problem(16, 200, 17), 1.0
    steps = {}
    for glob in (False, True):
        if glob:
            monkeypatch.setenv("PBA_SKYLINE_GLOBAL", "1")
        with make_engine(pb, huber, (0, 1)) as eng:
            if case == "intrinsics":
                eng.set_optimize_intrinsics(True)
            eng.gn_linearize()
            m, st = eng.gn_step(1e-3)
            assert st == 0
            steps[glob] = (*eng.gn_last_step(), np.array([m]))
    for a, b in zip(steps[False], steps[True]):
        assert np.linalg.norm(a - b) <= 1e-9 * np.linalg.norm(b), (case, np.linalg.norm(a - b) / np.linalg.norm(b))


def _intrinsics_rig(n_frames, n_points, seed, n_cams, model=0):
    """A rig of n_cams cameras (keyframe f uses camera f % n_cams) whose intrinsics state differs from the cameras the
    hosts unproject with (reprojection.h:93-98)."""
    pb0 = synth.make_problem(kind=1, model=model, n_frames=n_frames, n_points=n_points, width=376, height=240,
                             seed=seed, border=12)
    intr = np.stack([pb0.intrinsics[0] * np.array([1 + 0.01 * c, 1 - 0.01 * c, 1, 1, 1, 1, 1, 1])
                     for c in range(n_cams)])
    pb = synth.make_problem(kind=1, model=model, n_frames=n_frames, n_points=n_points, width=376, height=240, seed=seed,
                            border=12, intrinsics=intr, frame_cam=(np.arange(n_frames) % n_cams).astype(np.int32),
                            obs_sigma=0.3)
    return pb, intr * np.array([1.003, 0.998, 1.0005, 0.9995, 1, 1, 1, 1])


@pytest.mark.parametrize("n_cams", [1, 2, 3, 4])
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_arrow_and_front_solvers_agree(n_cams, lam, monkeypatch):
    """Free intrinsics (map_utils.h:339-345): the reduced system is an arrow — the keyframes' band plus the 2·nc border
    frames' dense rows.  arrow_solve (parallel cyclic reduction of the band with the border's 12·nc columns as extra
    right-hand sides in batches of 16 — 1, 2, 3 and 4 batches here — then the border's Schur complement) and
    front_solve_kernel (the skyline Cholesky, border last: the same elimination order; PBA_SOLVER=front) give the same
    pose, intrinsics and inverse-distance steps and model decrease to fp64 rounding."""
    pb, state = _intrinsics_rig(23, 260, 31 + n_cams, n_cams)
    out = {}
    for solver in ("arrow", "front"):
        if solver == "front":
            monkeypatch.setenv("PBA_SOLVER", "front")
        with make_engine(pb, 1.0, (0, 1)) as eng:
            eng.set_optimize_intrinsics(True)
            eng.set_intrinsics_state(state)
            eng.gn_linearize()
            m, st = eng.gn_step(lam)
            assert st == 0, solver
            dp, dr = eng.gn_last_step()
            eng.gn_accept()
            out[solver] = (dp, dr, eng.get_intrinsics() - state, np.array([m]))
    for name, a, b in zip(("poses", "rho", "intrinsics", "model"), out["arrow"], out["front"]):
        err = np.linalg.norm(a - b) / np.linalg.norm(b)
        print(f"\nn_cams {n_cams} λ {lam}: {name} {err:.2e}")
        assert err <= 1e-8, (name, err)


@pytest.mark.parametrize("n_cams", [1, 2, 3, 4])
def test_point_sums_in_rows_match_separate_kernel(n_cams, monkeypatch):
    """Free intrinsics: the points' W sums (per camera Σ W_i, and W_h) are formed by intr_rows_kernel itself when every
    GN point fits one wave (point-aligned waves of ≤ 64 blocks), else by intr_pw_kernel after 64-block waves
    (PBA_TEST_ROW_WAVES64 forces it; test build).  The same sums in the same block order: the two paths give the same
    reduced-system step (measured: bit-identical, all three paths).  Likewise the keyframe border kernel's
    Schur terms from the point's one block targeting the keyframe (ib_pblk) and from a walk over the point's blocks (the
    path of a point observed twice by one keyframe; PBA_TEST_PBLK_WALK forces it)."""
    pb, state = _intrinsics_rig(23, 260, 41 + n_cams, n_cams)
    out = {}
    for path in ("fused", "separate", "walk"):
        monkeypatch.delenv("PBA_TEST_ROW_WAVES64", raising=False)
        if path == "separate":
            monkeypatch.setenv("PBA_TEST_ROW_WAVES64", "1")
        if path == "walk":
            monkeypatch.setenv("PBA_TEST_PBLK_WALK", "1")
        with make_engine(pb, 1.0, (0, 1), E.TEST_LIB_PATH) as eng:
            eng.set_optimize_intrinsics(True)
            eng.set_intrinsics_state(state)
            eng.gn_linearize()
            m, st = eng.gn_step(1e-3)
            assert st == 0, path
            dp, dr = eng.gn_last_step()
            eng.gn_accept()
            out[path] = (dp, dr, eng.get_intrinsics() - state, np.array([m]))
    for other in ("separate", "walk"):
        for name, a, b in zip(("poses", "rho", "intrinsics", "model"), out["fused"], out[other]):
            err = np.linalg.norm(a - b) / np.linalg.norm(b)
            print(f"\nn_cams {n_cams} {other}: {name} {err:.2e}")
            assert err <= 1e-12, (other, name, err)


@pytest.fixture(scope="module")
def c3():
    """BASELINE configs[2] (C3): 200 keyframes × 20k points × 8 px × 4 targets = 80k blocks, rendered images."""
    pb = synth.make_problem(n_frames=200, n_points=20000, seed=42)
    pb.poses[:2] = pb.poses_gt[:2]
    return pb


@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_c3_reduced_system_and_step_against_fp64_reference(c3, lam):
    """At full C3 size: the device's reduced camera system S and right-hand side g_S (fp32 rows, fp64 JᵀJ block
    products on the fp64 matrix cores since round 5, point elimination and assembly in fp64) against the fp64 system
    built block-sparsely from the oracle's Jacobians (gn_reference.reduced_system_sparse, the
    schur_complement_solver.cc:138-146 quantities), and the step against the dense fp64 solve of the reference system.
    Measured (MI355X, round 5): S 7.7e-8 and g 3.8e-8 of their scale, the step 2.0e-7 relative at λ = 1e-4 (round 4's
    fp32 block products: 3.2e-5 — the weakly damped system amplified their rounding), the cost 1.5e-8.
    Bounds: 1e-6 (cost, S, g), the north star's 1e-5 (step)."""
    fixed = (0, 1)
    S_ref, g_ref, c_ref = GR.reduced_system_sparse(c3, c3.poses, c3.rho, 9.0, lam, fixed)
    dp_ref = np.linalg.solve(S_ref, -g_ref)
    with make_engine(c3, 9.0, fixed) as eng:
        c = eng.gn_linearize()
        _, st = eng.gn_step(lam)
        assert st == 0
        S, g = eng.gn_reduced_system()
        dp, _ = eng.gn_last_step()
    eS = np.abs(S - S_ref).max() / np.abs(S_ref).max()
    eg = np.abs(g - g_ref).max() / np.abs(g_ref).max()
    ep = np.linalg.norm(dp.ravel() - dp_ref) / np.linalg.norm(dp_ref)
    print(f"\nC3 λ={lam}: cost {abs(c - c_ref) / c_ref:.2e}, S {eS:.2e}, g {eg:.2e}, step {ep:.2e}")
    assert abs(c - c_ref) <= 1e-6 * c_ref
    assert eS <= 1e-6, eS
    assert eg <= 1e-6, eg
    assert ep <= 1e-5, ep


def test_c3_engine_lm_matches_ceres_cpu(c3):
    """pba_solve at full C3 size against real Ceres 2.0.0 LM (SPARSE_SCHUR, AutoDiff over the restated photometric
    functor, the reference's LocalParameterizationSE3): the same successful / unsuccessful step counts and the final
    cost to 1e-5.  The state after 10 iterations (not converged: Ceres stops at the iteration limit) measured |Δt| ≤
    6.3e-4 m and Δρ/ρ ≤ 3.6e-2 at the worst point (the 99th percentile is printed): weakly observed inverse distances
    move along their null direction with the order of the fp64 sums; bounded at ~3× those."""
    if not CR.available():
        pytest.skip("oracle/_ref/ceres_lm_driver not built")
    ref = CR.run("cpu", c3, iters=10, huber=9.0, threads=THREADS, timeout=1200)
    with make_engine(c3, 9.0, (0, 1)) as eng:
        s = eng.solve(max_iterations=10)
        poses, rho = eng.get_state()
    dt = np.abs(poses[:, 4:] - ref["poses"][:, 4:]).max()
    dr = (np.abs(rho - ref["rho"]) / np.abs(ref["rho"])).max()
    dr99 = np.percentile(np.abs(rho - ref["rho"]) / np.abs(ref["rho"]), 99)
    print(f"\nC3 LM final state vs Ceres: max |Δt| {dt:.2e} m, max Δρ/ρ {dr:.2e} (99th percentile {dr99:.2e})")
    print(f"\nC3 LM: engine {s['successful_steps']}/{s['unsuccessful_steps']} final {s['final_cost']:.9g}, Ceres "
          f"{ref['successful_steps'] - 1}/{ref['unsuccessful_steps']} final {ref['final_cost']:.9g} ({ref['message']})")
    assert s["successful_steps"] == ref["successful_steps"] - 1, (s, ref["message"])
    assert s["unsuccessful_steps"] == ref["unsuccessful_steps"], (s, ref["message"])
    assert abs(s["initial_cost"] - ref["costs"][0]) <= 1e-6 * ref["costs"][0]
    assert abs(s["final_cost"] - ref["final_cost"]) <= 1e-5 * ref["final_cost"], (s["final_cost"], ref["final_cost"])
    assert dt <= 2e-3 and dr <= 0.1, (dt, dr)


def test_set_frames_after_gn_reanalyses_the_problem():
    """pba_set_frames after a Gauss-Newton step re-analyses the GN structure (the pairs' camera records, the frame
    count): re-assigning the keyframes' cameras on a prepared engine gives the linearisation (bit for bit) and the
    step of a fresh engine built with the new assignment."""
    import ctypes as C
    intr = np.array([[460.0, 455.0, 188.0, 120.0, 0, 0, 0, 0], [430.0, 440.0, 180.0, 125.0, 0, 0, 0, 0]])
    pb = synth.make_problem(kind=0, model=0, n_frames=8, n_points=60, width=376, height=240, seed=5, border=14,
                            intrinsics=intr, frame_cam=np.arange(8, dtype=np.int32) % 2)
    eng = make_engine(pb, 9.0, (0,))
    eng.gn_linearize()
    eng.gn_step(1e-3)
    d0 = eng.gn_last_step()  # the step with the old camera assignment
    new_fc = (1 - pb.frame_cam).astype(np.int32)
    imgs = np.ascontiguousarray(pb.images, np.uint8)
    rc = eng._L.pba_set_frames(eng._h, 8, new_fc.ctypes.data_as(C.c_void_p), pb.width, pb.height,
                               imgs.ctypes.data_as(C.c_void_p))
    assert rc == 0
    eng.set_state(pb.poses, pb.rho)
    c1 = eng.gn_linearize()
    eng.gn_step(1e-3)
    d1 = eng.gn_last_step()
    eng.close()
    pb.frame_cam = new_fc
    ref = make_engine(pb, 9.0, (0,))
    c2 = ref.gn_linearize()
    ref.gn_step(1e-3)
    d2 = ref.gn_last_step()
    ref.close()
    assert c1 == c2  # the linearisation at the new assignment is bit for bit a fresh engine's
    # the steps agree to rounding (the re-prepared engine reuses its buffers), and differ from the old assignment's
    for a, b, o in zip(d1, d2, d0):
        assert np.allclose(a, b, rtol=1e-9, atol=1e-12 * np.abs(b).max())
        assert np.abs(o - b).max() > 1e-3 * np.abs(b).max()


@pytest.mark.parametrize("model", [0, 1, 2, 3])
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_free_intrinsics_reduced_system_and_step(model, lam):
    """Free intrinsics (pba_set_optimize_intrinsics; optimize_intrinsics, map_utils.h:339-345) in the on-device Schur GN:
    two cameras (a stereo rig) whose intrinsics state differs from the cameras the hosts unproject with
    (reprojection.h:93-98).  The device's reduced camera system over the keyframes AND the 8 intrinsics of each camera
    (the dense border of the skyline system) and its right-hand side against the dense fp64 reference built from the
    oracle's 44-value records (gn_reference.linearize_intrinsics / schur_step_intrinsics), the pose and inverse-distance
    step, the candidate intrinsics k + δk and the LM model decrease."""
    pb0 = synth.make_problem(kind=1, model=model, n_frames=10, n_points=120, width=376, height=240, seed=13, border=12)
    k1 = pb0.intrinsics[0].copy()
    k1[:4] *= np.array([1.01, 0.99, 1.0, 1.0])
    intr = np.stack([pb0.intrinsics[0], k1])
    pb = synth.make_problem(kind=1, model=model, n_frames=10, n_points=120, width=376, height=240, seed=13, border=12,
                            intrinsics=intr, frame_cam=np.arange(10, dtype=np.int32) % 2)
    state = intr * np.array([1.003, 0.998, 1.0005, 0.9995, 1, 1, 1, 1])
    fixed = (0, 1)
    nf, nc = pb.n_frames, 2
    H, g, c_ref = GR.linearize_intrinsics(pb, pb.poses, pb.rho, state, 1.0, fixed)
    S_ref, gS_ref, df_ref, dl_ref, m_ref = GR.schur_step_intrinsics(H, g, nf, nc, lam, fixed)
    with make_engine(pb, 1.0, fixed) as eng:
        eng.set_optimize_intrinsics(True)
        eng.set_intrinsics_state(state)
        c = eng.gn_linearize()
        m, st = eng.gn_step(lam)
        assert st == 0
        assert eng.gn_system_size() == 6 * nf + 12 * nc
        S, gs = eng.gn_reduced_system()
        dp, dr = eng.gn_last_step()
        eng.gn_accept()
        k_new = eng.get_intrinsics()
    idx = GR.intrinsics_system_index(nf, nc)
    Ss, gss = S[np.ix_(idx, idx)], gs[idx]
    eS = np.abs(Ss - S_ref).max() / np.abs(S_ref).max()
    eg = np.abs(gss - gS_ref).max() / np.abs(gS_ref).max()
    dk = (k_new - state).ravel()
    ep = np.linalg.norm(np.concatenate([dp.ravel(), dk]) - df_ref) / np.linalg.norm(df_ref)
    el = np.linalg.norm(dr - dl_ref) / np.linalg.norm(dl_ref)
    print(f"\nintrinsics model {model} λ={lam}: cost {abs(c - c_ref) / c_ref:.2e} S {eS:.2e} g {eg:.2e} "
          f"step {ep:.2e} δρ {el:.2e} model {abs(m - m_ref) / abs(m_ref):.2e}")
    # the pads: identity rows, zero gradient
    pad = np.concatenate([6 * nf + 12 * c + np.arange(8, 12) for c in range(nc)])
    assert np.allclose(S[np.ix_(pad, pad)], np.eye(len(pad)) * (1 + lam)) and not gs[pad].any()
    assert abs(c - c_ref) <= 1e-6 * c_ref
    assert eS <= 1e-5 and eg <= 1e-5, (eS, eg)
    assert ep <= 1e-3 and el <= 1e-3, (ep, el)
    assert abs(m - m_ref) <= 1e-3 * abs(m_ref)


_INTR_REF = {}  # rig → (pb, state, (H, g, cost)): the fp64 linearisation, formed once per rig and left unchanged


def _intrinsics_rig_reference(n_frames, n_points, seed, n_cams, model=0):
    key = (n_frames, n_points, seed, n_cams, model)
    if key not in _INTR_REF:
        pb, state = _intrinsics_rig(n_frames, n_points, seed, n_cams, model)
        _INTR_REF[key] = (pb, state, GR.linearize_intrinsics(pb, pb.poses, pb.rho, state, 1.0, (0, 1)))
    return _INTR_REF[key]


def _check_free_intrinsics_step(label, pb, state, lam, lin, library=None):
    """One free-intrinsics step of the engine (fixed frames 0 and 1, Huber 1.0) against the fp64 reference's, with the
    comparisons and tolerances of test_free_intrinsics_reduced_system_and_step: cost 1e-6; S and g (through
    intrinsics_system_index) 1e-5 of their scale; the pads; pose + intrinsics step, δρ and model decrease 1e-3.  Prints
    and returns the measured errors."""
    fixed = (0, 1)
    nf, nc = pb.n_frames, pb.intrinsics.shape[0]
    H, g, c_ref = lin
    S_ref, gS_ref, df_ref, dl_ref, m_ref = GR.schur_step_intrinsics(H, g, nf, nc, lam, fixed)
    with make_engine(pb, 1.0, fixed, library) as eng:
        eng.set_optimize_intrinsics(True)
        eng.set_intrinsics_state(state)
        c = eng.gn_linearize()
        m, st = eng.gn_step(lam)
        assert st == 0
        assert eng.gn_system_size() == 6 * nf + 12 * nc
        S, gs = eng.gn_reduced_system()
        dp, dr = eng.gn_last_step()
        eng.gn_accept()
        k_new = eng.get_intrinsics()
    idx = GR.intrinsics_system_index(nf, nc)
    Ss, gss = S[np.ix_(idx, idx)], gs[idx]
    err = {"cost": abs(c - c_ref) / c_ref,
           "S": np.abs(Ss - S_ref).max() / np.abs(S_ref).max(),
           "g": np.abs(gss - gS_ref).max() / np.abs(gS_ref).max(),
           "step": np.linalg.norm(np.concatenate([dp.ravel(), (k_new - state).ravel()]) - df_ref) / np.linalg.norm(df_ref),
           "drho": np.linalg.norm(dr - dl_ref) / np.linalg.norm(dl_ref),
           "model": abs(m - m_ref) / abs(m_ref)}
    print(f"\n{label} λ={lam}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    pad = np.concatenate([6 * nf + 12 * c + np.arange(8, 12) for c in range(nc)])
    assert np.allclose(S[np.ix_(pad, pad)], np.eye(len(pad)) * (1 + lam)) and not gs[pad].any()
    assert err["cost"] <= 1e-6, err
    assert err["S"] <= 1e-5 and err["g"] <= 1e-5, err
    assert err["step"] <= 1e-3 and err["drho"] <= 1e-3, err
    assert err["model"] <= 1e-3, err
    return err


def _free_intrinsics_step(pb, state, lam, library=None):
    """(pose step, δρ, intrinsics step, [model decrease]) of one free-intrinsics step, fixed frames 0 and 1."""
    with make_engine(pb, 1.0, (0, 1), library) as eng:
        eng.set_optimize_intrinsics(True)
        eng.set_intrinsics_state(state)
        eng.gn_linearize()
        m, st = eng.gn_step(lam)
        assert st == 0
        dp, dr = eng.gn_last_step()
        eng.gn_accept()
        return dp, dr, eng.get_intrinsics() - state, np.array([m])


def _assert_same_step(label, a, b, bound):
    worst = 0.0
    for name, x, y in zip(("poses", "rho", "intrinsics", "model"), a, b):
        err = np.linalg.norm(x - y) / np.linalg.norm(y)
        print(f"\n{label}: {name} {err:.2e}")
        assert err <= bound, (label, name, err)
        worst = max(worst, err)
    return worst


# (keyframes, points, cameras, camera model): the smallest rigs with nf·nc ≥ 512 (512 and 513) — enqueue_border's
# three-launch branch without a hook; 5200 and 4000 blocks (5200 % 256 = 80, 4000 % 256 = 160), 7-8 cyclic-reduction
# levels under the arrow solve with 4 and 3 right-hand-side batches; model 1: the 6-parameter double-sphere intrinsics
SPLIT_RIGS = [(128, 1300, 4, 0), (171, 1000, 3, 0), (128, 1300, 4, 1)]


@pytest.mark.parametrize("nf,npts,n_cams,model", SPLIT_RIGS)
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_free_intrinsics_split_border_against_fp64_reference(nf, npts, n_cams, model, lam):
    """The border branch of C3/C4-sized free-intrinsics problems — intr_border_kernel with two waves per keyframe block,
    intr_cam_dir_kernel and intr_cam_sch_kernel as three launches (enqueue_border, nf·nc ≥ 512) — reached by size alone,
    against the fp64 reference (gn_reference.linearize_intrinsics / schur_step_intrinsics) with the comparisons and
    tolerances of test_free_intrinsics_reduced_system_and_step.
    Measured (MI355X), the worst of the six cases: cost 1.8e-8, S 5.5e-8, g 3.8e-8, pose + intrinsics
    step 2.2e-6, δρ 7.9e-6, model decrease 7.5e-9 (λ = 1e-4; at λ = 1e-1 the steps are within 3.4e-8 / 2.1e-7)."""
    pb, state, lin = _intrinsics_rig_reference(nf, npts, 61 + n_cams + model, n_cams, model)
    assert pb.n_frames * pb.intrinsics.shape[0] >= 512  # the three-launch branch
    assert pb.n_blocks % 256 in (80, 160)
    _check_free_intrinsics_step(f"split border ({nf}, {npts}, {n_cams}) model {model}", pb, state, lam, lin)


@pytest.mark.parametrize("nf,npts,n_cams", [(23, 260, 1), (23, 260, 2), (23, 260, 3), (23, 260, 4), (128, 1300, 4),
                                            (23, 2600, 1), (23, 2600, 2)])
def test_split_and_fused_border_agree(nf, npts, n_cams, monkeypatch):
    """enqueue_border's two branches on the same problem (PBA_TEST_BORDER = fused | split, test build): one launch with
    four waves per keyframe block against three launches with two.  The same fp64 terms added in another lane order, so
    not bit-identical; held to the bound of test_arrow_and_front_solvers_agree for a differently ordered fp64
    computation of the same step, 1e-8 relative.
    Measured (MI355X): bit-identical (0.0) on the 260-point rigs and at (128, 1300, 4) — every
    keyframe's lists there hold fewer than 64 entries, all taken by the first wave's lanes under either kpw; the
    2600-point rigs (hundreds of entries per keyframe list, so every one of the two or four waves of a keyframe adds
    entries) are the cases where the lane order differs: pose step 3.7e-15 / 7.0e-15, δρ 3.8e-15 / 1.7e-15, model decrease 1.3e-16 / 0, intrinsics step
    0 (one and two cameras)."""
    if (nf, npts, n_cams) in ((128, 1300, 4), (23, 2600, 2)):
        pb, state, _ = _intrinsics_rig_reference(nf, npts, 61 + n_cams, n_cams, 0)
    else:
        pb, state = _intrinsics_rig(nf, npts, 51 + n_cams, n_cams)
    out = {}
    for branch in ("fused", "split"):
        monkeypatch.setenv("PBA_TEST_BORDER", branch)
        out[branch] = _free_intrinsics_step(pb, state, 1e-3, E.TEST_LIB_PATH)
    _assert_same_step(f"border split vs fused ({nf}, {npts}, {n_cams})", out["split"], out["fused"], 1e-8)


@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_free_intrinsics_long_keyframe_lists_against_fp64_reference(lam):
    """Keyframe lists longer than one wave takes: 23 keyframes × 2600 points × 2 cameras gives a keyframe ≈ 550 hosted and
    ≈ 550 targeting blocks, hundreds of entries per (camera, keyframe) list, so all four waves of a keyframe block (kpw =
    4, the one-launch branch) add entries
    and their sums are added in order through LDS (border_keyframes, sub ≥ 1) — on the 260-point rigs and at the
    split-border sizes above only the first wave has any.  ≈ 137 points per host: two Schur chunks per host.  Against
    the fp64 reference with the tolerances of test_free_intrinsics_reduced_system_and_step.
    Measured (MI355X): cost 1.7e-8, S 3.8e-8, g 2.6e-8, step 1.0e-6, δρ 2.7e-6, model 1.1e-8."""
    pb, state, lin = _intrinsics_rig_reference(23, 2600, 63, 2)
    assert np.bincount(pb.point_host).min() * 4 > 256  # every hosting keyframe's block list exceeds 4 waves' lanes
    _check_free_intrinsics_step("long keyframe lists (23, 2600, 2)", pb, state, lam, lin)


def _long_point_problem(seed):
    """_intrinsics_rig(23, 260, seed, 2) with 66 further observations of one point by its targets host + 1 … host + 4
    (each its own block with its own observation noise): a point of 70 blocks while the keyframe band stays 4."""
    pb, state = _intrinsics_rig(23, 260, seed, 2)
    rng = np.random.default_rng(seed + 1000)
    p = int(np.nonzero(pb.point_host == 9)[0][0])
    h = int(pb.point_host[p])
    tg = (h + 1 + np.arange(66) % 4).astype(np.int32)
    Th, Tt = pb.poses_gt[h], pb.poses_gt[tg]
    b = synth.unproject(pb.model, pb.intrinsics[pb.frame_cam[h]], pb.u_ref[p:p + 1])
    pw = synth.quat_to_rot(Th[:4]) @ (b[0] / pb.rho_gt[p]) + Th[4:]
    pt = (np.swapaxes(synth.quat_to_rot(Tt[:, :4]), -1, -2) @ (pw - Tt[:, 4:])[..., None])[..., 0]
    assert (pt[:, 2] > 0.5).all()
    uo = synth.project(pb.model, pb.intrinsics[pb.frame_cam[tg]], pt) + rng.normal(0, 0.3, (66, 2))
    pb = synth.Problem(**{**pb.__dict__, "block_point": np.concatenate([pb.block_point, np.full(66, p, np.int32)]),
                          "block_target": np.concatenate([pb.block_target, tg]),
                          "u_obs": np.concatenate([pb.u_obs, uo])})
    return pb, state


@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_free_intrinsics_point_of_seventy_blocks_against_fp64_reference(lam):
    """A point with more than 64 blocks, without a hook: gn_prepare gives up the point-aligned waves (ir_waves = 0), so
    intr_rows_kernel runs its 64-block waves — 1106 blocks, 1106 % 256 = 82: the last workgroup's last two waves lie
    wholly past the end and return — and intr_pw_kernel forms the points' sums; the keyframe border walks the point's
    blocks (ib_pblk = −2: ~17 blocks of the point target each of its four keyframes).  The band stays 4 (the arrow
    solve).  Against the fp64 reference, which sums per block, with the tolerances of
    test_free_intrinsics_reduced_system_and_step.
    Measured (MI355X): cost 1.5e-8, S 3.5e-8, g 2.7e-8, step 8.9e-7, δρ 2.5e-6, model 4.8e-9."""
    key = ("long point", 47)
    if key not in _INTR_REF:
        pb, state = _long_point_problem(47)
        _INTR_REF[key] = (pb, state, GR.linearize_intrinsics(pb, pb.poses, pb.rho, state, 1.0, (0, 1)))
    pb, state, lin = _INTR_REF[key]
    assert pb.n_blocks == 1106 and 1 <= pb.n_blocks % 256 <= 192  # a wave wholly past the end
    assert np.bincount(pb.block_point).max() == 70  # > 64: no point-aligned waves
    assert np.abs(pb.block_target - pb.point_host[pb.block_point]).max() == 4  # the band
    _check_free_intrinsics_step("70-block point", pb, state, lam, lin)


@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_free_intrinsics_five_cameras_against_fp64_reference(lam):
    """Five cameras: more than the arrow solve takes (kArrowMaxNc = 4), so the skyline front solver gets the 10-row
    border; 6·nf + 12·5 system rows (asserted in the shared check).  Against the fp64 reference with the tolerances of
    test_free_intrinsics_reduced_system_and_step.
    Measured (MI355X): cost 1.8e-8, S 4.9e-8, g 2.1e-8, step 1.3e-6, δρ 4.3e-6, model 6.9e-9."""
    pb, state, lin = _intrinsics_rig_reference(40, 400, 73, 5)
    assert pb.intrinsics.shape[0] == 5 and np.bincount(pb.frame_cam[pb.block_target], minlength=5).all()
    _check_free_intrinsics_step("five cameras (40, 400, 5)", pb, state, lam, lin)


def test_five_cameras_point_sums_in_rows_match_separate_kernel(monkeypatch):
    """Five cameras through intr_pw_kernel (PBA_TEST_ROW_WAVES64, test build): its second group of four cameras holds
    one camera.  The same sums in the same block order as intr_rows_kernel's point-aligned waves: the step to 1e-12, as
    test_point_sums_in_rows_match_separate_kernel.  Measured (MI355X): bit-identical (0.0)."""
    pb, state, _ = _intrinsics_rig_reference(40, 400, 73, 5)
    out = {}
    for path in ("fused", "separate"):
        if path == "separate":
            monkeypatch.setenv("PBA_TEST_ROW_WAVES64", "1")
        out[path] = _free_intrinsics_step(pb, state, 1e-3, E.TEST_LIB_PATH)
    _assert_same_step("five cameras, separate point sums", out["separate"], out["fused"], 1e-12)


@pytest.mark.parametrize("force_degen", [False, True])
@pytest.mark.parametrize("kind,model,huber,ps,rs,min_rel,iters", [LM_CASES[0], LM_CASES[2], LM_CASES[4]])
def test_lm_point_elimination_paths_agree(kind, model, huber, ps, rs, min_rel, iters, force_degen, monkeypatch):
    """The single-GPU LM loop eliminates the points once per linearisation, λ-free (P = Σ W Wᵀ/H, scaled by 1/(1 + λ)
    in the assembly: exact for every point whose H_ρρ lies inside the LM diagonal's clamp [1e-6, 1e32]), and falls back
    to the per-trial λ-specific elimination of schur_kernel for a set with a point outside it.  PBA_TEST_FORCE_DEGEN
    flags every set, so every trial takes the fallback: both paths take the reference LM's decisions, and their final
    costs agree to 1e-9 (the two orders of the same sums).  (PBA_TEST_FORCE_DEGEN is a hook of the library's test build,
    libpba_test.so, which the forced runs load.)"""
    if force_degen:
        monkeypatch.setenv("PBA_TEST_FORCE_DEGEN", "1")
    pb = synth.make_problem(kind=kind, model=model, n_frames=8, n_points=120, width=376, height=240, seed=31,
                            border=12, obs_sigma=0.3, pose_sigma=ps, rho_sigma=rs)
    pb.poses[:2] = pb.poses_gt[:2]
    ref = GR.lm(pb, huber, (0, 1), max_iterations=iters, min_relative_decrease=min_rel, summary=True)
    with make_engine(pb, huber, (0, 1), E.TEST_LIB_PATH if force_degen else None) as eng:
        summ = eng.solve(max_iterations=iters, min_relative_decrease=min_rel)
        poses, rho = eng.get_state()
        traj = eng.solver_iterations()
    _same_lm(summ, poses, rho, ref)
    assert len(traj["cost"]) >= 2 and traj["cost"][0] == summ["initial_cost"]
    key = (kind, model, min_rel)
    _ELIM_RESULTS.setdefault(key, {})[force_degen] = summ["final_cost"]
    if len(_ELIM_RESULTS[key]) == 2:
        a, b = _ELIM_RESULTS[key][False], _ELIM_RESULTS[key][True]
        assert abs(a - b) <= 1e-9 * abs(a), (a, b)


_ELIM_RESULTS = {}
