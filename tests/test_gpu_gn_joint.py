"""The joint solve of poses, inverse distances and affine brightness on the device: pba_joint_* and pba_solve_joint
(engine.joint_* / solve_joint), photometric engines with pba_set_affine_brightness.

Reference: tests/gn_joint_reference.py (dense fp64 over photometric_affine_reference.compose's 18·P records;
tests/test_gn_joint_reference.py asserts on the CPU the input conditions under which the bounds here mean something).

Problems: gn_affine_reference.problem(...) at state(pb) (a ∈ ±0.3, b ∈ ±20), poses of keyframes 0 and 1 constant,
(a, b) of keyframe 0 constant; the graphs of tests/graph_problems.py with the brightness change.

Bounds (the project's): cost 1e-5 relative; S and g within 1e-4 of the largest entry of each
part — S over pose×pose, pose×(a, b) and (a, b)×(a, b), g over pose, a and b, because taken globally the pose entries
(1e9) would hide the brightness ones; the step within 1e-3 of the largest reference entry of each part (pose, a, b, δρ);
model decrease 1e-3; candidate cost 1e-5.  Every test prints what it measured; DESIGN.md §20 holds the worst values.

Measured (MI355X), worst over the six-keyframe cases: cost 3.9e-8; S 5.5e-7 / 1.0e-6 / 6.4e-7; g 4.4e-7 / 1.4e-7 /
1.4e-7; step pose 4.4e-7, a 3.7e-6, b 4.2e-7, δρ 9.5e-7; model decrease 5.4e-8; candidate cost 4.2e-7.  Graphs: step
pose 1.2e-5, everything else below 1.2e-6.  solve_joint: the reference's eight decisions, final cost 9587.087.
"""
import numpy as np
import pytest

import gn_affine_reference as GA
import gn_joint_reference as R
import graph_problems as G
from helpers import engine_module, synth

pytestmark = pytest.mark.gpu
E = engine_module()
INVALID_ARGUMENT = "invalid argument"
NOT_READY = "not ready"
FIXED, FIXED_AB, HUBER = R.FIXED, R.FIXED_AB, R.HUBER
ALTERNATION_END = 9773.35  # three rounds of solve and solve_affine, 36 trials
JOINT_END = 9587.087       # the dense fp64 joint LM after 8 trials at the default options


def open_engine(pb, ab=None, huber=HUBER, fixed=FIXED, fixed_ab=FIXED_AB, affine=True):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array(fixed, np.int32))
    eng.set_state(pb.poses, pb.rho)
    if affine:
        eng.set_affine_brightness(True)
        if ab is not None:
            eng.set_affine_state(ab)
        eng.set_fixed_affine_frames(np.array(fixed_ab, np.int32))
    return eng


def engine_step(eng, lam):
    """One host-driven step: (cost, model decrease, S, g, keyframe step, δρ)."""
    c = eng.joint_linearize()
    m, st = eng.joint_step(lam)
    assert st == 0
    S, g = eng.joint_get_reduced_system()
    dk, dr = eng.joint_get_step()
    return c, m, S, g, dk, dr


def part_err(got, ref):
    """max |got − ref| over the largest |ref| (a part that is zero in the reference must be zero)."""
    top = np.abs(ref).max(initial=0.0)
    if top == 0.0:
        assert not np.any(got)
        return 0.0
    return float(np.abs(got - ref).max() / top)


def check_joint(label, pb, ab, lam, lin, eng, huber=HUBER, fixed=FIXED, fixed_ab=FIXED_AB):
    """The engine's system and step at λ against the reference linearisation `lin` = (H, g, cost[, …]); the candidate
    cost against the reference cost at the ENGINE's candidate."""
    H, g_ref, c_ref = lin[:3]
    nf = pb.n_frames
    S_ref, gS_ref, dk_ref, dl_ref, m_ref, fx = R.schur_step(H, g_ref, ab, nf, lam, fixed, fixed_ab)
    c, m, S, gs, dk, dr = engine_step(eng, lam)
    assert eng.joint_system_size() == 8 * nf
    c_cand = eng.joint_candidate_cost()
    poses_c, rho_c, ab_c = R.apply_step(pb.poses, pb.rho, ab, dk, dr)
    cc_ref, _ = R.candidate_cost(pb, ab_c, poses_c, rho_c, huber)
    ix = R.parts(nf)
    ip, iab = ix["pose"], np.sort(np.concatenate([ix["a"], ix["b"]]))
    err = {"cost": abs(c - c_ref) / c_ref,
           "S_pp": part_err(S[np.ix_(ip, ip)], S_ref[np.ix_(ip, ip)]),
           "S_pab": part_err(S[np.ix_(ip, iab)], S_ref[np.ix_(ip, iab)]),
           "S_abab": part_err(S[np.ix_(iab, iab)], S_ref[np.ix_(iab, iab)]),
           "g_pose": part_err(gs[ip], gS_ref[ip]), "g_a": part_err(gs[ix["a"]], gS_ref[ix["a"]]),
           "g_b": part_err(gs[ix["b"]], gS_ref[ix["b"]]),
           "step_pose": part_err(dk[:, :6], dk_ref[:, :6]), "step_a": part_err(dk[:, 6], dk_ref[:, 6]),
           "step_b": part_err(dk[:, 7], dk_ref[:, 7]), "drho": part_err(dr, dl_ref),
           "model": abs(m - m_ref) / abs(m_ref), "candidate": abs(c_cand - cc_ref) / cc_ref}
    print(f"\n{label} λ={lam}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()) + f" min ρ+δρ {rho_c.min():.3g}")
    assert np.array_equal(S, S.T)
    assert np.array_equal(S[fx][:, fx], np.eye(int(fx.sum()))) and not S[fx][:, ~fx].any() and not gs[fx].any()
    assert not dk.ravel()[fx].any()
    assert err["cost"] <= 1e-5, err
    assert max(err[k] for k in ("S_pp", "S_pab", "S_abab", "g_pose", "g_a", "g_b")) <= 1e-4, err
    assert max(err[k] for k in ("step_pose", "step_a", "step_b", "drho", "model")) <= 1e-3, err
    assert err["candidate"] <= 1e-5, err
    return err, fx


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items()) or "base"


# 1. system and step: 1–4 rows per lane, an odd P, a partial last pass; pinhole and KB4; both interpolators; two cameras;
# block counts that are no multiple of 32 either way; a keyframe without a valid block; Huber 9, 60 and off
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
@pytest.mark.parametrize("case", R.CASES, ids=case_id)
def test_system_and_step(case, lam):
    kw = dict(case)
    huber = kw.pop("huber", HUBER)
    pb = R.problem(**kw)
    ab = R.state(pb)
    lin = R.reference(huber=huber, **kw)
    with open_engine(pb, ab, huber=huber) as eng:
        _, fx = check_joint(case_id(case), pb, ab, lam, lin, eng, huber)
        assert np.array_equal(eng.get_affine_state(), ab)  # a step moves nothing
        fx = fx.reshape(-1, 8)
        assert fx[0].all() and fx[1, :6].all() and not fx[1, 6:].any() and not fx[[2, 4, 5]].any()
        assert fx[3].all() == bool(kw.get("turned"))  # no valid block: all 8 unknowns constant, no step
        if kw.get("turned"):
            assert lin[3] == 483 and not eng.joint_get_step()[0][3].any()
        else:
            assert lin[3] == pb.n_blocks


# pyramid level 1: the level's images, cameras and points; (a, b) carry no level factor
def test_system_and_step_at_level_1():
    pb = R.problem()
    ab = R.state(pb)
    with open_engine(pb, ab) as eng:
        eng.build_pyramid(2)
        eng.set_level(1)
        pb1 = synth.level_problem(pb, 1, host_intensity=eng.host_intensities())
        pb1.interp = 0
        nv = []
        lin = R.linearize(pb1, ab, pb.poses, pb.rho, HUBER, nv)
        assert nv[0] > 0.8 * pb.n_blocks
        check_joint("level 1", pb1, ab, 1e-3, lin, eng)


# the two halves of a keyframe are independent: keyframe 1's pose constant and its (a, b) free, keyframe 2's (a, b)
# constant and its pose free
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_halves_are_independent(lam):
    pb = R.problem()
    ab = R.state(pb)
    with open_engine(pb, ab, fixed_ab=(0, 2)) as eng:
        _, fx = check_joint("halves", pb, ab, lam, R.reference(), eng, fixed_ab=(0, 2))
        fx = fx.reshape(-1, 8)
        assert fx[1, :6].all() and not fx[1, 6:].any() and fx[2, 6:].all() and not fx[2, :6].any()
        dk, _ = eng.joint_get_step()
        assert dk[1, 6:].all() and not dk[1, :6].any() and dk[2, :6].all() and not dk[2, 6:].any()


# 2. the linearisation's cost is the evaluation's (evaluate + get_cost: the record path's r)
@pytest.mark.parametrize("P", [8, 21])
def test_linearisation_cost_is_the_evaluation_cost(P):
    pb = R.problem(P=P)
    ab = R.state(pb)
    with open_engine(pb, ab) as eng:
        c_lin = eng.joint_linearize()
        eng.evaluate(False)
        c_eval, n_valid = eng.cost()
    print(f"\nP {P}: joint linearise {c_lin!r} evaluate {c_eval!r}")
    assert n_valid == pb.n_blocks and abs(c_lin - c_eval) <= 1e-6 * c_eval


# 3. with every (a, b) constant the joint step is the geometry step at that state (pba_gn_step under
# pba_gn_set_solve_affine), within the step bounds
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_constant_brightness_is_the_geometry_step(lam):
    pb = R.problem()
    ab = R.state(pb)
    with open_engine(pb, ab, fixed_ab=tuple(range(pb.n_frames))) as eng:
        c, m, S, g, dk, dr = engine_step(eng, lam)
        eng.gn_set_solve_affine(True)
        c_gn = eng.gn_linearize()
        m_gn, st = eng.gn_step(lam)
        dp_gn, dr_gn = eng.gn_last_step()
    err = {"cost": abs(c - c_gn) / c_gn, "step_pose": part_err(dk[:, :6], dp_gn), "drho": part_err(dr, dr_gn),
           "model": abs(m - m_gn) / abs(m_gn)}
    print(f"\nconstant brightness λ={lam}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert st == 0 and not dk[:, 6:].any() and dp_gn.any()
    assert err["cost"] <= 1e-6 and max(err[k] for k in ("step_pose", "drho", "model")) <= 1e-3, err


# 4. keyframe graphs: a band, loop closures (fill in the profile) and an idle keyframe
@pytest.mark.parametrize("name", ["band37", "closed100", "closed100_idle"])
def test_graphs(name):
    pb = G.problem(name, changed=True)
    ab = R.state(pb)
    nv = []
    lin = R.linearize(pb, ab, pb.poses, pb.rho, HUBER, nv)
    with open_engine(pb, ab) as eng:
        for lam in (1e-4, 1e-1):
            _, fx = check_joint(name, pb, ab, lam, lin, eng)
        if name == "closed100_idle":
            assert fx.reshape(-1, 8)[50].all()


def same_lm(summ, its, ref):
    """The engine's trajectory against the reference loop's: the decisions, the trial costs and the end."""
    poses, rho, ab, c0, c1, it, info = ref
    print(f"\nsolve_joint: {summ}\ncosts {its['cost']}\nreference: {c0} -> {c1}, {it} iterations, {info}")
    assert abs(summ["initial_cost"] - c0) <= 1e-5 * c0
    assert summ["iterations"] == it and summ["stop_reason"] == info["stop_reason"], (summ, info)
    assert summ["successful_steps"] == info["successful_steps"], (summ, info)
    assert summ["unsuccessful_steps"] == info["unsuccessful_steps"], (summ, info)
    assert (summ["termination"] == 0) == info["converged"], (summ, info)
    assert its["step_is_successful"][1:].astype(bool).tolist() == info["decisions"]
    trial = np.array(info["trial_costs"])  # an accepted entry holds the new cost, a rejected one the candidate's
    assert np.abs(its["cost"][1:] - trial).max() <= 1e-5 * trial.max(), (its["cost"], trial)
    # (the relative decreases are printed, not bounded: late in the run the cost falls by 0.14 of 9587, so the cost
    # bound alone lets them move by more than the decisions' 0.1 margin would suggest — the decisions are the check)
    print("relative decreases", its["relative_decrease"][1:], "reference", info["rel"])
    assert abs(summ["final_cost"] - c1) <= 1e-5 * c1, (summ, c1)


# 5. solve_joint from (a, b) = 0 on the base problem: the reference's decisions and trial costs for 8 iterations at the
# default options, and the feature's point — the end lies below the alternation's
def test_solve_joint_matches_reference_lm():
    pb = R.problem()
    ref = R.lm_reference()
    p_ref, r_ref, ab_ref = ref[:3]
    with open_engine(pb, None) as eng:
        summ = eng.solve_joint(max_iterations=R.LM_ITERATIONS)
        its = eng.solver_iterations()
        poses, rho = eng.get_state()
        ab = eng.get_affine_state()
        c_after = eng.joint_linearize()
    same_lm(summ, its, ref)
    assert abs(summ["final_cost"] - JOINT_END) <= 1e-5 * JOINT_END
    assert summ["final_cost"] < ALTERNATION_END
    # the state is the accepted candidate; the constants are bit for bit what they were
    assert abs(c_after - summ["final_cost"]) <= 1e-9 * c_after
    assert np.array_equal(poses[:2], pb.poses[:2]) and np.array_equal(ab[0], np.zeros(2))
    np.testing.assert_allclose(poses[:, 4:], p_ref[:, 4:], atol=1e-5)
    np.testing.assert_allclose(rho, r_ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ab, ab_ref, atol=1e-3)
    assert np.abs(ab[1:]).min() > 0


def test_solve_joint_rejects_a_trial():
    pb = R.problem()
    ref = R.lm_reference(**R.LM_REJECT)
    assert ref[6]["successful_steps"] >= 2 and ref[6]["unsuccessful_steps"] >= 1
    with open_engine(pb, None) as eng:
        summ = eng.solve_joint(**R.LM_REJECT)
        its = eng.solver_iterations()
    same_lm(summ, its, ref)


# the trial that meets the function tolerance is not applied: one iteration, the state bit for bit the initial one
def test_solve_joint_function_tolerance_applies_nothing():
    pb = R.problem()
    with open_engine(pb, None) as eng:
        before = (*eng.get_state(), eng.get_affine_state())
        summ = eng.solve_joint(function_tolerance=1.0)
        its = eng.solver_iterations()
        after = (*eng.get_state(), eng.get_affine_state())
    print(f"\nsolve_joint(function_tolerance=1): {summ}")
    assert summ["iterations"] == 1 and summ["stop_reason"] == "function_tolerance" and summ["termination"] == 0
    assert summ["successful_steps"] == 0 and summ["unsuccessful_steps"] == 0 and len(its["cost"]) == 1
    assert summ["final_cost"] == summ["initial_cost"] > 0
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


# 6. reproducible: two engines, two runs each — the system, the step and the solve bitwise equal
def test_reproducible():
    pb = R.problem(P=12, cams=2)
    ab = R.state(pb)
    out = []
    for _ in range(2):
        with open_engine(pb, ab) as eng:
            for _ in range(2):
                eng.set_state(pb.poses, pb.rho)
                eng.set_affine_state(ab)
                c, m, S, g, dk, dr = engine_step(eng, 1e-3)
                summ = eng.solve_joint(max_iterations=4)
                out.append((np.array([c, m, summ["final_cost"]]), S, g, dk, dr, *eng.get_state(), eng.get_affine_state()))
    assert out[0][1].any() and out[0][3].any() and not np.array_equal(out[0][7], ab)
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


# 7. refusals and staleness, each leaving the engine as it was
def joint_calls(eng):
    return (eng.joint_linearize, eng.joint_system_size, lambda: eng.joint_step(1e-3), eng.joint_get_reduced_system,
            eng.joint_get_step, eng.joint_candidate_cost, eng.joint_accept, eng.solve_joint)


def test_refusals():
    pb = R.problem()
    ab = R.state(pb)
    with open_engine(pb, affine=False) as eng:  # photometric, affine brightness off
        c = eng.gn_linearize()
        for call in joint_calls(eng):
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                call()
        assert eng.gn_linearize() == c
    pg = synth.make_problem(kind=1, n_frames=6, n_points=40, width=376, height=240, seed=13, border=12)
    with E.Engine(pg.kind, pg.model, huber_width=1.0) as eng:  # geometric
        eng.set_problem(pg)
        eng.set_state(pg.poses, pg.rho)
        for call in joint_calls(eng):
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                call()
    with open_engine(pb, ab) as eng:
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.joint_step(-1.0)
        # a call before the one it follows
        for call in (lambda: eng.joint_step(1e-3), eng.joint_get_reduced_system, eng.joint_get_step,
                     eng.joint_candidate_cost, eng.joint_accept):
            with pytest.raises(E.PbaError, match=NOT_READY):
                call()
        c = eng.joint_linearize()
        for call in (eng.joint_get_reduced_system, eng.joint_get_step, eng.joint_candidate_cost, eng.joint_accept):
            with pytest.raises(E.PbaError, match=NOT_READY):  # the linearisation stands, but there is no step yet
                call()
        assert np.array_equal(eng.get_affine_state(), ab) and np.array_equal(eng.get_state()[0], pb.poses)
        m, st = eng.joint_step(1e-3)
        assert st == 0 and m > 0 and eng.joint_linearize() == c
        # the on-device Gauss-Newton still refuses by default, and the joint solve goes on
        for call in (eng.gn_linearize, lambda: eng.gn_step(1e-3), lambda: eng.solve(max_iterations=2)):
            with pytest.raises(E.PbaError, match="affine brightness"):
                call()
        assert eng.joint_step(1e-3) == (m, st)


def test_staleness():
    pb = R.problem()
    ab = R.state(pb)

    def stale(eng):
        for call in (lambda: eng.joint_step(1e-3), eng.joint_candidate_cost, eng.joint_accept, eng.joint_get_step,
                     eng.joint_get_reduced_system):
            with pytest.raises(E.PbaError, match=NOT_READY):
                call()

    with open_engine(pb, ab) as eng:
        eng.build_pyramid(2)

        def fresh():
            c = eng.joint_linearize()
            assert eng.joint_step(1e-3)[1] == 0
            return c

        def affine_accept():
            eng.affine_linearize()
            eng.affine_step(1e-1)
            eng.affine_accept()

        def gn_accept():
            eng.gn_set_solve_affine(True)
            eng.gn_linearize()
            eng.gn_step(1e-1)
            eng.gn_accept()
            eng.gn_set_solve_affine(False)

        changes = (lambda: eng.set_state(pb.poses, pb.rho), lambda: eng.set_affine_state(ab),
                   lambda: eng.set_fixed_frames(np.array(FIXED, np.int32)),
                   lambda: eng.set_fixed_affine_frames(np.array(FIXED_AB, np.int32)),
                   lambda: eng.set_level(1), lambda: eng.set_level(0), eng.joint_accept, affine_accept, gn_accept)
        c0 = fresh()
        for change in changes:
            change()
            stale(eng)
            fresh()
        # back at the first state, the first linearisation
        eng.set_state(pb.poses, pb.rho)
        eng.set_affine_state(ab)
        assert fresh() == c0
        # accept moves poses, ρ and the affine state to the candidate
        dk, dr = eng.joint_get_step()
        c_cand = eng.joint_candidate_cost()
        eng.joint_accept()
        poses, rho = eng.get_state()
        p_ref, r_ref, ab_ref = R.apply_step(pb.poses, pb.rho, ab, dk, dr)
        np.testing.assert_allclose(poses, p_ref, atol=1e-10)
        np.testing.assert_allclose(rho, r_ref, rtol=1e-12)
        np.testing.assert_allclose(eng.get_affine_state(), ab_ref, rtol=1e-12, atol=1e-300)
        assert abs(eng.joint_linearize() - c_cand) <= 1e-6 * c_cand
