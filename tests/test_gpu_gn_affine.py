"""The on-device Gauss-Newton at a constant affine brightness state: pba_set_affine_brightness + pba_gn_set_solve_affine.

With the switch on, gn_linearize / gn_step / gn_candidate_cost / gn_accept, gn_reduced_system / gn_last_step, solve and
solve_pyramid run with r_k = (I_t − b_t) − E·(I_h,k − b_h) at the engine's affine state and leave that state alone.
Reference: tests/gn_affine_reference.py (dense fp64 over photometric_affine_reference.compose's first 14·P columns;
tests/test_gn_affine_reference.py asserts on the CPU the input conditions under which the bounds here mean something).

Problems: 6 keyframes, 161 points, 376×240, 644 blocks (4 past a multiple of 32), the brightness-changed images of
brightness_case with poses and ρ perturbed; affine state parity_state; keyframes 0 and 1 fixed.  Huber widths 9 (at
parity_state nearly every block is past it: the median ‖r‖ is 105), 60 (a quarter of the blocks inside) and off.

Bounds (the project's for photometric Gauss-Newton, tests/test_gpu_gn.py): cost 1e-5 relative; S and g within 1e-4 of
their largest entry; pose step, δρ and model decrease within 1e-3; candidate cost 1e-5.  At the zero state everything
is the plain engine's bit for bit.

Measured (MI355X), worst over the 32 step cases: cost 3.9e-8, S 3.5e-7, g 3.6e-7, pose step 2.0e-6,
δρ 5.0e-7, model decrease 1.8e-7, candidate cost 5.0e-8; the linearisation's cost against the evaluation's: equal.
The brightness solve (pba_affine_*, pba_solve_affine) against reference (ii), worst over its 32 cases: cost 3.9e-8,
H 3.9e-7, g 2.4e-7, δ 1.7e-7, model decrease 3.7e-8, candidate cost 2.5e-7; solve_affine on brightness_case ends at
2113.30404 (reference 2113.30391); three rounds of solve and solve_affine end at 9773.3511 (reference 9773.3504).
"""
import numpy as np
import pytest

import gn_affine_reference as R
import gn_reference as GR
from helpers import engine_module, synth

pytestmark = pytest.mark.gpu
E = engine_module()
INVALID_ARGUMENT = "invalid argument"
FIXED, HUBER = R.FIXED, R.HUBER
KB4 = synth.KB4


def open_engine(pb, ab=None, huber=HUBER, fixed=FIXED, library=None, affine=True, switch=True):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber, library=library)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array(fixed, np.int32))
    eng.set_state(pb.poses, pb.rho)
    if affine:
        eng.set_affine_brightness(True)
        if ab is not None:
            eng.set_affine_state(ab)
        if switch:
            eng.gn_set_solve_affine(True)
    return eng


def engine_step(eng, lam):
    """One host-driven step: (cost, model decrease, S, g, pose step, δρ)."""
    c = eng.gn_linearize()
    m, st = eng.gn_step(lam)
    assert st == 0
    S, g = eng.gn_reduced_system()
    dp, dr = eng.gn_last_step()
    return c, m, S, g, dp, dr


def check_step(label, pb, ab, lam, lin, eng, huber=HUBER):
    """The engine's system and step at λ against the reference linearisation `lin` = (H, g, cost) and against
    reduced_system_from_records; the candidate cost against compose at the ENGINE's candidate."""
    H, g_ref, c_ref = lin
    S_ref, gS_ref, dp_ref, dl_ref, m_ref = GR.schur_step(H, g_ref, pb.n_frames, lam, FIXED)
    S_rec, g_rec, c_rec = R.reduced_system(pb, ab, huber, lam, FIXED)
    c, m, S, gs, dp, dr = engine_step(eng, lam)
    c_cand = eng.gn_candidate_cost()
    cc_ref, _ = R.cost_at(pb, ab, synth.se3_plus(pb.poses, dp), pb.rho + dr, huber)

    def part(a, b):
        return np.abs(a - b).max() / np.abs(b).max()

    err = {"cost": abs(c - c_ref) / c_ref, "S": part(S, S_ref), "g": part(gs, gS_ref),
           "S_records": part(S, S_rec), "g_records": part(gs, g_rec),
           "step": np.linalg.norm(dp - dp_ref) / np.linalg.norm(dp_ref),
           "drho": np.linalg.norm(dr - dl_ref) / np.linalg.norm(dl_ref),
           "model": abs(m - m_ref) / abs(m_ref), "candidate": abs(c_cand - cc_ref) / cc_ref}
    print(f"\n{label} λ={lam}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert abs(c_rec - c_ref) <= 1e-12 * c_ref
    assert err["cost"] <= 1e-5, err
    assert err["S"] <= 1e-4 and err["g"] <= 1e-4 and err["S_records"] <= 1e-4 and err["g_records"] <= 1e-4, err
    assert err["step"] <= 1e-3 and err["drho"] <= 1e-3 and err["model"] <= 1e-3, err
    assert err["candidate"] <= 1e-5, err
    return err


# 1. the zero state is the plain solve, bit for bit (8 px: one row per lane; 12 px: two)
@pytest.mark.parametrize("P", [8, 12])
def test_zero_state_is_the_plain_solve(P):
    pb = R.problem(P=P)
    out = []
    for affine in (False, True):
        with open_engine(pb, None, affine=affine) as eng:
            if affine:
                assert np.all(eng.get_affine_state() == 0.0)
            c, m, S, g, dp, dr = engine_step(eng, 1e-3)
            c_cand = eng.gn_candidate_cost()
            eng.set_state(pb.poses, pb.rho)
            summ = eng.solve(max_iterations=5)
            its = eng.solver_iterations()
            poses, rho = eng.get_state()
            out.append((np.array([c, m, c_cand]), S, g, dp, dr, poses, rho, its["cost"], its["step_is_successful"],
                        its["trust_region_radius"], np.array([summ["initial_cost"], summ["final_cost"]])))
    names = ("cost, model decrease, candidate cost", "S", "g", "pose step", "δρ", "final poses", "final ρ",
             "trajectory costs", "trajectory decisions", "trajectory radii", "summary costs")
    assert out[0][1].any() and out[0][3].any() and len(out[0][7]) >= 3
    for name, a, b in zip(names, *out):
        assert np.array_equal(a, b), name


# 2. geometry at a non-zero state: partial lane set (5) and 1, 2, 3, 4 rows per lane; pinhole and KB4; both
# interpolators; two cameras; a block count that is no multiple of 32 either way (637); a keyframe without a valid
# block; Huber 9, 60 and off
CASES = [
    dict(), dict(interp=1), dict(P=5), dict(P=12, interp=1), dict(P=21), dict(P=32, interp=1),
    dict(model=KB4, interp=1), dict(model=KB4, P=21), dict(P=12, cams=2), dict(cams=2), dict(drop=7),
    dict(turned=True), dict(turned=True, P=21), dict(huber=60.0), dict(huber=0.0), dict(huber=60.0, P=32),
]


@pytest.mark.parametrize("lam", [1e-4, 1e-1])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()) or "base")
def test_geometry_system_and_step(case, lam):
    kw = dict(case)
    huber = kw.pop("huber", HUBER)
    pb = R.problem(**kw)
    ab = R.state(pb)
    valid, lin, _ = R.reference(huber=huber, **kw)
    with open_engine(pb, ab, huber=huber) as eng:
        check_step(str(case), pb, ab, lam, lin, eng, huber)
        assert np.array_equal(eng.get_affine_state(), ab)  # held constant
        if kw.get("turned"):  # keyframe 3 has no valid block: nothing but the damping in its rows, no step
            assert not valid[(pb.point_host[pb.block_point] == 3) | (pb.block_target == 3)].any()
            S, g = eng.gn_reduced_system()
            rows = 18 + np.arange(6)
            off = np.delete(np.arange(S.shape[0]), rows)
            assert not S[np.ix_(rows, off)].any() and not g[rows].any()
            assert not eng.gn_last_step()[0][3].any()


# the linearisation's cost is the evaluation's (evaluate + get_cost: the record path's r), at pyramid levels 0 and 1
@pytest.mark.parametrize("P", [8, 21])
def test_linearisation_cost_is_the_evaluation_cost(P):
    pb = R.problem(P=P)
    ab = R.state(pb)
    with open_engine(pb, ab) as eng:
        eng.build_pyramid(2)
        for level in (0, 1):
            eng.set_level(level)
            c_lin = eng.gn_linearize()
            eng.evaluate(False)
            c_eval, n_valid = eng.cost()
            print(f"\nP {P} level {level}: linearise {c_lin!r} evaluate {c_eval!r}")
            assert n_valid > 0.9 * pb.n_blocks and abs(c_lin - c_eval) <= 1e-6 * c_eval
        eng.set_level(0)
        c_ref, _ = R.cost_at(pb, ab, pb.poses, pb.rho, HUBER)
        assert abs(eng.gn_linearize() - c_ref) <= 1e-5 * c_ref


# a new affine state is what the next linearisation runs at; accept moves poses and ρ only
def test_state_change_and_accept():
    pb = R.problem()
    ab = R.state(pb)
    with open_engine(pb, ab) as eng:
        c_a = eng.gn_linearize()
        eng.set_affine_state(0.5 * ab)
        c_b = eng.gn_linearize()
        eng.gn_step(1e-3)
        dp, dr = eng.gn_last_step()
        c_cand = eng.gn_candidate_cost()
        eng.gn_accept()
        poses, rho = eng.get_state()
        c_after = eng.gn_linearize()
        assert np.array_equal(eng.get_affine_state(), 0.5 * ab)
    ra, _ = R.cost_at(pb, ab, pb.poses, pb.rho, HUBER)
    rb, _ = R.cost_at(pb, 0.5 * ab, pb.poses, pb.rho, HUBER)
    assert abs(ra - rb) > 0.1 * ra  # (the two states are far apart in cost: the check below is not vacuous)
    assert abs(c_a - ra) <= 1e-5 * ra and abs(c_b - rb) <= 1e-5 * rb
    np_, nr = GR.apply_step(pb.poses, pb.rho, dp, dr)
    np.testing.assert_allclose(poses, np_, atol=1e-10)
    np.testing.assert_allclose(rho, nr, rtol=1e-12)
    assert abs(c_after - c_cand) <= 1e-6 * c_cand


# 3. solve takes the reference LM's decisions; solve_pyramid runs and leaves the affine state bit for bit
def test_solve_matches_reference_lm():
    pb = R.problem()
    ab = R.state(pb)
    p_ref, r_ref, c0_ref, c1_ref, it_ref, info = R.lm_reference()
    assert info["successful_steps"] >= 3 and info["unsuccessful_steps"] >= 1
    with open_engine(pb, ab) as eng:
        summ = eng.solve(**R.LM_OPTIONS)
        poses, rho = eng.get_state()
        its = eng.solver_iterations()
        assert np.array_equal(eng.get_affine_state(), ab)
    print(f"\nsolve: {summ}\nreference: {c0_ref} -> {c1_ref}, {it_ref} iterations, {info['history']}")
    # _same_lm (tests/test_gpu_gn.py)
    assert abs(summ["initial_cost"] - c0_ref) <= 1e-5 * c0_ref
    assert abs(summ["final_cost"] - c1_ref) <= 1e-5 * c1_ref, (summ, c1_ref)  # (the cost bound, not _same_lm's 1e-3)
    assert summ["iterations"] == it_ref, (summ, it_ref, info)
    assert summ["successful_steps"] == info["successful_steps"], (summ, info)
    assert summ["unsuccessful_steps"] == info["unsuccessful_steps"], (summ, info)
    assert summ["stop_reason"] == info["stop_reason"], (summ, info)
    assert (summ["termination"] == 0) == info["converged"], (summ, info)
    assert its["step_is_successful"][1:].astype(bool).tolist() == [h[1] for h in info["history"]]
    np.testing.assert_allclose(poses[:, 4:], p_ref[:, 4:], atol=1e-5)
    np.testing.assert_allclose(rho, r_ref, rtol=1e-4, atol=1e-6)


def test_solve_pyramid_leaves_the_affine_state():
    pb = R.problem()
    ab = R.state(pb)
    c_init, _ = R.cost_at(pb, ab, pb.poses, pb.rho, HUBER)
    with open_engine(pb, ab) as eng:
        eng.build_pyramid(2)
        summ = eng.solve_pyramid(max_iterations=4, initial_trust_region_radius=1.0)
        poses, rho = eng.get_state()
        assert eng.level()[0] == 0
        assert np.array_equal(eng.get_affine_state(), ab)
    c_final, _ = R.cost_at(pb, ab, poses, rho, HUBER)
    print(f"\nsolve_pyramid: initial {c_init:.6g} final {c_final:.6g} (summary {summ['final_cost']:.6g})")
    assert summ["successful_steps"] >= 1 and abs(summ["final_cost"] - c_final) <= 1e-5 * c_final
    assert c_final < c_init


# 7. reproducible: two engines, the system, the step and the solve bitwise equal
def test_reproducible():
    pb = R.problem(P=12, cams=2)
    ab = R.state(pb)
    out = []
    for _ in range(2):
        with open_engine(pb, ab) as eng:
            for _ in range(2):
                eng.set_state(pb.poses, pb.rho)
                c, m, S, g, dp, dr = engine_step(eng, 1e-3)
                eng.solve(max_iterations=4)
                out.append((np.array([c, m]), S, g, dp, dr, *eng.get_state()))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


# 8. refusals, each leaving the engine as it was
def test_opt_in_and_refusals(monkeypatch):
    import torch
    pb = R.problem()
    ab = R.state(pb)
    c_ref, _ = R.cost_at(pb, ab, pb.poses, pb.rho, HUBER)
    x = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    # without affine brightness the switch is refused, and the plain solve goes on
    with open_engine(pb, affine=False) as eng:
        c_plain = eng.gn_linearize()
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.gn_set_solve_affine(True)
        eng.gn_set_solve_affine(False)  # (off is always legal)
        assert eng.gn_linearize() == c_plain
    with E.Engine(synth.GEOMETRIC, synth.PINHOLE) as eng:
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.gn_set_solve_affine(True)
    with open_engine(pb, ab, switch=False) as eng:
        for call in (eng.gn_linearize, lambda: eng.gn_step(1e-3), eng.gn_candidate_cost, eng.gn_accept,
                     lambda: eng.solve(max_iterations=2), lambda: eng.solve_pyramid(max_iterations=2),
                     eng.gn_system_size, eng.gn_reduced_system):
            with pytest.raises(E.PbaError, match="affine brightness"):
                call()
        eng.gn_set_solve_affine(True)
        c = eng.gn_linearize()
        assert abs(c - c_ref) <= 1e-5 * c_ref and eng.gn_system_size() == 6 * pb.n_frames
        # the multi-GPU entry points still refuse, with the same message
        L, h = eng._L, eng._h
        for call in (lambda: eng.gn_step_export(1e-3, 4, x.data_ptr()), lambda: eng.gn_step_import(1e-3, 4, x.data_ptr()),
                     lambda: eng.solve_distributed(4, x.data_ptr(), lambda p, n: None, max_iterations=2),
                     lambda: eng._ck(L.pba_solve_distributed_comm(h, None, 1, None, None), "comm")):
            with pytest.raises(E.PbaError, match="affine brightness"):
                call()
        assert eng.gn_linearize() == c and np.array_equal(eng.get_affine_state(), ab)
        eng.gn_set_solve_affine(False)
        with pytest.raises(E.PbaError, match="affine brightness"):
            eng.gn_linearize()
        # disabling affine brightness clears the switch: enabled again, the solve refuses until asked for again
        eng.gn_set_solve_affine(True)
        eng.set_affine_brightness(False)
        assert eng.gn_linearize() > 0.0
        eng.set_affine_brightness(True)
        with pytest.raises(E.PbaError, match="affine brightness"):
            eng.gn_linearize()
    # the 14-column lineariser of the test build has no affine form
    monkeypatch.setenv("PBA_LIN_LEGACY", "1")
    with open_engine(pb, ab, library=E.TEST_LIB_PATH) as eng:
        eng.build_pyramid(2)
        for call in (eng.gn_linearize, lambda: eng.solve(max_iterations=2), lambda: eng.solve_pyramid(max_iterations=2)):
            with pytest.raises(E.PbaError, match="14-column lineariser"):
                call()
            assert eng.level()[0] == 0  # refused before a level was switched
        eng.evaluate(False)  # the engine still evaluates
        assert abs(eng.cost()[0] - c_ref) <= 1e-5 * c_ref
        eng.set_affine_brightness(False)  # and the hook's plain solve runs
        assert eng.gn_linearize() > 0.0


# ---- the brightness solve at fixed poses and ρ (pba_affine_*, pba_solve_affine) against reference (ii) ---------------
def check_brightness(label, pb, ab, huber, fixed, lam, eng):
    """affine_linearize cost, affine_system, affine_step (δ, model decrease, status), affine_candidate_cost and
    affine_accept against gn_affine_reference.linearize_ab / step_ab.  Bounds: cost 1e-5; H blocks and g within 1e-4 of
    their largest entry; δ and model decrease 1e-3; candidate cost 1e-5."""
    H_ref, g_ref, c_ref, free = R.linearize_ab(pb, ab, huber, fixed)
    d_ref, m_ref = R.step_ab(H_ref, g_ref, free, lam)
    eng.set_fixed_affine_frames(np.array(fixed, np.int32))
    c = eng.affine_linearize()
    H, g = eng.affine_system()
    m, st = eng.affine_step(lam)
    assert st == 0 and eng.affine_system_size() == 2 * pb.n_frames
    d = eng.affine_last_step()
    c_cand = eng.affine_candidate_cost()
    cc_ref = R.cost_ab(pb, ab + d, huber)
    eng.affine_accept()
    fx = np.repeat(~free, 2)
    err = {"cost": abs(c - c_ref) / c_ref, "H": np.abs(H - H_ref).max() / np.abs(H_ref).max(),
           "g": np.abs(g - g_ref).max() / np.abs(g_ref).max(),
           "step": np.linalg.norm(d - d_ref) / np.linalg.norm(d_ref), "model": abs(m - m_ref) / abs(m_ref),
           "candidate": abs(c_cand - cc_ref) / cc_ref}
    print(f"\nbrightness {label} fixed {fixed} λ={lam}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert np.array_equal(H[fx][:, fx], np.eye(int(fx.sum()))) and not H[fx][:, ~fx].any() and not g[fx].any()
    assert not d[~free].any() and np.array_equal(eng.get_affine_state(), ab + d)
    assert err["cost"] <= 1e-5 and err["H"] <= 1e-4 and err["g"] <= 1e-4, err
    assert err["step"] <= 1e-3 and err["model"] <= 1e-3 and err["candidate"] <= 1e-5, err
    return free


# 4. the brightness system: the pattern sizes and models of case 2, keyframe 0 fixed and none fixed
@pytest.mark.parametrize("fixed", [(0,), ()])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()) or "base")
def test_brightness_system_and_step(case, fixed):
    kw = dict(case)
    huber = kw.pop("huber", HUBER)
    pb = R.problem(**kw)
    ab = R.state(pb)
    with open_engine(pb, ab, huber=huber, switch=False) as eng:
        free = check_brightness(str(case), pb, ab, huber, fixed, 1e-1, eng)
    assert free[3] == (not kw.get("turned"))  # a keyframe without a valid block is constant


def test_brightness_non_finite_a():
    """A keyframe with a non-finite a: its blocks are invalid and contribute nothing; it is constant."""
    pb = R.problem()
    ab = R.state(pb)
    ab[3, 0] = np.nan
    H_ref, g_ref, c_ref, free = R.linearize_ab(pb, ab, HUBER, (0,))
    assert not free[3] and free[[1, 2, 4, 5]].all()
    with open_engine(pb, ab, switch=False) as eng:
        eng.set_fixed_affine_frames(np.array([0], np.int32))
        c = eng.affine_linearize()
        H, g = eng.affine_system()
        m, st = eng.affine_step(1e-1)
        d = eng.affine_last_step()
    d_ref, m_ref = R.step_ab(H_ref, g_ref, free, 1e-1)
    assert st == 0 and abs(c - c_ref) <= 1e-5 * c_ref and not d[3].any() and not d[0].any()
    assert np.abs(H - H_ref).max() <= 1e-4 * np.abs(H_ref).max() and np.abs(g - g_ref).max() <= 1e-4 * np.abs(g_ref).max()
    assert np.linalg.norm(d - d_ref) <= 1e-3 * np.linalg.norm(d_ref) and abs(m - m_ref) <= 1e-3 * abs(m_ref)


# 5. brightness comes back on the device
def test_solve_affine_brings_brightness_back():
    import photometric_affine_reference as PAR
    pb, gain, offset = PAR.brightness_case()
    ab_ref, c0_ref, c1_ref, it_ref, info = R.lm_ab(pb, np.zeros((pb.n_frames, 2)), 0.0, (0,))
    c_run, _ = PAR.brightness_run(lambda s: PAR.compose(pb, s)[:2], pb)
    with open_engine(pb, None, huber=0.0, fixed=(), switch=False) as eng:
        eng.set_fixed_affine_frames(np.array([0], np.int32))
        summ = eng.solve_affine()
        its = eng.solver_iterations()
        ab = eng.get_affine_state()
    print(f"\nsolve_affine: {summ}\nreference: {c0_ref} -> {c1_ref}, {it_ref} iterations, {info}\nbrightness_run {c_run}")
    assert abs(summ["initial_cost"] - c0_ref) <= 1e-5 * c0_ref
    assert summ["iterations"] == it_ref and summ["stop_reason"] == info["stop_reason"], (summ, info)
    assert summ["successful_steps"] == info["successful_steps"], (summ, info)
    assert summ["unsuccessful_steps"] == info["unsuccessful_steps"], (summ, info)
    assert its["step_is_successful"][1:].astype(bool).tolist() == info["decisions"][:len(its["cost"]) - 1]
    assert abs(summ["final_cost"] - c_run[-1]) <= 1e-3 * c_run[-1]
    assert abs(summ["final_cost"] - c1_ref) <= 1e-5 * c1_ref
    assert np.abs(ab - ab_ref).max() <= 1e-3 and not ab[0].any()


# the trial that meets the function tolerance is not applied: one iteration, the state bit for bit the initial one
def test_solve_affine_function_tolerance_applies_nothing():
    pb = R.problem()
    with open_engine(pb, None, switch=False) as eng:
        eng.set_fixed_affine_frames(np.array([0], np.int32))
        before = (*eng.get_state(), eng.get_affine_state())
        summ = eng.solve_affine(function_tolerance=1.0)
        its = eng.solver_iterations()
        after = (*eng.get_state(), eng.get_affine_state())
    print(f"\nsolve_affine(function_tolerance=1): {summ}")
    assert summ["iterations"] == 1 and summ["stop_reason"] == "function_tolerance" and summ["termination"] == 0
    assert summ["successful_steps"] == 0 and summ["unsuccessful_steps"] == 0 and len(its["cost"]) == 1
    assert summ["final_cost"] == summ["initial_cost"] > 0
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


# 6. in turn: three rounds of solve, then solve_affine
def test_alternation():
    pb = R.problem()
    plain = R.problem(changed=True)
    kw = dict(max_iterations=6, initial_trust_region_radius=1.0)
    with open_engine(plain, affine=False) as eng:  # the plain solve on the same images, affine brightness off
        c_plain = eng.solve(max_iterations=40, initial_trust_region_radius=1.0)["final_cost"]
    costs, ref = [], []
    with open_engine(pb, None) as eng:
        eng.set_fixed_affine_frames(np.array([0], np.int32))
        costs.append(eng.gn_linearize())
        for _ in range(3):
            costs.append(eng.solve(**kw)["final_cost"])
            costs.append(eng.solve_affine(**kw)["final_cost"])
    ab, poses, rho = np.zeros((pb.n_frames, 2)), pb.poses, pb.rho
    ref.append(R.cost_at(pb, ab, poses, rho, HUBER)[0])
    decisions_agree = True
    for _ in range(3):
        import dataclasses
        poses, rho, _, c, _, info = R.lm(dataclasses.replace(pb, poses=poses, rho=rho), ab, HUBER, FIXED, summary=True,
                                         max_iterations=6, radius=1.0)
        ref.append(c)
        ab, _, c, _, _ = R.lm_ab(pb, ab, HUBER, (0,), max_iterations=6, radius=1.0, poses=poses, rho=rho)
        ref.append(c)
    print(f"\nalternation: engine {costs}\nreference {ref}\nplain solve {c_plain}")
    assert all(b <= a * (1 + 1e-12) for a, b in zip(costs, costs[1:]))  # never rises across calls
    assert costs[-1] < c_plain
    assert abs(costs[-1] - ref[-1]) <= 1e-3 * ref[-1], (costs, ref)


# 7. reproducible: the brightness system, step and solve_affine result bitwise equal
def test_brightness_reproducible():
    pb = R.problem(P=12, cams=2)
    ab = R.state(pb)
    out = []
    for _ in range(2):
        with open_engine(pb, ab, switch=False) as eng:
            for _ in range(2):
                eng.set_affine_state(ab)
                eng.set_fixed_affine_frames(np.array([0], np.int32))
                c = eng.affine_linearize()
                H, g = eng.affine_system()
                m, st = eng.affine_step(1e-2)
                d = eng.affine_last_step()
                eng.solve_affine(max_iterations=4)
                out.append((np.array([c, m]), H, g, d, eng.get_affine_state()))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


# 8. refusals of the brightness entry points, each leaving the engine as it was
def test_brightness_refusals():
    pb = R.problem()
    ab = R.state(pb)

    def calls(eng):
        return (lambda: eng.set_fixed_affine_frames(np.array([0], np.int32)), eng.affine_linearize, eng.affine_system_size,
                eng.affine_system, lambda: eng.affine_step(1e-3), eng.affine_last_step, eng.affine_candidate_cost,
                eng.affine_accept, eng.solve_affine)

    with open_engine(pb, affine=False) as eng:  # photometric, affine brightness off
        c = eng.gn_linearize()
        for call in calls(eng):
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                call()
        assert eng.gn_linearize() == c
    pg = synth.make_problem(kind=1, n_frames=6, n_points=40, width=376, height=240, seed=13, border=12)
    with E.Engine(pg.kind, pg.model, huber_width=1.0) as eng:
        eng.set_problem(pg)
        eng.set_state(pg.poses, pg.rho)
        for call in calls(eng):
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                call()
    with open_engine(pb, ab, switch=False) as eng:
        eng.set_fixed_affine_frames(np.array([0], np.int32))
        c = eng.affine_linearize()
        for bad in ([-1], [pb.n_frames], [0, 99]):
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.set_fixed_affine_frames(np.array(bad, np.int32))
        with pytest.raises(E.PbaError, match="not ready"):  # the linearisation stands, but there is no step yet
            eng.affine_candidate_cost()
        assert eng.affine_linearize() == c and np.array_equal(eng.get_affine_state(), ab)
        H, _ = eng.affine_system()
        assert np.array_equal(H[:2, :2], np.eye(2))  # keyframe 0 is still the fixed one
