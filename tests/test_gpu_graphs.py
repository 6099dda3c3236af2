"""The on-device solves on two-way and loop-closed keyframe graphs (tests/graph_problems.py).

Every other GPU test takes its blocks from synth.make_problem, whose targets are host+1 … host+4: no keyframe observes a
point hosted by a later one, and a row of the brightness system is at most 12 scalars wide.  Here the pairs run both ways
(band37), and loop closures make rows 63/64, 65/66, 129/130 and 199/200 scalars wide (closed100: the 64-lane strides of
affine_factor_kernel from both sides, more than 256 pairs and skyline blocks, envelope blocks no pair fills), with a
keyframe without any block inside the wide rows (closed100_idle).  tests/test_graph_problems.py asserts that structure
and the references' sensitivity on the CPU.

Groups: a. the pose system, plain photometric, under every reduced solver; b. geometric; c. the brightness system and step
(check_brightness of tests/test_gpu_gn_affine.py); d. geometry at a constant affine state; e. pba_solve and
pba_solve_affine against the reference loops; f. bitwise reproducibility at width; g. free intrinsics.

Bounds (the project's): cost 1e-5 relative; S, H and g within 1e-4 of their largest entry; pose step, δρ, brightness step
and model decrease 1e-3; candidate cost 1e-5; free geometric intrinsics cost 1e-6, S and g 1e-5.  All references are
dense fp64 on the CPU.

Measured (MI355X), worst per group:
  a (24 cases)  cost 1.4e-8, S 8.4e-8, g 5.3e-8, pose step 1.8e-6, δρ 5.5e-7, model decrease 9.6e-9, candidate 2.2e-8
  b (6 cases)   cost 1.6e-8, S 1.0e-7, g 3.6e-8, pose step 5.6e-6, δρ 4.5e-6, model decrease 1.7e-8, candidate 1.7e-8
  c (28 cases)  cost 2.8e-8, H 1.4e-7, g 2.0e-7, brightness step 5.2e-7, model decrease 2.6e-8, candidate 4.8e-8
  d (2 cases)   cost 2.8e-8, S 1.1e-7, g 1.1e-7, pose step 8.3e-6, δρ 2.6e-7, model decrease 6.5e-9, candidate 3.0e-8
  e             solve ends at 103206.4478 (reference 103206.4507, 2.8e-8) with the reference's AAArrrrrAA;
                solve_affine at 3758311.83 (reference 3758311.89, 1.5e-8) with its AAArrrr
  f             bitwise equal
  g             geometric: cost 2.0e-8, S 4.1e-8, g 2.6e-8, step 7.1e-8, δρ 1.1e-7, model decrease 8.2e-9;
                photometric: cost 1.7e-8, S parts 1.4e-7, g 4.5e-8, step 1.7e-7, δρ 2.4e-7, model 9.6e-10, candidate 1.3e-8
"""
import numpy as np
import pytest

import gn_affine_reference as R
import gn_reference as GR
import graph_problems as G
import photometric_affine_reference as PAR
import test_gpu_gn_affine as TA
from helpers import engine_module, synth

pytestmark = pytest.mark.gpu
E = engine_module()
FIXED = G.FIXED
WORST = {}  # group → quantity → the worst error so far (printed as the cases go)


def note(group, err):
    w = WORST.setdefault(group, {})
    for k, v in err.items():
        w[k] = max(w.get(k, 0.0), float(v))
    print(f"worst so far, group {group}: " + " ".join(f"{k} {v:.2e}" for k, v in w.items()))


def printed_errors(capsys):
    """The figures of check_brightness's last line "brightness …: name value name value …" (it returns none of them)."""
    out = capsys.readouterr().out
    print(out, end="")
    words = [l for l in out.splitlines() if l.startswith("brightness ")][-1].split(": ")[1].split()
    return dict(zip(words[::2], map(float, words[1::2])))


def plain_engine(pb, huber, fixed=FIXED):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array(fixed, np.int32))
    eng.set_state(pb.poses, pb.rho)
    return eng


def check_pose_step(label, pb, lam, ref, eng, huber):
    """TA.check_step for either residual kind at the zero affine state: the engine's system and step at λ against the
    reference linearisation and against reduced_system_from_records; the candidate cost at the ENGINE's candidate."""
    rec, valid, (H, g_ref, c_ref) = ref
    S_ref, gS_ref, dp_ref, dl_ref, m_ref = GR.schur_step(H, g_ref, pb.n_frames, lam, FIXED)
    S_rec, g_rec, c_rec = GR.reduced_system_from_records(pb, rec, valid, huber, lam, FIXED)
    c, m, S, gs, dp, dr = TA.engine_step(eng, lam)
    c_cand = eng.gn_candidate_cost()
    cc_ref = G.candidate_cost(pb, None, synth.se3_plus(pb.poses, dp), pb.rho + dr, huber)

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


# a. the pose system, plain photometric: the default solver and every forced one, each against the reference
VARIANTS = {"band37": [{}, {"PBA_SOLVER": "cr"}, {"PBA_SOLVER": "band"}, {"PBA_SOLVER": "skyline"}],
            "closed100": [{}, {"PBA_SKYLINE_GLOBAL": "1"}]}


@pytest.mark.parametrize("lam", G.LAMBDAS)
@pytest.mark.parametrize("name,huber,env", [(n, h, v) for n, h in G.POSE_CASES for v in VARIANTS[n]],
                         ids=lambda x: "-".join(f"{k}={v}" for k, v in x.items()) or "default" if isinstance(x, dict) else str(x))
def test_pose_system_photometric(name, huber, env, lam, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pb = G.problem(name)
    with plain_engine(pb, huber) as eng:
        err = check_pose_step(f"{name} Huber {huber} {env}", pb, lam, G.pose_reference(name, huber), eng, huber)
    note("a", err)


# b. the pose system, geometric, Huber 1
@pytest.mark.parametrize("lam", G.LAMBDAS)
@pytest.mark.parametrize("name,model", G.GEOMETRIC_CASES)
def test_pose_system_geometric(name, model, lam):
    pb = G.problem(name, kind=synth.GEOMETRIC, model=model)
    ref = G.pose_reference(name, 1.0, kind=synth.GEOMETRIC, model=model)
    with plain_engine(pb, 1.0) as eng:
        err = check_pose_step(f"geometric {name} model {model}", pb, lam, ref, eng, 1.0)
    note("b", err)


# c. the brightness system and step at parity_state: wide rows, both directions, constant keyframes inside wide rows
@pytest.mark.parametrize("lam", G.LAMBDAS)
@pytest.mark.parametrize("name,P,huber,fixed", G.BRIGHTNESS_CASES)
def test_brightness_system_and_step(name, P, huber, fixed, lam, capsys):
    pb = G.problem(name, P=P, changed=True)
    ab = PAR.parity_state(pb.n_frames)
    H_ref, _, _, free_ref = R.linearize_ab(pb, ab, huber, fixed)
    with TA.open_engine(pb, ab, huber=huber, switch=False) as eng:
        free = TA.check_brightness(f"{name} P {P} Huber {huber}", pb, ab, huber, fixed, lam, eng)
        moved = eng.get_affine_state()  # (check_brightness accepted its step)
        eng.set_affine_state(ab)
        eng.affine_linearize()
        H, g = eng.affine_system()
    note("c", printed_errors(capsys))
    constant = set(fixed) | ({50} if name == "closed100_idle" else set())
    assert np.array_equal(free, free_ref) and set(np.nonzero(~free)[0].tolist()) == constant
    assert not H[H_ref == 0.0].any()  # outside the pairs — the envelope blocks no pair fills included — exactly zero
    if name == "closed100_idle":  # the idle keyframe: identity rows, a zero gradient and a zero step
        assert not free[50] and 50 not in fixed
        rows = np.array([100, 101])
        off = np.delete(np.arange(2 * pb.n_frames), rows)
        assert np.array_equal(H[np.ix_(rows, rows)], np.eye(2)) and not H[np.ix_(rows, off)].any()
        assert not g[rows].any() and np.array_equal(moved[50], ab[50])


# d. geometry at a constant affine state on a two-way graph
@pytest.mark.parametrize("lam", G.LAMBDAS)
def test_geometry_at_constant_affine_state(lam):
    pb = G.problem("band37", changed=True)
    ab = PAR.parity_state(pb.n_frames)
    _, _, lin = G.pose_reference("band37", R.HUBER, changed=True)
    with TA.open_engine(pb, ab) as eng:
        err = TA.check_step("band37 at parity_state", pb, ab, lam, lin, eng)
        assert np.array_equal(eng.get_affine_state(), ab)
    note("d", err)


# e. the loops take the reference's decisions
def test_solve_matches_reference_lm():
    pb = G.problem("band37")
    p_ref, r_ref, c0_ref, c1_ref, it_ref, info = G.lm_reference()
    assert info["successful_steps"] >= 3 and info["unsuccessful_steps"] >= 1
    with plain_engine(pb, G.LM_HUBER) as eng:
        summ = eng.solve(**G.LM_OPTIONS)
        poses, rho = eng.get_state()
        its = eng.solver_iterations()
    print(f"\nsolve: {summ}\nreference: {c0_ref} -> {c1_ref}, {it_ref} iterations, {info['history']}")
    note("e", {"solve final cost": abs(summ["final_cost"] - c1_ref) / c1_ref})
    assert abs(summ["initial_cost"] - c0_ref) <= 1e-5 * c0_ref
    assert abs(summ["final_cost"] - c1_ref) <= 1e-5 * c1_ref, (summ, c1_ref)
    assert summ["iterations"] == it_ref, (summ, it_ref, info)
    assert summ["successful_steps"] == info["successful_steps"], (summ, info)
    assert summ["unsuccessful_steps"] == info["unsuccessful_steps"], (summ, info)
    assert summ["stop_reason"] == info["stop_reason"], (summ, info)
    assert (summ["termination"] == 0) == info["converged"], (summ, info)
    assert its["step_is_successful"][1:].astype(bool).tolist() == [h[1] for h in info["history"]]
    np.testing.assert_allclose(poses[:, 4:], p_ref[:, 4:], atol=1e-5)
    np.testing.assert_allclose(rho, r_ref, rtol=1e-4, atol=1e-6)


def test_solve_affine_matches_reference_lm():
    pb = G.problem("closed100", changed=True)
    ab_ref, c0_ref, c1_ref, it_ref, info = G.lm_ab_reference()
    assert info["successful_steps"] >= 3 and info["unsuccessful_steps"] >= 1
    with TA.open_engine(pb, G.lm_ab_start(pb), huber=G.LM_AB_HUBER, fixed=(), switch=False) as eng:
        eng.set_fixed_affine_frames(np.array(G.LM_AB_FIXED, np.int32))
        summ = eng.solve_affine(**G.LM_AB_OPTIONS)
        its = eng.solver_iterations()
        ab = eng.get_affine_state()
    print(f"\nsolve_affine: {summ}\nreference: {c0_ref} -> {c1_ref}, {it_ref} iterations, {info}")
    note("e", {"solve_affine final cost": abs(summ["final_cost"] - c1_ref) / c1_ref})
    assert abs(summ["initial_cost"] - c0_ref) <= 1e-5 * c0_ref
    assert summ["iterations"] == it_ref and summ["stop_reason"] == info["stop_reason"], (summ, info)
    assert summ["successful_steps"] == info["successful_steps"], (summ, info)
    assert summ["unsuccessful_steps"] == info["unsuccessful_steps"], (summ, info)
    assert its["step_is_successful"][1:].astype(bool).tolist() == info["decisions"][:len(its["cost"]) - 1]
    assert abs(summ["final_cost"] - c1_ref) <= 1e-5 * c1_ref
    assert np.abs(ab - ab_ref).max() <= 1e-3 and np.array_equal(ab[0], G.lm_ab_start(pb)[0])


# f. reproducible at width: two engines, two runs each, bitwise equal (butterflies over more than one 64-lane pass)
def test_brightness_reproducible_at_width():
    pb = G.problem("closed100", changed=True)
    ab = PAR.parity_state(pb.n_frames)
    out = []
    for _ in range(2):
        with TA.open_engine(pb, ab, switch=False) as eng:
            for _ in range(2):
                eng.set_affine_state(ab)
                eng.set_fixed_affine_frames(np.array([0], np.int32))
                c = eng.affine_linearize()
                H, g = eng.affine_system()
                m, st = eng.affine_step(1e-2)
                assert st == 0
                d = eng.affine_last_step()
                eng.solve_affine(max_iterations=3)
                out.append((np.array([c, m]), H, g, d, eng.get_affine_state()))
    assert out[0][1].any() and out[0][3].any() and not np.array_equal(out[0][4], ab)
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


def test_pose_solve_reproducible_at_width():
    pb = G.problem("closed100", changed=True)
    ab = PAR.parity_state(pb.n_frames)
    out = []
    for _ in range(2):
        with TA.open_engine(pb, ab) as eng:
            for _ in range(2):
                eng.set_state(pb.poses, pb.rho)
                c, m, S, g, dp, dr = TA.engine_step(eng, 1e-3)
                eng.solve(max_iterations=3, initial_trust_region_radius=1.0)
                out.append((np.array([c, m]), S, g, dp, dr, *eng.get_state()))
    assert out[0][1].any() and out[0][3].any() and not np.array_equal(out[0][5], pb.poses)
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


# g. free intrinsics: the border lists ("host or target") on a two-way graph
def test_free_intrinsics_geometric_two_way():
    import test_gpu_gn as TG
    pb = G.problem("band37", kind=synth.GEOMETRIC, cams=2)
    state = G.intrinsics_state(pb)
    lin = GR.linearize_intrinsics(pb, pb.poses, pb.rho, state, 1.0, FIXED)
    note("g", TG._check_free_intrinsics_step("band37 two cameras, geometric", pb, state, 1e-1, lin))


def test_free_intrinsics_photometric_two_way():
    import gn_photometric_intrinsics_reference as RI
    import test_gpu_gn_photometric_intrinsics as TI
    pb = G.problem("band37", cams=2)
    K = RI.state(pb)
    lin = RI.linearize(pb, pb.poses, pb.rho, K, RI.HUBER, FIXED)
    with TI.open_engine(pb, K) as eng:
        err, _, (dp, dr), c_cand = TI.check_step("band37 two cameras, photometric", pb, K, 1e-1, lin, eng)
        k_new = eng.get_intrinsics()
    c_ref, _ = RI.cost_at(pb, synth.se3_plus(pb.poses, dp), pb.rho + dr, k_new, RI.HUBER)
    err["candidate"] = abs(c_cand - c_ref) / c_ref
    note("g", err)
    assert err["candidate"] <= 1e-5
