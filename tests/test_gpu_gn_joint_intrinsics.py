"""The joint solve with free intrinsics on the device: pba_joint_* and pba_solve_joint under
pba_joint_set_solve_intrinsics (engine.joint_set_solve_intrinsics), photometric engines with both
pba_set_optimize_intrinsics and pba_set_affine_brightness — poses, inverse distances, (a, b) and the cameras'
intrinsics in one solve.

Reference: tests/gn_joint_intrinsics_reference.py (dense fp64 over photometric_affine_intrinsics_reference.compose's
26·P records; tests/test_gn_joint_intrinsics_reference.py asserts on the CPU the input conditions under which the bounds
here mean something).

Problems: gn_affine_reference.problem(...) at state(pb) (a ∈ ±0.3, b ∈ ±20) and the intrinsics state k_state(pb), poses
of keyframes 0 and 1 constant, (a, b) of keyframe 0 constant; 644 blocks: 20 workgroups of 32 and 4 more.

Bounds (the joint solve's, tests/test_gpu_gn_joint.py): cost 1e-5 relative; S and g within 1e-4 of the largest reference
entry of each part — S over pose×pose, pose×(a, b), (a, b)×(a, b), intr×pose, intr×(a, b), intr×intr, g over pose, a,
b, intr; the step within 1e-3 of the largest reference entry of each part (pose, a, b, intr over the parameters the
model uses, δρ); model decrease 1e-3; candidate cost 1e-5.  Every test prints what it measured; DESIGN.md §25 holds
the worst values.

Measured (MI355X), worst over the cases: cost 4.8e-8; S 3.2e-7 / 9.0e-7 / 5.1e-7 (keyframes), 4.8e-7 / 1.3e-6 / 1.8e-7
(intr×pose, intr×(a, b), intr×intr); g 4.3e-7 / 1.4e-7 / 1.5e-7 / 5.2e-6; step pose 5.0e-7, a 3.9e-6, b 3.9e-7, intr
2.0e-5 (double sphere at λ = 1e-4, where rounding the records to fp32 alone moves it by 7.6e-6), δρ 5.8e-7; model
decrease 4.8e-8; candidate cost 4.3e-7.  At the cameras' intrinsics against the plain joint solve: the cost bit for bit,
S within 3.8e-8, g within 3.8e-9.  solve_joint: the reference's decisions in both runs, every trial cost within 1.2e-6.
"""
import ctypes as C

import numpy as np
import pytest

import gn_joint_intrinsics_reference as R
import gn_joint_reference as GJ
import photometric_intrinsics_reference as PIR
from helpers import engine_module, synth

pytestmark = pytest.mark.gpu
E = engine_module()
INVALID_ARGUMENT = "invalid argument"
NOT_READY = "not ready"
FIXED, FIXED_AB, HUBER = R.FIXED, R.FIXED_AB, R.HUBER


def open_engine(pb, K=None, ab=None, huber=HUBER, fixed=FIXED, fixed_ab=FIXED_AB, switch=True):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array(fixed, np.int32))
    eng.set_state(pb.poses, pb.rho)
    eng.set_intrinsics_with_affine(True)
    eng.set_optimize_intrinsics(True)
    eng.set_affine_brightness(True)
    if K is not None:
        eng.set_intrinsics_state(K)
    if ab is not None:
        eng.set_affine_state(ab)
    eng.set_fixed_affine_frames(np.array(fixed_ab, np.int32))
    if switch:
        eng.joint_set_solve_intrinsics(True)
    return eng


def engine_step(eng, lam):
    """One host-driven step: (cost, model decrease, S, g, keyframe step, camera step, δρ)."""
    c = eng.joint_linearize()
    m, st = eng.joint_step(lam)
    assert st == 0
    S, g = eng.joint_get_reduced_system()
    dk, dr = eng.joint_get_step()
    return c, m, S, g, dk, eng.joint_get_intrinsics_step(), dr


def part_err(got, ref):
    """max |got − ref| over the largest |ref| (a part that is zero in the reference must be zero)."""
    top = np.abs(ref).max(initial=0.0)
    if top == 0.0:
        assert not np.any(got)
        return 0.0
    return float(np.abs(got - ref).max() / top)


def check_joint(label, pb, K, ab, lam, lin, eng, huber=HUBER, level=0):
    """The engine's system and step at λ against the reference linearisation `lin` = (H, g, cost[, …]) of `pb` (the
    active level's problem) ; the candidate cost against the reference cost at the ENGINE's candidate.  K: the level-0
    intrinsics state."""
    H, g_ref, c_ref = lin[:3]
    nf, nc = pb.n_frames, K.shape[0]
    S_ref, gS_ref, dk_ref, dc_ref, dl_ref, m_ref, fx = R.schur_step(H, g_ref, ab, nf, nc, lam, FIXED, FIXED_AB)
    c, m, S, gs, dk, dc, dr = engine_step(eng, lam)
    assert eng.joint_system_size() == 8 * (nf + nc) == S.shape[0] == gs.shape[0]
    c_cand = eng.joint_candidate_cost()
    poses_c, rho_c, ab_c, K_c = R.apply_step(pb.poses, pb.rho, ab, K, dk, dc, dr)
    cc_ref, _ = R.candidate_cost(pb, PIR.level_state(K_c, level), ab_c, poses_c, rho_c, huber)
    ix = R.parts(nf, nc, pb.model)
    ip, ii, iu = ix["pose"], ix["intr"], ix["unused"]
    iab = np.sort(np.concatenate([ix["a"], ix["b"]]))
    used = R.N_USED[pb.model]

    def sub(M, r, c_):
        return M[np.ix_(r, c_)]

    err = {"cost": abs(c - c_ref) / c_ref,
           "S_pp": part_err(sub(S, ip, ip), sub(S_ref, ip, ip)), "S_pab": part_err(sub(S, ip, iab), sub(S_ref, ip, iab)),
           "S_abab": part_err(sub(S, iab, iab), sub(S_ref, iab, iab)),
           "S_ip": part_err(sub(S, ii, ip), sub(S_ref, ii, ip)), "S_iab": part_err(sub(S, ii, iab), sub(S_ref, ii, iab)),
           "S_ii": part_err(sub(S, ii, ii), sub(S_ref, ii, ii)),
           "g_pose": part_err(gs[ip], gS_ref[ip]), "g_a": part_err(gs[ix["a"]], gS_ref[ix["a"]]),
           "g_b": part_err(gs[ix["b"]], gS_ref[ix["b"]]), "g_intr": part_err(gs[ii], gS_ref[ii]),
           "step_pose": part_err(dk[:, :6], dk_ref[:, :6]), "step_a": part_err(dk[:, 6], dk_ref[:, 6]),
           "step_b": part_err(dk[:, 7], dk_ref[:, 7]), "step_intr": part_err(dc[:, :used], dc_ref[:, :used]),
           "drho": part_err(dr, dl_ref), "model": abs(m - m_ref) / abs(m_ref), "candidate": abs(c_cand - cc_ref) / cc_ref}
    print(f"\n{label} λ={lam}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()) + f" min ρ+δρ {rho_c.min():.3g}")
    assert np.array_equal(S, S.T)
    assert np.array_equal(S[fx][:, fx], np.eye(int(fx.sum()))) and not S[fx][:, ~fx].any() and not gs[fx].any()
    assert not np.concatenate([dk.ravel(), dc.ravel()])[fx].any()
    # a parameter the model does not use (of a camera with a valid block): exactly Ceres' clamp on the diagonal, zeros
    # elsewhere, a zero gradient and a zero step
    iu = iu[~fx[iu]]
    assert np.array_equal(S[iu][:, iu], lam * 1e-6 * np.eye(iu.size)) and not np.delete(S[iu], iu, axis=1).any()
    assert not gs[iu].any() and not dc[:, used:].any()
    assert err["cost"] <= 1e-5, err
    assert max(err[k] for k in err if k[:2] in ("S_", "g_")) <= 1e-4, err
    assert max(err[k] for k in ("step_pose", "step_a", "step_b", "step_intr", "drho", "model")) <= 1e-3, err
    assert err["candidate"] <= 1e-5, err
    return err, fx


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items()) or "base"


# 1. system and step (the cases: gn_joint_intrinsics_reference.CASES)
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
@pytest.mark.parametrize("case", R.CASES, ids=case_id)
def test_system_and_step(case, lam):
    kw = dict(case)
    huber = kw.pop("huber", HUBER)
    pb = R.problem(**kw)
    K, ab = R.k_state(pb), R.state(pb)
    lin = R.reference(huber=huber, **kw)
    nf, nc = pb.n_frames, K.shape[0]
    with open_engine(pb, K, ab, huber=huber) as eng:
        _, fx = check_joint(case_id(case), pb, K, ab, lam, lin, eng, huber)
        assert np.array_equal(eng.get_affine_state(), ab) and np.array_equal(eng.get_intrinsics(), K)  # a step moves nothing
        fk, fc = fx[:8 * nf].reshape(nf, 8), fx[8 * nf:].reshape(nc, 8)
        assert fk[0].all() and fk[1, :6].all() and not fk[1, 6:].any() and not fk[[2, 4, 5]].any()
        away = bool(kw.get("turned") or kw.get("unseen"))
        assert fk[3].all() == away and not fc[0].any()
        assert lin[3] == (483 if away else pb.n_blocks)
        if kw.get("unseen"):  # camera 1 is keyframe 3's alone: no valid block, identity rows, no step
            assert fc[1].all() and not eng.joint_get_intrinsics_step()[1].any()
        elif nc == 2:
            assert not fc[1].any() and eng.joint_get_intrinsics_step()[1, :4].all()


# 2. pyramid level 1: the level's images, points and image of the intrinsics state; J_intr's columns 0–3 carry ½; after
# joint_accept the level-0 state is the old one plus δk
def test_system_and_step_at_level_1():
    pb = R.problem()
    K, ab = R.k_state(pb), R.state(pb)
    with open_engine(pb, K, ab) as eng:
        eng.build_pyramid(2)
        eng.set_level(1)
        pb1 = synth.level_problem(pb, 1, host_intensity=eng.host_intensities())
        pb1.interp = 0
        nv = []
        lin = R.linearize(pb1, PIR.level_state(K, 1), ab, pb.poses, pb.rho, HUBER, nv, intr_scale=0.5)
        assert nv[0] > 0.8 * pb.n_blocks
        check_joint("level 1", pb1, K, ab, 1e-3, lin, eng, level=1)
        dc = eng.joint_get_intrinsics_step()
        assert np.array_equal(eng.get_intrinsics(), K)
        eng.joint_accept()
        err = np.abs(eng.get_intrinsics() - (K + dc)).max()
        print(f"\nlevel 1 accept: |k − (k₀ + δk)| {err:.2e}, |δk| {np.abs(dc).max():.3g}")
        assert err <= 1e-9 and np.abs(dc[:, :4]).min() > 0
        assert eng.level()[0] == 1


# 3. at the cameras' intrinsics the keyframes' part of S and g and the cost are those of the plain joint solve (an engine
# without free intrinsics) at the same (a, b).  Both are fp64 sums, in the same order, of products of the same fp32 rows;
# the rows come from two instantiations of photometric_row, whose fp32 chains the compiler may contract differently: a
# few 2⁻²⁴ per row entry.  Bound 1e-6 of each part's largest entry; measured: see the print.
@pytest.mark.parametrize("kw", [dict(), dict(P=21, cams=2)], ids=case_id)
def test_at_the_cameras_intrinsics_it_is_the_joint_solve(kw):
    pb = R.problem(**kw)
    ab = R.state(pb)
    nf = pb.n_frames
    lam = 1e-3
    with open_engine(pb, None, ab) as eng:
        assert np.array_equal(eng.get_intrinsics(), pb.intrinsics)
        c, m, S, g, dk, dc, dr = engine_step(eng, lam)
    with E.Engine(pb.kind, pb.model, huber_width=HUBER) as eng:
        eng.set_problem(pb)
        eng.set_fixed_frames(np.array(FIXED, np.int32))
        eng.set_state(pb.poses, pb.rho)
        eng.set_affine_brightness(True)
        eng.set_affine_state(ab)
        eng.set_fixed_affine_frames(np.array(FIXED_AB, np.int32))
        c0 = eng.joint_linearize()
        assert eng.joint_step(lam)[1] == 0
        S0, g0 = eng.joint_get_reduced_system()
    n = 8 * nf
    ix = GJ.parts(nf)
    ip, iab = ix["pose"], np.sort(np.concatenate([ix["a"], ix["b"]]))
    Sk = S[:n, :n]
    err = {"cost": abs(c - c0) / c0, "S_pp": part_err(Sk[np.ix_(ip, ip)], S0[np.ix_(ip, ip)]),
           "S_pab": part_err(Sk[np.ix_(ip, iab)], S0[np.ix_(ip, iab)]),
           "S_abab": part_err(Sk[np.ix_(iab, iab)], S0[np.ix_(iab, iab)]),
           "g_pose": part_err(g[:n][ip], g0[ip]), "g_ab": part_err(g[:n][iab], g0[iab])}
    print(f"\nat the cameras' intrinsics {case_id(kw)}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()) +
          f" bitwise equal: S {np.array_equal(Sk, S0)} cost {c == c0}")
    assert S0.shape == (n, n) and S.shape[0] == n + 8 * pb.intrinsics.shape[0] and S[n:, :n].any()
    assert max(err.values()) <= 1e-6, err


# 4. the candidate: its cost against the reference (check_joint), and against the engine's own evaluation once accepted
@pytest.mark.parametrize("kw", [dict(), dict(model=R.KB4, P=12, interp=1)], ids=case_id)
def test_candidate_cost_is_the_evaluation_cost_after_accept(kw):
    pb = R.problem(**kw)
    K, ab = R.k_state(pb), R.state(pb)
    with open_engine(pb, K, ab) as eng:
        c, m, S, g, dk, dc, dr = engine_step(eng, 1e-3)
        c_cand = eng.joint_candidate_cost()
        poses_c, rho_c, ab_c, K_c = R.apply_step(pb.poses, pb.rho, ab, K, dk, dc, dr)
        cc_ref, nv_ref = R.candidate_cost(pb, K_c, ab_c, poses_c, rho_c, HUBER)
        eng.joint_accept()
        np.testing.assert_allclose(eng.get_intrinsics(), K_c, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(eng.get_affine_state(), ab_c, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(eng.get_state()[0], poses_c, atol=1e-10)
        eng.evaluate(False)
        c_eval, n_valid = eng.cost()
        c_lin = eng.joint_linearize()
    print(f"\ncandidate {case_id(kw)}: candidate cost {c_cand!r} reference {cc_ref!r} evaluate {c_eval!r} "
          f"linearise {c_lin!r}; valid {n_valid} reference {nv_ref}; cost before {c!r}")
    assert n_valid == nv_ref == pb.n_blocks and c_cand < c
    assert abs(c_cand - cc_ref) <= 1e-5 * cc_ref
    assert abs(c_cand - c_eval) <= 1e-6 * c_eval and abs(c_lin - c_eval) <= 1e-6 * c_eval


def same_lm(summ, its, ref):
    """The engine's trajectory against the reference loop's: the decisions, the trial costs and the end."""
    *_, c0, c1, it, info = ref
    print(f"\nsolve_joint: {summ}\ncosts {its['cost']}\nreference: {c0} -> {c1}, {it} iterations, {info}")
    assert abs(summ["initial_cost"] - c0) <= 1e-5 * c0
    assert summ["iterations"] == it and summ["stop_reason"] == info["stop_reason"], (summ, info)
    assert summ["successful_steps"] == info["successful_steps"], (summ, info)
    assert summ["unsuccessful_steps"] == info["unsuccessful_steps"], (summ, info)
    assert (summ["termination"] == 0) == info["converged"], (summ, info)
    assert its["step_is_successful"][1:].astype(bool).tolist() == info["decisions"]
    # every evaluated trial's cost: an accepted entry of the trajectory holds the new cost, a rejected one the
    # candidate's — each within 1e-5 of its own reference value
    trial = np.array(info["trial_costs"])
    rel = np.abs(its["cost"][1:] - trial) / trial
    print("trial cost errors", rel, "relative decreases", its["relative_decrease"][1:], "reference", info["rel"])
    assert rel.max() <= 1e-5, (its["cost"], trial)
    assert abs(summ["final_cost"] - c1) <= 1e-5 * c1, (summ, c1)


def final_state(eng):
    return (*eng.get_state(), eng.get_affine_state(), eng.get_intrinsics())


# 5. solve_joint from (a, b) = 0 and k_state: the reference's decisions and trial costs — eight accepted trials with one
# camera; with two cameras trials 5–7 rejected.  The state bounds are the joint LM test's (poses 1e-5, ρ 1e-4 relative,
# (a, b) 1e-3); the intrinsics are plain parameter blocks like ρ and take its relative bound, 1e-4 of the largest entry.
@pytest.mark.parametrize("name", ["accepts", "rejects"])
def test_solve_joint_matches_reference_lm(name):
    kw = R.LM_CASES[name]
    pb = R.problem(cams=kw["cams"])
    K0 = R.k_state(pb)
    ref = R.lm_reference(name)
    p_ref, r_ref, ab_ref, K_ref = ref[:4]
    with open_engine(pb, K0, None) as eng:
        summ = eng.solve_joint(max_iterations=kw["max_iterations"])
        its = eng.solver_iterations()
        poses, rho, ab, K = final_state(eng)
        c_after = eng.joint_linearize()
    same_lm(summ, its, ref)
    assert abs(c_after - summ["final_cost"]) <= 1e-9 * c_after  # the state is the accepted candidate
    assert np.array_equal(poses[:2], pb.poses[:2]) and np.array_equal(ab[0], np.zeros(2))
    print("final intrinsics", K, "reference", K_ref, "start", K0)
    np.testing.assert_allclose(poses[:, 4:], p_ref[:, 4:], atol=1e-5)
    np.testing.assert_allclose(rho, r_ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ab, ab_ref, atol=1e-3)
    assert np.abs(K - K_ref).max() <= 1e-4 * np.abs(K_ref).max() and np.array_equal(K[:, 4:], K0[:, 4:])
    assert np.abs(K[:, :4] - K0[:, :4]).min() > 0 and np.abs(ab[1:]).min() > 0


# a rejected trial leaves the state — the intrinsics included — bit for bit: with two cameras the run that ends after the
# three rejected trials 5–7 ends where the run of four trials ends
def test_rejected_trials_leave_the_state():
    pb = R.problem(cams=2)
    K0 = R.k_state(pb)
    out = []
    for n in (4, 7):
        with open_engine(pb, K0, None) as eng:
            summ = eng.solve_joint(max_iterations=n)
            out.append((summ, final_state(eng)))
    (s4, st4), (s7, st7) = out
    print(f"\n4 trials: {s4}\n7 trials: {s7}")
    assert (s4["successful_steps"], s4["unsuccessful_steps"]) == (4, 0)
    assert (s7["successful_steps"], s7["unsuccessful_steps"]) == (4, 3)
    assert s7["final_cost"] == s4["final_cost"] and not np.array_equal(st4[3], K0)
    for a, b in zip(st4, st7):
        assert np.array_equal(a, b)


# reproducible: two engines, two runs each — the system, the step, the summaries and the final states bitwise equal
def test_reproducible():
    pb = R.problem(P=12, cams=2)
    K, ab = R.k_state(pb), R.state(pb)
    out = []
    for _ in range(2):
        with open_engine(pb, K, ab) as eng:
            for _ in range(2):
                eng.set_state(pb.poses, pb.rho)
                eng.set_affine_state(ab)
                eng.set_intrinsics_state(K)
                c, m, S, g, dk, dc, dr = engine_step(eng, 1e-3)
                summ = eng.solve_joint(max_iterations=4)
                summary = np.array([c, m, summ["initial_cost"], summ["final_cost"], summ["iterations"],
                                    summ["successful_steps"], summ["gradient_max_norm"]])
                out.append((summary, S, g, dk, dc, dr, *final_state(eng)))
    assert out[0][1].any() and out[0][4].any() and not np.array_equal(out[0][9], K)
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


# 6. switch rules, refusals and staleness, each leaving the engine as it was
def joint_calls(eng):
    return {"joint_linearize": eng.joint_linearize, "joint_system_size": eng.joint_system_size,
            "joint_step": lambda: eng.joint_step(1e-3), "joint_get_reduced_system": eng.joint_get_reduced_system,
            "joint_get_step": eng.joint_get_step, "joint_get_intrinsics_step": eng.joint_get_intrinsics_step,
            "joint_candidate_cost": eng.joint_candidate_cost, "joint_accept": eng.joint_accept,
            "solve_joint": eng.solve_joint}


def refused_calls(eng):
    """The entry points that refuse an engine with both switches on whatever pba_joint_set_solve_intrinsics says."""
    import torch
    ex = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    cb = E.ALLREDUCE_FN(lambda *a: 0)
    eng._keep += [ex, cb]
    L, h = eng._L, eng._h
    X = C.c_void_p(ex.data_ptr())
    return {
        "joint_band": eng.joint_band, "joint_exchange_size": lambda: eng.joint_exchange_size(1),
        "joint_step_export": lambda: eng.joint_step_export(1e-4, 1, ex.data_ptr()),
        "joint_step_import": lambda: eng.joint_step_import(1e-4, 1, ex.data_ptr()),
        "solve_joint_distributed": lambda: eng._ck(L.pba_solve_joint_distributed(h, None, 1, X, cb, None, None), "jd"),
        "gn_linearize": eng.gn_linearize, "gn_step": lambda: eng.gn_step(1e-4), "gn_candidate_cost": eng.gn_candidate_cost,
        "gn_accept": eng.gn_accept, "gn_system_size": eng.gn_system_size, "solve": lambda: eng.solve(max_iterations=2),
        "solve_pyramid": lambda: eng.solve_pyramid(max_iterations=2),
        "affine_linearize": eng.affine_linearize, "affine_step": lambda: eng.affine_step(1e-4),
        "affine_candidate_cost": lambda: eng._ck(L.pba_affine_candidate_cost(h, C.byref(C.c_double())), "acc"),
        "affine_accept": eng.affine_accept, "solve_affine": lambda: eng._ck(L.pba_solve_affine(h, None, None), "sa"),
    }


def test_switch_rules():
    pb = R.problem()
    K, ab = R.k_state(pb), R.state(pb)
    # refused: a geometric engine; one switch alone
    with E.Engine(synth.GEOMETRIC, synth.PINHOLE) as eng:
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.joint_set_solve_intrinsics(True)
        eng.joint_set_solve_intrinsics(False)
    for only in ("intr", "affine"):
        with E.Engine(pb.kind, pb.model, huber_width=HUBER) as eng:
            eng.set_problem(pb)
            eng.set_state(pb.poses, pb.rho)
            eng.set_optimize_intrinsics(True) if only == "intr" else eng.set_affine_brightness(True)
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.joint_set_solve_intrinsics(True)
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.joint_get_intrinsics_step()
            if only == "affine":  # the plain joint solve runs as ever
                assert eng.joint_linearize() > 0 and eng.joint_system_size() == 8 * pb.n_frames
    # both on, without the switch: every joint entry point refuses as before it existed; the two pba_gn_set_solve_*
    # opt-ins make no difference
    with open_engine(pb, K, ab, switch=False) as eng:
        eng.build_pyramid(2)
        for opted in (False, True):
            if opted:
                eng.gn_set_solve_intrinsics(True)
                eng.gn_set_solve_affine(True)
            for name, call in joint_calls(eng).items():
                with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                    call()
        # with it: the full problem runs; what stays refused leaves states, level and records intact
        eng.joint_set_solve_intrinsics(True)
        c = eng.joint_linearize()
        m, st = eng.joint_step(1e-3)
        assert st == 0 and m > 0 and eng.joint_system_size() == 8 * (pb.n_frames + 1)
        eng.evaluate(True)
        rec, valid = eng.records()
        for name, call in refused_calls(eng).items():
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                call()
            print("refused:", name)
        assert eng.level()[0] == 0 and eng.record_floats == 26 * pb.P
        assert np.array_equal(eng.get_intrinsics(), K) and np.array_equal(eng.get_affine_state(), ab)
        poses, rho = eng.get_state()
        assert np.array_equal(poses, pb.poses) and np.array_equal(rho, pb.rho)
        rec2, valid2 = eng.records()
        assert np.array_equal(rec, rec2) and np.array_equal(valid, valid2)
        assert eng.joint_step(1e-3) == (m, st) and eng.joint_linearize() == c
        # turning either switch off clears it: back on, the joint entry points refuse until it is asked for again
        for off, on in ((lambda: eng.set_affine_brightness(False), lambda: eng.set_affine_brightness(True)),
                        (lambda: eng.set_optimize_intrinsics(False), lambda: eng.set_optimize_intrinsics(True))):
            off()
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.joint_set_solve_intrinsics(True)
            on()
            for name, call in joint_calls(eng).items():
                with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                    call()
            eng.joint_set_solve_intrinsics(True)
            eng.set_intrinsics_state(K)
            eng.set_affine_state(ab)
            assert abs(eng.joint_linearize() - c) <= 1e-12 * c


def test_staleness():
    pb = R.problem()
    K, ab = R.k_state(pb), R.state(pb)

    def stale(eng):
        for call in (lambda: eng.joint_step(1e-3), eng.joint_candidate_cost, eng.joint_accept, eng.joint_get_step,
                     eng.joint_get_intrinsics_step, eng.joint_get_reduced_system):
            with pytest.raises(E.PbaError, match=NOT_READY):
                call()

    with open_engine(pb, K, ab) as eng:
        eng.build_pyramid(2)
        stale(eng)  # a call before the one it follows
        c0 = eng.joint_linearize()
        for call in (eng.joint_get_reduced_system, eng.joint_get_step, eng.joint_get_intrinsics_step,
                     eng.joint_candidate_cost, eng.joint_accept):
            with pytest.raises(E.PbaError, match=NOT_READY):  # the linearisation stands, but there is no step yet
                call()

        def fresh():
            c = eng.joint_linearize()
            assert eng.joint_step(1e-3)[1] == 0
            return c

        fresh()
        for change in (lambda: eng.set_intrinsics_state(K), lambda: eng.set_state(pb.poses, pb.rho),
                       lambda: eng.set_affine_state(ab), lambda: eng.set_level(1), lambda: eng.set_level(0),
                       eng.joint_accept):
            change()
            stale(eng)
            fresh()
        eng.set_state(pb.poses, pb.rho)
        eng.set_affine_state(ab)
        eng.set_intrinsics_state(K)
        assert fresh() == c0  # back at the first state, the first linearisation
