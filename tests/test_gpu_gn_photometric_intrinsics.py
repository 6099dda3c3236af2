"""Photometric free intrinsics in the on-device Gauss-Newton: pba_set_optimize_intrinsics + pba_gn_set_solve_intrinsics.

The reduced camera system over the keyframes and every camera's 8 intrinsics (the border of the skyline system, formed
from the blocks' moment records — intr_rows_photometric_kernel), its step, the candidate, the accept, the LM loop and the
pyramid, against the dense fp64 reference of tests/gn_photometric_intrinsics_reference.py (compose's records, every
product in fp64).  The problems and their references come from that module; tests/test_gn_photometric_intrinsics_
reference.py asserts on the CPU that they meet the input conditions under which the bounds here mean something.

Base problem: 6 keyframes, 161 points, 376×240, 644 blocks (132 past a multiple of 256); state PIR.perturbed_state;
keyframes 0 and 1 fixed; Huber 9.0.  Bounds (the project's for photometric Gauss-Newton, tests/test_gpu_gn.py): cost 1e-5
relative; the pose–pose, pose–intrinsics and intrinsics–intrinsics parts of S each within 1e-4 of that part's largest
reference entry; g within 1e-4 of its scale; pose + intrinsics step, δρ and model decrease within 1e-3; the pads are
identity·(1 + λ) with zero gradient.

Measured (MI355X), worst over the cases: cost 2.3e-8, S parts 2.2e-7, g 6.4e-8, step 5.4e-6, δρ 1.4e-6,
model decrease 1.9e-8, candidate cost 2.6e-8; split against fused border 2.2e-13.
"""
import numpy as np
import pytest

import gn_photometric_intrinsics_reference as R
import gn_reference as GR
import photometric_intrinsics_reference as PIR
from helpers import engine_module, synth

pytestmark = pytest.mark.gpu
E = engine_module()
INVALID_ARGUMENT = "invalid argument"
FIXED, HUBER = R.FIXED, R.HUBER


def open_engine(pb, K, huber=HUBER, fixed=FIXED, library=None, opt_in=True):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber, library=library)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array(fixed, np.int32))
    eng.set_state(pb.poses, pb.rho)
    eng.set_optimize_intrinsics(True)
    eng.set_intrinsics_state(K)
    if opt_in:
        eng.gn_set_solve_intrinsics(True)
    return eng


def engine_step(eng, lam):
    """One host-driven step: (cost, model decrease, S, g, pose step, δρ)."""
    c = eng.gn_linearize()
    m, st = eng.gn_step(lam)
    assert st == 0
    S, g = eng.gn_reduced_system()
    dp, dr = eng.gn_last_step()
    return c, m, S, g, dp, dr


def check_step(label, pb, K, lam, lin, eng, idle_cams=()):
    """The engine's system and step at λ against the reference linearisation `lin` = (H, g, cost); accepts the step and
    returns (errors, reference (δposes, δK, δρ), engine (δposes, δρ), candidate cost).  K is the level-0 state; the
    accepted intrinsics are compared as level-0 values.  idle_cams: cameras that no block observes — constant, so
    their pads are plain identity rows like the rest of their rows."""
    nf, nc = pb.n_frames, pb.intrinsics.shape[0]
    H, g_ref, c_ref = lin
    S_ref, gS_ref, df_ref, dp_ref, dk_ref, dl_ref, m_ref = R.step(H, g_ref, pb, lam, FIXED)
    c, m, S, gs, dp, dr = engine_step(eng, lam)
    assert eng.gn_system_size() == 6 * nf + 12 * nc
    c_cand = eng.gn_candidate_cost()
    eng.gn_accept()
    k_new = eng.get_intrinsics()
    idx = GR.intrinsics_system_index(nf, nc)
    Ss, gss = S[np.ix_(idx, idx)], gs[idx]
    n6 = 6 * nf

    def part(a, b):
        return np.abs(a - b).max() / np.abs(b).max()

    err = {"cost": abs(c - c_ref) / c_ref,
           "S_pp": part(Ss[:n6, :n6], S_ref[:n6, :n6]),
           "S_pk": part(Ss[n6:, :n6], S_ref[n6:, :n6]),
           "S_kk": part(Ss[n6:, n6:], S_ref[n6:, n6:]),
           "g": part(gss, gS_ref),
           "step": np.linalg.norm(np.concatenate([dp.ravel(), (k_new - K).ravel()]) - df_ref) / np.linalg.norm(df_ref),
           "drho": np.linalg.norm(dr - dl_ref) / np.linalg.norm(dl_ref),
           "model": abs(m - m_ref) / abs(m_ref)}
    print(f"\n{label} λ={lam}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    pad = np.concatenate([n6 + 12 * c_ + np.arange(8, 12) for c_ in range(nc)])
    pad_diag = np.concatenate([np.full(4, 1.0 if c_ in idle_cams else 1 + lam) for c_ in range(nc)])
    assert np.allclose(S[np.ix_(pad, pad)], np.diag(pad_diag)) and not gs[pad].any()
    assert err["cost"] <= 1e-5, err
    assert err["S_pp"] <= 1e-4 and err["S_pk"] <= 1e-4 and err["S_kk"] <= 1e-4 and err["g"] <= 1e-4, err
    assert err["step"] <= 1e-3 and err["drho"] <= 1e-3 and err["model"] <= 1e-3, err
    return err, (dp_ref, dk_ref, dl_ref), (dp, dr), c_cand


# 1. reduced system and step, every camera model × both interpolators; candidate cost; accept
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("model", [synth.PINHOLE, synth.DOUBLE_SPHERE, synth.EUCM, synth.KB4])
def test_reduced_system_and_step(model, interp, lam):
    pb = R.problem(model, interp)
    K = R.state(pb)
    _, _, lin, _ = R.reference(model, interp)
    with open_engine(pb, K) as eng:
        _, (dp_ref, dk_ref, dl_ref), (dp, dr), c_cand = check_step(f"model {model} interp {interp}", pb, K, lam, lin, eng)
        k_new = eng.get_intrinsics()
    # the candidate cost at (poses ⊞ δ, ρ + δρ, K + δk) of the ENGINE's step, against compose there
    c_ref, _ = R.cost_at(pb, synth.se3_plus(pb.poses, dp), pb.rho + dr, k_new, HUBER)
    print(f"candidate cost {abs(c_cand - c_ref) / c_ref:.2e}")
    assert abs(c_cand - c_ref) <= 1e-5 * c_ref
    # the accepted intrinsics: the state plus the step the reference predicts, within the step bound
    scale = np.linalg.norm(np.concatenate([dp_ref.ravel(), dk_ref.ravel()]))
    assert np.linalg.norm(k_new - (K + dk_ref)) <= 1e-3 * scale


# 2. pattern sizes
@pytest.mark.parametrize("P", [1, 8, 21, 32])
def test_pattern_sizes(P):
    pb = R.problem(P=P)
    K = R.state(pb)
    _, _, lin, _ = R.reference(P=P)
    with open_engine(pb, K) as eng:
        check_step(f"P {P}", pb, K, 1e-3, lin, eng)


# 3. two cameras; and a camera that nothing observes
@pytest.mark.parametrize("cams", ["two", "idle"])
def test_two_cameras(cams):
    pb = R.problem(cams=cams)
    K = R.state(pb)
    _, _, lin, _ = R.reference(cams=cams)
    nf = pb.n_frames
    with open_engine(pb, K) as eng:
        check_step(f"cameras {cams}", pb, K, 1e-3, lin, eng, idle_cams=(1,) if cams == "idle" else ())
        k_new = eng.get_intrinsics()
        eng.gn_linearize()
        eng.gn_step(1e-3)
        S, g = eng.gn_reduced_system()
    if cams == "idle":  # camera 1: identity rows and columns, zero gradient, intrinsics unchanged
        rows = 6 * nf + 12 + np.arange(12)
        assert np.array_equal(S[rows][:, rows], np.eye(12)) and not g[rows].any()
        off = np.delete(np.arange(S.shape[0]), rows)
        assert not S[np.ix_(rows, off)].any() and not S[np.ix_(off, rows)].any()
        assert np.array_equal(k_new[1], K[1])
    else:
        assert (np.abs(k_new[:, :4] - K[:, :4]) > 0).all()  # both cameras' intrinsics moved


# 4. a keyframe turned away: (nearly all of) its blocks are invalid
def test_turned_keyframe():
    """Keyframe 3 turned 120° about its y axis: 23 % of the blocks are invalid in the reference, all of them blocks that
    target it (tests/test_gn_photometric_intrinsics_reference.py); the producer's zero records are where the
    linearisation's invalid blocks are, so the system matches."""
    pb = R.problem(turned=True)
    K = R.state(pb)
    _, valid, lin, _ = R.reference(turned=True)
    assert 0.05 <= 1.0 - valid.mean() <= 0.40
    with open_engine(pb, K) as eng:
        check_step("turned keyframe", pb, K, 1e-3, lin, eng)


# 5. Huber off and on
@pytest.mark.parametrize("huber", [0.0, 9.0])
def test_huber(huber):
    pb = R.problem()
    K = R.state(pb)
    _, valid, lin, w = R.reference(huber=huber)
    if huber > 0:
        assert (w[valid == 1] < 1.0).mean() >= 0.05
    with open_engine(pb, K, huber=huber) as eng:
        check_step(f"huber {huber}", pb, K, 1e-3, lin, eng)


# 6. a point of 70 blocks; waves past the end of the block list
def test_point_of_seventy_blocks():
    pb = R.long_point_problem()
    assert pb.n_frames >= 71 and np.bincount(pb.block_point).max() == 70
    assert 1 <= pb.n_blocks % 256 <= 192
    K = R.state(pb)
    lin = R.linearize(pb, pb.poses, pb.rho, K, HUBER, FIXED)
    with open_engine(pb, K) as eng:
        check_step("70-block point", pb, K, 1e-3, lin, eng)


# 7. split and fused border
def test_split_and_fused_border_agree(monkeypatch):
    pb = R.problem(cams="two")
    K = R.state(pb)
    out = {}
    for branch in ("fused", "split"):
        monkeypatch.setenv("PBA_TEST_BORDER", branch)
        with open_engine(pb, K, library=E.TEST_LIB_PATH) as eng:
            _, m, _, _, dp, dr = engine_step(eng, 1e-3)
            eng.gn_accept()
            out[branch] = (dp, dr, eng.get_intrinsics() - K, np.array([m]))
    for name, x, y in zip(("poses", "rho", "intrinsics", "model"), out["split"], out["fused"]):
        err = np.linalg.norm(x - y) / np.linalg.norm(y)
        print(f"\nborder split vs fused: {name} {err:.2e}")
        assert err <= 1e-12, (name, err)


# 8. pyramid
def test_pyramid_level_one_step():
    pb = R.problem()
    K = R.state(pb)
    with open_engine(pb, K) as eng:
        eng.build_pyramid(2)
        eng.set_level(1)
        pb1 = synth.level_problem(pb, 1, host_intensity=eng.host_intensities())
        lin = R.linearize(pb1, pb.poses, pb.rho, PIR.level_state(K, 1), HUBER, FIXED, intr_scale=0.5)
        # (pb1's cameras are level 1's; the step δk is the level-0 state's, so the accepted state is compared at level 0)
        check_step("level 1", pb1, K, 1e-3, lin, eng)


def test_pyramid_accept_returns_level_zero_values():
    pb = R.problem()
    K = R.state(pb)
    with open_engine(pb, K) as eng:
        eng.build_pyramid(2)
        eng.set_level(1)
        eng.gn_linearize()
        eng.gn_step(1e-3)
        eng.gn_accept()
        k1 = eng.get_intrinsics()
        poses, rho = eng.get_state()
        assert np.abs(k1[:, :2] - K[:, :2]).max() < 5.0 and np.abs(k1 - K).max() > 0  # level-0 focal lengths, moved
        eng.set_level(0)
        assert np.array_equal(eng.get_intrinsics(), k1)
        c0 = eng.gn_linearize()
    c_ref, _ = R.cost_at(pb, poses, rho, k1, HUBER)
    assert abs(c0 - c_ref) <= 1e-5 * c_ref


def test_solve_pyramid_carries_the_intrinsics():
    pb = R.problem()
    K = R.state(pb)
    c_init, _ = R.cost_at(pb, pb.poses, pb.rho, K, HUBER)
    with open_engine(pb, K) as eng:
        eng.build_pyramid(2)
        summ = eng.solve_pyramid(max_iterations=6)
        poses, rho = eng.get_state()
        k = eng.get_intrinsics()
        assert eng.level()[0] == 0
    c_final, _ = R.cost_at(pb, poses, rho, k, HUBER)
    print(f"\nsolve_pyramid: initial {c_init:.6g} final {c_final:.6g} (summary {summ['final_cost']:.6g}) δK {k - K}")
    assert abs(summ["final_cost"] - c_final) <= 1e-5 * c_final
    assert c_final <= c_init and np.abs(k - K).max() > 0


# 9. LM decisions
def test_lm_matches_reference_lm():
    pb, K, kw = R.lm_case()
    p_ref, r_ref, k_ref, c0_ref, c1_ref, it_ref, info = R.lm_reference()
    with open_engine(pb, K) as eng:
        summ = eng.solve(**kw)
        poses, rho = eng.get_state()
        k = eng.get_intrinsics()
        its = eng.solver_iterations()
    # _same_lm (tests/test_gpu_gn.py)
    assert abs(summ["initial_cost"] - c0_ref) <= 1e-5 * c0_ref
    assert abs(summ["final_cost"] - c1_ref) <= 1e-3 * c1_ref + 1e-6, (summ, c1_ref)
    assert summ["iterations"] == it_ref, (summ, it_ref, info)
    assert summ["successful_steps"] == info["successful_steps"], (summ, info)
    assert summ["unsuccessful_steps"] == info["unsuccessful_steps"], (summ, info)
    assert summ["stop_reason"] == info["stop_reason"], (summ, info)
    assert (summ["termination"] == 0) == info["converged"], (summ, info)
    np.testing.assert_allclose(poses[:, 4:], p_ref[:, 4:], atol=1e-5)
    np.testing.assert_allclose(rho, r_ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(k, k_ref, rtol=1e-5, atol=1e-12)
    # the trajectory is consistent with the summary
    assert its["cost"][0] == pytest.approx(summ["initial_cost"], rel=1e-12)
    assert its["cost"][-1] == pytest.approx(summ["final_cost"], rel=1e-12)
    assert int(its["step_is_successful"][1:].sum()) == summ["successful_steps"]


# 10. recovery of a perturbed calibration
def test_recovery():
    pb, K0 = R.recovery_problem()
    c_gt, _ = R.cost_at(pb, pb.poses_gt, pb.rho_gt, pb.intrinsics, HUBER)
    with open_engine(pb, K0) as eng:
        eng.solve(max_iterations=20)
        poses, rho = eng.get_state()
        k = eng.get_intrinsics()
    c_final, _ = R.cost_at(pb, poses, rho, k, HUBER)
    e0, e1 = np.abs(K0[0, :2] - pb.intrinsics[0, :2]), np.abs(k[0, :2] - pb.intrinsics[0, :2])
    print(f"\nrecovery: cost {c_final:.6g} against {c_gt:.6g} at ground truth; |fx, fy error| {e0} -> {e1}")
    assert c_final <= 1.05 * c_gt
    assert (e1 < e0).all()


# 11. reproducibility
def test_solve_is_reproducible():
    pb = R.problem(cams="two")
    K = R.state(pb)
    out = []
    for _ in range(2):
        with open_engine(pb, K) as eng:
            eng.solve(max_iterations=4)
            out.append((*eng.get_state(), eng.get_intrinsics()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# 12. opt-in and refusals
def test_opt_in_and_refusals():
    import torch
    pb = R.problem()
    K = R.state(pb)
    with open_engine(pb, K, opt_in=False) as eng:
        x = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
        for call in (eng.gn_linearize, lambda: eng.gn_step(1e-3), eng.gn_candidate_cost, eng.gn_accept,
                     lambda: eng.solve(max_iterations=2), lambda: eng.solve_pyramid(max_iterations=2),
                     eng.gn_system_size, eng.gn_reduced_system):
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                call()
        eng.gn_set_solve_intrinsics(True)
        assert eng.gn_linearize() > 0.0
        # the multi-GPU entry points still refuse, with the same message
        for call in (lambda: eng.gn_step_export(1e-3, 4, x.data_ptr()), lambda: eng.gn_step_import(1e-3, 4, x.data_ptr()),
                     lambda: eng.solve_distributed(4, x.data_ptr(), lambda p, n: None, max_iterations=2)):
            with pytest.raises(E.PbaError, match="free intrinsics on a photometric engine"):
                call()
        # the half formats stay refused with free intrinsics
        for fmt in (E.RECORD_F16, E.RECORD_F16_SCALED):
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.set_record_format(fmt)
        eng.gn_set_solve_intrinsics(False)
        with pytest.raises(E.PbaError, match="free intrinsics on a photometric engine"):
            eng.gn_linearize()
    # enabling it without set_optimize_intrinsics is legal and changes nothing until that is set
    with E.Engine(pb.kind, pb.model, huber_width=HUBER) as eng:
        eng.set_problem(pb)
        eng.set_fixed_frames(np.array(FIXED, np.int32))
        eng.set_state(pb.poses, pb.rho)
        eng.gn_set_solve_intrinsics(True)
        eng.gn_linearize()
        eng.gn_step(1e-3)
        assert eng.gn_system_size() == 6 * pb.n_frames
    # a geometric engine: OK, and its step is bit-identical with and without the call
    pg = synth.make_problem(kind=1, n_frames=10, n_points=120, width=376, height=240, seed=13, border=12)
    steps = []
    for on in (False, True):
        with E.Engine(pg.kind, pg.model, huber_width=1.0) as eng:
            eng.set_problem(pg)
            eng.set_fixed_frames(np.array(FIXED, np.int32))
            eng.set_state(pg.poses, pg.rho)
            eng.set_optimize_intrinsics(True)
            eng.set_intrinsics_state(pg.intrinsics * np.array([1.003, 0.998, 1.0005, 0.9995, 1, 1, 1, 1]))
            if on:
                eng.gn_set_solve_intrinsics(True)
            eng.gn_linearize()
            eng.gn_step(1e-3)
            dp, dr = eng.gn_last_step()
            eng.gn_accept()
            steps.append((dp, dr, eng.get_intrinsics()))
    for a, b in zip(*steps):
        assert np.array_equal(a, b)
