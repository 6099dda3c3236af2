"""CPU checks of tests/gn_joint_intrinsics_reference.py and of the inputs the GPU tests
(tests/test_gpu_gn_joint_intrinsics.py) take from it: the reference's gradient against central differences of its own
cost, its agreement with gn_joint_reference when the cameras' columns are dropped, the conditions under which the GPU
bounds mean something for every problem those tests use, and the two LM runs as literals."""
import numpy as np
import pytest

import gn_joint_intrinsics_reference as R
import gn_joint_reference as GJ
from helpers import synth

FIXED, FIXED_AB, HUBER = R.FIXED, R.FIXED_AB, R.HUBER


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items()) or "base"


def test_gradient_matches_central_differences():
    """g·d of linearize against central differences of the reference's own cost (bicubic interpolation, Huber off) along
    three random directions over poses, ρ, (a, b) and all 8 intrinsics (KB4).  Bound 1e-5, gn_joint_reference's
    (tests/test_gn_joint_reference.py): the central difference's own error h²·(third derivative / first) with h = 1e-4
    of steps of 1e-3 (poses), 1e-2 (ρ), 1e-2 and 1 ((a, b)) and, for the intrinsics, 1e-1 px on fx, fy, cx, cy and
    1e-3 on the distortion — image displacements of the size the pose steps cause."""
    pb = R.problem(synth.KB4, 1)
    ab, K = R.state(pb), R.k_state(pb)
    nf, nc = pb.n_frames, K.shape[0]
    _, g, _ = R.linearize(pb, K, ab, pb.poses, pb.rho, 0.0)
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(3):
        dk = np.concatenate([1e-3 * rng.normal(size=(nf, 6)), rng.normal(size=(nf, 2)) * np.array([1e-2, 1.0])], 1)
        dc = rng.normal(size=(nc, 8)) * np.array([1e-1] * 4 + [1e-3] * 4)
        dl = 1e-2 * rng.normal(size=pb.n_points)
        d = np.concatenate([dk.ravel(), dc.ravel(), dl])
        h = 1e-4

        def cost(s):
            poses, rho, ab_s, K_s = R.apply_step(pb.poses, pb.rho, ab, K, s * dk, s * dc, s * dl)
            c, nv = R.cost_at(pb, K_s, ab_s, poses, rho, 0.0)
            assert nv == pb.n_blocks
            return c

        fd = (cost(h) - cost(-h)) / (2 * h)
        err = abs(float(g @ d) - fd) / abs(fd)
        print(f"g·d {float(g @ d):.9g} finite difference {fd:.9g} relative disagreement {err:.2e}")
        worst = max(worst, err)
    assert worst <= 1e-5


@pytest.mark.parametrize("kw", [dict(), dict(model=synth.KB4, cams=2, P=12)], ids=case_id)
def test_without_the_camera_columns_it_is_the_joint_reference(kw):
    """At the cameras' intrinsics, with the cameras' rows and columns dropped, H, g and the cost are
    gn_joint_reference.linearize's (the same records from another composition: 1e-12 of the largest entry)."""
    pb = R.problem(**kw)
    ab = R.state(pb)
    nf, nc = pb.n_frames, pb.intrinsics.shape[0]
    H, g, c = R.linearize(pb, pb.intrinsics, ab, pb.poses, pb.rho, HUBER)
    H0, g0, c0 = GJ.linearize(pb, ab, pb.poses, pb.rho, HUBER)
    keep = np.r_[0:8 * nf, 8 * (nf + nc):H.shape[0]]
    assert abs(c - c0) <= 1e-12 * c0
    assert np.abs(H[np.ix_(keep, keep)] - H0).max() <= 1e-12 * np.abs(H0).max()
    assert np.abs(g[keep] - g0).max() <= 1e-12 * np.abs(g0).max()
    assert H[8 * nf:8 * (nf + nc)].any()


def _step_parts(pb, dk, dc, dl):
    used = R.N_USED[pb.model]
    return {"pose": dk[:, :6], "a": dk[:, 6], "b": dk[:, 7], "intr": dc[:, :used], "drho": dl}


def _conditions(label, pb, K, ab, lin, huber, intr_scale=1.0):
    """The damped reduced system is well inside what a Cholesky factorisation in fp64 resolves — the smallest eigenvalue
    of the Jacobi-scaled system at λ = 1e-4 is ≥ 1e-4 — and the step moves by ≤ 1e-5 of each part's largest entry when
    the records are rounded to fp32, a hundredth of the GPU step bound: that bound then tests the kernels."""
    nf, nc = pb.n_frames, K.shape[0]
    H, g = lin[:2]
    H2, g2, _ = R.linearize(pb, K, ab, pb.poses, pb.rho, huber, fp32=True, intr_scale=intr_scale)
    for lam in (1e-4, 1e-1):
        S, gS, dk, dc, dl, m, fx = R.schur_step(H, g, ab, nf, nc, lam, FIXED, FIXED_AB)
        d = 1.0 / np.sqrt(np.diag(S))
        ev = np.linalg.eigvalsh(S * d[:, None] * d[None, :])
        ev_raw = np.linalg.eigvalsh(S)
        _, _, dk2, dc2, dl2, m2, _ = R.schur_step(H2, g2, ab, nf, nc, lam, FIXED, FIXED_AB)
        p1, p2 = _step_parts(pb, dk, dc, dl), _step_parts(pb, dk2, dc2, dl2)
        shift = {k: float(np.abs(p2[k] - p1[k]).max() / np.abs(p1[k]).max()) for k in p1}
        shift["model"] = abs(m2 - m) / m
        print(f"{label} λ={lam}: Jacobi-scaled eigenvalues {ev[0]:.3g} … {ev[-1]:.3g} (unscaled {ev_raw[0]:.3g} … "
              f"{ev_raw[-1]:.3g}); fp32 shift " + " ".join(f"{k} {v:.2e}" for k, v in shift.items()))
        assert m > 0
        if lam == 1e-4:
            assert ev[0] >= 1e-4
        assert max(shift.values()) <= 1e-5
        # a parameter the model does not use: its pivot is Ceres' clamp, exactly, and it does not move
        iu = R.parts(nf, nc, pb.model)["unused"]
        iu = iu[~fx[iu]]
        assert np.array_equal(S[iu][:, iu], lam * 1e-6 * np.eye(iu.size)) and not gS[iu].any()
        assert not np.delete(S[iu], iu, axis=1).any() and not dc[:, R.N_USED[pb.model]:].any()


@pytest.mark.parametrize("case", R.CASES, ids=case_id)
def test_gpu_problem_conditions(case):
    """Every system-and-step problem of the GPU tests: all blocks valid (483 of 644 with keyframe 3 turned away), the
    expected constants, the system definite, the fp32 shift small."""
    kw = dict(case)
    huber = kw.pop("huber", HUBER)
    pb = R.problem(**kw)
    lin = R.reference(huber=huber, **kw)
    away = kw.get("turned") or kw.get("unseen")
    assert lin[3] == (483 if away else pb.n_blocks)
    K, ab = R.k_state(pb), R.state(pb)
    nf, nc = pb.n_frames, K.shape[0]
    fx = R.constants(lin[0], ab, nf, nc, FIXED, FIXED_AB)
    fc = fx[8 * nf:].reshape(nc, 8)
    assert fx[:8 * nf].reshape(nf, 8)[3].all() == bool(away)
    assert not fc[0].any() and (nc == 1 or fc[1].all() == bool(kw.get("unseen")))
    if kw.get("unseen"):
        assert tuple(pb.frame_cam) == R.UNSEEN_FRAME_CAM
    _conditions(case_id(case), pb, K, ab, lin, huber)


def test_level_1_problem_conditions():
    """The pyramid-level test's problem: level 1 of the base problem at the level's image of the state, J_intr's first
    four columns halved."""
    import photometric_intrinsics_reference as PIR
    pb = R.problem()
    pb1 = synth.level_problem(pb, 1)
    pb1.interp = 0
    K1, ab = PIR.level_state(R.k_state(pb), 1), R.state(pb)
    nv = []
    lin = R.linearize(pb1, K1, ab, pb.poses, pb.rho, HUBER, nv, intr_scale=0.5)
    assert nv[0] > 0.8 * pb.n_blocks
    _conditions("level 1", pb1, K1, ab, lin, HUBER, intr_scale=0.5)


# the two LM runs: cost before, then every trial's candidate cost
ACCEPTS = [223181.86171, 96409.56790, 20024.70402, 10108.80929, 9181.88381, 9128.52583, 9113.29012, 9109.19265, 9107.84829]
REJECTS = [224835.89738, 76976.70166, 14815.15817, 9414.89431, 9215.50153, 9635.61865, 9572.91295, 9340.22128,
           9005.15061, 8945.34360, 8919.80180]
REJECTS_DECISIONS = [True] * 4 + [False] * 3 + [True] * 3
JOINT_END = 9587.087  # the joint solve at the cameras' intrinsics after 8 trials (tests/test_gpu_gn_joint.py)


@pytest.mark.parametrize("name,costs,decisions", [("accepts", ACCEPTS, [True] * 8), ("rejects", REJECTS, REJECTS_DECISIONS)])
def test_lm_cases(name, costs, decisions):
    """The decisions and costs of the two LM runs, and the same decisions with fp32-rounded records with every cost within
    1e-6 relative.  No relative decrease lies within 0.1 of the threshold; every candidate keeps all blocks valid and
    every ρ positive.  (The intrinsics are only weakly determined by six keyframes: they do not come back to the
    cameras' values, and nothing here claims they do.)"""
    pb = R.problem(cams=R.LM_CASES[name]["cams"])
    *_, c0, c1, it, info = R.lm_reference(name)
    print(name, "relative decreases", np.round(info["rel"], 3), "costs", c0, info["trial_costs"])
    assert it == len(decisions) and info["decisions"] == decisions and info["stop_reason"] == "max_iterations"
    got = np.array([c0] + info["trial_costs"])
    assert np.abs(got - np.array(costs)).max() <= 1e-4
    assert np.abs(np.array(info["rel"]) - 1e-3).min() >= 0.1
    assert info["invalid_candidates"] == 0 and info["valid"] == [pb.n_blocks] * len(decisions)
    assert min(info["min_rho"]) > 0.07
    accepted = [c for c, d in zip(info["trial_costs"], decisions) if d]
    assert c1 == accepted[-1]
    if name == "accepts":
        assert c1 < JOINT_END
    *_, c0f, c1f, itf, infof = R.lm_reference(name, fp32=True)
    gotf = np.array([c0f] + infof["trial_costs"])
    print(name, "fp32 records: worst relative cost difference", float((np.abs(gotf - got) / got).max()))
    assert itf == it and infof["decisions"] == decisions
    assert (np.abs(gotf - got) / got).max() <= 1e-6
