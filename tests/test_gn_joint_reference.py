"""CPU checks of tests/gn_joint_reference.py and of the inputs the GPU tests (tests/test_gpu_gn_joint.py) take from it:
the reference's gradient against finite differences of its own cost, its agreement with gn_affine_reference when every
(a, b) is constant, and — for every problem those tests use — the conditions under which their bounds mean something."""
import numpy as np
import pytest

import gn_affine_reference as GA
import gn_joint_reference as R
import gn_reference as GR
import graph_problems as G
from helpers import synth

FIXED, FIXED_AB, HUBER = R.FIXED, R.FIXED_AB, R.HUBER


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items()) or "base"


def test_gradient_matches_central_differences():
    """g·d of linearize against central differences of the reference's own cost (bicubic interpolation, Huber off)
    along three random directions over poses, ρ and (a, b).  Bound 1e-5, as tests/test_gn_affine_reference.py derives it:
    the central difference's own error, h² · (third derivative / first) with h = 1e-4 of steps of 1e-3, 1e-2 and — for
    (a, b), in which the cost is smooth (exp and products) — 1e-2 and 1, is of order 1e-8…1e-6 on these images."""
    pb = R.problem(synth.DOUBLE_SPHERE, 1)
    ab = R.state(pb)
    nf = pb.n_frames
    _, g, _ = R.linearize(pb, ab, pb.poses, pb.rho, 0.0)
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(3):
        dk = np.concatenate([1e-3 * rng.normal(size=(nf, 6)), rng.normal(size=(nf, 2)) * np.array([1e-2, 1.0])], 1)
        dl = 1e-2 * rng.normal(size=pb.n_points)
        d = np.concatenate([dk.ravel(), dl])
        h = 1e-4

        def cost(s):
            poses, rho, ab_s = R.apply_step(pb.poses, pb.rho, ab, s * dk, s * dl)
            c, nv = R.cost_at(pb, ab_s, poses, rho, 0.0)
            assert nv == pb.n_blocks
            return c

        fd = (cost(h) - cost(-h)) / (2 * h)
        err = abs(float(g @ d) - fd) / abs(fd)
        print(f"g·d {float(g @ d):.9g} finite difference {fd:.9g} relative disagreement {err:.2e}")
        worst = max(worst, err)
    assert worst <= 1e-5


@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_constant_brightness_is_the_geometry_reference(lam):
    """With every keyframe's (a, b) constant, S, g and the step equal gn_affine_reference's to 1e-12."""
    pb = R.problem()
    ab = R.state(pb)
    nf = pb.n_frames
    H, g, c, _ = R.reference()
    S, gS, dk, dl, m, fx = R.schur_step(H, g, ab, nf, lam, FIXED, tuple(range(nf)))
    H0, g0, c0 = GA.linearize(pb, ab, pb.poses, pb.rho, HUBER, FIXED)
    S0, gS0, dp0, dl0, m0 = GR.schur_step(H0, g0, nf, lam, FIXED)
    ip = R.parts(nf)["pose"]
    assert abs(c - c0) <= 1e-12 * c0 and abs(m - m0) <= 1e-12 * m0
    assert np.abs(S[np.ix_(ip, ip)] - S0).max() <= 1e-12 * np.abs(S0).max()
    assert np.abs(gS[ip] - gS0).max() <= 1e-12 * np.abs(gS0).max()
    assert np.abs(dk[:, :6] - dp0).max() <= 1e-12 * np.abs(dp0).max() and not dk[:, 6:].any()
    assert np.abs(dl - dl0).max() <= 1e-12 * np.abs(dl0).max()


def _conditions(label, pb, ab, lin, huber, fixed_ab=FIXED_AB):
    """The reduced system is positive definite at λ = 1e-4 (and inside fp64: a condition below 1e12 leaves a Cholesky
    factorisation four digits, ten times the step bound; measured ≤ 4e10 on the six-keyframe problems, 6e10 on the
    graphs, whose smallest eigenvalue is 0.024 against 0.57…1 there), and the step
    moves by < 2e-4 of each part's largest entry — a fifth of the GPU step bound — when the records are rounded to fp32:
    the GPU bounds then test the kernels, not rounding."""
    nf = pb.n_frames
    H, g = lin[:2]
    H2, g2, _ = R.linearize(pb, ab, pb.poses, pb.rho, huber, fp32=True)
    for lam in (1e-4, 1e-1):
        S, gS, dk, dl, m, fx = R.schur_step(H, g, ab, nf, lam, FIXED, fixed_ab)
        ev = np.linalg.eigvalsh(S)
        _, _, dk2, dl2, m2, _ = R.schur_step(H2, g2, ab, nf, lam, FIXED, fixed_ab)
        shift = {"pose": np.abs(dk2[:, :6] - dk[:, :6]).max() / np.abs(dk[:, :6]).max(),
                 "a": np.abs(dk2[:, 6] - dk[:, 6]).max() / np.abs(dk[:, 6]).max(),
                 "b": np.abs(dk2[:, 7] - dk[:, 7]).max() / np.abs(dk[:, 7]).max(),
                 "drho": np.abs(dl2 - dl).max() / np.abs(dl).max(), "model": abs(m2 - m) / m}
        print(f"{label} λ={lam}: eigenvalues {ev[0]:.3g} … {ev[-1]:.3g}; fp32 shift " +
              " ".join(f"{k} {v:.2e}" for k, v in shift.items()))
        assert ev[0] > 0 and ev[-1] < 1e12 * ev[0] and m > 0
        assert max(shift.values()) < 2e-4


@pytest.mark.parametrize("case", R.CASES, ids=case_id)
def test_gpu_problem_conditions(case):
    """Every system-and-step problem of the GPU tests: all blocks valid (483 of 644 with keyframe 3 turned away), the
    system definite, the fp32 shift small."""
    kw = dict(case)
    huber = kw.pop("huber", HUBER)
    pb = R.problem(**kw)
    lin = R.reference(huber=huber, **kw)
    assert lin[3] == (483 if kw.get("turned") else pb.n_blocks)
    _conditions(case_id(case), pb, R.state(pb), lin, huber)
    if not case:
        _conditions("halves", pb, R.state(pb), lin, huber, (0, 2))


@pytest.mark.parametrize("name", ["band37", "closed100", "closed100_idle"])
def test_graph_problem_conditions(name):
    pb = G.problem(name, changed=True)
    ab = R.state(pb)
    nv = []
    lin = R.linearize(pb, ab, pb.poses, pb.rho, HUBER, nv)
    assert nv[0] > 0.95 * pb.n_blocks
    _conditions(name, pb, ab, lin, HUBER)


def test_lm_case_conditions():
    """No trial's relative decrease lies within 0.1 of the threshold in either LM case; every candidate keeps all blocks
    valid and every ρ positive; the default run ends below the alternation's 9773.35 after 4 trials, at
    9587.087 after 8; the run with min_relative_decrease 1.3 accepts trials 1 and 2 and rejects 3 and 4."""
    pb = R.problem()
    *_, c0, c1, it, info = R.lm_reference()
    print("relative decreases", np.round(info["rel"], 3), "costs", c0, info["trial_costs"])
    assert it == R.LM_ITERATIONS and info["decisions"] == [True] * 8
    assert np.abs(np.array(info["rel"]) - 1e-3).min() >= 0.1
    assert info["invalid_candidates"] == 0 and info["valid"] == [pb.n_blocks] * 8 and min(info["min_rho"]) > 0.08
    assert abs(c0 - 223378.5547) <= 1e-3 and abs(c1 - 9587.087) <= 1e-3
    assert info["trial_costs"][3] < 9773.35
    *_, c1r, itr, infor = R.lm_reference(**R.LM_REJECT)
    print("with a rejection: relative decreases", np.round(infor["rel"], 3), "decisions", infor["decisions"])
    assert infor["decisions"] == [True, True, False, False] and itr == 4
    assert np.abs(np.array(infor["rel"]) - R.LM_REJECT["min_relative_decrease"]).min() >= 0.1
    assert infor["invalid_candidates"] == 0 and c1r == info["trial_costs"][1]
