"""CPU checks of tests/gn_affine_reference.py and of the inputs the GPU tests (tests/test_gpu_gn_affine.py) take from it:
the reference's gradient against finite differences of its own cost at a non-zero affine state, and — for every problem
those tests use — the conditions under which their bounds mean something."""
import numpy as np
import pytest

import gn_affine_reference as R
import gn_reference as GR
import photometric_affine_reference as PAR
from helpers import synth

FIXED, HUBER = R.FIXED, R.HUBER


def test_problem_is_brightness_case_perturbed():
    """The base problem has brightness_case's images and host intensities, and a state away from the true one."""
    pb = R.problem()
    bc, _, _ = PAR.brightness_case()
    assert np.array_equal(pb.images, bc.images) and np.array_equal(pb.host_intensity, bc.host_intensity)
    assert np.array_equal(pb.block_point, bc.block_point) and np.array_equal(pb.block_target, bc.block_target)
    assert np.abs(pb.poses - bc.poses).max() > 1e-3 and np.abs(pb.rho / bc.rho - 1).max() > 1e-2
    assert pb.n_blocks % 32 == 4 and R.problem(drop=7).n_blocks % 32 == 29


def test_gradient_matches_central_differences():
    """g·d of linearize against central differences of the reference's own cost (bicubic interpolation, Huber off, the
    affine state at parity_state and constant) along three random directions over poses and ρ.
    Bound 1e-5: the central difference's own error, h² · (third derivative / first) with h = 1e-4 of steps of 1e-3 and
    1e-2, is of order 1e-8…1e-6 on these images (tests/test_gn_photometric_intrinsics_reference.py measured ≤ 7e-8)."""
    pb = R.problem(synth.DOUBLE_SPHERE, 1)
    ab = R.state(pb)
    nf = pb.n_frames
    _, g, _ = R.linearize(pb, ab, pb.poses, pb.rho, 0.0)
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(3):
        dp = 1e-3 * rng.normal(size=(nf, 6))
        dl = 1e-2 * rng.normal(size=pb.n_points)
        d = np.concatenate([dp.ravel(), dl])
        h = 1e-4

        def cost(s):
            c, nv = R.cost_at(pb, ab, synth.se3_plus(pb.poses, s * dp), pb.rho + s * dl, 0.0)
            assert nv == pb.n_blocks
            return c

        fd = (cost(h) - cost(-h)) / (2 * h)
        err = abs(float(g @ d) - fd) / abs(fd)
        print(f"g·d {float(g @ d):.9g} finite difference {fd:.9g} relative disagreement {err:.2e}")
        worst = max(worst, err)
    assert worst <= 1e-5


def test_zero_state_is_the_plain_reference():
    """At a = b = 0 the reference is gn_reference's own linearisation of the same problem."""
    pb = R.problem()
    H, g, c = R.linearize(pb, np.zeros((pb.n_frames, 2)), pb.poses, pb.rho, HUBER, FIXED)
    H0, g0, c0 = GR.linearize(pb, pb.poses, pb.rho, HUBER, FIXED)
    assert abs(c - c0) <= 1e-12 * c0
    assert np.abs(H - H0).max() <= 1e-12 * np.abs(H0).max() and np.abs(g - g0).max() <= 1e-12 * np.abs(g0).max()


def _fp32_shift(pb, ab, H, g, huber, lam):
    """How far the reference step moves when the records are rounded to fp32 and back."""
    dp = GR.schur_step(H, g, pb.n_frames, lam, FIXED)[2]
    H2, g2, _ = R.linearize(pb, ab, pb.poses, pb.rho, huber, FIXED, fp32=True)
    return np.linalg.norm(GR.schur_step(H2, g2, pb.n_frames, lam, FIXED)[2] - dp) / np.linalg.norm(dp)


CASES = [dict(), dict(interp=1), dict(P=5), dict(P=12, interp=1), dict(P=21), dict(P=32, interp=1),
         dict(model=synth.KB4, interp=1), dict(model=synth.KB4, P=21), dict(P=12, cams=2), dict(cams=2), dict(drop=7),
         dict(turned=True), dict(turned=True, P=21), dict(huber=60.0), dict(huber=0.0), dict(huber=60.0, P=32)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()) or "base")
def test_gpu_problem_conditions(case):
    """Every problem of the GPU tests: the valid share (all blocks, or all but keyframe 3's when it is turned away); the
    affine state matters (the cost at parity_state is at least twice the cost at zeros); Huber 9 weights nearly every
    block, Huber 60 between 5 % and 95 % of them; and the reference step moves by < 2e-4 (a fifth of the step bound) when
    it is rebuilt from records rounded to fp32."""
    kw = dict(case)
    huber = kw.pop("huber", HUBER)
    pb = R.problem(**kw)
    ab = R.state(pb)
    valid, (H, g, cost), w = R.reference(huber=huber, **kw)
    m = valid == 1
    third = (pb.point_host[pb.block_point] == 3) | (pb.block_target == 3)
    if kw.get("turned"):
        assert third.sum() == 161 and not m[third].any() and m[~third].all()
    else:
        assert m.all()
    c0, _ = R.cost_at(pb, np.zeros_like(ab), pb.poses, pb.rho, huber)
    assert cost >= 2.0 * c0
    if huber == HUBER:
        assert (w[m] < 1.0).mean() >= 0.95
    elif huber > 0:
        assert 0.05 <= (w[m] < 1.0).mean() <= 0.95
    for lam in (1e-4, 1e-1):
        shift = _fp32_shift(pb, ab, H, g, huber, lam)
        print(f"{case} λ={lam}: inside the Huber width {(w[m] == 1.0).mean():.3f}, fp32 step shift {shift:.2e}")
        assert shift < 2e-4


def test_lm_case_conditions():
    """Every relative decrease of the reference run lies ≥ 0.1 from min_relative_decrease (1e-3), the run accepts and
    rejects trials, no candidate invalidates a block, and the cost falls by more than a tenth."""
    p, rho, c0, c1, it, info = R.lm_reference()
    print("relative decreases", np.round(info["rel"], 3), "costs", c0, c1)
    assert len(info["rel"]) == R.LM_OPTIONS["max_iterations"] == it
    assert np.abs(np.array(info["rel"]) - 1e-3).min() >= 0.1
    assert info["successful_steps"] >= 3 and info["unsuccessful_steps"] >= 1 and info["invalid_candidates"] == 0
    assert c1 < 0.9 * c0


def test_brightness_gradient_matches_central_differences():
    """Reference (ii): g·d of linearize_ab against central differences of the cost along three random (a, b) directions
    (Huber off; nothing fixed).  The cost is smooth in (a, b) — exp and products — so the difference quotient's own error
    at h = 1e-4 is ~h² ≈ 1e-8 relative; bound 1e-7."""
    pb = R.problem()
    ab = R.state(pb)
    _, g, _, free = R.linearize_ab(pb, ab, 0.0)
    assert free.all()
    rng = np.random.default_rng(1)
    for _ in range(3):
        d = rng.normal(size=(pb.n_frames, 2)) * np.array([1e-2, 1.0])
        h = 1e-4
        fd = (R.cost_ab(pb, ab + h * d, 0.0) - R.cost_ab(pb, ab - h * d, 0.0)) / (2 * h)
        err = abs(float(g @ d.ravel()) - fd) / abs(fd)
        print(f"g·d {float(g @ d.ravel()):.9g} finite difference {fd:.9g} relative disagreement {err:.2e}")
        assert err <= 1e-7


def test_brightness_reference_conditions():
    """The brightness problems of the GPU tests: with keyframe 0 fixed the system is well conditioned enough for the
    1e-3 step bound (the step moves < 2e-4 when r and the J_ab blocks are rounded to fp32 — here through the cost of a
    1e-7 relative perturbation of H and g), the turned keyframe and a non-finite a are constant, and the reference LM on
    brightness_case ends at brightness_run's 2113 figure."""
    pb = R.problem()
    ab = R.state(pb)
    for fixed in ((0,), ()):
        H, g, _, free = R.linearize_ab(pb, ab, HUBER, fixed)
        d, _ = R.step_ab(H, g, free, 1e-1)
        rng = np.random.default_rng(2)
        H2 = H * (1 + 1e-7 * rng.uniform(-1, 1, H.shape))
        H2 = 0.5 * (H2 + H2.T)
        d2, _ = R.step_ab(H2, g * (1 + 1e-7 * rng.uniform(-1, 1, g.shape)), free, 1e-1)
        shift = np.linalg.norm(d2 - d) / np.linalg.norm(d)
        print(f"fixed {fixed}: step shift under a 1e-7 perturbation {shift:.2e}")
        assert shift < 2e-4
    assert not R.linearize_ab(R.problem(turned=True), ab, HUBER, (0,))[3][3]
    bad = ab.copy()
    bad[3, 0] = np.nan
    assert not R.linearize_ab(pb, bad, HUBER, (0,))[3][3]
    bc, _, _ = PAR.brightness_case()
    _, c0, c1, it, info = R.lm_ab(bc, np.zeros((bc.n_frames, 2)), 0.0, (0,))
    c_run, _ = PAR.brightness_run(lambda s: PAR.compose(bc, s)[:2], bc)
    print(f"lm_ab on brightness_case: {c0} -> {c1} in {it} iterations ({info['stop_reason']}); brightness_run {c_run[-1]}")
    assert abs(c1 - c_run[-1]) <= 1e-6 * c_run[-1] and info["converged"]
    assert np.abs(np.array(info["rel"]) - 1e-3).min() >= 0.1
