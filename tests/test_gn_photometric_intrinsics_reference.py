"""CPU checks of tests/gn_photometric_intrinsics_reference.py and of the inputs the GPU tests
(tests/test_gpu_gn_photometric_intrinsics.py) take from it: the reference's gradient against finite differences of its
own cost, and — for every problem those tests use — the conditions under which their bounds mean something."""
import numpy as np
import pytest

import gn_photometric_intrinsics_reference as R
import photometric_intrinsics_reference as PIR
from helpers import synth

FIXED, HUBER = R.FIXED, R.HUBER


def test_gradient_matches_central_differences():
    """g·d of linearize against central differences of the reference's own cost (bicubic interpolation, Huber off) along
    three random directions over poses, K and ρ, at step sizes 1e-6 of each part's scale.
    Measured: relative disagreement 7.0e-8, 4.7e-8, 2.6e-9 → bound 7e-7 (10× the largest; no looser than 1e-4)."""
    pb = R.problem(synth.DOUBLE_SPHERE, 1)
    K = R.state(pb)
    nf, nc = pb.n_frames, pb.intrinsics.shape[0]
    _, g, _ = R.linearize(pb, pb.poses, pb.rho, K, 0.0)
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(3):
        dp = 1e-3 * rng.normal(size=(nf, 6))
        dk = rng.normal(size=(nc, 8)) * np.array([1, 1, 1, 1, 1e-3, 1e-3, 0, 0])
        dl = 1e-2 * rng.normal(size=pb.n_points)
        d = np.concatenate([dp.ravel(), dk.ravel(), dl])
        h = 1e-4

        def cost(s):
            c, nv = R.cost_at(pb, synth.se3_plus(pb.poses, s * dp), pb.rho + s * dl, K + s * dk, 0.0)
            assert nv == pb.n_blocks
            return c

        fd = (cost(h) - cost(-h)) / (2 * h)
        err = abs(float(g @ d) - fd) / abs(fd)
        print(f"g·d {float(g @ d):.9g} finite difference {fd:.9g} relative disagreement {err:.2e}")
        worst = max(worst, err)
    assert worst <= 7e-7


@pytest.mark.parametrize("model", [0, 1, 2, 3])
@pytest.mark.parametrize("interp", [0, 1])
def test_residuals_at_agrees_with_compose(model, interp):
    """residuals_at (the warp with ρ itself, for candidates that may carry ρ ≤ 0) against compose's residuals where
    compose is defined (ρ > 0): the same validity and the same residuals to fp64 rounding of the projection."""
    pb = R.problem(model, interp)
    K = R.state(pb)
    assert (pb.rho > 0).all()
    rec, valid, _ = PIR.compose(pb, K, want_jac=False)
    r, v = R.residuals_at(pb, pb.poses, pb.rho, K)
    assert np.array_equal(v, valid)
    err = np.abs(r - rec[:, :pb.pattern.shape[0]]).max()
    print(f"model {model} interp {interp}: max residual difference {err:.2e}")
    assert err <= 1e-8


def _fp32_shift(pb, rec, valid, H, g, huber, lam):
    """How far the reference step moves when the records are rounded to fp32 and back."""
    df = R.step(H, g, pb, lam, FIXED)[2]
    H2, g2, _, _ = R.system_from_records(pb, rec.astype(np.float32).astype(np.float64), valid, huber, FIXED)
    return np.linalg.norm(R.step(H2, g2, pb, lam, FIXED)[2] - df) / np.linalg.norm(df)


CASES = ([dict(model=m, interp=i) for m in range(4) for i in (0, 1)] + [dict(P=P) for P in (1, 21, 32)] +
         [dict(cams="two"), dict(cams="idle"), dict(huber=0.0)])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_gpu_problem_conditions(case):
    """Every base-problem variant of the GPU tests: ≥ 0.9 of the blocks valid, and the reference step moves by < 2e-4 (a
    fifth of the step bound) when it is rebuilt from records rounded to fp32 — the precedent of
    gn_reference.reduced_system_from_records."""
    huber = case.get("huber", HUBER)
    pb = R.problem(**{k: v for k, v in case.items() if k != "huber"})
    rec, valid, (H, g, _), w = R.reference(**case)
    assert valid.sum() >= 0.9 * pb.n_blocks
    if huber > 0:
        assert (w[valid == 1] < 1.0).mean() >= 0.05
    for lam in ((1e-4, 1e-1) if "model" in case else (1e-3,)):
        shift = _fp32_shift(pb, rec, valid, H, g, huber, lam)
        print(f"{case} λ={lam}: fp32 step shift {shift:.2e}")
        assert shift < 2e-4


def test_turned_keyframe_conditions():
    """Keyframe 3 turned 120° about its y axis: between 5 % and 40 % of the blocks are invalid, all of them blocks that
    target it, and every other block is valid.  (Not every block targeting it is invalid: with a ±39° field of view a
    point up to 9° inside one image edge still lies in front of the turned pinhole camera — its pixels project far
    outside the image, where the interpolator's edge clamp gives a residual with a zero gradient.)"""
    pb = R.problem(turned=True)
    rec, valid, (H, g, _), _ = R.reference(turned=True)
    share = 1.0 - valid.mean()
    print(f"invalid share {share:.3f}; of the blocks targeting keyframe 3: {1 - valid[pb.block_target == 3].mean():.3f}")
    assert 0.05 <= share <= 0.40
    assert valid[pb.block_target == 3].mean() <= 0.2 and valid[pb.block_target != 3].all()
    assert _fp32_shift(pb, rec, valid, H, g, HUBER, 1e-3) < 2e-4


def test_long_point_conditions():
    pb = R.long_point_problem()
    assert pb.n_frames >= 71 and np.bincount(pb.block_point).max() == 70 and 1 <= pb.n_blocks % 256 <= 192
    K = R.state(pb)
    rec, valid = R.records(pb, pb.poses, pb.rho, K)
    assert valid.sum() >= 0.9 * pb.n_blocks
    H, g, _, _ = R.system_from_records(pb, rec, valid, HUBER, FIXED)
    assert _fp32_shift(pb, rec, valid, H, g, HUBER, 1e-3) < 2e-4


def test_pyramid_level_conditions():
    pb = R.problem()
    pb1 = synth.level_problem(pb, 1)
    rec, valid = R.records(pb1, pb.poses, pb.rho, PIR.level_state(R.state(pb), 1), intr_scale=0.5)
    assert valid.sum() >= 0.9 * pb.n_blocks
    H, g, _, _ = R.system_from_records(pb1, rec, valid, HUBER, FIXED)
    assert _fp32_shift(pb1, rec, valid, H, g, HUBER, 1e-3) < 2e-4


def test_lm_case_conditions():
    """Every relative decrease of the reference run lies ≥ 0.03 from min_relative_decrease, and the run rejects trials."""
    _, _, kw = R.lm_case()
    info = R.lm_reference()[6]
    print("relative decreases", np.round(info["rel"], 3), "cost decreases", np.round(info["dcost"], 1))
    assert len(info["rel"]) == kw["max_iterations"]
    assert np.abs(np.array(info["rel"]) - kw["min_relative_decrease"]).min() >= 0.03
    assert info["unsuccessful_steps"] >= 1 and info["successful_steps"] >= 1
    assert info["min_rho"] > 0  # every candidate inside the reference's own domain (compose's twin needs ρ > 0)


def test_recovery_conditions():
    """The reference LM recovers the calibration with a factor 2 to spare on both of the GPU test's criteria: the final
    cost within 2.5 % of the cost at ground truth, |fx − fx_gt| and |fy − fy_gt| at most half of what they start at."""
    pb, K0 = R.recovery_problem()
    c_gt, _ = R.cost_at(pb, pb.poses_gt, pb.rho_gt, pb.intrinsics, HUBER)
    _, _, k, _, c_final, _, info = R.recovery_reference()
    e0, e1 = np.abs(K0[0, :2] - pb.intrinsics[0, :2]), np.abs(k[0, :2] - pb.intrinsics[0, :2])
    print(f"cost {c_final:.6g} against {c_gt:.6g}; |fx, fy error| {e0} -> {e1}; {info['stop_reason']}")
    assert c_final <= 1.025 * c_gt and info["min_rho"] > 0
    assert (e1 <= 0.5 * e0).all()
