"""CPU checks of tests/graph_problems.py: the conditions under which the bounds of tests/test_gpu_graphs.py mean something.
The structure of every problem by brute force from (point_host, block_point, block_target); the share of valid blocks;
how far the reference's own steps move when its records are rounded to fp32 (at most 1e-5, 100× under the 1e-3 step
bound, at every case the GPU tests use); and the margins of every decision of the two reference LM runs."""
import numpy as np
import pytest

import gn_affine_reference as R
import gn_reference as GR
import graph_problems as G
import photometric_affine_reference as PAR
from helpers import synth

SHIFT = 1e-5


def test_linearize_records_is_gn_reference_linearize():
    """The block-sparse accumulation of graph_problems.linearize_records against gn_reference.linearize's dense one
    (geometric band37: 592 unknowns), and against gn_affine_reference.linearize on the photometric problem."""
    pb = G.problem("band37", kind=synth.GEOMETRIC)
    _, _, (H, g, c) = G.pose_reference("band37", 1.0, kind=synth.GEOMETRIC)
    H0, g0, c0 = GR.linearize(pb, pb.poses, pb.rho, 1.0, G.FIXED)
    assert abs(c - c0) <= 1e-12 * c0
    assert np.abs(H - H0).max() <= 1e-12 * np.abs(H0).max() and np.abs(g - g0).max() <= 1e-12 * np.abs(g0).max()
    pb = G.problem("band37", changed=True)
    _, _, (H, g, c) = G.pose_reference("band37", 9.0, changed=True)
    H0, g0, c0 = R.linearize(pb, PAR.parity_state(37), pb.poses, pb.rho, 9.0, G.FIXED)
    assert c == c0 and np.array_equal(H, H0) and np.array_equal(g, g0)


@pytest.mark.parametrize("name", list(G.NAMED))
def test_structure(name):
    pb = G.problem(name)
    st = G.structure(pb)
    print({k: v for k, v in st.items() if k not in ("widths", "first")}, sorted(w for w in st["widths"] if w > 10))
    assert pb.n_frames == G.NAMED[name]["n_frames"] and pb.n_points == G.NAMED[name]["n_points"]
    assert np.all(np.diff(pb.block_point) >= 0)  # a point's blocks are contiguous
    assert 3 * st["backward_pairs"] >= st["pairs"]
    assert st["both_ways"] >= 100
    assert st["straddling_points"] >= 1
    if name == "band37":
        assert st["max_width"] == 10
    else:
        assert st["max_width"] == 200 and {63, 64, 65, 66, 129, 130, 199, 200} <= st["widths"]
        assert st["pairs"] > 256 and st["skyline_blocks"] > 256
        assert st["unfilled_envelope_blocks"] >= 1 and st["first_right"] >= 1 and st["first_left"] >= 1
        host = pb.point_host[pb.block_point]
        for h, t in G.CLOSURES:  # every closure is there, in its direction
            assert ((host == h) & (pb.block_target == t)).any()
    if name == "closed100_idle":
        assert not ((pb.point_host[pb.block_point] == 50) | (pb.block_target == 50)).any()
        assert st["first"][50] == 50 and st["first"][64] == 0  # no block, inside a wide row


@pytest.mark.parametrize("name", list(G.NAMED))
def test_validity(name):
    """At least 95 % of the blocks are valid at the perturbed state, in every form the GPU tests use."""
    for kw in (dict(), dict(changed=True), dict(kind=synth.GEOMETRIC)):
        pb = G.problem(name, **kw)
        _, valid = G.records(pb, PAR.parity_state(pb.n_frames) if kw.get("changed") else None)
        print(name, kw, pb.n_blocks, "blocks,", float(valid.mean()), "valid")
        assert valid.mean() >= 0.95
    extra = {"band37": (dict(kind=synth.GEOMETRIC, model=synth.KB4), dict(cams=2), dict(kind=synth.GEOMETRIC, cams=2)),
             "closed100": (dict(P=21, changed=True),)}
    for kw in extra.get(name, ()):
        assert G.records(G.problem(name, **kw))[1].mean() >= 0.95


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


POSE = ([(n, h, {}) for n, h in G.POSE_CASES]
        + [(n, 1.0, dict(kind=synth.GEOMETRIC, model=m)) for n, m in G.GEOMETRIC_CASES]
        + [("band37", R.HUBER, dict(changed=True))])


@pytest.mark.parametrize("name,huber,kw", POSE, ids=lambda x: str(x).replace(" ", ""))
def test_pose_reference_sensitivity(name, huber, kw):
    """Groups a, b and d: the reference's pose step, δρ and model decrease from records rounded to fp32."""
    pb = G.problem(name, **kw)
    _, _, (H, g, _) = G.pose_reference(name, huber, **kw)
    _, _, (H2, g2, _) = G.pose_reference(name, huber, fp32=True, **kw)
    for lam in G.LAMBDAS:
        _, _, dp, dl, m = GR.schur_step(H, g, pb.n_frames, lam, G.FIXED)
        _, _, dp2, dl2, m2 = GR.schur_step(H2, g2, pb.n_frames, lam, G.FIXED)
        shift = (_rel(dp2, dp), _rel(dl2, dl), abs(m2 - m) / abs(m))
        print(f"{name} Huber {huber} {kw} λ={lam}: pose step {shift[0]:.2e} δρ {shift[1]:.2e} model {shift[2]:.2e}")
        assert max(shift) <= SHIFT


@pytest.mark.parametrize("name,P,huber,fixed", G.BRIGHTNESS_CASES)
def test_brightness_reference_sensitivity(name, P, huber, fixed):
    """Group c: the reference's brightness step and model decrease from compose's records rounded to fp32 with ±1.5e-5
    of noise on r; and the constant keyframes are the fixed ones (and the idle one) alone."""
    pb = G.problem(name, P=P, changed=True)
    ab = PAR.parity_state(pb.n_frames)
    H, g, _, free = R.linearize_ab(pb, ab, huber, fixed)
    with G.perturbed_compose():
        H2, g2, _, free2 = R.linearize_ab(pb, ab, huber, fixed)
    assert np.array_equal(free, free2) and not np.array_equal(H, H2)
    constant = set(fixed) | ({50} if name == "closed100_idle" else set())
    assert set(np.nonzero(~free)[0].tolist()) == constant
    for lam in G.LAMBDAS:
        d, m = R.step_ab(H, g, free, lam)
        d2, m2 = R.step_ab(H2, g2, free2, lam)
        print(f"{name} P {P} Huber {huber} fixed {fixed} λ={lam}: step {_rel(d2, d):.2e} model {abs(m2 - m) / abs(m):.2e}")
        assert _rel(d2, d) <= SHIFT and abs(m2 - m) <= SHIFT * abs(m)


def test_free_intrinsics_reference_sensitivity():
    """Group g: the two free-intrinsics references take the rewired problem as it is; their f-step (poses and
    intrinsics) and δρ at λ = 1e-1 from records rounded to fp32."""
    import gn_photometric_intrinsics_reference as RI
    pb = G.problem("band37", cams=2)
    assert pb.intrinsics.shape[0] == 2 and np.array_equal(pb.frame_cam, np.arange(37) % 2)
    K = RI.state(pb)
    rec, valid = RI.records(pb, pb.poses, pb.rho, K)
    out = []
    for r in (rec, rec.astype(np.float32).astype(np.float64)):
        H, g, _, _ = RI.system_from_records(pb, r, valid, RI.HUBER, G.FIXED)
        out.append(RI.step(H, g, pb, 1e-1, G.FIXED))
    shift = (_rel(out[1][2], out[0][2]), _rel(out[1][5], out[0][5]), abs(out[1][6] - out[0][6]) / abs(out[0][6]))
    print(f"photometric free intrinsics: f-step {shift[0]:.2e} δρ {shift[1]:.2e} model {shift[2]:.2e}")
    assert valid.mean() >= 0.95 and max(shift) <= SHIFT
    pg = G.problem("band37", kind=synth.GEOMETRIC, cams=2)
    plain, out = GR.O.evaluate_intrinsics, []
    for fp32 in (False, True):
        def evaluate(*args, **kw):
            rec, valid = plain(*args, **kw)
            return (rec.astype(np.float32).astype(np.float64) if fp32 else rec), valid

        GR.O.evaluate_intrinsics = evaluate
        try:
            H, g, _ = GR.linearize_intrinsics(pg, pg.poses, pg.rho, G.intrinsics_state(pg), 1.0, G.FIXED)
        finally:
            GR.O.evaluate_intrinsics = plain
        out.append(GR.schur_step_intrinsics(H, g, 37, 2, 1e-1, G.FIXED))
    shift = (_rel(out[1][2], out[0][2]), _rel(out[1][3], out[0][3]), abs(out[1][4] - out[0][4]) / abs(out[0][4]))
    print(f"geometric free intrinsics: f-step {shift[0]:.2e} δρ {shift[1]:.2e} model {shift[2]:.2e}")
    assert max(shift) <= SHIFT and not np.array_equal(out[0][2], out[1][2])


def test_lm_case_conditions():
    """The pose loop on band37: at least 3 accepted and 1 rejected trial; every relative decrease at least 0.1 from
    min_relative_decrease; every tolerance test a factor 2 from its threshold (Ceres' defaults: function 1e-6, parameter
    1e-8, gradient 1e-10); no candidate invalidates a block or carries ρ ≤ 0."""
    _, _, c0, c1, it, info = G.lm_reference()
    rel, hist, costs = np.array(info["rel"]), info["history"], info["trial_costs"]
    print("relative decreases", np.round(rel, 3), "decisions", [h[1] for h in hist], "costs", c0, c1, info["stop_reason"])
    assert it == G.LM_OPTIONS["max_iterations"] == len(rel) and info["stop_reason"] == "max_iterations"
    assert info["successful_steps"] >= 3 and info["unsuccessful_steps"] >= 1
    assert info["invalid_candidates"] == 0 and info["min_rho"] > 0.0
    assert np.abs(rel - G.LM_OPTIONS["min_relative_decrease"]).min() >= 0.1
    cur = costs[0]
    assert info["gnorm0"] >= 2 * 1e-10
    for (_, accepted, step, x_norm, gnorm), cand in zip(hist, costs[1:]):
        assert step >= 2 * 1e-8 * (x_norm + 1e-8) and abs(cur - cand) >= 2 * 1e-6 * cur
        if accepted:
            cur = cand
            assert gnorm >= 2 * 1e-10
    assert cur == c1 < 0.9 * c0


def test_lm_ab_case_conditions():
    """The brightness loop on closed100: the same conditions."""
    pb = G.problem("closed100", changed=True)
    ab, c0, c1, it, info = G.lm_ab_reference()
    rel = np.array(info["rel"])
    print("relative decreases", np.round(rel, 3), "decisions", info["decisions"], "costs", c0, c1, info["stop_reason"])
    assert it == G.LM_AB_OPTIONS["max_iterations"] == len(rel) and info["stop_reason"] == "max_iterations"
    assert info["successful_steps"] >= 3 and info["unsuccessful_steps"] >= 1
    assert np.abs(rel - G.LM_AB_OPTIONS["min_relative_decrease"]).min() >= 0.1
    cur, x, x_norm = c0, G.lm_ab_start(pb), -1.0
    free = np.ones(pb.n_frames, bool)
    free[list(G.LM_AB_FIXED)] = False

    def gradient(state):
        _, g, _, fr = R.linearize_ab(pb, state, G.LM_AB_HUBER, G.LM_AB_FIXED)
        assert np.array_equal(fr, free)
        return np.abs(g).max()

    assert gradient(x) >= 2 * 1e-10
    for accepted, cand, d in zip(info["decisions"], info["candidates"], info["steps"]):
        assert np.linalg.norm(d) >= 2 * 1e-8 * (x_norm + 1e-8) and abs(cur - cand) >= 2 * 1e-6 * cur
        if accepted:
            cur, x = cand, x + d
            x_norm = float(np.linalg.norm(x[free]))
            assert gradient(x) >= 2 * 1e-10
    assert np.array_equal(x, ab) and abs(cur - c1) <= 1e-12 * c1 and c1 < 0.9 * c0
