"""CPU tests of the dense GN/LM reference (tests/gn_reference.py) used to check the on-device solver."""
import numpy as np

import gn_reference as GR
from helpers import synth


def test_reference_lm_recovers_geometric_problem():
    pb = synth.make_problem(kind="geometric", n_frames=7, n_points=80, seed=3, obs_sigma=0.0, pose_sigma=0.002,
                            rho_sigma=0.02)
    pb.poses[:2] = pb.poses_gt[:2]  # gauge: two constant frames, as map_utils.h:334-336 / sfm.cpp:1903
    poses, rho, c0, c1, it = GR.lm(pb, a=1.0, fixed=(0, 1))
    assert c1 < 1e-8 * max(c0, 1.0) + 1e-12
    np.testing.assert_allclose(poses[:, 4:], pb.poses_gt[:, 4:], atol=1e-6)
    np.testing.assert_allclose(rho, pb.rho_gt, rtol=1e-6)


def test_schur_step_equals_full_solve():
    pb = synth.make_problem(n_frames=6, n_points=40, width=320, height=200, seed=4, border=12)
    H, g, _ = GR.linearize(pb, pb.poses, pb.rho, 9.0, fixed=(0,))
    lam = 1e-3
    S, gS, dp, dl, model = GR.schur_step(H, g, pb.n_frames, lam, fixed=(0,))
    # full damped system with frame 0 removed
    D = np.clip(np.diag(H), 1e-6, 1e32)
    keep = np.ones(H.shape[0], bool)
    keep[:6] = False
    Ha = (H + lam * np.diag(D))[np.ix_(keep, keep)]
    full = np.linalg.solve(Ha, -g[keep])
    np.testing.assert_allclose(np.concatenate([dp.ravel()[6:], dl]), full, rtol=1e-6, atol=1e-9)
    assert model > 0


def test_linearize_intrinsics_equals_dense_per_block_accumulation():
    """linearize_intrinsics adds each block's 21 nonzero columns (np.ix_ scatter); held here to the dense accumulation
    it replaced — a 2 × N Jacobian and an N × N product per block — on the 10-keyframe, 2-camera rig of
    test_free_intrinsics_reduced_system_and_step: H equal (to 1e-15 of its scale), g to 1e-12 of its scale, the cost
    the same number."""
    import oracle as O
    pb0 = synth.make_problem(kind=1, model=0, n_frames=10, n_points=120, width=376, height=240, seed=13, border=12)
    k1 = pb0.intrinsics[0].copy()
    k1[:4] *= np.array([1.01, 0.99, 1.0, 1.0])
    intr = np.stack([pb0.intrinsics[0], k1])
    pb = synth.make_problem(kind=1, model=0, n_frames=10, n_points=120, width=376, height=240, seed=13, border=12,
                            intrinsics=intr, frame_cam=np.arange(10, dtype=np.int32) % 2)
    state = intr * np.array([1.003, 0.998, 1.0005, 0.9995, 1, 1, 1, 1])
    fixed = (0, 1)
    H, g, cost = GR.linearize_intrinsics(pb, pb.poses, pb.rho, state, 1.0, fixed)
    # the dense accumulation
    rec, valid = O.evaluate_intrinsics(pb, state, poses=pb.poses, rho=pb.rho)
    r, Jh, Jt, Jr = O.split_record(rec[:, :28], 2)
    Ji = rec[:, 28:44].reshape(-1, 2, 8)
    cost_b, w = GR.huber((r ** 2).sum(1), 1.0)
    w = np.where(valid == 1, w, 0.0)
    nf, nc, npt = pb.n_frames, 2, pb.n_points
    K0 = 6 * nf
    N = K0 + 8 * nc + npt
    Hd, gd = np.zeros((N, N)), np.zeros(N)
    for b in range(pb.n_blocks):
        if w[b] == 0:
            continue
        p = pb.block_point[b]
        h, t = pb.point_host[p], pb.block_target[b]
        c = pb.frame_cam[t]
        J = np.zeros((2, N))
        if h not in fixed:
            J[:, 6 * h:6 * h + 6] = Jh[b]
        if t not in fixed:
            J[:, 6 * t:6 * t + 6] = Jt[b]
        J[:, K0 + 8 * c:K0 + 8 * c + 8] = Ji[b]
        J[:, K0 + 8 * nc + p] = Jr[b]
        Hd += w[b] * J.T @ J
        gd += w[b] * J.T @ r[b]
    assert H.shape == (N, N) and g.shape == (N,) and (w > 0).sum() > 0.9 * pb.n_blocks
    eH, eg = np.abs(H - Hd).max() / np.abs(Hd).max(), np.abs(g - gd).max() / np.abs(gd).max()
    print(f"\nlinearize_intrinsics vs dense: H {eH:.2e} g {eg:.2e} of their scale")
    assert eH <= 1e-15, eH
    assert eg <= 1e-12, eg
    assert cost == float(np.where(valid == 1, cost_b, 0.0).sum())
    assert not H[:12].any() and not H[:, :12].any() and not g[:12].any()  # the constant frames' columns
