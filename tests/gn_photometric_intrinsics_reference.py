"""Dense fp64 Gauss-Newton / LM reference for photometric blocks with the target camera's intrinsics free
(pba_set_optimize_intrinsics + pba_gn_set_solve_intrinsics): gn_reference.linearize_intrinsics generalised to P rows.

The rows come from photometric_intrinsics_reference.compose (22·P values per block: r, J_host, J_target, J_rho and
J_intr = ∇I·∂π/∂k with respect to the target camera's intrinsics state), every product and sum is fp64, and the step is
gn_reference.schur_step_intrinsics over the unknowns [6 per keyframe | 8 per camera | 1 per point].

Also the problems the GPU tests use (tests/test_gpu_gn_photometric_intrinsics.py), so that the CPU tests
(tests/test_gn_photometric_intrinsics_reference.py) assert their input conditions on exactly the same inputs.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import gn_reference as GR
import photometric_intrinsics_reference as PIR
from helpers import synth

FIXED = (0, 1)
HUBER = 9.0


def records(pb, poses, rho, K, intr_scale: float = 1.0):
    """compose's records and validity at (poses, ρ, K); J_intr columns 0-3 scaled by intr_scale (2^−level: the unknown is
    the level-0 state, pba.h)."""
    rec, valid, _ = PIR.compose(pb, K, poses, rho)
    if intr_scale != 1.0:
        P = pb.pattern.shape[0]
        Ji = rec[:, 14 * P:].reshape(-1, P, 8)
        Ji[:, :, :4] *= intr_scale
    return rec, valid


def system_from_records(pb, rec, valid, a, fixed=()):
    """(H, g, cost, w) over N = 6·nf + 8·nc + n_points from 22·P-value records; fixed frames' columns zeroed."""
    P = pb.pattern.shape[0]
    rec = np.asarray(rec, np.float64)
    r, Jh, Jt, Jr, Ji = PIR.split(rec, P)
    s = (r ** 2).sum(1)
    cost_b, w = GR.huber(s, a)
    w = np.where(valid == 1, w, 0.0)
    cost = float(np.where(valid == 1, cost_b, 0.0).sum())
    nf, nc, npt = pb.n_frames, pb.intrinsics.shape[0], pb.n_points
    K0 = 6 * nf
    N = K0 + 8 * nc + npt
    fixed = set(int(f) for f in fixed)
    H = np.zeros((N, N))
    g = np.zeros(N)
    six, eight = np.arange(6), np.arange(8)
    for b in range(pb.n_blocks):
        if w[b] == 0:
            continue
        p = pb.block_point[b]
        h, t = pb.point_host[p], pb.block_target[b]
        c = pb.frame_cam[t]
        cols, parts = [], []
        if h not in fixed:
            cols.append(6 * h + six)
            parts.append(Jh[b])
        if t not in fixed:
            cols.append(6 * t + six)
            parts.append(Jt[b])
        cols += [K0 + 8 * c + eight, np.array([K0 + 8 * nc + p])]
        parts += [Ji[b], Jr[b][:, None]]
        idx, J = np.concatenate(cols), np.concatenate(parts, axis=1)
        H[np.ix_(idx, idx)] += w[b] * J.T @ J
        g[idx] += w[b] * J.T @ r[b]
    return H, g, cost, w


def linearize(pb, poses, rho, K, a, fixed=(), intr_scale: float = 1.0, n_valid=None):
    """(H, g, cost) over N = 6·nf + 8·nc + n_points at (poses, ρ, K)."""
    rec, valid = records(pb, poses, rho, K, intr_scale)
    if n_valid is not None:
        n_valid.append(int(valid.sum()))
    H, g, cost, _ = system_from_records(pb, rec, valid, a, fixed)
    return H, g, cost


def residuals_at(pb, poses, rho, K):
    """(residuals (n_blocks, P), valid) at (poses, ρ, K) straight from the warp p̃ = R_th b + ρ t_th: π_K(p̃) sampled with
    the oracle's interpolator, minus I_h; valid where every p̃ lies in the state camera's projection domain and every
    value is finite.  compose goes through the geometric twin b/ρ, which is the same point only while ρ > 0; a
    Gauss-Newton candidate may carry ρ ≤ 0, and the engine (like photometric_error.h:158-159) warps with ρ itself."""
    import oracle as O
    P = pb.pattern.shape[0]
    K = np.ascontiguousarray(K, np.float64).reshape(-1, 8)
    with np.errstate(all="ignore"):
        p = PIR.warped_points(pb, np.ascontiguousarray(poses, np.float64), np.ascontiguousarray(rho, np.float64))
    Kt = K[pb.frame_cam[pb.block_target]]
    r = np.zeros((pb.n_blocks, P))
    ok = np.ones(pb.n_blocks, bool)
    interp = int(getattr(pb, "interp", 0))
    for k in range(P):
        ok &= PIR.in_domain(pb.model, Kt, p[:, k])
        with np.errstate(all="ignore"):
            uv = synth.project(pb.model, Kt, p[:, k])
        fin = np.isfinite(uv).all(1)
        ok &= fin
        for t in np.unique(pb.block_target):
            sel = np.nonzero((pb.block_target == t) & fin)[0]
            if sel.size:
                r[sel, k] = O.sample(pb.images[t], uv[sel], interp)[:, 0] - pb.host_intensity[pb.block_point[sel], k]
    ok &= np.isfinite(r).all(1)
    r[~ok] = 0.0
    return r, ok.astype(np.uint8)


def cost_at(pb, poses, rho, K, a):
    """The robust cost and the number of valid blocks at (poses, ρ, K), residuals only (residuals_at)."""
    r, valid = residuals_at(pb, poses, rho, K)
    cost_b, _ = GR.huber((r ** 2).sum(1), a)
    return float(np.where(valid == 1, cost_b, 0.0).sum()), int(valid.sum())


def step(H, g, pb, lam, fixed=()):
    """schur_step_intrinsics with the f-step split: (S, gS, δ_f, δposes (nf, 6), δK (nc, 8), δρ, model decrease)."""
    nf, nc = pb.n_frames, pb.intrinsics.shape[0]
    S, gS, df, dl, model = GR.schur_step_intrinsics(H, g, nf, nc, lam, fixed)
    return S, gS, df, df[:6 * nf].reshape(nf, 6), df[6 * nf:].reshape(nc, 8), dl, model


def apply_step(poses, rho, K, dp, dk, dl):
    return synth.se3_plus(poses, dp), rho + dl, K + dk


def lm(pb, K0, a, fixed=(), max_iterations=20, radius=1e4, function_tolerance=1e-6, min_relative_decrease=1e-3,
       parameter_tolerance=1e-8, gradient_tolerance=1e-10, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
       max_num_consecutive_invalid_steps=5):
    """gn_reference.lm (Ceres' trust-region loop with the LM strategy, in its order of tests) over (poses, K, ρ).
    Returns (poses, rho, K, initial cost, final cost, iterations, summary); summary also holds `rel` and `dcost`, the relative
    and the absolute cost decrease of every valid trial."""
    poses, rho, K = pb.poses.copy(), pb.rho.copy(), np.array(K0, np.float64, copy=True)
    nf, nc = pb.n_frames, pb.intrinsics.shape[0]
    nv = []
    H, g, cost = linearize(pb, poses, rho, K, a, fixed, n_valid=nv)
    valid_cur = nv[-1]
    cost0 = cost
    fx = set(int(x) for x in fixed)
    free = np.array([f not in fx and np.any(H[6 * f:6 * f + 6, :]) for f in range(nf)])
    cam_free = np.array([np.any(H[6 * nf + 8 * c:6 * nf + 8 * c + 8, :]) for c in range(nc)])
    has_blocks = np.zeros(pb.n_points, bool)
    has_blocks[pb.block_point] = True

    def gnorm(poses, g):
        tg = synth.se3_plus(poses, -g[:6 * nf].reshape(nf, 6))
        gp = np.abs(poses - tg)[free].max() if free.any() else 0.0
        gk = np.abs(g[6 * nf:6 * nf + 8 * nc].reshape(nc, 8))[cam_free].max() if cam_free.any() else 0.0
        gl = np.abs(g[6 * nf + 8 * nc:])[has_blocks].max() if has_blocks.any() else 0.0
        return max(gp, gk, gl)

    def xvec(poses, rho, K):
        return np.concatenate([poses[free].ravel(), K[cam_free].ravel(), rho[has_blocks]])

    factor = 2.0
    ok = bad = 0
    it = 0
    x_norm = -1.0
    invalid = 0
    invalid_candidates = 0
    history, rels, dcosts = [], [], []
    min_rho = np.inf  # over every candidate: compose (the twin b/ρ) is the photometric warp only while ρ > 0
    reason = "max_iterations"
    gnorm0 = gnorm(poses, g)
    if gnorm0 <= gradient_tolerance:
        reason = "gradient_tolerance"
    else:
        for it in range(1, max_iterations + 1):
            lam = 1.0 / radius
            _, _, _, dp, dk, dl, model = step(H, g, pb, lam, fixed)
            if not model > 0:
                invalid += 1
                if invalid >= max_num_consecutive_invalid_steps:
                    reason = "invalid_steps"
                    it -= 1
                    break
                radius /= factor
                factor *= 2
                bad += 1
                if radius <= min_trust_region_radius:
                    reason = "min_trust_region_radius"
                    break
                continue
            invalid = 0
            np_, nr, nk = apply_step(poses, rho, K, dp, dk, dl)
            min_rho = min(min_rho, float(nr[has_blocks].min()))
            nv = []
            H1, g1, cost_new = linearize(pb, np_, nr, nk, a, fixed, n_valid=nv)
            if nv[-1] < valid_cur:
                cost_new = np.finfo(np.float64).max
                invalid_candidates += 1
            st = np.linalg.norm(xvec(np_, nr, nk) - xvec(poses, rho, K))
            history.append([it, False, st, x_norm, None])
            if st <= parameter_tolerance * (x_norm + parameter_tolerance):
                reason = "parameter_tolerance"
                break
            if abs(cost - cost_new) <= function_tolerance * cost:
                reason = "function_tolerance"
                break
            rel = (cost - cost_new) / model
            rels.append(rel)
            dcosts.append(cost - cost_new)
            if rel > min_relative_decrease:
                poses, rho, K, cost, valid_cur = np_, nr, nk, cost_new, nv[-1]
                x_norm = float(np.linalg.norm(xvec(poses, rho, K)))
                radius = min(max_trust_region_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
                factor = 2.0
                ok += 1
                H, g = H1, g1
                history[-1][1] = True
                history[-1][4] = gnorm(poses, g)
                if it < max_iterations and history[-1][4] <= gradient_tolerance:
                    reason = "gradient_tolerance"
                    break
            else:
                radius /= factor
                factor *= 2
                bad += 1
                if radius <= min_trust_region_radius:
                    reason = "min_trust_region_radius"
                    break
    converged = reason not in ("max_iterations", "invalid_steps")
    return poses, rho, K, cost0, cost, it, {"successful_steps": ok, "unsuccessful_steps": bad, "converged": converged,
                                            "stop_reason": reason, "invalid_candidates": invalid_candidates,
                                            "history": history, "gnorm0": gnorm0, "rel": rels,
                                            "dcost": dcosts, "min_rho": min_rho}


# ---- the problems of the GPU tests --------------------------------------------------------------------------------
def pattern(P):
    """The patterns of tests/test_gpu_photometric_intrinsics.py's pattern(P)."""
    if P == 8:
        return synth.PATTERN8
    if P == 1:
        return np.zeros((1, 2), np.float32)
    return np.random.default_rng(P).integers(-3, 4, (P, 2)).astype(np.float32)


def _rig(model, frame_cam):
    k0 = np.array(synth.DEFAULT_INTRINSICS[model], np.float64)
    k0[:4] *= 376 / 752.0
    k1 = k0.copy()
    k1[:4] *= 1.02
    return dict(intrinsics=np.stack([k0, k1]), frame_cam=np.asarray(frame_cam, np.int32))


@functools.lru_cache(maxsize=None)
def problem(model=synth.PINHOLE, interp=0, P=8, cams="one", turned=False):
    """The base problem: 6 keyframes, 161 points, 376×240, 644 blocks (132 past a multiple of 256).
    cams: "one"; "two" (alternating over the keyframes); "idle" (camera 1 is keyframe 0's alone: a fixed keyframe that no
    block targets, so nothing observes camera 1).  turned: keyframe 3 turned 120° about its y axis (every block
    targeting it leaves the projection domain / the image)."""
    kw = {}
    if cams == "two":
        kw = _rig(model, np.arange(6) % 2)
    elif cams == "idle":
        kw = _rig(model, [1, 0, 0, 0, 0, 0])
    pb = synth.make_problem(n_frames=6, n_points=161, width=376, height=240, border=12, model=model,
                            pattern=pattern(P), **kw)
    pb.interp = interp
    if turned:
        poses = pb.poses.copy()
        h = np.deg2rad(120.0) / 2
        poses[3, :4] = synth.quat_mul(poses[3:4, :4], np.array([[0.0, np.sin(h), 0.0, np.cos(h)]]))[0]
        pb = dataclasses.replace(pb, poses=poses)
    return pb


def state(pb):
    K = PIR.perturbed_state(pb)
    if K.shape[0] == 2:  # the second camera's state perturbed the other way
        K[1] = PIR.perturbed_state(pb, -1.0)[1]
    return K


@functools.lru_cache(maxsize=None)
def reference(model=synth.PINHOLE, interp=0, P=8, cams="one", turned=False, huber=HUBER):
    """(records, valid, (H, g, cost), block weights) of problem(…) at its state: formed once, left unchanged."""
    pb = problem(model, interp, P, cams, turned)
    rec, valid = records(pb, pb.poses, pb.rho, state(pb))
    H, g, cost, w = system_from_records(pb, rec, valid, huber, FIXED)
    for x in (rec, valid, H, g, w):
        x.setflags(write=False)
    return rec, valid, (H, g, cost), w


@functools.lru_cache(maxsize=None)
def long_point_problem(seed=5):
    """A point of 70 blocks among 72 small keyframes: 72 keyframes of 96×64 on a slow trajectory (2 cm a frame, so the
    point stays in every image), 30 points of 4 blocks each, and the point hosted by keyframe 0 that lies nearest the
    image centre observed by keyframes 1 … 70 instead of 1 … 4: 116 + 70 = 186 blocks."""
    nf = 72
    pb = synth.make_problem(n_frames=nf, n_points=30, width=96, height=64, border=10, seed=seed,
                            poses_gt=synth.trajectory(nf, step=0.02, yaw=0.0005))
    own = np.nonzero(pb.point_host == 0)[0]
    p = int(own[np.argmin(np.abs(pb.u_ref[own] - np.array([48.0, 32.0])).sum(1))])
    keep = pb.block_point != p
    bp = np.concatenate([pb.block_point[keep], np.full(70, p, np.int32)])
    bt = np.concatenate([pb.block_target[keep], np.arange(1, 71, dtype=np.int32)])
    order = np.argsort(bp, kind="stable")
    return dataclasses.replace(pb, block_point=bp[order].astype(np.int32), block_target=bt[order].astype(np.int32))


@functools.lru_cache(maxsize=None)
def recovery_problem(seed=7, sigma=1e-3):
    """Images rendered at the true K (bicubic interpolation); keyframes 0 and 1 at their true poses, the others perturbed
    (σ 1e-3), the inverse distances by 1 %, and the state starts at K·(1 + σ·[1, −1, 0.5, −0.5]) on fx, fy, cx, cy."""
    pb = synth.make_problem(n_frames=6, n_points=161, width=376, height=240, border=12, seed=seed, pose_sigma=0.001,
                            rho_sigma=0.01)
    pb.interp = 1
    pb.poses[:2] = pb.poses_gt[:2]
    K = np.array(pb.intrinsics, np.float64, copy=True)
    K[:, :4] *= 1.0 + sigma * np.array([1.0, -1.0, 0.5, -0.5])
    return pb, K


LM_OPTIONS = dict(max_iterations=8, min_relative_decrease=0.9, initial_trust_region_radius=1.0)


def lm_case():
    """The LM case: the base problem at its state, with an acceptance threshold of 0.9 (as tests/test_gpu_gn.py's
    LM_CASES[4] raises it) and an initial trust-region radius of 1: the reference's relative decreases are 1.399 1.211
    1.191 1.311 1.586 0.742 1.372 1.186 — one rejection, every trial at least 0.15 from the threshold, every cost
    decrease above 8000 (the cost is 1.9e5), and every candidate keeps ρ > 0 (with Ceres' default radius of 1e4 the
    first candidates carry negative inverse distances, where compose's geometric twin is not the photometric warp).
    Returns (problem, state, solver options)."""
    pb = problem()
    return pb, state(pb), dict(LM_OPTIONS)


@functools.lru_cache(maxsize=None)
def lm_reference():
    pb, K, kw = lm_case()
    kw["radius"] = kw.pop("initial_trust_region_radius")
    return lm(pb, K, HUBER, FIXED, **kw)


@functools.lru_cache(maxsize=None)
def recovery_reference():
    pb, K = recovery_problem()
    return lm(pb, K, HUBER, FIXED, max_iterations=20)
