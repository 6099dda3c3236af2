"""Dense fp64 reference for the joint solve of poses, inverse distances, affine brightness and intrinsics
(pba_joint_* and pba_solve_joint under pba_joint_set_solve_intrinsics): photometric engines with both
pba_set_optimize_intrinsics and pba_set_affine_brightness.

Built on photometric_affine_intrinsics_reference.compose's 26·P records [r | J_host | J_target | J_rho | J_intr |
J_ab_host | J_ab_target], in the style of gn_joint_reference.py.  Unknowns: 8 per keyframe, [δpose (6, right update
T·exp δ) | δa δb], then 8 per camera, δk with respect to the level-0 intrinsics state (a block's J_intr sits on the
camera of its target), then one δρ per point: N = 8·n_frames + 8·n_cams + n_points.
  * linearize: H = Σ w JᵀJ, g = Σ w Jᵀr with the Corrector weight (gn_reference.huber), cost Σ ½ρ(‖r‖²).  intr_scale =
    2^−level scales J_intr's columns 0–3: at pyramid level l the records are those of the level's problem at the
    level's image of the state, whose first four entries are the level-0 state's over 2^l;
  * schur_step: gn_joint_reference.schur_step's rules over the 8·(n_frames + n_cams) reduced system.  Constants: the
    keyframes' two halves as there; a camera that no valid block targets.  A parameter the camera model does not use is
    not a constant: its row and column are zero, its pivot λ·1e-6 (Ceres' clamp), its gradient and step zero;
  * lm: gn_joint_reference.lm's loop with the intrinsics of the cameras that have a valid block in the three norms.

The problems are gn_affine_reference.problem's at gn_affine_reference.state, with the intrinsics state of
tests/test_gpu_photometric_affine_intrinsics.py's k_state, and an unseen-camera variant (problem(unseen=True)).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import gn_affine_reference as GA
import gn_joint_reference as GJ
import gn_reference as GR
import photometric_affine_intrinsics_reference as PAIR
import photometric_affine_reference as PAR
import photometric_intrinsics_reference as PIR
from helpers import synth

FIXED, FIXED_AB, HUBER = GJ.FIXED, GJ.FIXED_AB, GJ.HUBER
N_USED = PIR.N_USED


def linearize(pb, K, ab, poses, rho, a, n_valid=None, fp32=False, intr_scale=1.0):
    """H (N×N), g, cost at the intrinsics state K (the active level's image) and the affine state ab; nothing constant
    yet (schur_step).  n_valid (a list): the number of valid blocks is appended.  fp32: the records rounded to fp32
    and back first."""
    rec, valid, _ = PAIR.compose(pb, K, ab, poses, rho)
    if fp32:
        rec = rec.astype(np.float32).astype(np.float64)
    if n_valid is not None:
        n_valid.append(int(valid.sum()))
    P, nf, nc = pb.pattern.shape[0], pb.n_frames, pb.intrinsics.shape[0]
    r, Jh, Jt, Jr, Ji, Jabh, Jabt = PAIR.split(rec, P)
    Ji = Ji * np.array([intr_scale] * 4 + [1.0] * 4)
    cost_b, w = GR.huber((r ** 2).sum(1), a)
    w = np.where(valid == 1, w, 0.0)
    cost = float(np.where(valid == 1, cost_b, 0.0).sum())
    N = 8 * (nf + nc) + pb.n_points
    H, g = np.zeros((N, N)), np.zeros(N)
    eight = np.arange(8)
    for b in np.nonzero(w)[0]:
        p = pb.block_point[b]
        h, t = int(pb.point_host[p]), int(pb.block_target[b])
        c = int(pb.frame_cam[t])
        idx = np.concatenate([8 * h + eight, 8 * t + eight, 8 * (nf + c) + eight, [8 * (nf + nc) + p]])
        J = np.concatenate([Jh[b], Jabh[b], Jt[b], Jabt[b], Ji[b], Jr[b][:, None]], axis=1)
        H[np.ix_(idx, idx)] += w[b] * J.T @ J
        g[idx] += w[b] * J.T @ r[b]
    return H, g, cost


def constants(H, ab, nf, nc, fixed=(), fixed_ab=()):
    """Boolean mask (8·(n_frames + n_cams),) of the constant unknowns: gn_joint_reference.constants for the keyframes,
    and all 8 of a camera without a valid block (a camera with one has a non-zero fx row in every model)."""
    fx = np.zeros(8 * (nf + nc), bool)
    fx[:8 * nf] = GJ.constants(H, ab, nf, fixed, fixed_ab)
    for c in range(nc):
        rows = slice(8 * (nf + c), 8 * (nf + c) + 8)
        fx[rows] = not np.any(H[rows, :])
    return fx


def schur_step(H, g, ab, nf, nc, lam, fixed=(), fixed_ab=()):
    """(S, gS, δ_keyframes (nf, 8), δk (nc, 8), δρ, model decrease, constant mask) of (H + λD)δ = −g with the ρ
    eliminated; S is 8·(nf + nc) square, keyframes first."""
    K = 8 * (nf + nc)
    D = np.clip(np.diag(H), 1e-6, 1e32)
    fx = constants(H, ab, nf, nc, fixed, fixed_ab)
    Ha = H + lam * np.diag(D)
    A, B, C = Ha[:K, :K].copy(), Ha[:K, K:].copy(), np.diag(Ha[K:, K:]).copy()
    gk, gl = g[:K].copy(), g[K:].copy()
    A[fx, :] = 0
    A[:, fx] = 0
    A[fx, fx] = 1.0
    B[fx, :] = 0
    gk[fx] = 0
    Ci = np.where(np.diag(H)[K:] > 0, 1.0 / C, 0.0)  # (a point without a valid block: no step)
    S = A - (B * Ci) @ B.T
    gS = gk - B @ (Ci * gl)
    S[fx, :] = 0
    S[:, fx] = 0
    S[fx, fx] = 1.0
    gS[fx] = 0
    dk = np.linalg.solve(S, -gS)
    dk[fx] = 0.0
    dl = -(gl + B.T @ dk) * Ci
    delta = np.concatenate([dk, dl])
    Dm = D.copy()
    Dm[:K][fx] = 0
    Dm[K:][Ci == 0] = 0
    model = 0.5 * (lam * float(delta @ (Dm * delta)) - float(np.concatenate([gk, gl]) @ delta))
    return S, gS, dk[:8 * nf].reshape(nf, 8), dk[8 * nf:].reshape(nc, 8), dl, model, fx


def apply_step(poses, rho, ab, K0, dk, dc, dl):
    """The candidate (poses, ρ, (a, b), level-0 intrinsics state)."""
    ab = np.asarray(ab, np.float64).reshape(-1, 2)
    return synth.se3_plus(poses, dk[:, :6]), rho + dl, ab + dk[:, 6:], np.asarray(K0, np.float64) + dc


def cost_at(pb, K, ab, poses, rho, a):
    """(Σ ½ρ(‖r‖²) over the valid blocks, their number)."""
    rec, valid, _ = PAIR.compose(pb, K, ab, poses, rho, want_jac=False)
    P = pb.pattern.shape[0]
    cost_b, _ = GR.huber((rec[:, :P] ** 2).sum(1), a)
    return float(cost_b[valid == 1].sum()), int(valid.sum())


def candidate_cost(pb, K, ab, poses, rho, a):
    """(cost, valid blocks) at a candidate.  compose goes through the geometric twin b/ρ, the same point only while
    ρ > 0; where a candidate carries ρ ≤ 0 the residuals come from the warp with ρ itself
    (gn_photometric_intrinsics_reference.residuals_at at the state K), as the engine's do."""
    seen = np.unique(pb.block_point)
    if (np.asarray(rho)[seen] > 0).all():
        return cost_at(pb, K, ab, poses, rho, a)
    import gn_photometric_intrinsics_reference as GPI
    ab = np.asarray(ab, np.float64).reshape(pb.n_frames, 2)
    r0, valid = GPI.residuals_at(pb, poses, rho, K)
    host = pb.point_host[pb.block_point]
    Ih = pb.host_intensity[pb.block_point].astype(np.float64)
    with np.errstate(all="ignore"):
        E = np.exp(ab[pb.block_target, 0] - ab[host, 0])[:, None]
        r = ((r0 + Ih) - ab[pb.block_target, 1][:, None]) - E * (Ih - ab[host, 1][:, None])
    ok = (valid == 1) & np.isfinite(r).all(1)
    cost_b, _ = GR.huber((np.where(ok[:, None], r, 0.0) ** 2).sum(1), a)
    return float(cost_b[ok].sum()), int(ok.sum())


def parts(nf, nc, model):
    """Index sets of the 8·(n_frames + n_cams) unknowns: pose, a, b, intr (the parameters the model uses) and unused."""
    i = np.arange(8 * nf)
    c = 8 * nf + np.arange(8 * nc)
    used = np.arange(8 * nc) % 8 < N_USED[model]
    return {"pose": i[i % 8 < 6], "a": i[i % 8 == 6], "b": i[i % 8 == 7], "intr": c[used], "unused": c[~used]}


def lm(pb, K0, ab0, a, fixed=(), fixed_ab=(), max_iterations=20, radius=1e4, function_tolerance=1e-6,
       min_relative_decrease=1e-3, parameter_tolerance=1e-8, gradient_tolerance=1e-10, max_trust_region_radius=1e16,
       min_trust_region_radius=1e-32, max_num_consecutive_invalid_steps=5, fp32=False):
    """gn_joint_reference.lm's loop over poses, ρ, (a, b) and the intrinsics.  Returns (poses, ρ, ab, K, initial cost,
    final cost, iterations, info) with gn_joint_reference.lm's info."""
    poses, rho = pb.poses.copy(), pb.rho.copy()
    nf, nc = pb.n_frames, pb.intrinsics.shape[0]
    ab = np.array(ab0, np.float64).reshape(nf, 2).copy()
    K = np.array(K0, np.float64).reshape(nc, 8).copy()
    nv = []
    H, g, cost = linearize(pb, K, ab, poses, rho, a, nv, fp32)
    valid_cur, cost0 = nv[-1], cost
    fx = constants(H, ab, nf, nc, fixed, fixed_ab)
    fk = fx[:8 * nf].reshape(nf, 8)
    free_p, free_ab, free_c = ~fk[:, 0], ~fk[:, 6], ~fx[8 * nf:].reshape(nc, 8)[:, 0]
    has_blocks = np.zeros(pb.n_points, bool)
    has_blocks[pb.block_point] = True

    def gnorm(poses, g):
        gk = g[:8 * nf].reshape(nf, 8)
        gc = g[8 * nf:8 * (nf + nc)].reshape(nc, 8)
        tg = synth.se3_plus(poses, -gk[:, :6])
        return max(np.abs(poses - tg)[free_p].max(initial=0.0), np.abs(gk[:, 6:])[free_ab].max(initial=0.0),
                   np.abs(gc)[free_c].max(initial=0.0), np.abs(g[8 * (nf + nc):])[has_blocks].max(initial=0.0))

    def xvec(poses, rho, ab, K):
        return np.concatenate([poses[free_p].ravel(), rho[has_blocks], ab[free_ab].ravel(), K[free_c].ravel()])

    info = {"decisions": [], "rel": [], "trial_costs": [], "valid": [], "min_rho": [], "successful_steps": 0,
            "unsuccessful_steps": 0, "invalid_candidates": 0, "stop_reason": "max_iterations", "n_valid0": valid_cur}
    factor, x_norm, invalid, it = 2.0, -1.0, 0, 0
    if gnorm(poses, g) <= gradient_tolerance:
        info["stop_reason"] = "gradient_tolerance"
    else:
        for it in range(1, max_iterations + 1):
            _, _, dk, dc, dl, model, _ = schur_step(H, g, ab, nf, nc, 1.0 / radius, fixed, fixed_ab)
            if not model > 0:
                invalid += 1
                if invalid >= max_num_consecutive_invalid_steps:
                    info["stop_reason"] = "invalid_steps"
                    it -= 1
                    break
                radius /= factor
                factor *= 2
                info["unsuccessful_steps"] += 1
                if radius <= min_trust_region_radius:
                    info["stop_reason"] = "min_trust_region_radius"
                    break
                continue
            invalid = 0
            np_, nr, nab, nK = apply_step(poses, rho, ab, K, dk, dc, dl)
            nv = []
            H1, g1, cost_new = linearize(pb, nK, nab, np_, nr, a, nv, fp32)
            info["trial_costs"].append(cost_new)
            info["valid"].append(nv[-1])
            info["min_rho"].append(float(nr.min()))
            if nv[-1] < valid_cur:
                cost_new = np.finfo(np.float64).max
                info["invalid_candidates"] += 1
            step = np.linalg.norm(xvec(np_, nr, nab, nK) - xvec(poses, rho, ab, K))
            if step <= parameter_tolerance * (x_norm + parameter_tolerance):
                info["stop_reason"] = "parameter_tolerance"
                break
            if abs(cost - cost_new) <= function_tolerance * cost:
                info["stop_reason"] = "function_tolerance"
                break
            rel = (cost - cost_new) / model
            info["rel"].append(rel)
            info["decisions"].append(bool(rel > min_relative_decrease))
            if rel > min_relative_decrease:
                poses, rho, ab, K, cost, valid_cur = np_, nr, nab, nK, cost_new, nv[-1]
                x_norm = float(np.linalg.norm(xvec(poses, rho, ab, K)))
                radius = min(max_trust_region_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
                factor = 2.0
                info["successful_steps"] += 1
                H, g = H1, g1
                if it < max_iterations and gnorm(poses, g) <= gradient_tolerance:
                    info["stop_reason"] = "gradient_tolerance"
                    break
            else:
                radius /= factor
                factor *= 2
                info["unsuccessful_steps"] += 1
                if radius <= min_trust_region_radius:
                    info["stop_reason"] = "min_trust_region_radius"
                    break
    info["converged"] = info["stop_reason"] not in ("max_iterations", "invalid_steps")
    return poses, rho, ab, K, cost0, cost, it, info


# ---- the problems of the GPU tests --------------------------------------------------------------------------------
state = GA.state
UNSEEN_FRAME_CAM = (0, 0, 0, 1, 0, 0)


@functools.lru_cache(maxsize=None)
def problem(model=synth.PINHOLE, interp=0, P=8, cams=1, turned=False, drop=0, unseen=False):
    """gn_affine_reference.problem(…).  unseen: its two cameras with frame_cam = [0, 0, 0, 1, 0, 0] (the images rendered
    so) and keyframe 3 turned away, so that camera 1 has no valid block."""
    if not unseen:
        return GA.problem(model, interp, P, cams, turned, drop)
    assert cams == 1 and not turned and not drop
    k0 = np.array(synth.DEFAULT_INTRINSICS[model], np.float64)
    k0[:4] *= 376 / 752.0
    k1 = k0.copy()
    k1[:4] *= 1.02
    pb = synth.make_problem(n_frames=6, n_points=161, width=376, height=240, border=12, model=model,
                            pattern=GA.pattern(P), seed=GA.SEED, intrinsics=np.stack([k0, k1]),
                            frame_cam=np.array(UNSEEN_FRAME_CAM))
    pb.interp = interp
    gain, offset = GA.brightness(pb.n_frames, float(pb.images.min()), float(pb.images.max()))
    pb = PAR.apply_brightness(pb, gain, offset)
    poses = pb.poses.copy()
    h = np.deg2rad(180.0) / 2
    poses[3, :4] = synth.quat_mul(poses[3:4, :4], np.array([[0.0, np.sin(h), 0.0, np.cos(h)]]))[0]
    pb = dataclasses.replace(pb, poses=poses)
    pb.interp = interp
    return pb


def k_state(pb):
    """tests/test_gpu_photometric_affine_intrinsics.py's k_state: perturbed_state, a second camera's the other way."""
    K = PIR.perturbed_state(pb)
    if K.shape[0] == 2:
        K[1] = PIR.perturbed_state(pb, -1.0)[1]
    return K


# system-and-step cases of tests/test_gpu_gn_joint_intrinsics.py (keyword arguments of problem, plus huber), each the
# smallest that reaches another path: P = 5 one pass with idle lanes, 8 one full pass, 12 a partial second, 21 and 32
# three and four; KB4 all 8 intrinsics, double sphere and EUCM 6, pinhole 4 with 4 unused; both interpolators; two
# cameras; a block count with another remainder; a keyframe and a camera without a valid block; Huber off, 9, 60
KB4, DS, EUCM = synth.KB4, synth.DOUBLE_SPHERE, synth.EUCM
CASES = [
    dict(P=5), dict(), dict(P=12, interp=1), dict(P=21), dict(P=32, interp=1), dict(model=KB4, interp=1),
    dict(model=DS), dict(model=EUCM, P=12), dict(cams=2), dict(drop=7), dict(turned=True), dict(unseen=True),
    dict(huber=0.0), dict(huber=60.0),
]


@functools.lru_cache(maxsize=None)
def reference(model=synth.PINHOLE, interp=0, P=8, cams=1, turned=False, drop=0, unseen=False, huber=HUBER):
    """(H, g, cost, valid blocks) of problem(…) at state(…) and k_state(…): formed once, left unchanged."""
    pb = problem(model, interp, P, cams, turned, drop, unseen)
    nv = []
    H, g, cost = linearize(pb, k_state(pb), state(pb), pb.poses, pb.rho, huber, nv)
    H.setflags(write=False)
    g.setflags(write=False)
    return H, g, cost, nv[0]


# The LM cases, from (a, b) = 0 and k_state at Ceres' default options: one camera, 8 iterations, every trial accepted;
# two cameras, 10 iterations, trials 5–7 rejected.
LM_CASES = {"accepts": dict(cams=1, max_iterations=8), "rejects": dict(cams=2, max_iterations=10)}


@functools.lru_cache(maxsize=None)
def lm_reference(name, fp32=False):
    kw = LM_CASES[name]
    pb = problem(cams=kw["cams"])
    return lm(pb, k_state(pb), np.zeros((pb.n_frames, 2)), HUBER, FIXED, FIXED_AB, max_iterations=kw["max_iterations"],
              fp32=fp32)
