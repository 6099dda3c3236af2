"""Dense fp64 reference for the joint solve of poses, inverse distances and affine brightness (pba_joint_*,
pba_solve_joint): photometric engines with pba_set_affine_brightness.

Built on photometric_affine_reference.compose's 18·P records [r | J_host | J_target | J_rho | J_ab_host | J_ab_target],
in the style of gn_affine_reference.py.  Unknowns: 8 per keyframe, [δpose (6, right update T·exp δ) | δa δb], then one
δρ per point: N = 8·n_frames + n_points.
  * linearize: H = Σ w JᵀJ, g = Σ w Jᵀr with the Corrector weight w = ρ'(‖r‖²) (gn_reference.huber), cost Σ ½ρ(‖r‖²);
  * schur_step: Ceres' LM damping (H + λ·clamp(diag H, 1e-6, 1e32)) δ = −g, the ρ eliminated into the 8·n_frames
    reduced system, δρ by back-substitution, the model decrease ½(λ δᵀDδ − gᵀδ) over the free unknowns.  Constants get
    identity rows, a zero gradient and a zero step; the two halves of a keyframe are independent: its pose is constant
    when it is in `fixed` or has no valid block, its (a, b) when it is in `fixed_ab`, has no valid block or a
    non-finite a or b;
  * lm: gn_reference.lm's loop (trust_region_minimizer.cc, the same order of tests) with norms over the free poses
    (ambient [q | t]), the ρ of points with blocks and the free (a, b).

The problems are gn_affine_reference.problem's, at gn_affine_reference.state.
"""
from __future__ import annotations

import functools

import numpy as np

import gn_affine_reference as GA
import gn_reference as GR
import photometric_affine_reference as PAR
from helpers import synth

FIXED = (0, 1)     # constant poses
FIXED_AB = (0,)    # constant (a, b)
HUBER = GA.HUBER


def linearize(pb, ab, poses, rho, a, n_valid=None, fp32=False):
    """H (N×N), g, cost, N = 8·n_frames + n_points; nothing constant yet (schur_step).  n_valid (a list): the number
    of valid blocks is appended.  fp32: the records rounded to fp32 and back first."""
    rec, valid, _ = PAR.compose(pb, ab, poses, rho)
    if fp32:
        rec = rec.astype(np.float32).astype(np.float64)
    if n_valid is not None:
        n_valid.append(int(valid.sum()))
    P, nf = pb.pattern.shape[0], pb.n_frames
    r, Jh, Jt, Jr, Jabh, Jabt = PAR.split(rec, P)
    cost_b, w = GR.huber((r ** 2).sum(1), a)
    w = np.where(valid == 1, w, 0.0)
    cost = float(np.where(valid == 1, cost_b, 0.0).sum())
    N = 8 * nf + pb.n_points
    H, g = np.zeros((N, N)), np.zeros(N)
    eight = np.arange(8)
    for b in np.nonzero(w)[0]:
        p = pb.block_point[b]
        h, t = int(pb.point_host[p]), int(pb.block_target[b])
        idx = np.concatenate([8 * h + eight, 8 * t + eight, [8 * nf + p]])
        J = np.concatenate([Jh[b], Jabh[b], Jt[b], Jabt[b], Jr[b][:, None]], axis=1)
        H[np.ix_(idx, idx)] += w[b] * J.T @ J
        g[idx] += w[b] * J.T @ r[b]
    return H, g, cost


def constants(H, ab, nf, fixed=(), fixed_ab=()):
    """Boolean mask (8·n_frames,) of the constant keyframe unknowns."""
    ab = np.asarray(ab, np.float64).reshape(nf, 2)
    fp, fa = set(int(f) for f in fixed), set(int(f) for f in fixed_ab)
    fx = np.zeros(8 * nf, bool)
    for i in range(nf):
        seen = bool(np.any(H[8 * i:8 * i + 8, :]))  # (the b column of a keyframe with a valid block is never zero)
        fx[8 * i:8 * i + 6] = i in fp or not seen
        fx[8 * i + 6:8 * i + 8] = i in fa or not seen or not np.isfinite(ab[i]).all()
    return fx


def schur_step(H, g, ab, nf, lam, fixed=(), fixed_ab=()):
    """(S, gS, δ_keyframes (nf, 8), δρ, model decrease, constant mask) of (H + λD)δ = −g with the ρ eliminated."""
    K = 8 * nf
    D = np.clip(np.diag(H), 1e-6, 1e32)
    fx = constants(H, ab, nf, fixed, fixed_ab)
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
    return S, gS, dk.reshape(nf, 8), dl, model, fx


def apply_step(poses, rho, ab, dk, dl):
    ab = np.asarray(ab, np.float64).reshape(-1, 2)
    return synth.se3_plus(poses, dk[:, :6]), rho + dl, ab + dk[:, 6:]


def cost_at(pb, ab, poses, rho, a):
    """(Σ ½ρ(‖r‖²) over the valid blocks, their number)."""
    return GA.cost_at(pb, ab, poses, rho, a)


def candidate_cost(pb, ab, poses, rho, a):
    """(cost, valid blocks) at a candidate.  compose goes through the geometric twin b/ρ, the same point only while
    ρ > 0; where a candidate carries ρ ≤ 0 the residuals come from the warp with ρ itself
    (gn_photometric_intrinsics_reference.residuals_at), as the engine's do."""
    seen = np.unique(pb.block_point)
    if (np.asarray(rho)[seen] > 0).all():
        return cost_at(pb, ab, poses, rho, a)
    import gn_photometric_intrinsics_reference as GPI
    ab = np.asarray(ab, np.float64).reshape(pb.n_frames, 2)
    r0, valid = GPI.residuals_at(pb, poses, rho, pb.intrinsics)
    host = pb.point_host[pb.block_point]
    Ih = pb.host_intensity[pb.block_point].astype(np.float64)
    with np.errstate(all="ignore"):
        E = np.exp(ab[pb.block_target, 0] - ab[host, 0])[:, None]
        r = ((r0 + Ih) - ab[pb.block_target, 1][:, None]) - E * (Ih - ab[host, 1][:, None])
    ok = (valid == 1) & np.isfinite(r).all(1)
    cost_b, _ = GR.huber((np.where(ok[:, None], r, 0.0) ** 2).sum(1), a)
    return float(cost_b[ok].sum()), int(ok.sum())


def parts(nf):
    """Index sets of the 8·n_frames keyframe unknowns: pose, a, b."""
    i = np.arange(8 * nf)
    return {"pose": i[i % 8 < 6], "a": i[i % 8 == 6], "b": i[i % 8 == 7]}


def lm(pb, ab0, a, fixed=(), fixed_ab=(), max_iterations=20, radius=1e4, function_tolerance=1e-6,
       min_relative_decrease=1e-3, parameter_tolerance=1e-8, gradient_tolerance=1e-10, max_trust_region_radius=1e16,
       min_trust_region_radius=1e-32, max_num_consecutive_invalid_steps=5):
    """gn_reference.lm's loop over poses, ρ and (a, b).  Returns (poses, ρ, ab, initial cost, final cost, iterations,
    info): info's decisions (accepted per evaluated trial), relative decreases, candidate costs of every evaluated trial,
    valid blocks of every candidate, min ρ of every candidate."""
    poses, rho = pb.poses.copy(), pb.rho.copy()
    nf = pb.n_frames
    ab = np.array(ab0, np.float64).reshape(nf, 2).copy()
    nv = []
    H, g, cost = linearize(pb, ab, poses, rho, a, nv)
    valid_cur, cost0 = nv[-1], cost
    fx = constants(H, ab, nf, fixed, fixed_ab).reshape(nf, 8)
    free_p, free_ab = ~fx[:, 0], ~fx[:, 6]
    has_blocks = np.zeros(pb.n_points, bool)
    has_blocks[pb.block_point] = True

    def gnorm(poses, g):
        gk = g[:8 * nf].reshape(nf, 8)
        tg = synth.se3_plus(poses, -gk[:, :6])
        return max(np.abs(poses - tg)[free_p].max(initial=0.0), np.abs(gk[:, 6:])[free_ab].max(initial=0.0),
                   np.abs(g[8 * nf:])[has_blocks].max(initial=0.0))

    def xvec(poses, rho, ab):
        return np.concatenate([poses[free_p].ravel(), rho[has_blocks], ab[free_ab].ravel()])

    info = {"decisions": [], "rel": [], "trial_costs": [], "valid": [], "min_rho": [], "successful_steps": 0,
            "unsuccessful_steps": 0, "invalid_candidates": 0, "stop_reason": "max_iterations", "n_valid0": valid_cur}
    factor, x_norm, invalid, it = 2.0, -1.0, 0, 0
    if gnorm(poses, g) <= gradient_tolerance:
        info["stop_reason"] = "gradient_tolerance"
    else:
        for it in range(1, max_iterations + 1):
            _, _, dk, dl, model, _ = schur_step(H, g, ab, nf, 1.0 / radius, fixed, fixed_ab)
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
            np_, nr, nab = apply_step(poses, rho, ab, dk, dl)
            nv = []
            H1, g1, cost_new = linearize(pb, nab, np_, nr, a, nv)
            info["trial_costs"].append(cost_new)
            info["valid"].append(nv[-1])
            info["min_rho"].append(float(nr.min()))
            if nv[-1] < valid_cur:
                cost_new = np.finfo(np.float64).max
                info["invalid_candidates"] += 1
            step = np.linalg.norm(xvec(np_, nr, nab) - xvec(poses, rho, ab))
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
                poses, rho, ab, cost, valid_cur = np_, nr, nab, cost_new, nv[-1]
                x_norm = float(np.linalg.norm(xvec(poses, rho, ab)))
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
    return poses, rho, ab, cost0, cost, it, info


# ---- the problems of the GPU tests --------------------------------------------------------------------------------
problem, state = GA.problem, GA.state

# system-and-step cases of tests/test_gpu_gn_joint.py (keyword arguments of problem, plus huber)
KB4 = synth.KB4
CASES = [
    dict(), dict(interp=1), dict(P=5), dict(P=12, interp=1), dict(P=21), dict(P=32, interp=1),
    dict(model=KB4, interp=1), dict(model=KB4, P=21), dict(P=12, cams=2), dict(cams=2), dict(drop=7),
    dict(turned=True), dict(turned=True, P=21), dict(huber=60.0), dict(huber=0.0), dict(huber=60.0, P=32),
]


@functools.lru_cache(maxsize=None)
def reference(model=synth.PINHOLE, interp=0, P=8, cams=1, turned=False, drop=0, huber=HUBER):
    """(H, g, cost, valid blocks) of problem(…) at state(…): formed once, left unchanged."""
    pb = problem(model, interp, P, cams, turned, drop)
    nv = []
    H, g, cost = linearize(pb, state(pb), pb.poses, pb.rho, huber, nv)
    H.setflags(write=False)
    g.setflags(write=False)
    return H, g, cost, nv[0]


# The LM cases: from (a, b) = 0 at Ceres' default options, 8 iterations; and a run with a rejection
# (min_relative_decrease 1.3: trials 1 and 2 accepted at 1.485 and 1.737, trial 3 rejected at 1.152).
LM_ITERATIONS = 8
LM_REJECT = dict(max_iterations=4, min_relative_decrease=1.3)


@functools.lru_cache(maxsize=None)
def lm_reference(max_iterations=LM_ITERATIONS, min_relative_decrease=1e-3, radius=1e4):
    pb = problem()
    return lm(pb, np.zeros((pb.n_frames, 2)), HUBER, FIXED, FIXED_AB, max_iterations=max_iterations,
              min_relative_decrease=min_relative_decrease, radius=radius)
