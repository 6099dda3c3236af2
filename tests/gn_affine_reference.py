"""Dense fp64 reference for the on-device Gauss-Newton at a constant affine brightness state
(pba_gn_set_solve_affine): the geometry solve of a photometric engine with pba_set_affine_brightness.

Built on photometric_affine_reference.compose: r_k = (I_t − b_t) − E·(I_h,k − b_h) at the state `ab`, and the geometric
columns J_host, J_target, J_rho of the oracle (∇I does not depend on (a, b)).  The first 14·P values of compose's
records are a plain [r | J_host | J_target | J_rho] record with the new r, so the system is gn_reference's own:
reduced_system_from_records on them, and — for the step, δρ, the model decrease and the LM loop — gn_reference.linearize
/ schur_step / lm over the same records.  The (a, b) blocks are constant, as under Ceres' SetParameterBlockConstant:
they have no columns.

(ii), at the end of the module: the brightness solve at fixed poses and ρ (pba_affine_*, pba_solve_affine) — the (a, b)
normal equations from compose's r and its two J_ab blocks with the Corrector weight, their damped step, model decrease
and the same trust-region loop over the free (a, b).

The problems are the brightness-changed images of photometric_affine_reference.brightness_case (the same gains and
offsets, seed 11) with poses and inverse distances perturbed; the affine state is parity_state.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import gn_reference as GR
import photometric_affine_reference as PAR
from helpers import synth

FIXED = (0, 1)
HUBER = 9.0
SEED = 11  # brightness_case's


def records(pb, ab, poses=None, rho=None):
    """([r | J_host | J_target | J_rho] (n_blocks, 14·P) float64, valid) at the affine state ab."""
    rec, valid, _ = PAR.compose(pb, ab, poses, rho)
    return rec[:, :14 * pb.pattern.shape[0]], valid


def linearize(pb, ab, poses, rho, a, fixed=(), n_valid=None, fp32=False):
    """gn_reference.linearize over records(…): H (N×N), g, cost with N = 6·n_frames + n_points.  fp32: the records
    rounded to fp32 and back first (what the engine's rows can hold at best)."""
    rec, valid = records(pb, ab, poses, rho)
    if fp32:
        rec = rec.astype(np.float32).astype(np.float64)
    if n_valid is not None:
        n_valid.append(int(valid.sum()))
    R = pb.R
    r, Jh, Jt, Jr = GR.O.split_record(rec, R)
    cost_b, w = GR.huber((r ** 2).sum(1), a)
    w = np.where(valid == 1, w, 0.0)
    cost = float(np.where(valid == 1, cost_b, 0.0).sum())
    nf = pb.n_frames
    N = 6 * nf + pb.n_points
    fixed = set(int(f) for f in fixed)
    H, g = np.zeros((N, N)), np.zeros(N)
    six = np.arange(6)
    for b in np.nonzero(w)[0]:
        p = pb.block_point[b]
        h, t = int(pb.point_host[p]), int(pb.block_target[b])
        cols, parts = [np.array([6 * nf + p])], [Jr[b][:, None]]
        if h not in fixed:
            cols.append(6 * h + six)
            parts.append(Jh[b])
        if t not in fixed:
            cols.append(6 * t + six)
            parts.append(Jt[b])
        idx, J = np.concatenate(cols), np.concatenate(parts, axis=1)
        H[np.ix_(idx, idx)] += w[b] * J.T @ J
        g[idx] += w[b] * J.T @ r[b]
    return H, g, cost


def reduced_system(pb, ab, a, lam, fixed=(), poses=None, rho=None):
    """(S, g_S, cost): gn_reference.reduced_system_from_records on the first 14·P columns."""
    rec, valid = records(pb, ab, poses, rho)
    return GR.reduced_system_from_records(pb, rec, valid, a, lam, fixed)


def cost_at(pb, ab, poses, rho, a):
    """(Σ ½ρ(‖r‖²) over the valid blocks, their number)."""
    rec, valid, _ = PAR.compose(pb, ab, poses, rho, want_jac=False)
    P = pb.pattern.shape[0]
    cost_b, _ = GR.huber((rec[:, :P] ** 2).sum(1), a)
    return float(cost_b[valid == 1].sum()), int(valid.sum())


def lm(pb, ab, a, fixed=(), **kw):
    """gn_reference.lm (Ceres' trust-region loop as that module restates it) with the linearisation above: the module's
    linearize is the only thing the loop knows of the residual, so it is swapped for the call."""
    plain, plain_step = GR.linearize, GR.schur_step
    costs, models = [], []

    def lin(pb_, poses, rho, a_, fixed_=(), n_valid=None):
        out = linearize(pb_, ab, poses, rho, a_, fixed_, n_valid)
        costs.append(out[2])
        return out

    def step(*args, **kwargs):
        out = plain_step(*args, **kwargs)
        models.append(out[4])
        return out

    GR.linearize, GR.schur_step = lin, step
    try:
        out = GR.lm(pb, a, fixed, **kw)
    finally:
        GR.linearize, GR.schur_step = plain, plain_step
    if kw.get("summary"):  # every trial's relative decrease (cost − candidate cost) / model decrease, in order
        hist = out[5]["history"]
        if len(hist) == len(models) and len(costs) >= len(models) + 1:  # (every step valid and evaluated)
            cur, rel = costs[0], []
            for (_, accepted, *_), m, c in zip(hist, models, costs[1:]):
                rel.append((cur - c) / m)
                cur = c if accepted else cur
            out[5]["rel"] = rel
    return out


# ---- the problems of the GPU tests --------------------------------------------------------------------------------
def pattern(P):
    """The patterns of tests/test_gpu_photometric_affine.py's pattern(P)."""
    if P == 8:
        return synth.PATTERN8
    return np.random.default_rng(P).integers(-3, 4, (P, 2)).astype(np.float32)


def brightness(n_frames, lo, hi, seed=SEED):
    """brightness_case's gains and offsets (frame 0 left alone; within ±10 % and ±8 grey levels, shrunk by halves until
    the images' range [lo, hi] does not clip)."""
    rng = np.random.default_rng(seed)
    dg, do = rng.uniform(-0.10, 0.10, n_frames), rng.uniform(-8.0, 8.0, n_frames)
    dg[0] = do[0] = 0.0
    s = 1.0
    while True:
        gain, offset = 1.0 + s * dg, s * do
        if (gain * lo + offset).min() >= 0.0 and (gain * hi + offset).max() <= 255.0:
            return gain, offset
        s *= 0.5
        assert s > 1e-3


@functools.lru_cache(maxsize=None)
def problem(model=synth.PINHOLE, interp=0, P=8, cams=1, turned=False, drop=0, changed=True):
    """6 keyframes, 161 points, 376×240, 644 blocks (4 past a multiple of 32) with brightness_case's brightness change
    on keyframes 1–5, poses and inverse distances perturbed (make_problem's defaults).  cams = 2: a second camera 2 %
    apart on the odd keyframes.  turned: keyframe 3 turned 180° about its y axis, so that it has no valid block (at 120°
    17 of its 161 blocks stay valid, with a zero column: the reference's own step is rounding noise there).  drop: that
    many blocks off the end (block counts that are no multiple of 32 either way).  changed = False: the images as
    rendered (the plain problem of the same geometry)."""
    kw = {}
    if cams == 2:
        k0 = np.array(synth.DEFAULT_INTRINSICS[model], np.float64)
        k0[:4] *= 376 / 752.0
        k1 = k0.copy()
        k1[:4] *= 1.02
        kw = dict(intrinsics=np.stack([k0, k1]), frame_cam=np.arange(6) % 2)
    pb = synth.make_problem(n_frames=6, n_points=161, width=376, height=240, border=12, model=model, pattern=pattern(P),
                            seed=SEED, **kw)
    pb.interp = interp
    if changed:
        gain, offset = brightness(pb.n_frames, float(pb.images.min()), float(pb.images.max()))
        pb = PAR.apply_brightness(pb, gain, offset)
    elif interp:  # (make_problem samples I_h bilinearly)
        pb = PAR.apply_brightness(pb, np.ones(pb.n_frames), np.zeros(pb.n_frames))
    if turned:
        poses = pb.poses.copy()
        h = np.deg2rad(180.0) / 2
        poses[3, :4] = synth.quat_mul(poses[3:4, :4], np.array([[0.0, np.sin(h), 0.0, np.cos(h)]]))[0]
        pb = dataclasses.replace(pb, poses=poses)
        pb.interp = interp
    if drop:
        pb = dataclasses.replace(pb, block_point=pb.block_point[:-drop], block_target=pb.block_target[:-drop])
        pb.interp = interp
    return pb


def state(pb):
    return PAR.parity_state(pb.n_frames)


@functools.lru_cache(maxsize=None)
def reference(model=synth.PINHOLE, interp=0, P=8, cams=1, turned=False, drop=0, huber=HUBER):
    """(valid, (H, g, cost), block weights) of problem(…) at state(…): formed once, left unchanged."""
    pb = problem(model, interp, P, cams, turned, drop)
    rec, valid = records(pb, state(pb))
    H, g, cost = linearize(pb, state(pb), pb.poses, pb.rho, huber, FIXED)
    _, w = GR.huber((rec[:, :pb.pattern.shape[0]] ** 2).sum(1), huber)
    for x in (valid, H, g, w):
        x.setflags(write=False)
    return valid, (H, g, cost), w


# The LM case: Ceres' defaults but a trust-region radius of 1 and few iterations (tests/gn_photometric_intrinsics_
# reference.py's lm_case: with the default radius of 1e4 the first candidates carry negative inverse distances).
LM_OPTIONS = dict(max_iterations=6, initial_trust_region_radius=1.0)


@functools.lru_cache(maxsize=None)
def lm_reference(min_relative_decrease=1e-3):
    pb = problem()
    kw = dict(LM_OPTIONS, min_relative_decrease=min_relative_decrease)
    kw["radius"] = kw.pop("initial_trust_region_radius")
    return lm(pb, state(pb), HUBER, FIXED, summary=True, **kw)


# ---- (ii) the brightness system at fixed poses and ρ ------------------------------------------------------------------
def linearize_ab(pb, ab, a, fixed=(), poses=None, rho=None):
    """H (2·n_frames square), g, cost of the (a, b) normal equations from compose's r and its two J_ab blocks with the
    Corrector weight w = ρ'(‖r‖²); unknowns [a_0 b_0 a_1 b_1 …].  Constant keyframes — `fixed`, and those without a valid
    block — get identity rows and a zero gradient.  Also returns the free mask (n_frames,)."""
    rec, valid, _ = PAR.compose(pb, ab, poses, rho)
    P, nf = pb.pattern.shape[0], pb.n_frames
    r, _, _, _, Jh, Jt = PAR.split(rec, P)
    cost_b, w = GR.huber((r ** 2).sum(1), a)
    w = np.where(valid == 1, w, 0.0)
    cost = float(cost_b[valid == 1].sum())
    host = pb.point_host[pb.block_point]
    H, g = np.zeros((2 * nf, 2 * nf)), np.zeros(2 * nf)
    for b in np.nonzero(w)[0]:
        h, t = int(host[b]), int(pb.block_target[b])
        idx = np.array([2 * h, 2 * h + 1, 2 * t, 2 * t + 1])
        J = np.concatenate([Jh[b], Jt[b]], 1)
        H[np.ix_(idx, idx)] += w[b] * J.T @ J
        g[idx] += w[b] * J.T @ r[b]
    free = np.array([f not in set(int(x) for x in fixed) and H[2 * f + 1, 2 * f + 1] > 0 for f in range(nf)])
    fx = np.repeat(~free, 2)
    H[fx, :] = 0.0
    H[:, fx] = 0.0
    H[fx, fx] = 1.0
    g[fx] = 0.0
    return H, g, cost, free


def step_ab(H, g, free, lam):
    """(δ (n_frames, 2), model decrease) of (H + λ·clamp(diag H, 1e-6, 1e32)) δ = −g over the free keyframes."""
    fx = np.repeat(~free, 2)
    D = np.where(fx, 0.0, np.clip(np.diag(H), 1e-6, 1e32))
    d = np.linalg.solve(H + lam * np.diag(D), -g)
    d[fx] = 0.0
    return d.reshape(-1, 2), 0.5 * (lam * float(d @ (D * d)) - float(g @ d))


def cost_ab(pb, ab, a, poses=None, rho=None):
    return cost_at(pb, ab, pb.poses if poses is None else poses, pb.rho if rho is None else rho, a)[0]


def lm_ab(pb, ab0, a, fixed=(), max_iterations=20, radius=1e4, function_tolerance=1e-6, min_relative_decrease=1e-3,
          parameter_tolerance=1e-8, gradient_tolerance=1e-10, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
          max_num_consecutive_invalid_steps=5, poses=None, rho=None):
    """gn_reference.lm's loop (trust_region_minimizer.cc, the same order of tests) over the free (a, b).  Returns (ab,
    initial cost, final cost, iterations, info) with info's decisions (accepted per trial) and relative decreases."""
    ab = np.array(ab0, np.float64).reshape(pb.n_frames, 2).copy()
    H, g, cost, free = linearize_ab(pb, ab, a, fixed, poses, rho)
    cost0, factor, x_norm, invalid, it = cost, 2.0, -1.0, 0, 0
    info = {"decisions": [], "rel": [], "costs": [cost], "successful_steps": 0, "unsuccessful_steps": 0,
            "stop_reason": "max_iterations"}
    fm = np.repeat(free, 2)
    if np.abs(g[fm]).max(initial=0.0) <= gradient_tolerance:
        info["stop_reason"] = "gradient_tolerance"
    else:
        for it in range(1, max_iterations + 1):
            d, model = step_ab(H, g, free, 1.0 / radius)
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
            cand = cost_ab(pb, ab + d, a, poses, rho)
            step = float(np.linalg.norm(d))
            if step <= parameter_tolerance * (x_norm + parameter_tolerance):
                info["stop_reason"] = "parameter_tolerance"
                break
            if abs(cost - cand) <= function_tolerance * cost:
                info["stop_reason"] = "function_tolerance"
                break
            rel = (cost - cand) / model
            info["rel"].append(rel)
            info["decisions"].append(bool(rel > min_relative_decrease))
            if rel > min_relative_decrease:
                ab = ab + d
                H, g, cost, free = linearize_ab(pb, ab, a, fixed, poses, rho)
                x_norm = float(np.linalg.norm(ab[free]))
                radius = min(max_trust_region_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
                factor = 2.0
                info["successful_steps"] += 1
                info["costs"].append(cost)
                if it < max_iterations and np.abs(g[fm]).max(initial=0.0) <= gradient_tolerance:
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
    return ab, cost0, cost, it, info
