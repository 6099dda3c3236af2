"""Two-way and loop-closed keyframe graphs for the on-device solves (tests/test_gpu_graphs.py; tests/test_graph_problems.py
asserts on the CPU the conditions under which that file's bounds mean something).

synth.make_problem's blocks target host+1 … host+4, so the host index of every pair lies below its target's and a row of
the keyframe systems is at most 5 keyframes wide.  Here the keyframes stand on a closed trajectory — keyframe k at
(0.3·cos θ_k, 0.3·sin θ_k, 0), θ_k = 2πk/n, turned by so3_exp((0, 0.002·sin θ_k, 0)) — so that any two of them see each
other's points, and the blocks are rewired by point index p (h the point's host; targets outside [0, n) are dropped):

    p % 3 = 0: targets h+1 … h+4        p % 3 = 1: targets h−1 … h−4        p % 3 = 2: targets h−2, h−1, h+1, h+2

`closures` (host, target): every point hosted by `host` gains a block targeting `target`.  `idle`: keyframes from which
every block that hosts or targets them is removed.  Geometric problems get their observations regenerated from the true
poses and inverse distances with make_problem's noise; changed = True applies gn_affine_reference's brightness change.

The named problems:
    band37          37 keyframes,  370 points: a two-way band of half-width 4
    closed100      100 keyframes, 1000 points, closures (0→99) (0→31) (0→32) (0→64) (95→1) (10→60) (61→12): rows of the
                   brightness system 63/64, 65/66, 129/130 and 199/200 scalars wide
    closed100_idle the same with keyframe 50 idle
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import gn_affine_reference as R
import gn_reference as GR
import photometric_affine_reference as PAR
from helpers import synth

FIXED = (0, 1)
CLOSURES = ((0, 99), (0, 31), (0, 32), (0, 64), (95, 1), (10, 60), (61, 12))
NAMED = {"band37": dict(n_frames=37, n_points=370),
         "closed100": dict(n_frames=100, n_points=1000, closures=CLOSURES),
         "closed100_idle": dict(n_frames=100, n_points=1000, closures=CLOSURES, idle=(50,))}
SEED = 23
OBS_SIGMA = 0.5  # make_problem's


def closed_trajectory(n):
    th = 2.0 * np.pi * np.arange(n) / n
    z = np.zeros(n)
    q = synth.so3_exp(np.stack([z, 0.002 * np.sin(th), z], -1))
    return np.concatenate([q, np.stack([0.3 * np.cos(th), 0.3 * np.sin(th), z], -1)], -1)


def _observations(pb, block_point, block_target, rng):
    """make_problem's u_obs for the given blocks: the true projection plus N(0, OBS_SIGMA) per coordinate."""
    kf = pb.intrinsics[pb.frame_cam]
    host = pb.point_host[block_point]
    b = synth.unproject(pb.model, kf[pb.point_host], pb.u_ref)
    ph = b / pb.rho_gt[:, None]
    Th, Tt = pb.poses_gt[host], pb.poses_gt[block_target]
    pw = (synth.quat_to_rot(Th[:, :4]) @ ph[block_point, :, None])[..., 0] + Th[:, 4:]
    pt = (np.swapaxes(synth.quat_to_rot(Tt[:, :4]), -1, -2) @ (pw - Tt[:, 4:])[..., None])[..., 0]
    return synth.project(pb.model, kf[block_target], pt) + rng.normal(0, OBS_SIGMA, (len(block_point), 2))


def build(n_frames, n_points, seed=SEED, kind=synth.PHOTOMETRIC, model=synth.PINHOLE, pattern=None, closures=(),
          idle=(), changed=False, cams=1):
    """The rewired problem (module docstring).  cams = 2: a second camera 2 % apart on the odd keyframes."""
    kw = {}
    if cams == 2:
        k0 = np.array(synth.DEFAULT_INTRINSICS[model], np.float64)
        k0[:4] *= 188 / 752.0
        k1 = k0.copy()
        k1[:4] *= 1.02
        kw = dict(intrinsics=np.stack([k0, k1]), frame_cam=np.arange(n_frames) % 2)
    pb = synth.make_problem(n_frames=n_frames, n_points=n_points, width=188, height=120, border=12, kind=kind,
                            model=model, pattern=pattern, seed=seed, poses_gt=closed_trajectory(n_frames), **kw)
    offsets = (np.array([1, 2, 3, 4]), np.array([-1, -2, -3, -4]), np.array([-2, -1, 1, 2]))
    closing = {}
    for h, t in closures:
        closing.setdefault(int(h), []).append(int(t))
    idle = set(int(f) for f in idle)
    bp, bt = [], []
    for p in range(n_points):
        h = int(pb.point_host[p])
        if h in idle:
            continue
        targets = [int(t) for t in h + offsets[p % 3] if 0 <= t < n_frames]
        targets += [t for t in closing.get(h, []) if t not in targets]
        for t in targets:
            if t not in idle:
                bp.append(p)
                bt.append(t)
    bp, bt = np.array(bp, np.int32), np.array(bt, np.int32)
    u_obs = None
    if pb.kind == synth.GEOMETRIC:
        u_obs = _observations(pb, bp, bt, np.random.default_rng(seed + 1))
    pb = dataclasses.replace(pb, block_point=bp, block_target=bt, u_obs=u_obs)
    pb.interp = 0
    if changed:
        gain, offset = R.brightness(pb.n_frames, float(pb.images.min()), float(pb.images.max()))
        pb = PAR.apply_brightness(pb, gain, offset)
    return pb


@functools.lru_cache(maxsize=None)
def problem(name, kind=synth.PHOTOMETRIC, model=synth.PINHOLE, P=8, changed=False, cams=1):
    """A named problem; its arrays are shared among the tests and left unchanged."""
    pb = build(kind=kind, model=model, pattern=R.pattern(P), changed=changed, cams=cams, **NAMED[name])
    for x in (pb.block_point, pb.block_target, pb.point_host, pb.poses, pb.rho):
        x.setflags(write=False)
    return pb


# ---- the graph, by brute force from (point_host, block_point, block_target) ------------------------------------------
def structure(pb):
    """Figures of the keyframe graph and of the lower 2×2-block skyline of the brightness system (row i starts at the
    smallest keyframe it shares a pair with)."""
    nf = pb.n_frames
    host = pb.point_host[pb.block_point].astype(np.int64)
    tgt = pb.block_target.astype(np.int64)
    pairs = set(zip(host.tolist(), tgt.tolist()))
    first = np.arange(nf)
    for h, t in pairs:
        first[max(h, t)] = min(first[max(h, t)], min(h, t))
    und = set((min(h, t), max(h, t)) for h, t in pairs)
    envelope = [(i, j) for i in range(nf) for j in range(first[i], i)]
    straddle = 0
    for p in np.unique(pb.block_point):
        d = tgt[pb.block_point == p] - int(pb.point_host[p])
        straddle += bool((d < 0).any() and (d > 0).any())
    right = left = 0  # envelope entries (r, c) whose row c starts right / left of row r's first column
    for i, j in envelope:
        right += first[j] > first[i]
        left += first[j] < first[i]
    widths = np.concatenate([2 * (np.arange(nf) - first) + 1, 2 * (np.arange(nf) - first) + 2])
    return {"pairs": len(pairs), "backward_pairs": sum(h > t for h, t in pairs),
            "both_ways": sum((t, h) in pairs for h, t in pairs if h < t), "straddling_points": straddle,
            "skyline_blocks": len(envelope) + nf, "unfilled_envelope_blocks": sum(e[::-1] not in und for e in envelope),
            "first_right": int(right), "first_left": int(left), "widths": set(widths.tolist()),
            "max_width": int(widths.max()), "first": first}


# ---- references --------------------------------------------------------------------------------------------------------
def records(pb, ab=None, poses=None, rho=None):
    """([r | J_host | J_target | J_rho] float64, valid): the oracle's for a geometric problem, gn_affine_reference's at
    the affine state ab (zeros: the plain photometric records) otherwise."""
    if pb.kind == synth.GEOMETRIC:
        return GR.O.evaluate(pb, poses=pb.poses if poses is None else poses, rho=pb.rho if rho is None else rho,
                             want_jac=True)
    return R.records(pb, np.zeros((pb.n_frames, 2)) if ab is None else ab, poses, rho)


def linearize_records(pb, rec, valid, a, fixed=(), fp32=False):
    """gn_reference.linearize's (H, g, cost) over N = 6·n_frames + n_points from given records, each block adding only
    its 13 nonzero columns (as gn_affine_reference.linearize does), so that 100 keyframes × 1000 points take a fraction of a
    second.  fp32: the records rounded to fp32 and back first."""
    rec = np.asarray(rec, np.float64)
    if fp32:
        rec = rec.astype(np.float32).astype(np.float64)
    r, Jh, Jt, Jr = GR.O.split_record(rec, pb.R)
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


@functools.lru_cache(maxsize=None)
def pose_reference(name, huber, kind=synth.PHOTOMETRIC, model=synth.PINHOLE, changed=False, fp32=False):
    """(records, valid, (H, g, cost)) of problem(name, …) with keyframes FIXED constant, at parity_state when `changed`:
    formed once, left unchanged."""
    pb = problem(name, kind=kind, model=model, changed=changed)
    rec, valid = records(pb, PAR.parity_state(pb.n_frames) if changed else None)
    H, g, cost = linearize_records(pb, rec, valid, huber, FIXED, fp32)
    for x in (rec, valid, H, g):
        x.setflags(write=False)
    return rec, valid, (H, g, cost)


def candidate_cost(pb, ab, poses, rho, a):
    """The robust cost at a candidate (poses, ρ)."""
    if pb.kind == synth.GEOMETRIC:
        rec, valid = GR.O.evaluate(pb, poses=poses, rho=rho, want_jac=False)
        cost_b, _ = GR.huber((rec[:, :2] ** 2).sum(1), a)
        return float(cost_b[valid == 1].sum())
    return R.cost_at(pb, np.zeros((pb.n_frames, 2)) if ab is None else ab, poses, rho, a)[0]


class perturbed_compose:
    """While entered, photometric_affine_reference.compose returns its records rounded to fp32 and back, with uniform
    noise of ±1.5e-5 on r (helpers.py's measured fp32 residual error): what linearize_ab would see of fp32 rows."""

    def __init__(self, seed=3):
        self.rng = np.random.default_rng(seed)

    def __enter__(self):
        self.plain = PAR.compose

        def compose(pb, ab, poses=None, rho=None, want_jac=True):
            rec, valid, uv = self.plain(pb, ab, poses, rho, want_jac)
            rec = rec.astype(np.float32).astype(np.float64)
            P = pb.pattern.shape[0]
            rec[:, :P] += self.rng.uniform(-1.5e-5, 1.5e-5, (rec.shape[0], P)) * (valid[:, None] == 1)
            return rec, valid, uv

        PAR.compose = compose
        return self

    def __exit__(self, *exc):
        PAR.compose = self.plain


# ---- the cases of the GPU tests ----------------------------------------------------------------------------------------
LAMBDAS = (1e-4, 1e-1)
POSE_CASES = [(name, huber) for name in ("band37", "closed100") for huber in (9.0, 0.0)]  # a: plain photometric
GEOMETRIC_CASES = [("band37", synth.PINHOLE), ("band37", synth.KB4), ("closed100", synth.PINHOLE)]  # b: Huber 1
BRIGHTNESS_CASES = (  # c: (problem, P, Huber width, fixed (a, b) keyframes)
    [("closed100", 8, huber, fixed) for huber in (9.0, 60.0, 0.0) for fixed in ((0,), (), (0, 37, 99))]
    + [("closed100_idle", 8, huber, fixed) for huber, fixed in ((9.0, (0,)), (60.0, ()), (0.0, (0, 37, 99)))]
    + [("closed100", 21, 9.0, (0,)), ("band37", 8, 9.0, (0,))])

# e: the loops.  Ceres' defaults but the options below, found by a search on the CPU for runs with at least three
# accepted and one rejected trial whose decisions all lie far from their thresholds (tests/test_graph_problems.py).
# With min_relative_decrease at its default of 1e-3 no radius between 1 and 1e4 gave such a run: the pose loop's late
# trials have relative decreases within 0.1 of 1e-3, and the brightness loop (nearly linear least squares: relative
# decreases of 0.64 … 1.7 from parity_state and from three times it, radius 1e2 … 1e8) rejects nothing.  The raised
# thresholds (as tests/test_gpu_gn.py's LM_CASES raise theirs) give, in the reference,
#   pose loop:       1.844 1.478 1.132 | 0.389 0.415 0.429 0.435 0.619 | 1.003 0.985     (AAA rrrrr AA)
#   brightness loop: 1.384 0.918 0.971 | 0.700 0.700 0.701 0.707                         (AAA rrrr)
LM_HUBER = 9.0
LM_OPTIONS = dict(max_iterations=10, initial_trust_region_radius=100.0, min_relative_decrease=0.8)
LM_AB_HUBER = 60.0
LM_AB_FIXED = (0,)
LM_AB_OPTIONS = dict(max_iterations=7, initial_trust_region_radius=1e4, min_relative_decrease=0.81)


def intrinsics_state(pb):
    """g, geometric: an intrinsics state away from the cameras the hosts unproject with (tests/test_gpu_gn.py's rigs)."""
    return pb.intrinsics * np.array([1.003, 0.998, 1.0005, 0.9995, 1, 1, 1, 1])


def lm_ab_start(pb):
    return PAR.parity_state(pb.n_frames)


def _reference_options(options):
    kw = dict(options)
    kw["radius"] = kw.pop("initial_trust_region_radius")
    return kw


@functools.lru_cache(maxsize=None)
def lm_reference():
    """gn_reference.lm (through gn_affine_reference.lm at the zero affine state, whose linearisation adds only each
    block's own columns) on band37.  The summary also gets `trial_costs` (the initial cost, then every candidate's)
    and `min_rho` (the smallest inverse distance any candidate carries)."""
    pb = problem("band37")
    plain = R.linearize
    costs, min_rho = [], []

    def linearize(pb_, ab, poses, rho, *args, **kw):
        out = plain(pb_, ab, poses, rho, *args, **kw)
        costs.append(out[2])
        min_rho.append(float(np.min(rho)))
        return out

    R.linearize = linearize
    try:
        out = R.lm(pb, np.zeros((pb.n_frames, 2)), LM_HUBER, FIXED, summary=True, **_reference_options(LM_OPTIONS))
    finally:
        R.linearize = plain
    n = len(out[5]["history"]) + 1
    out[5]["trial_costs"], out[5]["min_rho"] = costs[:n], min(min_rho[:n])
    return out


@functools.lru_cache(maxsize=None)
def lm_ab_reference():
    """gn_affine_reference.lm_ab on closed100 from parity_state.  The summary also gets `candidates` and `steps`: every
    trial's candidate cost and step δ."""
    pb = problem("closed100", changed=True)
    plain_cost, plain_step = R.cost_ab, R.step_ab
    cands, steps = [], []

    def cost_ab(*args, **kw):
        cands.append(plain_cost(*args, **kw))
        return cands[-1]

    def step_ab(*args, **kw):
        out = plain_step(*args, **kw)
        steps.append(out[0].copy())
        return out

    R.cost_ab, R.step_ab = cost_ab, step_ab
    try:
        out = R.lm_ab(pb, lm_ab_start(pb), LM_AB_HUBER, LM_AB_FIXED, **_reference_options(LM_AB_OPTIONS))
    finally:
        R.cost_ab, R.step_ab = plain_cost, plain_step
    out[4]["candidates"], out[4]["steps"] = cands, steps
    return out
