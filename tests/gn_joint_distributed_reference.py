"""The exchange of the multi-GPU joint solve (pba_joint_step_export / import) restated in numpy over
gn_joint_reference.linearize: every shard's keyframe system with its points eliminated at λ — undamped, no constants —,
the sum over the shards in rank order, then damping and constants from the summed diagonal and the summed counts of valid
blocks, one solve, and every shard's own back-substitution.

tests/test_gn_joint_distributed_reference.py checks it against gn_joint_reference.schur_step on the whole problem.
"""
from __future__ import annotations

import importlib

import numpy as np

import gn_joint_reference as R
import photometric_affine_reference as PAR

D = importlib.import_module("photometric-bundle-adjustment_amd.distributed")


def shards(pb, world, bounds=None):
    """[(shard problem, point ids, block ids)] of distributed.shard_problem, rank order."""
    return [D.shard_problem(pb, world, r, bounds) for r in range(world)]


def export(sub, ab, lam, huber=R.HUBER):
    """One rank's contribution at λ: dict of S (8·nf square), g_S, g_direct, diag, count (valid blocks per keyframe),
    cost, and what its back-substitution needs (B, 1/C', g_ρ, the damped points' diagonal)."""
    nf = sub.n_frames
    K = 8 * nf
    H, g, cost = R.linearize(sub, ab, sub.poses, sub.rho, huber)
    _, valid, _ = PAR.compose(sub, ab, sub.poses, sub.rho)
    count = np.zeros(nf)
    np.add.at(count, sub.point_host[sub.block_point], (valid == 1).astype(np.float64))
    np.add.at(count, sub.block_target, (valid == 1).astype(np.float64))
    A, B, C = H[:K, :K], H[:K, K:], np.diag(H)[K:]
    Dp = np.clip(C, 1e-6, 1e32)
    Ci = np.where(C > 0, 1.0 / (C + lam * Dp), 0.0)  # (a point without a valid block: no step)
    return {"S": A - (B * Ci) @ B.T, "gS": g[:K] - B @ (Ci * g[K:]), "g": g[:K].copy(), "diag": np.diag(A).copy(),
            "count": count, "cost": cost, "B": B, "Ci": Ci, "gl": g[K:].copy(), "Dp": np.where(Ci > 0, Dp, 0.0)}


def exchange_step(parts, ab, nf, lam, fixed=(), fixed_ab=()):
    """The ranks' exports summed in rank order, damped, constants applied, solved; every rank's δρ and point part.
    Returns (S, g_S, δ_keyframes (nf, 8), [δρ per rank], model decrease of the keyframes, [of each rank's points],
    constant mask)."""
    tot = {k: sum(p[k] for p in parts) for k in ("S", "gS", "g", "diag", "count")}  # (0 + rank 0 + rank 1 + …)
    ab = np.asarray(ab, np.float64).reshape(nf, 2)
    fp, fa = set(int(f) for f in fixed), set(int(f) for f in fixed_ab)
    fx = np.zeros(8 * nf, bool)
    for i in range(nf):
        seen = tot["count"][i] > 0
        fx[8 * i:8 * i + 6] = i in fp or not seen
        fx[8 * i + 6:8 * i + 8] = i in fa or not seen or not np.isfinite(ab[i]).all()
    Dk = np.clip(tot["diag"], 1e-6, 1e32)
    S = tot["S"] + lam * np.diag(Dk)
    gS = tot["gS"].copy()
    S[fx, :] = 0
    S[:, fx] = 0
    S[fx, fx] = 1.0
    gS[fx] = 0
    dk = np.linalg.solve(S, -gS)
    dk[fx] = 0.0
    free = ~fx
    model_kf = 0.5 * (lam * float(dk[free] @ (Dk[free] * dk[free])) - float(tot["g"][free] @ dk[free]))
    dls, model_pts = [], []
    for p in parts:
        dl = -(p["gl"] + p["B"].T @ dk) * p["Ci"]
        dls.append(dl)
        model_pts.append(0.5 * (lam * float(dl @ (p["Dp"] * dl)) - float(p["gl"] @ dl)))
    return S, gS, dk.reshape(nf, 8), dls, model_kf, model_pts, fx
