"""CPU reference for photometric records with free target intrinsics (pba_set_optimize_intrinsics on a photometric
engine), composed from the oracle's geometric intrinsics evaluation and its interpolator.  The oracle itself has no
photometric intrinsics Jacobian.

For a central camera π(p̃) = π(p̃/ρ), so pixel k of a photometric block is the geometric block of a point at
u_ref + o_k with the same ρ.  For every pattern pixel k:
  * oracle.evaluate_intrinsics on that geometric twin with u_obs = 0 (so π = −r), projecting with the intrinsics
    state K of the target's camera and unprojecting with the problem's cameras;
  * oracle.sample(image[target], π, interp) → [I, I_u, I_v];
  * r_k = I − I_h,k, and every Jacobian block is −(I_u · J_geo[row 0] + I_v · J_geo[row 1]), J_intr included.
A block is valid when every pixel's p̃ lies in the state camera's projection domain (the oracle's own rule) and every
value is finite; an invalid block's record is zero.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

import oracle as O
from helpers import synth


def warped_points(pb, poses=None, rho=None) -> np.ndarray:
    """p̃_k = R_th b_k + ρ t_th of every (block, pixel): (n_blocks, P, 3), numpy double; the host unprojects with the
    problem's cameras."""
    poses = pb.poses if poses is None else poses
    rho = pb.rho if rho is None else rho
    host = pb.point_host[pb.block_point]
    Th, Tt = poses[host], poses[pb.block_target]
    kh = pb.intrinsics[pb.frame_cam[host]]
    ur = pb.u_ref[pb.block_point]
    Rh, Rt = synth.quat_to_rot(Th[:, :4]), synth.quat_to_rot(Tt[:, :4])
    Rth = np.swapaxes(Rt, 1, 2) @ Rh
    tth = (np.swapaxes(Rt, 1, 2) @ (Th[:, 4:] - Tt[:, 4:])[..., None])[..., 0]
    r = rho[pb.block_point]
    p = np.empty((pb.n_blocks, pb.pattern.shape[0], 3))
    for j, d in enumerate(pb.pattern.astype(np.float64)):
        b = synth.unproject(pb.model, kh, ur + d[None, :])
        p[:, j] = (Rth @ b[..., None])[..., 0] + r[:, None] * tth
    return p


def in_domain(model: int, K: np.ndarray, p: np.ndarray) -> np.ndarray:
    """The oracle's projection-domain rule for points p (n, 3) with per-point intrinsics K (n, 8)."""
    L = O.lib()
    K = np.ascontiguousarray(K, np.float64)
    p = np.ascontiguousarray(p, np.float64)
    out = np.zeros(p.shape[0], bool)
    for i in range(p.shape[0]):
        out[i] = bool(L.orc_in_domain(int(model), C.c_void_p(K[i].ctypes.data), C.c_void_p(p[i].ctypes.data)))
    return out


def compose(pb, K_state, poses=None, rho=None, want_jac: bool = True):
    """(records (n_blocks, 22·P) float64 = [r | J_host (P×6) | J_target (P×6) | J_rho | J_intr (P×8)], valid (n_blocks,)
    uint8, uv (n_blocks, P, 2) the projected positions).  Residual-only (want_jac False): only r is filled."""
    assert pb.kind == synth.PHOTOMETRIC
    K_state = np.ascontiguousarray(K_state, np.float64).reshape(-1, 8)
    poses = np.ascontiguousarray(pb.poses if poses is None else poses, np.float64)
    rho = np.ascontiguousarray(pb.rho if rho is None else rho, np.float64)
    nb, P = pb.n_blocks, pb.pattern.shape[0]
    interp = int(getattr(pb, "interp", 0))
    rec = np.zeros((nb, 22 * P))
    uv = np.zeros((nb, P, 2))
    ok = np.ones(nb, bool)
    with np.errstate(all="ignore"):
        p = warped_points(pb, poses, rho)
    Kt = K_state[pb.frame_cam[pb.block_target]]
    for k in range(P):
        ok &= in_domain(pb.model, Kt, p[:, k])
        twin = dataclasses.replace(pb, kind=synth.GEOMETRIC, images=None, host_intensity=None,
                                   u_ref=pb.u_ref + pb.pattern[k].astype(np.float64)[None, :],
                                   u_obs=np.zeros((nb, 2)))
        geo, vg = O.evaluate_intrinsics(twin, K_state, poses, rho, want_jac=want_jac)
        ok &= vg.astype(bool)
        pi = -geo[:, :2]
        uv[:, k] = pi
        for t in np.unique(pb.block_target):
            sel = np.nonzero((pb.block_target == t) & vg.astype(bool))[0]
            if sel.size == 0:
                continue
            s = O.sample(pb.images[t], pi[sel], interp)
            rec[sel, k] = s[:, 0] - pb.host_intensity[pb.block_point[sel], k].astype(np.float64)
            if not want_jac:
                continue
            Iu, Iv = s[:, 1, None], s[:, 2, None]
            g = geo[sel]
            rec[sel, P + 6 * k:P + 6 * k + 6] = -(Iu * g[:, 2:8] + Iv * g[:, 8:14])
            rec[sel, 7 * P + 6 * k:7 * P + 6 * k + 6] = -(Iu * g[:, 14:20] + Iv * g[:, 20:26])
            rec[sel, 13 * P + k] = -(Iu[:, 0] * g[:, 26] + Iv[:, 0] * g[:, 27])
            rec[sel, 14 * P + 8 * k:14 * P + 8 * k + 8] = -(Iu * g[:, 28:36] + Iv * g[:, 36:44])
    ok &= np.isfinite(rec).all(1)
    rec[~ok] = 0.0
    return rec, ok.astype(np.uint8), uv


def split(rec: np.ndarray, P: int):
    """(r, J_host, J_target, J_rho, J_intr) views of 22·P-value records."""
    n = rec.shape[0]
    return (rec[:, :P], rec[:, P:7 * P].reshape(n, P, 6), rec[:, 7 * P:13 * P].reshape(n, P, 6),
            rec[:, 13 * P:14 * P], rec[:, 14 * P:22 * P].reshape(n, P, 8))


def perturbed_state(pb, sign: float = 1.0) -> np.ndarray:
    """The tests' intrinsics state: the cameras × (1 + 1e-3·[1, −1, 0.5, −0.5]) on fx, fy, cx, cy, ±1e-3 on the model's
    first two distortion terms, ±1e-4 on KB4's last two.  sign = −1 perturbs the other way (a second camera)."""
    K = np.array(pb.intrinsics, np.float64, copy=True)
    K[:, :4] *= 1.0 + sign * 1e-3 * np.array([1.0, -1.0, 0.5, -0.5])
    if pb.model != synth.PINHOLE:
        K[:, 4] += sign * 1e-3
        K[:, 5] -= sign * 1e-3
    if pb.model == synth.KB4:
        K[:, 6] += sign * 1e-4
        K[:, 7] -= sign * 1e-4
    return K


def level_state(K: np.ndarray, level: int) -> np.ndarray:
    """The level-l image of an intrinsics state: fx/2^l, fy/2^l, c_l = (c + 0.5)/2^l − 0.5, distortion unchanged."""
    s = 0.5 ** level
    K = np.array(K, np.float64, copy=True)
    K[:, 0] *= s
    K[:, 1] *= s
    K[:, 2] = (K[:, 2] + 0.5) * s - 0.5
    K[:, 3] = (K[:, 3] + 0.5) * s - 0.5
    return K


N_USED = {synth.PINHOLE: 4, synth.DOUBLE_SPHERE: 6, synth.EUCM: 6, synth.KB4: 8}


def compare(P: int, got, ref, valid_got, valid_ref, uv, bilinear: bool, r_atol: float = 1e-4, j_rtol: float = 1e-5,
            max_masked: float = 0.02):
    """The project's fp32-vs-double bounds (tests/helpers.py compare_records) over all 22·P columns: |Δr| ≤ r_atol,
    each Jacobian block — J_intr normalised on its own like the others — within j_rtol of its block's largest reference
    entry, validity identical.  Bilinear: pixels within 2e-3 px of a cell edge are left out of the Jacobian comparison,
    at most max_masked of them.  Prints and returns the figures."""
    from helpers import near_cell_boundary
    assert np.array_equal(np.asarray(valid_got).astype(bool), np.asarray(valid_ref).astype(bool)), "validity flags differ"
    m = np.asarray(valid_ref).astype(bool)
    g, r = got[m].astype(np.float64), ref[m]
    n = g.shape[0]
    st = {"blocks": int(n)}
    st["r_maxabs"] = float(np.abs(g[:, :P] - r[:, :P]).max()) if n else 0.0
    pix_ok = ~near_cell_boundary(uv[m]) if bilinear else np.ones((n, P), bool)
    st["masked_frac"] = float((~pix_ok).mean()) if n else 0.0
    for name, lo, hi in (("J_host", P, 7 * P), ("J_target", 7 * P, 13 * P), ("J_rho", 13 * P, 14 * P),
                         ("J_intr", 14 * P, 22 * P)):
        w = (hi - lo) // P
        gj, rj = g[:, lo:hi].reshape(n, P, w), r[:, lo:hi].reshape(n, P, w)
        scale = np.maximum(np.abs(rj).reshape(n, -1).max(1), 1e-12)[:, None, None]
        err = (np.abs(gj - rj) / scale)[pix_ok]
        st[name + "_rel"] = float(err.max()) if err.size else 0.0
    print("photometric-intrinsics parity:", st)
    assert st["r_maxabs"] <= r_atol, st
    assert st["masked_frac"] <= max_masked, st
    for name in ("J_host", "J_target", "J_rho", "J_intr"):
        assert st[name + "_rel"] <= j_rtol, (name, st)
    return st
