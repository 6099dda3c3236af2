"""CPU reference for photometric records with free target intrinsics AND affine brightness
(pba_set_intrinsics_with_affine, then pba_set_optimize_intrinsics and pba_set_affine_brightness), composed in numpy
double from the two existing references.

photometric_intrinsics_reference.compose(pb, K) gives the 22 columns [r₀ | J_host | J_target | J_rho | J_intr] with
r₀ = I − I_h at the intrinsics state K (the target projects with K, the host unprojects with the cameras).  With
I = r₀ + I_h, h the block's host, t its target and E = exp(a_t − a_h), the residual and the brightness columns follow as
in photometric_affine_reference.compose, and the geometric and intrinsics columns are the 22-column reference's own (∇I
does not depend on (a, b)):

    26·P values: [ r | J_host (P×6) | J_target (P×6) | J_rho | J_intr (P×8) | J_ab_host (P×2) | J_ab_target (P×2) ]
    r_k = (I − b_t) − E·(I_h,k − b_h)
    row k: J_ab_host = [+E·(I_h,k − b_h), +E],  J_ab_target = [−E·(I_h,k − b_h), −1]

A block is valid when the 22-column reference says so and every value is finite; an invalid block's record is zero.
"""
from __future__ import annotations

import numpy as np

import photometric_affine_reference as PAR
import photometric_intrinsics_reference as PIR
from helpers import near_cell_boundary, synth


def compose(pb, K_state, ab, poses=None, rho=None, want_jac: bool = True):
    """(records (n_blocks, 26·P) float64, valid (n_blocks,) uint8, uv (n_blocks, P, 2) the projected positions) at the
    intrinsics state K_state (n_cams, 8) and the affine state ab (n_frames, 2).  Residual-only (want_jac False): only r
    is filled."""
    assert pb.kind == synth.PHOTOMETRIC
    ab = np.ascontiguousarray(ab, np.float64).reshape(pb.n_frames, 2)
    nb, P = pb.n_blocks, pb.pattern.shape[0]
    rec22, valid, uv = PIR.compose(pb, K_state, poses, rho, want_jac=want_jac)
    with np.errstate(all="ignore"):
        host = pb.point_host[pb.block_point]
        Ih = pb.host_intensity[pb.block_point].astype(np.float64)  # (nb, P)
        I = rec22[:, :P] + Ih
        E = np.exp(ab[pb.block_target, 0] - ab[host, 0])[:, None]
        bh, bt = ab[host, 1][:, None], ab[pb.block_target, 1][:, None]
        g = E * (Ih - bh)
        rec = np.zeros((nb, 26 * P))
        rec[:, :P] = (I - bt) - g
        if want_jac:
            rec[:, P:22 * P] = rec22[:, P:22 * P]
            rec[:, 22 * P:24 * P] = np.stack([g, np.broadcast_to(E, g.shape)], -1).reshape(nb, 2 * P)
            rec[:, 24 * P:26 * P] = np.stack([-g, -np.ones_like(g)], -1).reshape(nb, 2 * P)
    ok = valid.astype(bool) & np.isfinite(rec).all(1)
    rec[~ok] = 0.0
    return rec, ok.astype(np.uint8), uv


def split(rec: np.ndarray, P: int):
    """(r, J_host, J_target, J_rho, J_intr, J_ab_host, J_ab_target) views of 26·P-value records."""
    n = rec.shape[0]
    return (rec[:, :P], rec[:, P:7 * P].reshape(n, P, 6), rec[:, 7 * P:13 * P].reshape(n, P, 6), rec[:, 13 * P:14 * P],
            rec[:, 14 * P:22 * P].reshape(n, P, 8), rec[:, 22 * P:24 * P].reshape(n, P, 2),
            rec[:, 24 * P:26 * P].reshape(n, P, 2))


BLOCKS = (("J_host", 1, 7), ("J_target", 7, 13), ("J_rho", 13, 14), ("J_intr", 14, 22), ("J_ab_host", 22, 24),
          ("J_ab_target", 24, 26))


def compare(P: int, got, ref, valid_got, valid_ref, uv, bilinear: bool, r_atol: float = 1e-4, j_rtol: float = 1e-5,
            max_masked: float = 0.02):
    """The project's fp32-vs-double bounds (tests/helpers.py compare_records) over all 26·P columns: |Δr| ≤ r_atol,
    each Jacobian block — J_intr, J_ab_host and J_ab_target each normalised on its own like the others — within j_rtol
    of its block's largest reference entry, validity identical.  Bilinear: pixels within 2e-3 px of a cell edge are left
    out of the Jacobian comparison, at most max_masked of them.  Prints and returns the figures."""
    assert np.array_equal(np.asarray(valid_got).astype(bool), np.asarray(valid_ref).astype(bool)), "validity flags differ"
    m = np.asarray(valid_ref).astype(bool)
    g, r = np.asarray(got)[m].astype(np.float64), ref[m]
    n = g.shape[0]
    st = {"blocks": int(n)}
    st["r_maxabs"] = float(np.abs(g[:, :P] - r[:, :P]).max()) if n else 0.0
    pix_ok = ~near_cell_boundary(uv[m]) if bilinear else np.ones((n, P), bool)
    st["masked_frac"] = float((~pix_ok).mean()) if n else 0.0
    for name, c0, c1 in BLOCKS:
        lo, hi, w = c0 * P, c1 * P, c1 - c0
        gj, rj = g[:, lo:hi].reshape(n, P, w), r[:, lo:hi].reshape(n, P, w)
        scale = np.maximum(np.abs(rj).reshape(n, -1).max(1), 1e-12)[:, None, None]
        err = (np.abs(gj - rj) / scale)[pix_ok]
        st[name + "_rel"] = float(err.max()) if err.size else 0.0
    print("photometric-affine-intrinsics parity:", st)
    assert st["r_maxabs"] <= r_atol, st
    assert st["masked_frac"] <= max_masked, st
    for name, _, _ in BLOCKS:
        assert st[name + "_rel"] <= j_rtol, (name, st)
    return st


def both_run(evaluate_at, pb, K0, n_iter: int = 6):
    """"Both come back": Gauss-Newton in numpy over the 14 unknowns fx, fy, cx, cy of the one camera and (a_f, b_f), f ≥ 1
    (frame 0 is the brightness gauge), from the intrinsics state K0 and (a, b) = 0, on r, J_intr[..., :4] and the two
    brightness blocks of evaluate_at(K, ab) → (records (n_blocks, 26·P), valid).  Returns (the cost ½Σr² before every step
    and after the last, the final intrinsics state, the final affine state)."""
    P, nf = pb.pattern.shape[0], pb.n_frames
    assert pb.intrinsics.shape[0] == 1
    host = pb.point_host[pb.block_point]
    K, ab, costs = np.array(K0, np.float64, copy=True), np.zeros((nf, 2)), []
    for it in range(n_iter + 1):
        rec, valid = evaluate_at(K, ab)
        m = np.asarray(valid).astype(bool)
        r, _, _, _, Ji, Jh, Jt = split(np.asarray(rec)[m].astype(np.float64), P)
        costs.append(0.5 * float((r * r).sum()))
        if it == n_iter:
            break
        n = r.shape[0]
        Jab = np.zeros((n, P, nf, 2))
        idx = np.arange(n)
        Jab[idx, :, host[m], :] += Jh
        Jab[idx, :, pb.block_target[m], :] += Jt
        J = np.concatenate([Ji[:, :, :4].reshape(n * P, 4), Jab.reshape(n * P, 2 * nf)[:, 2:]], 1)
        d = np.linalg.solve(J.T @ J, J.T @ r.reshape(-1))
        K[0, :4] -= d[:4]
        ab[1:] -= d[4:].reshape(nf - 1, 2)
    return costs, K, ab


def both_case():
    """The set-up of "both come back": PAR.brightness_case() (true poses and ρ, gains and offsets on frames 1–5) and the
    intrinsics state started at PIR.perturbed_state.  Returns (problem, K0)."""
    pb, _, _ = PAR.brightness_case()
    return pb, PIR.perturbed_state(pb)
