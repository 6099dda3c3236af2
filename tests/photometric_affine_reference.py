"""CPU reference for photometric records with affine brightness (pba_set_affine_brightness), composed in numpy double
from the oracle's plain photometric evaluation.  The oracle itself has no brightness parameters.

Every keyframe f has (a_f, b_f); with h the block's host, t its target and E = exp(a_t − a_h)

    r_k = (I_t(π(p̃_k)) − b_t) − E·(I_h,k − b_h)

oracle.evaluate gives r₀ = I − I_h and the 14 columns [r₀ | J_host | J_target | J_rho]; with I = r₀ + I_h the residual
above and the four new columns follow, and the geometric columns are the oracle's own (∇I does not depend on (a, b)):

    18·P values: [ r | J_host (P×6) | J_target (P×6) | J_rho | J_ab_host (P×2) | J_ab_target (P×2) ]
    row k: J_ab_host = [∂r/∂a_h, ∂r/∂b_h] = [+E·(I_h,k − b_h), +E],  J_ab_target = [∂r/∂a_t, ∂r/∂b_t] = [−E·(I_h,k − b_h), −1]

A block is valid when the oracle says so and every value is finite; an invalid block's record is zero.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import oracle as O
from helpers import near_cell_boundary, projected_uv, synth


def compose(pb, ab, poses=None, rho=None, want_jac: bool = True):
    """(records (n_blocks, 18·P) float64, valid (n_blocks,) uint8, uv (n_blocks, P, 2) the projected positions) at the
    affine state ab (n_frames, 2) = [a_f, b_f].  Residual-only (want_jac False): only r is filled."""
    assert pb.kind == synth.PHOTOMETRIC
    ab = np.ascontiguousarray(ab, np.float64).reshape(pb.n_frames, 2)
    poses = np.ascontiguousarray(pb.poses if poses is None else poses, np.float64)
    rho = np.ascontiguousarray(pb.rho if rho is None else rho, np.float64)
    nb, P = pb.n_blocks, pb.pattern.shape[0]
    rec14, valid = O.evaluate(pb, poses, rho, want_jac=want_jac)
    with np.errstate(all="ignore"):
        uv = projected_uv(dataclasses.replace(pb, poses=poses, rho=rho))
        host = pb.point_host[pb.block_point]
        Ih = pb.host_intensity[pb.block_point].astype(np.float64)  # (nb, P)
        I = rec14[:, :P] + Ih
        E = np.exp(ab[pb.block_target, 0] - ab[host, 0])[:, None]
        bh, bt = ab[host, 1][:, None], ab[pb.block_target, 1][:, None]
        g = E * (Ih - bh)
        rec = np.zeros((nb, 18 * P))
        rec[:, :P] = (I - bt) - g
        if want_jac:
            rec[:, P:14 * P] = rec14[:, P:14 * P]
            rec[:, 14 * P:16 * P] = np.stack([g, np.broadcast_to(E, g.shape)], -1).reshape(nb, 2 * P)
            rec[:, 16 * P:18 * P] = np.stack([-g, -np.ones_like(g)], -1).reshape(nb, 2 * P)
    ok = valid.astype(bool) & np.isfinite(rec).all(1)
    rec[~ok] = 0.0
    return rec, ok.astype(np.uint8), uv


def split(rec: np.ndarray, P: int):
    """(r, J_host, J_target, J_rho, J_ab_host, J_ab_target) views of 18·P-value records."""
    n = rec.shape[0]
    return (rec[:, :P], rec[:, P:7 * P].reshape(n, P, 6), rec[:, 7 * P:13 * P].reshape(n, P, 6), rec[:, 13 * P:14 * P],
            rec[:, 14 * P:16 * P].reshape(n, P, 2), rec[:, 16 * P:18 * P].reshape(n, P, 2))


BLOCKS = (("J_host", 1, 7), ("J_target", 7, 13), ("J_rho", 13, 14), ("J_ab_host", 14, 16), ("J_ab_target", 16, 18))


def compare(P: int, got, ref, valid_got, valid_ref, uv, bilinear: bool, r_atol: float = 1e-4, j_rtol: float = 1e-5,
            max_masked: float = 0.02):
    """The project's fp32-vs-double bounds (tests/helpers.py compare_records) over all 18·P columns: |Δr| ≤ r_atol,
    each Jacobian block — J_ab_host and J_ab_target normalised on their own like the others — within j_rtol of its
    block's largest reference entry, validity identical.  Bilinear: pixels within 2e-3 px of a cell edge are left out of
    the Jacobian comparison, at most max_masked of them.  Prints and returns the figures."""
    assert np.array_equal(np.asarray(valid_got).astype(bool), np.asarray(valid_ref).astype(bool)), "validity flags differ"
    m = np.asarray(valid_ref).astype(bool)
    g, r = got[m].astype(np.float64), ref[m]
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
    print("photometric-affine parity:", st)
    assert st["r_maxabs"] <= r_atol, st
    assert st["masked_frac"] <= max_masked, st
    for name, _, _ in BLOCKS:
        assert st[name + "_rel"] <= j_rtol, (name, st)
    return st


def parity_state(n_frames: int, seed: int = 7) -> np.ndarray:
    """The parity tests' affine state: a_f uniform in [−0.3, 0.3], b_f uniform in [−20, 20], frame 0 included."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.3, 0.3, n_frames), rng.uniform(-20.0, 20.0, n_frames)], 1)



def apply_brightness(pb, gain, offset):
    """The problem with frame f's image replaced by round(gain_f · img + offset_f) (u8) and host_intensity re-sampled
    from the changed host images (oracle.sample at u_ref + pattern).  No pixel may clip at 0 or 255."""
    gain = np.asarray(gain, np.float64).reshape(pb.n_frames)
    offset = np.asarray(offset, np.float64).reshape(pb.n_frames)
    x = gain[:, None, None] * pb.images.astype(np.float64) + offset[:, None, None]
    assert x.min() >= 0.0 and x.max() <= 255.0, ("a pixel clips", float(x.min()), float(x.max()))
    images = np.rint(x).astype(np.uint8)
    interp = int(getattr(pb, "interp", 0))
    hi = np.empty((pb.n_points, pb.pattern.shape[0]), np.float32)
    for f in np.unique(pb.point_host):
        sel = np.nonzero(pb.point_host == f)[0]
        pos = pb.u_ref[sel, None, :] + pb.pattern[None, :, :].astype(np.float64)
        hi[sel] = O.sample(images[f], pos.reshape(-1, 2), interp)[:, 0].reshape(sel.size, -1).astype(np.float32)
    out = dataclasses.replace(pb, images=images, host_intensity=hi)
    if hasattr(pb, "interp"):
        out.interp = pb.interp
    return out


def brightness_case(seed: int = 11):
    """"Brightness comes back": the small problem at the true poses and ρ with frame 0 left alone (gain 1, offset 0, the
    gauge) and distinct gains and offsets on frames 1–5, drawn within ±10 % and ±8 grey levels and shrunk by halves
    until no pixel clips.  Returns (problem, gain, offset)."""
    pb = synth.make_problem(n_frames=6, n_points=161, width=376, height=240, border=12, perturb=False, seed=seed)
    pb.interp = 0
    rng = np.random.default_rng(seed)
    dg, do = rng.uniform(-0.10, 0.10, pb.n_frames), rng.uniform(-8.0, 8.0, pb.n_frames)
    dg[0] = do[0] = 0.0
    lo, hi = float(pb.images.min()), float(pb.images.max())
    s = 1.0
    while True:
        gain, offset = 1.0 + s * dg, s * do
        if (gain * lo + offset).min() >= 0.0 and (gain * hi + offset).max() <= 255.0:  # (gains are positive)
            return apply_brightness(pb, gain, offset), gain, offset
        s *= 0.5
        assert s > 1e-3, "the images span the whole u8 range: no brightness change fits"


def brightness_run(evaluate_at, pb, n_iter: int = 4):
    """Gauss-Newton in numpy over the 10 unknowns (a_f, b_f), f ≥ 1 (frame 0 is the gauge), from the zero state, on r and
    the two brightness Jacobian blocks of evaluate_at(ab) → (records (n_blocks, 18·P), valid).  Returns (the cost
    ½Σr² before every step and after the last, the final state (n_frames, 2))."""
    P, nf = pb.pattern.shape[0], pb.n_frames
    host = pb.point_host[pb.block_point]
    ab, costs = np.zeros((nf, 2)), []
    for it in range(n_iter + 1):
        rec, valid = evaluate_at(ab)
        m = np.asarray(valid).astype(bool)
        r, _, _, _, Jh, Jt = split(np.asarray(rec)[m].astype(np.float64), P)
        costs.append(0.5 * float((r * r).sum()))
        if it == n_iter:
            break
        n = r.shape[0]
        J = np.zeros((n, P, nf, 2))
        idx = np.arange(n)
        J[idx, :, host[m], :] += Jh
        J[idx, :, pb.block_target[m], :] += Jt
        J = J.reshape(n * P, 2 * nf)[:, 2:]
        ab[1:] -= np.linalg.solve(J.T @ J, J.T @ r.reshape(-1)).reshape(nf - 1, 2)
    return costs, ab
