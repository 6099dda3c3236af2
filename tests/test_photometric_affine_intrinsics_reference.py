"""The CPU yardstick of the 26-column records — free target intrinsics together with affine brightness
(tests/photometric_affine_intrinsics_reference.py) — pinned.

On the project's small problem (6 keyframes, 161 points, 376×240, 644 blocks), at the intrinsics state
PIR.perturbed_state and the affine state PAR.parity_state:
  * J_intr's used columns and the four brightness columns match central differences of the composition's own r;
  * at a = b = 0 the first 22 columns are the 22-column reference's, at the cameras' intrinsics the 18-column
    reference's columns are reproduced;
  * the input conditions of the GPU tests hold on the reference alone (valid share, cell-edge mask);
  * "both come back": Gauss-Newton over fx, fy, cx, cy and (a_f, b_f), f ≥ 1, from a perturbed calibration and zero
    brightness recovers the calibration and drops the cost by more than 100.
Also: the Ceres drop-in's GpuPhotometricAffineIntrinsicsCost compiles against the Ceres 2.0 interface
(tests/cpp/photometric_affine_intrinsics_adapter_driver.cpp over tests/cpp/mock_ceres).
"""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import photometric_affine_intrinsics_reference as PAIR
import photometric_affine_reference as PAR
import photometric_intrinsics_reference as PIR
from helpers import ROOT, engine_module, near_cell_boundary, synth

DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "photometric_affine_intrinsics_adapter_driver.cpp")


@functools.lru_cache(maxsize=None)
def problem(model=synth.PINHOLE):
    pb = synth.make_problem(n_frames=6, n_points=161, width=376, height=240, border=12, model=model)
    pb.interp = 0
    return pb


@pytest.mark.parametrize("model", [synth.PINHOLE, synth.DOUBLE_SPHERE, synth.EUCM, synth.KB4])
def test_intrinsics_jacobian_matches_central_differences(model):
    """As tests/test_photometric_intrinsics_reference.py, on the affine residual: steps 1e-3 on fx, fy, cx, cy (r is
    bilinear in the position inside a cell and the position linear in those four: exact up to rounding) and 1e-6 on the
    distortion terms; rows whose ± positions share a cell with the centre, more than 95 % of them; within 1e-7 of the
    column's largest entry.  (a, b) scale neither I nor ∇I, so the bound is the 22-column reference's."""
    pb = problem(model)
    P = pb.P
    K, ab = PIR.perturbed_state(pb), PAR.parity_state(pb.n_frames)
    rec, valid, uv = PAIR.compose(pb, K, ab)
    m = valid.astype(bool)
    Ji = PAIR.split(rec, P)[4]
    assert np.all(Ji[:, :, PIR.N_USED[model]:] == 0.0)
    cell = np.floor(uv)
    for j in range(PIR.N_USED[model]):
        h = 1e-3 if j < 4 else 1e-6
        Kp, Km = K.copy(), K.copy()
        Kp[:, j] += h
        Km[:, j] -= h
        rp, vp, uvp = PAIR.compose(pb, Kp, ab, want_jac=False)
        rm, vm, uvm = PAIR.compose(pb, Km, ab, want_jac=False)
        keep = (m & vp.astype(bool) & vm.astype(bool))[:, None] & (np.floor(uvp) == cell).all(-1) & \
            (np.floor(uvm) == cell).all(-1)
        frac = keep.sum() / (m.sum() * P)
        fd = (rp[:, :P] - rm[:, :P]) / (2 * h)
        err = np.abs(fd - Ji[:, :, j])[keep].max() / np.abs(Ji[:, :, j][keep]).max()
        print(f"model {model} column {j}: kept {frac:.4f}, error {err:.3e} of the column's largest entry")
        assert frac > 0.95
        assert err <= 1e-7


def test_brightness_columns_match_central_differences():
    """As tests/test_photometric_affine_reference.py, at the perturbed intrinsics state: step 1e-4 in a (the central
    difference's own error is h²/6 of the entry, 1.7e-9) and 1 in b (r is linear in b: exact up to rounding); bound 2e-8
    of the column's largest entry.  One perturbed evaluation per (keyframe, parameter, sign) serves both sides: the
    blocks the keyframe hosts give J_ab_host's column, the blocks it is the target of give J_ab_target's."""
    pb = problem()
    P = pb.P
    K, ab = PIR.perturbed_state(pb), PAR.parity_state(pb.n_frames)
    rec, valid, _ = PAIR.compose(pb, K, ab)
    m = valid.astype(bool)
    host = pb.point_host[pb.block_point]
    parts = PAIR.split(rec, P)
    worst = 0.0
    for c, h in ((0, 1e-4), (1, 1.0)):
        fd_h, fd_t = np.zeros((pb.n_blocks, P)), np.zeros((pb.n_blocks, P))
        for f in range(pb.n_frames):
            p, q = ab.copy(), ab.copy()
            p[f, c] += h
            q[f, c] -= h
            d = (PAIR.compose(pb, K, p, want_jac=False)[0][:, :P] - PAIR.compose(pb, K, q, want_jac=False)[0][:, :P]) / (2 * h)
            fd_h[host == f] = d[host == f]
            fd_t[pb.block_target == f] = d[pb.block_target == f]
        for side, fd, J in (("host", fd_h, parts[5]), ("target", fd_t, parts[6])):
            err = np.abs(fd - J[:, :, c])[m].max() / np.abs(J[:, :, c][m]).max()
            print(f"J_ab_{side} column {c}: error {err:.3e} of the column's largest entry")
            worst = max(worst, err)
            assert err <= 2e-8
    assert worst > 0.0  # (the comparison ran on non-trivial columns)
    assert np.all(parts[6][m][:, :, 1] == -1.0) and np.all(rec[~m] == 0.0)


def test_composition_reduces_to_the_two_references():
    pb = problem()
    P = pb.P
    K, ab = PIR.perturbed_state(pb), PAR.parity_state(pb.n_frames)
    # a = b = 0: the 22-column reference (r = ((r₀ + I_h) − 0) − 1·(I_h − 0): r₀ up to one rounding of the sum)
    rec, valid, uv = PAIR.compose(pb, K, np.zeros_like(ab))
    ref22, v22, uv22 = PIR.compose(pb, K)
    m = v22.astype(bool)
    assert np.array_equal(valid, v22) and np.array_equal(uv, uv22)
    assert np.array_equal(rec[:, P:22 * P], ref22[:, P:22 * P]) and np.abs(rec[m, :P] - ref22[m, :P]).max() <= 1e-13
    Jh, Jt = PAIR.split(rec, P)[5:]
    assert np.array_equal(Jh[m][:, :, 0], pb.host_intensity[pb.block_point][m].astype(np.float64))
    assert np.all(Jh[m][:, :, 1] == 1.0) and np.array_equal(Jt[m], -Jh[m])
    # the cameras' intrinsics: the 18-column reference's r and brightness columns (another evaluation of the same
    # projection: r within 1e-9, as the 22-column reference is pinned against the oracle)
    rec, valid, _ = PAIR.compose(pb, pb.intrinsics, ab)
    ref18, v18, _ = PAR.compose(pb, ab)
    m = v18.astype(bool)
    assert np.array_equal(valid, v18)
    assert np.abs(rec[m, :P] - ref18[m, :P]).max() <= 1e-9
    assert np.array_equal(rec[:, 22 * P:], ref18[:, 14 * P:])


def test_input_conditions_of_the_gpu_tests():
    pb = problem()
    K, ab = PIR.perturbed_state(pb), PAR.parity_state(pb.n_frames)
    rec, valid, uv = PAIR.compose(pb, K, ab)
    m = valid.astype(bool)
    masked = near_cell_boundary(uv[m]).mean()
    print(f"valid blocks {m.sum()} of {pb.n_blocks}, cell-edge pixels {masked:.4f}")
    assert m.sum() > 0.9 * pb.n_blocks and masked <= 0.02


def test_both_come_back():
    """The reference run of the GPU suite's "both come back": PAR.brightness_case() (true poses and ρ, gains and offsets
    on frames 1–5), the intrinsics state started 0.229, 0.229, 0.092 and 0.062 px off (PIR.perturbed_state), (a, b) at 0;
    six Gauss-Newton steps over fx, fy, cx, cy and (a_f, b_f), f ≥ 1.  Measured: cost 316612.65 → 2772.38 → 2108.31 →
    2108.1975, then flat (a ratio of 150); the intrinsics come back to ≤ 4.4e-3 px of the cameras'.  Bounds: 100 on the
    drop, 1e-2 px on the calibration (2.3× the measured error: the floor is the rendered keyframes' photo-consistency,
    tests/test_photometric_affine_reference.py), no rise after convergence."""
    pb, K0 = PAIR.both_case()
    d0 = np.abs(K0[0, :4] - pb.intrinsics[0, :4])
    costs, K, ab = PAIR.both_run(lambda K, s: PAIR.compose(pb, K, s)[:2], pb, K0)
    err = np.abs(K[0, :4] - pb.intrinsics[0, :4])
    print("reference costs", costs, "initial intrinsics error", d0, "final", err, "final (a, b)", ab)
    assert costs[0] > 100 * costs[-1] and costs[-1] <= costs[-2] * (1 + 1e-9)
    assert d0.min() > 0.05 and err.max() <= 1e-2
    assert np.all(ab[0] == 0.0) and np.abs(ab[1:]).max() > 1e-2


def test_photometric_affine_intrinsics_cost_compiles_against_ceres_interface():
    E = engine_module()
    E.build()
    libdir = os.path.dirname(E.LIB_PATH)
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "photometric_affine_intrinsics_adapter_driver")
        cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
               "-I", os.path.join(ROOT, "tests", "cpp", "mock_ceres"), DRIVER_SRC, "-o", exe,
               "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"]
        subprocess.run(cmd, check=True, capture_output=True, text=True)
        assert os.path.exists(exe)
