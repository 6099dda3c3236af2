"""The CPU yardstick of the photometric free-intrinsics records (tests/photometric_intrinsics_reference.py), pinned.

With the state at the cameras' values the composition must reproduce oracle.evaluate — r within 1e-9, every Jacobian
block within 1e-10 of its block's largest entry, the same validity flags — and the unused distortion columns of J_intr
are exact zeros.  J_intr itself is checked against central differences of the composed residual over the state
(bilinear; rows whose ± positions share a cell with the centre, more than 95 % of them): within 1e-7 of the column's
largest entry.  The steps: 1e-3 on fx, fy, cx, cy — r is bilinear in the position inside a cell and the position is
linear in those four, so the central difference is exact up to rounding — and 1e-6 on the distortion terms.

Also: the Ceres drop-in's photometric cost with an intrinsics block compiles against the Ceres 2.0 interface
(tests/cpp/photometric_intrinsics_adapter_driver.cpp over tests/cpp/mock_ceres).
"""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle as O
import photometric_intrinsics_reference as PIR
from helpers import ROOT, engine_module, synth

MODELS = [synth.PINHOLE, synth.DOUBLE_SPHERE, synth.EUCM, synth.KB4]
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "photometric_intrinsics_adapter_driver.cpp")


@functools.lru_cache(maxsize=None)
def problem(model, interp):
    pb = synth.make_problem(n_frames=6, n_points=160, width=376, height=240, border=12, model=model)
    pb.interp = interp
    return pb


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_composition_reproduces_the_oracle_at_the_cameras(model, interp):
    pb = problem(model, interp)
    P = pb.P
    rec, valid, _ = PIR.compose(pb, pb.intrinsics)
    ref, vref = O.evaluate(pb)
    assert np.array_equal(valid.astype(bool), vref.astype(bool))
    m = vref.astype(bool)
    assert m.sum() > 0.9 * pb.n_blocks
    dr = np.abs(rec[m, :P] - ref[m, :P]).max()
    print("r", dr)
    assert dr <= 1e-9
    for name, lo, hi in (("J_host", P, 7 * P), ("J_target", 7 * P, 13 * P), ("J_rho", 13 * P, 14 * P)):
        scale = np.abs(ref[m, lo:hi]).max(1, keepdims=True)
        e = (np.abs(rec[m, lo:hi] - ref[m, lo:hi]) / np.maximum(scale, 1e-300)).max()
        print(name, e)
        assert e <= 1e-10, name
    Ji = PIR.split(rec, P)[4]
    assert np.all(Ji[:, :, PIR.N_USED[model]:] == 0.0)
    assert np.abs(Ji[m][:, :, :PIR.N_USED[model]]).max(axis=(0, 1)).min() > 0.0  # every used column is populated
    assert np.all(rec[~m] == 0.0)


@pytest.mark.parametrize("model", MODELS)
def test_intrinsics_jacobian_matches_central_differences(model):
    pb = problem(model, 0)
    P = pb.P
    K = PIR.perturbed_state(pb)
    rec, valid, uv = PIR.compose(pb, K)
    m = valid.astype(bool)
    Ji = PIR.split(rec, P)[4]
    cell = np.floor(uv)
    for j in range(PIR.N_USED[model]):
        h = 1e-3 if j < 4 else 1e-6
        Kp, Km = K.copy(), K.copy()
        Kp[:, j] += h
        Km[:, j] -= h
        rp, vp, uvp = PIR.compose(pb, Kp, want_jac=False)
        rm, vm, uvm = PIR.compose(pb, Km, want_jac=False)
        keep = (m & vp.astype(bool) & vm.astype(bool))[:, None] & (np.floor(uvp) == cell).all(-1) & \
            (np.floor(uvm) == cell).all(-1)
        frac = keep.sum() / (m.sum() * P)
        fd = (rp[:, :P] - rm[:, :P]) / (2 * h)
        err = np.abs(fd - Ji[:, :, j])[keep].max() / np.abs(Ji[:, :, j][keep]).max()
        print(f"model {model} column {j}: kept {frac:.4f}, error {err:.3e} of the column's largest entry")
        assert frac > 0.95
        assert err <= 1e-7


def test_photometric_intrinsics_cost_compiles_against_ceres_interface():
    E = engine_module()
    E.build()
    libdir = os.path.dirname(E.LIB_PATH)
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "photometric_intrinsics_adapter_driver")
        cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
               "-I", os.path.join(ROOT, "tests", "cpp", "mock_ceres"), DRIVER_SRC, "-o", exe,
               "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"]
        subprocess.run(cmd, check=True, capture_output=True, text=True)
        assert os.path.exists(exe)
