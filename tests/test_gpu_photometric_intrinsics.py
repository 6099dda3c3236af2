"""Free target intrinsics on a photometric engine: pba_set_optimize_intrinsics(engine, 1) with PBA_RESIDUAL_PHOTOMETRIC.

The target camera projects with the intrinsics state, the host keeps unprojecting with pba_set_cameras' values, and every
record grows to 22·P floats [r | J_host | J_target | J_rho | J_intr (P×8)] with J_intr row k = ∇I · ∂π/∂k at p̃_k.

Reference: tests/photometric_intrinsics_reference.py, the oracle's geometric intrinsics evaluation composed with its
interpolator (pinned on the CPU by tests/test_photometric_intrinsics_reference.py).  Base problem: 6 keyframes, 161 points,
376×240, 644 blocks — 4 past a multiple of the 32 blocks of a workgroup.  State: the cameras × (1 + 1e-3·[1, −1, 0.5,
−0.5]) on fx, fy, cx, cy, ±1e-3 on the model's first two distortion terms, ±1e-4 on KB4's last two.

Bounds (tests/helpers.py): |Δr| ≤ 1e-4, each Jacobian block — J_intr on its own — within 1e-5 of its block's largest
reference entry, validity identical; bilinear pixels within 2e-3 px of a cell edge are left out of the Jacobian
comparison (at most 2 % of them), none for bicubic.
"""
import ctypes as C
import dataclasses
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import oracle as O
import photometric_intrinsics_reference as PIR
from helpers import ROOT, compare_records, engine_module, projected_uv, synth

pytestmark = pytest.mark.gpu
E = engine_module()
MODELS = [synth.PINHOLE, synth.DOUBLE_SPHERE, synth.EUCM, synth.KB4]
INVALID_ARGUMENT = "invalid argument"


def pattern(P):
    if P == 8:
        return synth.PATTERN8
    if P == 1:
        return np.zeros((1, 2), np.float32)
    return np.random.default_rng(P).integers(-3, 4, (P, 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(model=synth.PINHOLE, interp=0, P=8, cams=1):
    kw = {}
    if cams == 2:  # a rig of two cameras 2 % apart, alternating over the keyframes
        k0 = np.array(synth.DEFAULT_INTRINSICS[model], np.float64)
        k0[:4] *= 376 / 752.0
        k1 = k0.copy()
        k1[:4] *= 1.02
        kw = dict(intrinsics=np.stack([k0, k1]), frame_cam=np.arange(6) % 2)
    pb = synth.make_problem(n_frames=6, n_points=161, width=376, height=240, border=12, model=model,
                            pattern=pattern(P), **kw)
    pb.interp = interp
    return pb


def state(pb):
    K = PIR.perturbed_state(pb)
    if K.shape[0] == 2:  # the second camera's state perturbed the other way
        K[1] = PIR.perturbed_state(pb, -1.0)[1]
    return K


@functools.lru_cache(maxsize=None)
def reference(model=synth.PINHOLE, interp=0, P=8, cams=1):
    pb = problem(model, interp, P, cams)
    return PIR.compose(pb, state(pb))


def open_engine(pb, K=None, huber=0.0):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber)
    eng.set_problem(pb)
    eng.set_optimize_intrinsics(True)
    if K is not None:
        eng.set_intrinsics_state(K)
    return eng


def evaluate(eng, pb, path, jac=True, poses=None):
    """One evaluation at the problem's state: set_state + evaluate, or evaluate_state_device (the fused prologue that
    also adopts the state)."""
    poses = pb.poses if poses is None else poses
    if path == "host":
        eng.set_state(poses, pb.rho)
        eng.evaluate(jac)
        return
    import torch
    p = torch.from_numpy(np.ascontiguousarray(poses)).cuda()
    r = torch.from_numpy(np.ascontiguousarray(pb.rho)).cuda()
    eng._keep += [p, r]
    eng.evaluate_state_device(p.data_ptr(), r.data_ptr(), jac)


# 1. all 22·P columns, every model and interpolator, both evaluation entry points
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_all_columns_match_the_composition(model, interp, path):
    pb = problem(model, interp)
    ref, vref, uv = reference(model, interp)
    with open_engine(pb, state(pb)) as eng:
        assert eng.record_floats == 22 * pb.P
        evaluate(eng, pb, path)
        rec, valid = eng.records()
    assert rec.shape == (pb.n_blocks, 22 * pb.P) and vref.sum() > 0.9 * pb.n_blocks
    PIR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=interp == 0)
    Ji = E.split_record(rec, pb.P)[4]
    assert Ji.shape == (pb.n_blocks, pb.P, 8)
    assert np.all(Ji[:, :, PIR.N_USED[model]:] == 0.0)  # parameters the model does not use: exact zeros


def test_states_device_evaluates_at_the_state():
    """pba_evaluate_states_device: two states back to back, the records hold the last one's evaluation."""
    import torch
    pb = problem()
    ref, vref, uv = reference()
    other = synth.se3_plus(pb.poses, 1e-3 * np.random.default_rng(3).normal(0, 1, (pb.n_frames, 6)))
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (other, pb.poses, pb.rho)]
    with open_engine(pb, state(pb)) as eng:
        eng.evaluate_states_device([t[0].data_ptr(), t[1].data_ptr()], [t[2].data_ptr(), t[2].data_ptr()])
        rec, valid = eng.records()
    PIR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=True)


# 2. two cameras: the host side keeps the cameras, the target side takes its own camera's state
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("model", [synth.PINHOLE, synth.DOUBLE_SPHERE])
def test_two_cameras(model, path):
    pb = problem(model, 0, 8, 2)
    ref, vref, uv = reference(model, 0, 8, 2)
    with open_engine(pb, state(pb)) as eng:
        evaluate(eng, pb, path)
        rec, valid = eng.records()
        assert np.array_equal(eng.get_intrinsics(), state(pb))
    assert vref.sum() > 0.9 * pb.n_blocks
    PIR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=True)


# 3. pattern sizes: the 8-lane kernel with dead lanes (1, 5), 2, 3 and 4 pixels per lane, 256 and 128 threads; one
# camera (the one-camera variant) and two (the camera-table variant)
@pytest.mark.parametrize("cams", [1, 2])
@pytest.mark.parametrize("P", [1, 5, 9, 16, 21, 32])
def test_pattern_sizes(P, cams):
    pb = problem(synth.PINHOLE, 0, P, cams)
    ref, vref, uv = reference(synth.PINHOLE, 0, P, cams)
    with open_engine(pb, state(pb)) as eng:
        assert (eng.record_floats, eng.record_bytes) == (22 * P, 88 * P)
        evaluate(eng, pb, "device")
        rec, valid = eng.records()
        eng.evaluate(False)  # residual-only at the adopted state: r at the 22·P stride
        r_only, v_only = eng.records()
    assert vref.sum() > 0.8 * pb.n_blocks
    PIR.compare(P, rec, ref, valid, vref, uv, bilinear=True)
    assert np.array_equal(v_only, valid)
    assert np.abs(r_only[:, :P] - ref[:, :P]).max() <= 1e-4


# 4. block counts: one block, and one block past a workgroup
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("n_blocks", [1, 33])
def test_block_counts(n_blocks, path):
    base = problem()
    ref, vref, uv = reference()
    pb = dataclasses.replace(base, block_point=base.block_point[:n_blocks], block_target=base.block_target[:n_blocks])
    with open_engine(pb, state(base)) as eng:
        evaluate(eng, pb, path)
        rec, valid = eng.records()
    assert rec.shape == (n_blocks, 22 * pb.P) and vref[:n_blocks].all()
    # (8 and 264 pixels: the 2 % ceiling on cell-edge pixels is a statement about the whole problem, asserted there)
    PIR.compare(pb.P, rec, ref[:n_blocks], valid, vref[:n_blocks], uv[:n_blocks], bilinear=True, max_masked=1.0)


# 5. a non-finite pose: its blocks are invalid with zero records, the rest keep parity
@pytest.mark.parametrize("P", [8, 21])
def test_non_finite_pose(P):
    pb = problem(synth.PINHOLE, 0, P)
    poses = pb.poses.copy()
    poses[3, 5] = np.nan
    touched = (pb.point_host[pb.block_point] == 3) | (pb.block_target == 3)
    ref, vref, uv = PIR.compose(pb, state(pb), poses=poses)
    assert touched.any() and not vref[touched].any() and vref[~touched].sum() > 0.8 * (~touched).sum()
    with open_engine(pb, state(pb)) as eng:
        evaluate(eng, pb, "host", poses=poses)
        rec, valid = eng.records()
    assert not valid[touched].any()
    assert np.all(rec[~valid.astype(bool)] == 0.0) and rec.shape[1] == 22 * P
    PIR.compare(P, rec, ref, valid, vref, np.nan_to_num(uv), bilinear=True)


# 6. residual-only evaluation: r at the 22·P stride, pba_get_residuals and the Huber block costs at the state
def test_residual_only_evaluation():
    pb = problem()
    ref, vref, _ = reference()
    m = vref.astype(bool)
    with open_engine(pb, state(pb), huber=9.0) as eng:
        evaluate(eng, pb, "host", jac=False)
        rec, valid = eng.records()
        res, v_res = eng.residuals()
        costs = eng.block_costs()
        total, n_valid = eng.cost()
        evaluate(eng, pb, "host", jac=True)
        res_j, _ = eng.residuals()  # after a Jacobian evaluation: the pitched copy out of the 22·P records
    assert rec.shape == (pb.n_blocks, 22 * pb.P)
    assert np.array_equal(valid, vref) and np.array_equal(v_res, vref) and n_valid == m.sum()
    assert np.array_equal(rec[:, :pb.P].view(np.uint32), res.view(np.uint32))
    assert np.abs(res[m] - ref[m, :pb.P]).max() <= 1e-4 and np.all(res[~m] == 0.0)
    assert np.abs(res_j[m] - ref[m, :pb.P]).max() <= 1e-4
    for b in range(pb.n_blocks):
        if not m[b]:
            assert costs[b] == 0
            continue
        c_ref, _ = O.huber_block(ref[b, :pb.P], 9.0)
        # the bound the residual tolerance implies, as tests/test_gpu_parity.py: |Δ½Σr²| ≤ Σ|r|·δr (+ fp32 summation)
        assert abs(costs[b] - c_ref) <= 1e-4 * np.abs(ref[b, :pb.P]).sum() + 1e-5 * abs(c_ref) + 1e-5, (b, costs[b], c_ref)
    assert abs(total - float(costs.astype(np.float64).sum())) <= 1e-6 * abs(total)


# 7. sizes and read-back paths; switching free intrinsics off restores the 14·P records
def test_sizes_and_read_back_paths():
    import torch
    pb = problem()
    P, nb = pb.P, pb.n_blocks
    with E.Engine(pb.kind, pb.model) as eng:
        eng.set_problem(pb)
        assert (eng.record_floats, eng.record_bytes) == (14 * P, 56 * P)
        eng.set_optimize_intrinsics(True)
        assert np.array_equal(eng.get_intrinsics(), pb.intrinsics)  # the state starts at the cameras' values
        eng.set_intrinsics_state(state(pb))
        assert (eng.record_floats, eng.record_bytes) == (22 * P, 88 * P)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        assert rec.shape == (nb, 22 * P)
        raw = eng.records_raw()
        assert raw.dtype == np.float32 and np.array_equal(raw.view(np.uint32), rec.view(np.uint32))
        out = torch.full((nb * 22 * P + 8,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.decode_records_device(out.data_ptr() + 16)
        eng.synchronize()
        dec = out.cpu().numpy()
        assert np.isnan(dec[:4]).all() and np.isnan(dec[4 + rec.size:]).all()  # nothing written around the records
        assert np.array_equal(dec[4:4 + rec.size].view(np.uint32), rec.reshape(-1).view(np.uint32))
        L, h = eng._L, eng._h
        L.pba_get_records_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.pba_wait_records.argtypes = [C.c_void_p, C.c_int32]
        buf = C.c_void_p()
        assert L.pba_host_alloc(C.c_size_t(rec.nbytes + nb), C.byref(buf)) == 0
        try:
            assert L.pba_get_records_async(h, buf, C.c_void_p(buf.value + rec.nbytes), 64) == 0  # 11 chunks
            assert L.pba_wait_records(h, nb - 1) == 0
            got = np.frombuffer((C.c_float * rec.size).from_address(buf.value), np.float32).reshape(rec.shape)
            assert np.array_equal(got.view(np.uint32), rec.view(np.uint32))
            got_v = np.frombuffer((C.c_uint8 * nb).from_address(buf.value + rec.nbytes), np.uint8)
            assert np.array_equal(got_v, valid)
        finally:
            L.pba_host_free(buf)
        eng.set_optimize_intrinsics(False)  # back to the cameras and the 14·P records
        assert (eng.record_floats, eng.record_bytes) == (14 * P, 56 * P)
        evaluate(eng, pb, "host")
        rec14, valid14 = eng.records()
    assert rec14.shape == (nb, 14 * P)
    ref14, vref14 = O.evaluate(pb)
    compare_records(0, P, rec14, ref14, valid14, vref14, projected_uv(pb))


# 8. pyramid level 1: the target projects with the level-1 image of the state, J_intr stays ∂/∂(level-0 state)
@pytest.mark.parametrize("model", [synth.PINHOLE, synth.KB4])
def test_pyramid_level_1(model):
    pb = problem(model)
    K = state(pb)
    with open_engine(pb, K) as eng:
        eng.build_pyramid(2)
        eng.set_level(1)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        hi = eng.host_intensities()
        assert np.array_equal(eng.get_intrinsics(), K)  # the level-0 state, whatever level is active
        eng.set_intrinsics_state(pb.intrinsics)         # a new state at level 1 …
        eng.set_intrinsics_state(K)                     # … and back: the level's device copy follows
        evaluate(eng, pb, "device")
        rec_b, valid_b = eng.records()
        eng.set_level(0)
        evaluate(eng, pb, "host")
        rec0, valid0 = eng.records()
    lp = synth.level_problem(pb, 1)
    assert np.abs(hi - lp.host_intensity).max() <= 1e-3
    lp.host_intensity = hi
    ref, vref, uv = PIR.compose(lp, PIR.level_state(K, 1))
    Ji = PIR.split(ref, pb.P)[4]
    Ji[:, :, :4] *= 0.5  # ∂(fx, fy, cx, cy at level 1)/∂(level-0 state) = ½ (a view: ref is scaled in place)
    assert vref.sum() > 0.8 * pb.n_blocks
    PIR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=True)
    PIR.compare(pb.P, rec_b, ref, valid_b, vref, uv, bilinear=True)
    ref0, vref0, uv0 = reference(model)
    PIR.compare(pb.P, rec0, ref0, valid0, vref0, uv0, bilinear=True)


# 9. the calibration comes back: Gauss-Newton on the four pinhole intrinsics from the engine's r and J_intr
def calibration_run(evaluate_at, K0, n_iter=4):
    K, costs = K0.copy(), []
    for _ in range(n_iter):
        rec, valid = evaluate_at(K)
        m = valid.astype(bool)
        r = rec[m, :8].astype(np.float64).reshape(-1)
        J = rec[m, 14 * 8:].astype(np.float64).reshape(-1, 8)[:, :4]
        costs.append(0.5 * float(r @ r))
        K[0, :4] -= np.linalg.solve(J.T @ J, J.T @ r)
    return costs, K


def test_calibration_comes_back():
    pb = synth.make_problem(n_frames=6, n_points=160, width=376, height=240, border=12, model=synth.PINHOLE,
                            perturb=False, seed=11)
    pb.interp = 1
    K0 = pb.intrinsics.copy()
    K0[0, :4] = [K0[0, 0] * 1.005, K0[0, 1] * 0.995, K0[0, 2] + 0.6, K0[0, 3] - 0.4]
    c_ref, K_ref = calibration_run(lambda K: PIR.compose(pb, K)[:2], K0)
    print("reference costs", c_ref, "final error", np.abs(K_ref - pb.intrinsics).max())
    assert c_ref[0] > 100 * c_ref[-1] and np.abs(K_ref - pb.intrinsics).max() < 0.01
    with open_engine(pb) as eng:
        eng.set_state(pb.poses, pb.rho)

        def at(K):
            eng.set_intrinsics_state(K)
            eng.evaluate(True)
            return eng.records()

        c_eng, K_eng = calibration_run(at, K0)
    print("engine costs", c_eng, "difference of the final intrinsics", np.abs(K_eng - K_ref).max())
    for a, b in zip(c_eng, c_ref):
        assert abs(a - b) <= 1e-3 * b
    assert np.abs(K_eng - K_ref).max() <= 1e-3


# 10. refusals: half records with free intrinsics (either order), the on-device solve; the engine stays usable
def test_refusals():
    pb = problem()
    ref, vref, uv = reference()
    for fmt in (E.RECORD_F16, E.RECORD_F16_SCALED):
        with open_engine(pb, state(pb)) as eng:
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.set_record_format(fmt)
            assert eng.record_format == E.RECORD_F32
            evaluate(eng, pb, "host")
            rec, valid = eng.records()
            PIR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=True)
        with E.Engine(pb.kind, pb.model) as eng:
            eng.set_problem(pb)
            eng.set_record_format(fmt)
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.set_optimize_intrinsics(True)
            assert eng.record_floats == 14 * pb.P and eng.record_format == fmt
            evaluate(eng, pb, "host")
            rec, valid = eng.records()
            assert rec.shape == (pb.n_blocks, 14 * pb.P) and np.array_equal(valid, O.evaluate(pb)[1])
    with open_engine(pb, state(pb)) as eng:
        eng.set_state(pb.poses, pb.rho)
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.gn_linearize()
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.solve(max_iterations=2)
        with pytest.raises(E.PbaError, match="free intrinsics"):
            eng.solve_pyramid(max_iterations=2)
        eng.evaluate(True)
        rec, valid = eng.records()
        PIR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=True)
        eng.set_optimize_intrinsics(False)  # with the intrinsics fixed again the on-device solve runs
        assert eng.gn_linearize() > 0.0


# 11. the Ceres drop-in: GpuPhotometricIntrinsicsCost<8> hands jacobians[3] the records' tail
def test_adapter_photometric_intrinsics_cost():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden import write_problem
    pb = problem()
    ref, vref, uv = reference()
    P, nb = pb.P, pb.n_blocks
    libdir = os.path.dirname(E.LIB_PATH)
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "photometric_intrinsics_adapter_driver")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "tests", "cpp", "mock_ceres"),
                        os.path.join(ROOT, "tests", "cpp", "photometric_intrinsics_adapter_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"],
                       check=True, capture_output=True, text=True)
        fin, fk, fout = (os.path.join(td, n) for n in ("in.bin", "state.bin", "out.bin"))
        with open(fin, "wb") as f:
            write_problem(f, pb)
        state(pb).astype(np.float64).tofile(fk)
        subprocess.run([exe, fin, fk, fout], check=True)
        raw = np.fromfile(fout, np.uint8)
    o = 0
    out22 = raw[o:o + 8 * nb * 22 * P].view(np.float64).reshape(nb, 22 * P); o += 8 * nb * 22 * P
    valid22 = raw[o:o + nb]; o += nb
    out14 = raw[o:o + 8 * nb * 14 * P].view(np.float64).reshape(nb, 14 * P); o += 8 * nb * 14 * P
    valid14 = raw[o:o + nb]; o += nb
    flags = raw[o:o + 12].view(np.int32)
    assert o + 12 == raw.size
    PIR.compare(P, out22, ref, valid22, vref, uv, bilinear=True)
    # with jacobians[3] == nullptr the other three blocks are unchanged
    assert np.array_equal(valid14, valid22) and np.array_equal(out14, out22[:, :14 * P])
    # an evaluator without the intrinsics blocks refuses the request (and only that)
    assert flags.tolist() == [1, 1, 1]
