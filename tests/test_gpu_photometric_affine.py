"""Affine brightness per keyframe on a photometric engine: pba_set_affine_brightness(engine, 1).

With the affine state [a_0 b_0 a_1 b_1 …], h the block's host, t its target and E = exp(a_t − a_h),
r_k = (I_t(π(p̃_k)) − b_t) − E·(I_h,k − b_h), and every record grows to 18·P floats
[r | J_host | J_target | J_rho | J_ab_host (P×2) | J_ab_target (P×2)], J_ab_host row k = [E·(I_h,k − b_h), E],
J_ab_target row k = [−E·(I_h,k − b_h), −1].

Reference: tests/photometric_affine_reference.py, composed in double from the oracle's plain photometric evaluation
(pinned on the CPU by tests/test_photometric_affine_reference.py).  Base problem: 6 keyframes, 161 points, 376×240,
644 blocks — 4 past a multiple of the 32 blocks of a workgroup.  State: a_f uniform in [−0.3, 0.3], b_f uniform in
[−20, 20], fixed seed, frame 0 included.

Bounds (tests/helpers.py): |Δr| ≤ 1e-4, each Jacobian block — J_ab_host and J_ab_target each on its own — within 1e-5 of
its block's largest reference entry, validity identical; bilinear pixels within 2e-3 px of a cell edge are left out of
the Jacobian comparison (at most 2 % of them), none for bicubic.
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
import photometric_affine_reference as PAR
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
    if cams > 1:  # a rig of cameras 2 % apart each, dealt round-robin over the keyframes
        k0 = np.array(synth.DEFAULT_INTRINSICS[model], np.float64)
        k0[:4] *= 376 / 752.0
        ks = np.stack([k0] * cams)
        ks[:, :4] *= (1.0 + 0.02 * np.arange(cams))[:, None]
        kw = dict(intrinsics=ks, frame_cam=np.arange(6) % cams)
    pb = synth.make_problem(n_frames=6, n_points=161, width=376, height=240, border=12, model=model,
                            pattern=pattern(P), **kw)
    pb.interp = interp
    return pb


def state(pb):
    return PAR.parity_state(pb.n_frames)


@functools.lru_cache(maxsize=None)
def reference(model=synth.PINHOLE, interp=0, P=8, cams=1):
    pb = problem(model, interp, P, cams)
    return PAR.compose(pb, state(pb))


def open_engine(pb, ab=None, huber=0.0):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber)
    eng.set_problem(pb)
    eng.set_affine_brightness(True)
    if ab is not None:
        eng.set_affine_state(ab)
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


# 1. all 18·P columns, every model and interpolator, both evaluation entry points
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_all_columns_match_the_composition(model, interp, path):
    pb = problem(model, interp)
    ref, vref, uv = reference(model, interp)
    with open_engine(pb, state(pb)) as eng:
        assert eng.record_floats == 18 * pb.P
        evaluate(eng, pb, path)
        rec, valid = eng.records()
    assert rec.shape == (pb.n_blocks, 18 * pb.P) and vref.sum() > 0.9 * pb.n_blocks
    PAR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=interp == 0)
    parts = E.split_record(rec, pb.P)
    assert len(parts) == 6 and parts[4].shape == parts[5].shape == (pb.n_blocks, pb.P, 2)
    assert np.all(parts[5][valid.astype(bool)][:, :, 1] == np.float32(-1.0))


# 2. pba_evaluate_states_device: two states back to back, the records hold the last one's evaluation
def test_states_device_evaluates_at_the_state():
    import torch
    pb = problem()
    ref, vref, uv = reference()
    other = synth.se3_plus(pb.poses, 1e-3 * np.random.default_rng(3).normal(0, 1, (pb.n_frames, 6)))
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (other, pb.poses, pb.rho)]
    with open_engine(pb, state(pb)) as eng:
        eng.evaluate_states_device([t[0].data_ptr(), t[1].data_ptr()], [t[2].data_ptr(), t[2].data_ptr()])
        rec, valid = eng.records()
    PAR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=True)


# 3. pattern sizes: the 8-lane kernel with dead lanes (1, 5), 2, 3 and 4 pixels per lane, 256 and 128 threads, odd P;
# one camera (the one-camera variant) and two (the camera-table variant)
@pytest.mark.parametrize("cams", [1, 2])
@pytest.mark.parametrize("P", [1, 5, 9, 16, 21, 32])
def test_pattern_sizes(P, cams):
    pb = problem(synth.PINHOLE, 0, P, cams)
    ref, vref, uv = reference(synth.PINHOLE, 0, P, cams)
    with open_engine(pb, state(pb)) as eng:
        assert (eng.record_floats, eng.record_bytes) == (18 * P, 72 * P)
        evaluate(eng, pb, "device")
        rec, valid = eng.records()
        eng.evaluate(False)  # residual-only at the adopted state: r at the 18·P stride
        r_only, v_only = eng.records()
        evaluate(eng, pb, "host")  # set_state + evaluate: the same launch at the engine's own state
        rec_h, valid_h = eng.records()
    assert vref.sum() > 0.8 * pb.n_blocks
    PAR.compare(P, rec, ref, valid, vref, uv, bilinear=True)
    assert np.array_equal(v_only, valid)
    assert np.abs(r_only[:, :P] - ref[:, :P]).max() <= 1e-4
    assert np.array_equal(rec_h.view(np.uint32), rec.view(np.uint32)) and np.array_equal(valid_h, valid)


# five cameras are past the LDS camera table (4): the 256-thread kernel with the cameras in every tile block
def test_more_cameras_than_the_table():
    pb = problem(synth.PINHOLE, 0, 16, 5)
    ref, vref, uv = reference(synth.PINHOLE, 0, 16, 5)
    with open_engine(pb, state(pb)) as eng:
        evaluate(eng, pb, "device")
        rec, valid = eng.records()
    assert vref.sum() > 0.8 * pb.n_blocks
    PAR.compare(16, rec, ref, valid, vref, uv, bilinear=True)


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
    assert rec.shape == (n_blocks, 18 * pb.P) and vref[:n_blocks].all()
    # (8 and 264 pixels: the 2 % ceiling on cell-edge pixels is a statement about the whole problem, asserted there)
    PAR.compare(pb.P, rec, ref[:n_blocks], valid, vref[:n_blocks], uv[:n_blocks], bilinear=True, max_masked=1.0)


# 5. a non-finite pose, and a non-finite a_f: that keyframe's blocks are invalid with zero records, the rest keep parity
@pytest.mark.parametrize("what", ["pose", "a"])
@pytest.mark.parametrize("P", [8, 21])
def test_non_finite_keyframe(P, what):
    pb = problem(synth.PINHOLE, 0, P)
    poses, ab = pb.poses.copy(), state(pb)
    if what == "pose":
        poses[3, 5] = np.nan
    else:
        ab[3, 0] = np.nan
    touched = (pb.point_host[pb.block_point] == 3) | (pb.block_target == 3)
    ref, vref, uv = PAR.compose(pb, ab, poses=poses)
    assert touched.any() and not vref[touched].any() and vref[~touched].sum() > 0.8 * (~touched).sum()
    with open_engine(pb, ab) as eng:
        evaluate(eng, pb, "host", poses=poses)
        rec, valid = eng.records()
    assert np.array_equal(valid.astype(bool), ~touched & vref.astype(bool))
    assert np.all(rec[~valid.astype(bool)] == 0.0) and rec.shape[1] == 18 * P
    PAR.compare(P, rec, ref, valid, vref, np.nan_to_num(uv), bilinear=True)


# 6. residual-only evaluation: r at the 18·P stride, pba_get_residuals and the Huber block costs on the new r
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
        res_j, _ = eng.residuals()  # after a Jacobian evaluation: the pitched copy out of the 18·P records
    assert rec.shape == (pb.n_blocks, 18 * pb.P)
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


# 7. the zero state: the first 14·P values, validity and costs are those of a plain engine, bit for bit
@pytest.mark.parametrize("P", [8, 21])
def test_zero_state_is_the_plain_record(P):
    pb = problem(synth.PINHOLE, 0, P)
    with E.Engine(pb.kind, pb.model, huber_width=9.0) as eng:
        eng.set_problem(pb)
        evaluate(eng, pb, "host")
        rec14, valid14 = eng.records()
        costs14 = eng.block_costs()
    with open_engine(pb, None, huber=9.0) as eng:
        assert np.all(eng.get_affine_state() == 0.0)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        costs = eng.block_costs()
        eng.set_affine_brightness(False)  # back to the 14·P records
        assert (eng.record_floats, eng.record_bytes) == (14 * P, 56 * P)
        evaluate(eng, pb, "host")
        rec_off, valid_off = eng.records()
    assert rec14.shape == (pb.n_blocks, 14 * P) and rec.shape == (pb.n_blocks, 18 * P) and valid14.sum() > 0.8 * pb.n_blocks
    assert np.array_equal(rec[:, :14 * P].view(np.uint32), rec14.view(np.uint32))
    assert np.array_equal(valid, valid14) and np.array_equal(costs.view(np.uint32), costs14.view(np.uint32))
    m = valid.astype(bool)
    Jh, Jt = E.split_record(rec, P)[4:]
    assert np.array_equal(Jh[m][:, :, 0], pb.host_intensity[pb.block_point][m]) and np.all(Jh[m][:, :, 1] == 1.0)
    assert np.array_equal(Jt[m][:, :, 0], -Jh[m][:, :, 0]) and np.all(Jt[m][:, :, 1] == -1.0)
    assert np.array_equal(rec_off.view(np.uint32), rec14.view(np.uint32)) and np.array_equal(valid_off, valid14)
    ref14, vref14 = O.evaluate(pb)
    compare_records(0, P, rec_off, ref14, valid_off, vref14, projected_uv(pb))


# 8. sizes and read-back paths; the affine state through the host and the device setter
def test_sizes_and_read_back_paths():
    import torch
    pb = problem()
    P, nb = pb.P, pb.n_blocks
    ab = state(pb)
    with E.Engine(pb.kind, pb.model) as eng:
        with pytest.raises(E.PbaError, match="not ready"):  # before pba_set_frames
            eng._ck(eng._L.pba_set_affine_state(eng._h, C.c_void_p(ab.ctypes.data)), "pba_set_affine_state")
        eng.set_problem(pb)
        assert (eng.record_floats, eng.record_bytes) == (14 * P, 56 * P)
        eng.set_affine_brightness(True)
        assert (eng.record_floats, eng.record_bytes) == (18 * P, 72 * P)
        assert np.all(eng.get_affine_state() == 0.0)  # the state starts at zeros
        eng.set_affine_state(ab)
        assert np.array_equal(eng.get_affine_state(), ab)
        d_ab = torch.from_numpy(-ab).cuda()
        eng.set_affine_state_device(d_ab.data_ptr())
        assert np.array_equal(eng.get_affine_state(), -ab)
        eng.set_affine_state(ab)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        assert rec.shape == (nb, 18 * P)
        raw = eng.records_raw()
        assert raw.dtype == np.float32 and np.array_equal(raw.view(np.uint32), rec.view(np.uint32))
        d_rec, d_valid, _ = eng.device_records()  # the engine's own device arrays: 18·P floats per block
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        dev, dev_v = np.empty_like(rec), np.empty_like(valid)
        assert hip.hipMemcpy(dev.ctypes.data, d_rec, rec.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        assert hip.hipMemcpy(dev_v.ctypes.data, d_valid, nb, 2) == 0
        assert np.array_equal(dev.view(np.uint32), rec.view(np.uint32)) and np.array_equal(dev_v, valid)
        out = torch.full((nb * 18 * P + 8,), float("nan"), dtype=torch.float32, device="cuda")
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
        eng.set_problem(pb)  # pba_set_frames resets the state to zeros
        assert np.all(eng.get_affine_state() == 0.0) and eng.record_floats == 18 * P
    ref, vref, uv = reference()
    PAR.compare(P, rec, ref, valid, vref, uv, bilinear=True)


# 9. pyramid level 1: (a, b) are shared by the levels, no level factor
def test_pyramid_level_1():
    pb = problem()
    ab = state(pb)
    with open_engine(pb, ab) as eng:
        eng.build_pyramid(2)
        eng.set_level(1)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        hi = eng.host_intensities()
        assert np.array_equal(eng.get_affine_state(), ab)
        evaluate(eng, pb, "device")
        rec_b, valid_b = eng.records()
        eng.set_level(0)
        evaluate(eng, pb, "host")
        rec0, valid0 = eng.records()
    lp = synth.level_problem(pb, 1)
    assert np.abs(hi - lp.host_intensity).max() <= 1e-3
    lp.host_intensity = hi
    lp.interp = 0
    ref, vref, uv = PAR.compose(lp, ab)
    assert vref.sum() > 0.8 * pb.n_blocks
    PAR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=True)
    PAR.compare(pb.P, rec_b, ref, valid_b, vref, uv, bilinear=True)
    ref0, vref0, uv0 = reference()
    PAR.compare(pb.P, rec0, ref0, valid0, vref0, uv0, bilinear=True)


# 10. brightness comes back: Gauss-Newton on (a_f, b_f), f ≥ 1, from the engine's r and brightness columns tracks the
# reference run (tests/test_photometric_affine_reference.py has the reference run's own figures)
def test_brightness_comes_back():
    pb, gain, offset = PAR.brightness_case()
    c_ref, ab_ref = PAR.brightness_run(lambda s: PAR.compose(pb, s)[:2], pb)
    with open_engine(pb) as eng:
        eng.set_state(pb.poses, pb.rho)

        def at(ab):
            eng.set_affine_state(ab)
            eng.evaluate(True)
            return eng.records()

        c_eng, ab_eng = PAR.brightness_run(at, pb)
    print("engine costs", c_eng, "reference costs", c_ref, "difference of the final states", np.abs(ab_eng - ab_ref).max())
    assert c_ref[0] > 100 * c_ref[-1]
    for a, b in zip(c_eng, c_ref):
        assert abs(a - b) <= 1e-3 * b
    assert np.abs(ab_eng - ab_ref).max() <= 1e-3


# 11. refusals, each leaving the engine as it was
def test_refusals():
    pb = problem()
    ref, vref, uv = reference()

    def still_works(eng):
        assert (eng.record_floats, eng.record_bytes, eng.record_format) == (18 * pb.P, 72 * pb.P, E.RECORD_F32)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        PAR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=True)

    for fmt in (E.RECORD_F16, E.RECORD_F16_SCALED):
        with open_engine(pb, state(pb)) as eng:
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.set_record_format(fmt)
            still_works(eng)
        with E.Engine(pb.kind, pb.model) as eng:
            eng.set_problem(pb)
            eng.set_record_format(fmt)
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.set_affine_brightness(True)
            assert eng.record_floats == 14 * pb.P and eng.record_format == fmt
            evaluate(eng, pb, "host")
            rec, valid = eng.records()
            assert rec.shape == (pb.n_blocks, 14 * pb.P) and np.array_equal(valid, O.evaluate(pb)[1])
    with open_engine(pb, state(pb)) as eng:  # free intrinsics second
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.set_optimize_intrinsics(True)
        still_works(eng)
    with E.Engine(pb.kind, pb.model) as eng:  # affine brightness second
        eng.set_problem(pb)
        eng.set_optimize_intrinsics(True)
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.set_affine_brightness(True)
        assert (eng.record_floats, eng.record_bytes) == (22 * pb.P, 88 * pb.P)
    with open_engine(pb, state(pb)) as eng:  # every on-device Gauss-Newton entry point
        eng.set_state(pb.poses, pb.rho)
        import torch
        ex = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
        L, h = eng._L, eng._h
        calls = {
            "gn_linearize": eng.gn_linearize,
            "gn_step": lambda: eng.gn_step(1e-4),
            "gn_candidate_cost": eng.gn_candidate_cost,
            "gn_accept": eng.gn_accept,
            "gn_system_size": eng.gn_system_size,
            "solve": lambda: eng.solve(max_iterations=2),
            "solve_pyramid": lambda: eng.solve_pyramid(max_iterations=2),
            "gn_step_export": lambda: eng._ck(L.pba_gn_step_export(h, 1e-4, 1, C.c_void_p(ex.data_ptr())), "export"),
            "gn_step_import": lambda: eng._ck(L.pba_gn_step_import(h, 1e-4, 1, C.c_void_p(ex.data_ptr()), None, None,
                                                                   None), "import"),
            "solve_distributed": lambda: eng._ck(L.pba_solve_distributed(
                h, None, 1, C.c_void_p(ex.data_ptr()), E.ALLREDUCE_FN(lambda *a: 0), None, None), "distributed"),
            "solve_distributed_comm": lambda: eng._ck(L.pba_solve_distributed_comm(h, None, 1, None, None), "comm"),
        }
        for name, call in calls.items():
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                call()
            print("refused:", name)
        eng.build_pyramid(2)
        with pytest.raises(E.PbaError, match="affine brightness"):
            eng.solve_pyramid(max_iterations=2)
        assert eng.level()[0] == 0  # refused before a level was switched
        still_works(eng)
        eng.set_affine_brightness(False)  # without it the on-device solve runs
        assert eng.gn_linearize() > 0.0
    with E.Engine(synth.GEOMETRIC, synth.PINHOLE) as eng:
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.set_affine_brightness(True)


# 12. the Ceres drop-in: GpuPhotometricAffineCost<8> hands jacobians[3] and [4] the records' tail
def test_adapter_photometric_affine_cost():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden import write_problem
    pb = problem()
    ref, vref, uv = reference()
    P, nb = pb.P, pb.n_blocks
    libdir = os.path.dirname(E.LIB_PATH)
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "photometric_affine_adapter_driver")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "tests", "cpp", "mock_ceres"),
                        os.path.join(ROOT, "tests", "cpp", "photometric_affine_adapter_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"],
                       check=True, capture_output=True, text=True)
        fin, fk, fout = (os.path.join(td, n) for n in ("in.bin", "state.bin", "out.bin"))
        with open(fin, "wb") as f:
            write_problem(f, pb)
        state(pb).astype(np.float64).tofile(fk)
        subprocess.run([exe, fin, fk, fout], check=True)
        raw = np.fromfile(fout, np.uint8)
    o = 0
    out18 = raw[o:o + 8 * nb * 18 * P].view(np.float64).reshape(nb, 18 * P); o += 8 * nb * 18 * P
    valid18 = raw[o:o + nb]; o += nb
    out14 = raw[o:o + 8 * nb * 14 * P].view(np.float64).reshape(nb, 14 * P); o += 8 * nb * 14 * P
    valid14 = raw[o:o + nb]; o += nb
    flags = raw[o:o + 12].view(np.int32)
    assert o + 12 == raw.size
    PAR.compare(P, out18, ref, valid18, vref, uv, bilinear=True)
    # with jacobians[3] == jacobians[4] == nullptr the other three blocks are unchanged
    assert np.array_equal(valid14, valid18) and np.array_equal(out14, out18[:, :14 * P])
    # an evaluator without the (a, b) blocks refuses the request (and only that)
    assert flags.tolist() == [1, 1, 1]
