"""Free target intrinsics together with affine brightness on a photometric engine:
pba_set_intrinsics_with_affine(engine, 1), then pba_set_optimize_intrinsics and pba_set_affine_brightness, either order.

Every record is 26·P floats [r | J_host | J_target | J_rho | J_intr (P×8) | J_ab_host (P×2) | J_ab_target (P×2)] with
r_k = (I_t(π_K(p̃_k)) − b_t) − E·(I_h,k − b_h): the target projects with the intrinsics state, the host unprojects with the
cameras' values, E = exp(a_t − a_h).

Reference: tests/photometric_affine_intrinsics_reference.py, the 22-column intrinsics reference with the affine residual
and brightness columns composed on top (pinned on the CPU by tests/test_photometric_affine_intrinsics_reference.py).
Base problem: 6 keyframes, 161 points, 376×240, 644 blocks — 20 workgroups of 32 blocks plus 4.  State:
PIR.perturbed_state for the intrinsics, PAR.parity_state for (a, b).

Bounds (tests/helpers.py): |Δr| ≤ 1e-4, each Jacobian block — J_intr, J_ab_host and J_ab_target each on its own — within
1e-5 of its block's largest reference entry, validity identical; bilinear pixels within 2e-3 px of a cell edge are left
out of the Jacobian comparison (at most 2 % of them), none for bicubic.
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
import photometric_affine_intrinsics_reference as PAIR
import photometric_affine_reference as PAR
import photometric_intrinsics_reference as PIR
from helpers import ROOT, engine_module, synth

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


def k_state(pb):
    K = PIR.perturbed_state(pb)
    if K.shape[0] == 2:  # the second camera's state perturbed the other way
        K[1] = PIR.perturbed_state(pb, -1.0)[1]
    return K


def ab_state(pb):
    return PAR.parity_state(pb.n_frames)


@functools.lru_cache(maxsize=None)
def reference(model=synth.PINHOLE, interp=0, P=8, cams=1):
    pb = problem(model, interp, P, cams)
    return PAIR.compose(pb, k_state(pb), ab_state(pb))


def open_engine(pb, K=None, ab=None, huber=0.0, intr_first=True):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber)
    eng.set_problem(pb)
    eng.set_intrinsics_with_affine(True)
    for first in ((True, False) if intr_first else (False, True)):
        if first:
            eng.set_optimize_intrinsics(True)
        else:
            eng.set_affine_brightness(True)
    if K is not None:
        eng.set_intrinsics_state(K)
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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# 1. all 26·P columns, every model and interpolator, both evaluation entry points
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_all_columns_match_the_composition(model, interp, path):
    pb = problem(model, interp)
    ref, vref, uv = reference(model, interp)
    with open_engine(pb, k_state(pb), ab_state(pb)) as eng:
        assert eng.record_floats == 26 * pb.P
        evaluate(eng, pb, path)
        rec, valid = eng.records()
    assert rec.shape == (pb.n_blocks, 26 * pb.P) and vref.sum() > 0.9 * pb.n_blocks
    PAIR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=interp == 0)
    parts = E.split_record(rec, pb.P)
    assert len(parts) == 7 and parts[4].shape == (pb.n_blocks, pb.P, 8)
    assert parts[5].shape == parts[6].shape == (pb.n_blocks, pb.P, 2)
    assert np.all(parts[4][:, :, PIR.N_USED[model]:] == 0.0)  # parameters the model does not use: exact zeros
    assert np.all(parts[6][valid.astype(bool)][:, :, 1] == np.float32(-1.0))


# 2. pattern sizes: the 8-lane kernel with dead lanes (1, 5), 2, 3 and 4 pixels per lane (128 threads each); odd P takes
# the 8-B form of the J_intr stage and leaves the last slab off a 16-B size; one camera and two
@pytest.mark.parametrize("cams", [1, 2])
@pytest.mark.parametrize("P", [1, 5, 9, 16, 21, 32])
def test_pattern_sizes(P, cams):
    pb = problem(synth.PINHOLE, 0, P, cams)
    ref, vref, uv = reference(synth.PINHOLE, 0, P, cams)
    with open_engine(pb, k_state(pb), ab_state(pb)) as eng:
        assert (eng.record_floats, eng.record_bytes) == (26 * P, 104 * P)
        evaluate(eng, pb, "device")
        rec, valid = eng.records()
        evaluate(eng, pb, "host")  # set_state + evaluate: the same launch at the engine's own state
        rec_h, valid_h = eng.records()
    assert vref.sum() > 0.8 * pb.n_blocks
    PAIR.compare(P, rec, ref, valid, vref, uv, bilinear=True)
    assert np.array_equal(bits(rec_h), bits(rec)) and np.array_equal(valid_h, valid)


# 3. block counts: one block, and one block past a workgroup (a short last slab: 104·P bytes, the 4-B store path for
# P = 1 — 104 B is no multiple of 16)
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("n_blocks", [1, 33])
@pytest.mark.parametrize("P", [8, 1])
def test_block_counts(P, n_blocks, path):
    base = problem(synth.PINHOLE, 0, P)
    ref, vref, uv = reference(synth.PINHOLE, 0, P)
    pb = dataclasses.replace(base, block_point=base.block_point[:n_blocks], block_target=base.block_target[:n_blocks])
    with open_engine(pb, k_state(base), ab_state(base)) as eng:
        evaluate(eng, pb, path)
        rec, valid = eng.records()
    assert rec.shape == (n_blocks, 26 * P) and vref[:n_blocks].all()
    # (a handful of pixels: the 2 % ceiling on cell-edge pixels is a statement about the whole problem, asserted there)
    PAIR.compare(P, rec, ref[:n_blocks], valid, vref[:n_blocks], uv[:n_blocks], bilinear=True, max_masked=1.0)


# 4. the zero affine state: the first 22·P columns are the record of an engine with free intrinsics only, bit for bit,
# and the last 4·P are [I_h, 1, −I_h, −1]
@pytest.mark.parametrize("P", [8, 21])
def test_zero_affine_state_is_the_intrinsics_record(P):
    pb = problem(synth.PINHOLE, 0, P)
    K = k_state(pb)
    with E.Engine(pb.kind, pb.model, huber_width=9.0) as eng:
        eng.set_problem(pb)
        eng.set_optimize_intrinsics(True)
        eng.set_intrinsics_state(K)
        evaluate(eng, pb, "host")
        rec22, valid22 = eng.records()
        costs22 = eng.block_costs()
    with open_engine(pb, K, None, huber=9.0) as eng:
        assert np.all(eng.get_affine_state() == 0.0)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        costs = eng.block_costs()
    assert rec22.shape == (pb.n_blocks, 22 * P) and rec.shape == (pb.n_blocks, 26 * P) and valid22.sum() > 0.8 * pb.n_blocks
    diff = bits(rec[:, :22 * P]) != bits(rec22)
    print("values of the first 22·P columns that differ:", int(diff.sum()), "largest difference",
          float(np.abs(rec[:, :22 * P].astype(np.float64) - rec22)[diff].max()) if diff.any() else 0.0)
    assert not diff.any()
    assert np.array_equal(valid, valid22) and np.array_equal(bits(costs), bits(costs22))
    m = valid.astype(bool)
    Jh, Jt = E.split_record(rec, P)[5:]
    assert np.array_equal(Jh[m][:, :, 0], pb.host_intensity[pb.block_point][m]) and np.all(Jh[m][:, :, 1] == 1.0)
    assert np.array_equal(Jt[m][:, :, 0], -Jh[m][:, :, 0]) and np.all(Jt[m][:, :, 1] == -1.0)


# 5. a non-finite a, pose or fx: the affected blocks are invalid with 26·P zeros, all other blocks unchanged bit for bit
@pytest.mark.parametrize("what", ["a", "pose", "fx"])
@pytest.mark.parametrize("P", [8, 21])
def test_non_finite_state(P, what):
    pb = problem(synth.PINHOLE, 0, P, 2)
    poses, K, ab = pb.poses.copy(), k_state(pb), ab_state(pb)
    host = pb.point_host[pb.block_point]
    if what == "a":
        ab[3, 0] = np.nan
        touched = (host == 3) | (pb.block_target == 3)
    elif what == "pose":
        poses[3, 5] = np.nan
        touched = (host == 3) | (pb.block_target == 3)
    else:  # the second camera's state: the blocks whose TARGET is one of its keyframes (the host keeps the cameras)
        K[1, 0] = np.nan
        touched = pb.frame_cam[pb.block_target] == 1
    assert touched.any() and not touched.all()
    with open_engine(pb, k_state(pb), ab_state(pb)) as eng:
        evaluate(eng, pb, "host")
        rec0, valid0 = eng.records()
        eng.set_intrinsics_state(K)
        eng.set_affine_state(ab)
        evaluate(eng, pb, "host", poses=poses)
        rec, valid = eng.records()
    assert valid0[~touched].sum() > 0.8 * (~touched).sum()
    assert not valid[touched].any() and np.all(rec[touched] == 0.0) and rec.shape[1] == 26 * P
    assert np.array_equal(valid[~touched], valid0[~touched])
    assert np.array_equal(bits(rec[~touched]), bits(rec0[~touched]))
    assert np.all(rec[~valid.astype(bool)] == 0.0)


# 6. residual-only evaluation: r at the 26·P stride equals the Jacobian evaluation's r bit for bit; pba_get_residuals
@pytest.mark.parametrize("P", [8, 21])
def test_residual_only_evaluation(P):
    pb = problem(synth.PINHOLE, 0, P)
    ref, vref, _ = reference(synth.PINHOLE, 0, P)
    m = vref.astype(bool)
    with open_engine(pb, k_state(pb), ab_state(pb)) as eng:
        evaluate(eng, pb, "host", jac=True)
        rec_j, valid_j = eng.records()
        res_j, _ = eng.residuals()  # after a Jacobian evaluation: the pitched copy out of the 26·P records
        evaluate(eng, pb, "host", jac=False)
        rec, valid = eng.records()
        res, v_res = eng.residuals()  # the contiguous residuals the residual-only launch also wrote
    assert rec.shape == (pb.n_blocks, 26 * P)
    assert np.array_equal(valid, vref) and np.array_equal(v_res, vref) and np.array_equal(valid_j, vref)
    assert np.array_equal(bits(rec[:, :P]), bits(rec_j[:, :P]))
    assert np.array_equal(bits(res), bits(rec[:, :P])) and np.array_equal(bits(res_j), bits(rec_j[:, :P]))
    assert np.abs(res[m] - ref[m, :P]).max() <= 1e-4 and np.all(res[~m] == 0.0)


# 7. sizes and read-back paths, in both switch orders
@pytest.mark.parametrize("intr_first", [True, False])
def test_sizes_and_read_back_paths(intr_first):
    import torch
    pb = problem()
    P, nb = pb.P, pb.n_blocks
    K, ab = k_state(pb), ab_state(pb)
    with E.Engine(pb.kind, pb.model) as eng:
        eng.set_problem(pb)
        assert (eng.record_floats, eng.record_bytes) == (14 * P, 56 * P)
        eng.set_intrinsics_with_affine(True)
        assert (eng.record_floats, eng.record_bytes) == (14 * P, 56 * P)  # the switch alone changes no record
        if intr_first:
            eng.set_optimize_intrinsics(True)
            assert (eng.record_floats, eng.record_bytes) == (22 * P, 88 * P)
            eng.set_affine_brightness(True)
        else:
            eng.set_affine_brightness(True)
            assert (eng.record_floats, eng.record_bytes) == (18 * P, 72 * P)
            eng.set_optimize_intrinsics(True)
        assert (eng.record_floats, eng.record_bytes) == (26 * P, 104 * P)
        assert np.array_equal(eng.get_intrinsics(), pb.intrinsics)  # the state starts at the cameras' values
        assert np.all(eng.get_affine_state() == 0.0)                # and (a, b) at zeros
        eng.set_intrinsics_state(K)
        eng.set_affine_state(ab)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        assert rec.shape == (nb, 26 * P)
        raw = eng.records_raw()
        assert raw.dtype == np.float32 and np.array_equal(bits(raw), bits(rec))
        d_rec, d_valid, _ = eng.device_records()  # the engine's own device arrays: 26·P floats per block
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        dev, dev_v = np.empty_like(rec), np.empty_like(valid)
        assert hip.hipMemcpy(dev.ctypes.data, d_rec, rec.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        assert hip.hipMemcpy(dev_v.ctypes.data, d_valid, nb, 2) == 0
        assert np.array_equal(bits(dev), bits(rec)) and np.array_equal(dev_v, valid)
        out = torch.full((nb * 26 * P + 8,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.decode_records_device(out.data_ptr() + 16)
        eng.synchronize()
        dec = out.cpu().numpy()
        assert np.isnan(dec[:4]).all() and np.isnan(dec[4 + rec.size:]).all()  # nothing written around the records
        assert np.array_equal(bits(dec[4:4 + rec.size]), bits(rec.reshape(-1)))
        L, h = eng._L, eng._h
        L.pba_get_records_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.pba_wait_records.argtypes = [C.c_void_p, C.c_int32]
        buf = C.c_void_p()
        assert L.pba_host_alloc(C.c_size_t(rec.nbytes + nb), C.byref(buf)) == 0
        try:
            assert L.pba_get_records_async(h, buf, C.c_void_p(buf.value + rec.nbytes), 64) == 0  # 11 chunks
            assert L.pba_wait_records(h, nb - 1) == 0
            got = np.frombuffer((C.c_float * rec.size).from_address(buf.value), np.float32).reshape(rec.shape)
            assert np.array_equal(bits(got), bits(rec))
            got_v = np.frombuffer((C.c_uint8 * nb).from_address(buf.value + rec.nbytes), np.uint8)
            assert np.array_equal(got_v, valid)
        finally:
            L.pba_host_free(buf)
        # a new problem: pba_set_frames zeroes (a, b), pba_set_cameras restarts the intrinsics state at the cameras'
        eng.set_problem(pb)
        assert np.all(eng.get_affine_state() == 0.0) and np.array_equal(eng.get_intrinsics(), pb.intrinsics)
        assert (eng.record_floats, eng.record_bytes) == (26 * P, 104 * P)
        eng.set_intrinsics_state(K)
        eng.set_affine_state(ab)
        # turning one of the two off gives the other's record back
        if intr_first:
            eng.set_affine_brightness(False)
            assert (eng.record_floats, eng.record_bytes) == (22 * P, 88 * P)
            evaluate(eng, pb, "host")
            rec1, valid1 = eng.records()
            ref1, vref1, uv1 = PIR.compose(pb, K)
            PIR.compare(P, rec1, ref1, valid1, vref1, uv1, bilinear=True)
        else:
            eng.set_optimize_intrinsics(False)
            assert (eng.record_floats, eng.record_bytes) == (18 * P, 72 * P)
            evaluate(eng, pb, "host")
            rec1, valid1 = eng.records()
            ref1, vref1, uv1 = PAR.compose(pb, ab)
            PAR.compare(P, rec1, ref1, valid1, vref1, uv1, bilinear=True)
    ref, vref, uv = reference()
    PAIR.compare(P, rec, ref, valid, vref, uv, bilinear=True)


# 8. pyramid level 1: the target projects with the level-1 image of the state, J_intr stays ∂/∂(level-0 state), (a, b)
# carry no level factor; then level 0 again
def test_pyramid_level_1():
    pb = problem()
    K, ab = k_state(pb), ab_state(pb)
    with open_engine(pb, K, ab) as eng:
        eng.build_pyramid(2)
        eng.set_level(1)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        hi = eng.host_intensities()
        assert np.array_equal(eng.get_intrinsics(), K) and np.array_equal(eng.get_affine_state(), ab)
        evaluate(eng, pb, "device")
        rec_b, valid_b = eng.records()
        eng.set_level(0)
        evaluate(eng, pb, "host")
        rec0, valid0 = eng.records()
    lp = synth.level_problem(pb, 1)
    assert np.abs(hi - lp.host_intensity).max() <= 1e-3
    lp.host_intensity = hi
    lp.interp = 0
    ref, vref, uv = PAIR.compose(lp, PIR.level_state(K, 1), ab)
    Ji = PAIR.split(ref, pb.P)[4]
    Ji[:, :, :4] *= 0.5  # ∂(fx, fy, cx, cy at level 1)/∂(level-0 state) = ½ (a view: ref is scaled in place)
    assert vref.sum() > 0.8 * pb.n_blocks
    PAIR.compare(pb.P, rec, ref, valid, vref, uv, bilinear=True)
    PAIR.compare(pb.P, rec_b, ref, valid_b, vref, uv, bilinear=True)
    ref0, vref0, uv0 = reference()
    PAIR.compare(pb.P, rec0, ref0, valid0, vref0, uv0, bilinear=True)


# 9. the per-block cost with Huber width 9 is ½ρ(Σr²) of the engine's own r (in double), within 1e-5 relative: an fp32
# sum of at most 32 squares errs below 32·2⁻²⁴ = 2e-6
@pytest.mark.parametrize("P", [8, 21])
def test_block_costs_are_the_huber_cost_of_the_new_r(P):
    pb = problem(synth.PINHOLE, 0, P)
    linear = []
    with open_engine(pb, k_state(pb), None, huber=9.0) as eng:
        # at the parity state every block's Σr² is past 81 (ρ's linear part: offsets of up to ±20 grey levels); at the
        # zero affine state some blocks stay in the quadratic part (25 of 644 at 8 px, 2 at 21 px, on the reference)
        for ab in (ab_state(pb), np.zeros((pb.n_frames, 2))):
            eng.set_affine_state(ab)
            evaluate(eng, pb, "host")
            rec, valid = eng.records()
            costs = eng.block_costs()
            total, n_valid = eng.cost()
            m = valid.astype(bool)
            assert m.sum() > 0.8 * pb.n_blocks and n_valid == m.sum() and np.all(costs[~m] == 0.0)
            expect = np.array([O.huber_block(rec[b, :P].astype(np.float64), 9.0)[0] for b in range(pb.n_blocks)])
            rel = np.abs(costs[m] - expect[m]) / expect[m]
            linear.append(np.sum(rec[m, :P].astype(np.float64) ** 2, 1) > 81.0)
            print("largest relative cost difference", float(rel.max()), "blocks in the linear part", int(linear[-1].sum()),
                  "of", int(m.sum()))
            assert rel.max() <= 1e-5
            assert abs(total - float(costs.astype(np.float64).sum())) <= 1e-6 * abs(total)
    assert linear[0].any() and not linear[1].all()  # both branches of ρ are exercised


# 10. switch rules; each refusal leaves record size, format and a following evaluation intact
def solve_calls(eng):
    import torch
    ex = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    eng._keep.append(ex)
    L, h = eng._L, eng._h
    X = C.c_void_p(ex.data_ptr())
    cb = E.ALLREDUCE_FN(lambda *a: 0)
    eng._keep.append(cb)
    return {
        "gn_linearize": eng.gn_linearize,
        "gn_step": lambda: eng.gn_step(1e-4),
        "gn_candidate_cost": eng.gn_candidate_cost,
        "gn_accept": eng.gn_accept,
        "gn_system_size": eng.gn_system_size,
        "solve": lambda: eng.solve(max_iterations=2),
        "solve_pyramid": lambda: eng.solve_pyramid(max_iterations=2),
        "gn_step_export": lambda: eng._ck(L.pba_gn_step_export(h, C.c_double(1e-4), 1, X), "export"),
        "gn_step_import": lambda: eng._ck(L.pba_gn_step_import(h, C.c_double(1e-4), 1, X, None, None, None), "import"),
        "solve_distributed": lambda: eng._ck(L.pba_solve_distributed(h, None, 1, X, cb, None, None), "distributed"),
        "solve_distributed_comm": lambda: eng._ck(L.pba_solve_distributed_comm(h, None, 1, None, None), "comm"),
        "affine_linearize": lambda: eng._ck(L.pba_affine_linearize(h, None), "affine_linearize"),
        "affine_system_size": lambda: eng._ck(L.pba_affine_system_size(h, C.byref(C.c_int32())), "affine_system_size"),
        "affine_get_system": lambda: eng._ck(L.pba_affine_get_system(h, None, None), "affine_get_system"),
        "affine_step": lambda: eng._ck(L.pba_affine_step(h, C.c_double(1e-4), None, None), "affine_step"),
        "affine_get_step": lambda: eng._ck(L.pba_affine_get_step(h, X), "affine_get_step"),
        "affine_candidate_cost": lambda: eng._ck(L.pba_affine_candidate_cost(h, C.byref(C.c_double())), "affine_cc"),
        "affine_accept": lambda: eng._ck(L.pba_affine_accept(h), "affine_accept"),
        "solve_affine": lambda: eng._ck(L.pba_solve_affine(h, None, None), "solve_affine"),
        "joint_linearize": lambda: eng._ck(L.pba_joint_linearize(h, None), "joint_linearize"),
        "joint_system_size": lambda: eng._ck(L.pba_joint_system_size(h, C.byref(C.c_int32())), "joint_system_size"),
        "joint_step": lambda: eng._ck(L.pba_joint_step(h, C.c_double(1e-4), None, None), "joint_step"),
        "joint_get_reduced_system": lambda: eng._ck(L.pba_joint_get_reduced_system(h, None, None), "joint_get_reduced"),
        "joint_get_step": lambda: eng._ck(L.pba_joint_get_step(h, None, None), "joint_get_step"),
        "joint_candidate_cost": lambda: eng._ck(L.pba_joint_candidate_cost(h, C.byref(C.c_double())), "joint_cc"),
        "joint_accept": lambda: eng._ck(L.pba_joint_accept(h), "joint_accept"),
        "solve_joint": lambda: eng._ck(L.pba_solve_joint(h, None, None), "solve_joint"),
        "joint_band": lambda: eng._ck(L.pba_joint_band(h, C.byref(C.c_int32())), "joint_band"),
        "joint_exchange_size": lambda: eng._ck(L.pba_joint_exchange_size(h, 1, C.byref(C.c_int64())), "joint_exchange_size"),
        "joint_step_export": lambda: eng._ck(L.pba_joint_step_export(h, C.c_double(1e-4), 1, X), "joint_export"),
        "joint_step_import": lambda: eng._ck(L.pba_joint_step_import(h, C.c_double(1e-4), 1, X, None, None, None), "joint_import"),
        "solve_joint_distributed": lambda: eng._ck(L.pba_solve_joint_distributed(h, None, 1, X, cb, None, None),
                                                   "joint_distributed"),
    }


def test_switch_rules():
    pb = problem()
    P = pb.P
    K, ab = k_state(pb), ab_state(pb)
    ref, vref, uv = reference()

    def still_26(eng):
        assert (eng.record_floats, eng.record_bytes, eng.record_format) == (26 * P, 104 * P, E.RECORD_F32)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        PAIR.compare(P, rec, ref, valid, vref, uv, bilinear=True)

    # default off: the mutual refusal, whichever switch comes second (as test_gpu_photometric_affine.py::test_refusals)
    ref18, vref18, uv18 = PAR.compose(pb, ab)
    with E.Engine(pb.kind, pb.model) as eng:  # free intrinsics second
        eng.set_problem(pb)
        eng.set_affine_brightness(True)
        eng.set_affine_state(ab)
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.set_optimize_intrinsics(True)
        assert (eng.record_floats, eng.record_bytes, eng.record_format) == (18 * P, 72 * P, E.RECORD_F32)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        PAR.compare(P, rec, ref18, valid, vref18, uv18, bilinear=True)
        eng.set_intrinsics_with_affine(True)   # on and off again with one switch on: allowed, and off refuses again
        eng.set_intrinsics_with_affine(False)
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.set_optimize_intrinsics(True)
        assert eng.record_floats == 18 * P
    ref22, vref22, uv22 = PIR.compose(pb, K)
    with E.Engine(pb.kind, pb.model) as eng:  # affine brightness second
        eng.set_problem(pb)
        eng.set_optimize_intrinsics(True)
        eng.set_intrinsics_state(K)
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.set_affine_brightness(True)
        assert (eng.record_floats, eng.record_bytes, eng.record_format) == (22 * P, 88 * P, E.RECORD_F32)
        evaluate(eng, pb, "host")
        rec, valid = eng.records()
        PIR.compare(P, rec, ref22, valid, vref22, uv22, bilinear=True)
    # the opt-in refused: a geometric engine; a half format active; enable = 0 while both switches are on
    with E.Engine(synth.GEOMETRIC, synth.PINHOLE) as eng:
        with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
            eng.set_intrinsics_with_affine(True)
    ref14, vref14 = O.evaluate(pb)
    for fmt in (E.RECORD_F16, E.RECORD_F16_SCALED):
        with E.Engine(pb.kind, pb.model) as eng:
            eng.set_problem(pb)
            eng.set_record_format(fmt)
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.set_intrinsics_with_affine(True)
            assert eng.record_floats == 14 * P and eng.record_format == fmt
            evaluate(eng, pb, "host")
            rec, valid = eng.records()
            assert rec.shape == (pb.n_blocks, 14 * P) and np.array_equal(valid, vref14)
        with open_engine(pb, K, ab) as eng:  # the half formats refused while both are on
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.set_record_format(fmt)
            still_26(eng)
    for intr_first in (True, False):
        with open_engine(pb, K, ab, intr_first=intr_first) as eng:
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                eng.set_intrinsics_with_affine(False)
            still_26(eng)
            eng.set_intrinsics_with_affine(True)  # (again: no change)
            still_26(eng)
    # every on-device solve entry point, with and without the two pba_gn_set_solve_* opt-ins
    with open_engine(pb, K, ab) as eng:
        eng.set_state(pb.poses, pb.rho)
        eng.build_pyramid(2)
        for opted in (False, True):
            if opted:
                eng.gn_set_solve_intrinsics(True)
                eng.gn_set_solve_affine(True)
            for name, call in solve_calls(eng).items():
                with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                    call()
                print("refused:", name, "(with the solve opt-ins)" if opted else "")
            assert eng.level()[0] == 0  # solve_pyramid refused before a level was switched
            assert np.array_equal(eng.get_intrinsics(), K) and np.array_equal(eng.get_affine_state(), ab)
            still_26(eng)
        # with one switch off and its solve opt-in the on-device solve runs
        eng.set_affine_brightness(False)
        eng.gn_set_solve_intrinsics(True)
        assert (eng.record_floats, eng.record_bytes) == (22 * P, 88 * P)
        eng.set_state(pb.poses, pb.rho)
        assert eng.gn_linearize() > 0.0


# 11. both come back: Gauss-Newton over fx, fy, cx, cy and (a_f, b_f), f ≥ 1, from the engine's r, J_intr and brightness
# columns tracks the reference run (tests/test_photometric_affine_intrinsics_reference.py has the reference's own figures)
def test_both_come_back():
    pb, K0 = PAIR.both_case()
    c_ref, K_ref, ab_ref = PAIR.both_run(lambda K, s: PAIR.compose(pb, K, s)[:2], pb, K0)
    with open_engine(pb) as eng:
        eng.set_state(pb.poses, pb.rho)

        def at(K, ab):
            eng.set_intrinsics_state(K)
            eng.set_affine_state(ab)
            eng.evaluate(True)
            return eng.records()

        c_eng, K_eng, ab_eng = PAIR.both_run(at, pb, K0)
    print("engine costs", c_eng, "reference costs", c_ref, "difference of the final (a, b)", np.abs(ab_eng - ab_ref).max(),
          "of the final fx, fy, cx, cy", np.abs(K_eng - K_ref)[0, :4], "reference's error",
          np.abs(K_ref - pb.intrinsics)[0, :4])
    assert c_ref[0] > 100 * c_ref[-1]
    for a, b in zip(c_eng, c_ref):
        assert abs(a - b) <= 1e-3 * b
    assert np.abs(ab_eng - ab_ref).max() <= 1e-3
    assert np.abs(K_eng - K_ref)[0, :4].max() <= 1e-4


# 12. the Ceres drop-in: GpuPhotometricAffineIntrinsicsCost<8> hands jacobians[3], [4] and [5] the records' tail
def test_adapter_photometric_affine_intrinsics_cost():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden import write_problem
    pb = problem()
    ref, vref, uv = reference()
    P, nb = pb.P, pb.n_blocks
    libdir = os.path.dirname(E.LIB_PATH)
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "photometric_affine_intrinsics_adapter_driver")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "tests", "cpp", "mock_ceres"),
                        os.path.join(ROOT, "tests", "cpp", "photometric_affine_intrinsics_adapter_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"],
                       check=True, capture_output=True, text=True)
        fin, fk, fab, fout = (os.path.join(td, n) for n in ("in.bin", "k.bin", "ab.bin", "out.bin"))
        with open(fin, "wb") as f:
            write_problem(f, pb)
        k_state(pb).astype(np.float64).tofile(fk)
        ab_state(pb).astype(np.float64).tofile(fab)
        subprocess.run([exe, fin, fk, fab, fout], check=True)
        raw = np.fromfile(fout, np.uint8)
    o = 0
    out26 = raw[o:o + 8 * nb * 26 * P].view(np.float64).reshape(nb, 26 * P); o += 8 * nb * 26 * P
    valid26 = raw[o:o + nb]; o += nb
    out14 = raw[o:o + 8 * nb * 14 * P].view(np.float64).reshape(nb, 14 * P); o += 8 * nb * 14 * P
    valid14 = raw[o:o + nb]; o += nb
    flags = raw[o:o + 12].view(np.int32)
    assert o + 12 == raw.size
    PAIR.compare(P, out26, ref, valid26, vref, uv, bilinear=True)
    # with jacobians[3] == [4] == [5] == nullptr the other three blocks are unchanged
    assert np.array_equal(valid14, valid26) and np.array_equal(out14, out26[:, :14 * P])
    # an evaluator without the matching blocks refuses the request (and only that)
    assert flags.tolist() == [1, 1, 1]
