"""PBA_RECORD_F16_SCALED: half records with one power-of-two scale per pixel row (include/pba.h).

The input is a problem whose Jacobians leave the half range, so that PBA_RECORD_F16 clamps it: 320×200 frames of a
4-px checkerboard (0 / 255) seen with fx = fy = 600, 7 frames, 300 points × 4 targets = 1200 blocks (a 16-block tail
slab: 1200 % 32 = 16).  Every test compares against the fp32 records of the same engine at the same state, WITHOUT the
clip to ±65504 that helpers.fp16_violations applies for the clamping format.

Bounds.  Residuals: one half rounding, 2⁻¹¹·|r| + 2⁻¹⁴.  Jacobian entry v of pixel row k: the scaled value v/e is
rounded to a half once — 2⁻¹¹·|v| relative, or half a subnormal step 2⁻²⁵·e ≤ 2⁻²⁴·e absolute — plus 1e-6 of the block's
largest |J|, the project's allowance for the fp32 and the half instantiations contracting their fp32 arithmetic
differently (helpers.fp16_violations).  Columns of pixels within 2e-3 px of a bilinear cell edge are left out as there
(helpers.near_cell_boundary); at most 5 % of the rows may go that way.
"""
import dataclasses
import functools

import numpy as np
import pytest

from helpers import engine_module, near_cell_boundary, projected_uv, synth

pytestmark = pytest.mark.gpu
E = engine_module()

PATTERNS = [8, 5, 9, 21, 30]
CASES = [(P, "host") for P in PATTERNS] + [(8, "device"), (21, "device")]
INTRINSICS = [600.0, 600.0, 159.5, 99.5, 0.0, 0.0, 0.0, 0.0]


def pattern(P):
    return synth.PATTERN8 if P == 8 else np.random.default_rng(P).integers(-3, 4, (P, 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(P, n_points=300):
    pb = synth.make_problem(n_frames=7, n_points=n_points, width=320, height=200, pattern=pattern(P), seed=0,
                            border=16, intrinsics=[INTRINSICS])
    y, x = np.mgrid[0:200, 0:320]
    pb.images = np.stack([np.where(((x + 2 * f) // 4 + (y + f) // 4) & 1, 255, 0) for f in range(7)]).astype(np.uint8)
    for f in np.unique(pb.point_host):
        sel = np.nonzero(pb.point_host == f)[0]
        pb.host_intensity[sel] = synth.bilinear(pb.images[f], pb.u_ref[sel, None, 0] + pb.pattern[None, :, 0],
                                                pb.u_ref[sel, None, 1] + pb.pattern[None, :, 1]).astype(np.float32)
    return pb


def evaluator(eng, pb, path):
    """jac -> one evaluation at the problem's state: from host memory + pba_evaluate, or pba_evaluate_state_device."""
    if path == "host":
        eng.set_state(pb.poses, pb.rho)
        return lambda jac: eng.evaluate(jac)
    import torch
    poses = torch.from_numpy(np.ascontiguousarray(pb.poses)).cuda()
    rho = torch.from_numpy(np.ascontiguousarray(pb.rho)).cuda()
    eng._keep += [poses, rho]
    return lambda jac: eng.evaluate_state_device(poses.data_ptr(), rho.data_ptr(), jac)


def device_decode(eng, offset=0):
    """pba_decode_records_device into a fresh device buffer (`offset` floats past its 16-byte aligned start)"""
    import torch
    n = eng.n_blocks * eng.record_floats
    out = torch.full((n + offset + 4,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.decode_records_device(out.data_ptr() + 4 * offset)
    eng.synchronize()
    host = out.cpu().numpy()
    assert np.isnan(host[:offset]).all() and np.isnan(host[offset + n:]).all()  # nothing written around the records
    return host[offset:offset + n].reshape(eng.n_blocks, eng.record_floats)


@functools.lru_cache(maxsize=None)
def run_case(P, path):
    """One engine per case: the three formats at the same state, then the residual-only evaluation in the new format."""
    pb = problem(P)
    out = {}
    with E.Engine(pb.kind, pb.model) as eng:
        eng.set_problem(pb)
        ev = evaluator(eng, pb, path)
        for name, fmt in (("f32", E.RECORD_F32), ("f16", E.RECORD_F16), ("scaled", E.RECORD_F16_SCALED)):
            eng.set_record_format(fmt)
            ev(True)
            rec, valid = eng.records()
            out[name] = {"rec": rec, "valid": valid, "raw": eng.records_raw(), "dev": device_decode(eng),
                         "record_bytes": eng.record_bytes, "record_floats": eng.record_floats}
        out["res_strided"] = eng.residuals()[0]  # after a Jacobian evaluation: the first P halves of every record
        ev(False)
        out["res_only"], out["res_only_valid"] = eng.residuals()
        out["raw_res_only"] = eng.records_raw()
        ev(True)
        out["raw_again"] = eng.records_raw()
    return out


def halves(raw_u16):
    return raw_u16.view(np.float16).astype(np.float64)


def row_scales(raw_u16, P):
    return halves(raw_u16)[:, 14 * P:]


def per_row(x, P):
    """(n, P) per pixel row → (n, 13·P) per Jacobian column of [J_host (P×6) | J_target (P×6) | J_rho (P)]"""
    return np.concatenate([np.repeat(x, 6, 1), np.repeat(x, 6, 1), x], 1)


def row_max(rec, P):
    """largest Jacobian magnitude of every pixel row, (n, P)"""
    n = rec.shape[0]
    a = np.abs(rec)
    return np.maximum(np.maximum(a[:, P:7 * P].reshape(n, P, 6).max(2), a[:, 7 * P:13 * P].reshape(n, P, 6).max(2)),
                      a[:, 13 * P:14 * P])


def check_against_fp32(dec, raw, r32, valid, uv, P):
    """Check 3 of the issue: the decoded scaled records against the fp32 records, no clipping."""
    m = valid.astype(bool)
    a, d = r32[m].astype(np.float64), dec[m].astype(np.float64)
    assert (np.abs(d[:, :P] - a[:, :P]) <= 2.0 ** -11 * np.abs(a[:, :P]) + 2.0 ** -14).all()
    edge = near_cell_boundary(uv[m])
    assert edge.mean() <= 0.05, edge.mean()
    jscale = np.abs(a[:, P:]).max(1, keepdims=True)
    bound = 2.0 ** -11 * np.abs(a[:, P:]) + 2.0 ** -24 * per_row(row_scales(raw[m], P), P) + 1e-6 * jscale
    bad = ~(np.abs(d[:, P:] - a[:, P:]) <= bound) & ~per_row(edge, P)
    assert not bad.any(), (int(bad.sum()), np.unique(np.nonzero(bad)[1]))


@pytest.mark.parametrize("P", PATTERNS)
def test_input_reaches_the_clamp(P):
    """The fp32 records of the checkerboard problem: rows beyond the half range and rows within it, blocks valid."""
    c = run_case(P, "host")["f32"]
    big = row_max(c["rec"][c["valid"].astype(bool)], P) > 65504.0
    assert big.mean() >= 0.25 and (~big).mean() >= 0.25, big.mean()
    assert c["valid"].mean() >= 0.9


@pytest.mark.parametrize("P,path", CASES)
def test_validity_and_sizes(P, path):
    c = run_case(P, path)
    n = problem(P).n_blocks
    assert np.array_equal(c["scaled"]["valid"], c["f32"]["valid"])
    assert c["scaled"]["record_bytes"] == 30 * P and c["scaled"]["record_floats"] == 14 * P
    assert c["f16"]["record_bytes"] == 28 * P and c["f32"]["record_bytes"] == 56 * P
    raw = c["scaled"]["raw"]
    assert raw.dtype == np.uint16 and raw.size == n * 15 * P
    assert c["f16"]["raw"].dtype == np.uint16 and c["f16"]["raw"].size == n * 14 * P
    assert c["f32"]["raw"].dtype == np.float32 and c["f32"]["raw"].size == n * 14 * P


@pytest.mark.parametrize("P,path", CASES)
def test_raw_records_are_self_consistent(P, path):
    c = run_case(P, path)["scaled"]
    raw = c["raw"][c["valid"].astype(bool)]
    h = halves(raw)
    assert np.isfinite(h).all()
    e = h[:, 14 * P:]
    assert ((e >= 1) & (e <= 2.0 ** 15)).all() and (np.log2(e) == np.rint(np.log2(e))).all()
    stored = row_max(h, P)
    assert ((stored >= 16384) & (stored <= 32768))[e > 1].all()
    assert (stored <= 65504)[e == 1].all()
    assert (e > 1).any() and (e == 1).any()
    # an invalid block stores 15·P zero halves
    assert not c["raw"][~c["valid"].astype(bool)].any()


@pytest.mark.parametrize("P,path", CASES)
def test_decoded_records_match_fp32_without_clipping(P, path):
    c = run_case(P, path)
    pb = problem(P)
    r32, valid = c["f32"]["rec"], c["f32"]["valid"]
    check_against_fp32(c["scaled"]["rec"], c["scaled"]["raw"], r32, valid, projected_uv(pb), P)
    # the same input through PBA_RECORD_F16 is off by more than 10 % somewhere: it reaches the clamp
    m = valid.astype(bool)
    a, h = r32[m].astype(np.float64), c["f16"]["rec"][m].astype(np.float64)
    assert (np.abs(h - a) > 0.1 * np.abs(a)).any()


@pytest.mark.parametrize("P,path", CASES)
def test_half_records_saturate_at_the_half_range(P, path):
    """PBA_RECORD_F16 saturates at ±65504 (include/pba.h): with a the fp32 record and h the raw halves of the valid
    blocks, every half is finite, |a| ≥ 65536 gives exactly ±65504 with a's sign, and |a| ≤ 65000 stays within the range.
    The band between is left out: the fp32 and the half instantiations may contract their arithmetic differently (the
    1e-6 allowance above), so an entry next to 65520 may round to either side there.  It holds at most 0.1 % of the
    Jacobian entries, and at least 1000 entries lie beyond it."""
    c = run_case(P, path)
    m = c["f32"]["valid"].astype(bool)
    assert np.array_equal(c["f16"]["valid"], c["f32"]["valid"])
    a, h = c["f32"]["rec"][m].astype(np.float64), halves(c["f16"]["raw"][m])
    assert a.shape == h.shape
    big, small = np.abs(a) >= 65536.0, np.abs(a) <= 65000.0
    assert big.sum() >= 1000, int(big.sum())
    assert (~big & ~small)[:, P:].mean() <= 1e-3, int((~big & ~small).sum())
    assert np.isfinite(h).all()
    assert np.array_equal(h[big], np.copysign(65504.0, a[big]))
    assert (np.abs(h[small]) <= 65504.0).all()


@pytest.mark.parametrize("P,path", CASES)
def test_host_numpy_and_device_decodes_agree_bitwise(P, path):
    c = run_case(P, path)
    s = c["scaled"]
    ref = E.decode_scaled(s["raw"], P)
    assert np.array_equal(s["rec"].view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(s["dev"].view(np.uint32), ref.view(np.uint32))
    for name in ("f32", "f16"):
        assert np.array_equal(c[name]["dev"].view(np.uint32), c[name]["rec"].view(np.uint32)), name
    assert np.array_equal(c["f32"]["raw"].view(np.uint32), c["f32"]["rec"].view(np.uint32))
    assert np.array_equal(c["f16"]["raw"].view(np.float16).astype(np.float32).view(np.uint32),
                          c["f16"]["rec"].view(np.uint32))


@pytest.mark.parametrize("P,path", CASES)
def test_residual_only_evaluation(P, path):
    c = run_case(P, path)
    r = c["f32"]["rec"][:, :P].astype(np.float64)
    tol = 2.0 ** -11 * np.abs(r) + 2.0 ** -14
    assert np.array_equal(c["res_only_valid"], c["f32"]["valid"])
    assert (np.abs(c["res_only"] - r) <= tol).all()
    assert (np.abs(c["res_strided"] - r) <= tol).all()
    assert (np.abs(halves(c["raw_res_only"])[:, :P] - r) <= tol).all()  # written at the 15·P stride
    assert np.array_equal(c["raw_again"], c["scaled"]["raw"])


@pytest.mark.parametrize("P", PATTERNS)
def test_small_launch_and_invalid_blocks(P):
    """20 blocks — less than one workgroup — and 19: with an odd pattern an odd number of 15·P-half records ends on a
    2-byte boundary, the slab store's narrowest path.  ρ = NaN invalidates a point's blocks: 15·P zero halves."""
    pb = problem(P, 5)
    assert pb.n_blocks == 20
    pb19 = dataclasses.replace(pb, block_point=pb.block_point[:19], block_target=pb.block_target[:19])
    rho_nan = pb.rho.copy()
    rho_nan[:4] = np.nan
    dead = np.isin(pb.block_point, np.arange(4))
    with E.Engine(pb.kind, pb.model) as eng:
        eng.set_problem(pb)
        eng.set_state(pb.poses, pb.rho)
        eng.evaluate(True)
        r32, v32 = eng.records()
        eng.set_record_format(E.RECORD_F16_SCALED)
        eng.evaluate(True)
        raw, valid = eng.records_raw(), eng.records()[1]
        dec = eng.records()[0]
        eng.set_state(pb.poses, rho_nan)
        eng.evaluate(True)
        raw_nan, valid_nan = eng.records_raw(), eng.records()[1]
    assert np.array_equal(valid, v32) and valid.all()
    check_against_fp32(dec, raw, r32, valid, projected_uv(pb), P)
    assert not valid_nan[dead].any() and valid_nan[~dead].all() and dead.sum() == 16
    assert not raw_nan[dead].any()
    assert np.array_equal(raw_nan[~dead], raw[~dead])
    with E.Engine(pb.kind, pb.model) as eng:
        eng.set_problem(pb19)
        eng.set_record_format(E.RECORD_F16_SCALED)
        eng.set_state(pb.poses, pb.rho)
        eng.evaluate(True)
        raw19 = eng.records_raw()
        dev19 = device_decode(eng)
        dev19_unaligned = device_decode(eng, offset=1)  # a destination that is only 4-byte aligned
    assert np.array_equal(raw19, raw[:19])
    assert np.array_equal(dev19.view(np.uint32), dec[:19].view(np.uint32))
    assert np.array_equal(dev19_unaligned.view(np.uint32), dec[:19].view(np.uint32))


def test_multi_pixel_kernel_forms_agree_bitwise():
    """The 21-px kernel at a device state takes its camera constants from the camera record (one camera), the LDS camera
    table (two cameras, here with equal intrinsics) or each block's tile (the problem registered with six cameras): the
    three forms of test_gpu_pyramid.test_multi_pixel_kernel_forms_agree_bitwise.  Same values, same arithmetic: the raw
    scaled records are bit-identical."""
    P = 21
    pb = problem(P)
    forms = {"one camera": pb,
             "camera table": dataclasses.replace(pb, intrinsics=np.repeat(pb.intrinsics, 2, 0),
                                                 frame_cam=(np.arange(7) % 2).astype(np.int32)),
             "per block": dataclasses.replace(pb, intrinsics=np.repeat(pb.intrinsics, 6, 0))}
    raw = {}
    for name, prob in forms.items():
        with E.Engine(pb.kind, pb.model) as eng:
            eng.set_problem(prob)
            eng.set_record_format(E.RECORD_F16_SCALED)
            evaluator(eng, pb, "device")(True)
            raw[name] = (eng.records_raw(), eng.records()[1])
    ref = run_case(P, "device")["scaled"]
    for name, (r, v) in raw.items():
        assert np.array_equal(v, ref["valid"]), name
        assert np.array_equal(r, ref["raw"]), name


@pytest.mark.parametrize("P", [8, 21])
def test_pyramid_level(P):
    """Level 1 of a 2-level pyramid: the scaled records against that level's fp32 records (the accuracy bounds of the
    level-0 cases; whether the half-resolution input still reaches the clamp is not part of this check)."""
    pb = problem(P)
    with E.Engine(pb.kind, pb.model) as eng:
        eng.set_problem(pb)
        eng.set_state(pb.poses, pb.rho)
        eng.build_pyramid(2)
        eng.set_level(1)
        eng.evaluate(True)
        r32, v32 = eng.records()
        eng.set_record_format(E.RECORD_F16_SCALED)
        eng.evaluate(True)
        dec, valid = eng.records()
        raw = eng.records_raw()
    assert np.array_equal(valid, v32) and valid.mean() >= 0.9
    check_against_fp32(dec, raw, r32, valid, projected_uv(synth.level_problem(pb, 1)), P)
    assert np.array_equal(dec.view(np.uint32), E.decode_scaled(raw, P).view(np.uint32))


def test_asynchronous_read_back_refuses_half_records():
    """pba_get_records_async copies fp32 records: it refuses the scaled format as it refuses PBA_RECORD_F16."""
    import ctypes as C
    pb = problem(8, 5)
    rec = np.zeros((pb.n_blocks, 14 * 8), np.float32)
    valid = np.zeros(pb.n_blocks, np.uint8)
    with E.Engine(pb.kind, pb.model) as eng:
        eng.set_problem(pb)
        eng.set_state(pb.poses, pb.rho)
        rcs = {}
        for fmt in (E.RECORD_F16, E.RECORD_F16_SCALED):  # (fp32: test_gpu_parity, into page-locked memory)
            eng.set_record_format(fmt)
            eng.evaluate(True)
            rcs[fmt] = eng._L.pba_get_records_async(eng._h, C.c_void_p(rec.ctypes.data), C.c_void_p(valid.ctypes.data),
                                                    C.c_int32(8))
            assert b"fp32 records only" in eng._L.pba_last_error()
    assert rcs == {E.RECORD_F16: -1, E.RECORD_F16_SCALED: -1}  # PBA_ERR_INVALID_ARGUMENT
    assert not rec.any() and not valid.any()


def test_geometric_engine_rejects_the_format():
    g = synth.make_problem(kind="geometric", n_frames=6, n_points=20, seed=64)
    with E.Engine(g.kind, g.model) as eng:
        eng.set_problem(g)
        rc = eng._L.pba_set_record_format(eng._h, E.RECORD_F16_SCALED)
        assert rc == -1 and eng._L.pba_status_string(rc) == b"invalid argument"  # PBA_ERR_INVALID_ARGUMENT
        assert eng.record_format == E.RECORD_F32 and eng.record_bytes == 4 * eng.record_floats
