"""The 8-lane block kernel (photometric_block_kernel, patterns of at most 8 pixels) with one LDS region and one record
store per wave (pba_wave_slab.h): a workgroup is 4 waves × 8 blocks, each wave overwrites its own tile blocks with its
staged records and stores its own run of them, with no workgroup barrier after the prologue's.

Problem: 6 keyframes, 161 points, 376×240, 644 blocks (20 workgroups of 32 blocks plus 4), evaluated at a state whose
keyframe 5 has a NaN pose, so the blocks that target it (about one in eight, scattered over the waves) are invalid:
all-zero record, validity 0, cost 0.  Formats: fp32, PBA_RECORD_F16, PBA_RECORD_F16_SCALED, free intrinsics (22
columns), affine brightness (18) and both (26), at P = 8 and P = 5 (dead lanes, records off a 16-B size).

Entries: pba_set_state + pba_evaluate ("host") and pba_evaluate_state_device ("device") both reach the kernel's
fused-state prologue (stage_tile_wg).  The kernel's other prologue, the pair table (a.poses == nullptr, stage_tile<8>),
has no caller in the product library: every evaluation and every cost-only launch of a photometric engine passes the
state's poses.  It is kept, runs through the same per-wave placement, and is reached here by the test build's hook
PBA_TEST_PAIR_TABLE (libpba_test.so: pba_evaluate copies the state, forms the pair table with pair_kernel and launches
with a.poses == nullptr): path "table", over the same block counts, formats and patterns.

Bounds, all existing ones: fp32 records against the double oracle by helpers.compare_records (|Δr| ≤ 1e-4, each
Jacobian block within 1e-5 of its largest reference entry, validity identical, pixels within 2e-3 px of a bilinear cell
edge left out of the Jacobian comparison); the 22-, 18- and 26-column records by their references' compare functions
(the same bounds over the added blocks); half records against the fp32 records of the same blocks — which the same
test holds to the oracle — by helpers.fp16_violations and by test_gpu_record_scaled's bound for the scaled format: a
half rounds at 2⁻¹¹ relative, so the oracle's 1e-5 cannot apply to a stored half.  Costs: ½ Σ r² of the reference
residuals; |Δr| ≤ 1e-4 per pixel and fp32 rounding give |Δcost| ≤ 1e-4·Σ|r| + 1e-5·cost + 1e-4.
"""
import contextlib
import dataclasses
import functools
import os

import numpy as np
import pytest

import oracle as O
import photometric_affine_intrinsics_reference as PAIR
import photometric_affine_reference as PAR
import photometric_intrinsics_reference as PIR
from helpers import compare_records, engine_module, fp16_violations, near_cell_boundary, projected_uv, synth
from test_gpu_record_scaled import per_row, row_scales

pytestmark = pytest.mark.gpu
E = engine_module()

FORMATS = ["f32", "f16", "scaled", "intr", "affine", "intr_affine"]
COLS = {"f32": 14, "f16": 14, "scaled": 15, "intr": 22, "affine": 18, "intr_affine": 26}
REFERENCE = {"f32": "plain", "f16": "plain", "scaled": "plain", "intr": "intr", "affine": "affine",
             "intr_affine": "intr_affine"}
# partial tiles, waves with no live block, exact fits of a wave, a tile and two tiles
BLOCK_COUNTS = [1, 5, 8, 9, 24, 31, 32, 33, 40, 57, 64, 65]
NAN_FRAME = 5


def pattern(P):
    return synth.PATTERN8 if P == 8 else np.random.default_rng(P).integers(-3, 4, (P, 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(P):
    return synth.make_problem(n_frames=6, n_points=161, width=376, height=240, border=12, pattern=pattern(P))


def nan_state(pb):
    poses = pb.poses.copy()
    poses[NAN_FRAME, 4] = np.nan
    return poses


def hit_blocks(pb):
    return (pb.block_target == NAN_FRAME) | (pb.point_host[pb.block_point] == NAN_FRAME)


def blocks_of(pb, idx):
    return dataclasses.replace(pb, block_point=np.ascontiguousarray(pb.block_point[idx]),
                               block_target=np.ascontiguousarray(pb.block_target[idx]))


def k_state(pb):
    return PIR.perturbed_state(pb)


def ab_state(pb):
    return PAR.parity_state(pb.n_frames)


@functools.lru_cache(maxsize=None)
def reference(kind, P):
    """(records float64, valid, uv) of all 644 blocks at the state with the NaN pose: the oracle at the finite state,
    the blocks that use keyframe 5 zeroed and invalid (a block's record depends on no other block)."""
    pb = problem(P)
    if kind == "plain":
        ref, vref = O.evaluate(pb)
        uv = projected_uv(pb)
    elif kind == "intr":
        ref, vref, uv = PIR.compose(pb, k_state(pb))
    elif kind == "affine":
        ref, vref, uv = PAR.compose(pb, ab_state(pb))
    else:
        ref, vref, uv = PAIR.compose(pb, k_state(pb), ab_state(pb))
    ref, vref = np.array(ref, np.float64), np.array(vref, np.uint8)
    hit = hit_blocks(pb)
    assert hit.sum() >= 40 and vref[~hit].mean() > 0.9
    ref[hit] = 0.0
    vref[hit] = 0
    return ref, vref, uv


def open_engine(pb, fmt, library=None):
    base = problem(pb.P)
    eng = E.Engine(pb.kind, pb.model, library=library)
    eng.set_problem(pb)
    if fmt == "f16":
        eng.set_record_format(E.RECORD_F16)
    if fmt == "scaled":
        eng.set_record_format(E.RECORD_F16_SCALED)
    if fmt == "intr_affine":
        eng.set_intrinsics_with_affine(True)
    if fmt in ("intr", "intr_affine"):
        eng.set_optimize_intrinsics(True)
        eng.set_intrinsics_state(k_state(base))
    if fmt in ("affine", "intr_affine"):
        eng.set_affine_brightness(True)
        eng.set_affine_state(ab_state(base))
    return eng


@contextlib.contextmanager
def pair_table_hook(on):
    """PBA_TEST_PAIR_TABLE for the evaluations inside (read by the test build at every pba_evaluate)."""
    if on:
        os.environ["PBA_TEST_PAIR_TABLE"] = "1"
    try:
        yield
    finally:
        os.environ.pop("PBA_TEST_PAIR_TABLE", None)


def run(pb, fmt, path, poses=None):
    """One Jacobian evaluation: decoded records, validity, the raw record bytes (one row per block) and block costs."""
    poses = nan_state(pb) if poses is None else poses
    table = path == "table"
    with open_engine(pb, fmt, E.TEST_LIB_PATH if table else None) as eng, pair_table_hook(table):
        assert eng.record_floats == (14 if fmt == "scaled" else COLS[fmt]) * pb.P
        if path in ("host", "table"):
            eng.set_state(poses, pb.rho)
            eng.evaluate(True)
        else:
            import torch
            p = torch.from_numpy(np.ascontiguousarray(poses)).cuda()
            r = torch.from_numpy(np.ascontiguousarray(pb.rho)).cuda()
            eng._keep += [p, r]
            eng.evaluate_state_device(p.data_ptr(), r.data_ptr(), True)
        rec, valid = eng.records()
        raw = np.ascontiguousarray(eng.records_raw()).reshape(pb.n_blocks, -1)
        costs = np.array(eng.block_costs())
    assert raw.shape[1] == COLS[fmt] * pb.P
    return {"rec": rec, "valid": np.asarray(valid), "raw": raw, "costs": costs}


@functools.lru_cache(maxsize=None)
def full_run(fmt, P, path):
    return run(problem(P), fmt, path)


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check(fmt, P, path, got, idx):
    """Records, validity and costs of the blocks idx of the 644-block problem against the references."""
    ref, vref, uv = (x[idx] for x in reference(REFERENCE[fmt], P))
    rec, valid = got["rec"], got["valid"]
    m = vref.astype(bool)
    assert np.array_equal(valid.astype(bool), m)
    if fmt == "f32":
        compare_records(0, P, rec, ref, valid, vref, uv)
    elif fmt == "intr":
        PIR.compare(P, rec, ref, valid, vref, uv, bilinear=True, max_masked=1.0)
    elif fmt == "affine":
        PAR.compare(P, rec, ref, valid, vref, uv, bilinear=True, max_masked=1.0)
    elif fmt == "intr_affine":
        PAIR.compare(P, rec, ref, valid, vref, uv, bilinear=True, max_masked=1.0)
    else:
        r32 = full_run("f32", P, path)["rec"][idx]  # held to the oracle by this test's fp32 case
        if fmt == "f16":
            bad = fp16_violations(rec, r32, uv, P)
            assert not bad.any(), (int(bad.sum()), np.unique(np.nonzero(bad)[1]))
        else:
            a, d = r32[m].astype(np.float64), rec[m].astype(np.float64)
            assert (np.abs(d[:, :P] - a[:, :P]) <= 2.0 ** -11 * np.abs(a[:, :P]) + 2.0 ** -14).all()
            jscale = np.abs(a[:, P:]).max(1, keepdims=True) if a.size else a[:, P:]
            bound = 2.0 ** -11 * np.abs(a[:, P:]) + 2.0 ** -24 * per_row(row_scales(got["raw"][m], P), P) + 1e-6 * jscale
            bad = ~(np.abs(d[:, P:] - a[:, P:]) <= bound) & ~per_row(near_cell_boundary(uv[m]), P)
            assert not bad.any(), (int(bad.sum()), np.unique(np.nonzero(bad)[1]))
    # an invalid block: an all-zero record and no cost
    assert not got["raw"][~m].any() and not got["costs"][~m].any()
    r = ref[:, :P]
    cost_ref = 0.5 * (r * r).sum(1)
    tol = 1e-4 * np.abs(r).sum(1) + 1e-5 * cost_ref + 1e-4
    assert (np.abs(got["costs"] - cost_ref) <= tol)[m].all(), float(np.abs(got["costs"] - cost_ref)[m].max())


@pytest.mark.parametrize("path", ["device", "host", "table"])
@pytest.mark.parametrize("P", [8, 5])
@pytest.mark.parametrize("fmt", FORMATS)
def test_block_counts(fmt, P, path):
    """The first n blocks of the problem, n over BLOCK_COUNTS: against the references, and block i's record, validity
    and cost bit-identical to those of the 644-block launch (the parent commit's kernel has that property too)."""
    pb = problem(P)
    full = full_run(fmt, P, path)
    check(fmt, P, path, full, np.arange(pb.n_blocks))
    assert 0 < full["valid"].sum() < pb.n_blocks
    for n in BLOCK_COUNTS:
        got = run(blocks_of(pb, np.arange(n)), fmt, path)
        check(fmt, P, path, got, np.arange(n))
        assert same_bytes(got["raw"], full["raw"][:n]), n
        assert np.array_equal(got["valid"], full["valid"][:n]) and same_bytes(got["costs"], full["costs"][:n]), n


def morton_order(pb):
    """synth.c4_shard's "morton" block order: by host, then target, then the Morton code of u_ref."""
    def spread(x):
        x = x.astype(np.uint64) & np.uint64(0xFFFF)
        for s, mask in ((8, 0x00FF00FF), (4, 0x0F0F0F0F), (2, 0x33333333), (1, 0x55555555)):
            x = (x | (x << np.uint64(s))) & np.uint64(mask)
        return x
    ur = pb.u_ref[pb.block_point].astype(np.int64)
    code = spread(ur[:, 0]) | (spread(ur[:, 1]) << np.uint64(1))
    return np.lexsort((code, pb.block_target, pb.point_host[pb.block_point]))


@pytest.mark.parametrize("P", [8, 5])
@pytest.mark.parametrize("fmt", FORMATS)
def test_morton_block_order(fmt, P):
    """Block order "morton" (a tile's 32 blocks share a host and mostly a target) beside the "point" order of the other
    tests: all 644 blocks and the first 57, against the references and bit-identical to the point-order launch."""
    pb = problem(P)
    order = morton_order(pb)
    assert not np.array_equal(order, np.arange(pb.n_blocks))
    full = full_run(fmt, P, "device")
    for n in (pb.n_blocks, 57):
        idx = order[:n]
        got = run(blocks_of(pb, idx), fmt, "device")
        check(fmt, P, "device", got, idx)
        assert same_bytes(got["raw"], full["raw"][idx]) and same_bytes(got["costs"], full["costs"][idx])


@pytest.mark.parametrize("path", ["device", "table"])
@pytest.mark.parametrize("wave", [0, 2, 3])
@pytest.mark.parametrize("fmt", FORMATS)
def test_nan_pose_fills_one_wave(fmt, wave, path):
    """40 blocks whose blocks 8·wave … 8·wave + 7 — all eight blocks of the first, a middle or the last wave of the
    first tile — use the keyframe with the NaN pose and no other block does: that wave stores 8 all-zero records with
    validity 0, every other wave's records are the references' (the second tile holds one live wave)."""
    P = 8
    pb = problem(P)
    hit = hit_blocks(pb)
    bad, good = np.nonzero(hit)[0], np.nonzero(~hit)[0]
    idx = np.concatenate([good[:8 * wave], bad[:8], good[8 * wave:32]])
    assert idx.size == 40 and hit[idx[8 * wave:8 * wave + 8]].all() and hit[idx].sum() == 8
    got = run(blocks_of(pb, idx), fmt, path)
    check(fmt, P, path, got, idx)
    dead = np.zeros(40, bool)
    dead[8 * wave:8 * wave + 8] = True
    assert not got["valid"][dead].any() and not got["raw"][dead].any() and not got["costs"][dead].any()
    assert got["valid"][~dead].sum() >= 28  # (a live block may leave the image)
    full = full_run(fmt, P, path)
    assert same_bytes(got["raw"], full["raw"][idx])


@functools.lru_cache(maxsize=None)
def large_problem():
    return synth.make_problem(n_frames=6, n_points=16386, width=376, height=240, border=12, texture="noise", seed=3)


@pytest.mark.parametrize("n_blocks", [65536, 65544])
def test_both_slab_store_paths(n_blocks):
    """65,536 blocks are 2,048 workgroups, the largest launch that stores its slabs write-through (kSlabWtGrid);
    65,544 are 2,049, the first that takes the plain non-temporal stores.  fp32 records at P = 8: sampled blocks — the
    first and the last two tiles and 2,000 others — against the oracle, every block's cost against its own record, and
    the two launches' common blocks bit-identical."""
    big = large_problem()
    assert big.n_blocks == 65544 and (65536 * 8 + 255) // 256 == 2048
    pb = blocks_of(big, np.arange(n_blocks))
    got = run(pb, "f32", "device", poses=pb.poses)
    rec, valid = got["rec"], got["valid"]
    assert valid.mean() > 0.9 and np.isfinite(rec).all() and not got["raw"][~valid.astype(bool)].any()
    s = (rec[:, :8].astype(np.float64) ** 2).sum(1)
    np.testing.assert_allclose(got["costs"], 0.5 * s, rtol=1e-5, atol=1e-4)
    idx = np.unique(np.concatenate([np.arange(64), np.arange(n_blocks - 72, n_blocks),
                                    np.random.default_rng(0).choice(n_blocks, 2000, replace=False)]))
    sub = blocks_of(pb, idx)
    ref, vref = O.evaluate(sub, n_threads=8)
    compare_records(0, 8, rec[idx], ref, valid[idx], vref, projected_uv(sub))
    if n_blocks == 65544:
        other = run(blocks_of(big, np.arange(65536)), "f32", "device", poses=big.poses)
        assert same_bytes(other["raw"], got["raw"][:65536]) and np.array_equal(other["valid"], valid[:65536])
