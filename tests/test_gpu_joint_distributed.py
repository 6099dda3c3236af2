"""The joint solve of poses, inverse distances and (a, b) over several GPUs, rehearsed with shard engines on one device:
pba_joint_band / exchange_size / step_export / step_import and pba_solve_joint_distributed (engine.joint_* and
solve_joint_distributed, distributed.solve_joint_distributed).

The summed exchange of the host-keyframe shards must reproduce the single-engine step (pba_joint_linearize +
pba_joint_step on the whole problem), and the distributed loop pba_solve_joint's trajectory.  Problems:
gn_affine_reference.problem() (its points are hosted by keyframes 0 and 1: two shards of 332 / 312 blocks) and the graphs
of tests/graph_problems.py with the brightness change, at parity_state, Huber 9, gn_joint_reference.FIXED / FIXED_AB; the
loops start from (a, b) = 0, where gn_joint_reference's LM cases were chosen.

Bounds (tests/test_gpu_distributed.py's): both sides are the same fp64 arithmetic up to the order of the sums (per
shard, then across shards; tests/test_gn_joint_distributed_reference.py measures that reorder at 1.2e-10 of the step in
numpy), so Σ shard costs, the model decrease and Σ candidate costs agree to 1e-8 relative, the keyframe step to 1e-6 of
each part's (pose, a, b) largest entry, δρ to rtol 1e-6, the summed system to 1e-10 of the largest entry of S and of g;
LM runs to 1e-6 in every cost, in poses and (a, b), rtol 1e-6 in ρ.  Across ranks the keyframe step, the keyframes' part
of the model decrease and the solved poses and (a, b) are equal bit for bit.  Every test prints what it measured.

Measured (MI355X), worst over all exchange cases: Σ shard costs and Σ candidate costs equal to the last bit; model
decrease 1.5e-15; step pose 3.4e-12, a 3.9e-13, b 1.5e-13; δρ 3.6e-11; S 1.3e-15; g_S 9.4e-16.
"""
import functools
import importlib
import threading

import numpy as np
import pytest

import gn_joint_reference as R
import graph_problems as G
from helpers import engine_module, synth

pytestmark = pytest.mark.gpu
E = engine_module()
D = importlib.import_module("photometric-bundle-adjustment_amd.distributed")
INVALID_ARGUMENT = "invalid argument"
NOT_READY = "not ready"
FIXED, FIXED_AB, HUBER = R.FIXED, R.FIXED_AB, R.HUBER


def problem(name):
    return R.problem() if name == "six" else G.problem(name, changed=True)


def open_engine(pb, ab=None, affine=True, level=0):
    eng = E.Engine(pb.kind, pb.model, huber_width=HUBER)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array(FIXED, np.int32))
    eng.set_state(pb.poses, pb.rho)
    if affine:
        eng.set_affine_brightness(True)
        if ab is not None:
            eng.set_affine_state(ab)
        eng.set_fixed_affine_frames(np.array(FIXED_AB, np.int32))
    if level:
        eng.build_pyramid(level + 1)
        eng.set_level(level)
    return eng


def shard_engines(pb, ab, world, level=0):
    """[(engine, point ids, shard problem)] in rank order."""
    out = []
    for r in range(world):
        sub, pids, _ = D.shard_problem(pb, world, r)
        out.append((open_engine(sub, ab, level=level), pids, sub))
    return out


def close_all(sh):
    for e, _, _ in sh:
        e.close()


@functools.lru_cache(maxsize=None)
def whole_step(name, lam, level=0):
    """The single-engine step on the whole problem: formed once per case, left unchanged."""
    pb = problem(name)
    with open_engine(pb, R.state(pb), level=level) as eng:
        c = eng.joint_linearize()
        m, st = eng.joint_step(lam)
        assert st == 0
        S, g = eng.joint_get_reduced_system()
        dk, dr = eng.joint_get_step()
        cc = eng.joint_candidate_cost()
    for x in (S, g, dk, dr):
        x.setflags(write=False)
    return {"cost": c, "model": m, "S": S, "g": g, "dk": dk, "dr": dr, "candidate": cc}


def part_err(got, ref):
    """max |got − ref| over the largest |ref| (a part that is zero in the reference must be zero)."""
    top = np.abs(ref).max(initial=0.0)
    if top == 0.0:
        assert not np.any(got)
        return 0.0
    return float(np.abs(got - ref).max() / top)


def exchange(sh, lam, band=None, fill=float("nan")):
    """Export on every shard into buffers pre-filled with `fill`, the torch sum in rank order, import on every shard.
    Returns (band, the ranks' buffers, per rank (cost, model keyframes, model points, S, g, δ keyframes, δρ, candidate))."""
    import torch
    costs = [e.joint_linearize() for e, _, _ in sh]
    local = max(e.joint_band() for e, _, _ in sh)
    band = local if band is None else band
    assert band >= local
    n = sh[0][0].joint_exchange_size(band)
    assert all(e.joint_exchange_size(band) == n for e, _, _ in sh)
    nf = sh[0][0].n_frames
    assert n == nf * ((band + 1) * 64 + 32) + 16
    bufs = [torch.full((n,), fill, dtype=torch.float64, device="cuda") for _ in sh]
    for (e, _, _), b in zip(sh, bufs):
        e.joint_step_export(lam, band, b.data_ptr())
    torch.cuda.synchronize()
    tot = bufs[0].clone()
    for b in bufs[1:]:
        tot += b
    torch.cuda.synchronize()
    out = []
    for (e, _, _), c in zip(sh, costs):
        mk, mp, st = e.joint_step_import(lam, band, tot.data_ptr())
        assert st == 0
        S, g = e.joint_get_reduced_system()
        dk, dr = e.joint_get_step()
        out.append((c, mk, mp, S, g, dk, dr, e.joint_candidate_cost()))
    return band, bufs, out


def check_exchange(label, name, world, lam, band=None, level=0):
    pb = problem(name)
    ref = whole_step(name, lam, level)
    sh = shard_engines(pb, R.state(pb), world, level)
    try:
        band, bufs, out = exchange(sh, lam, band)
        assert not any(bool(b.isnan().any()) for b in bufs)  # every double of a NaN-filled buffer is written
        dr = np.zeros(pb.n_points)
        for (_, pids, _), o in zip(sh, out):
            dr[pids] = o[6]
        err = {"cost": abs(sum(o[0] for o in out) - ref["cost"]) / ref["cost"],
               "model": abs(out[0][1] + sum(o[2] for o in out) - ref["model"]) / abs(ref["model"]),
               "candidate": abs(sum(o[7] for o in out) - ref["candidate"]) / ref["candidate"],
               "pose": max(part_err(o[5][:, :6], ref["dk"][:, :6]) for o in out),
               "a": max(part_err(o[5][:, 6], ref["dk"][:, 6]) for o in out),
               "b": max(part_err(o[5][:, 7], ref["dk"][:, 7]) for o in out),
               "drho": float(np.abs(dr / np.where(ref["dr"] != 0, ref["dr"], 1.0) - 1.0)[ref["dr"] != 0].max()),
               "S": max(part_err(o[3], ref["S"]) for o in out), "g": max(part_err(o[4], ref["g"]) for o in out)}
        print(f"\n{label} world {world} band {band} λ={lam}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
        for o in out[1:]:  # the keyframe part is one computation from one buffer: bit for bit the same on every rank
            assert o[1] == out[0][1] and np.array_equal(o[5], out[0][5])
            assert np.array_equal(o[3], out[0][3]) and np.array_equal(o[4], out[0][4])
        assert err["cost"] <= 1e-8 and err["model"] <= 1e-8 and err["candidate"] <= 1e-8, err
        assert max(err["pose"], err["a"], err["b"]) <= 1e-6, err
        np.testing.assert_allclose(dr, ref["dr"], rtol=1e-6, atol=1e-12 * np.abs(ref["dr"]).max())
        assert err["S"] <= 1e-10 and err["g"] <= 1e-10, err
        return sh, out, ref
    except BaseException:
        close_all(sh)
        raise


EXCHANGE_CASES = [("six", 2, None, 1e-4), ("six", 2, None, 1e-1), ("band37", 2, None, 1e-4), ("band37", 2, None, 1e-1),
                  ("band37", 3, None, 1e-4), ("band37", 3, None, 1e-1), ("closed100", 3, 99, 1e-4)]


# 1. the exchange against the single-engine step
@pytest.mark.parametrize("name,world,band,lam", EXCHANGE_CASES,
                         ids=[f"{n}-world{w}-lam{l}" for n, w, _, l in EXCHANGE_CASES])
def test_exchange_matches_single_engine_step(name, world, band, lam):
    sh, out, _ = check_exchange(name, name, world, lam, band)
    try:
        if name == "six":
            assert [e.n_blocks for e, _, _ in sh] == [332, 312]
        if name == "band37":
            assert [e.n_blocks for e, _, _ in sh] == ([728, 688] if world == 2 else [504, 452, 460])
        # accept works after an import as after a step: the state becomes the candidate
        e, _, sub = sh[0]
        dk, dr = out[0][5], out[0][6]
        cc = e.joint_candidate_cost()
        e.joint_accept()
        poses, rho = e.get_state()
        p_ref, r_ref, ab_ref = R.apply_step(sub.poses, sub.rho, R.state(sub), dk, dr)
        np.testing.assert_allclose(poses, p_ref, atol=1e-10)
        np.testing.assert_allclose(rho, r_ref, rtol=1e-12)
        np.testing.assert_allclose(e.get_affine_state(), ab_ref, rtol=1e-12, atol=1e-300)
        assert abs(e.joint_linearize() - cc) <= 1e-6 * cc
    finally:
        close_all(sh)


# 2. constants come after the sum: a keyframe without a valid block on this rank moves with the whole engine's step
def test_constants_are_decided_after_the_sum():
    lam = 1e-4
    sh, out, ref = check_exchange("constants", "band37", 2, lam)
    try:
        e0, _, sub = sh[0]
        touched = np.union1d(sub.point_host[sub.block_point], sub.block_target)
        away = np.setdiff1d(np.arange(sub.n_frames), touched)
        assert len(away) > 0 and len(touched) == 21  # rank 0 has blocks on 21 of the 37 keyframes
        e0.joint_step(lam)  # on its own the shard takes them for constants …
        assert not e0.joint_get_step()[0][away].any()
        dk0 = out[0][5]     # … the import does not
        assert np.abs(dk0[away, :6]).min() > 0 and np.abs(dk0[away, 6:]).min() > 0
        assert part_err(dk0[away, :6], ref["dk"][away, :6]) <= 1e-6
        assert part_err(dk0[away, 6:], ref["dk"][away, 6:]) <= 1e-6
    finally:
        close_all(sh)


# 3. an idle keyframe (no block on any rank): identity row, zero step, on every rank
def test_idle_keyframe_is_constant_on_every_rank():
    sh, out, ref = check_exchange("idle", "closed100_idle", 3, 1e-4, band=99)
    try:
        idle = np.arange(8 * 50, 8 * 51)
        for o in out:
            S, g, dk = o[3], o[4], o[5]
            assert np.array_equal(S[np.ix_(idle, idle)], np.eye(8)) and not g[idle].any() and not dk[50].any()
            others = np.setdiff1d(np.arange(S.shape[0]), idle)
            assert not S[np.ix_(idle, others)].any() and not S[np.ix_(others, idle)].any()
        assert not ref["dk"][50].any()
    finally:
        close_all(sh)


# 4. pyramid level 1
def test_exchange_at_level_1():
    sh, _, _ = check_exchange("level 1", "six", 2, 1e-3, level=1)
    close_all(sh)


# 5. bitwise: two exports of one linearisation are the same bits (NaN-filled buffers fully overwritten: check_exchange)
def test_export_is_reproducible():
    import torch
    pb = problem("band37")
    sh = shard_engines(pb, R.state(pb), 2)
    try:
        e = sh[1][0]
        e.joint_linearize()
        band = e.joint_band()
        n = e.joint_exchange_size(band)
        a = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        b = torch.full((n,), float("inf"), dtype=torch.float64, device="cuda")
        e.joint_step_export(1e-4, band, a.data_ptr())
        e.joint_step_export(1e-1, band, b.data_ptr())  # (another λ in between)
        e.joint_step_export(1e-4, band, b.data_ptr())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(a).all()) and bool(a.abs().max() > 0)
        assert torch.equal(a, b)
        wide = torch.full((e.joint_exchange_size(36),), float("nan"), dtype=torch.float64, device="cuda")
        e.joint_step_export(1e-4, 36, wide.data_ptr())  # K = n_frames − 1: the same blocks, further right
        torch.cuda.synchronize()
        assert bool(torch.isfinite(wide).all())
        va = a[:-16].reshape(37, -1)
        vw = wide[:-16].reshape(37, -1)
        assert torch.equal(va[:, -32:], vw[:, -32:]) and torch.equal(va[:, :-32], vw[:, (36 - band) * 64:-32])
        assert not bool(vw[:, :(36 - band) * 64].any())
    finally:
        close_all(sh)


def run_ranks(fn, world, barrier):
    res, errs = [None] * world, []

    def run(r):
        try:
            res[r] = fn(r)
        except BaseException as ex:  # noqa: BLE001 (reported below)
            errs.append(ex)
            barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not errs, errs
    return res


def same_solve(pb, ref, ranks):
    """ranks: per rank (summary, trajectory, poses, ρ, (a, b), point ids) against the single engine's `ref`."""
    s_ref, its_ref, poses_ref, rho_ref, ab_ref = ref
    rho = np.zeros(pb.n_points)
    for s, its, poses, rr, ab, pids in ranks:
        print(f"\nrank: {s}\ncosts {its['cost']}\nsingle engine: {s_ref}\ncosts {its_ref['cost']}")
        assert s["iterations"] == s_ref["iterations"] and s["successful_steps"] == s_ref["successful_steps"], (s, s_ref)
        assert s["unsuccessful_steps"] == s_ref["unsuccessful_steps"] and s["stop_reason"] == s_ref["stop_reason"]
        assert np.array_equal(its["step_is_successful"], its_ref["step_is_successful"])
        assert np.abs(its["cost"] / its_ref["cost"] - 1.0).max() <= 1e-6, (its["cost"], its_ref["cost"])
        assert abs(s["initial_cost"] - s_ref["initial_cost"]) <= 1e-8 * s_ref["initial_cost"]
        assert abs(s["final_cost"] - s_ref["final_cost"]) <= 1e-6 * s_ref["final_cost"], (s, s_ref)
        np.testing.assert_allclose(poses, poses_ref, atol=1e-6)
        np.testing.assert_allclose(ab, ab_ref, atol=1e-6)
        rho[pids] = rr
        assert np.array_equal(poses, ranks[0][2]) and np.array_equal(ab, ranks[0][4])  # bit for bit across ranks
        assert np.array_equal(its["cost"], ranks[0][1]["cost"])
    np.testing.assert_allclose(rho, rho_ref, rtol=1e-6)
    assert s_ref["final_cost"] < s_ref["initial_cost"] and s_ref["successful_steps"] >= 2


def single_solve(pb, options):
    with open_engine(pb, None) as full:
        s = full.solve_joint(**options)
        return s, full.solver_iterations(), *full.get_state(), full.get_affine_state()


LOOP_CASES = [("six", 2, dict(max_iterations=R.LM_ITERATIONS)), ("six", 2, R.LM_REJECT),
              ("band37", 3, dict(max_iterations=6))]


# 6. the loop over shard engines in threads, summed in-process, against pba_solve_joint
@pytest.mark.parametrize("name,world,options", LOOP_CASES, ids=["six-iterations", "six-reject", "band37-world3"])
def test_solve_joint_distributed_matches_solve_joint(name, world, options):
    import torch
    pb = problem(name)
    ref = single_solve(pb, options)
    if options is R.LM_REJECT:
        assert ref[0]["unsuccessful_steps"] >= 1
    sh = shard_engines(pb, None, world)
    try:
        band = max(e.joint_band() for e, _, _ in sh)
        n = sh[0][0].joint_exchange_size(band)
        bufs = [torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in sh]
        comm = D.InProcessAllReduce(bufs, timeout=120)

        def run(r):
            e, pids, _ = sh[r]
            s = e.solve_joint_distributed(band, bufs[r].data_ptr(), comm.rank(r), **options)
            return s, e.solver_iterations(), *e.get_state(), e.get_affine_state(), pids

        same_solve(pb, ref, run_ranks(run, world, comm.barrier))
    finally:
        close_all(sh)


# 7. two processes on one GPU over gloo: distributed.solve_joint_distributed (TorchAllReduce, the band by a max
# all-reduce), and its error for a rank without blocks
def test_two_process_gloo_solve_joint_matches_solve_joint():
    import socket

    import torch.multiprocessing as mp

    import joint_dist_workers
    pb = problem("six")
    options = dict(max_iterations=R.LM_ITERATIONS)
    ref = single_solve(pb, options)
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=joint_dist_workers.solve_joint_worker, args=(r, 2, port, options, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = {}
        for _ in range(2):
            r, v = q.get(timeout=240)
            res[r] = v
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in range(2):
        assert isinstance(res[r], dict), res[r]
        assert "no blocks" in res[r]["empty_shard_error"]
    same_solve(pb, ref, [(res[r]["summary"], res[r]["iterations"], res[r]["poses"], res[r]["rho"], res[r]["ab"],
                          res[r]["pids"]) for r in range(2)])


# 8. refusals, each leaving the engine working
def exchange_calls(eng, band, ptr):
    return (lambda: eng.joint_exchange_size(band), lambda: eng.joint_step_export(1e-3, band, ptr),
            lambda: eng.joint_step_import(1e-3, band, ptr),
            lambda: eng.solve_joint_distributed(band, ptr, lambda p, n: None, max_iterations=1))


def test_refusals():
    import torch
    pb = problem("six")
    ab = R.state(pb)
    sub, _, _ = D.shard_problem(pb, 2, 0)
    buf = torch.zeros(6 * (6 * 64 + 32) + 16, dtype=torch.float64, device="cuda")
    ptr = buf.data_ptr()
    with open_engine(sub, ab) as eng:
        band = eng.joint_band()
        assert 1 <= band <= 5
        # export without a linearisation, import without an export
        with pytest.raises(E.PbaError, match=NOT_READY):
            eng.joint_step_export(1e-3, band, ptr)
        c = eng.joint_linearize()
        with pytest.raises(E.PbaError, match=NOT_READY):
            eng.joint_step_import(1e-3, band, ptr)
        # a band below the local one or above n_frames − 1; a null buffer
        for bad in (band - 1, 6):
            for call in exchange_calls(eng, bad, ptr):
                with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                    call()
        for call in exchange_calls(eng, band, 0)[1:]:
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                call()
        # an import follows an export of this linearisation at the same λ and band
        eng.joint_step_export(1e-3, band, ptr)
        for lam, k in ((1e-2, band), (1e-3, 5)):
            with pytest.raises(E.PbaError, match=NOT_READY):
                eng.joint_step_import(lam, k, ptr)
        assert eng.joint_linearize() == c
        with pytest.raises(E.PbaError, match=NOT_READY):  # (the export was the previous linearisation's)
            eng.joint_step_import(1e-3, band, ptr)
        eng.joint_step_export(1e-3, band, ptr)
        mk, mp, st = eng.joint_step_import(1e-3, band, ptr)  # one rank's buffer is a sum over one rank
        assert st == 0 and mk + mp > 0
        m, st = eng.joint_step(1e-3)  # … and pba_joint_step goes on as before
        assert st == 0 and m > 0
    with open_engine(sub, affine=False) as eng:  # affine brightness off
        c = eng.gn_linearize()
        for call in (eng.joint_band,) + exchange_calls(eng, 4, ptr):
            with pytest.raises(E.PbaError, match=INVALID_ARGUMENT):
                call()
        assert eng.gn_linearize() == c
    # a shard without blocks (six keyframes in three shards leave one empty): frames, no points or blocks
    with E.Engine(pb.kind, pb.model, huber_width=HUBER) as eng:
        L, h = eng._L, eng._h
        intr = np.ascontiguousarray(pb.intrinsics, np.float64)
        fc = np.ascontiguousarray(pb.frame_cam, np.int32)
        imgs = np.ascontiguousarray(pb.images, np.uint8)
        pat = np.ascontiguousarray(pb.pattern, np.float32)
        assert L.pba_set_cameras(h, intr.shape[0], intr.ctypes.data) == 0
        assert L.pba_set_frames(h, fc.shape[0], fc.ctypes.data, pb.width, pb.height, imgs.ctypes.data) == 0
        assert L.pba_set_pattern(h, pat.shape[0], pat.ctypes.data) == 0
        eng.set_affine_brightness(True)
        assert len(D.shard_problem(pb, 3, 2)[2]) == 0 or len(D.shard_problem(pb, 3, 1)[2]) == 0
        for call in (eng.joint_band,) + exchange_calls(eng, 4, ptr):
            with pytest.raises(E.PbaError, match=NOT_READY):
                call()
        eng.set_problem(sub)  # … and the engine takes a problem afterwards
        eng.set_state(sub.poses, sub.rho)
        eng.set_affine_brightness(True)
        assert eng.joint_linearize() > 0
