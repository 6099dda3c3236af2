"""GPU parity of the multi-GPU Gauss-Newton path (include/pba.h §8e) with shard engines on one device:
the summed exchange of two/three host-keyframe shards must reproduce the single-engine step
(pba_gn_step on the whole problem) and pba_solve_distributed must take the same LM decisions as pba_solve.

Tolerances: identical arithmetic up to the order of the fp64 sums (per-rank sums, then across ranks), so
steps agree to 1e-6 relative, model decreases and costs to 1e-8 relative; LM runs to 1e-6 in final cost
and 1e-6 in poses."""
import importlib
import threading

import numpy as np
import pytest

import gn_reference as GR
from helpers import engine_module, synth

pytestmark = pytest.mark.gpu
E = engine_module()
D = importlib.import_module("photometric-bundle-adjustment_amd.distributed")


def engine_for(pb, huber, fixed, library=None):
    eng = E.Engine(pb.kind, pb.model, huber_width=huber, library=library)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array(fixed, np.int32))
    eng.set_state(pb.poses, pb.rho)
    return eng


def shards(pb, world, huber, fixed, library=None):
    out = []
    for r in range(world):
        sub, pids, bids = D.shard_problem(pb, world, r)
        out.append((engine_for(sub, huber, fixed, library), pids))
    return out


@pytest.mark.parametrize("kind,model,huber,world", [(0, 0, 9.0, 2), (1, 0, 1.0, 2), (0, 1, 9.0, 3), (1, 1, 1.0, 3)])
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_exchange_matches_single_engine_step(kind, model, huber, world, lam):
    import torch
    pb = synth.make_problem(kind=kind, model=model, n_frames=14, n_points=140, width=376, height=240,
                            seed=71 + model, border=12, obs_sigma=0.3)
    fixed = (0,)
    with engine_for(pb, huber, fixed) as full:
        c_full = full.gn_linearize()
        m_full, st_full = full.gn_step(lam)
        dp_full, dr_full = full.gn_last_step()
    assert st_full == 0
    sh = shards(pb, world, huber, fixed)
    try:
        costs = [e.gn_linearize() for e, _ in sh]
        assert abs(sum(costs) - c_full) <= 1e-8 * c_full
        band = max(e.gn_band() for e, _ in sh)
        n = sh[0][0].gn_exchange_size(band)
        bufs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in sh]
        for (e, _), b in zip(sh, bufs):
            e.gn_step_export(lam, band, b.data_ptr())
        tot = bufs[0].clone()
        for b in bufs[1:]:
            tot += b
        torch.cuda.synchronize()
        model_pts, dr = 0.0, np.zeros(pb.n_points)
        mps = []
        for e, pids in sh:
            mp, mq, st = e.gn_step_import(lam, band, tot.data_ptr())
            assert st == 0
            mps.append(mp)
            model_pts += mq
            dp, drs = e.gn_last_step()
            assert np.linalg.norm(dp - dp_full) <= 1e-6 * np.linalg.norm(dp_full)
            dr[pids] = drs
        assert max(mps) - min(mps) <= 1e-12 * abs(mps[0])  # identical pose step on every rank
        assert abs(mps[0] + model_pts - m_full) <= 1e-8 * abs(m_full)
        np.testing.assert_allclose(dr, dr_full, rtol=1e-6, atol=1e-12 * np.abs(dr_full).max())
    finally:
        for e, _ in sh:
            e.close()
    # and against the dense reference
    H, g, _ = GR.linearize(pb, pb.poses, pb.rho, huber, fixed)
    _, _, dp_ref, _, _ = GR.schur_step(H, g, pb.n_frames, lam, fixed)
    assert np.linalg.norm(dp_full - dp_ref) <= 1e-3 * np.linalg.norm(dp_ref)


@pytest.mark.parametrize("kind,model,huber", [(0, 0, 9.0), (1, 0, 1.0)])
def test_solve_distributed_matches_solve(kind, model, huber):
    """Three shard engines in three threads, summed in-process: same LM trajectory as one engine."""
    import torch
    pb = synth.make_problem(kind=kind, model=model, n_frames=16, n_points=400, width=376, height=240, seed=81,
                            border=12, obs_sigma=0.3)
    pb.poses[:2] = pb.poses_gt[:2]
    fixed = (0, 1)
    with engine_for(pb, huber, fixed) as full:
        ref = full.solve(max_iterations=12)
        poses_ref, rho_ref = full.get_state()
    world = 3
    sh = shards(pb, world, huber, fixed)
    try:
        band = max(e.gn_band() for e, _ in sh)
        n = sh[0][0].gn_exchange_size(band)
        bufs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in sh]
        comm = D.InProcessAllReduce(bufs, timeout=120)
        res, errs = [None] * world, []

        def run(r):
            try:
                res[r] = sh[r][0].solve_distributed(band, bufs[r].data_ptr(), comm.rank(r), max_iterations=12)
            except BaseException as ex:
                errs.append(ex)
                comm.barrier.abort()

        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(300)
        assert not errs, errs
        rho = np.zeros(pb.n_points)
        for r, (e, pids) in enumerate(sh):
            s = res[r]
            assert s["iterations"] == ref["iterations"] and s["successful_steps"] == ref["successful_steps"], (s, ref)
            assert abs(s["initial_cost"] - ref["initial_cost"]) <= 1e-8 * ref["initial_cost"]
            assert abs(s["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"], (s, ref)
            poses, rr = e.get_state()
            np.testing.assert_allclose(poses, poses_ref, atol=1e-6)
            rho[pids] = rr
        np.testing.assert_allclose(rho, rho_ref, rtol=1e-6)
        assert ref["final_cost"] < ref["initial_cost"]
    finally:
        for e, _ in sh:
            e.close()


def run_ranks(fn, world, timeout=600):
    res, errs = [None] * world, []

    def run(r):
        try:
            res[r] = fn(r)
        except BaseException as ex:  # noqa: BLE001 (reported below)
            errs.append(ex)

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    assert not any(t.is_alive() for t in th), "rank thread hung"
    assert not errs, errs
    return res


def check_same_solve(pb, sh, res, ref, poses_ref, rho_ref, cost_rtol=1e-6, pose_atol=1e-6):
    rho = np.zeros(pb.n_points)
    for r, (e, pids) in enumerate(sh):
        s = res[r]
        for k in ("iterations", "successful_steps", "unsuccessful_steps", "termination", "stop_reason"):
            assert s[k] == ref[k], (k, s, ref)
        assert abs(s["initial_cost"] - ref["initial_cost"]) <= 1e-8 * ref["initial_cost"]
        assert abs(s["final_cost"] - ref["final_cost"]) <= cost_rtol * ref["final_cost"], (s, ref)
        poses, rr = e.get_state()
        np.testing.assert_allclose(poses, poses_ref, atol=pose_atol)
        rho[pids] = rr
    np.testing.assert_allclose(rho, rho_ref, rtol=1e-6, atol=1e-9 * np.abs(rho_ref).max())


@pytest.mark.parametrize("kind,model,huber", [(0, 0, 9.0), (1, 0, 1.0)])
def test_solve_distributed_comm_local_group_matches_solve(kind, model, huber):
    """The stream-ordered loop (pba_solve_distributed_comm): three shard engines in three threads over an in-process
    pba_comm group — both sums of every trial enqueued on the engine streams, the next trial enqueued ahead of the
    decision — take pba_solve's trajectory."""
    pb = synth.make_problem(kind=kind, model=model, n_frames=16, n_points=400, width=376, height=240, seed=81,
                            border=12, obs_sigma=0.3)
    pb.poses[:2] = pb.poses_gt[:2]
    fixed = (0, 1)
    with engine_for(pb, huber, fixed) as full:
        ref = full.solve(max_iterations=12)
        poses_ref, rho_ref = full.get_state()
    world = 3
    sh = shards(pb, world, huber, fixed)
    comms = E.Comm.local_group(world)
    try:
        band = max(e.gn_band() for e, _ in sh)
        res = run_ranks(lambda r: sh[r][0].solve_distributed_comm(band, comms[r], max_iterations=12), world)
        check_same_solve(pb, sh, res, ref, poses_ref, rho_ref)
        assert ref["final_cost"] < ref["initial_cost"]
    finally:
        for c in comms:
            c.close()
        for e, _ in sh:
            e.close()


@pytest.mark.parametrize("mode,trial", [(1, 3), (2, 3), (1, 6), (2, 6)])
def test_solve_distributed_comm_desync_fails_loudly(monkeypatch, mode, trial):
    """The decision-word check of the device-steered loop: every trial's scalar all-reduce also sums each rank's
    previous decision word and its square (N·Σw² = (Σw)² iff the words agree).  PBA_TEST_PERTURB_DECISION overrides
    one rank's decision of one trial (mode 1 flips accept, mode 2 ends that rank's solve) — a hook of the library's test
    build (libpba_test.so, PBA_TEST_HOOKS), which this test loads: every rank must then return an error naming the
    trial — not hang on mismatched collectives — including a perturbed last trial, which only the final verification
    all-reduce sees."""
    pb = synth.make_problem(kind=0, model=0, n_frames=16, n_points=400, width=376, height=240, seed=81,
                            border=12, obs_sigma=0.3)
    pb.poses[:2] = pb.poses_gt[:2]
    world, iters = 3, 6
    sh = shards(pb, world, 9.0, (0, 1), E.TEST_LIB_PATH)
    comms = E.Comm.local_group(world, library=E.TEST_LIB_PATH)
    try:
        band = max(e.gn_band() for e, _ in sh)
        res = run_ranks(lambda r: sh[r][0].solve_distributed_comm(band, comms[r], max_iterations=iters), world,
                        timeout=120)
        assert all(s["iterations"] == iters for s in res), res  # unperturbed: the loop runs its iterations
        for e, pids in sh:
            e.set_state(pb.poses, pb.rho[pids])
        monkeypatch.setenv("PBA_TEST_PERTURB_DECISION", f"1:{trial}:{mode}")
        errs = [None] * world

        def run(r):
            try:
                sh[r][0].solve_distributed_comm(band, comms[r], max_iterations=iters)
            except RuntimeError as ex:
                errs[r] = str(ex)
            return 0

        run_ranks(run, world, timeout=120)
        for r in range(world):
            assert errs[r] is not None and f"differed at trial {trial} " in errs[r], (r, errs)
        print("\n" + errs[0])
    finally:
        for c in comms:
            c.close()
        for e, _ in sh:
            e.close()


def test_solve_distributed_rccl_single_rank_matches_solve():
    """RCCL itself (librccl through pba_comm_init, one rank on this GPU — two ranks cannot share a device under
    RCCL): ncclAllReduce on the engine stream inside the device-steered loop gives pba_solve's trajectory."""
    pb = synth.make_problem(kind=0, n_frames=16, n_points=400, width=376, height=240, seed=85, border=12)
    pb.poses[:2] = pb.poses_gt[:2]
    with engine_for(pb, 9.0, (0, 1)) as full:
        ref = full.solve(max_iterations=10)
        poses_ref, rho_ref = full.get_state()
    comm = E.Comm.rccl(E.Comm.unique_id(), 1, 0, 0)
    try:
        assert comm.rank == 0 and comm.size == 1
        with engine_for(pb, 9.0, (0, 1)) as e:
            s = e.solve_distributed_comm(e.gn_band(), comm, max_iterations=10)
            check_same_solve(pb, [(e, np.arange(pb.n_points))], [s], ref, poses_ref, rho_ref)
    finally:
        comm.close()


def test_c4_eight_shard_rehearsal_matches_solve():
    """The 8-GPU split of the C4 problem rehearsed on one GPU: the full 1000-keyframe × 100k-point problem (rendered
    images) sharded by host keyframe over 8 engines, one thread each, summed through an in-process pba_comm group with
    the stream-ordered device-steered loop.  Same LM trajectory as pba_solve on the whole problem: after one
    iteration the states agree to rounding (the sums only run in another order); over four iterations the same
    decisions and costs to 1e-6 — the C4 reduced system is so poorly conditioned (a 1000-keyframe chain held by two
    frames) that the order of the fp64 sums alone moves the fourth iterate by ~1e-4 in some poses: pba_solve
    against the same loop on ONE shard differs as much (tools/probe/rehearsal_probe.py: 1.9e-4 at W = 1, 9.4e-5 at
    W = 8; 3e-14 after the first iteration)."""
    import time

    import torch
    pb, images = synth.c4_shard(torch.device("cuda", 0), texture="render")
    fixed = (0, 1)
    iters = 4

    def engine_c4(p):
        eng = E.Engine(0, 0, huber_width=9.0)
        eng.set_problem(p, images_device_ptr=images.data_ptr())
        eng.set_fixed_frames(np.array(fixed, np.int32))
        eng.set_state(p.poses, p.rho)
        return eng

    with engine_c4(pb) as full:
        ref1 = full.solve(max_iterations=1)  # (also the warm-up)
        poses_ref1, rho_ref1 = full.get_state()
        full.set_state(pb.poses, pb.rho)
        ref = full.solve(max_iterations=iters)
        poses_ref, rho_ref = full.get_state()
    world = 8
    sh = []
    for r in range(world):
        sub, pids, _ = D.shard_problem(pb, world, r)
        sh.append((engine_c4(sub), pids))
    comms = E.Comm.local_group(world)
    try:
        band = max(e.gn_band() for e, _ in sh)
        res1 = run_ranks(lambda r: sh[r][0].solve_distributed_comm(band, comms[r], max_iterations=1), world)
        check_same_solve(pb, sh, res1, ref1, poses_ref1, rho_ref1, cost_rtol=1e-10, pose_atol=1e-10)
        for r, (e, pids) in enumerate(sh):
            e.set_state(pb.poses, pb.rho[pids])
        t0 = time.perf_counter()
        res = run_ranks(lambda r: sh[r][0].solve_distributed_comm(band, comms[r], max_iterations=iters), world)
        wall = time.perf_counter() - t0
        for r in range(world):
            for k in ("iterations", "successful_steps", "unsuccessful_steps", "termination", "stop_reason"):
                assert res[r][k] == ref[k], (k, res[r], ref)
            assert abs(res[r]["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"], (res[r], ref)
        print(f"\nC4 8-shard rehearsal on one GPU: {res[0]['iterations']} iterations, {1e3 * wall / iters:.3f} ms per "
              f"iteration (one engine: {ref['total_ms'] / max(ref['iterations'], 1):.3f} ms)")
    finally:
        for c in comms:
            c.close()
        for e, _ in sh:
            e.close()


@pytest.mark.parametrize("kind,huber", [(0, 9.0), (1, 1.0)])
def test_two_process_gloo_solve_matches_solve(kind, huber):
    """Two processes, one engine each (both on cuda:0), a world-size-2 gloo group: distributed.solve_distributed
    (the engine's export → torch.distributed all-reduce → import, every scalar of the LM decision all-reduced) takes
    the same LM trajectory as one engine on the whole problem — the bench's multi-GPU GN path with gloo standing in
    for RCCL (two ranks cannot share a device under RCCL)."""
    import socket

    import torch.multiprocessing as mp

    import dist_workers
    case = dict(kind=kind, n_frames=16, n_points=400, seed=83, huber=huber, fixed=[0, 1], iters=10)
    pb = synth.make_problem(kind=kind, n_frames=16, n_points=400, width=376, height=240, seed=83, border=12,
                            obs_sigma=0.3)
    pb.poses[:2] = pb.poses_gt[:2]
    with engine_for(pb, huber, (0, 1)) as full:
        ref = full.solve(max_iterations=10)
        poses_ref, rho_ref = full.get_state()
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=dist_workers.solve_worker, args=(r, 2, port, case, q)) for r in range(2)]
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
    rho = np.zeros(pb.n_points)
    for r in range(2):
        assert isinstance(res[r], dict), res[r]
        s = res[r]["summary"]
        assert s["iterations"] == ref["iterations"] and s["successful_steps"] == ref["successful_steps"], (s, ref)
        assert abs(s["initial_cost"] - ref["initial_cost"]) <= 1e-8 * ref["initial_cost"]
        assert abs(s["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"], (s, ref)
        np.testing.assert_allclose(res[r]["poses"], poses_ref, atol=1e-6)
        rho[res[r]["pids"]] = res[r]["rho"]
    np.testing.assert_allclose(rho, rho_ref, rtol=1e-6)
    assert ref["final_cost"] < ref["initial_cost"]


@pytest.mark.parametrize("comm", ["callback", "rccl"])
def test_one_rank_nccl_group_solve_matches_solve(comm):
    """bench.py's multi-GPU GN leg under an "nccl" (RCCL) torch.distributed group, with the one rank a single GPU allows:
    the default host-callback loop (TorchAllReduce: torch's all_reduce on the exchange buffer between trials) and the
    opt-in device-steered loop (the RCCL communicator distributed.rccl_comm sets up from the group) both take
    pba_solve's trajectory."""
    import socket

    import torch.multiprocessing as mp

    import dist_workers
    case = dict(kind=0, n_frames=16, n_points=400, seed=83, huber=9.0, fixed=[0, 1], iters=10, backend="nccl",
                comm=False if comm == "callback" else None)
    pb = synth.make_problem(kind=0, n_frames=16, n_points=400, width=376, height=240, seed=83, border=12,
                            obs_sigma=0.3)
    pb.poses[:2] = pb.poses_gt[:2]
    with engine_for(pb, 9.0, (0, 1)) as full:
        ref = full.solve(max_iterations=10)
        poses_ref, rho_ref = full.get_state()
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=dist_workers.solve_worker, args=(0, 1, port, case, q))
    p.start()
    try:
        r, v = q.get(timeout=240)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    assert isinstance(v, dict), v
    s = v["summary"]
    assert s["iterations"] == ref["iterations"] and s["successful_steps"] == ref["successful_steps"], (s, ref)
    assert abs(s["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"], (s, ref)
    np.testing.assert_allclose(v["poses"], poses_ref, atol=1e-6)
    np.testing.assert_allclose(v["rho"], rho_ref, rtol=1e-6)


def test_band_too_small_is_rejected():
    import torch
    pb = synth.make_problem(kind="geometric", n_frames=12, n_points=60, seed=5)
    with engine_for(pb, 1.0, (0,)) as e:
        e.gn_linearize()
        b = e.gn_band()
        with pytest.raises(E.PbaError, match="band"):
            e.gn_exchange_size(b - 1)
        n = e.gn_exchange_size(b)
        # banded rows + the 16 scalars of a trial (point part from every rank, pose part + solve status from rank 0)
        assert n == 12 * ((E_band(b) + 1) * 36 + 24) + 16


def intrinsics_problem(n_frames, n_points, seed, model=0):
    """A stereo rig (two cameras, alternate keyframes) whose intrinsics state differs from the cameras the hosts
    unproject with (reprojection.h:93-98), as test_gpu_gn's free-intrinsics tests."""
    pb0 = synth.make_problem(kind=1, model=model, n_frames=n_frames, n_points=n_points, width=376, height=240,
                             seed=seed, border=12)
    k1 = pb0.intrinsics[0].copy()
    k1[:4] *= np.array([1.01, 0.99, 1.0, 1.0])
    intr = np.stack([pb0.intrinsics[0], k1])
    pb = synth.make_problem(kind=1, model=model, n_frames=n_frames, n_points=n_points, width=376, height=240,
                            seed=seed, border=12, intrinsics=intr, frame_cam=np.arange(n_frames, dtype=np.int32) % 2,
                            obs_sigma=0.3)
    return pb, intr * np.array([1.003, 0.998, 1.0005, 0.9995, 1, 1, 1, 1])


def intrinsics_engine(pb, state, fixed):
    e = engine_for(pb, 1.0, fixed)
    e.set_optimize_intrinsics(True)
    e.set_intrinsics_state(state)
    return e


@pytest.mark.parametrize("world,model", [(2, 0), (3, 0), (2, 1), (2, 2), (2, 3)])
@pytest.mark.parametrize("lam", [1e-4, 1e-1])
def test_free_intrinsics_exchange_matches_single_engine_step(world, model, lam):
    """Free intrinsics on several GPUs (optimize_intrinsics, map_utils.h:339-345): each rank exports its keyframe band
    AND its undamped border rows (the cameras' intrinsics against every keyframe and camera, direct − Schur terms at λ,
    the direct diagonal, g, observed cameras) after the band; the importer builds the summed skyline system (band K +
    border) and solves it with its active front in LDS.  Every rank's pose step, candidate intrinsics and point steps
    equal the single engine's (pinhole, double sphere, EUCM, KB4)."""
    pb, state = intrinsics_problem(14, 200, 23, model)
    check_free_intrinsics_exchange(pb, state, world, lam)


def test_free_intrinsics_exchange_at_split_border_size():
    """The same exchange at the smallest size where enqueue_border takes its three-launch branch (nf·nc = 256·2 = 512:
    intr_border_kernel with two waves per keyframe block, intr_cam_dir_kernel, intr_cam_sch_kernel) on every rank: the
    export (X ≠ nullptr) through the split kernels, summed over two ranks, against the single engine's step."""
    pb, state = intrinsics_problem(256, 2600, 27)
    assert pb.n_frames * pb.intrinsics.shape[0] >= 512
    check_free_intrinsics_exchange(pb, state, 2, 1e-3)


def check_free_intrinsics_exchange(pb, state, world, lam):
    import torch
    fixed = (0, 1)
    with intrinsics_engine(pb, state, fixed) as full:
        c_full = full.gn_linearize()
        m_full, st_full = full.gn_step(lam)
        dp_full, dr_full = full.gn_last_step()
        full.gn_accept()
        k_full = full.get_intrinsics()
    assert st_full == 0
    sh = [(intrinsics_engine(sub, state, fixed), pids)
          for sub, pids, _ in (D.shard_problem(pb, world, r) for r in range(world))]
    try:
        costs = [e.gn_linearize() for e, _ in sh]
        assert abs(sum(costs) - c_full) <= 1e-8 * c_full
        band = max(e.gn_band() for e, _ in sh)
        n = sh[0][0].gn_exchange_size(band)
        nfs = pb.n_frames + 4
        assert n == pb.n_frames * ((E_band(band) + 1) * 36 + 24) + 4 * (nfs * 36 + 24) + 16
        bufs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in sh]
        for (e, _), b in zip(sh, bufs):
            e.gn_step_export(lam, band, b.data_ptr())
        tot = bufs[0].clone()
        for b in bufs[1:]:
            tot += b
        torch.cuda.synchronize()
        model_pts, dr, mps = 0.0, np.zeros(pb.n_points), []
        for e, pids in sh:
            mp, mq, st = e.gn_step_import(lam, band, tot.data_ptr())
            assert st == 0
            mps.append(mp)
            model_pts += mq
            dp, drs = e.gn_last_step()
            assert np.linalg.norm(dp - dp_full) <= 1e-6 * np.linalg.norm(dp_full)
            dr[pids] = drs
            e.gn_accept()
            np.testing.assert_allclose(e.get_intrinsics() - state, k_full - state,
                                       rtol=1e-6, atol=1e-9 * np.abs(k_full - state).max())
        assert max(mps) - min(mps) <= 1e-12 * abs(mps[0])  # identical pose (+ intrinsics) step on every rank
        assert abs(mps[0] + model_pts - m_full) <= 1e-8 * abs(m_full)
        np.testing.assert_allclose(dr, dr_full, rtol=1e-6, atol=1e-12 * np.abs(dr_full).max())
    finally:
        for e, _ in sh:
            e.close()


@pytest.mark.parametrize("band", [4, 8, 16])
def test_free_intrinsics_exchange_solver_paths(band):
    """The summed free-intrinsics system of a multi-GPU step through each of its solvers, with a four-camera rig (8 border
    frames): exchange band 4 — the arrow solve (band by cyclic reduction, 49 right-hand sides in 4 batches); 8 — the
    skyline Cholesky with its active front in LDS (F = 8 + 1 + 8 slots); 16 — a front of 25 slots (≈ 180 KB) that does
    not fit LDS, solved through global memory (skyline_solve_kernel) instead of failing.  Every path gives
    the single engine's step."""
    import torch
    n_cams = 4
    pb0 = synth.make_problem(kind=1, n_frames=20, n_points=260, width=376, height=240, seed=41, border=12)
    intr = np.stack([pb0.intrinsics[0] * np.array([1 + 0.01 * c, 1 - 0.01 * c, 1, 1, 1, 1, 1, 1]) for c in range(n_cams)])
    pb = synth.make_problem(kind=1, n_frames=20, n_points=260, width=376, height=240, seed=41, border=12, intrinsics=intr,
                            frame_cam=(np.arange(20) % n_cams).astype(np.int32), obs_sigma=0.3)
    state = intr * np.array([1.003, 0.998, 1.0005, 0.9995, 1, 1, 1, 1])
    fixed, lam, world = (0, 1), 1e-3, 2
    with intrinsics_engine(pb, state, fixed) as full:
        full.gn_linearize()
        m_full, st_full = full.gn_step(lam)
        dp_full, dr_full = full.gn_last_step()
    assert st_full == 0
    sh = [(intrinsics_engine(sub, state, fixed), pids)
          for sub, pids, _ in (D.shard_problem(pb, world, r) for r in range(world))]
    try:
        for e, _ in sh:
            e.gn_linearize()
        assert band >= max(e.gn_band() for e, _ in sh)
        n = sh[0][0].gn_exchange_size(band)
        bufs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in sh]
        for (e, _), b in zip(sh, bufs):
            e.gn_step_export(lam, band, b.data_ptr())
        tot = bufs[0] + bufs[1]
        torch.cuda.synchronize()
        for e, _ in sh:
            mp, mq, st = e.gn_step_import(lam, band, tot.data_ptr())
            assert st == 0
            dp, _ = e.gn_last_step()
            assert np.linalg.norm(dp - dp_full) <= 1e-6 * np.linalg.norm(dp_full), np.linalg.norm(dp - dp_full)
    finally:
        for e, _ in sh:
            e.close()


@pytest.mark.parametrize("loop", ["host", "comm"])
def test_free_intrinsics_solve_distributed_matches_solve(loop):
    """The multi-GPU LM loops with free intrinsics — host-callback sums (pba_solve_distributed) and the device-steered
    loop over an in-process pba_comm group — take pba_solve's trajectory: the same steps, final cost, poses, inverse
    distances and intrinsics."""
    import torch
    pb, state = intrinsics_problem(16, 300, 29)
    fixed = (0, 1)
    with intrinsics_engine(pb, state, fixed) as full:
        ref = full.solve(max_iterations=8)
        poses_ref, rho_ref = full.get_state()
        k_ref = full.get_intrinsics()
    world = 3
    sh = [(intrinsics_engine(sub, state, fixed), pids)
          for sub, pids, _ in (D.shard_problem(pb, world, r) for r in range(world))]
    comms = E.Comm.local_group(world) if loop == "comm" else []
    try:
        band = max(e.gn_band() for e, _ in sh)
        if loop == "comm":
            res = run_ranks(lambda r: sh[r][0].solve_distributed_comm(band, comms[r], max_iterations=8), world)
        else:
            n = sh[0][0].gn_exchange_size(band)
            bufs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in sh]
            ar = D.InProcessAllReduce(bufs, timeout=120)
            res = run_ranks(lambda r: sh[r][0].solve_distributed(band, bufs[r].data_ptr(), ar.rank(r),
                                                                 max_iterations=8), world)
        check_same_solve(pb, sh, res, ref, poses_ref, rho_ref)
        for e, _ in sh:
            np.testing.assert_allclose(e.get_intrinsics(), k_ref, rtol=1e-7)
        assert ref["final_cost"] < ref["initial_cost"]
    finally:
        for c in comms:
            c.close()
        for e, _ in sh:
            e.close()


def E_band(b):
    return 4 if b <= 4 else (8 if b <= 8 else 16)
