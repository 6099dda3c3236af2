#!/usr/bin/env python3
"""Diagnostic: is the device LM loop reproducible?  Builds the C4 problem (seeded), then runs the same sequence of
calls several times in one process — linearise at the initial state, one host-driven step, a pba_solve — and prints
a hash of every result, so two processes (or two calls) can be compared bit for bit.

    python tools/det_probe.py [--frames 1000 --points 100000] [--repeats 2]
    python tools/det_probe.py --geometric --intrinsics --frames 24 --cameras 2 --points 300 [--library libpba_test.so]

--geometric: a reprojection rig instead of the photometric shard; --intrinsics: with free intrinsics (intr_rows_kernel and
the border kernels; the intrinsics are hashed with the state).  --library: the engine build to load, so two builds can be
compared by the same script (PBA_TEST_BORDER=fused|split acts on the test build).
"""
import argparse
import hashlib
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
synth = importlib.import_module("photometric-bundle-adjustment_amd.synth")
E = importlib.import_module("photometric-bundle-adjustment_amd.engine")


def h(*arrays):
    m = hashlib.sha1()
    for a in arrays:
        m.update(memoryview(a).cast("B"))
    return m.hexdigest()[:12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--geometric", action="store_true")
    ap.add_argument("--intrinsics", action="store_true")
    ap.add_argument("--cameras", type=int, default=2)
    ap.add_argument("--library", default=None)
    args = ap.parse_args()
    import numpy as np
    if args.geometric:
        return geometric(args, np)
    import torch
    dev = torch.device("cuda", 0)
    pb, images = synth.c4_shard(dev, n_frames=args.frames, n_points=args.points)
    print("problem", h(np.ascontiguousarray(pb.poses), np.ascontiguousarray(pb.rho),
                       np.ascontiguousarray(pb.host_intensity)), "images", h(images.cpu().numpy()), flush=True)
    eng = E.Engine(synth.PHOTOMETRIC, synth.PINHOLE, device=0, huber_width=9.0, library=args.library)
    eng.set_problem(pb, images_device_ptr=images.data_ptr())
    eng.set_fixed_frames(np.array([0, 1], np.int32))
    for rep in range(args.repeats):
        eng.set_state(pb.poses, pb.rho)
        c0 = eng.gn_linearize()
        eng.gn_step(1e-4)
        S, g = eng.gn_reduced_system()  # the system gn_step assembled
        step = eng.gn_last_step()
        cc = eng.gn_candidate_cost()
        eng.set_state(pb.poses, pb.rho)
        s = eng.solve(max_iterations=args.iters, function_tolerance=0.0)
        poses, rho = eng.get_state()
        print(f"rep {rep}: cost0 {c0!r} S {h(np.ascontiguousarray(S))} g {h(np.ascontiguousarray(g))} "
              f"dposes {h(np.ascontiguousarray(step[0]))} drho {h(np.ascontiguousarray(step[1]))} "
              f"cand {cc!r} | solve it {s['iterations']} ok {s['successful_steps']} final {s['final_cost']!r} "
              f"state {h(np.ascontiguousarray(poses), np.ascontiguousarray(rho))}", flush=True)
    eng.close()


def geometric(args, np):
    """The same sequence on a rig of --cameras cameras (keyframe f uses camera f % cameras) whose intrinsics state differs
    from the cameras the hosts unproject with."""
    kw = dict(kind=1, model=0, n_frames=args.frames, n_points=args.points, width=376, height=240, seed=53, border=12)
    k0 = synth.make_problem(**kw).intrinsics[0]
    intr = np.stack([k0 * np.array([1 + 0.01 * c, 1 - 0.01 * c, 1, 1, 1, 1, 1, 1]) for c in range(args.cameras)])
    pb = synth.make_problem(**kw, intrinsics=intr, frame_cam=(np.arange(args.frames) % args.cameras).astype(np.int32),
                            obs_sigma=0.3)
    state = intr * np.array([1.003, 0.998, 1.0005, 0.9995, 1, 1, 1, 1])
    print("problem", h(np.ascontiguousarray(pb.poses), np.ascontiguousarray(pb.rho), np.ascontiguousarray(pb.u_obs)),
          "blocks", pb.n_blocks, flush=True)
    eng = E.Engine(pb.kind, pb.model, device=0, huber_width=1.0, library=args.library)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array([0, 1], np.int32))
    for rep in range(args.repeats):
        eng.set_state(pb.poses, pb.rho)
        if args.intrinsics:
            eng.set_optimize_intrinsics(True)
            eng.set_intrinsics_state(state)
        c0 = eng.gn_linearize()
        eng.gn_step(1e-4)
        S, g = eng.gn_reduced_system()
        step = eng.gn_last_step()
        cc = eng.gn_candidate_cost()
        eng.set_state(pb.poses, pb.rho)
        if args.intrinsics:
            eng.set_intrinsics_state(state)
        s = eng.solve(max_iterations=args.iters, function_tolerance=0.0)
        poses, rho = eng.get_state()
        k = eng.get_intrinsics() if args.intrinsics else np.zeros(0)
        print(f"rep {rep}: cost0 {c0!r} S {h(np.ascontiguousarray(S))} g {h(np.ascontiguousarray(g))} "
              f"dposes {h(np.ascontiguousarray(step[0]))} drho {h(np.ascontiguousarray(step[1]))} "
              f"cand {cc!r} | solve it {s['iterations']} ok {s['successful_steps']} final {s['final_cost']!r} "
              f"state {h(np.ascontiguousarray(poses), np.ascontiguousarray(rho), np.ascontiguousarray(k))}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
