#!/usr/bin/env python3
"""Diagnostic: what one LM iteration of the full solve (pba_solve_joint under pba_joint_set_solve_intrinsics: poses,
inverse distances, (a, b) and the cameras' intrinsics together) costs against one iteration of the joint solve at fixed
intrinsics, on the same build, at C3 size (200 keyframes × 20k points, 80k blocks) and C4 size (1004 keyframes × 100k
points, 400k blocks), pinhole, 8-px pattern, rendered images (synth.c4_shard, texture "render").  Two engines live in
one process, both with affine brightness at a state of a_f within ±0.05 and b_f within ±3 grey levels, keyframe 0's
(a, b) and the poses of keyframes 0 and 1 constant; the full engine starts its intrinsics state 0.1 % off the cameras'.
Their solves are interleaved (full, joint, full, …) from the same start after one warm-up solve each; prints each
solve's median ms per LM iteration with its spread, and the costs.

    python3 tools/probe/joint_intrinsics_probe.py                       # both sizes, medians of 7
    python3 tools/probe/joint_intrinsics_probe.py --sizes c4 --repeats 9
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python3 tools/probe/joint_intrinsics_probe.py --sizes c4 --repeats 1 --only full
                                    # the per-kernel split of a full iteration: joint_intr_moments_kernel<0>, the keyframe
                                    # kernels of the joint solve, joint_intr_pair_kernel, joint_intr_block_kernel,
                                    # joint_cam_kernel, joint_intr_assemble_kernel, joint_intr_gradient_kernel,
                                    # joint_solve_kernel, joint_intr_update_kernel and the cost-only launch
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
synth = importlib.import_module("photometric-bundle-adjustment_amd.synth")
E = importlib.import_module("photometric-bundle-adjustment_amd.engine")

SIZES = {"c3": (196, 20000), "c4": (1000, 100000)}  # (host keyframes, points): c4_shard adds the K = 4 last targets
SOLVES = ("full", "joint")


def open_engine(pb, images, ab, lib, K):
    eng = E.Engine(pb.kind, pb.model, huber_width=9.0, library=lib)
    eng.set_problem(pb, images_device_ptr=images.data_ptr())
    eng.set_fixed_frames(np.array([0, 1], np.int32))
    if K is not None:
        eng.set_intrinsics_with_affine(True)
        eng.set_optimize_intrinsics(True)
    eng.set_affine_brightness(True)
    eng.set_affine_state(ab)
    eng.set_fixed_affine_frames(np.array([0], np.int32))
    if K is not None:
        eng.set_intrinsics_state(K)
        eng.joint_set_solve_intrinsics(True)
    return eng


def run(size, args):
    import torch
    nf, npts = SIZES[size]
    pb, images = synth.c4_shard(torch.device("cuda", 0), n_frames=nf, n_points=npts, texture="render")
    pb.poses[:2] = pb.poses_gt[:2]
    rng = np.random.default_rng(7)
    ab = np.stack([rng.uniform(-0.05, 0.05, pb.n_frames), rng.uniform(-3.0, 3.0, pb.n_frames)], 1)
    K = np.array(pb.intrinsics, np.float64, copy=True)
    K[:, :4] *= 1.0 + 1e-3 * np.array([1.0, -1.0, 0.5, -0.5])
    solves = [s for s in SOLVES if args.only in ("all", s)]
    engines = {s: open_engine(pb, images, ab, args.lib, K if s == "full" else None) for s in solves}
    per_iter = {s: [] for s in solves}
    last = {}
    try:
        for i in range(args.repeats + 1):  # (solve 0 of every kind: warm-up, not timed)
            for s in solves:
                eng = engines[s]
                eng.set_state(pb.poses, pb.rho)
                eng.set_affine_state(ab)
                if s == "full":
                    eng.set_intrinsics_state(K)
                summ = eng.solve_joint(max_iterations=2 if i == 0 else args.iterations, function_tolerance=0.0)
                if i > 0:
                    per_iter[s].append(summ["total_ms"] / max(summ["iterations"], 1))
                    last[s] = summ
        size_full = engines["full"].joint_system_size() if "full" in engines else 0
    finally:
        for eng in engines.values():
            eng.close()
    med = {}
    for s in solves:
        a, summ = np.array(per_iter[s]), last[s]
        med[s] = float(np.median(a))
        print(f"{size} {s}: {pb.n_blocks} blocks, {pb.n_frames} keyframes, {pb.intrinsics.shape[0]} camera(s): median "
              f"{med[s]:.4f} ms per LM iteration (min {a.min():.4f}, max {a.max():.4f}, {len(a)} solves of "
              f"{summ['iterations']} iterations, {summ['successful_steps']} accepted / {summ['unsuccessful_steps']} "
              f"rejected, cost {summ['initial_cost']:.9g} -> {summ['final_cost']:.9g})", flush=True)
    if len(solves) == 2:
        print(f"{size}: one full iteration ({size_full} reduced unknowns) {med['full']:.4f} ms against one joint iteration "
              f"at fixed intrinsics {med['joint']:.4f} ms: {med['full'] / med['joint']:.3f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=E.LIB_PATH, help="the engine library to measure")
    ap.add_argument("--sizes", default="c3,c4")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", default="all", choices=("all",) + SOLVES)
    args = ap.parse_args()
    args.lib = os.path.abspath(args.lib)
    for size in args.sizes.split(","):
        run(size, args)
