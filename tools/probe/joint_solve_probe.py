#!/usr/bin/env python3
"""Diagnostic: what one iteration of the joint solve (pba_solve_joint: poses, inverse distances and (a, b) together)
costs against one iteration each of the two solves it replaces — pba_solve with the affine state held constant
(pba_gn_set_solve_affine) plus pba_solve_affine — on the same build, at C3 size (200 keyframes × 20k points, 80k blocks)
and C4 size (1004 keyframes × 100k points, 400k blocks), pinhole, 8-px pattern, rendered images (synth.c4_shard,
texture "render").  Two engines live in one process, both with affine brightness at a state of a_f within ±0.05 and
b_f within ±3 grey levels, keyframe 0's (a, b) and the poses of keyframes 0 and 1 constant; their solves are
interleaved (joint, geometry, brightness, joint, …) from the same start after one warm-up solve each; prints each
solve's median ms per LM iteration with its spread, and the costs.

    python3 tools/probe/joint_solve_probe.py                       # both sizes, medians of 7
    python3 tools/probe/joint_solve_probe.py --sizes c4 --repeats 9
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python3 tools/probe/joint_solve_probe.py --sizes c4 --repeats 1 --only joint
                                    # the per-kernel split of a joint iteration: joint_moments_kernel<0>, joint_pair_kernel,
                                    # joint_block_kernel, joint_point_kernel, joint_frame_kernel, joint_damp_kernel,
                                    # joint_assemble_kernel, joint_gradient_kernel, joint_solve_kernel, joint_update_kernel
                                    # and the cost-only launch
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
SOLVES = ("joint", "geometry", "brightness")


def open_engine(pb, images, ab, lib, switch):
    eng = E.Engine(pb.kind, pb.model, huber_width=9.0, library=lib)
    eng.set_problem(pb, images_device_ptr=images.data_ptr())
    eng.set_fixed_frames(np.array([0, 1], np.int32))
    eng.set_affine_brightness(True)
    eng.set_affine_state(ab)
    eng.set_fixed_affine_frames(np.array([0], np.int32))
    if switch:
        eng.gn_set_solve_affine(True)
    return eng


def run(size, args):
    import torch
    nf, npts = SIZES[size]
    pb, images = synth.c4_shard(torch.device("cuda", 0), n_frames=nf, n_points=npts, texture="render")
    pb.poses[:2] = pb.poses_gt[:2]
    rng = np.random.default_rng(7)
    ab = np.stack([rng.uniform(-0.05, 0.05, pb.n_frames), rng.uniform(-3.0, 3.0, pb.n_frames)], 1)
    solves = [s for s in SOLVES if args.only in ("all", s)]
    engines = {"joint": open_engine(pb, images, ab, args.lib, False), "pair": open_engine(pb, images, ab, args.lib, True)}
    per_iter = {s: [] for s in solves}
    last = {}
    try:
        for i in range(args.repeats + 1):  # (solve 0 of every kind: warm-up, not timed)
            for s in solves:
                eng = engines["joint" if s == "joint" else "pair"]
                eng.set_state(pb.poses, pb.rho)
                eng.set_affine_state(ab)
                call = {"joint": eng.solve_joint, "geometry": eng.solve, "brightness": eng.solve_affine}[s]
                summ = call(max_iterations=2 if i == 0 else args.iterations, function_tolerance=0.0)
                if i > 0:
                    per_iter[s].append(summ["total_ms"] / max(summ["iterations"], 1))
                    last[s] = summ
    finally:
        for eng in engines.values():
            eng.close()
    med = {}
    for s in solves:
        a, summ = np.array(per_iter[s]), last[s]
        med[s] = float(np.median(a))
        print(f"{size} {s}: {pb.n_blocks} blocks: median {med[s]:.4f} ms per LM iteration (min {a.min():.4f}, max "
              f"{a.max():.4f}, {len(a)} solves of {summ['iterations']} iterations, {summ['successful_steps']} accepted / "
              f"{summ['unsuccessful_steps']} rejected, cost {summ['initial_cost']:.9g} -> {summ['final_cost']:.9g})", flush=True)
    if len(solves) == 3:
        both = med["geometry"] + med["brightness"]
        print(f"{size}: one joint iteration {med['joint']:.4f} ms against one geometry + one brightness iteration "
              f"{both:.4f} ms: {med['joint'] / both:.3f}", flush=True)


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
