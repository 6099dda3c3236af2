#!/usr/bin/env python3
"""Diagnostic: pba_solve on photometric engines with the intrinsics fixed and free (pba_gn_set_solve_intrinsics) at C3 size
(200 keyframes × 20k points, 80k blocks) and C4 size (1004 keyframes × 100k points, 400k blocks), pinhole, 8-px pattern,
rendered images (synth.c4_shard, texture "render"); and the geometric free-intrinsics solve at C4 size (intr_probe.py's
case).  Prints the median ms per LM iteration of each case over --repeats solves of --iterations trials.

    python3 tools/probe/photometric_gn_intrinsics_probe.py                      # every case
    python3 tools/probe/photometric_gn_intrinsics_probe.py --lib OTHER/libpba.so --cases photo_fixed_c4,geo_free_c4
                                                # the untouched paths on another build (an A/B against a parent build:
                                                # alternate the two commands, compare the medians with the spreads)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python3 tools/probe/photometric_gn_intrinsics_probe.py --cases photo_free_c3,photo_free_c4 --repeats 1
                                                # kernel times: intr_rows_photometric_kernel (the producer), intr_pw_kernel
                                                # and the border launches intr_border*_kernel, intr_cam_*_kernel
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
CASES = ["photo_fixed_c3", "photo_free_c3", "photo_fixed_c4", "photo_free_c4", "geo_free_c4"]


def timed_solves(eng, pb, K0, iterations, repeats):
    """ms per LM iteration of `repeats` solves from the same start (after one warm-up solve), and the last summary."""
    out, s = [], None
    for i in range(repeats + 1):
        eng.set_state(pb.poses, pb.rho)
        if K0 is not None:
            eng.set_intrinsics_state(K0)
        s = eng.solve(max_iterations=2 if i == 0 else iterations, function_tolerance=0.0)
        if i > 0:
            out.append(s["total_ms"] / max(s["iterations"], 1))
    return out, s


def report(tag, lib, pb, per_iter, s):
    a = np.array(per_iter)
    print(f"{tag} [{os.path.relpath(lib, ROOT)}]: {pb.n_blocks} blocks: median {np.median(a):.4f} ms per LM iteration "
          f"(min {a.min():.4f}, max {a.max():.4f}, {len(a)} solves of {s['iterations']} iterations, "
          f"{s['successful_steps']} accepted / {s['unsuccessful_steps']} rejected, cost {s['initial_cost']:.6g} -> "
          f"{s['final_cost']:.6g})", flush=True)


def photometric(tag, size, free, args, cache):
    import torch
    dev = torch.device("cuda", 0)
    if size not in cache:
        nf, npts = SIZES[size]
        pb, images = synth.c4_shard(dev, n_frames=nf, n_points=npts, texture="render")
        pb.poses[:2] = pb.poses_gt[:2]
        cache[size] = (pb, images)
    pb, images = cache[size]
    K0 = None
    with E.Engine(pb.kind, pb.model, huber_width=9.0, library=args.lib) as eng:
        eng.set_problem(pb, images_device_ptr=images.data_ptr())
        eng.set_fixed_frames(np.array([0, 1], np.int32))
        if free:
            K0 = pb.intrinsics * (1.0 + 1e-3 * np.array([1.0, -1.0, 0.5, -0.5, 0, 0, 0, 0]))
            eng.set_optimize_intrinsics(True)
            eng.gn_set_solve_intrinsics(True)
        per_iter, s = timed_solves(eng, pb, K0, args.iterations, args.repeats)
        if free:
            print(f"{tag}: intrinsics error {np.abs(K0 - pb.intrinsics)[0, :4]} -> "
                  f"{np.abs(eng.get_intrinsics() - pb.intrinsics)[0, :4]}")
    report(tag, args.lib, pb, per_iter, s)


def geometric(tag, size, args):
    nf, npts = SIZES[size]
    pb = synth.make_problem(kind="geometric", model="pinhole", n_frames=nf, n_points=npts, K=4, seed=5,
                            with_images=False, obs_sigma=0.5)
    pb.poses[:2] = pb.poses_gt[:2]
    with E.Engine(pb.kind, pb.model, huber_width=1.0, library=args.lib) as eng:
        eng.set_problem(pb)
        eng.set_fixed_frames(np.array([0, 1], np.int32))
        eng.set_optimize_intrinsics(True)
        per_iter, s = timed_solves(eng, pb, pb.intrinsics.copy(), args.iterations, args.repeats)
    report(tag, args.lib, pb, per_iter, s)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=E.LIB_PATH, help="the engine library to measure")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    args.lib = os.path.abspath(args.lib)
    cache = {}
    for case in args.cases.split(","):
        kind, mode, size = case.split("_")
        if kind == "photo":
            photometric(case, size, mode == "free", args, cache)
        else:
            geometric(case, size, args)
