#!/usr/bin/env python3
"""Diagnostic: pba_solve with affine brightness held constant (pba_gn_set_solve_affine) against the same build's plain
engine, at C3 size (200 keyframes × 20k points, 80k blocks) and C4 size (1004 keyframes × 100k points, 400k blocks),
pinhole, 8-px pattern, rendered images (synth.c4_shard, texture "render").  Three engines live in one process —
plain, affine at the zero state, affine at a state of a_f within ±0.05 and b_f within ±3 grey levels — and their
solves are interleaved (plain, zero, state, plain, …) after one warm-up solve each; prints each mode's median ms per LM
iteration with its spread, and the final costs (plain and zero must agree bit for bit); then pba_solve_affine on the
third engine, ms per LM iteration (host driven: one linearisation, one factorisation and one cost launch per trial).

    python3 tools/probe/affine_solve_probe.py                       # both sizes
    python3 tools/probe/affine_solve_probe.py --sizes c4 --repeats 9
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python3 tools/probe/affine_solve_probe.py --sizes c4 --repeats 1
                                    # kernel times: linearize_adj_kernel<0, 1, 256, false> against <0, 1, 256, true>;
                                    # affine_moments_kernel<0> against photometric_block_kernel<0, 8, 2, AffineF32> (the
                                    # cost-only launch); affine_factor_kernel's share of a pba_solve_affine iteration
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
MODES = ("plain", "affine_zero", "affine_state")


def open_engine(pb, images, mode, lib):
    eng = E.Engine(pb.kind, pb.model, huber_width=9.0, library=lib)
    eng.set_problem(pb, images_device_ptr=images.data_ptr())
    eng.set_fixed_frames(np.array([0, 1], np.int32))
    if mode != "plain":
        eng.set_affine_brightness(True)
        eng.gn_set_solve_affine(True)
        if mode == "affine_state":
            rng = np.random.default_rng(7)
            eng.set_affine_state(np.stack([rng.uniform(-0.05, 0.05, pb.n_frames), rng.uniform(-3.0, 3.0, pb.n_frames)], 1))
    return eng


def run(size, args):
    import torch
    nf, npts = SIZES[size]
    pb, images = synth.c4_shard(torch.device("cuda", 0), n_frames=nf, n_points=npts, texture="render")
    pb.poses[:2] = pb.poses_gt[:2]
    engines = {m: open_engine(pb, images, m, args.lib) for m in MODES}
    per_iter = {m: [] for m in MODES}
    last = {}
    try:
        for i in range(args.repeats + 1):  # (solve 0 of every mode: warm-up, not timed)
            for m in MODES:
                eng = engines[m]
                eng.set_state(pb.poses, pb.rho)
                s = eng.solve(max_iterations=2 if i == 0 else args.iterations, function_tolerance=0.0)
                if i > 0:
                    per_iter[m].append(s["total_ms"] / max(s["iterations"], 1))
                    last[m] = s
        # the brightness solve on the affine_state engine: pba_solve_affine from the same start, keyframe 0 fixed
        eng = engines["affine_state"]
        eng.set_state(pb.poses, pb.rho)
        ab0 = eng.get_affine_state()
        eng.set_fixed_affine_frames(np.array([0], np.int32))
        ab_iter = []
        for i in range(args.repeats + 1):
            eng.set_affine_state(ab0)
            s_ab = eng.solve_affine(max_iterations=3 if i == 0 else 10, function_tolerance=0.0)
            if i > 0:
                ab_iter.append(s_ab["total_ms"] / max(s_ab["iterations"], 1))
    finally:
        for eng in engines.values():
            eng.close()
    a = np.array(ab_iter)
    print(f"{size} solve_affine: median {np.median(a):.4f} ms per LM iteration (min {a.min():.4f}, max {a.max():.4f}, "
          f"{len(a)} solves of {s_ab['iterations']} iterations, {s_ab['successful_steps']} accepted / "
          f"{s_ab['unsuccessful_steps']} rejected, cost {s_ab['initial_cost']:.9g} -> {s_ab['final_cost']:.9g})", flush=True)
    for m in MODES:
        a, s = np.array(per_iter[m]), last[m]
        print(f"{size} {m}: {pb.n_blocks} blocks: median {np.median(a):.4f} ms per LM iteration (min {a.min():.4f}, max "
              f"{a.max():.4f}, {len(a)} solves of {s['iterations']} iterations, {s['successful_steps']} accepted / "
              f"{s['unsuccessful_steps']} rejected, cost {s['initial_cost']:.9g} -> {s['final_cost']:.9g})", flush=True)
    same = last["plain"]["final_cost"] == last["affine_zero"]["final_cost"]
    print(f"{size}: affine_zero's final cost is plain's bit for bit: {same}; affine_zero / plain "
          f"{np.median(per_iter['affine_zero']) / np.median(per_iter['plain']):.4f}, affine_state / plain "
          f"{np.median(per_iter['affine_state']) / np.median(per_iter['plain']):.4f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=E.LIB_PATH, help="the engine library to measure")
    ap.add_argument("--sizes", default="c3,c4")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    args.lib = os.path.abspath(args.lib)
    for size in args.sizes.split(","):
        run(size, args)
