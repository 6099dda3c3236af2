#!/usr/bin/env python3
"""Diagnostic: what the multi-GPU exchange of the joint solve (pba_joint_step_export / import) costs one shard, rehearsed
on ONE GPU — no run on more than one GPU exists.  At C3 size (200 keyframes × 20k points, 80k blocks, pinhole, 8-px
pattern, rendered images: synth.c4_shard, texture "render") the problem is split by host keyframe into 1 and 8 shards
(distributed.shard_problem), every shard in its own engine on the one device.  One LM-like iteration is driven from the
host, shard after shard, each stage timed on its own with the stream drained: linearise, export at λ, [the buffers summed
with torch, not a shard's stage], import (damping, constants, the replicated solve, the update), candidate cost, accept.
Prints, per number of shards, the median over the iterations of shard 0's stages and of the slowest shard's sum — what an
iteration would take next to the collectives if every shard had its own GPU — and, interleaved with them, the median ms
per LM iteration of pba_solve_joint on the whole problem (joint_solve_probe.py's problem, state and options: run that
tool from a checkout of the parent commit, alternating with this one, for the parent's figure).

    python3 tools/probe/joint_distributed_probe.py                                  # 1 and 8 shards, 10 iterations
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python3 tools/probe/joint_distributed_probe.py --shards 8 --iterations 4 --only exchange
                                    # µs per call of joint_export_kernel, joint_import_kernel, joint_solve_kernel,
                                    # joint_update_parts_kernel
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
synth = importlib.import_module("photometric-bundle-adjustment_amd.synth")
E = importlib.import_module("photometric-bundle-adjustment_amd.engine")
D = importlib.import_module("photometric-bundle-adjustment_amd.distributed")

STAGES = ("linearize", "export", "import", "candidate", "accept")
LAMBDA = 1e-4


def open_engine(pb, images, ab, lib):
    eng = E.Engine(pb.kind, pb.model, huber_width=9.0, library=lib)
    eng.set_problem(pb, images_device_ptr=images.data_ptr())
    eng.set_fixed_frames(np.array([0, 1], np.int32))
    eng.set_state(pb.poses, pb.rho)
    eng.set_affine_brightness(True)
    eng.set_affine_state(ab)
    eng.set_fixed_affine_frames(np.array([0], np.int32))
    return eng


def timed(eng, fn):
    t0 = time.perf_counter()
    out = fn()
    eng.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def exchange_iterations(pb, images, ab, world, args):
    """(per-stage ms of every shard and iteration: dict stage → (iterations, world), the costs)."""
    import torch
    engines = [open_engine(D.shard_problem(pb, world, r)[0], images, ab, args.lib) for r in range(world)]
    t = {s: np.zeros((args.iterations + 1, world)) for s in STAGES}
    costs = []
    try:
        for e in engines:
            e.joint_linearize()
        band = max(e.joint_band() for e in engines)
        bufs = [torch.zeros(e.joint_exchange_size(band), dtype=torch.float64, device="cuda") for e in engines]
        for it in range(args.iterations + 1):  # (iteration 0: warm-up, not reported)
            c = 0.0
            for r, e in enumerate(engines):
                cr, t["linearize"][it, r] = timed(e, e.joint_linearize)
                c += cr
            for r, e in enumerate(engines):
                _, t["export"][it, r] = timed(e, lambda: e.joint_step_export(LAMBDA, band, bufs[r].data_ptr()))
            tot = bufs[0].clone()
            for b in bufs[1:]:
                tot += b
            torch.cuda.synchronize()
            cand = 0.0
            for r, e in enumerate(engines):
                (_, _, st), t["import"][it, r] = timed(e, lambda: e.joint_step_import(LAMBDA, band, tot.data_ptr()))
                assert st == 0
                cc, t["candidate"][it, r] = timed(e, e.joint_candidate_cost)
                cand += cc
            costs.append(c)
            if cand < c:
                for r, e in enumerate(engines):
                    _, t["accept"][it, r] = timed(e, e.joint_accept)
    finally:
        for e in engines:
            e.close()
    return {s: v[1:] for s, v in t.items()}, costs, band


def solve_joint_ms(pb, images, ab, lib, iterations):
    eng = open_engine(pb, images, ab, lib)
    try:
        eng.solve_joint(max_iterations=2, function_tolerance=0.0)  # warm-up
        eng.set_state(pb.poses, pb.rho)
        eng.set_affine_state(ab)
        s = eng.solve_joint(max_iterations=iterations, function_tolerance=0.0)
    finally:
        eng.close()
    return s["total_ms"] / max(s["iterations"], 1), s


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=E.LIB_PATH, help="the engine library to measure")
    ap.add_argument("--shards", default="1,8")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="interleaved rounds of (exchange per shard count, solve_joint)")
    ap.add_argument("--only", default="all", choices=("all", "exchange"))
    args = ap.parse_args()
    args.lib = os.path.abspath(args.lib)
    import torch
    pb, images = synth.c4_shard(torch.device("cuda", 0), n_frames=196, n_points=20000, texture="render")
    pb.poses[:2] = pb.poses_gt[:2]
    rng = np.random.default_rng(7)
    ab = np.stack([rng.uniform(-0.05, 0.05, pb.n_frames), rng.uniform(-3.0, 3.0, pb.n_frames)], 1)
    worlds = [int(w) for w in args.shards.split(",")]
    ex = {w: [] for w in worlds}
    single = []
    for _ in range(args.repeats):
        for w in worlds:
            ex[w].append(exchange_iterations(pb, images, ab, w, args))
        if args.only == "all":
            single.append(solve_joint_ms(pb, images, ab, args.lib, args.iterations))
    for w in worlds:
        t = {s: np.concatenate([run[0][s] for run in ex[w]]) for s in STAGES}  # (rounds · iterations, shards)
        total = sum(t[s] for s in STAGES)
        costs, band = ex[w][-1][1], ex[w][-1][2]
        print(f"c3 {w} shard(s), band {band}, {pb.n_blocks} blocks, {total.shape[0]} iterations: shard 0 median ms per "
              f"iteration {np.median(total[:, 0]):.4f} (" + ", ".join(f"{s} {np.median(t[s][:, 0]):.4f}" for s in STAGES)
              + f"); slowest shard {np.median(total.max(1)):.4f} (min {total.max(1).min():.4f}, max "
              f"{total.max(1).max():.4f}); cost {costs[0]:.9g} -> {costs[-1]:.9g}", flush=True)
    if single:
        a = np.array([r[0] for r in single])
        s = single[-1][1]
        print(f"c3 pba_solve_joint: median {np.median(a):.4f} ms per LM iteration (min {a.min():.4f}, max {a.max():.4f}, "
              f"{len(a)} solves of {s['iterations']} iterations, cost {s['initial_cost']:.9g} -> {s['final_cost']:.9g})",
              flush=True)
