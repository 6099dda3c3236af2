#!/usr/bin/env python3
"""Measurement: the 8-px record launch for camera models, interpolators and record formats other than the headline's,
at C4 size (synth.c4_shard's 400,000 blocks with the model's default camera in place of the pinhole one: the geometry
is the pinhole problem's, so some blocks leave the image — the rows are branch-free, an invalid block costs what a
valid one costs).  One engine per case; timing is the engine's own kernel timing, as in record_format_probe.py.

    [PBA_LIBRARY=variants/libpba_X.so] python3 tools/probe/block_kernel_models_probe.py [--launches 200] [--repeats 5]

Cases: instantiations whose register allocation crossed an occupancy step, either way, while DESIGN.md §24's change
was made."""
import argparse
import copy
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
bench = importlib.import_module("bench")
synth = importlib.import_module("photometric-bundle-adjustment_amd.synth")
E = importlib.import_module("photometric-bundle-adjustment_amd.engine")

# (camera model, interpolator, format)
CASES = [(synth.PINHOLE, 0, "intr"), (synth.EUCM, 0, "f16"), (synth.EUCM, 0, "affine"), (synth.KB4, 0, "f16"),
         (synth.PINHOLE, 1, "scaled"), (synth.KB4, 1, "intr"), (synth.EUCM, 0, "scaled"), (synth.PINHOLE, 1, "f16"),
         (synth.DOUBLE_SPHERE, 1, "f16"), (synth.PINHOLE, 1, "intr_affine"), (synth.DOUBLE_SPHERE, 1, "intr")]
NAMES = {synth.PINHOLE: "pinhole", synth.DOUBLE_SPHERE: "ds", synth.EUCM: "eucm", synth.KB4: "kb4"}


def launches(eng, states, n):
    eng.evaluate_states_device([states[i & 1][0].data_ptr() for i in range(n)],
                               [states[i & 1][1].data_ptr() for i in range(n)], True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    pb8, images = synth.c4_shard(dev, n_frames=1000, n_points=100000, K=4)
    states = bench.make_states(pb8, torch, dev, 7)
    print(f"block_kernel_models_probe: {pb8.n_blocks} blocks, 8 px, {args.repeats} x {args.launches} launches per case; "
          "kernel us per launch", flush=True)
    for model, interp, fmt in CASES:
        pb = copy.copy(pb8)
        pb.model = model
        pb.intrinsics = np.array([synth.DEFAULT_INTRINSICS[model]], np.float64)
        pb.interp = interp
        eng = E.Engine(synth.PHOTOMETRIC, model, device=0, huber_width=9.0)
        eng.set_problem(pb, images_device_ptr=images.data_ptr())
        if fmt == "f16":
            eng.set_record_format(E.RECORD_F16)
        if fmt == "scaled":
            eng.set_record_format(E.RECORD_F16_SCALED)
        if fmt == "intr_affine":
            eng.set_intrinsics_with_affine(True)
        if fmt in ("intr", "intr_affine"):
            eng.set_optimize_intrinsics(True)
        if fmt in ("affine", "intr_affine"):
            eng.set_affine_brightness(True)
        eng.enable_kernel_timing(True)
        us = []
        for _ in range(args.repeats):
            launches(eng, states, args.warmup)
            eng.kernel_timing()  # reset
            launches(eng, states, args.launches)
            ms, n = eng.kernel_timing()
            us.append(1e3 * ms / n)
        eng.close()
        a = np.array(us)
        print(f"  {NAMES[model]:8s} {'bicubic ' if interp else 'bilinear'} {fmt:7s} median {np.median(a):7.2f} us"
              f"  min {a.min():7.2f}  max {a.max():7.2f}", flush=True)
