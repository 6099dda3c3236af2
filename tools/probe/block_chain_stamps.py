#!/usr/bin/env python3
"""Where a workgroup of the 8-lane record kernel spends its lifetime: the C4 launch (synth.c4_shard: 1000 keyframes,
100k points × 4 targets, 12,500 workgroups) with a library built with PBA_EVAL_STAMPS,

    tools/build_variant.sh stamps -DPBA_EVAL_STAMPS
    PBA_LIBRARY=variants/libpba_stamps.so python3 tools/probe/block_chain_stamps.py [OUT.txt]

Wave 0 of every workgroup stamps the 100-MHz clock at: entry | its block record arrived | the prologue's loads arrived
| barrier 1 passed | I_h arrived | row evaluated (taps, Jacobian chain, block reductions) | record stage may begin
(barrier 2 where there is one) | records staged (barrier 3 where there is one) | slab stored and acknowledged.  The
stamped kernel waits for all outstanding loads at every "arrived" stamp, which the product kernel does not: the table
splits the chain, it does not time the product.

Printed per interval: mean and 10th/90th percentile over the workgroups of dispatch rounds 2–5 (blockIdx 2048 … 10239
at 2048 resident workgroups), so the launch's fill and drain are left out; 10-ns resolution."""
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
bench = importlib.import_module("bench")
synth = importlib.import_module("photometric-bundle-adjustment_amd.synth")
E = importlib.import_module("photometric-bundle-adjustment_amd.engine")

NAMES = ["entry -> block_rec arrived", "-> prologue loads arrived", "-> barrier 1 passed", "-> I_h arrived",
         "-> row evaluated", "-> record stage may begin", "-> records staged", "-> slab stored"]
RESIDENT = 2048  # 256 CUs × 8 workgroups

if __name__ == "__main__":
    import torch
    dev = torch.device("cuda", 0)
    pb, images = synth.c4_shard(dev, n_frames=1000, n_points=100000, K=4)
    eng = E.Engine(synth.PHOTOMETRIC, synth.PINHOLE, device=0, huber_width=9.0)
    if not hasattr(eng._L, "pba_test_set_eval_stamps"):
        sys.exit("block_chain_stamps: the library has no stamps (build it with -DPBA_EVAL_STAMPS, set PBA_LIBRARY)")
    eng.set_problem(pb, images_device_ptr=images.data_ptr())
    states = bench.make_states(pb, torch, dev, 7)
    n_wg = (pb.n_blocks * 8 + 255) // 256
    buf = torch.zeros((n_wg, 16), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    set_stamps = eng._L.pba_test_set_eval_stamps
    set_stamps.argtypes, set_stamps.restype = [C.c_void_p], C.c_int
    lines = [f"block_chain_stamps: {pb.n_blocks} blocks, {n_wg} workgroups; us, workgroups {RESIDENT}..{5 * RESIDENT - 1}",
             f"library: {os.path.basename(E.LIB_PATH)}"]
    for rep in range(3):  # the first launch warms the caches; the figures are the last launch's
        assert set_stamps(buf.data_ptr()) == 0
        eng.evaluate_state_device(states[rep & 1][0].data_ptr(), states[rep & 1][1].data_ptr(), True)
        eng.synchronize()
    assert set_stamps(None) == 0
    t = buf.cpu().numpy()[:, :9].astype(np.float64) * 0.01  # 100 MHz → us
    sel = t[RESIDENT:5 * RESIDENT]
    assert (sel[:, 0] > 0).all(), "a workgroup left no stamps"
    d = np.diff(sel, axis=1)
    life = sel[:, 8] - sel[:, 0]
    lines.append(f"{'interval':32s} {'mean':>7s} {'p10':>7s} {'p90':>7s}")
    for i, name in enumerate(NAMES):
        lines.append(f"{name:32s} {d[:, i].mean():7.2f} {np.percentile(d[:, i], 10):7.2f} {np.percentile(d[:, i], 90):7.2f}")
    lines.append(f"{'workgroup lifetime':32s} {life.mean():7.2f} {np.percentile(life, 10):7.2f} {np.percentile(life, 90):7.2f}")
    lines.append(f"launch, first entry to last store: {t[:, 8].max() - t[:, 0].min():.2f} us")
    eng.close()
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
