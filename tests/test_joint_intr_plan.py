"""The joint solve's host plan with free intrinsics (csrc/pba_joint_plan.cpp with JointPlanInput::n_cams > 0: the cameras'
block rows behind the keyframes' skyline, a third entry per block, the border and per-camera pair lists) under
AddressSanitizer and UBSan: tests/cpp/joint_intr_plan_check.cpp, a stand-alone program with its own main.  It checks
its own random problems and the structure of the test problems, written here to a file: the six-keyframe problem, the
graphs of tests/graph_problems.py and the unseen-camera variant, each with one and with two cameras."""
import os
import subprocess
import tempfile

import numpy as np

import gn_joint_intrinsics_reference as R
import graph_problems as G
from helpers import ROOT

CSRC = os.path.join(ROOT, "photometric-bundle-adjustment_amd", "csrc")


def structures():
    """(n_frames, n_cams, frame_cam, point_host, block_point, block_target) of every problem, one and two cameras."""
    out = []
    pbs = [R.problem(), R.problem(unseen=True)] + [G.problem(n) for n in ("band37", "closed100", "closed100_idle")]
    for pb in pbs:
        nf = pb.n_frames
        for frame_cam in (np.zeros(nf, int), np.arange(nf) % 2, np.array(R.UNSEEN_FRAME_CAM) if nf == 6 else None):
            if frame_cam is not None:
                out.append((nf, int(frame_cam.max()) + 1, frame_cam, pb.point_host, pb.block_point, pb.block_target))
    return out


def test_joint_intrinsics_plan_under_sanitizers():
    items = structures()
    assert len(items) == 12 and {s[1] for s in items} == {1, 2}
    with tempfile.TemporaryDirectory() as td:
        exe, path = os.path.join(td, "joint_intr_plan_check"), os.path.join(td, "problems.txt")
        with open(path, "w") as f:
            f.write(f"{len(items)}\n")
            for nf, nc, frame_cam, point_host, block_point, block_target in items:
                f.write(f"{nf} {nc} {len(point_host)} {len(block_point)}\n")
                for a in (frame_cam, point_host, block_point, block_target):
                    f.write(" ".join(str(int(v)) for v in a) + "\n")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "joint_intr_plan_check.cpp"),
                        os.path.join(CSRC, "pba_joint_plan.cpp"), os.path.join(CSRC, "pba_gn_plan.cpp"), "-o", exe],
                       check=True, capture_output=True, text=True)
        out = subprocess.run([exe, path], check=True, capture_output=True, text=True)
    print(out.stdout)
    assert f"joint intrinsics plan: ok ({len(items)} problems from the file" in out.stdout
