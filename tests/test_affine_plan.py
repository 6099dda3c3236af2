"""The brightness solve's host plan (csrc/pba_affine_plan.cpp: block → pair → keyframe lists and the skyline profile)
under AddressSanitizer and UBSan: tests/cpp/affine_plan_check.cpp, a stand-alone program with its own main."""
import os
import subprocess
import tempfile

from helpers import ROOT

CSRC = os.path.join(ROOT, "photometric-bundle-adjustment_amd", "csrc")


def test_affine_plan_under_sanitizers():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "affine_plan_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "affine_plan_check.cpp"),
                        os.path.join(CSRC, "pba_affine_plan.cpp"), "-o", exe], check=True, capture_output=True, text=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "affine plan: ok" in out.stdout
