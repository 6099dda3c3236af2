"""The host plan of the multi-GPU joint exchange (csrc/pba_joint_plan.cpp build_joint_exchange: band profile, offsets,
per-block sources) under AddressSanitizer and UBSan: tests/cpp/joint_exchange_check.cpp, a stand-alone program with its
own main.  And the library exports the exchange's entry points."""
import ctypes
import os
import subprocess
import tempfile

from helpers import ROOT, engine_module

CSRC = os.path.join(ROOT, "photometric-bundle-adjustment_amd", "csrc")
ENTRY_POINTS = ("pba_joint_band", "pba_joint_exchange_size", "pba_joint_step_export", "pba_joint_step_import",
                "pba_solve_joint_distributed")


def test_joint_exchange_plan_under_sanitizers():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "joint_exchange_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "joint_exchange_check.cpp"),
                        os.path.join(CSRC, "pba_joint_plan.cpp"), os.path.join(CSRC, "pba_gn_plan.cpp"), "-o", exe],
                       check=True, capture_output=True, text=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "joint exchange plan: ok" in out.stdout


def test_library_exports_the_joint_exchange():
    E = engine_module()
    assert set(ENTRY_POINTS) <= set(E.header_functions())
    L = ctypes.CDLL(E.LIB_PATH)
    missing = [n for n in ENTRY_POINTS if not hasattr(L, n)]
    assert not missing, missing
