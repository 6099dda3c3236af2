"""The Gauss-Newton symbolic analysis on the host (pba_gn_plan.cpp: build_gn_plan).  It builds every index structure
the GN kernels read without checking — block order, linearise and Schur chunks with their offsets, uint8 local indices,
pair slots, skyline contribution lists, the free-intrinsics border lists and the wave table — so an error in it is an
out-of-range index inside a kernel.  The unit is plain C++ (pba_host.h, no HIP): g++ builds it with
-fsanitize=address,undefined -fno-sanitize-recover=all together with tests/cpp/gn_plan_check.cpp, which generates the
topologies (a)-(i) of its main() from a fixed LCG, checks the invariants stated in the code's comments with plain
conditions, and prints the counts and an FNV-1a hash of every plan vector.  A violated invariant or a sanitizer report
ends the driver with a non-zero exit."""
import json
import os
import subprocess
import tempfile

from helpers import ROOT

CSRC = os.path.join(ROOT, "photometric-bundle-adjustment_amd", "csrc")


def test_gn_plan_invariants_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "gn_plan_check")
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
               os.path.join(CSRC, "pba_gn_plan.cpp"), os.path.join(ROOT, "tests", "cpp", "gn_plan_check.cpp"),
               "-o", exe]
        subprocess.run(cmd, check=True, capture_output=True, text=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        env.pop("LD_PRELOAD", None)
        r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
        out = json.loads(r.stdout.strip().splitlines()[-1])
    plans = {k: v for k, v in out.items() if k != "h"}
    assert set(plans) == {"a", "a_lpb8", "b", "c", "c_lpb8", "d", "d_lpb8", "e", "f", "g"}, sorted(out)
    for name, c in plans.items():
        assert c["chunks"] > 0 and c["schur"] > 0 and c["sky"] > 0, (name, c)
        assert len(c["hash"]) == 41, (name, c)
    for name in ("b", "e", "f", "g"):  # free intrinsics: the border lists
        assert plans[name]["border"] > 0, (name, plans[name])
    assert plans["c"]["schur"] >= 3, plans["c"]  # 300 points of one host: cut at SCHUR_PTS
    assert plans["d"]["noncanon"] >= 1 and plans["d"]["target_cuts"] >= 1, plans["d"]
    assert plans["b"]["ir_waves"] > 0 and plans["e"]["ir_waves"] == 0 and plans["g"]["ir_waves"] == 0
    # (i) host 0 of (c) has ≥ 300 blocks of ≤ 4 targets: cut at 64 against 32 blocks per chunk
    assert plans["c"]["chunks"] < plans["c_lpb8"]["chunks"], (plans["c"], plans["c_lpb8"])
    assert out["h"] == {"error": "a point observes too many keyframes"}
