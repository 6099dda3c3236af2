#!/usr/bin/env python3
"""Diagnostic: everything a caller can observe of the brightness solve, the joint solve and pba_solve on the
six-keyframe problems of tests/gn_affine_reference.py, as bytes — to compare two builds of the engine bit for bit
(the shared host LM loop and device helpers of DESIGN.md §21 must change nothing).

Problems: problem() (644 blocks, P = 8, pinhole), its P = 12, cams = 2 variant and its KB4, interp = 1 variant; poses
of keyframes 0 and 1 and (a, b) of keyframe 0 constant, (a, b) = 0 at the start.
Per problem: solve_affine and solve_joint at the default options and solve_joint(**LM_REJECT) — the summary without
total_ms, every pba_iteration_summary, the final poses, ρ and (a, b); one joint_linearize + joint_step(1e-3) — cost,
model decrease, the dense reduced system, gradient, step and candidate cost; pba_solve at the affine state held
constant — the summary and the final state.

    python3 tools/probe/host_lm_probe.py OUT.txt                       # this build
    PBA_LIBRARY=/path/to/other/libpba.so python3 tools/probe/host_lm_probe.py OTHER.txt
    cmp OUT.txt OTHER.txt

Every line is a name and the value's bytes in hex (arrays: sha256 of the bytes and the shape), so equal files mean
equal bits.
"""
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # (the references' `import oracle` is oracle/oracle.py)
synth = importlib.import_module("photometric-bundle-adjustment_amd.synth")
E = importlib.import_module("photometric-bundle-adjustment_amd.engine")
import gn_affine_reference as GA  # noqa: E402
import gn_joint_reference as GJ  # noqa: E402

PROBLEMS = {"base": {}, "P12_cams2": dict(P=12, cams=2), "kb4_interp1": dict(model=synth.KB4, interp=1)}
TIMES = ("total_ms", "linearize_ms", "solve_ms", "cost_ms")


def open_engine(pb, switch):
    eng = E.Engine(pb.kind, pb.model, huber_width=GA.HUBER)
    eng.set_problem(pb)
    eng.set_fixed_frames(np.array(GJ.FIXED, np.int32))
    eng.set_state(pb.poses, pb.rho)
    eng.set_affine_brightness(True)
    eng.set_fixed_affine_frames(np.array(GJ.FIXED_AB, np.int32))
    if switch:
        eng.gn_set_solve_affine(True)
    return eng


def emit(out, name, value):
    if isinstance(value, np.ndarray):
        a = np.ascontiguousarray(value)
        out.append(f"{name} {a.dtype} {a.shape} sha256 {hashlib.sha256(a.tobytes()).hexdigest()}")
    elif isinstance(value, float):
        out.append(f"{name} {value.hex()} ({value!r})")
    else:
        out.append(f"{name} {value!r}")


def emit_solve(out, name, eng, summ):
    for k in sorted(summ):
        if k not in TIMES:
            emit(out, f"{name}.summary.{k}", summ[k])
    its = eng.solver_iterations()
    for k in sorted(its):
        emit(out, f"{name}.iterations.{k}", its[k])
        if its[k].dtype.kind == "f":
            for i, v in enumerate(its[k]):
                emit(out, f"{name}.iterations.{k}[{i}]", float(v))
    poses, rho = eng.get_state()
    emit(out, f"{name}.poses", poses)
    emit(out, f"{name}.rho", rho)
    emit(out, f"{name}.ab", eng.get_affine_state())


def probe(out, label, pb):
    for name, call, kw in (("solve_affine", "solve_affine", {}), ("solve_joint", "solve_joint", {}),
                           ("solve_joint_reject", "solve_joint", GJ.LM_REJECT)):
        with open_engine(pb, False) as eng:
            emit_solve(out, f"{label}.{name}", eng, getattr(eng, call)(**kw))
    with open_engine(pb, False) as eng:
        emit(out, f"{label}.joint.cost", float(eng.joint_linearize()))
        m, st = eng.joint_step(1e-3)
        emit(out, f"{label}.joint.model_decrease", float(m))
        emit(out, f"{label}.joint.status", int(st))
        S, g = eng.joint_get_reduced_system()
        dk, dr = eng.joint_get_step()
        for k, v in (("S", S), ("g", g), ("d_keyframes", dk), ("d_inv_dist", dr)):
            emit(out, f"{label}.joint.{k}", v)
        emit(out, f"{label}.joint.candidate_cost", float(eng.joint_candidate_cost()))
    with open_engine(pb, True) as eng:
        emit_solve(out, f"{label}.solve", eng, eng.solve())


if __name__ == "__main__":
    lines = [f"# host_lm_probe: {len(PROBLEMS)} problems"]
    for label, kw in PROBLEMS.items():
        probe(lines, label, GA.problem(**kw))
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {sys.argv[1]} (library {E.LIB_PATH})")
