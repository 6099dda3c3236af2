#!/usr/bin/env python3
"""Per-kernel facts from a gfx950 assembly listing (hipcc -S --cuda-device-only): the multiset of floating-point
arithmetic instructions, the vector-memory loads, barriers and VGPRs of every kernel.  Records must stay the parent's
byte for byte and the compiler re-contracts the rows' arithmetic when the code around them moves, so a
change to a block kernel is compared here, on the CPU, before any GPU run:

  tools/isa_arith.py parent.s new.s [name-filter]     kernels whose arithmetic multiset differs (exit 1 if any)
  tools/isa_arith.py new.s [name-filter]              one line per kernel
"""
import collections
import re
import subprocess
import sys

ARITH = re.compile(r"^v_(pk_)?(add|sub|subrev|mul|mul_legacy|fma|fmac|fmaak|fmamk|mad|mac|div_scale|div_fmas|div_fixup|"
                   r"rcp|rsq|sqrt|min|max|min3|max3|med3|fract|floor|ceil|trunc|rndne|ldexp|frexp_mant|exp|log|"
                   r"cvt|dot2|dot2c)_(f16|f32|f64|legacy_f32)|^v_cvt_|^v_mfma")


def kernels(path):
    out, name, cur = {}, None, None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w+):", s)
        if m:
            name, cur = m.group(1), collections.Counter()
            out[name] = cur
            continue
        if cur is None or not s or s[0] in ".;":
            if cur is not None and s.startswith(".end_amdhsa_kernel"):
                cur = None
            m = re.match(r"^\.amdhsa_next_free_vgpr (\d+)", s)
            if m and name in out:
                out[name]["#vgpr"] = int(m.group(1))
            m = re.match(r"^\.amdhsa_group_segment_fixed_size (\d+)", s)
            if m and name in out:
                out[name]["#lds"] = int(m.group(1))
            continue
        op = s.split()[0]
        if ARITH.match(op):
            cur[op] += 1
        elif op.startswith(("global_load", "buffer_load", "flat_load")):
            cur["#vmem_load"] += 1
        elif op.startswith(("global_store", "buffer_store", "flat_store")):
            cur["#vmem_store"] += 1
        elif op == "s_barrier":
            cur["#barrier"] += 1
        elif op.startswith("s_load") or op.startswith("s_buffer_load"):
            cur["#smem_load"] += 1
    return out


def demangle(names):
    # (binutils' c++filt does not know _Float16, DF16_: demangled as `short`, then renamed)
    r = subprocess.run(["c++filt"], input="\n".join(n.replace("DF16_", "s") for n in names), capture_output=True, text=True)
    if r.returncode != 0:
        return {n: n for n in names}
    return {n: (d.replace("short", "_Float16") if "DF16_" in n else d) for n, d in zip(names, r.stdout.splitlines())}


def facts(c):
    return " ".join(f"{k[1:]}={c[k]}" for k in ("#vgpr", "#lds", "#vmem_load", "#smem_load", "#vmem_store", "#barrier"))


def arith(c):
    return {k: v for k, v in c.items() if not k.startswith("#")}


def main():
    args = sys.argv[1:]
    files = [a for a in args if a.endswith(".s")]
    flt = [a for a in args if not a.endswith(".s")]
    flt = flt[0] if flt else ""
    ks = [kernels(f) for f in files]
    dm = demangle(sorted(set().union(*[set(k) for k in ks])))
    if len(ks) == 1:
        for n, c in ks[0].items():
            if flt in dm[n]:
                print(dm[n], facts(c), "arith=%d" % sum(arith(c).values()))
        return 0
    a, b = ks
    bad = 0
    for n in sorted(set(a) | set(b)):
        if flt not in dm[n]:
            continue
        if n not in a or n not in b:
            print("ONLY IN", "new" if n in b else "parent", dm[n])
            bad += 1
            continue
        if arith(a[n]) != arith(b[n]):
            bad += 1
            d = {k: (a[n].get(k, 0), b[n].get(k, 0)) for k in set(arith(a[n])) | set(arith(b[n]))
                 if a[n].get(k, 0) != b[n].get(k, 0)}
            print("ARITH DIFFERS", dm[n], d)
        elif facts(a[n]) != facts(b[n]):
            print("same arith  ", dm[n], "|", facts(a[n]), "->", facts(b[n]))
    print(f"{bad} kernels with a different arithmetic multiset of {len(set(a) | set(b))}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
