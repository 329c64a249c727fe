#!/usr/bin/env python3
"""What single VALU instructions cost in issue slots on gfx950, as multiples of v_fma_f32.

    python scripts/valu_issue_cost.py [--build-only] [--trips N] [--out profiles/valu_issue_costs.txt]

Compiles scripts/valu_issue_cost.hip for gfx950 into build/valu_issue_cost (kept if it is newer than the source; no
GPU needed for that, --build-only stops there), runs it once — one process, a few seconds — and prints a table: per
instruction the time of one instruction of one wave at 1 and at 7 waves per SIMD on every CU, and its ratio to
v_fma_f32's at the same occupancy. --out also writes the table to a file. scripts/static_profile.py's `wt` column
uses the 7-wave ratios, rounded (ISSUE_WEIGHTS there).
"""
import argparse
import collections
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "scripts", "valu_issue_cost.hip")
EXE = os.path.join(ROOT, "build", "valu_issue_cost")


def build():
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= os.path.getmtime(SRC):
        return
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-o", EXE, SRC], check=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--trips", type=int, default=8192, help="loop trips per wave, 64 instructions each")
    ap.add_argument("--out")
    args = ap.parse_args()
    build()
    if args.build_only:
        return
    raw = subprocess.run([EXE, str(args.trips)], check=True, capture_output=True, text=True, timeout=120).stdout
    rows = collections.OrderedDict()
    head = []
    for line in raw.splitlines():
        if line.startswith("#"):
            head.append(line)
            continue
        name, wps, ms, ns, x = line.split()
        rows.setdefault(name, {})[int(wps)] = (float(ms), float(ns), float(x))
    text = head[:1] + [n for n in head[1:] if n.startswith("# note")]
    text.append(f"{'instruction':16s} {'1 wave/SIMD: ns':>16s} {'x v_fma_f32':>12s} {'7 waves/SIMD: ns':>17s} {'x v_fma_f32':>12s}")
    for name, r in rows.items():
        text.append(f"{name:16s} {r[1][1]:16.4f} {r[1][2]:12.3f} {r[7][1]:17.4f} {r[7][2]:12.3f}")
    text = "\n".join(text) + "\n"
    sys.stdout.write(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
