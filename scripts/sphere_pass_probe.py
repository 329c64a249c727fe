#!/usr/bin/env python3
"""What one sphere test costs on C2 (Cornell 1920x1080, 8 bounces, 64 frames per call, the
shape-specialized k_paths): the Cornell box against the same box with an exact duplicate of its second
sphere appended last. Equal t goes to the lower original index, so the duplicate never wins a hit and
the image is the Cornell box's, bit for bit (asserted at 96x64 over 8 frames before anything is timed);
the second scene's kernel only runs one more sphere test per step. The difference, with the root
stage's share of a sphere test's instructions (the kernel's assembly), bounds what a kernel that runs
one root stage per ray instead of one per sphere can gain. With the one-pass test (spt_device.h
flat_sphere_pass) the duplicate is a second candidate wherever its original is one, so the second
scene then prices the second pass too.

`--count` renders one call of each scene with the counting kernels and prints the wave-level second
passes of the sphere test (spt_stats.flat_sphere_second_passes) beside the wave-steps.

The two scenes alternate, `--runs` runs each; a run's time comes from one event pair around its timed
launches (SPT_PROFILE_SPAN) after a warm-up. Prints one line per run and the two means.

    python scripts/sphere_pass_probe.py [--runs 4] [--calls 20] [--warmup 5]

SQ_INSTS_VALU per launch of the two kernels comes from a counter run of its own:

    rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d DIR -- python scripts/sphere_pass_probe.py --runs 1 --calls 3 --warmup 1
    python scripts/sphere_pass_probe.py --pmc-dir DIR
"""
import argparse
import collections
import csv
import glob
import importlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BOUNCES, RR, FRAMES = 1920, 1080, 8, 2, 64
SPHERE = 7  # scenes.cpp scene_cornell: six walls, then the two spheres


def scenes(spt):
    prims, mats, env = spt.build_scene("cornell")
    dup = np.concatenate([prims, prims[[SPHERE]]])
    return (("cornell", prims, mats, env), ("cornell+1", dup, mats, env))


def pmc_summary(d):
    vals = collections.defaultdict(list)
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == "SQ_INSTS_VALU" and "k_paths" in r["Kernel_Name"]:
                vals[r["Kernel_Name"].split("(")[0].replace("void ", "").strip()].append(float(r["Counter_Value"]))
    for name, v in sorted(vals.items()):
        # (the first launch of a view still computes bounce 0 in its chunks: the maximum)
        print(f"{name}: SQ_INSTS_VALU per launch median {statistics.median(v):,.0f} (min {min(v):,.0f}, "
              f"max {max(v):,.0f}, {len(v)} launches)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4, help="runs per scene, the two scenes alternating")
    ap.add_argument("--calls", type=int, default=20, help="timed calls of 64 frames per run")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--count", action="store_true", help="also count the sphere test's second passes (one call each)")
    ap.add_argument("--pmc-dir", help="summarize a rocprofv3 --pmc SQ_INSTS_VALU csv directory and exit")
    args = ap.parse_args()
    if args.pmc_dir:
        pmc_summary(args.pmc_dir)
        return
    spt = importlib.import_module("software-path-tracer_amd")
    both = scenes(spt)
    ms = {name: [] for name, *_ in both}
    with spt.Context(0) as ctx:
        # the duplicate changes no pixel
        images = []
        for name, prims, mats, env in both:
            ctx.set_scene(prims, mats, env)
            ctx.configure(96, 64, BOUNCES, RR, 0)
            ctx.specialize_scene()
            ctx.render(0, 8)
            st = ctx.stats()
            assert int(st.specialized) == 1 and int(st.schedule) == spt.SCHEDULE_PERSISTENT, name
            images.append(ctx.read_accum().view(np.uint32).copy())
        assert np.array_equal(images[0], images[1]), "the duplicated sphere changed the image"
        print("96x64 x8 frames: the two scenes' accumulations are equal as uint32", flush=True)
        for run in range(args.runs):
            for name, prims, mats, env in both:
                ctx.set_scene(prims, mats, env)
                ctx.configure(W, H, BOUNCES, RR, 0)
                ctx.specialize_scene()  # (compiled once per shape; later runs find it in the process cache)
                frame = 0
                for _ in range(args.warmup):
                    ctx.render(frame, FRAMES)
                    frame += FRAMES
                ctx.synchronize()
                ctx.clear_stats()
                ctx.set_profiling(True, span=True)
                for _ in range(args.calls):
                    ctx.render(frame, FRAMES)
                    frame += FRAMES
                ctx.set_profiling(False)
                st = ctx.stats()
                assert int(st.specialized) == 1, name
                t = st.persistent_ms / max(1, int(st.persistent_launches))
                ms[name].append(t)
                print(f"run {run + 1} {name:10s}: {W * H * FRAMES / t / 1e6:7.2f} Gsamples/s, {t:.4f} ms per call "
                      f"({int(st.persistent_launches)} launches)", flush=True)
        if args.count:
            ctx.set_tuning(specialize=1)  # (the counting kernel is compiled on first use: wait for it)
            for name, prims, mats, env in both:
                ctx.set_scene(prims, mats, env)
                ctx.configure(W, H, BOUNCES, RR, 0)
                ctx.specialize_scene()
                ctx.clear_stats()
                ctx.set_profiling(False, counters=True)
                ctx.render(0, FRAMES)
                st = ctx.stats()
                ctx.set_profiling(False)
                assert int(st.specialized) == 1, name
                steps = int(st.lane_slots) // 64
                second = int(getattr(st, "flat_sphere_second_passes", 0))
                print(f"count {name:10s}: {second} sphere second passes in {steps} wave-steps "
                      f"({100.0 * second / max(1, steps):.2f} %), lane density {int(st.lane_busy) / max(1, int(st.lane_slots)):.3f}",
                      flush=True)
    a, b = (statistics.fmean(ms[name]) for name, *_ in both)
    print(f"mean ms per call: cornell {a:.4f} (min {min(ms['cornell']):.4f}, max {max(ms['cornell']):.4f}), "
          f"cornell+1 {b:.4f} (min {min(ms['cornell+1']):.4f}, max {max(ms['cornell+1']):.4f}): "
          f"one more sphere test costs {100.0 * (b - a) / b:.2f} % of the longer call")


if __name__ == "__main__":
    main()
