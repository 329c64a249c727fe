#!/usr/bin/env python3
"""What reusing a view after a camera move costs on one MI355X: Cornell 1920x1080.

Times, each the median of --reps device-event intervals on the ctx's stream after --warmup untimed calls, for a
small move of the eye (E -> (1.35, .8, -1.9)) and for the large move of the tests (I -> E):
  - spt_history_capture and spt_reproject with the captured view as three float4 images (a;
    spt_set_history_layout 0) and as one 48-byte record per pixel (b; 1), the two layouts alternating inside
    every repetition;
  - spt_history_blend (the layouts do not reach it) and spt_denoise_blended with the default parameters.
Beside each: the compulsory traffic's time at the 6.29 TB/s an MI355X streams — reproject 96 B per pixel (32 B
current features, 48 B captured view, 16 B out), blend 48 B, capture 128 B (16 B sums, 16 B history, 32 B
features in, 48 B out; 112 B without a history) — and the recorded one-frame render. Derived floors, not targets.

    python scripts/reproject_rate.py [--reps 30] [--warmup 5] [--out profiles/reproject_rates.txt]
"""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BOUNCES, RR = 1920, 1080, 8, 2
STREAM_TBS = 6.29
RENDER_US = "68.9-70.3"  # the recorded one-frame Cornell 1080p render (README)
T, VFOV = (0.0, -1.0, 5.0), 55.0
MOVES = {"small": (((1.5, 0.75, -2.0), T), ((1.35, 0.8, -1.9), T)),
         "large": (((0.0, 0.0, 4.0), (0.0, -1.0, 8.0)), ((1.5, 0.75, -2.0), T))}


def floor_us(bytes_per_pixel):
    return bytes_per_pixel * W * H / (STREAM_TBS * 1e12) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_rates.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch

    spt = importlib.import_module("software-path-tracer_amd")
    stream = torch.cuda.Stream()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def interval(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        return a, b

    def summary(pairs):
        us = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)
        return statistics.median(us), us[0], us[-1]

    def line(what, stat, floor):
        med, lo, hi = stat
        say(f"  {what:44s} {med:7.1f} us ({lo:.1f} .. {hi:.1f}); floor {floor:5.1f} us = {100.0 * floor / med:4.1f} % of it")

    with spt.Context(0) as ctx:
        ctx.set_stream(stream.cuda_stream)
        ctx.set_scene(*spt.build_scene("cornell"))
        ctx.configure(W, H, BOUNCES, RR, 0)
        ctx.specialize_scene()
        say(f"reproject rates: Cornell {W}x{H}; medians of {args.reps} after {args.warmup} warm-up (min .. max); "
            f"{torch.cuda.get_device_name(0)}")
        say(f"the one-frame Cornell render these calls stand beside: {RENDER_US} us")
        for move, ((eye0, at0), (eye1, at1)) in MOVES.items():
            old, new = spt.look_at(eye0, at0, vfov=VFOV), spt.look_at(eye1, at1, vfov=VFOV)
            samples = {k: [] for k in ("capture a", "capture b", "capture+history a", "capture+history b", "reproject a",
                                       "reproject b", "blend", "denoise_blended")}
            share = 0.0
            for k in range(args.warmup + args.reps):
                keep = k >= args.warmup
                for layout, tag in ((0, "a"), (1, "b")):
                    ctx.set_history_layout(layout)
                    ctx.set_camera(old)
                    ctx.render(0, 4)
                    ctx.render_features()
                    pair = interval(lambda: ctx.history_capture(4))
                    if keep:
                        samples[f"capture {tag}"].append(pair)
                    ctx.set_camera(new)
                    ctx.render_features()
                    pair = interval(ctx.reproject)
                    if keep:
                        samples[f"reproject {tag}"].append(pair)
                    ctx.render(0, 1)
                    pair = interval(lambda: ctx.history_capture(1))  # (with the active history blended in)
                    if keep:
                        samples[f"capture+history {tag}"].append(pair)
                pair = interval(lambda: ctx.history_blend(1))
                if keep:
                    samples["blend"].append(pair)
                pair = interval(ctx.denoise_blended)
                if keep:
                    samples["denoise_blended"].append(pair)
                if k == 0:
                    share = float(np.mean(ctx.read_history()[:, 3] > 0))
            stream.synchronize()
            say(f"{move} move, eye {eye0} -> {eye1}: {100.0 * share:.1f} % of the pixels receive history")
            for tag, name in (("a", "three images"), ("b", "48-byte records")):
                line(f"spt_history_capture, no history ({tag}) {name}", summary(samples[f"capture {tag}"]), floor_us(112))
                line(f"spt_history_capture, history    ({tag}) {name}", summary(samples[f"capture+history {tag}"]), floor_us(128))
                line(f"spt_reproject                   ({tag}) {name}", summary(samples[f"reproject {tag}"]), floor_us(96))
            line("spt_history_blend", summary(samples["blend"]), floor_us(48))
            line("spt_denoise_blended, defaults (5 levels)", summary(samples["denoise_blended"]), floor_us(5 * 64))
        ctx.set_history_layout(-1)
        ctx.synchronize()
        ctx.set_stream(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
