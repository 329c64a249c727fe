#!/usr/bin/env python3
"""What showing a denoised frame costs on one MI355X: Cornell 1920x1080, one frame accumulated.

Times, each the median of --reps device-event intervals on the ctx's stream after --warmup untimed calls:
  - spt_render_features (one camera ray per pixel, three float4 images written);
  - spt_denoise with levels = 1 .. 5 for the straight form (a; spt_set_denoise_form 0) and the LDS-tiled form (b; 1),
    the two forms alternating inside every repetition; the time of the level at step 1 << (L - 1) is the
    difference between levels = L and levels = L - 1 (level 0 also divides by the frame count);
  - the whole default spt_denoise with the forms the library picks (atrous_form_of_step).
Beside each level: the compulsory traffic's time, 64 B per pixel (16 B colour in, 16 B out, 32 B features)
at the 6.29 TB/s an MI355X streams, as a share of the measured time. A derived floor, not a target.

    python scripts/denoise_rate.py [--reps 30] [--warmup 5] [--out profiles/denoise_rates.txt]
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
FLOOR_US = 64 * W * H / (STREAM_TBS * 1e12) * 1e6
RENDER_US = "68.9-70.3"  # the recorded one-frame Cornell 1080p render (README)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_rates.txt"))
    args = ap.parse_args()
    import torch

    spt = importlib.import_module("software-path-tracer_amd")
    stream = torch.cuda.Stream()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, before=None):
        """Median and spread in microseconds of fn's interval on the stream."""
        pairs = []
        for k in range(args.warmup + args.reps):
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            if k >= args.warmup:
                pairs.append((a, b))
        stream.synchronize()
        us = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)
        return statistics.median(us), us[0], us[-1]

    with spt.Context(0) as ctx:
        ctx.set_stream(stream.cuda_stream)
        ctx.set_scene(*spt.build_scene("cornell"))
        ctx.configure(W, H, BOUNCES, RR, 0)
        ctx.specialize_scene()
        say(f"denoise rates: Cornell {W}x{H}, 1 frame accumulated; medians of {args.reps} after {args.warmup} warm-up "
            f"(min .. max); {torch.cuda.get_device_name(0)}")
        say(f"compulsory traffic per level: 64 B x {W * H} pixels at {STREAM_TBS} TB/s = {FLOOR_US:.1f} us")
        med, lo, hi = timed(ctx.render_features, before=lambda: ctx.set_camera(None))  # (set_camera: the images are stale)
        say(f"spt_render_features: {med:7.1f} us ({lo:.1f} .. {hi:.1f})")
        ctx.render(0, 1)
        ctx.render_features()
        # levels = 1..5 per form, the forms alternating
        totals = {"a": {}, "b": {}}
        for levels in range(1, 6):
            params = spt.DenoiseParams(levels=levels)
            samples = {"a": [], "b": []}
            for k in range(args.warmup + args.reps):
                for form in ("a", "b"):
                    ctx.set_denoise_form(0 if form == "a" else 1)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    ctx.denoise(1, params)
                    b.record(stream)
                    if k >= args.warmup:
                        samples[form].append((a, b))
            stream.synchronize()
            for form in ("a", "b"):
                us = sorted(a.elapsed_time(b) * 1e3 for a, b in samples[form])
                totals[form][levels] = (statistics.median(us), us[0], us[-1])
        ctx.set_denoise_form(-1)
        for form, name in (("a", "straight"), ("b", "LDS-tiled")):
            prev = 0.0
            for levels in range(1, 6):
                med, lo, hi = totals[form][levels]
                step_us = med - prev
                prev = med
                say(f"form ({form}) {name:9s} step {1 << (levels - 1):2d}: {step_us:7.1f} us "
                    f"(floor {FLOOR_US:.1f} us = {100.0 * FLOOR_US / step_us:4.1f} % of it); "
                    f"levels={levels} {med:7.1f} us ({lo:.1f} .. {hi:.1f})")
        med, lo, hi = timed(lambda: ctx.denoise(1))
        say(f"spt_denoise, defaults (5 levels, the forms kept): {med:7.1f} us ({lo:.1f} .. {hi:.1f}); "
            f"the one-frame Cornell render it follows: {RENDER_US} us")
        ctx.synchronize()
        ctx.set_stream(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
