#!/usr/bin/env python3
"""What showing a variance-guided denoised frame costs on one MI355X: Cornell 1920x1080, 4 one-frame batches folded.

Times, each the median of --reps device-event intervals on the ctx's stream after --warmup untimed calls:
  - spt_denoise_guided with levels = 1 .. 5 for the straight form (a; spt_set_denoise_form 0) and the LDS-tiled form
    (b; 1), the two forms alternating inside every repetition; the time of the level at step 1 << (L - 1) is the
    difference between levels = L and levels = L - 1 (levels = 1 also holds k_guided_variance and divides by the
    frame count, so step 1's line is the level's time plus the variance kernel's);
  - k_guided_variance alone, with and without the prefilter: the kernel's device time as the profiler records it
    (the C-ABI has no call that runs it alone), the median over the same number of guided calls;
  - the whole default spt_denoise_guided (the forms the library picks, guided_form_of_step) beside the whole default
    spt_denoise, alternating inside every repetition.
Beside each level: the compulsory traffic's time, 72 B per pixel (16 B colour + 4 B variance in and out, 32 B features)
at the 6.29 TB/s an MI355X streams, as a share of the measured time. A derived floor, not a target.

    python scripts/guided_rate.py [--reps 30] [--warmup 5] [--out profiles/guided_rates.txt] [--skip-profiler]
"""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BOUNCES, RR = 1920, 1080, 8, 2
BATCHES = 4
STREAM_TBS = 6.29
FLOOR_US = 72 * W * H / (STREAM_TBS * 1e12) * 1e6
RENDER_US = "68.9-70.3"  # the recorded one-frame Cornell 1080p render (README)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_rates.txt"))
    ap.add_argument("--skip-profiler", action="store_true", help="leave k_guided_variance's own time out")
    args = ap.parse_args()
    import torch

    spt = importlib.import_module("software-path-tracer_amd")
    stream = torch.cuda.Stream()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def alternating(calls):
        """{name: (median, min, max)} in microseconds of each call's interval on the stream, the calls taking turns
        inside every repetition."""
        samples = {name: [] for name, _ in calls}
        for k in range(args.warmup + args.reps):
            for name, fn in calls:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                if k >= args.warmup:
                    samples[name].append((a, b))
        stream.synchronize()
        out = {}
        for name, pairs in samples.items():
            us = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)
            out[name] = (statistics.median(us), us[0], us[-1])
        return out

    def variance_kernel_us(ctx, prefilter):
        """The median device time of k_guided_variance over --reps guided calls, from the profiler's kernel records;
        None if the profiler records no such kernel."""
        from torch.profiler import ProfilerActivity, profile

        params = spt.GuidedParams(levels=1, prefilter=prefilter)
        for _ in range(args.warmup):
            ctx.denoise_guided(BATCHES, params)
        stream.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(args.reps):
                ctx.denoise_guided(BATCHES, params)
            stream.synchronize()
        us = sorted(float(e.device_time if hasattr(e, "device_time") else e.cuda_time)
                    for e in prof.events() if "k_guided_variance" in e.name)
        return (statistics.median(us), us[0], us[-1], len(us)) if us else None

    with spt.Context(0) as ctx:
        ctx.set_stream(stream.cuda_stream)
        ctx.set_scene(*spt.build_scene("cornell"))
        ctx.configure(W, H, BOUNCES, RR, 0)
        ctx.specialize_scene()
        say(f"guided denoise rates: Cornell {W}x{H}, {BATCHES} one-frame batches folded; medians of {args.reps} after "
            f"{args.warmup} warm-up (min .. max); {torch.cuda.get_device_name(0)}")
        say(f"compulsory traffic per level: 72 B x {W * H} pixels at {STREAM_TBS} TB/s = {FLOOR_US:.1f} us")
        for k in range(BATCHES):
            ctx.render(k, 1)
            ctx.noise_update(k + 1)
        ctx.render_features()
        # levels = 1..5 per form, the forms alternating
        totals = {"a": {}, "b": {}}
        for levels in range(1, 6):
            params = spt.GuidedParams(levels=levels)

            def run(form, params=params):
                ctx.set_denoise_form(form)
                ctx.denoise_guided(BATCHES, params)

            got = alternating([("a", lambda: run(0)), ("b", lambda: run(1))])
            for form in ("a", "b"):
                totals[form][levels] = got[form]
        ctx.set_denoise_form(-1)
        for form, name in (("a", "straight"), ("b", "LDS-tiled")):
            prev = 0.0
            for levels in range(1, 6):
                med, lo, hi = totals[form][levels]
                step_us = med - prev
                prev = med
                note = " (with k_guided_variance)" if levels == 1 else ""
                say(f"form ({form}) {name:9s} step {1 << (levels - 1):2d}: {step_us:7.1f} us{note} "
                    f"(floor {FLOOR_US:.1f} us = {100.0 * FLOOR_US / step_us:4.1f} % of it); "
                    f"levels={levels} {med:7.1f} us ({lo:.1f} .. {hi:.1f})")
        got = alternating([("guided", lambda: ctx.denoise_guided(BATCHES)), ("plain", lambda: ctx.denoise(BATCHES))])
        for name, what in (("guided", "spt_denoise_guided, defaults (variance + 5 levels, the forms kept)"),
                           ("plain", "spt_denoise, defaults (5 levels, the forms kept)")):
            med, lo, hi = got[name]
            say(f"{what}: {med:7.1f} us ({lo:.1f} .. {hi:.1f})")
        say(f"the one-frame Cornell render either follows: {RENDER_US} us")
        for prefilter in (() if args.skip_profiler else (1, 0)):
            try:
                got = variance_kernel_us(ctx, prefilter)
            except Exception as e:  # (a profiler that cannot trace is no reason to lose the event timings)
                got = None
                say(f"k_guided_variance, prefilter {prefilter}: the profiler failed: {type(e).__name__}: {e}")
            if got:
                med, lo, hi, count = got
                say(f"k_guided_variance, prefilter {prefilter}: {med:7.1f} us ({lo:.1f} .. {hi:.1f}), the profiler's device "
                    f"time of {count} launches")
            else:
                say(f"k_guided_variance, prefilter {prefilter}: no kernel record from the profiler")
        ctx.synchronize()
        ctx.set_stream(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
