#!/usr/bin/env python3
"""What metering and displaying a frame costs on one MI355X, at 1920x1080.

Kernel times come from a kernel trace: the meter and display entry points wait for their result, so an event
interval around a call would hold a memset, a copy and the launch gaps besides the kernel. This script therefore
runs each measurement as a child process of its own under `rocprofv3 --kernel-trace` and reads the dispatches'
begin and end timestamps (median of --reps after --warmup dispatches per kernel, min .. max):
  - k_meter in form 0 (an LDS add per lane) and form 1 (an add per distinct bin of a wave), alternating, on three
    images: Cornell after CONVERGED frames (concentrated bins), Cornell after 1 frame, and a uniformly random
    log-luminance image (spread bins);
  - k_display per operator beside k_resolve, alternating, on Cornell after 8 frames (through the staging image).
Beside each: the compulsory traffic's time (k_meter 16 B read per pixel + 1 KB; k_display 16 B read + 4 B written
per pixel) at the 6.29 TB/s an MI355X streams, as a share of the measured time. A derived floor, not a target.
  - the Python backend's whole get_render_result() with auto-exposure and ACES beside the plain one: host wall
    clock around the call (no profiler), the App's scene, 1 sample per pixel accumulated.

    python scripts/display_rate.py [--reps 30] [--warmup 5] [--out profiles/display_rates.txt]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BOUNCES, RR = 1920, 1080, 8, 2
CONVERGED = 128
STREAM_TBS = 6.29
METER_FLOOR_US = (16 * W * H + 1024) / (STREAM_TBS * 1e12) * 1e6
DISPLAY_FLOOR_US = 20 * W * H / (STREAM_TBS * 1e12) * 1e6
IMAGES = {"converged": f"Cornell, {CONVERGED} frames", "onespp": "Cornell, 1 frame", "random": "random log-luminance"}
OPERATORS = {"clamp": 0, "reinhard": 1, "aces": 2}


# ---- the children ---------------------------------------------------------------------------------------
def cornell(spt, frames):
    ctx = spt.Context(0)
    ctx.set_scene(*spt.build_scene("cornell"))
    ctx.configure(W, H, BOUNCES, RR, 0)
    ctx.specialize_scene()
    ctx.render(0, frames)
    ctx.synchronize()
    return ctx


def worker_meter(spt, image, n_calls):
    import numpy as np
    import torch

    if image == "random":
        rng = np.random.default_rng(1)
        img = np.exp2(rng.uniform(-16.0, 16.0, size=(W * H, 1))).astype(np.float32).repeat(4, axis=1)
        t = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        ctx = spt.Context(0)
        meter = lambda: ctx.meter_device_image(t.data_ptr(), W * H, 1.0)  # noqa: E731
    else:
        frames = CONVERGED if image == "converged" else 1
        ctx = cornell(spt, frames)
        meter = lambda: ctx.meter_luminance(frames)  # noqa: E731
    counts = None
    for _ in range(n_calls):
        for form in (0, 1):
            ctx.set_meter_form(form)
            got = meter()
            assert counts is None or (got == counts).all()
            counts = got
    ctx.close()
    top = sorted((int(c) for c in counts), reverse=True)
    print(json.dumps({"occupied": int((counts > 0).sum()), "top2_share": (top[0] + top[1]) / float(W * H)}))


def worker_display(spt, op, n_calls):
    ctx = cornell(spt, 8)
    d = spt.Display(OPERATORS[op], 1.5)
    for _ in range(n_calls):
        ctx.resolve_rgba8(8, 1.5)
        ctx.resolve_display_rgba8(8, d)
    ctx.close()
    print(json.dumps({}))


def worker_backend(spt, reps, warmup):
    pt = spt.HIPPathTracer(settings_mode=True)
    scene = spt.Scene()
    spheres = [(0.0, -1.0, 5.0, 1.0), (0.0, -102.0, 5.0, 100.0)]
    spheres += [(float(x), float(y), 10.0, 0.5) for x in range(-5, 6, 2) for y in range(-5, 6, 2)]
    for x, y, z, r in spheres:
        node = scene.CreateNode(spt.SphereObject, "sphere")
        node.SetPosition((x, y, z))
        node.SetRadius(r)
    settings = spt.RenderSettings()
    settings.setResolution(W, H)
    settings.setSamplesPerPixel(1)
    pt.set_scene(scene)
    pt.set_settings(settings)
    out = {}
    for name, auto, op in (("plain", False, spt.TONEMAP_CLAMP), ("metered", True, spt.TONEMAP_ACES)):
        settings.setAutoExposure(auto)
        pt.set_tonemap(op)
        pt.render()
        us = []
        for k in range(warmup + reps):
            t0 = time.perf_counter()
            pt.get_render_result()
            if k >= warmup:
                us.append((time.perf_counter() - t0) * 1e6)
        us.sort()
        out[name] = (statistics.median(us), us[0], us[-1])
    print(json.dumps(out))


# ---- the parent -------------------------------------------------------------------------------------------
def run_child(task, args, traced):
    """Run `task` in a child; returns (its JSON line, {kernel name: [dispatch durations in us, in order]})."""
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", task, "--reps", str(args.reps), "--warmup", str(args.warmup)]
    with tempfile.TemporaryDirectory() as tmp:
        if traced:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--"] + cmd
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"{task}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        info = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        durations = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                rows = sorted(csv.DictReader(f), key=lambda row: int(row["Start_Timestamp"]))
            for row in rows:
                us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                durations.setdefault(row["Kernel_Name"], []).append(us)
        if traced and not durations:
            raise SystemExit(f"{task}: no kernel trace found under the profiler's output directory")
    return info, durations


def of_kernel(durations, needle, warmup):
    """(median, min, max, dispatches) of the kernel whose name holds `needle`, after `warmup` dispatches."""
    names = [n for n in durations if needle in n]
    if len(names) != 1:
        raise SystemExit(f"kernel {needle}: {len(names)} names match among {sorted(durations)}")
    us = sorted(durations[names[0]][warmup:])
    return statistics.median(us), us[0], us[-1], len(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display_rates.txt"))
    ap.add_argument("--worker", help="internal: run one measurement in this process")
    args = ap.parse_args()
    if args.worker:
        spt = importlib.import_module("software-path-tracer_amd")
        kind, _, what = args.worker.partition(":")
        if kind == "meter":
            worker_meter(spt, what, args.warmup + args.reps)
        elif kind == "display":
            worker_display(spt, what, args.warmup + args.reps)
        else:
            worker_backend(spt, args.reps, args.warmup)
        return

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"display rates: {W}x{H}; kernel times from a kernel trace, medians of {args.reps} dispatches after "
        f"{args.warmup} warm-up (min .. max), the two kernels of a line's group alternating")
    say(f"compulsory traffic at {STREAM_TBS} TB/s: k_meter (16 B x {W * H} pixels + 1 KB) = {METER_FLOOR_US:.1f} us; "
        f"k_display (20 B x {W * H} pixels) = {DISPLAY_FLOOR_US:.1f} us")
    for image, label in IMAGES.items():
        info, durations = run_child(f"meter:{image}", args, traced=True)
        say(f"image: {label}: {info['occupied']} bins occupied, the two fullest hold {100.0 * info['top2_share']:.1f} % of the pixels")
        for form, name in ((0, "an add per lane"), (1, "an add per distinct bin")):
            med, lo, hi, n = of_kernel(durations, f"k_meter<{form}>", args.warmup)
            say(f"  k_meter form {form} ({name:23s}): {med:7.1f} us ({lo:.1f} .. {hi:.1f}; {n} dispatches); "
                f"floor {METER_FLOOR_US:.1f} us = {100.0 * METER_FLOOR_US / med:4.1f} % of it")
    for op in OPERATORS:
        _, durations = run_child(f"display:{op}", args, traced=True)
        med, lo, hi, n = of_kernel(durations, "k_display", args.warmup)
        rmed, rlo, rhi, _ = of_kernel(durations, "k_resolve", args.warmup)
        say(f"k_display {op:8s}: {med:7.1f} us ({lo:.1f} .. {hi:.1f}; {n} dispatches); floor {DISPLAY_FLOOR_US:.1f} us = "
            f"{100.0 * DISPLAY_FLOOR_US / med:4.1f} % of it; k_resolve beside it: {rmed:7.1f} us ({rlo:.1f} .. {rhi:.1f})")
    info, _ = run_child("backend", args, traced=False)
    for name, what in (("plain", "auto-exposure off, CLAMP (the plain resolve)"),
                       ("metered", "auto-exposure on, ACES (meter, exposure, display resolve)")):
        med, lo, hi = info[name]
        say(f"HIPPathTracer.get_render_result(), host wall clock, {what}: {med:7.1f} us ({lo:.1f} .. {hi:.1f})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
