#!/usr/bin/env python3
"""What the noise estimate costs on one MI355X, at 1920x1080 on Cornell (8 bounces), and the cadences it allows.

Kernel times come from a kernel trace: the metering waits for its result, so an event interval around the call
would hold a memset, a copy and the launch gaps besides the kernel. The script runs the traced measurement as a
child process of its own under `rocprofv3 --kernel-trace` and reads the dispatches' begin and end timestamps
(median of --reps after --warmup dispatches per kernel, min .. max):
  - k_frame, one frame per call: the frames the estimate rides beside;
  - k_noise_update after every frame;
  - k_noise_meter at radius 0, 1 and 2, one after the other (the pooled kernel has one form: the straight one,
    every tap a global load, lost at both radii and was dropped; profiles/noise_meter_grid_sweep.txt holds its
    last measurement beside the tiled form's).
Beside each: the compulsory traffic's time at the 6.29 TB/s an MI355X streams (update: 48 B per pixel; meter:
16 B read + 4 B written per pixel), as a share of the measured time. A derived floor, not a target.

A second child, without the profiler, takes host wall clock in one process:
  - one frame per call, CALLS calls and one wait: per frame, alone, with a fold every U frames, and with a fold
    every U frames and a metering every M folds (U, M: the backends' constants);
  - one metering on an idle stream (memset, kernel, 1 KB copy, wait);
  - the Python backend's render() on the App's scene (it builds its scene from spheres only) with and without a
    noise target that is never reached.
From the first child's k_noise_update and the second's frame and metering times the script derives the least
cadences that keep the folds and the waits below 5 % each of the frames they follow, and says whether the
backends' constants satisfy them.

    python scripts/noise_rate.py [--reps 30] [--warmup 5] [--out profiles/noise_rates.txt]
"""
import argparse
import csv
import glob
import importlib
import json
import math
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BOUNCES, RR = 1920, 1080, 8, 2
STREAM_TBS = 6.29
UPDATE_FLOOR_US = 48 * W * H / (STREAM_TBS * 1e12) * 1e6
METER_FLOOR_US = 20 * W * H / (STREAM_TBS * 1e12) * 1e6
CALLS = 512
SHARE = 0.05


def cornell(spt):
    ctx = spt.Context(0)
    ctx.set_scene(*spt.build_scene("cornell"))
    ctx.configure(W, H, BOUNCES, RR, 0)
    ctx.specialize_scene()
    return ctx


# ---- the children ---------------------------------------------------------------------------------------
def worker_kernels(spt, n_calls):
    ctx = cornell(spt)
    counts = {}
    for k in range(n_calls + 1):
        ctx.render(k, 1)
        ctx.noise_update(k + 1)
        if k == 0:
            continue
        for radius in (0, 1, 2):
            counts[radius] = ctx.noise_meter(radius)
    ctx.close()
    print(json.dumps({"occupied": int((counts[1] > 0).sum()), "rel_error": spt.noise_from_histogram(counts[1])}))


def per_frame_us(ctx, first, calls, update_every, meter_every):
    """CALLS one-frame calls from frame `first` on and one wait, per frame; folds and meterings by the cadences."""
    ctx.synchronize()
    folds = 0
    t0 = time.perf_counter()
    for k in range(first, first + calls):
        ctx.render(k, 1)
        if update_every and (k + 1 - first) % update_every == 0:
            ctx.noise_update(k + 1)
            folds += 1
            if meter_every and folds % meter_every == 0:
                ctx.noise_meter(1)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls


def worker_wall(spt, reps, warmup):
    U, M = spt.HIPPathTracer.NOISE_UPDATE_EVERY, spt.HIPPathTracer.NOISE_METER_EVERY
    ctx = cornell(spt)
    out = {"U": U, "M": M}
    ctx.render(0, 4)
    ctx.noise_update(4)
    at = 4
    rows = {"frames": [], "folds": [], "meterings": []}
    for rep in range(3 + 5):  # (the three loops alternating; the first three rounds are warm-up)
        for name, u, m in (("frames", 0, 0), ("folds", U, 0), ("meterings", U, M)):
            us = per_frame_us(ctx, at, CALLS, u, m)
            at += CALLS
            if rep >= 3:
                rows[name].append(us)
    for name, us in rows.items():
        out[name] = (statistics.median(us), min(us), max(us))
    us = []
    for k in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.noise_meter(1)
        if k >= warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    out["metering"] = (statistics.median(us), min(us), max(us))
    ctx.close()

    pt = spt.HIPPathTracer()
    scene = spt.Scene()
    spheres = [(0.0, -1.0, 5.0, 1.0), (0.0, -102.0, 5.0, 100.0)]
    spheres += [(float(x), float(y), 10.0, 0.5) for x in range(-5, 6, 2) for y in range(-5, 6, 2)]
    for x, y, z, r in spheres:
        node = scene.CreateNode(spt.SphereObject, "sphere")
        node.SetPosition((x, y, z))
        node.SetRadius(r)
    settings = spt.RenderSettings()
    settings.setResolution(W, H)
    pt.set_scene(scene)
    pt.set_settings(settings)
    pt.render()
    rows = {"backend_off": [], "backend_on": []}
    for rep in range(2 + 5):
        for name, target in (("backend_off", 0.0), ("backend_on", 1e-9)):
            pt.set_noise_target(target)
            pt._ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                pt.render()
            pt._ctx.synchronize()
            if rep >= 2:
                rows[name].append((time.perf_counter() - t0) * 1e6 / CALLS)
    assert not pt.converged()
    for name, us in rows.items():
        out[name] = (statistics.median(us), min(us), max(us))
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
                durations.setdefault(row["Kernel_Name"].replace(" ", ""), []).append(us)
        if traced and not durations:
            raise SystemExit(f"{task}: no kernel trace found under the profiler's output directory")
    return info, durations


def of_kernel(durations, pattern, warmup):
    """(median, min, max, dispatches) of the kernels whose name (spaces removed) matches `pattern`, after `warmup`
    dispatches of each."""
    names = [n for n in durations if re.search(pattern, n)]
    if not names:
        raise SystemExit(f"kernel {pattern}: no name matches among {sorted(durations)}")
    us = sorted(v for n in names for v in durations[n][warmup:])
    return statistics.median(us), us[0], us[-1], len(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_rates.txt"))
    ap.add_argument("--worker", help="internal: run one measurement in this process")
    args = ap.parse_args()
    if args.worker:
        spt = importlib.import_module("software-path-tracer_amd")
        if args.worker == "kernels":
            worker_kernels(spt, args.warmup + args.reps)
        else:
            worker_wall(spt, args.reps, args.warmup)
        return

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"noise rates: Cornell {W}x{H}, {BOUNCES} bounces; kernel times from a kernel trace, medians of {args.reps} "
        f"dispatches after {args.warmup} warm-up (min .. max), the three radii in turn")
    say(f"compulsory traffic at {STREAM_TBS} TB/s: k_noise_update (48 B x {W * H} pixels) = {UPDATE_FLOOR_US:.1f} us; "
        f"k_noise_meter (20 B x {W * H} pixels) = {METER_FLOOR_US:.1f} us")
    info, durations = run_child("kernels", args, traced=True)
    say(f"image: one-frame batches; the last radius-1 histogram occupies {info['occupied']} bins, "
        f"its 0.95 quantile is a relative error of {info['rel_error']:.3f}")
    fmed, flo, fhi, n = of_kernel(durations, r"k_frame", args.warmup)
    say(f"k_frame, one frame                  : {fmed:7.1f} us ({flo:.1f} .. {fhi:.1f}; {n} dispatches)")
    umed, lo, hi, n = of_kernel(durations, r"k_noise_update", args.warmup)
    say(f"k_noise_update                      : {umed:7.1f} us ({lo:.1f} .. {hi:.1f}; {n} dispatches); "
        f"floor {UPDATE_FLOOR_US:.1f} us = {100.0 * UPDATE_FLOOR_US / umed:4.1f} % of it")
    med, lo, hi, n = of_kernel(durations, r"k_noise_meter(?!_pooled)", args.warmup)
    say(f"k_noise_meter radius 0              : {med:7.1f} us ({lo:.1f} .. {hi:.1f}; {n} dispatches); "
        f"floor {METER_FLOOR_US:.1f} us = {100.0 * METER_FLOOR_US / med:4.1f} % of it")
    for radius in (1, 2):
        med, lo, hi, n = of_kernel(durations, rf"k_noise_meter_pooled<{radius}>", args.warmup)
        say(f"k_noise_meter radius {radius} (LDS tiles)  : {med:7.1f} us ({lo:.1f} .. {hi:.1f}; {n} dispatches); "
            f"floor {METER_FLOOR_US:.1f} us = {100.0 * METER_FLOOR_US / med:4.1f} % of it")

    wall, _ = run_child("wall", args, traced=False)
    U, M = wall["U"], wall["M"]
    say(f"host wall clock, one frame per call, {CALLS} calls and one wait, per frame (median of 5 rounds, the loops alternating):")
    frame = wall["frames"][0]
    for name, what in (("frames", "frames alone"), ("folds", f"a fold every {U} frames"),
                       ("meterings", f"a fold every {U} frames, a metering (radius 1) every {M} folds")):
        med, lo, hi = wall[name]
        say(f"  {what:62s}: {med:7.2f} us ({lo:.2f} .. {hi:.2f}); {100.0 * (med / frame - 1.0):+5.1f} %")
    mmed, lo, hi = wall["metering"]
    say(f"one metering on an idle stream (memset, kernel, 1 KB copy, wait), host wall clock: {mmed:7.1f} us ({lo:.1f} .. {hi:.1f})")
    need_u = max(1, math.ceil(umed / (SHARE * frame)))
    need_m = max(1, math.ceil(mmed / (SHARE * U * frame)))
    say(f"cadences: folds at most {100 * SHARE:.0f} % of the frames they follow: update_every >= {umed:.1f} / ({SHARE} x {frame:.1f}) "
        f"= {need_u}; waits at most another {100 * SHARE:.0f} %: meter_every >= {mmed:.1f} / ({SHARE} x {U} x {frame:.1f}) = {need_m}")
    say(f"the backends' constants: update_every {U}, meter_every {M}: "
        f"{'satisfy both' if U >= need_u and M >= need_m else 'DO NOT satisfy them'}")
    for name, what in (("backend_off", "no noise target"), ("backend_on", "a noise target (never reached)")):
        med, lo, hi = wall[name]
        say(f"HIPPathTracer.render(), the App's scene {W}x{H}, host wall clock per call over {CALLS} calls, {what}: "
            f"{med:7.2f} us ({lo:.2f} .. {hi:.2f})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
