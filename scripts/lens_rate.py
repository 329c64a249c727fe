#!/usr/bin/env python3
"""What a thin lens costs on C2 (Cornell 1920x1080, 8 bounces, 64 frames per call, k_paths): the rate in five
camera modes — none (the reference's pinhole), posed (look_at from (1.5, 0.75, -2), 55 degrees), jitter
(SPT_CAMERA_JITTER), lens (the posed camera with a lens of radius 0.1 focused at 6.0) and lens+jitter. The
last three run the per-path form of k_paths (every path traces its own camera segment). Measured as
scripts/camera_rate.py measures: one event pair around the timed launches (SPT_PROFILE_SPAN) after a warm-up;
the traced segments of a call are counted once, with the counting kernels, outside the timed calls
(per-pixel cameras: bounce 0 is traced once per pixel and launch). One line per mode: Gsamples/s and traced
G segments/s.

    python scripts/lens_rate.py [--calls 20] [--warmup 10] [--modes none,posed,jitter,lens,lens+jitter]

With SPT_LIB_PATH naming a library built from a commit without the lens, --modes none,posed measures that
commit's rates (the A/B of profiles/lens_rates.txt).
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BOUNCES, RR, FRAMES = 1920, 1080, 8, 2, 64
EYE, TARGET, VFOV = (1.5, 0.75, -2.0), (0.0, -1.0, 5.0), 55.0
LENS = (0.1, 6.0)
MODES = ("none", "posed", "jitter", "lens", "lens+jitter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="timed calls of 64 frames per mode")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--modes", default=",".join(MODES))
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    assert all(m in MODES for m in modes), modes
    spt = importlib.import_module("software-path-tracer_amd")
    with spt.Context(0) as ctx:
        ctx.set_scene(*spt.build_scene("cornell"))
        ctx.configure(W, H, BOUNCES, RR, 0)
        for name in modes:
            cam = None if name == "none" else spt.look_at(EYE, TARGET, vfov=VFOV, jitter="jitter" in name)
            ctx.set_camera(cam)
            if "lens" in name:
                ctx.set_camera_lens(*LENS)
            elif cam is not None and hasattr(ctx.lib, "spt_set_camera_lens"):
                ctx.set_camera_lens(None)
            per_path = name not in ("none", "posed")
            ctx.specialize_scene()  # the flat shape's kernels (a per-path camera runs the generic ones)
            # the traced segments of one call, from the counting kernels
            ctx.set_profiling(False, counters=True)
            ctx.clear_stats()
            ctx.render(0, FRAMES)
            st = ctx.stats()
            seg = [int(x) for x in st.segments[:BOUNCES]]
            traced = sum(seg) if per_path else sum(seg[1:]) + W * H
            ctx.set_profiling(False)
            frame = FRAMES
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
            ms = st.persistent_ms / max(1, int(st.persistent_launches))
            samples = W * H * FRAMES
            print(f"camera {name:11s}: {samples / ms / 1e6:7.2f} Gsamples/s, {traced / ms / 1e6:7.2f} G traced segments/s "
                  f"({ms:.3f} ms per call of {FRAMES} frames, {traced / samples:.3f} traced segments per sample, "
                  f"specialized {int(st.specialized)}, {int(st.persistent_launches)} launches)", flush=True)


if __name__ == "__main__":
    main()
