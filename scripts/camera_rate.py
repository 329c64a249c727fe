#!/usr/bin/env python3
"""What a camera costs on C2 (Cornell 1920x1080, 8 bounces, 64 frames per call, k_paths): the rate
without a camera (the reference's pinhole), with a posed camera (look_at from (1.5, 0.75, -2), 55
degrees), and with the same camera jittered (SPT_CAMERA_JITTER: every path traces its own camera
segment, the kJitter form of k_paths). Times come from one event pair around the timed launches
(SPT_PROFILE_SPAN) after a warm-up; the traced segments of a call are counted once, with the counting
kernels, outside the timed calls: segments at bounce >= 1, plus one camera segment per pixel and launch
(no jitter: bounce 0 is traced once per pixel and reused by every frame) or per path (jitter). Prints
one line per camera: Gsamples/s and traced G segments/s.

    python scripts/camera_rate.py [--calls 20] [--warmup 10]
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BOUNCES, RR, FRAMES = 1920, 1080, 8, 2, 64
EYE, TARGET, VFOV = (1.5, 0.75, -2.0), (0.0, -1.0, 5.0), 55.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="timed calls of 64 frames per camera")
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    spt = importlib.import_module("software-path-tracer_amd")
    cameras = (("none", None), ("posed", spt.look_at(EYE, TARGET, vfov=VFOV)),
               ("jitter", spt.look_at(EYE, TARGET, vfov=VFOV, jitter=True)))
    with spt.Context(0) as ctx:
        ctx.set_scene(*spt.build_scene("cornell"))
        ctx.configure(W, H, BOUNCES, RR, 0)
        for name, cam in cameras:
            ctx.set_camera(cam)
            ctx.specialize_scene()  # the flat shape's kernels (a jittered camera runs the generic ones)
            # the traced segments of one call, from the counting kernels
            ctx.set_profiling(False, counters=True)
            ctx.clear_stats()
            ctx.render(0, FRAMES)
            st = ctx.stats()
            seg = [int(x) for x in st.segments[:BOUNCES]]
            traced = sum(seg) if cam is not None and cam.flags & spt.CAMERA_JITTER else sum(seg[1:]) + W * H
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
            print(f"camera {name:6s}: {samples / ms / 1e6:7.2f} Gsamples/s, {traced / ms / 1e6:7.2f} G traced segments/s "
                  f"({ms:.3f} ms per call of {FRAMES} frames, {traced / samples:.3f} traced segments per sample, "
                  f"specialized {int(st.specialized)}, {int(st.persistent_launches)} launches)", flush=True)


if __name__ == "__main__":
    main()
