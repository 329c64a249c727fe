#!/usr/bin/env python3
"""What material models cost on C2 (Cornell 1920x1080, 8 bounces, 64 frames per call, k_paths): the rate
as today (no models: the shape-specialized kernel with its per-pixel bounce 0), with the two spheres
METAL(0) and DIELECTRIC(1.5) on material entries of their own (the kBsdf form of k_paths: generic, every
path starts at bounce 0), and the same with next-event estimation (--nee). Times come from one event pair
around the timed launches (SPT_PROFILE_SPAN) after a warm-up; the traced segments of a call are counted
once, with the counting kernels, outside the timed calls: segments at bounce >= 1 plus one camera segment
per pixel and launch without models (bounce 0 is traced once per pixel and reused by every frame), every
segment with them; with NEE the shadow rays are traced segments too. Writes one line per configuration,
Gsamples/s and traced G segments/s, to --out (and prints it).

    python scripts/material_rate.py [--calls 20] [--warmup 10] [--out profiles/material_rates.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BOUNCES, RR, FRAMES = 1920, 1080, 8, 2, 64


def cornell_with_sphere_materials(spt):
    """Cornell with each sphere on a material entry of its own (the white wall's values), and the models
    that make the first a mirror and the second glass."""
    prims, mats, env = spt.build_scene("cornell")
    prims = prims.copy()
    spheres = [i for i in range(len(prims)) if prims[i]["type"] == 0]
    models = [(spt.MAT_DIFFUSE, 0.0)] * len(mats)
    for i, model in zip(spheres, ((spt.MAT_METAL, 0.0), (spt.MAT_DIELECTRIC, 1.5))):
        mats = np.concatenate([mats, mats[prims[i]["material"]:prims[i]["material"] + 1]])
        prims[i]["material"] = len(mats) - 1
        models.append(model)
    return prims, mats, env, models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="timed calls of 64 frames per configuration")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "material_rates.txt"))
    args = ap.parse_args()
    spt = importlib.import_module("software-path-tracer_amd")
    prims, mats, env, models = cornell_with_sphere_materials(spt)
    configs = (("as today", None, 0), ("metal + glass", models, 0), ("metal + glass, NEE", models, spt.FLAG_NEE))
    lines = [f"# python scripts/material_rate.py  (C2: Cornell {W}x{H}, {BOUNCES} bounces, {FRAMES} frames per call, "
             f"{args.calls} timed calls per configuration)"]
    with spt.Context(0) as ctx:
        for name, mdl, flags in configs:
            ctx.set_scene(prims, mats, env)
            ctx.configure(W, H, BOUNCES, RR, flags)
            ctx.set_material_models(mdl)
            ctx.specialize_scene()  # the flat shape's kernels (a scene with models runs the generic ones)
            # the traced segments of one call, from the counting kernels
            ctx.set_profiling(False, counters=True)
            ctx.clear_stats()
            ctx.render(0, FRAMES)
            st = ctx.stats()
            seg = [int(x) for x in st.segments[:BOUNCES]]
            traced = (sum(seg) if mdl is not None else sum(seg[1:]) + W * H) + int(st.shadow_rays)
            assert int(st.stalled_waves) == 0
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
            lines.append(f"{name:18s}: {samples / ms / 1e6:7.2f} Gsamples/s, {traced / ms / 1e6:7.2f} G traced segments/s "
                         f"({ms:.3f} ms per call of {FRAMES} frames, {traced / samples:.3f} traced segments per sample, "
                         f"specialized {int(st.specialized)}, {int(st.persistent_launches)} launches)")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
