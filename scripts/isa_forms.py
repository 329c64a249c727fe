#!/usr/bin/env python3
"""gfx950 assembly of chosen shape-specialized k_paths / k_frame instantiations, for scripts/isa_hash.py.

    python3 scripts/isa_forms.py OUT.s --key KEY [--csrc DIR] [--name-key KEY2] [--all] FORM ...

FORM is `paths:<stats>,<env>,<chan>,<nee>,<wide>` or `frame:<env>,<nee>,<rgba>` (0 / 1 / 2 as in
spt_launch_plan.h's variants; the arguments a flat scene's run-time compile never sets stay false). KEY is
the kernels' shape key (spt_kernels.h flat_shape_key with jit_config_key's bits; scripts/static_profile.py
spells Cornell's). --csrc: the source tree to compile (default: this checkout's), e.g. another commit's
csrc directory. --name-key: write KEY2 for KEY in the symbol names of OUT.s, so that kernels compiled for
two keys that should give the same code can be compared by name. --all: also every kernel of the offline
build (spt_kernels.hip as the library compiles it).

The compile flags are the Makefile's HIPFLAGS, which spt_jit.hip passes to hiprtc too.
"""
import argparse
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def form_expr(form, key):
    kind, args = form.split(":")
    a = [int(x) for x in args.split(",")]
    b = lambda x: "true" if x else "false"  # noqa: E731
    if kind == "paths":
        stats, env, chan, nee, wide = a
        return f"spt::k_paths<{b(stats)}, false, {env}, {key}ull, 0, {b(chan)}, {nee}, false, false, {b(wide)}>"
    env, nee, rgba = a
    return f"spt::k_frame<false, false, {env}, {key}ull, false, {nee}, {b(rgba)}, false>"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--key", type=int, required=True)
    ap.add_argument("--csrc", default=os.path.join(ROOT, "software-path-tracer_amd", "csrc"))
    ap.add_argument("--name-key", type=int)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("forms", nargs="*")
    args = ap.parse_intermixed_args()
    uses = "\n".join(f"    (void*)&{form_expr(f, args.key)}," for f in args.forms)
    text = '#include "spt_kernels.hip"\nvoid* spt_isa_forms[] = {\n' + uses + "\n    nullptr};\n"
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "forms.hip")
        open(src, "w").write(text)
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-fno-slp-vectorize", "-ffp-contract=off", "-fno-fast-math", "-std=c++17",
               "--offload-arch=gfx950", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"), "-I" + args.csrc,
               "--cuda-device-only", "-S", "-o", args.out, src]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    s = open(args.out).read()
    if not args.all:  # keep the specialized kernels only: the ones whose name carries the key
        keep, on = [], False
        for line in s.split("\n"):
            if line.startswith("_Z") and ":" in line.split(";")[0]:
                on = f"Lm{args.key}E" in line
            if on:
                keep.append(line)
            if line.startswith(".Lfunc_end"):
                on = False
        s = "\n".join(keep) + "\n"
    if args.name_key is not None:
        s = s.replace(f"Lm{args.key}E", f"Lm{args.name_key}E")
    open(args.out, "w").write(s)


if __name__ == "__main__":
    main()
