"""Static instruction profile of one k_paths instantiation between the SPT_MARK comments of a
-DSPT_STATIC_PROFILE build (analysis only: the markers constrain scheduling a little).

    python scripts/static_profile.py [--no-pairs] [--wide] [--ranges] [extra hipcc -D flags ...]

--wide: the C2 kernel's wide form (64-pixel chunks over a view's lists, the benchmark's) instead of the plain one.
--ranges: with the scene's range bit in the key (spt_kernels.h kShapeRanges): the step loop's guard-free forms.

Compiles the C2 shape-specialized flat kernel and the two BVH k_paths instantiations to assembly and
prints, per section of the step loop, the VALU / SALU / LDS / scalar-memory / vector-memory
instruction counts (the code the compiler placed after a marker, up to the next one in program
order; the sections of divergent branches interleave, so read the counts as the code size of each
part, not as executed instructions). Of the VALU count it also gives the fp64 instructions (any *_f64 operand
or result, the conversions included), the fp32 transcendentals (v_rcp / v_rsq / v_sqrt / v_exp / v_log / v_sin /
v_cos) and the integer instructions measured above one issue slot (`int`: the 32-bit and 24-bit multiplies and
multiply-adds, v_lshl_add_u32 / _u64, v_mad_u64_u32), and an issue-weighted total `wt`: each instruction at its
measured cost in multiples of v_fma_f32's at 7 waves per SIMD (ISSUE_WEIGHTS below; scripts/valu_issue_cost.py,
profiles/valu_issue_costs.txt), every other instruction at 1."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2_SHAPE = 77445755138  # flat_shape_key of the Cornell box (spt_kernels.h)
# ... with C2's launch configuration baked in (jit_config_key: 8 bounces, RR depth 2, sky, fast division)
C2_SHAPE |= (1 << 37) | (8 << 38) | (2 << 44) | (1 << 50) | (1 << 52)
C2_SHAPE |= 7 << 53  # every axis group of the box is walls (flat_rect_bits)
if "--no-pairs" in sys.argv:  # the same kernel with every wall tested (the key before flat_wall_pairs)
    sys.argv.remove("--no-pairs")
else:
    C2_SHAPE |= (1 | 1 << 2) << 57  # one opposite pair on x, one on y (flat_wall_pairs)
WIDE = "--wide" in sys.argv
if WIDE:
    sys.argv.remove("--wide")
if "--ranges" in sys.argv:
    sys.argv.remove("--ranges")
    C2_SHAPE |= 1 << 63
INST = r"""#include "spt_kernels.hip"
namespace spt {
#define I(S, B, SH, W, WIDE) template __global__ void k_paths<S, B, 0, SH, W, false, 0, false, false, WIDE>(const float4* __restrict__, const float4* __restrict__, \
    const float4* __restrict__, uint32_t, float4* __restrict__, unsigned long long* __restrict__, uint32_t* __restrict__, \
    uint32_t* __restrict__, ShadeParams, CameraParams, uint32_t, ChunkPlan, NeeParams, ViewPlan);
I(false, false, %dull, 0, %s)
}
""" % (C2_SHAPE, "true" if WIDE else "false")


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


TRANS = ("v_rcp_", "v_rsq_", "v_sqrt_", "v_exp_", "v_log_", "v_sin_", "v_cos_")
# the integer instructions measured at 1.5 issue slots (v_mad_u64_u32: 1.85, its own entry below)
INT15 = ("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u32_u24", "v_mul_u32_u24", "v_lshl_add_u64", "v_lshl_add_u32")
# Issue cost by kind, in multiples of v_fma_f32's at 7 waves per SIMD on every CU (profiles/valu_issue_costs.txt,
# rounded): v_fma_f64 1.52 and v_min_f64 1.50 stand for every *_f64; v_rcp_f32 2.97 and v_sqrt_f32 2.97 for the
# fp32 transcendentals; the six of INT15 1.49-1.52; v_mad_u64_u32 1.84. v_add_f32, v_mul_f32 and v_add_u32 measured
# 1.00, 0.96 and 1.04: the unit holds for the plain instructions.
ISSUE_WEIGHTS = {"f64": 1.5, "trans": 3.0, "int": 1.5, "mad64": 1.85}


def valu_kind(op):
    """'f64', 'trans', 'int', 'mad64' or None (a plain VALU instruction); an fp64 transcendental counts as fp64."""
    if "_f64" in op:
        return "f64"
    if op.startswith(TRANS):
        return "trans"
    if op.startswith("v_mad_u64_u32"):
        return "mad64"
    if op.startswith(INT15):
        return "int"
    return None


def weighted(c):
    """The issue-weighted VALU count of a section's counter."""
    return c["valu"] + sum((w - 1.0) * c[k] for k, w in ISSUE_WEIGHTS.items())


def main():
    flags = sys.argv[1:]
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "inst.hip")
        open(src, "w").write(INST)
        asm = os.path.join(td, "inst.s")
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-fno-slp-vectorize", "-ffp-contract=off", "-fno-fast-math",
               "-std=c++17", "--offload-arch=gfx950", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"),
               "-I" + os.path.join(ROOT, "software-path-tracer_amd", "csrc"), "--cuda-device-only", "-S",
               "-DSPT_STATIC_PROFILE", *flags, "-o", asm, src]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        lines = open(asm).read().split("\n")
    for kname in ("_ZN3spt7k_pathsILb0ELb0ELi0ELm%dELi0ELb0ELi0ELb0ELb0ELb%dE" % (C2_SHAPE, WIDE), "_ZN3spt7k_pathsILb0ELb1ELi0ELm0ELi8E",
                  "_ZN3spt7k_pathsILb0ELb1ELi0ELm0ELi0E"):
        on, sec = False, "prologue"
        cnt = collections.defaultdict(collections.Counter)
        for ln in lines:
            if re.match(r"^" + kname + r".*:", ln):
                on = True
                continue
            if not on:
                continue
            if ln.startswith(".Lfunc_end"):
                break
            m = re.search(r"SPT_MARK (\w+)", ln)
            if m:
                sec = m.group(1)
                continue
            s = ln.strip()
            if not s or s.startswith((";", ".")) or s.endswith(":"):
                continue
            cnt[sec][classify(s.split()[0])] += 1
            if classify(s.split()[0]) == "valu" and valu_kind(s.split()[0]):
                cnt[sec][valu_kind(s.split()[0])] += 1
        if not cnt:
            continue
        print(kname)
        tot = sum(c["valu"] for c in cnt.values())
        for sec, c in cnt.items():
            print(f"  {sec:26s} valu {c['valu']:5d} ({100.0 * c['valu'] / max(tot, 1):4.1f} %)  salu {c['salu']:4d}  "
                  f"lds {c['lds']:3d}  smem {c['smem']:3d}  vmem {c['vmem']:3d}  wait {c['wait']:3d}  "
                  f"f64 {c['f64']:3d}  trans {c['trans']:3d}  int {c['int'] + c['mad64']:3d}  wt {weighted(c):7.1f}")
        loop = [c for sec, c in cnt.items() if sec != "prologue"]
        v, f, t, i = (sum(c[k] for c in loop) for k in ("valu", "f64", "trans", "int"))
        i += sum(c["mad64"] for c in loop)
        wt = sum(weighted(c) for c in loop)
        print(f"  {'step loop (no prologue)':26s} valu {v:5d}  f64 {f:3d}  trans {t:3d}  int {i:3d}  wt {wt:7.1f} ({wt / max(v, 1):.3f} x)")


if __name__ == "__main__":
    main()
