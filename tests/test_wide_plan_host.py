"""The wide form's plans and bounds (spt_launch_plan.h make_view_plan / make_view_split / wide_call), on the host: no GPU.

tests/cpp/test_wide_plan.cpp is compiled here with g++ (the plan header is pure host code; the HIP headers it
includes for the vector types come from the ROCm install) and run: the default arguments give the plans of
before with Cornell 1080p's numbers, a wide plan's tiers cover every live record exactly once, no chunk or
sweep unit straddles the split's cut (empty and tiny halves too), the live-rank division is exact for every
n <= 64 and s <= 2^16, and the 512-frame cap keeps the ring's lap byte within a byte.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_plan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_wide_plan.cpp")
    exe = tmp_path / "test_wide_plan"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(ROOT, "software-path-tracer_amd", "csrc"), "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wide plan ok" in r.stdout
