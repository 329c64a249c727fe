"""The split of a view's lists into two halves (spt_launch_plan.h make_view_split), on the host: no GPU.

tests/cpp/test_split_plan.cpp is compiled here with g++ (the plan header is pure host code; the HIP headers it
includes for the vector types come from the ROCm install) and run: the two halves cover the live and the
constant list exactly once, the cuts are chunk- and sweep-aligned, each half's plan keeps the unsplit plan's
first-tier chunk size, the order keys of half A, half B and the unsplit plan differ pairwise, and Cornell
1080p's numbers are pinned.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_plan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_split_plan.cpp")
    exe = tmp_path / "test_split_plan"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(ROOT, "software-path-tracer_amd", "csrc"), "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "split plan ok" in r.stdout
