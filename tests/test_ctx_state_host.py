"""What each change to a context drops of its cached results (spt_ctx_state.h DerivedState), on the host: no GPU.

tests/cpp/test_ctx_state.cpp is compiled here with g++ (the record is pure host code; frame_hit_mode comes
from the plan header, whose vector types are the ROCm install's) and run: for every cause the dropped items
are the matrix written out in the test, from every item valid and from each item alone; a drop applied twice
changes nothing more; the compacted lists are never seen without the camera hits; a view-list build zeroes the
halves' chunk-order keys only.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctx_state(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_ctx_state.cpp")
    exe = tmp_path / "test_ctx_state"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(ROOT, "software-path-tracer_amd", "csrc"), "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ctx state ok" in r.stdout
    # the record itself needs no HIP header: it compiles without the ROCm include path
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "software-path-tracer_amd", "csrc"),
                    "-x", "c++", "-"], input='#include "spt_ctx_state.h"\nspt::DerivedState s;\n', text=True, check=True)
