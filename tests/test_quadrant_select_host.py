"""The new direction's quadrant applied after its products (spt_device.h bounce_dir_xy's kLateQuadrant form), on
the host: no GPU.

tests/cpp/test_quadrant_select.cpp is compiled here with hipcc (the __host__ side of spt_device.h, as
tests/cpp/test_sincos is built) and run: for phi at both ends of [0, 2 pi_f], around every multiple of pi / 2 and
over 2^20 stratified draws, and sin_t from 0 to 1, the form that swaps and signs the two converted floats gives
the same x and y words as the form that selects sin and cos as doubles, signed zeros included, with every
quadrant reached.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quadrant_select(tmp_path):
    csrc = os.path.join(ROOT, "software-path-tracer_amd", "csrc")
    exe = tmp_path / "test_quadrant_select"
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "--offload-arch=gfx950", "-I", csrc,
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "test_quadrant_select.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches: 0" in r.stdout and "PASS" in r.stdout
