"""The closest-hit keys' minimum (spt_device.h key_min), the CPU build's branch: no GPU.

tests/cpp/test_key_min_host.cpp is compiled here with hipcc (the __host__ side of spt_device.h, as
tests/cpp/test_sincos is built) and run over the pairs tests/cpp/test_key_min.hip runs on the device: every
ordered pair of the 54 keys made from the edge words (denormal doubles' high words, kTNear and its neighbours, 1.0f,
the largest finite float, +inf; indices 0, 1, 31, either side of the top bit, kMiss) and 2^22 random pairs. The
helper gives the keys' minimum word by word, and the keys read as doubles are positive, finite and ordered as the
integers are: what the device's one v_min_f64 rests on.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_min_host_branch(tmp_path):
    csrc = os.path.join(ROOT, "software-path-tracer_amd", "csrc")
    exe = tmp_path / "test_key_min_host"
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "--offload-arch=gfx950", "-I", csrc,
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "test_key_min_host.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2916 set pairs (54 keys), 4194304 random pairs" in r.stdout
    assert "mismatches: 0;" in r.stdout and "doubles: 0;" in r.stdout and "order otherwise: 0;" in r.stdout
    assert "PASS" in r.stdout
