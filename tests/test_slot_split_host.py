"""k_paths' slot split by shift and mask (spt_kernels.h slot_split_shift), on the host: no GPU.

tests/cpp/test_slot_split.cpp is compiled here with g++ (the header is host code too; the HIP headers it includes for
the vector types come from the ROCm install) and run: for px = 16, 32, 64 and every slot q < 2^16 the shift form
gives the frame and the live rank of the kernel's high multiply, (div_live(q), q - f * px), which are q / px and
q % px; for a partial chunk (n_live < px) the two differ, so the kernel's n_live == px test selects the form.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_split(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_slot_split.cpp")
    exe = tmp_path / "test_slot_split"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(ROOT, "software-path-tracer_amd", "csrc"), "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "slot split ok: 196608 slots" in r.stdout
