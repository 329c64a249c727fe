"""The opposite wall pairs of a flat scene (scene.cpp flat_wall_pairs) and their bits in the shape key
(spt_kernels.h flat_shape_key), on the host: no GPU.

tests/cpp/test_wall_pairs.cpp is compiled here with g++ together with the scene preparation it checks
(scene.cpp, scenes.cpp: pure host code; the HIP headers spt_kernels.h includes for the vector types come
from the ROCm install) and run: Cornell has one pair on x and one on y with the light unpaired and none
on z; four quads on one axis give two nested pairs; coplanar quads are never paired; a group that is
not all rectangles has none; every record is kept exactly once with the lower plane first in each pair;
the key round-trips.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wall_pairs(tmp_path):
    csrc = os.path.join(ROOT, "software-path-tracer_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "cpp", "test_wall_pairs.cpp"), os.path.join(csrc, "scene.cpp"),
           os.path.join(csrc, "scenes.cpp")]
    exe = tmp_path / "test_wall_pairs"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    "-o", str(exe), *src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wall pairs ok" in r.stdout
