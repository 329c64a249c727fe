"""tests/cpp/test_sphere_cull on the GPU: spt_device.h flat_sphere_pass against the loop over isect_sphere_fast."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sphere_cull_and_one_pass_selection(spt):
    """2^24 (ray, three spheres) inputs: a sphere with b > 0 && c > 0 returns kInf, and the one-pass selection
    with the second-pass rule returns the per-sphere loop's (t bits, index) and `redo`, for three and two spheres."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_sphere_cull")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/test_sphere_cull"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "culled spheres that returned a hit 0;" in r.stdout
    assert "key mismatches 0 (3 spheres) 0 (2 spheres); redo mismatches 0;" in r.stdout
