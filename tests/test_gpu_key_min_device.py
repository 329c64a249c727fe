"""tests/cpp/test_key_min on the GPU: spt_device.h key_min (one v_min_f64) against the integer minimum of two keys."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_min_is_the_integer_minimum(spt):
    """Every ordered pair of the 54 edge keys (high words from the smallest denormal double's to +inf's, kTNear and
    its two neighbours among them; low words 0, 1, 31, 0x7fffffff, 0x80000000, 0xffffffff; equal high words and
    equal keys included) and 2^22 random pairs with high words in [bits(kTNear), 0x7f800000], in both operand
    orders: 0 mismatches."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_key_min")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/test_key_min"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "2916 set pairs (54 keys), 4194304 random pairs" in r.stdout
    assert "mismatches 0 (set) 0 (random);" in r.stdout
