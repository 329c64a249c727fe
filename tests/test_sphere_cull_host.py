"""tests/cpp/test_sphere_cull --host (no kernel runs): its inputs reach every case the GPU check is aimed at."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sphere_cull_inputs_reach_their_cases(spt):
    exe = os.path.join(ROOT, "tests", "cpp", "test_sphere_cull")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/test_sphere_cull"], check=True)
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout and "not reached" not in r.stdout, r.stdout + r.stderr


def test_stats_struct_has_the_sphere_count(spt):
    """spt_stats.flat_sphere_second_passes is the struct's last field, behind view_split (the ABI only grows)."""
    names = [n for n, _ in spt.SptStats._fields_]
    assert names[-2:] == ["view_split", "flat_sphere_second_passes"]
