"""Stand-alone host programs under the sanitizers: csrc/spt_host.cpp (the library's host-only entry points, plain
C++) with one tests/cpp/*.cpp that has a main, built by g++ with AddressSanitizer and UndefinedBehaviorSanitizer.
Nothing of HIP's is linked, so the leak checker runs too; nothing sanitized is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "software-path-tracer_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "include")


def build(name, out_dir, with_host=True):
    """Build tests/cpp/<name>.cpp into out_dir/<name> and return its path; with_host=False for a program that
    includes a csrc header alone and calls nothing of spt_host.cpp's."""
    exe = os.path.join(str(out_dir), name)
    sources = [os.path.join(ROOT, "tests", "cpp", name + ".cpp")] + ([os.path.join(CSRC, "spt_host.cpp")] if with_host else [])
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", ROCM_INCLUDE,
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", exe] + sources, check=True)
    return exe
