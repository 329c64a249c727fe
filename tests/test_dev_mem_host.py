"""The owner of a context's device allocations (csrc/spt_dev_mem.h DevBuf), on the host: no GPU.

tests/cpp/test_dev_mem.cpp instantiates it over malloc / free with a count of live blocks and a request that can be
told to fail, and checks alloc, ensure (an equal size kept, any other replaced), the at-least form, that a failed
alloc or ensure leaves the buffer empty with the old block freed, that an element count whose bytes overflow size_t
fails without a request, that moves and swaps neither leak nor free twice, that a record of several buffers assigned
{} frees each once, and that nothing is alive at the end. It is compiled here with g++ and run, then once more under
the address and undefined-behaviour sanitizers: a stand-alone host program, run directly.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "software-path-tracer_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "test_dev_mem.cpp")


@pytest.mark.parametrize("name,flags", [
    ("plain", ["-O1"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_dev_mem(tmp_path, name, flags):
    exe = tmp_path / f"test_dev_mem_{name}"
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe), SRC], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dev mem ok" in r.stdout


def test_header_needs_no_hip():
    # the owner itself needs no HIP header: it compiles without the ROCm include path
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, "-x", "c++", "-"],
                   input='#include "spt_dev_mem.h"\nstruct A { static void* alloc(size_t) { return nullptr; } '
                         'static void free(void*) {} };\nspt::DevBuf<float, A> b;\nbool ok = b.ensure(4);\n',
                   text=True, check=True)
