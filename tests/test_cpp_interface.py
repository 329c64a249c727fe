"""The C++ render::PathTracer backend (libspt_render.so) driven the way the reference App drives
its backend (tests/cpp/test_pathtracer.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_pathtracer")


@pytest.fixture(scope="module")
def exe(spt):
    subprocess.run(["make", "-s", "-C", ROOT, "cpp-tests"], check=True)
    return EXE


def test_cpp_interface_cpu(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout


@pytest.mark.gpu
def test_cpp_app_scene_on_gpu(exe):
    r = subprocess.run([exe, "gpu", "256", "192", "8"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_resized_window_on_gpu(exe):
    """The App's window resized between frames: the backend reallocates and re-registers its
    RenderResult buffer (the resolve kernel stores into it directly); every size matches the oracle."""
    r = subprocess.run([exe, "resize"], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout


@pytest.mark.gpu
def test_cpp_changed_scene_on_gpu(exe):
    """SURVEY.md 8f row 2 through the C++ backend: a changed scene (one sphere added, one moved) handed
    over after 5 frames restarts the accumulation and renders the new geometry, vs the oracle."""
    r = subprocess.run([exe, "rescene", "192", "128"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("args", [
    ("160", "96", "3", "5", "6", "1", "1.7", "1"),   # progressive: 15 frames, k_paths calls of 5
    ("96", "64", "2", "2", "8", "3", "0.5", "0"),    # not progressive: every call frames 0..1 (k_frame)
    ("128", "80", "4", "1", "6", "2", "1.3", "1"),   # one frame per call: the resolve fused into k_frame
])
def test_cpp_settings_mode_on_gpu(exe, args):
    """HIPPathTracer::set_settings_mode(true): RenderSettings bounces / RR / spp / progressive /
    exposure honoured, vs the oracle; then back to reference mode."""
    r = subprocess.run([exe, "settings", *args], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


def test_bvh_quantized_nodes_contain_fp32_boxes(exe):
    """The device's 64-B quantized BVH nodes decode exactly and contain every fp32 child box they
    came from (C4, C5 and App scenes; scene.h BvhNodeQ) — so traversal finds the same hits."""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_bvh")], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


def test_stack_entry_code_is_a_lower_bound(exe):
    """The 4-B traversal stack entry (spt_kernels.h, SPT_BVH_STACK_ENTRY 4): for every code width the
    decoded entry distance never exceeds t0 (the pop's cull stays conservative: exact closest hits) and
    the child ref above the code survives."""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_stack_code")], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


def test_launch_plan_picks_the_kernels_and_grids(exe):
    """spt_launch_plan.h on the host: k_paths' chunk plan (tiling invariants over a sweep, exact tiers of
    the benchmark shapes), the k_paths / k_frame variant and run-time compiled kind each kind of scene
    runs, k_frame's grid rule, and the run-time compiled forms' name expressions (jit_name_expr). Every
    variant gives the same image, so no parity test sees a wrong choice."""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_launch_plan")], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


def test_device_sincos_matches_glibc(exe):
    """spt_device.h sincos_2pi (host build) vs glibc cos/sin on 2e7 reference-RNG draws: the float
    products the integrator uses must be identical."""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_sincos"), "20000000"], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_device_sqrt_unit_exhaustive(exe):
    """spt_device.h on the GPU: sqrt_unit == sqrtf on 0 and [2^-96, 2^96), inv_sqrt_ref == 1/sqrtf on all
    2^32 inputs, div_ref == n / s for every divisor in [2^-40, 2^20) (the flat loop's fast-path ranges)."""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_device_math")], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


DEVICE_RAYS = os.path.join(ROOT, "tests", "cpp", "test_device_rays")


def test_device_ray_inputs_reach_their_branches(exe):
    """tests/cpp/test_device_rays --host (no kernel runs): the inputs it aims at spt_device.h's branch points
    reach them — every coverage counter is non-zero, among them a `redo` lane, a disc = 0 lane and an
    alpha = -0 lane — and the host builds of the camera, bounce, BSDF step and octa_texel match the oracle."""
    r = subprocess.run([DEVICE_RAYS, "--host"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "host only" in r.stdout
    for counter in ("redo=", "disc=0=", "alpha=-0="):
        assert counter in r.stdout and counter + "0 " not in r.stdout, counter


@pytest.mark.gpu
def test_device_ray_steps_match_the_oracle(exe):
    """spt_device.h on the GPU, function by function, bit for bit against the oracle's plain C: the camera's
    fast path on both sides of every term of its gate, the intersectors' general and fast forms with the
    `redo` protocol, sincos_2pi / bounce_dir, bsdf_scatter, light_sample and octa_texel.
    (The oracle side takes about 2 s single-threaded on a slow core, under 1 s beside an MI355X, where the
    whole run took 1.2 s: timeout 120 s.)"""
    r = subprocess.run([DEVICE_RAYS], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout and "first:" not in r.stdout


REF_INCLUDE = "/root/reference/libs/render/include"
CSRC = os.path.join(ROOT, "software-path-tracer_amd", "csrc")
COMPAT = os.path.join(ROOT, "tests", "compat")  # glm declarations for the compile check only


def _syntax(src, includes):
    cmd = ["g++", "-std=c++20", "-fsyntax-only", "-Wall"] + [f"-I{d}" for d in includes] + [src]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.isdir(REF_INCLUDE), reason="reference checkout absent (GPU box)")
@pytest.mark.parametrize("src", ["HIPPathTracer.cpp", "PathTracer.cpp", "../../tests/cpp/app_handoff.cpp"])
def test_backend_compiles_against_reference_headers(src, tmp_path):
    """Drop-in check: the GPU_HIP backend and the App's scene-building / hand-off
    calls (App.cpp:98-133, 230-240) compile against the reference's OWN Scene.h / Types.h
    (glm::vec3 positions, unordered_map registry), with only the GPU_HIP enumerator added to
    PathTracer.h (this repo's include/render/PathTracer.h overlays it). glm comes from a
    declarations-only shim (tests/compat/glm): syntax check, nothing is linked or run."""
    overlay = tmp_path / "render"
    overlay.mkdir()
    (overlay / "PathTracer.h").write_text(open(os.path.join(ROOT, "include", "render", "PathTracer.h")).read())
    r = _syntax(os.path.normpath(os.path.join(CSRC, src)),
                [str(tmp_path), REF_INCLUDE, COMPAT, os.path.join(ROOT, "include"), CSRC])
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(not os.path.isdir(REF_INCLUDE), reason="reference checkout absent (GPU box)")
def test_reference_pathtracer_h_needs_only_the_gpu_hip_enumerator():
    """Against the reference's unmodified PathTracer.h the backend fails on GPU_HIP alone: the one
    line INTEGRATION.md §1 adds is the whole header change."""
    r = _syntax(os.path.join(CSRC, "HIPPathTracer.cpp"), [REF_INCLUDE, COMPAT, os.path.join(ROOT, "include"), CSRC])
    assert r.returncode != 0
    errors = [ln for ln in r.stderr.splitlines() if "error:" in ln]
    assert errors and all("GPU_HIP" in ln for ln in errors), r.stderr


def test_app_handoff_compiles_against_own_headers_with_glm():
    """With glm on the include path this repo's render/Scene.h takes glm::vec3 positions, so the
    App's own SetPosition(glm::vec3(...)) calls compile against it unchanged."""
    r = _syntax(os.path.join(ROOT, "tests", "cpp", "app_handoff.cpp"), [os.path.join(ROOT, "include"), COMPAT, CSRC])
    assert r.returncode == 0, r.stderr
