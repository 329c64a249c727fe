"""The camera (spt_set_camera: pose, field of view, per-sample jitter) on the GPU, bit for bit.

The expected image is composed here from the oracle's pieces, per pixel and frame in frame order: the
seed (ref_rng_seed), for a jittered camera the path's first two draws (ref_random_float), the ray from
spt.camera_ray (the host build of the function the kernels compile), ref_trace_ray from that ray and RNG
state, and float32 adds into RGBA. Case 1 ties the posed path to ref.render itself, independently of
this restatement. Sizes: 37x23 (odd: a partial last chunk, no zero direction component) and 48x32 (full
32-pixel chunks).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNCES, RR = 5, 2
SIZES = [(37, 23), (48, 32)]
EYE, TARGET, VFOV = (1.5, 0.75, -2.0), (0.0, -1.0, 5.0), 55.0
N_POSED, N_JITTER = 8, 15  # frames composed per case: 3 one-frame calls + a 5/6-frame call; first_frame 3 + 12

_scenes = {}
_frames = {}


def scene_of(spt, ref, name, env_map=False):
    """(prims, mats, env, RefScene, env map or None), built once per scene."""
    key = (name, env_map)
    if key not in _scenes:
        prims, mats, env = spt.build_scene(name)
        rs = ref.RefScene(prims, mats, env)
        em = spt.synthetic_env_map(64) if env_map else None
        if em is not None:
            rs.set_env_map(em)
        _scenes[key] = (prims, mats, env, rs, em)
    return _scenes[key]


def generic_camera(spt, jitter=False):
    return spt.look_at(EYE, TARGET, vfov=VFOV, jitter=jitter)


def sky_camera(spt, jitter=False):
    """Looks away from the Cornell box (z in [3, 8]): every pixel is sky."""
    return spt.look_at((0.5, 0.25, 0.0), (-0.75, 1.0, -4.0), vfov=70.0, jitter=jitter)


def frame_radiance(spt, ref, scene, w, h, cam, flags, n_frames, env_map=False, tag=""):
    """[n_frames, h, w, 4] float32: trace_ray's (L, 1) of every pixel of frames 0 .. n_frames - 1 through
    `cam` (its jitter flag included), composed from the oracle's pieces. Cached: read only."""
    key = (scene, w, h, tag, int(cam.flags), flags, n_frames, env_map)
    if key in _frames:
        return _frames[key]
    rs = scene_of(spt, ref, scene, env_map)[3]
    lib = ref.load()
    slib = spt.load_library()
    cfg = ref.RefConfig(w, h, BOUNCES, RR, flags)
    f3 = ctypes.c_float * 3
    o, d, out = f3(), f3(), (ctypes.c_float * 4)()
    state = ctypes.c_uint32()
    jitter = bool(cam.flags & spt.CAMERA_JITTER)
    img = np.zeros((n_frames, h, w, 4), dtype=np.float32)
    for f in range(n_frames):
        for y in range(h):
            for x in range(w):
                state.value = lib.ref_rng_seed(x, y, w, f + 1)
                jx = jy = 0.0
                if jitter:
                    jx = lib.ref_random_float(ctypes.byref(state))
                    jy = lib.ref_random_float(ctypes.byref(state))
                assert slib.spt_camera_ray(ctypes.byref(cam), w, h, x, y, jx, jy, o, d) == 0
                lib.ref_trace_ray(rs.h, ctypes.byref(cfg), o, d, ctypes.byref(state), out)
                img[f, y, x] = out[:]
    img.setflags(write=False)
    _frames[key] = img
    return img


def accumulate(frames, first, n):
    """The accumulation buffer after frames [first, first + n), added in frame order in float32."""
    acc = np.zeros(frames.shape[1:], dtype=np.float32)
    for f in range(first, first + n):
        acc = acc + frames[f]
    return acc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def assert_same(got, want, what):
    g, r = bits(got), bits(want)
    bad = np.flatnonzero(np.any(g != r, axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} pixels differ, first {bad[:5]}"


def setup(spt, ref, ctx, scene, w, h, flags, cam, env_map=False, **cfg):
    prims, mats, env, _, em = scene_of(spt, ref, scene, env_map)
    ctx.set_scene(prims, mats, env)
    ctx.set_env_map(em)
    ctx.configure(w, h, BOUNCES, RR, flags, **cfg)
    ctx.set_camera(cam)


@pytest.fixture(scope="module")
def cam_ctx(spt):
    """One context for the camera tests (not the session's: a camera outlives spt_configure)."""
    ctx = spt.Context(0)
    yield ctx
    ctx.close()


# ---- 1. the identity camera is the camera of a ctx without one, and the untouched oracle's ---------
@pytest.mark.parametrize("scene", ["cornell", "app"])
def test_identity_camera_equals_no_camera(spt, ref, cam_ctx, scene):
    w, h, frames = 37, 23, 5
    ident = spt.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0), 90.0)
    want = scene_of(spt, ref, scene)[3].render(w, h, 0, frames, BOUNCES, RR, 0)
    for cam in (None, ident):
        setup(spt, ref, cam_ctx, scene, w, h, 0, cam)
        cam_ctx.render(0, frames)
        assert_same(cam_ctx.read_accum(), want, f"{scene} {'identity' if cam else 'no'} camera, k_paths")
        cam_ctx.reset()
        for f in range(frames):
            cam_ctx.render(f, 1)
        assert_same(cam_ctx.read_accum(), want, f"{scene} {'identity' if cam else 'no'} camera, k_frame")


# ---- 2. + 3. a generic camera, posed and jittered, on every schedule --------------------------------
def run_schedules(spt, ref, ctx, scene, w, h, nee, jitter, sorted_rays):
    flags = spt.FLAG_NEE if nee else 0
    cam = generic_camera(spt, jitter)
    n = N_JITTER if jitter else N_POSED
    frames = frame_radiance(spt, ref, scene, w, h, cam, flags, n, tag="generic")
    what = f"{scene} {w}x{h} nee={nee} jitter={jitter}"
    # three consecutive one-frame calls (k_frame; posed: the hit cache stored, read, listed; jittered: no
    # cache, so a stale one would show), then a call of many frames (k_paths; jittered: 12 frames, so the
    # 256-slot ring wraps with 32 live pixels)
    setup(spt, ref, ctx, scene, w, h, flags, cam)
    for f in range(3):
        ctx.render(f, 1)
        assert int(ctx.stats().schedule) == spt.SCHEDULE_FRAME
        assert_same(ctx.read_accum(), accumulate(frames, 0, f + 1), f"{what}: one-frame call {f}")
    long_n = 12 if jitter else 5
    ctx.render(3, long_n)  # (first_frame = 3)
    assert int(ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
    assert_same(ctx.read_accum(), accumulate(frames, 0, 3 + long_n), f"{what}: k_paths after the one-frame calls")
    ctx.reset()
    ctx.render(0, long_n + 1)
    assert int(ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
    assert_same(ctx.read_accum(), accumulate(frames, 0, long_n + 1), f"{what}: k_paths")
    # the statistics kernels are instantiations of their own
    ctx.set_profiling(False, counters=True)
    ctx.reset()
    ctx.render(0, 4)
    ctx.render(4, 1)
    assert_same(ctx.read_accum(), accumulate(frames, 0, 5), f"{what}: counting kernels")
    st = ctx.stats()
    assert int(st.stalled_waves) == 0
    ctx.set_profiling(False)
    wave = [spt.FLAG_WAVEFRONT, spt.FLAG_WAVEFRONT | spt.FLAG_SPLIT_KERNELS]
    if sorted_rays:
        wave.append(spt.FLAG_SORTED_RAYS)
    for fl in wave:
        setup(spt, ref, ctx, scene, w, h, flags | fl, cam)
        ctx.render(0, 2)
        ctx.render(2, 4)
        assert int(ctx.stats().schedule) in (spt.SCHEDULE_FUSED, spt.SCHEDULE_SPLIT)
        assert_same(ctx.read_accum(), accumulate(frames, 0, 6), f"{what}: wavefront flags {fl:#x}")
    assert int(ctx.stats().stalled_waves) == 0


@pytest.mark.parametrize("nee", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("scene", ["cornell", "app"])
def test_posed_camera_every_schedule(spt, ref, cam_ctx, scene, w, h, nee):
    run_schedules(spt, ref, cam_ctx, scene, w, h, nee, False, scene == "app")


@pytest.mark.parametrize("nee", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("scene", ["cornell", "app"])
def test_jittered_camera_every_schedule(spt, ref, cam_ctx, scene, w, h, nee):
    run_schedules(spt, ref, cam_ctx, scene, w, h, nee, True, scene == "app")


@pytest.mark.parametrize("jitter", [False, True])
def test_camera_triangles_under_a_bvh(spt, ref, cam_ctx, jitter):
    """bunnylike (81,920 triangles, NEE without sphere lights): k_frame and k_paths."""
    w, h, flags = 37, 23, spt.FLAG_NEE
    cam = generic_camera(spt, jitter)
    frames = frame_radiance(spt, ref, "bunnylike", w, h, cam, flags, 6, tag="generic")
    setup(spt, ref, cam_ctx, "bunnylike", w, h, flags, cam)
    cam_ctx.render(0, 1)
    cam_ctx.render(1, 1)
    assert_same(cam_ctx.read_accum(), accumulate(frames, 0, 2), f"bunnylike jitter={jitter}: k_frame")
    cam_ctx.render(2, 4)
    assert int(cam_ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
    assert_same(cam_ctx.read_accum(), accumulate(frames, 0, 6), f"bunnylike jitter={jitter}: k_paths")
    assert int(cam_ctx.stats().stalled_waves) == 0


def test_posed_camera_shape_specialized_kernels(spt, ref, cam_ctx):
    """A flat scene's kernels compiled for its shape at run time take the camera as the generic ones do (a
    kernel argument); a jittered camera runs the generic kernels."""
    scene, (w, h) = "cornell", SIZES[1]
    cam = generic_camera(spt)
    frames = frame_radiance(spt, ref, scene, w, h, cam, 0, N_POSED, tag="generic")
    setup(spt, ref, cam_ctx, scene, w, h, 0, cam)
    cam_ctx.specialize_scene()  # (waits for the shape's compiles)
    for f in range(3):
        cam_ctx.render(f, 1)
        assert int(cam_ctx.stats().specialized) == 1
    assert_same(cam_ctx.read_accum(), accumulate(frames, 0, 3), "specialized k_frame")
    cam_ctx.render(3, 5)
    assert int(cam_ctx.stats().specialized) == 1
    assert_same(cam_ctx.read_accum(), accumulate(frames, 0, 8), "specialized k_paths")
    cam_ctx.set_camera(generic_camera(spt, True))
    cam_ctx.render(0, 4)
    st = cam_ctx.stats()
    assert int(st.specialized) == 0 and int(st.schedule) == spt.SCHEDULE_PERSISTENT
    fj = frame_radiance(spt, ref, scene, w, h, generic_camera(spt, True), 0, N_JITTER, tag="generic")
    assert_same(cam_ctx.read_accum(), accumulate(fj, 0, 4), "jittered k_paths after specialize_scene")


# ---- 4. a camera change restarts the accumulation and drops what was cached for the old camera -----
def test_camera_change(spt, ref, cam_ctx):
    scene, (w, h) = "cornell", SIZES[0]
    cam_a = spt.look_at((-1.0, 0.5, -1.0), (0.5, -1.0, 5.0), vfov=70.0)
    cam_b = generic_camera(spt)
    cam_bj = generic_camera(spt, True)
    fb = frame_radiance(spt, ref, scene, w, h, cam_b, 0, N_POSED, tag="generic")
    fbj = frame_radiance(spt, ref, scene, w, h, cam_bj, 0, N_JITTER, tag="generic")
    no_cam = scene_of(spt, ref, scene)[3].render(w, h, 0, 7, BOUNCES, RR, 0)

    def check(want_frames, what):
        assert cam_ctx.frame_count == 0, what
        cam_ctx.render(0, 1)
        cam_ctx.render(1, 1)
        got2 = cam_ctx.read_accum()
        cam_ctx.render(2, 5)
        got7 = cam_ctx.read_accum()
        if want_frames is None:
            assert_same(got7, no_cam, what)
        else:
            assert_same(got2, accumulate(want_frames, 0, 2), what + ": one-frame calls")
            assert_same(got7, accumulate(want_frames, 0, 7), what + ": then 5 frames")
        return got7

    setup(spt, ref, cam_ctx, scene, w, h, 0, cam_a)
    cam_ctx.render(0, 1)
    cam_ctx.render(1, 1)  # (camera A's hits are cached and listed now)
    assert cam_ctx.frame_count == 2
    cam_ctx.set_camera(cam_b)
    got_b = check(fb, "A -> B")
    with spt.Context(0) as fresh:
        setup(spt, ref, fresh, scene, w, h, 0, cam_b)
        fresh.render(0, 1)
        fresh.render(1, 1)
        fresh.render(2, 5)
        assert_same(got_b, fresh.read_accum(), "A -> B against a fresh context with B")
    cam_ctx.set_camera(cam_bj)
    check(fbj, "jitter on")
    cam_ctx.set_camera(cam_b)
    check(fb, "jitter off again")
    cam_ctx.set_camera(None)
    check(None, "no camera again")
    # kept across spt_configure
    cam_ctx.set_camera(cam_b)
    cam_ctx.configure(w, h, BOUNCES, RR, 0)
    check(fb, "B across a reconfigure")


# ---- 5. every pixel sky: the constant-pixel chunks with rotated directions --------------------------
@pytest.mark.parametrize("env_map", [False, True])
@pytest.mark.parametrize("jitter", [False, True])
def test_all_sky_view(spt, ref, cam_ctx, jitter, env_map):
    scene, (w, h) = "cornell", SIZES[1]
    cam = sky_camera(spt, jitter)
    n = 13
    frames = frame_radiance(spt, ref, scene, w, h, cam, 0, n, env_map=env_map, tag="sky")
    rs = scene_of(spt, ref, scene, env_map)[3]
    for y in range(h + 1):  # every pixel's footprint [x, x + 1] x [y, y + 1] misses the scene: its corners do
        for x in range(w + 1):
            assert rs.intersect(*spt.camera_ray(cam, w, h, x, y)) is None, (x, y)
    setup(spt, ref, cam_ctx, scene, w, h, 0, cam, env_map=env_map)
    for f in range(3):
        cam_ctx.render(f, 1)
    assert_same(cam_ctx.read_accum(), accumulate(frames, 0, 3), f"sky jitter={jitter} env={env_map}: k_frame")
    cam_ctx.render(3, 10)
    assert_same(cam_ctx.read_accum(), accumulate(frames, 0, n), f"sky jitter={jitter} env={env_map}: k_paths")
    if not jitter:  # a miss takes no draw: without jitter its paths end at the camera segment
        assert_same(accumulate(frames, 0, 1), accumulate(frames, 1, 1), "sky pixels are constant")
    cam_ctx.set_env_map(None)


# ---- 6. row shards -----------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True])
def test_camera_row_shard(spt, ref, cam_ctx, jitter):
    scene, (w, h) = "cornell", SIZES[0]
    cam = generic_camera(spt, jitter)
    n = N_JITTER if jitter else N_POSED
    frames = frame_radiance(spt, ref, scene, w, h, cam, 0, n, tag="generic")
    setup(spt, ref, cam_ctx, scene, w, h, 0, cam, shard_rank=1, shard_count=3)
    cam_ctx.render(0, 1)
    cam_ctx.render(1, 1)
    assert_same(cam_ctx.read_accum(), accumulate(frames, 0, 2)[1::3], f"shard jitter={jitter}: k_frame")
    cam_ctx.render(2, 6)
    assert_same(cam_ctx.read_accum(), accumulate(frames, 0, 8)[1::3], f"shard jitter={jitter}: k_paths")


# ---- 7. the fused hand-off --------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True])
def test_camera_fused_resolve(spt, ref, jitter):
    scene, (w, h) = "cornell", SIZES[1]
    cam = generic_camera(spt, jitter)
    frames = frame_radiance(spt, ref, scene, w, h, cam, 0, N_JITTER if jitter else N_POSED, tag="generic")
    with spt.Context(0) as plain, spt.Context(0) as fused:
        for c in (plain, fused):
            setup(spt, ref, c, scene, w, h, 0, cam)
        buf = np.zeros(fused.shard_pixels, dtype=np.uint32)
        fused.register_host_output(buf)
        frame = 0
        for n in (1, 1, 1, 2):
            plain.render(frame, n)
            want = plain.resolve_rgba8(frame + n)
            buf[:] = 0xdeadbeef
            fused.render_resolve_rgba8(frame, n, frame + n, out=buf)
            frame += n
            np.testing.assert_array_equal(buf, want, err_msg=f"jitter={jitter} after {frame} frames")
            np.testing.assert_array_equal(buf, ref.resolve_rgba8(accumulate(frames, 0, frame), frame))
        assert_same(fused.read_accum(), plain.read_accum(), "fused and plain accumulations")


# ---- 8. the C++ backend ------------------------------------------------------------------------------
CPP_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "render/PathTracer.h"
#include "render/Scene.h"
#include "render/Types.h"
#include "spt.h"
#include "HIPPathTracer.h"
using namespace render;
static void dump(HIPPathTracer& pt, const char* path) {
    std::vector<float> acc;
    pt.read_accumulation(acc);
    FILE* f = std::fopen(path, "wb");
    if (!f || std::fwrite(acc.data(), sizeof(float), acc.size(), f) != acc.size()) std::exit(3);
    std::fclose(f);
}
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    auto scene = std::make_shared<Scene>();
    auto* a = scene->CreateNode<SphereObject>("a");
    a->SetPosition(Vec3(0.0f, -1.0f, 5.0f));
    a->SetRadius(1.0f);
    auto* b = scene->CreateNode<SphereObject>("b");
    b->SetPosition(Vec3(0.0f, -102.0f, 5.0f));
    b->SetRadius(100.0f);
    auto settings = std::make_shared<RenderSettings>();
    settings->setResolution(48, 32);
    HIPPathTracer pt(0);
    pt.set_scene(scene);
    pt.set_settings(settings);
    const float eye[3] = {1.5f, 0.75f, -2.0f}, target[3] = {0.0f, -1.0f, 5.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    spt_camera cam;
    if (spt_camera_look_at(eye, target, up, 55.0f, &cam) != SPT_OK) return 4;
    pt.set_camera(&cam);
    for (int i = 0; i < 3; ++i) pt.render();
    if (pt.frame_count() != 3) return 5;
    dump(pt, argv[1]);
    cam.flags = SPT_CAMERA_JITTER;  // mid-accumulation: the next render() starts over
    pt.set_camera(&cam);
    if (pt.frame_count() != 3) return 6;
    pt.render();
    if (pt.frame_count() != 1) return 7;
    pt.render();
    dump(pt, argv[2]);
    pt.clear_camera();
    pt.render();
    if (pt.frame_count() != 1) return 8;
    (void)pt.get_render_result();
    std::puts("ok");
    return 0;
}
"""


def test_cpp_backend_camera(spt, ref, tmp_path):
    pkg = os.path.dirname(spt.LIB_PATH)
    src = tmp_path / "camera_backend.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "camera_backend"
    subprocess.run(["g++", "-O1", "-std=c++20", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(pkg, "csrc"), str(src), "-o", str(exe), "-L", pkg, "-lspt_render", "-lspt_hip",
                    f"-Wl,-rpath,{pkg}"], check=True)
    posed, jittered = tmp_path / "posed.f32", tmp_path / "jittered.f32"
    out = subprocess.run([str(exe), str(posed), str(jittered)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
    w, h = 48, 32
    prims = spt.sphere_prims([(0.0, -1.0, 5.0, 1.0), (0.0, -102.0, 5.0, 100.0)])
    with spt.Context(0) as ctx:
        ctx.set_scene(prims, spt.reference_materials(), spt.reference_env(True))
        ctx.configure(w, h, 4, 2, 0)
        for jitter, path, n in ((False, posed, 3), (True, jittered, 2)):
            ctx.set_camera(generic_camera(spt, jitter))
            for f in range(n):
                ctx.render(f, 1)
            assert_same(np.fromfile(path, dtype=np.float32), ctx.read_accum(), f"C++ backend, jitter={jitter}")
