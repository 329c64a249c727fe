"""The thin lens (spt_set_camera_lens: aperture radius, focus distance; Context.focus_at) on the GPU, bit for
bit on every schedule.

The expected image is composed here from the oracle's pieces, per pixel and frame in frame order, as
tests/test_gpu_camera.py does for the camera: the seed (ref_rng_seed), the two jitter draws of a jittered
camera, the lens's two draws (ref_random_float), the ray from spt_camera_lens_ray (the host build of the
function the kernels compile), ref_trace_ray — or MatScene.trace of tests/material_ref.py for material
models — from that ray and RNG state, and float32 adds into RGBA. Sizes: 37x23 (odd: a partial last chunk)
and 48x32 (full 32-pixel chunks); 5 bounces, Russian roulette from depth 2.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import material_ref as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNCES, RR = 5, 2
SIZES = [(37, 23), (48, 32)]
EYE, TARGET, VFOV = (1.5, 0.75, -2.0), (0.0, -1.0, 5.0), 55.0
LENS = (0.1, 6.0)
N_FRAMES = 15  # 3 one-frame calls + a 12-frame call (the 256-slot ring wraps with 32 live pixels)
EPS = 2.0 ** -23
BACKEND_SPHERES = [(0.0, -1.0, 5.0, 1.0), (0.0, -102.0, 5.0, 100.0)]

_scenes = {}
_frames = {}


def _oracle_entry(ref, prims, mats, env):
    rs = ref.RefScene(prims, mats, env)
    lib = ref.load()
    out = (ctypes.c_float * 4)()

    def trace(cfg, o, d, state):
        lib.ref_trace_ray(rs.h, ctypes.byref(cfg), o, d, ctypes.byref(state), out)
        return out[:]
    return (prims, mats, env, None, trace, rs)


def scene_of(spt, ref, name):
    """(prims, mats, env, models or None, tracer, the oracle's scene), built once per scene;
    tracer(cfg, o, d, state) -> (L, 1), the state advanced."""
    if name not in _scenes:
        if name == "cornell_materials":
            prims, mats, env, models = mr.cornell_materials(spt)
            ms = mr.MatScene(spt, ref, prims, mats, env, models)
            _scenes[name] = (prims, mats, env, models, ms.trace, ms)
        elif name == "backend":  # the two spheres of the backend programs, the reference's material and sky
            _scenes[name] = _oracle_entry(ref, spt.sphere_prims(BACKEND_SPHERES), spt.reference_materials(),
                                          spt.reference_env(True))
        else:
            _scenes[name] = _oracle_entry(ref, *spt.build_scene(name))
    return _scenes[name]


def camera(spt, jitter=False):
    return spt.look_at(EYE, TARGET, vfov=VFOV, jitter=jitter)


def make_lens(spt, lens):
    l = spt.SptLens()
    l.radius, l.focus_distance = lens
    return l


def lens_frames(spt, ref, scene, w, h, cam, lens, flags, n_frames, bounces=BOUNCES, rr=RR, tag="generic"):
    """[n_frames, h, w, 4] float32: trace_ray's (L, 1) of every pixel of frames 0 .. n_frames - 1 through `cam`
    (its jitter flag included) and `lens` (None: the pinhole), composed from the oracle's pieces. Cached: read only."""
    key = (scene, w, h, tag, int(cam.flags), lens, flags, n_frames, bounces, rr)
    if key in _frames:
        return _frames[key]
    trace = scene_of(spt, ref, scene)[4]
    lib, slib = ref.load(), spt.load_library()
    cfg = ref.RefConfig(w, h, bounces, rr, flags)
    f3 = ctypes.c_float * 3
    o, d, state = f3(), f3(), ctypes.c_uint32()
    jitter = bool(cam.flags & spt.CAMERA_JITTER)
    l = make_lens(spt, lens) if lens else None
    img = np.zeros((n_frames, h, w, 4), dtype=np.float32)
    for f in range(n_frames):
        for y in range(h):
            for x in range(w):
                state.value = lib.ref_rng_seed(x, y, w, f + 1)
                jx = jy = 0.0
                if jitter:
                    jx = lib.ref_random_float(ctypes.byref(state))
                    jy = lib.ref_random_float(ctypes.byref(state))
                if l is not None:
                    u1 = lib.ref_random_float(ctypes.byref(state))
                    u2 = lib.ref_random_float(ctypes.byref(state))
                    assert slib.spt_camera_lens_ray(ctypes.byref(cam), ctypes.byref(l), w, h, x, y, jx, jy, u1, u2, o, d) == 0
                else:
                    assert slib.spt_camera_ray(ctypes.byref(cam), w, h, x, y, jx, jy, o, d) == 0
                img[f, y, x] = trace(cfg, o, d, state)
    img.setflags(write=False)
    _frames[key] = img
    return img


accumulate, bits, assert_same = mr.accumulate, mr.bits, mr.assert_same


def setup(spt, ref, ctx, scene, w, h, flags, cam, lens, **cfg):
    prims, mats, env, models = scene_of(spt, ref, scene)[:4]
    ctx.set_scene(prims, mats, env)
    ctx.set_env_map(None)
    ctx.configure(w, h, BOUNCES, RR, flags, **cfg)
    ctx.set_material_models(models)
    ctx.set_camera(cam)
    if lens is None:
        ctx.set_camera_lens(None)
    else:
        ctx.set_camera_lens(*lens)


@pytest.fixture(scope="module")
def lens_ctx(spt):
    """One context for the lens tests (not the session's: a camera and its lens outlive spt_configure)."""
    ctx = spt.Context(0)
    yield ctx
    ctx.close()


# ---- every schedule ---------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("nee", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("scene", ["cornell", "app"])
def test_lens_every_schedule(spt, ref, lens_ctx, scene, w, h, nee, jitter):
    ctx = lens_ctx
    flags = spt.FLAG_NEE if nee else 0
    cam = camera(spt, jitter)
    frames = lens_frames(spt, ref, scene, w, h, cam, LENS, flags, N_FRAMES)
    what = f"{scene} {w}x{h} nee={nee} jitter={jitter} lens"
    # three one-frame calls (k_frame on hit_mode 0: a stale camera-hit cache would show), then 12 frames (k_paths)
    setup(spt, ref, ctx, scene, w, h, flags, cam, LENS)
    for f in range(3):
        ctx.render(f, 1)
        assert int(ctx.stats().schedule) == spt.SCHEDULE_FRAME
        assert_same(ctx.read_accum(), accumulate(frames, 0, f + 1), f"{what}: one-frame call {f}")
    ctx.render(3, 12)  # (first_frame = 3)
    st = ctx.stats()
    assert int(st.schedule) == spt.SCHEDULE_PERSISTENT and int(st.view_cached) == 0
    assert_same(ctx.read_accum(), accumulate(frames, 0, 15), f"{what}: k_paths after the one-frame calls")
    ctx.reset()
    ctx.render(0, 13)
    assert int(ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
    assert_same(ctx.read_accum(), accumulate(frames, 0, 13), f"{what}: k_paths")
    # the statistics kernels are instantiations of their own
    ctx.set_profiling(False, counters=True)
    ctx.reset()
    ctx.render(0, 4)
    ctx.render(4, 1)
    assert_same(ctx.read_accum(), accumulate(frames, 0, 5), f"{what}: counting kernels")
    assert int(ctx.stats().stalled_waves) == 0
    ctx.set_profiling(False)
    wave = [spt.FLAG_WAVEFRONT, spt.FLAG_WAVEFRONT | spt.FLAG_SPLIT_KERNELS]
    if scene == "app":
        wave.append(spt.FLAG_SORTED_RAYS)
    for fl in wave:
        setup(spt, ref, ctx, scene, w, h, flags | fl, cam, LENS)
        ctx.render(0, 2)
        ctx.render(2, 4)
        assert int(ctx.stats().schedule) in (spt.SCHEDULE_FUSED, spt.SCHEDULE_SPLIT)
        assert_same(ctx.read_accum(), accumulate(frames, 0, 6), f"{what}: wavefront flags {fl:#x}")
    assert int(ctx.stats().stalled_waves) == 0


@pytest.mark.parametrize("jitter", [False, True])
def test_lens_triangles_under_a_bvh(spt, ref, lens_ctx, jitter):
    """bunnylike (81,920 triangles, NEE without sphere lights): k_frame and k_paths."""
    w, h, flags = 37, 23, spt.FLAG_NEE
    cam = camera(spt, jitter)
    frames = lens_frames(spt, ref, "bunnylike", w, h, cam, LENS, flags, 6)
    setup(spt, ref, lens_ctx, "bunnylike", w, h, flags, cam, LENS)
    lens_ctx.render(0, 1)
    lens_ctx.render(1, 1)
    assert_same(lens_ctx.read_accum(), accumulate(frames, 0, 2), f"bunnylike jitter={jitter}: k_frame")
    lens_ctx.render(2, 4)
    assert int(lens_ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
    assert_same(lens_ctx.read_accum(), accumulate(frames, 0, 6), f"bunnylike jitter={jitter}: k_paths")
    assert int(lens_ctx.stats().stalled_waves) == 0


@pytest.mark.parametrize("jitter", [False, True])
def test_lens_with_material_models(spt, ref, lens_ctx, jitter):
    """Cornell with a mirror and a glass sphere (the kBsdf kernels read the camera's kind at run time)."""
    scene, (w, h) = "cornell_materials", SIZES[0]
    cam = camera(spt, jitter)
    frames = lens_frames(spt, ref, scene, w, h, cam, LENS, 0, 8)
    setup(spt, ref, lens_ctx, scene, w, h, 0, cam, LENS)
    lens_ctx.render(0, 1)
    lens_ctx.render(1, 1)
    assert int(lens_ctx.stats().schedule) == spt.SCHEDULE_FRAME
    assert_same(lens_ctx.read_accum(), accumulate(frames, 0, 2), f"materials jitter={jitter}: k_frame")
    lens_ctx.render(2, 6)
    assert int(lens_ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
    assert_same(lens_ctx.read_accum(), accumulate(frames, 0, 8), f"materials jitter={jitter}: k_paths")
    assert int(lens_ctx.stats().stalled_waves) == 0
    lens_ctx.set_material_models(None)


def test_lens_shape_specialized_k_frame(spt, ref, lens_ctx):
    """A flat scene's one-frame kernel compiled for its shape at run time (with a camera in its key) takes the
    lens as the generic one does; k_paths runs its generic per-path form."""
    scene, (w, h) = "cornell", SIZES[1]
    cam = camera(spt)
    frames = lens_frames(spt, ref, scene, w, h, cam, LENS, 0, N_FRAMES)
    setup(spt, ref, lens_ctx, scene, w, h, 0, cam, LENS)
    lens_ctx.specialize_scene()  # (waits for the shape's compiles)
    for f in range(3):
        lens_ctx.render(f, 1)
        st = lens_ctx.stats()
        assert int(st.schedule) == spt.SCHEDULE_FRAME and int(st.specialized) == 1
        assert_same(lens_ctx.read_accum(), accumulate(frames, 0, f + 1), f"specialized k_frame, frame {f}")
    lens_ctx.render(3, 4)
    st = lens_ctx.stats()
    assert int(st.specialized) == 0 and int(st.schedule) == spt.SCHEDULE_PERSISTENT
    assert_same(lens_ctx.read_accum(), accumulate(frames, 0, 7), "generic k_paths after specialize_scene")


@pytest.mark.parametrize("jitter", [False, True])
def test_lens_fused_resolve(spt, ref, jitter):
    scene, (w, h) = "cornell", SIZES[1]
    cam = camera(spt, jitter)
    frames = lens_frames(spt, ref, scene, w, h, cam, LENS, 0, N_FRAMES)
    with spt.Context(0) as plain, spt.Context(0) as fused:
        for c in (plain, fused):
            setup(spt, ref, c, scene, w, h, 0, cam, LENS)
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


@pytest.mark.parametrize("jitter", [False, True])
def test_lens_row_shard(spt, ref, lens_ctx, jitter):
    scene, (w, h) = "cornell", SIZES[0]
    cam = camera(spt, jitter)
    frames = lens_frames(spt, ref, scene, w, h, cam, LENS, 0, N_FRAMES)
    setup(spt, ref, lens_ctx, scene, w, h, 0, cam, LENS, shard_rank=1, shard_count=3)
    lens_ctx.render(0, 1)
    lens_ctx.render(1, 1)
    assert_same(lens_ctx.read_accum(), accumulate(frames, 0, 2)[1::3], f"shard jitter={jitter}: k_frame")
    lens_ctx.render(2, 6)
    assert_same(lens_ctx.read_accum(), accumulate(frames, 0, 8)[1::3], f"shard jitter={jitter}: k_paths")


# ---- state ------------------------------------------------------------------------------------------
def test_set_camera_lens_rejects_invalid_arguments(spt):
    lib = spt.load_library()
    with spt.Context(0) as ctx:
        good = make_lens(spt, LENS)
        # no camera: the reference's pinhole has no lens (not even none to remove)
        assert lib.spt_set_camera_lens(ctx.h, ctypes.byref(good)) == -1
        assert lib.spt_set_camera_lens(ctx.h, None) == -1
        ctx.set_camera(camera(spt))
        assert lib.spt_set_camera_lens(ctx.h, ctypes.byref(good)) == 0
        for radius in (-0.1, float("nan"), float("inf")):
            assert lib.spt_set_camera_lens(ctx.h, ctypes.byref(make_lens(spt, (radius, 6.0)))) == -1, radius
        for focus in (0.0, -1.0, float("nan"), float("inf")):
            assert lib.spt_set_camera_lens(ctx.h, ctypes.byref(make_lens(spt, (0.1, focus)))) == -1, focus
        for k in range(2):
            bad = make_lens(spt, LENS)
            bad.reserved[k] = 1
            assert lib.spt_set_camera_lens(ctx.h, ctypes.byref(bad)) == -1
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            ctx.set_camera_lens(-1.0, 6.0)
        assert lib.spt_set_camera_lens(ctx.h, None) == 0
        assert lib.spt_set_camera_lens(ctx.h, ctypes.byref(make_lens(spt, (0.0, 6.0)))) == 0


def test_lens_state(spt, ref, lens_ctx):
    ctx = lens_ctx
    scene, (w, h) = "cornell", SIZES[1]
    cam, cam2 = camera(spt), spt.look_at((-1.0, 0.5, -1.0), (0.5, -1.0, 5.0), vfov=70.0)
    lens2 = (0.5, 2.5)
    posed = lens_frames(spt, ref, scene, w, h, cam, None, 0, 12)
    f1 = lens_frames(spt, ref, scene, w, h, cam, LENS, 0, N_FRAMES)
    f2 = lens_frames(spt, ref, scene, w, h, cam, lens2, 0, 7)
    f3 = lens_frames(spt, ref, scene, w, h, cam2, lens2, 0, 7, tag="cam2")

    def check(want, what, n_long=5):
        """Two one-frame calls, then n_long frames in one call, from an accumulation that was reset."""
        assert ctx.frame_count == 0, what
        ctx.render(0, 1)
        ctx.render(1, 1)
        assert_same(ctx.read_accum(), accumulate(want, 0, 2), what + ": one-frame calls")
        ctx.render(2, n_long)
        assert int(ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
        assert_same(ctx.read_accum(), accumulate(want, 0, 2 + n_long), what + ": then a persistent call")

    # a lens set mid-accumulation restarts it, and drops what was cached for the posed camera's rays
    setup(spt, ref, ctx, scene, w, h, 0, cam, None)
    ctx.render(0, 1)
    ctx.render(1, 1)  # (the posed camera's hits are cached and listed now)
    ctx.render(2, 5)
    ctx.render(7, 5)  # (... and its view)
    assert int(ctx.stats().view_cached) == 1 and ctx.frame_count == 12
    assert_same(ctx.read_accum(), accumulate(posed, 0, 12), "posed, before the lens")
    ctx.set_camera_lens(*LENS)
    check(f1, "lens on")
    ctx.render(7, 5)  # a second persistent call: still no view
    st = ctx.stats()
    assert int(st.view_cached) == 0 and int(st.view_live_pixels) == 0
    assert_same(ctx.read_accum(), accumulate(f1, 0, 12), "lens: second persistent call")
    ctx.set_camera_lens(*lens2)  # another lens
    check(f2, "lens changed")
    ctx.set_camera(cam2)  # the lens stays, on the new camera's axes
    check(f3, "camera moved under the lens")
    ctx.set_camera(cam)
    ctx.configure(w, h, BOUNCES, RR, 0)  # kept across spt_configure
    check(f2, "lens across a reconfigure")
    # off again, both ways: the posed camera's bits, and its caches come back
    for off in (lambda: ctx.set_camera_lens(None), lambda: ctx.set_camera_lens(0.0, 3.0)):
        assert ctx.frame_count == 7
        off()
        check(posed, "lens off")
        ctx.render(7, 5)
        st = ctx.stats()
        assert int(st.view_cached) == 1 and int(st.view_live_pixels) > 0
        assert_same(ctx.read_accum(), accumulate(posed, 0, 12), "lens off: the cached view")
        ctx.set_camera_lens(*lens2)
        check(f2, "lens on again")
    # set_camera(None) drops the lens: the reference's camera renders, and a lens has no camera to sit on
    ctx.set_camera(None)
    no_cam = scene_of(spt, ref, scene)[5].render(w, h, 0, 7, BOUNCES, RR, 0)
    ctx.render(0, 1)
    ctx.render(1, 1)
    ctx.render(2, 5)
    assert_same(ctx.read_accum(), no_cam, "no camera, no lens")
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        ctx.set_camera_lens(*LENS)
    ctx.set_camera(cam)  # ... and a camera set afterwards has none
    check(posed, "a camera after set_camera(None)")


# ---- features and focus -----------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True])
def test_features_ignore_the_lens_and_focus_at(spt, ref, lens_ctx, jitter):
    ctx = lens_ctx
    scene, (w, h) = "app", SIZES[1]
    cam = camera(spt, jitter)
    prims = scene_of(spt, ref, scene)[0]
    setup(spt, ref, ctx, scene, w, h, 0, cam, None)
    plain = ctx.read_features()
    ctx.set_camera_lens(*LENS)  # (leaves the images valid) ...
    kept = ctx.read_features()
    ctx.configure(w, h, BOUNCES, RR, 0)  # ... and rendered again with the lens they are the same
    again = ctx.read_features()
    for a, b, c in zip(plain, kept, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))
    feat_a, feat_b, albedo = (a.reshape(h, w, 4) for a in again)
    prim = albedo.view(np.uint32)[..., 3]
    hit = prim != 0xFFFFFFFF
    sphere = hit & (prims["type"][np.where(hit, prim, 0)] == 0)
    assert sphere.any() and (~hit).any()
    # a sky pixel has nothing to focus on
    ys, xs = np.nonzero(~hit)
    assert ctx.focus_at(int(xs[0]), int(ys[0])) is None and ctx.focus_at(int(xs[-1]), int(ys[-1])) is None
    # a pixel on a sphere: the lens rays of that pixel, focused there, pass through its first hit
    O, U, V, Fw = (np.array(list(a), dtype=np.float64) for a in (cam.origin, cam.u, cam.v, cam.w))
    j = 0.5 if jitter else 0.0
    ys, xs = np.nonzero(sphere)
    for k in np.linspace(0, len(xs) - 1, 12).astype(int):
        x, y = int(xs[k]), int(ys[k])
        f = ctx.focus_at(x, y)
        assert f is not None and f == spt.camera_focus_at_hit(cam, w, h, x, y, float(feat_b[y, x, 3]), j, j)
        P = feat_a[y, x, :3].astype(np.float64)
        sx = ((x + j) / w * 2.0 - 1.0) * (w / h)
        sy = (1.0 - (y + j) / h) * 2.0 - 1.0
        p = sx * U + sy * V + Fw  # the pixel's image-plane vector, in float64
        bound = 32 * EPS * max(np.linalg.norm(O), f * np.linalg.norm(p))
        for u1, u2 in ((1.0, 0.0), (1.0, 0.4), (0.5, 0.75), (0.1, 0.2), (2.0 ** -32, 1.0)):
            o, d = spt.camera_lens_ray(cam, (0.2, f), w, h, x, y, j, j, u1, u2)
            o, d = o.astype(np.float64), d.astype(np.float64)
            v = P - o
            dist = np.linalg.norm(v - np.dot(v, d) / np.dot(d, d) * d)
            assert dist <= bound, (x, y, f, u1, u2, dist, bound)
    with pytest.raises(spt.SptError):
        ctx.focus_at(w, 0)


# ---- the backends -----------------------------------------------------------------------------------
def test_python_backend_set_lens(spt, ref):
    w, h = 48, 32
    cam = camera(spt)
    frames = lens_frames(spt, ref, "backend", w, h, cam, LENS, 0, 3, bounces=4, rr=2)
    posed = lens_frames(spt, ref, "backend", w, h, cam, None, 0, 2, bounces=4, rr=2)
    scene = spt.Scene()
    for x, y, z, r in BACKEND_SPHERES:
        s = scene.CreateNode(spt.SphereObject)
        s.SetPosition((x, y, z))
        s.SetRadius(r)
    settings = spt.RenderSettings()
    settings.setResolution(w, h)
    pt = spt.PathTracer.create_path_tracer(spt.BackendType.GPU_HIP)
    pt.set_scene(scene)
    pt.set_settings(settings)
    pt.set_camera(cam)
    pt.set_lens(*LENS)
    for _ in range(3):
        pt.render()
    assert_same(pt.read_accumulation(), accumulate(frames, 0, 3), "Python backend with a lens")
    pt.set_lens(None)  # mid-accumulation: the next render() starts over
    pt.render()
    pt.render()
    assert_same(pt.read_accumulation(), accumulate(posed, 0, 2), "Python backend, lens removed")
    pt.set_lens(spt.SptLens(*LENS))
    pt.render()
    assert_same(pt.read_accumulation(), accumulate(frames, 0, 1), "Python backend, an SptLens")
    # the camera cleared and set again with no render() between: the lens went with the cleared camera (the ctx
    # itself keeps a lens across set_camera(cam): the mirror has to remove it)
    pt.set_camera(None)
    pt.set_camera(cam)
    pt.render()
    pt.render()
    assert_same(pt.read_accumulation(), accumulate(posed, 0, 2), "Python backend, camera cleared and set again")
    # a pending lens goes with the camera too, as in the C++ backend; and removing none is nothing to do
    pt.set_lens(*LENS)
    pt.set_camera(None)
    pt.render()
    pt.set_lens(None)
    pt.render()
    # ... while a lens set after the camera was cleared has nothing to sit on
    pt.set_lens(*LENS)
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        pt.render()


def test_cpp_backend_set_lens(spt, ref, tmp_path):
    """tests/cpp/lens_backend.cpp drives render::HIPPathTracer::set_lens / clear_lens."""
    pkg = os.path.dirname(spt.LIB_PATH)
    exe = tmp_path / "lens_backend"
    subprocess.run(["g++", "-O1", "-std=c++20", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o",
                    str(exe), os.path.join(ROOT, "tests", "cpp", "lens_backend.cpp"), "-L", pkg, "-lspt_render",
                    "-lspt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    outs = [tmp_path / n for n in ("lens.f32", "lens2.f32", "posed.f32", "posed2.f32")]
    r = subprocess.run([str(exe)] + [str(p) for p in outs], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, (r.returncode, r.stdout, r.stderr)
    w, h = 48, 32
    cam = camera(spt)
    for path, lens, n in zip(outs, (LENS, (0.5, 2.5), None, None), (3, 2, 2, 2)):
        want = lens_frames(spt, ref, "backend", w, h, cam, lens, 0, n, bounces=4, rr=2)
        assert_same(np.fromfile(path, dtype=np.float32), accumulate(want, 0, n), f"C++ backend, lens {lens}")


# ---- the device build of the lens function ------------------------------------------------------------
def test_device_lens_rays(spt):
    """tests/cpp/test_device_lens: spt_device.h camera_lens_ray on the GPU against its host build, ray by ray,
    on either side of every term of the device fast path's gates."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_device_lens")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/test_device_lens"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout and " 0 mismatches" in r.stdout, r.stdout + r.stderr
    assert "x 2 forms" in r.stdout and "not reached" not in r.stdout
