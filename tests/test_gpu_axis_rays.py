"""Rays with exactly-zero direction components through the whole pipeline, bit for bit, on every schedule.

The BVH slab test has reasoned-about handling of 0 * inf = NaN and of an inverse direction of +-inf, and the
flat loop sends such lanes to its general loop; ordinary cameras produce next to none of these rays. Three
cameras that produce nothing else:
  u0   u = (0, 0, 0): every ray has d.x = 0 (the rays fan out in one plane of constant x)
  uv0  u = v = 0: every pixel gets the same ray, straight down +z
  down looks exactly down -y (u and v along z and x: every pixel of a row or column shares a zero-free
       component pattern, the centre column's rays lie in a plane of constant x)
The camera origin sits at coordinates that are also vertex coordinates of the scene, so rays run along
edges and through vertices (equal t on several primitives: the lowest index wins on every path).

The expected image is test_gpu_camera.frame_radiance's composition: seed, spt.camera_ray, the oracle's
trace_ray, float32 adds in frame order; for the scene with a METAL floor the same loop around the
restatement with material models (material_ref.MatScene.trace).
"""
import ctypes

import numpy as np
import pytest

import material_ref as mr
import test_gpu_camera as tgc
from test_gpu_parity import mixed_flat_scene

pytestmark = pytest.mark.gpu

W, H, FRAMES, BOUNCES, RR = 37, 23, 3, 3, 2

_scenes = {}
_frames = {}


def axis_triangle_grid(spt):
    """72 axis-aligned triangles — 2 x 3 unit cells of two triangles each in the planes x = +-2, y = +-2 and
    z = 3, 7 around (0, 0, 5), every fifth one an emitter — over a mirror floor (METAL, fuzz 0: a bounced ray
    keeps its zero components). 73 primitives: a BVH scene on both sides."""
    prims = np.zeros(73, dtype=spt.PRIM_DTYPE)
    mats = np.zeros(3, dtype=spt.MATERIAL_DTYPE)
    mats["albedo"] = [(0.75, 0.75, 0.75), (0.6, 0.6, 0.6), (0.9, 0.9, 0.9)]
    mats["emission"][1] = (5.0, 4.0, 3.0)
    centre = np.array((0.0, 0.0, 5.0), dtype=np.float32)
    k = 0
    for ax in range(3):
        u, v = [(1, 2), (0, 2), (0, 1)][ax]
        eu, ev = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
        eu[u], ev[v] = 1.0, 1.0
        for c in (-2.0, 2.0):
            for i in range(2):
                for j in range(3):
                    p = centre.copy()
                    p[ax] += c
                    p[u] += i - 1.0
                    p[v] += j - 1.0
                    for tri in ((p, p + eu, p + ev), (p + eu + ev, p + ev, p + eu)):
                        prims[k]["type"] = spt.PRIM_TRIANGLE
                        prims[k]["material"] = 1 if k % 5 == 0 else 0
                        prims[k]["p0"][:3], prims[k]["p1"][:3], prims[k]["p2"][:3] = tri
                        k += 1
    assert k == 72
    prims[72]["type"], prims[72]["material"] = spt.PRIM_QUAD, 2
    prims[72]["p0"][:3], prims[72]["p1"][:3], prims[72]["p2"][:3] = (-6, -3, -1), (12, 0, 0), (0, 0, 12)
    models = [(spt.MAT_DIFFUSE, 0.0), (spt.MAT_DIFFUSE, 0.0), (spt.MAT_METAL, 0.0)]
    return prims, mats, spt.reference_env(True), models


# scene -> (builder, camera origin: coordinates that occur among the scene's vertices)
ORIGINS = {"flat13": (-0.5, 2.0, 5.0), "bvh33": (-0.5, 2.0, 5.0), "grid": (0.0, 0.0, 5.0)}


def scene_of(spt, ref, name):
    """(prims, mats, env, models or None, tracer); the oracle's scene is also registered with test_gpu_camera
    under this name, so its frame_radiance composes the diffuse scenes' images."""
    if name not in _scenes:
        if name == "grid":
            prims, mats, env, models = axis_triangle_grid(spt)
            ms = mr.MatScene(spt, ref, prims, mats, env, models)
            _scenes[name] = (prims, mats, env, models, ms)
        else:
            prims, mats, env = mixed_flat_scene(spt, 13 if name == "flat13" else 33)
            rs = ref.RefScene(prims, mats, env)
            tgc._scenes[("axis_rays_" + name, False)] = (prims, mats, env, rs, None)
            _scenes[name] = (prims, mats, env, None, rs)
        coords = set(np.concatenate([_scenes[name][0][f][:, :3].ravel() for f in ("p0", "p1", "p2")]).tolist())
        coords |= {float(a + b) for a in coords for b in coords}  # (a quad's and the grid's far corners)
        assert all(c in coords for c in ORIGINS[name]), (name, ORIGINS[name])
    return _scenes[name]


def camera(spt, kind, origin):
    cam = spt.SptCamera()
    cam.origin[:] = origin
    if kind == "down":
        return spt.look_at(origin, (origin[0], origin[1] - 1.0, origin[2]), up=(0.0, 0.0, 1.0), vfov=90.0)
    cam.u[:] = (0.0, 0.0, 0.0)
    cam.v[:] = (0.0, 1.0, 0.0) if kind == "u0" else (0.0, 0.0, 0.0)
    cam.w[:] = (0.0, 0.0, 1.0)
    return cam


def frames_of(spt, ref, monkeypatch, name, kind, flags):
    key = (name, kind, flags)
    if key in _frames:
        return _frames[key]
    cam = camera(spt, kind, ORIGINS[name])
    models, tracer = scene_of(spt, ref, name)[3:]
    if models is None:
        monkeypatch.setattr(tgc, "BOUNCES", BOUNCES)  # (frame_radiance reads its module's bounce limit)
        monkeypatch.setattr(tgc, "RR", RR)
        img = tgc.frame_radiance(spt, ref, "axis_rays_" + name, W, H, cam, flags, FRAMES, tag="axis_" + kind)
    else:  # frame_radiance's loop around the restatement with material models
        lib, slib = ref.load(), spt.load_library()
        cfg = ref.RefConfig(W, H, BOUNCES, RR, flags)
        f3 = ctypes.c_float * 3
        o, d, state = f3(), f3(), ctypes.c_uint32()
        img = np.zeros((FRAMES, H, W, 4), dtype=np.float32)
        for f in range(FRAMES):
            for y in range(H):
                for x in range(W):
                    state.value = lib.ref_rng_seed(x, y, W, f + 1)
                    assert slib.spt_camera_ray(ctypes.byref(cam), W, H, x, y, 0.0, 0.0, o, d) == 0
                    img[f, y, x] = tracer.trace(cfg, o, d, state)
        img.setflags(write=False)
    # the rays are what the test is about: every one has a zero component (u0, uv0); the image is not empty
    dirs = np.array([spt.camera_ray(cam, W, H, x, y)[1] for y in range(H) for x in range(W)])
    if kind == "u0":
        assert np.all(dirs[:, 0] == 0.0) and np.all(dirs[:, 2] != 0.0)
    elif kind == "uv0":
        assert np.all(dirs == np.array((0.0, 0.0, 1.0), dtype=np.float32))
    else:
        assert np.all(dirs[:, 1] < 0.0)
    assert np.any(img[..., :3] != 0.0)
    _frames[key] = img
    return img


@pytest.fixture(scope="module")
def axis_ctx(spt):
    ctx = spt.Context(0)
    yield ctx
    ctx.close()


def setup(spt, ref, ctx, name, kind, flags):
    prims, mats, env, models, _ = scene_of(spt, ref, name)
    ctx.set_camera(None)
    ctx.set_scene(prims, mats, env)
    ctx.configure(W, H, BOUNCES, RR, flags)
    if models is not None:
        ctx.set_material_models(models)
    ctx.set_camera(camera(spt, kind, ORIGINS[name]))


@pytest.mark.parametrize("nee", [False, True])
@pytest.mark.parametrize("kind", ["u0", "uv0", "down"])
@pytest.mark.parametrize("name", ["flat13", "bvh33", "grid"])
def test_axis_parallel_rays_every_schedule(spt, ref, axis_ctx, monkeypatch, name, kind, nee):
    ctx = axis_ctx
    flags = spt.FLAG_NEE if nee else 0
    frames = frames_of(spt, ref, monkeypatch, name, kind, flags)
    want = tgc.accumulate(frames, 0, FRAMES)
    what = f"{name} camera {kind} nee={nee}"
    if nee:
        assert ref.RefScene(*scene_of(spt, ref, name)[:3]).emitter_count() > 0
    # test_gpu_camera.run_schedules' list: one-frame calls (k_frame), one call (k_paths), the counting
    # kernels, the wavefront schedules (fused / split; sorted queues under a BVH)
    setup(spt, ref, ctx, name, kind, flags)
    for f in range(FRAMES):
        ctx.render(f, 1)
        assert int(ctx.stats().schedule) == spt.SCHEDULE_FRAME
        tgc.assert_same(ctx.read_accum(), tgc.accumulate(frames, 0, f + 1), f"{what}: one-frame call {f}")
    try:
        ctx.set_tuning(persistent=1)  # (k_paths for a call of 3 frames)
        ctx.reset()
        ctx.render(0, FRAMES)
        assert int(ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
        tgc.assert_same(ctx.read_accum(), want, f"{what}: k_paths")
        ctx.set_profiling(False, counters=True)
        ctx.reset()
        ctx.render(0, 2)
        ctx.render(2, 1)
        tgc.assert_same(ctx.read_accum(), want, f"{what}: counting kernels")
        assert int(ctx.stats().stalled_waves) == 0
    finally:
        ctx.set_profiling(False)
        ctx.set_tuning()
    wave = [spt.FLAG_WAVEFRONT, spt.FLAG_WAVEFRONT | spt.FLAG_SPLIT_KERNELS]
    if name != "flat13":
        wave.append(spt.FLAG_SORTED_RAYS)
    for fl in wave:
        setup(spt, ref, ctx, name, kind, flags | fl)
        ctx.render(0, 2)
        ctx.render(2, 1)
        assert int(ctx.stats().schedule) in (spt.SCHEDULE_FUSED, spt.SCHEDULE_SPLIT)
        tgc.assert_same(ctx.read_accum(), want, f"{what}: wavefront flags {fl:#x}")
    assert int(ctx.stats().stalled_waves) == 0
