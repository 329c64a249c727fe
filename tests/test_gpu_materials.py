"""Material models (spt_set_material_models: METAL and DIELECTRIC beside the Lambertian surface) on the
GPU, bit for bit against the restatement tests/cpp/ref_materials.c (tests/material_ref.py), on every
schedule: k_frame, k_paths (and their counting forms), the fused and split wavefront kernels with
k_trace_tail, the sorted-ray schedule, row shards, a jittered camera, an environment map, the fused
RGBA8 resolve. Images are 37x23 (odd: a partial last chunk) and 48x32 (full 32-pixel chunks), 5 bounces,
Russian roulette from depth 2. Two scenes (material_ref.py): Cornell, flat, with a mirror sphere, a glass
sphere and a fuzzy metal back wall; the App scene, a BVH, with metal and glass grid spheres, a sphere
light and a closed glass tetrahedron of triangles."""
import ctypes

import numpy as np
import pytest

import material_ref as mr
from material_ref import BOUNCES, RR, SIZES, accumulate, assert_same

pytestmark = pytest.mark.gpu

N_FRAMES = 8
_scenes = {}
_frames = {}


def scene_of(spt, ref, name, env_map=False):
    """(prims, mats, env, models, MatScene, env map or None), built once."""
    key = (name, env_map)
    if key not in _scenes:
        prims, mats, env, models = (mr.cornell_materials if name == "cornell" else mr.app_materials)(spt)
        em = spt.synthetic_env_map(64) if env_map else None
        _scenes[key] = (prims, mats, env, models, mr.MatScene(spt, ref, prims, mats, env, models, em), em)
    return _scenes[key]


def frames_of(spt, ref, name, w, h, flags, env_map=False):
    key = (name, w, h, flags, env_map)
    if key not in _frames:
        _frames[key] = scene_of(spt, ref, name, env_map)[4].frames(w, h, 0, N_FRAMES, flags)
    return _frames[key]


def setup(spt, ref, ctx, name, w, h, flags, env_map=False, **cfg):
    prims, mats, env, models, _, em = scene_of(spt, ref, name, env_map)
    ctx.set_camera(None)
    ctx.set_scene(prims, mats, env)
    ctx.set_env_map(em)
    ctx.configure(w, h, BOUNCES, RR, flags, **cfg)
    ctx.set_material_models(models)


@pytest.fixture(scope="module")
def mat_ctx(spt):
    ctx = spt.Context(0)
    yield ctx
    ctx.close()


def no_stall(ctx):
    assert int(ctx.stats().stalled_waves) == 0


# ---- every schedule ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nee", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("scene", ["cornell", "app"])
def test_materials_every_schedule(spt, ref, mat_ctx, scene, w, h, nee):
    ctx = mat_ctx
    flags = spt.FLAG_NEE if nee else 0
    if nee:  # both scenes have an emitter, so the flag does select the NEE kernels
        assert scene_of(spt, ref, scene)[4].rs.emitter_count() > 0
    frames = frames_of(spt, ref, scene, w, h, flags)
    what = f"{scene} {w}x{h} nee={nee}"
    setup(spt, ref, ctx, scene, w, h, flags)
    for f in range(3):  # three one-frame calls, then a 5-frame call from first frame 3
        ctx.render(f, 1)
        assert int(ctx.stats().schedule) == spt.SCHEDULE_FRAME
        assert int(ctx.stats().specialized) == 0  # (the material kernels are the generic ones)
        assert_same(ctx.read_accum(), accumulate(frames, 0, f + 1), f"{what}: one-frame call {f}")
    no_stall(ctx)
    ctx.render(3, 5)
    assert int(ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
    no_stall(ctx)
    assert_same(ctx.read_accum(), accumulate(frames, 0, 8), f"{what}: k_paths from frame 3")
    ctx.reset()
    ctx.render(0, 6)  # first frame 0
    assert int(ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
    no_stall(ctx)
    assert_same(ctx.read_accum(), accumulate(frames, 0, 6), f"{what}: k_paths from frame 0")
    ctx.reset()
    ctx.render(3, 5)  # a fresh accumulation that starts at frame 3
    assert_same(ctx.read_accum(), accumulate(frames, 3, 5), f"{what}: k_paths, frames 3..7 alone")
    # the counting kernels are instantiations of their own
    ctx.set_profiling(False, counters=True)
    ctx.reset()
    ctx.render(0, 4)
    ctx.render(4, 1)
    assert_same(ctx.read_accum(), accumulate(frames, 0, 5), f"{what}: counting kernels")
    no_stall(ctx)
    ctx.set_profiling(False)
    wave = [spt.FLAG_WAVEFRONT, spt.FLAG_WAVEFRONT | spt.FLAG_SPLIT_KERNELS]
    if scene == "app":
        wave.append(spt.FLAG_SORTED_RAYS)
    for fl in wave:
        setup(spt, ref, ctx, scene, w, h, flags | fl)
        ctx.render(0, 3)
        ctx.render(3, 5)
        assert int(ctx.stats().schedule) in (spt.SCHEDULE_FUSED, spt.SCHEDULE_SPLIT)
        assert_same(ctx.read_accum(), accumulate(frames, 0, 8), f"{what}: wavefront flags {fl:#x}")
    no_stall(ctx)


def test_materials_change_the_image(spt, ref):
    """The scenes exercise what they claim: the models change pixels, glass is entered and left (spheres and
    the tetrahedron's triangles), and with NEE an emitter seen in a mirror counts."""
    w, h = SIZES[1]
    for name in ("cornell", "app"):
        prims, mats, env, models, ms, _ = scene_of(spt, ref, name)
        plain = mr.MatScene(spt, ref, prims, mats, env).frames(w, h, 0, 2, spt.FLAG_NEE)
        with_models = frames_of(spt, ref, name, w, h, spt.FLAG_NEE)[:2]
        changed = int(np.any(mr.bits(plain) != mr.bits(with_models), axis=1).sum())
        # from the geometry at 48x32 (16 pixels per unit of tan): Cornell's two spheres (r 0.8 at z 5 and 6) cover
        # ~5 x 5 pixels each and the back wall (5 x 5 at z 8) ~10 x 10; the App scene's tetrahedron (0.8 x 0.7 at
        # z 3) ~4 x 4 and each of its 12 metal / glass grid spheres (r 0.5 at z 10) at least one pixel
        assert changed >= (2 * 100 if name == "cornell" else 2 * 16), (name, changed)


# ---- row shards: all ranks on one context --------------------------------------------------------------
def test_materials_row_shards(spt, ref, mat_ctx):
    scene, (w, h) = "cornell", SIZES[0]
    frames = frames_of(spt, ref, scene, w, h, spt.FLAG_NEE)
    for rank in range(3):
        setup(spt, ref, mat_ctx, scene, w, h, spt.FLAG_NEE, shard_rank=rank, shard_count=3)
        mat_ctx.render(0, 1)
        mat_ctx.render(1, 1)
        assert_same(mat_ctx.read_accum(), accumulate(frames, 0, 2)[rank::3], f"rank {rank}: k_frame")
        mat_ctx.render(2, 6)
        assert_same(mat_ctx.read_accum(), accumulate(frames, 0, 8)[rank::3], f"rank {rank}: k_paths")
        no_stall(mat_ctx)
    setup(spt, ref, mat_ctx, scene, w, h, spt.FLAG_NEE | spt.FLAG_WAVEFRONT, shard_rank=1, shard_count=3)
    mat_ctx.render(0, 4)
    assert_same(mat_ctx.read_accum(), accumulate(frames, 0, 4)[1::3], "rank 1: wavefront")


# ---- a jittered camera together with models ------------------------------------------------------------
def test_materials_jittered_camera(spt, ref, mat_ctx):
    scene, (w, h) = "app", SIZES[0]
    flags = spt.FLAG_NEE
    ms = scene_of(spt, ref, scene)[4]
    cam = spt.look_at((1.5, 0.75, -2.0), (0.0, -1.0, 5.0), vfov=55.0, jitter=True)
    lib, slib = ref.load(), spt.load_library()
    cfg = ref.RefConfig(w, h, BOUNCES, RR, flags)
    f3 = ctypes.c_float * 3
    o, d, state = f3(), f3(), ctypes.c_uint32()
    frames = np.zeros((N_FRAMES, h, w, 4), dtype=np.float32)
    for f in range(N_FRAMES):
        for y in range(h):
            for x in range(w):
                state.value = lib.ref_rng_seed(x, y, w, f + 1)
                jx = lib.ref_random_float(ctypes.byref(state))
                jy = lib.ref_random_float(ctypes.byref(state))
                assert slib.spt_camera_ray(ctypes.byref(cam), w, h, x, y, jx, jy, o, d) == 0
                frames[f, y, x] = ms.trace(cfg, o, d, state)
    setup(spt, ref, mat_ctx, scene, w, h, flags)
    mat_ctx.set_camera(cam)
    mat_ctx.render(0, 1)
    mat_ctx.render(1, 1)
    assert_same(mat_ctx.read_accum(), accumulate(frames, 0, 2), "jitter: k_frame")
    mat_ctx.render(2, 6)
    assert int(mat_ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
    assert_same(mat_ctx.read_accum(), accumulate(frames, 0, 8), "jitter: k_paths")
    no_stall(mat_ctx)
    mat_ctx.configure(w, h, BOUNCES, RR, flags | spt.FLAG_WAVEFRONT)  # (the camera and the models are kept)
    mat_ctx.render(0, 4)
    assert_same(mat_ctx.read_accum(), accumulate(frames, 0, 4), "jitter: wavefront")
    mat_ctx.set_camera(None)


# ---- an environment map -----------------------------------------------------------------------------
def test_materials_environment_map(spt, ref, mat_ctx):
    scene, (w, h) = "cornell", SIZES[1]
    frames = frames_of(spt, ref, scene, w, h, 0, env_map=True)
    gradient = frames_of(spt, ref, scene, w, h, 0)
    assert np.any(mr.bits(frames[0]) != mr.bits(gradient[0]))  # the map is seen (directly and in the mirror)
    setup(spt, ref, mat_ctx, scene, w, h, 0, env_map=True)
    mat_ctx.render(0, 1)
    mat_ctx.render(1, 1)
    assert_same(mat_ctx.read_accum(), accumulate(frames, 0, 2), "env map: k_frame")
    mat_ctx.render(2, 6)
    assert_same(mat_ctx.read_accum(), accumulate(frames, 0, 8), "env map: k_paths")
    setup(spt, ref, mat_ctx, scene, w, h, spt.FLAG_WAVEFRONT, env_map=True)
    mat_ctx.render(0, 4)
    assert_same(mat_ctx.read_accum(), accumulate(frames, 0, 4), "env map: wavefront")
    no_stall(mat_ctx)
    mat_ctx.set_env_map(None)


# ---- the fused RGBA8 resolve -------------------------------------------------------------------------
def test_materials_fused_resolve(spt, ref):
    scene, (w, h) = "cornell", SIZES[1]
    frames = frames_of(spt, ref, scene, w, h, spt.FLAG_NEE)
    with spt.Context(0) as plain, spt.Context(0) as fused:
        for c in (plain, fused):
            setup(spt, ref, c, scene, w, h, spt.FLAG_NEE)
        buf = np.zeros(fused.shard_pixels, dtype=np.uint32)
        fused.register_host_output(buf)
        frame = 0
        for n in (1, 1, 1, 2):
            plain.render(frame, n)
            want = plain.resolve_rgba8(frame + n)
            buf[:] = 0xdeadbeef
            fused.render_resolve_rgba8(frame, n, frame + n, out=buf)
            frame += n
            np.testing.assert_array_equal(buf, want, err_msg=f"after {frame} frames")
            np.testing.assert_array_equal(buf, ref.resolve_rgba8(accumulate(frames, 0, frame), frame))
        assert_same(fused.read_accum(), plain.read_accum(), "fused and plain accumulations")


# ---- resets and scene changes ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cornell", "app"])
def test_no_models_is_the_untouched_integrator(spt, ref, mat_ctx, scene):
    """set_material_models(None) and an all-DIFFUSE array give the bits of a context that never had models,
    against ref.render itself; spt_set_scene clears the models; setting models resets the frame count."""
    w, h = SIZES[0]
    prims, mats, env, models, ms, _ = scene_of(spt, ref, scene)
    flags = spt.FLAG_NEE
    want = ms.rs.render(w, h, 0, 7, BOUNCES, RR, flags)
    with_models = frames_of(spt, ref, scene, w, h, flags)

    def check(what):
        assert mat_ctx.frame_count == 0, what
        mat_ctx.render(0, 1)
        mat_ctx.render(1, 1)
        mat_ctx.render(2, 5)
        assert_same(mat_ctx.read_accum(), want, what)

    setup(spt, ref, mat_ctx, scene, w, h, flags)
    mat_ctx.render(0, 1)
    mat_ctx.render(1, 1)
    assert mat_ctx.frame_count == 2
    assert_same(mat_ctx.read_accum(), accumulate(with_models, 0, 2), "with models")
    mat_ctx.set_material_models(None)
    check("models -> None")
    mat_ctx.set_material_models(models)
    assert mat_ctx.frame_count == 0
    mat_ctx.render(0, 4)
    assert_same(mat_ctx.read_accum(), accumulate(with_models, 0, 4), "models again")
    mat_ctx.set_material_models([(spt.MAT_DIFFUSE, 0.0)] * len(mats))
    check("an all-DIFFUSE array")
    mat_ctx.set_material_models(models)
    mat_ctx.set_scene(prims, mats, env)  # clears them
    check("spt_set_scene clears the models")
    with pytest.raises(spt.SptError):
        mat_ctx.set_material_models(models[:-1])  # a wrong n
    with pytest.raises(spt.SptError):
        mat_ctx.set_material_models([(spt.MAT_METAL, 1.5)] * len(mats))  # fuzz out of range
    with pytest.raises(spt.SptError):
        mat_ctx.set_material_models([(7, 0.0)] * len(mats))  # an unknown kind


@pytest.mark.parametrize("scene", ["cornell", "app"])
def test_update_prims_keeps_the_models(spt, ref, mat_ctx, scene):
    w, h = SIZES[0]
    prims, mats, env, models, _, _ = scene_of(spt, ref, scene)
    spheres = [i for i in range(len(prims)) if prims[i]["type"] == 0]
    idx = spheres[-1]  # Cornell: the glass sphere; the App scene: a grid sphere
    edited = prims.copy()
    edited[idx]["p0"][0] += 0.25
    edited[idx]["p0"][1] += 0.5
    want = mr.MatScene(spt, ref, edited, mats, env, models).frames(w, h, 0, 6, spt.FLAG_NEE)
    setup(spt, ref, mat_ctx, scene, w, h, spt.FLAG_NEE)
    mat_ctx.render(0, 2)
    mat_ctx.update_prims([idx], edited[idx:idx + 1])
    assert mat_ctx.frame_count == 0
    mat_ctx.render(0, 1)
    mat_ctx.render(1, 5)
    assert_same(mat_ctx.read_accum(), accumulate(want, 0, 6), f"{scene}: models after spt_update_prims")
    no_stall(mat_ctx)


def test_equal_materials_with_different_models_stay_distinct(spt, ref, mat_ctx):
    """A flat scene's materials are compacted by spt_set_scene: two entries with the same albedo and emission
    but different models are two materials."""
    w, h = SIZES[0]
    prims = spt.sphere_prims([(-1.1, 0.0, 5.0, 1.0), (1.1, 0.0, 5.0, 1.0), (0.0, -101.0, 5.0, 100.0)])
    mats = np.concatenate([spt.reference_materials()] * 3)
    for i in range(3):
        prims[i]["material"] = i
    models = [(spt.MAT_METAL, 0.0), (spt.MAT_DIELECTRIC, 1.5), (spt.MAT_DIFFUSE, 0.0)]
    env = spt.reference_env(True)
    want = mr.MatScene(spt, ref, prims, mats, env, models).frames(w, h, 0, 5, 0)
    mat_ctx.set_camera(None)
    mat_ctx.set_scene(prims, mats, env)
    mat_ctx.set_env_map(None)
    mat_ctx.configure(w, h, BOUNCES, RR, 0)
    mat_ctx.set_material_models(models)
    mat_ctx.render(0, 1)
    mat_ctx.render(1, 4)
    assert_same(mat_ctx.read_accum(), accumulate(want, 0, 5), "three equal materials, three models")


# ---- the C++ backend's pass-through ------------------------------------------------------------------
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
    spt_material_model glass{SPT_MAT_DIELECTRIC, 1.5f, {0, 0}};
    pt.set_material_models(&glass, 1);  // before the first render(): applied once the scene is uploaded
    for (int i = 0; i < 3; ++i) pt.render();
    if (pt.frame_count() != 3) return 5;
    dump(pt, argv[1]);
    spt_material_model metal{SPT_MAT_METAL, 0.25f, {0, 0}};
    pt.set_material_models(&metal, 1);  // mid-accumulation: the next render() starts over
    pt.render();
    if (pt.frame_count() != 1) return 6;
    pt.render();
    dump(pt, argv[2]);
    pt.set_material_models(nullptr, 0);
    pt.render();
    if (pt.frame_count() != 1) return 7;
    (void)pt.get_render_result();
    std::puts("ok");
    return 0;
}
"""


def test_cpp_backend_material_models(spt, ref, tmp_path):
    import os
    import subprocess

    pkg = os.path.dirname(spt.LIB_PATH)
    src = tmp_path / "materials_backend.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "materials_backend"
    subprocess.run(["g++", "-O1", "-std=c++20", "-ffp-contract=off", "-I", os.path.join(mr.ROOT, "include"),
                    "-I", os.path.join(pkg, "csrc"), str(src), "-o", str(exe), "-L", pkg, "-lspt_render", "-lspt_hip",
                    f"-Wl,-rpath,{pkg}"], check=True)
    glass, metal = tmp_path / "glass.f32", tmp_path / "metal.f32"
    out = subprocess.run([str(exe), str(glass), str(metal)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
    w, h = 48, 32
    prims = spt.sphere_prims([(0.0, -1.0, 5.0, 1.0), (0.0, -102.0, 5.0, 100.0)])
    mats, env = spt.reference_materials(), spt.reference_env(True)
    for model, path, n in (((spt.MAT_DIELECTRIC, 1.5), glass, 3), ((spt.MAT_METAL, 0.25), metal, 2)):
        want = mr.MatScene(spt, ref, prims, mats, env, [model]).frames(w, h, 0, n, 0, bounces=4, rr=2)
        assert_same(np.fromfile(path, dtype=np.float32), accumulate(want, 0, n), f"C++ backend, model {model}")
