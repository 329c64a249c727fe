"""The oracle's BVH (cpu_ref.c build / box_hit / closest) against the oracle's own brute-force mode, bit for bit.

Above 64 primitives RefScene walks a BVH of its own, padded like the product's by 1e-5 of the scene's
coordinate magnitude; every GPU test of a larger scene compares with that walk. RefScene(brute=True) visits
every primitive in index order and keeps the smallest t, the lowest index on a tie — the definition. Equal
images here make every existing GPU comparison mean "equal to brute force" by transitivity.

Every BVH scene the GPU suite renders, at each camera the suite uses it with, at a size or crop that keeps
brute force under about 5e8 primitive tests a case: bunnylike (81,920 triangles; the reference camera and
test_gpu_camera's posed one), the App scene (38 spheres: the oracle tests all of them in either mode, kept as
the trivial case), interior1m (a crop of a few dozen pixels, one frame), test_gpu_axis_rays' 73-primitive
grid under its three zero-component cameras, and test_gpu_bvh_depth's two deep trees. Each case renders
without and, where the scene has emitters, with FLAG_NEE (the shadow test, ref_visible); the first hits
(ref_intersect: t and primitive) are compared too, and ref_visible itself on the light samples of a few
thousand first hits.
"""
import numpy as np
import pytest

import brute_ref as br
import test_gpu_axis_rays as axis
import test_gpu_bvh_depth as depth
import test_gpu_camera as tgc

NEE = 1 << 4  # FLAG_NEE

_scenes = {}


def scene_pair(spt, ref, name):
    """(prims, mats, env, RefScene over its BVH, RefScene in brute mode), built once."""
    if name not in _scenes:
        if name == "grid":
            prims, mats, env = axis.axis_triangle_grid(spt)[:3]
        elif name == "chain":
            prims, mats, env = depth.doubling_chain(spt), spt.reference_materials(), spt.reference_env()
        elif name == "coincident":
            prims, mats, env = depth.coincident(spt), spt.reference_materials(), spt.reference_env()
        else:
            prims, mats, env = spt.build_scene(name)
        _scenes[name] = (prims, mats, env, ref.RefScene(prims, mats, env), ref.RefScene(prims, mats, env, brute=True))
    return _scenes[name]


def camera_of(spt, kind):
    if kind == "ref":
        return None
    if kind == "posed":
        return tgc.generic_camera(spt)
    return axis.camera(spt, kind, axis.ORIGINS["grid"])


# scene, camera, image size, crop (x0, y0, x1, y1), frames, bounces: the suite's own sizes or crops of them
CASES = [
    ("bunnylike", "ref", 160, 90, (60, 30, 100, 50), 2, 8),     # test_gpu_parity / smoke(): 800 pixels
    ("bunnylike", "posed", 37, 23, (8, 4, 30, 20), 2, 5),       # test_gpu_camera
    ("app", "ref", 128, 72, (0, 0, 128, 72), 3, 4),
    ("app", "posed", 37, 23, (0, 0, 37, 23), 3, 5),
    ("interior1m", "ref", 64, 36, (28, 14, 36, 19), 1, 8),      # 40 pixels, one frame
    ("grid", "u0", 37, 23, (0, 0, 37, 23), 3, 3),
    ("grid", "uv0", 37, 23, (0, 0, 37, 23), 3, 3),
    ("grid", "down", 37, 23, (0, 0, 37, 23), 3, 3),
    ("chain", "ref", 96, 64, (24, 16, 72, 48), 4, 4),
    ("coincident", "ref", 96, 64, (24, 16, 72, 48), 4, 4),
]


def test_brute_mode_is_off_by_default_and_switches(spt, ref):
    """A 65-primitive scene (the smallest with a BVH): two coincident pairs far apart in index give the lower
    index in both modes; set_brute toggles on one scene object."""
    prims = np.zeros(65, dtype=spt.PRIM_DTYPE)
    prims["type"] = spt.PRIM_SPHERE
    for i in range(65):
        prims[i]["p0"] = (0.25 * (i % 64) - 8.0, 0.0, 6.0, 0.1)  # 64 coincides with 0
    mats, env = spt.reference_materials(), spt.reference_env()
    rs = ref.RefScene(prims, mats, env)
    o, d = (-8.0, 0.0, 0.0), (0.0, 0.0, 1.0)
    a = rs.intersect(o, d)
    rs.set_brute(True)
    b = rs.intersect(o, d)
    rs.set_brute(False)
    c = rs.intersect(o, d)
    assert a[1] == b[1] == c[1] == 0 and a[0] == b[0] == c[0]
    assert not rs.visible(o, d, 100.0)
    rs.set_brute(True)
    assert not rs.visible(o, d, 100.0) and rs.visible(o, d, 5.0)


@pytest.mark.parametrize("name,kind,w,h,rect,frames,bounces", CASES)
def test_oracle_bvh_equals_brute_force(spt, ref, name, kind, w, h, rect, frames, bounces):
    prims, mats, env, bvh, brute = scene_pair(spt, ref, name)
    cam = camera_of(spt, kind)
    what = f"{name} camera {kind}"
    # first hits: t and the primitive (ties: the lowest index)
    tb, kb = br.first_hits(spt, ref, bvh, w, h, cam, rect)
    tf, kf = br.first_hits(spt, ref, brute, w, h, cam, rect)
    br.assert_same(tb[..., None], tf[..., None], what + ": first-hit t")
    assert np.array_equal(kb, kf), what + ": first-hit primitive"
    # whole paths, and the shadow test where the scene has emitters
    for flags in (0, NEE) if brute.emitter_count() > 0 else (0,):
        a = br.render(spt, ref, bvh, w, h, cam, frames, bounces, 2, flags, rect)
        b = br.render(spt, ref, brute, w, h, cam, frames, bounces, 2, flags, rect)
        br.assert_same(a, b, f"{what} flags={flags:#x}")
        assert np.all(b[..., 3] == float(frames))


@pytest.mark.parametrize("name,kind,w,h", [("bunnylike", "ref", 160, 90), ("grid", "down", 37, 23),
                                           ("interior1m", "ref", 64, 36)])
def test_oracle_shadow_test_equals_brute_force(spt, ref, name, kind, w, h):
    """ref_visible on the light samples of the first hits: the same answer from the BVH and from every
    primitive (any hit inside [0.001, tmax) occludes, so the two agree whichever primitive each meets)."""
    prims, mats, env, bvh, brute = scene_pair(spt, ref, name)
    assert brute.emitter_count() > 0
    cam = camera_of(spt, kind)
    budget = int(5e8 // max(len(prims), 1))  # brute primitive tests: one shadow ray per sample
    cap = min(budget, 3000)
    stride = max(1, (3 * w * h) // cap)  # pixels spread over the whole image, three samples each
    n = seen = occluded = 0
    for pix in range(0, w * h, stride):
        y, x = divmod(pix, w)
        if n >= cap:
            break
        o, d = (np.zeros(3, np.float32), ref.primary_dir(x, y, w, h)) if cam is None else spt.camera_ray(cam, w, h, x, y)
        got = bvh.intersect(o, d)
        if got is None:
            continue
        t, _, ng = got
        nn = ng / np.sqrt(np.float32((ng[0] * ng[0] + ng[1] * ng[1]) + ng[2] * ng[2]))
        p = (o + np.float32(t) * d) + nn * np.float32(1e-4)
        for k in range(3):
            ok, wdir, tmax, _, _ = bvh.light_sample(p, nn, (1.0, 1.0, 1.0), ref.rng_seed(x, y, w, k + 1))
            if not ok:
                continue
            n += 1
            va, vb = bvh.visible(p, wdir, tmax), brute.visible(p, wdir, tmax)
            assert va == vb, (name, x, y, k)
            seen += va
            occluded += not va
    print(f"{name}: {n} shadow rays, {seen} unoccluded, {occluded} occluded")
    assert seen > 0 and occluded > 0  # both answers occur
