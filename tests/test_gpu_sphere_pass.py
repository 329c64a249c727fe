"""The one-pass sphere test of the shape-specialized flat closest hit (spt_device.h flat_sphere_pass), bit for bit.

k_paths' kernels of a flat shape with two to four spheres compute every sphere's discriminant, run ONE root stage
per ray on the lane's first candidate sphere, and run it once more in a wave where some lane has two or
more candidates, on each lane's second candidate (spt_stats.flat_sphere_second_passes, counting kernels). Every case waits for the specialized
kernels, asserts that they ran, and compares the accumulation as uint32 with the generic kernels
(spt_tuning.specialize = -1) and with the oracle; then the counting form's image and its count of second passes.
96x64, 8 bounces, 8 frames per call (k_paths). Every scene keeps the Cornell box's walls, so its key has wall
pairs and its counting kernel is compiled for the shape.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, BOUNCES, RR, FRAMES = 96, 64, 8, 2, 8
N_WALLS = 6  # scenes.cpp cornell_walls: floor, ceiling, back, left, right, light; then the two spheres

_scenes = {}
_counts = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def assert_same(got, want, what):
    g, r = bits(got), bits(want)
    bad = np.flatnonzero(np.any(g != r, axis=1))
    print(f"{what}: {bad.size} of {g.shape[0]} pixels differ")
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} pixels differ, first {bad[:5]}"


def scene(spt, name):
    """(prims, mats, env, spheres) of a case's scene: the Cornell box's walls and the case's spheres."""
    if name in _scenes:
        return _scenes[name]
    prims, mats, env = spt.build_scene("cornell")
    walls = prims[:N_WALLS]
    if name == "cornell":
        out = prims
    elif name == "row":  # three in a row along the view axis (the camera at the origin looks down +z)
        out = np.concatenate([walls, spt.sphere_prims([(0.0, -0.4, 4.2, 0.6), (0.0, -0.4, 5.6, 0.6), (0.0, -0.4, 7.0, 0.6)])])
    elif name == "lens":  # two intersecting spheres: the paths leaving one inside the other start inside a sphere
        out = np.concatenate([walls, spt.sphere_prims([(-0.45, -1.5, 5.5, 1.0), (0.45, -1.5, 5.5, 1.0)])])
    elif name == "inside":  # the camera and the box inside one large sphere: c < 0 for every ray
        out = np.concatenate([prims, spt.sphere_prims([(0.0, 0.0, 5.0, 20.0)])])
    elif name == "emissive":  # the second sphere carries the light's material
        light = int(np.flatnonzero(mats["emission"].sum(axis=1) > 0)[0])
        out = prims.copy()
        out[N_WALLS + 1]["material"] = light
    elif name == "one":  # a one-sphere shape: the per-sphere loop, as before
        out = prims[:N_WALLS + 1]
    else:
        raise KeyError(name)
    _scenes[name] = (out, mats, env, int(np.sum(out["type"] == spt.PRIM_SPHERE)))
    return _scenes[name]


def render(spt, name, flags=0, specialize=1, counters=False):
    prims, mats, env, _ = scene(spt, name)
    with spt.Context(0) as ctx:
        ctx.set_tuning(specialize=specialize)
        ctx.set_scene(prims, mats, env)
        ctx.configure(W, H, BOUNCES, RR, flags)
        ctx.specialize_scene()
        if counters:
            ctx.set_profiling(False, counters=True)
        ctx.render(0, FRAMES)
        st = ctx.stats()
        return ctx.read_accum(), st


def check(spt, ref, name, flags=0):
    """The specialized kernels' image against the generic kernels' and the oracle's; then the counting form's
    image and its count of second passes, which is returned."""
    prims, mats, env, spheres = scene(spt, name)
    acc, st = render(spt, name, flags)
    assert st.schedule == spt.SCHEDULE_PERSISTENT
    assert st.specialized == 1, "the shape-specialized kernel did not run"
    assert st.flat_pairs == 2, st.flat_pairs
    gen, st_g = render(spt, name, flags, specialize=-1)
    assert st_g.specialized == 0
    assert_same(acc, gen, f"{name}: specialized against generic")
    want = ref.RefScene(prims, mats, env).render(W, H, 0, FRAMES, BOUNCES, RR, flags)
    assert_same(acc, want, f"{name}: specialized against the oracle")
    acc_c, st_c = render(spt, name, flags, counters=True)
    assert st_c.specialized == 1 and st_c.flat_pairs == 2
    assert_same(acc_c, acc, f"{name}: the counting form against the timed one")
    second = int(st_c.flat_sphere_second_passes)
    wave_steps = int(st_c.lane_slots) // 64
    print(f"{name} (flags {flags}): {spheres} spheres, sphere second passes {second} in {wave_steps} wave-steps, "
          f"pair second passes {st_c.flat_pair_second_passes}")
    _counts[(name, flags)] = (second, wave_steps)
    return second


def test_cornell(spt, ref):
    """The benchmark's scene: its two spheres stand side by side, so few rays have both as candidates."""
    check(spt, ref, "cornell")


def test_cornell_nee(spt, ref):
    """Light sampling: the shadow rays go through the one-pass test too, their search starting from smax."""
    check(spt, ref, "cornell", flags=spt.FLAG_NEE)


def test_three_spheres_in_a_row(spt, ref):
    """Many camera rays cross two or three of the spheres: the second pass runs."""
    assert check(spt, ref, "row") > 0


def test_two_intersecting_spheres(spt, ref):
    """Origins on one sphere inside the other: the near root lies behind the origin, the far root is the hit."""
    assert check(spt, ref, "lens") > 0


def test_camera_and_box_inside_a_large_sphere(spt, ref):
    """c < 0 for every ray against the large sphere: it is every lane's candidate, never culled."""
    assert check(spt, ref, "inside") > 0


def test_emissive_sphere(spt, ref):
    check(spt, ref, "emissive")


def test_one_sphere_runs_the_loop(spt, ref):
    """A key with one sphere keeps the per-sphere loop (and its machine code): nothing to count."""
    assert check(spt, ref, "one") == 0
