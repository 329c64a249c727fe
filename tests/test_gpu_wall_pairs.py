"""The paired wall test of the shape-specialized flat closest hit (spt_kernels.hip flat_pair_tests), bit for bit.

A flat scene's opposite walls are paired on the host (scene.cpp flat_wall_pairs, spt_stats.flat_pairs) and
the specialized k_paths tests, per lane, only the wall of a pair that the ray faces; a wave with a lane
whose ray starts outside the pair's slab tests both (spt_stats.flat_pair_second_passes, counting kernels).
Every case waits for the specialized kernels, asserts that they ran with pairs in their key, and compares
the accumulation as uint32 with the generic kernels (spt_tuning.specialize = -1) and with the oracle.
96x64, 8 bounces, 8 frames per call (k_paths); the last case 2 frames (k_frame, which ignores the pairs).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, BOUNCES, RR, FRAMES = 96, 64, 8, 2, 8
LEFT_WALL = 3  # scenes.cpp cornell_walls: floor, ceiling, back, left, right, light; then the two spheres

_oracle = {}
_generic = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def assert_same(got, want, what):
    g, r = bits(got), bits(want)
    bad = np.flatnonzero(np.any(g != r, axis=1))
    print(f"{what}: {bad.size} of {g.shape[0]} pixels differ")
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} pixels differ, first {bad[:5]}"


def quad(spt, q, u, v, material):
    p = np.zeros(1, dtype=spt.PRIM_DTYPE)
    p[0]["type"] = spt.PRIM_QUAD
    p[0]["material"] = material
    p[0]["p0"][:3], p[0]["p1"][:3], p[0]["p2"][:3] = q, u, v
    return p


def scene(spt, name):
    """(prims, mats, env) of a case's scene."""
    prims, mats, env = spt.build_scene("cornell")
    if name == "straddle":
        # a sphere through the right wall near the box's open front (its outer part is seen past the wall's
        # edge), a wall outside the box on x = 4 (the x pairs become (left, outer) with the right wall
        # unpaired between them) and the floor continued to x = 5 (a second, nested y pair with the light)
        sph = spt.sphere_prims([(2.5, 0.0, 3.4, 0.8)], material=0)
        outer = quad(spt, (4.0, -2.5, 3.0), (0.0, 0.0, 5.0), (0.0, 5.0, 0.0), 2)
        floor2 = quad(spt, (2.5, -2.5, 3.0), (0.0, 0.0, 5.0), (2.5, 0.0, 0.0), 0)
        prims = np.concatenate([prims, sph, outer, floor2])
    elif name == "moved":
        # the left wall (x = -2.5) moved to x = 4, right of the right wall: the pair's order flips
        prims = prims.copy()
        prims[LEFT_WALL]["p0"][0] = 4.0
    return prims, mats, env


def outside_camera(spt):
    """Right of the box (x = 4 > 2.5), looking into its open front and at the right wall's outer face."""
    return spt.look_at((4.0, 0.5, -1.0), (0.5, -1.0, 5.5), vfov=60.0)


def oracle(spt, ref, name, flags, frames, cam=None):
    key = (name, flags, frames, cam is not None)
    if key in _oracle:
        return _oracle[key]
    prims, mats, env = scene(spt, name)
    rs = ref.RefScene(prims, mats, env)
    if cam is None:
        acc = rs.render(W, H, 0, frames, BOUNCES, RR, flags)
    else:  # the oracle's pieces behind the camera's rays (spt_camera_ray: the function the kernels compile)
        lib, slib = ref.load(), spt.load_library()
        cfg = ref.RefConfig(W, H, BOUNCES, RR, flags)
        f3 = ctypes.c_float * 3
        o, d, out = f3(), f3(), (ctypes.c_float * 4)()
        state = ctypes.c_uint32()
        acc = np.zeros((H, W, 4), dtype=np.float32)
        for f in range(frames):
            img = np.zeros((H, W, 4), dtype=np.float32)
            for y in range(H):
                for x in range(W):
                    state.value = lib.ref_rng_seed(x, y, W, f + 1)
                    assert slib.spt_camera_ray(ctypes.byref(cam), W, H, x, y, 0.0, 0.0, o, d) == 0
                    lib.ref_trace_ray(rs.h, ctypes.byref(cfg), o, d, ctypes.byref(state), out)
                    img[y, x] = out[:]
            acc = acc + img
    acc.setflags(write=False)
    _oracle[key] = acc
    return acc


def render(spt, name, flags=0, frames=FRAMES, cam=None, specialize=1, counters=False, edit_from=None, **tuning):
    """A fresh ctx: the scene (edit_from: that scene first, then `name`'s left wall through spt_update_prims),
    the configuration, the camera; the specialized kernels waited for; one call of `frames` frames.
    Returns (accumulation, stats)."""
    prims, mats, env = scene(spt, name)
    with spt.Context(0) as ctx:
        ctx.set_tuning(specialize=specialize, **tuning)
        if edit_from is None:
            ctx.set_scene(prims, mats, env)
        else:
            ctx.set_scene(*scene(spt, edit_from))
            ctx.update_prims([LEFT_WALL], prims[[LEFT_WALL]])
        ctx.configure(W, H, BOUNCES, RR, flags)
        if cam is not None:
            ctx.set_camera(cam)
        ctx.specialize_scene()
        if counters:
            ctx.set_profiling(False, counters=True)
        ctx.render(0, frames)
        st = ctx.stats()
        return ctx.read_accum(), st


def generic(spt, name, flags=0, frames=FRAMES, cam=None, **tuning):
    key = (name, flags, frames, cam is not None, repr(sorted(tuning.items())))
    if key not in _generic:
        acc, st = render(spt, name, flags, frames, cam, specialize=-1, **tuning)
        assert st.specialized == 0 and st.flat_pairs == 0
        acc.setflags(write=False)
        _generic[key] = acc
    return _generic[key]


def check(spt, ref, name, flags=0, frames=FRAMES, cam=None, pairs=2, edit_from=None, **tuning):
    """The specialized kernels' image against the generic kernels' and the oracle's; then the counting form's
    image and its count of second passes, which is returned."""
    acc, st = render(spt, name, flags, frames, cam, edit_from=edit_from, **tuning)
    assert st.schedule == spt.SCHEDULE_PERSISTENT
    assert st.specialized == 1, "the shape-specialized kernel did not run"
    assert st.flat_pairs == pairs, (st.flat_pairs, pairs)
    assert_same(acc, generic(spt, name, flags, frames, cam, **tuning), f"{name}: specialized against generic")
    assert_same(acc, oracle(spt, ref, name, flags, frames, cam), f"{name}: specialized against the oracle")
    acc_c, st_c = render(spt, name, flags, frames, cam, counters=True, edit_from=edit_from, **tuning)
    assert st_c.specialized == 1 and st_c.flat_pairs == pairs
    assert_same(acc_c, acc, f"{name}: the counting form against the timed one")
    print(f"{name}: flat_pairs {st_c.flat_pairs}, second passes {st_c.flat_pair_second_passes}, "
          f"lane slots {st_c.lane_slots}")
    return int(st_c.flat_pair_second_passes)


@pytest.mark.parametrize("tuning", [{}, {"px_shift": 5}], ids=["auto-chan", "px_shift5-pixel-lanes"])
def test_cornell(spt, ref, tuning):
    """Every ray of the step loop starts inside the box (hit + 1e-4 * normal, far more than the rounding of a
    hit point on a wall at 2.5): no wave needs the second pass. Under the automatic plan (small chunks at
    this size: the channel-lane kernel) and with 32-pixel chunks (the pixel-lane kernel, the benchmark's)."""
    assert check(spt, ref, "cornell", **tuning) == 0


def test_cornell_nee(spt, ref):
    """Light sampling: the shadow rays go through the paired test too, their search starting from smax."""
    second = check(spt, ref, "cornell", flags=spt.FLAG_NEE)
    assert second == 0


def test_sphere_through_the_wall_and_quads_outside(spt, ref):
    """Rays leaving the sphere's outer part, the outer wall and the continued floor start outside a slab, in
    waves whose other lanes start inside: the second pass runs, for some waves. x: (left, outer), the right
    wall unpaired; y: (floor, ceiling) and (continued floor, light)."""
    assert check(spt, ref, "straddle", pairs=3) > 0


def test_camera_outside_the_x_slab(spt, ref):
    """The posed camera sees the right wall's outer face: the paths leaving it start at x > 2.5."""
    assert check(spt, ref, "cornell", cam=outside_camera(spt)) > 0


def test_wall_moved_past_its_partner(spt, ref):
    """spt_update_prims moves the left wall to x = 4: the scene is prepared again, the pair is (right, moved)
    and the box's inside now lies outside its slab, so nearly every wave takes the second pass."""
    assert check(spt, ref, "moved", edit_from="cornell") > 0


def test_two_frames_run_k_frame_with_the_new_key(spt, ref):
    """k_frame ignores the key's pair bits (it tests every wall) and runs specialized all the same."""
    acc, st = render(spt, "cornell", frames=2)
    assert st.schedule == spt.SCHEDULE_FRAME
    assert st.specialized == 1 and st.flat_pairs == 2
    assert_same(acc, generic(spt, "cornell", frames=2), "k_frame: specialized against generic")
    assert_same(acc, oracle(spt, ref, "cornell", 0, 2), "k_frame: specialized against the oracle")
