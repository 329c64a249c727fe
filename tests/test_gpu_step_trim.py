"""The trimmed step of the shape-specialized flat k_paths under the range bit, bit for bit.

Under the bit (spt_kernels.h kShapeRanges) the wide k_paths shades a step as a hit case and a miss case that
assign the path's state in place and add T * emission without the emission flag's select (spt_kernels.hip
shade_hit_ranged, shade_miss_ranged), and every ranged k_paths form applies the new direction's quadrant after
its products (spt_device.h bounce_dir_xy). Neither may change a bit: every case waits for the specialized
kernels, asserts that they ran with the bit, and compares the accumulation as uint32 with the generic kernels
(spt_tuning.specialize = -1) and with the oracle.

96x64, 8 bounces, RR depth 2, two calls of 64 frames continuing one accumulation (one test: of 8). The first
call builds the view's lists, the second runs the form under test over them:
  wide, wide-split   wide_chunks = 1, the halves on one stream or two (the benchmark's form)
  narrow             wide_chunks = -1 with 32-pixel chunks: the pixel-lane kernel
  shard              rank 3 of 8 by rows under the automatic plan: the channel-lane kernel
The scenes are the Cornell box with one thing changed: what the dropped select and the split touch (no sky, an
emissive sphere, a flagged emission with +0 components, an albedo channel of 0, sphere hits from inside).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, BOUNCES, RR = 96, 64, 8, 2
WHITE, RED, GREEN, LIGHT = 0, 1, 2, 3  # scenes.cpp cornell_walls' materials
SPHERE_B = 7  # its quads: floor, ceiling, back, left, right, light; then the two spheres
RANK, WORLD = 3, 8
FORMS = {
    "wide": dict(tuning={"wide_chunks": 1, "split_streams": -1}, wide=1, split=0),
    "wide-split": dict(tuning={"wide_chunks": 1, "split_streams": 1}, wide=1, split=1),
    "narrow": dict(tuning={"wide_chunks": -1, "px_shift": 5}, wide=0, split=None),
    "shard": dict(tuning={}, wide=0, split=None, rank=RANK, world=WORLD),
}
SCENES = ["cornell", "sky_off", "emissive_sphere", "emission_zero_flagged", "albedo_zero", "inside_sphere"]

_oracle = {}
_generic = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def assert_same(got, want, what):
    g, r = bits(got), bits(want)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bad = np.flatnonzero(np.any(g != r, axis=1))
    print(f"{what}: {bad.size} of {g.shape[0]} pixels differ")
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} pixels differ, first {bad[:5]}"


def scene(spt, name):
    prims, mats, env = spt.build_scene("cornell")
    prims, mats = prims.copy(), mats.copy()
    if name == "sky_off":  # a miss adds nothing: the miss case without its term
        env = spt.reference_env(False)
    elif name == "emissive_sphere":  # an emitter whose normal is computed, and whose paths go on (albedo 0.78)
        prims[SPHERE_B]["material"] = LIGHT
    elif name == "emission_zero_flagged":
        # the left wall: a flagged emission with two +0 components (a flagged all-zero emission cannot be set:
        # the flag is derived from the components); 2^-60 times a throughput >= 2^-40 is no denormal
        mats[RED]["emission"][:] = (0.0, 0.0, 2.0 ** -60)
    elif name == "albedo_zero":  # the white material's green: a throughput component of exactly 0 from the first hit on
        mats[WHITE]["albedo"][1] = 0.0
    elif name == "inside_sphere":  # the camera (the origin) inside a sphere: every camera ray hits it from inside
        prims = np.concatenate([prims, spt.sphere_prims([(0.2, -0.1, 0.3, 1.0)], material=WHITE)])
    else:
        assert name == "cornell", name
    return prims, mats, env


def oracle(spt, ref, name, frames):
    """The whole image, computed once per scene and length, read only; a shard takes its rows of it."""
    if (name, frames) not in _oracle:
        prims, mats, env = scene(spt, name)
        acc = ref.RefScene(prims, mats, env).render(W, H, 0, frames, BOUNCES, RR, 0)
        acc.setflags(write=False)
        _oracle[name, frames] = acc
    return _oracle[name, frames]


def render(spt, name, form, calls=(64, 64), specialize=1, counters=False):
    """A fresh ctx; `calls` continuing one accumulation. Returns (accumulation, stats after the last call)."""
    f = FORMS[form]
    prims, mats, env = scene(spt, name)
    with spt.Context(0) as ctx:
        ctx.set_tuning(specialize=specialize, **f["tuning"])
        ctx.set_scene(prims, mats, env)
        ctx.configure(W, H, BOUNCES, RR, 0, f.get("rank", 0), f.get("world", 1), 0)
        if counters:
            ctx.set_profiling(False, counters=True)
        ctx.specialize_scene()
        first = 0
        for n in calls:
            ctx.render(first, n)
            first += n
        return ctx.read_accum(), ctx.stats()


def generic(spt, name, form, calls=(64, 64)):
    if (name, form, calls) not in _generic:
        acc, st = render(spt, name, form, calls, specialize=-1)
        assert st.specialized == 0 and st.flat_ranges == 0
        acc.setflags(write=False)
        _generic[name, form, calls] = acc
    return _generic[name, form, calls]


def check_stats(spt, st, form):
    f = FORMS[form]
    assert st.schedule == spt.SCHEDULE_PERSISTENT
    assert st.specialized == 1, "the shape-specialized kernel did not run"
    assert st.flat_ranges == 1, "the kernel ran without the range bit"
    assert st.view_cached == 1 and st.view_wide == f["wide"]
    if f["split"] is not None:
        assert st.view_split == f["split"]


def check(spt, ref, name, form, calls=(64, 64)):
    acc, st = render(spt, name, form, calls)
    check_stats(spt, st, form)
    assert_same(acc, generic(spt, name, form, calls), f"{name}, {form}: specialized against generic")
    want = oracle(spt, ref, name, sum(calls))
    if "world" in FORMS[form]:
        want = want[RANK::WORLD]
    assert_same(acc, want, f"{name}, {form}: specialized against the oracle")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", SCENES)
def test_scene(spt, ref, name, form):
    check(spt, ref, name, form)


def test_eight_frames_per_call(spt, ref):
    """Short launches: the ring drains and the hand-out's window closes within a few steps of the loop."""
    check(spt, ref, "cornell", "wide-split", calls=(8, 8))


@pytest.mark.parametrize("form", ["wide", "narrow"])
@pytest.mark.parametrize("name", ["cornell", "sky_off", "emission_zero_flagged"])
def test_counting_form(spt, ref, name, form):
    """The counting kernels still evaluate `contributes` (the emission flag at a hit, the sky at a miss) for
    radiance_updates, which no select-free sum can stand in for: per bounce it and the segments equal the generic
    counting kernel's, and the image is the oracle's."""
    acc, st = render(spt, name, form, counters=True)
    check_stats(spt, st, form)
    gen, gst = render(spt, name, form, specialize=-1, counters=True)
    assert gst.specialized == 0 and gst.flat_ranges == 0
    print("segments", list(st.segments), "radiance_updates", list(st.radiance_updates))
    assert st.segments_total > 0
    assert list(st.segments) == list(gst.segments)
    assert list(st.radiance_updates) == list(gst.radiance_updates)
    assert_same(acc, gen, f"{name}, {form}, counting: specialized against generic")
    assert_same(acc, oracle(spt, ref, name, 128), f"{name}, {form}, counting: specialized against the oracle")
