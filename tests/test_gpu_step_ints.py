"""The wide ranged k_paths step with its integer and mask work in short forms (spt_kernels.hip kStepInts), bit for bit.

Under the range bit the wide form reads an LDS shading record at a 32-bit address formed by one 24-bit multiply-add
(shade_rec_lds), reads a live record's third word at a 32-bit lane offset from the chunk's base, splits a full
chunk's slot into frame and live rank by shift and mask (spt_kernels.h slot_split_shift; a partial chunk keeps the
high multiply), runs its loop on `oldest_s < n_slots` alone and takes closest_flat's `redo` test from the sphere
pass's own lane masks. None of it may change a bit: every case forces wide_chunks = 1, waits for the specialized
kernels, asserts that the wide kernel ran with the bit, and compares the accumulation as uint32 with the generic
kernels (spt_tuning.specialize = -1) and with the oracle.

Two calls continuing one accumulation: the first builds the view's lists, the second runs the wide form over them.
  cornell        96x64: the live count is no multiple of 64, so full chunks (shift) and a partial last one (multiply)
  one_partial    4x3: fewer than 16 live pixels, one partial chunk and nothing else: the multiply's path alone
  twenty         Cornell and twelve more spheres: hits on records 8 to 19, record offsets past 16 x 48 bytes (and a
                 shape of more than four spheres: the per-sphere loop, whose `redo` keeps its ballot)
  corner_zero    the box moved by +2.5 in x: the left wall lies in x = 0, the plane of the camera, and the floor's,
                 the ceiling's and the back wall's in-plane corner word in x is 0 (hu = s - 0 there): a scene for
                 which no form that needs nonzero corner words may be chosen
each split (two halves on two streams) and unsplit; cornell also with calls of 6 frames (slots no multiple of the
ring's 256), and the counting wide form's segments and radiance_updates against the generic counting form's.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUNCES, RR = 8, 2
WHITE, RED, GREEN = 0, 1, 2  # scenes.cpp cornell_walls' materials
FORMS = {
    "wide": dict(tuning={"wide_chunks": 1, "split_streams": -1}, split=0),
    "wide-split": dict(tuning={"wide_chunks": 1, "split_streams": 1}, split=1),
}
SIZES = {"cornell": (96, 64), "one_partial": (4, 3), "twenty": (96, 64), "corner_zero": (96, 64)}

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
    if name == "twenty":
        # a 4 x 3 grid of spheres in front of the box's own two, radius 0.3 (>= the scene's bound 8 / 32, so the
        # range bit holds), original indices 8 to 19
        grid = [(x, y, 4.2, 0.3) for y in (0.0, 0.9, 1.8) for x in (-1.5, -0.5, 0.5, 1.5)]
        more = spt.sphere_prims(grid, material=WHITE)
        for i in range(len(more)):
            more[i]["material"] = (WHITE, RED, GREEN)[i % 3]
        prims = np.concatenate([prims, more])
        assert len(prims) == 20
    elif name == "corner_zero":
        # every primitive's first point (a quad's corner Q, a sphere's centre) moves by +2.5 in x; the camera stays
        prims["p0"][:, 0] += 2.5
        assert prims[3]["p0"][0] == 0.0 and prims[0]["p0"][0] == 0.0 and prims[2]["p0"][0] == 0.0
    else:
        assert name in ("cornell", "one_partial"), name
    return prims, mats, env


def render(spt, name, form, calls, specialize=1, counters=False):
    """A fresh ctx; `calls` continuing one accumulation. Returns (accumulation, stats after the last call)."""
    w, h = SIZES[name]
    prims, mats, env = scene(spt, name)
    with spt.Context(0) as ctx:
        ctx.set_tuning(specialize=specialize, **FORMS[form]["tuning"])
        ctx.set_scene(prims, mats, env)
        ctx.configure(w, h, BOUNCES, RR, 0)
        if counters:
            ctx.set_profiling(False, counters=True)
        ctx.specialize_scene()
        first = 0
        for n in calls:
            ctx.render(first, n)
            first += n
        return ctx.read_accum(), ctx.stats()


def oracle(spt, ref, name, frames):
    """Computed once per scene and length, read only."""
    if (name, frames) not in _oracle:
        w, h = SIZES[name]
        prims, mats, env = scene(spt, name)
        acc = ref.RefScene(prims, mats, env).render(w, h, 0, frames, BOUNCES, RR, 0)
        acc.setflags(write=False)
        _oracle[name, frames] = acc
    return _oracle[name, frames]


def generic(spt, name, form, calls):
    if (name, form, calls) not in _generic:
        acc, st = render(spt, name, form, calls, specialize=-1)
        assert st.specialized == 0 and st.flat_ranges == 0 and st.view_wide == 1
        acc.setflags(write=False)
        _generic[name, form, calls] = acc
    return _generic[name, form, calls]


def check_stats(spt, st, name, form):
    assert st.schedule == spt.SCHEDULE_PERSISTENT
    assert st.specialized == 1, "the shape-specialized kernel did not run"
    assert st.flat_ranges == 1, "the kernel ran without the range bit"
    assert st.view_cached == 1 and st.view_wide == 1, "the wide kernel did not run"
    assert st.view_split == FORMS[form]["split"]
    live = int(st.view_live_pixels)
    print(f"{name}: {live} live pixels")
    if name == "one_partial":
        assert 0 < live < 16, "one partial chunk of the smallest tier"
    else:
        assert live > 4 * 64 and live % 64 != 0, "full 64-pixel chunks and a partial last chunk"


def check(spt, ref, name, form, calls=(64, 64)):
    acc, st = render(spt, name, form, calls)
    check_stats(spt, st, name, form)
    assert_same(acc, generic(spt, name, form, calls), f"{name}, {form}: specialized against generic")
    assert_same(acc, oracle(spt, ref, name, sum(calls)), f"{name}, {form}: specialized against the oracle")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(SIZES))
def test_scene(spt, ref, name, form):
    check(spt, ref, name, form)


@pytest.mark.parametrize("form", list(FORMS))
def test_six_frames_per_call(spt, ref, form):
    """6 frames of a live list that is no multiple of 64: the slots are no multiple of the ring's 256 entries, and the
    last frames are handed out while the window closes."""
    check(spt, ref, "cornell", form, calls=(6, 6))


@pytest.mark.parametrize("name", ["cornell", "twenty"])
def test_counting_form(spt, ref, name):
    """The counting wide form keeps its wave-level `tracing` ballot (lane_busy) and evaluates `contributes`: per bounce
    its segments and radiance_updates equal the generic counting form's, and the image is the oracle's."""
    acc, st = render(spt, name, "wide", (64, 64), counters=True)
    check_stats(spt, st, name, "wide")
    gen, gst = render(spt, name, "wide", (64, 64), specialize=-1, counters=True)
    assert gst.specialized == 0 and gst.flat_ranges == 0 and gst.view_wide == 1
    print("segments", list(st.segments), "radiance_updates", list(st.radiance_updates))
    assert st.segments_total > 0
    assert list(st.segments) == list(gst.segments)
    assert list(st.radiance_updates) == list(gst.radiance_updates)
    assert_same(acc, gen, f"{name}, counting: specialized against generic")
    assert_same(acc, oracle(spt, ref, name, 128), f"{name}, counting: specialized against the oracle")
