"""What each setter drops of a context's cached results (csrc/spt_ctx_state.h, DESIGN.md "What a change drops"), seen
from outside: a warmed context after one change renders the bits of a fresh context put into that state directly.

Cornell 70x37 (chunks cross row ends, the last chunk is partial, the view is mixed: box, sky around it), 2 bounces.
The warm-up fills every cache: two persistent calls of 5 frames (the second runs over the view's lists), two calls of
1 frame (k_frame's camera hits, stored and read), then a captured view, an active history, a blended and a denoised
image. Then one change and reset(), and 5 + 5 frames from frame 0; two more calls of 1 frame follow, so k_frame's
hits are stored and read again after the change. What survives the change is read off the entry points: the three
images raise or return, spt_reproject finds a captured view or not, and spt_stats.view_cached says whether the
first persistent call ran over lists. tests/cpp/test_ctx_state.cpp holds the whole matrix; the rows here are its
visible part.

configure_larger and configure_smaller change the image size (the Buffers cause): every configuration-sized buffer,
those the warm-up's post-processing allocated too, is of the old size and must go. Their warm-up also takes the noise
estimate (two updates and a metering), and after the renders both contexts run every post-processing producer at
the new size — noise update and meter, denoise, capture, reproject, blend — and their images are compared bit for
bit: a buffer that kept its old size would be written past its end (smaller to larger) or read with another pitch.
configure_larger_split does the same with the view split on two streams, so the halves' buffers are reallocated too.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, BOUNCES, RR = 70, 37, 2, 2
POSE = ((1.5, 0.75, -2.0), (0.0, -1.0, 5.0), 55.0)  # still sees the box, sky beside it
BASE = ((0.0, 0.0, 0.0), (0.0, -0.5, 5.0), 80.0)    # the lens case's camera (a lens needs one)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def assert_same(got, want, what):
    g, r = bits(got), bits(want)
    bad = np.flatnonzero(np.any(g != r, axis=1))
    print(f"{what}: {bad.size} of {g.shape[0]} pixels differ")
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} pixels differ, first {bad[:5]}"


def look(spt, pose):
    return spt.look_at(pose[0], pose[1], vfov=pose[2])


def moved_sphere(spt, prims):
    sphere = int(np.flatnonzero(prims["type"] == spt.PRIM_SPHERE)[0])
    moved = prims[sphere:sphere + 1].copy()
    moved["p0"][0, :3] += np.array([0.6, 0.9, -0.5], dtype=np.float32)
    return sphere, moved


def one_metal(spt, mats):
    return [(spt.MAT_METAL, 0.1) if i == 1 else (spt.MAT_DIFFUSE, 0.0) for i in range(len(mats))]


# The changes: each is applied to the warmed ctx, and to the fresh one right after its configure.
def _camera(spt, ctx, prims, mats):
    ctx.set_camera(look(spt, POSE))


def _lens(spt, ctx, prims, mats):
    ctx.set_camera_lens(0.05, 5.0)


def _env_map(spt, ctx, prims, mats):
    ctx.set_env_map(spt.synthetic_env_map(64))


def _materials(spt, ctx, prims, mats):
    ctx.set_material_models(one_metal(spt, mats))


def _update_prims(spt, ctx, prims, mats):
    sphere, moved = moved_sphere(spt, prims)
    ctx.update_prims([sphere], moved)


def _counters(spt, ctx, prims, mats):
    ctx.set_profiling(False, counters=True)


def _configure(spt, ctx, prims, mats):
    ctx.configure(W, H, BOUNCES + 1, RR, 0)


def _history_clear(spt, ctx, prims, mats):
    ctx.history_clear()


LARGER, SMALLER = (96, 54), (40, 21)


def _configure_larger(spt, ctx, prims, mats):
    ctx.configure(*LARGER, BOUNCES, RR, 0)


def _configure_smaller(spt, ctx, prims, mats):
    ctx.configure(*SMALLER, BOUNCES, RR, 0)


# case: the change; what is left after it, written out from the matrix — the active history, the blended and the
# denoised image are readable, spt_reproject finds a captured view — then whether the view's lists were dropped,
# and whether the new state's persistent launches take lists at all (not with a lens or with material models)
CASES = {
    "set_camera": (_camera, False, True, True, True, True, True),
    "set_camera_lens": (_lens, False, True, True, True, True, False),
    "set_env_map": (_env_map, False, True, True, False, True, True),
    "set_material_models": (_materials, False, True, True, False, True, False),
    "update_prims": (_update_prims, False, True, True, False, True, True),
    "set_profiling_counters": (_counters, True, True, True, True, True, True),
    "configure": (_configure, False, False, False, False, True, True),
    "history_clear": (_history_clear, False, True, True, False, False, True),
    "configure_larger": (_configure_larger, False, False, False, False, True, True),
    "configure_smaller": (_configure_smaller, False, False, False, False, True, True),
    "configure_larger_split": (_configure_larger, False, False, False, False, True, True),
}
# the image after the change, where it is not W x H
SIZE_AFTER = {"configure_larger": LARGER, "configure_smaller": SMALLER, "configure_larger_split": LARGER}


def start(spt, ctx, prims, mats, env, base_camera, split=False):
    if split:
        ctx.set_tuning(split_streams=1)  # every launch over a view's lists in two halves (their buffers: per configuration)
    ctx.set_scene(prims, mats, env)
    ctx.configure(W, H, BOUNCES, RR, 0)
    if base_camera:
        ctx.set_camera(look(spt, BASE))


def render_after(spt, ctx, noise=False):
    """5 + 5 frames from frame 0, then 1 + 1: (accumulation after 10 frames, view_cached after each persistent
    call, live pixels of the lists, accumulation after 12 frames). noise: the noise estimate's first update, of
    the 10 frames (a metering needs two)."""
    cached = []
    for first in (0, 5):
        ctx.render(first, 5)
        st = ctx.stats()
        assert st.schedule == spt.SCHEDULE_PERSISTENT
        cached.append(int(st.view_cached))
    live = int(st.view_live_pixels)
    acc10 = ctx.read_accum()
    if noise:
        ctx.noise_update(10)
    for first in (10, 11):
        ctx.render(first, 1)
        assert ctx.stats().schedule == spt.SCHEDULE_FRAME
    return acc10, cached, live, ctx.read_accum()


def post_process(ctx):
    """Every post-processing producer over the 12 frames (after render_after(noise=True)): the noise histogram and
    the images."""
    ctx.noise_update(12)
    counts = ctx.noise_meter()
    ctx.denoise(12)
    ctx.history_capture(12)
    ctx.reproject()
    ctx.history_blend(12)
    return counts, ctx.read_noise(), ctx.read_denoised(), ctx.read_history(), ctx.read_blended()


def readable(spt, read, message):
    try:
        read()
        return True
    except spt.SptError as e:
        assert message in str(e), e
        return False


@pytest.mark.parametrize("case", list(CASES))
def test_change_then_render(spt, case):
    change, hist, blend, dn, view, dropped, lists = CASES[case]
    prims, mats, env = spt.build_scene("cornell")
    lens = case == "set_camera_lens"
    resized = case in SIZE_AFTER
    split = case.endswith("_split")
    w, h = SIZE_AFTER.get(case, (W, H))
    with spt.Context(0) as ctx:
        start(spt, ctx, prims, mats, env, lens, split)
        ctx.render(0, 5)
        ctx.render(5, 5)
        st = ctx.stats()
        assert st.schedule == spt.SCHEDULE_PERSISTENT and st.view_cached == 1
        assert 0 < st.view_live_pixels < W * H
        if split:
            assert st.view_split == 1  # (the halves' buffers exist at the old size)
        if resized:
            ctx.noise_update(10)
        ctx.render(10, 1)
        ctx.render(11, 1)
        assert ctx.stats().schedule == spt.SCHEDULE_FRAME
        if resized:  # ... so the noise estimate's images exist at the old size as well
            ctx.noise_update(12)
            ctx.noise_meter()
            ctx.read_noise()
        ctx.history_capture(12)
        ctx.reproject()
        ctx.history_blend(12)
        ctx.denoise(12)
        ctx.read_history(), ctx.read_blended(), ctx.read_denoised()  # (all there: none raises)

        change(spt, ctx, prims, mats)
        ctx.reset()

        assert readable(spt, ctx.read_history, "no active history") == hist
        assert readable(spt, ctx.read_blended, "no blended image") == blend
        assert readable(spt, ctx.read_denoised, "no denoised image") == dn
        assert readable(spt, ctx.reproject, "no captured view") == view
        acc10, cached, live, acc12 = render_after(spt, ctx, resized)
        if split:
            assert ctx.stats().view_split == 1  # (the halves' buffers of the new size were used)
        post = post_process(ctx) if resized else None

    with spt.Context(0) as fresh:
        start(spt, fresh, prims, mats, env, lens, split)
        if case == "update_prims":  # the edited scene, set directly
            sphere, moved = moved_sphere(spt, prims)
            edited = prims.copy()
            edited[sphere:sphere + 1] = moved
            fresh.set_scene(edited, mats, env)
        else:
            change(spt, fresh, prims, mats)
        want10, want_cached, want_live, want12 = render_after(spt, fresh, resized)
        want_post = post_process(fresh) if resized else None

    print(f"{case}: view_cached {cached} (fresh {want_cached}), live pixels {live} (fresh {want_live})")
    assert want_cached == ([0, 1] if lists else [0, 0])
    assert cached == ([0 if dropped else 1, 1] if lists else [0, 0])
    if lists:
        assert live == want_live and 0 < live < w * h
    assert_same(acc10, want10, f"{case}: 5 + 5 frames, warmed vs fresh")
    assert_same(acc12, want12, f"{case}: ... and 1 + 1 frames, warmed vs fresh")
    if resized:
        assert acc12.shape[0] == w * h
        assert np.array_equal(post[0], want_post[0]), f"{case}: noise histogram, warmed vs fresh"
        assert np.array_equal(post[1].view(np.uint32), want_post[1].view(np.uint32)), f"{case}: noise image, warmed vs fresh"
        for got, want, what in zip(post[2:], want_post[2:], ("denoised", "history", "blended")):
            assert_same(got, want, f"{case}: {what} image at {w}x{h}, warmed vs fresh")
