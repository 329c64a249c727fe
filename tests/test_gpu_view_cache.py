"""Flat k_paths over a view's cached bounce 0 (spt_tuning.view_cache, spt_kernels.h ViewPlan), bit for bit.

The first persistent call after a change of scene, camera, sky or configuration computes every pixel's
bounce 0 in its chunks, as before, and builds the view's lists behind it; the calls that follow run over
the lists (spt_stats.view_cached). Every case compares the accumulation's bits with a ctx that never
caches (view_cache = -1) and, where the oracle renders the view, with the oracle. Cornell 70x37: chunks
cross row ends, the last chunk is partial, and the view is mixed (box, sky around it).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, BOUNCES, RR = 70, 37, 8, 2
CALLS = (5, 5, 5)  # three calls continuing one accumulation: built behind the first, recorded, ordered

_oracle = {}
_plain = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def assert_same(got, want, what):
    g, r = bits(got), bits(want)
    bad = np.flatnonzero(np.any(g != r, axis=1))
    print(f"{what}: {bad.size} of {g.shape[0]} pixels differ")
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} pixels differ, first {bad[:5]}"


def oracle(spt, ref, w, h, frames, bounces, flags, rank=0, world=1):
    key = (w, h, frames, bounces, flags, rank, world)
    if key not in _oracle:
        prims, mats, env = spt.build_scene("cornell")
        r = ref.RefScene(prims, mats, env).render(w, h, 0, frames, bounces, RR, flags, row_step=world, row_offset=rank)
        r.setflags(write=False)
        _oracle[key] = r
    return _oracle[key]


def render_calls(spt, calls=CALLS, w=W, h=H, bounces=BOUNCES, flags=0, tuning=None, counters=False, rank=0, world=1,
                 camera=None, edit=None, prelude=None):
    """A fresh ctx on the Cornell box: `prelude(ctx)` (renders of another state, then the change under test),
    then `calls` continuing one accumulation. Returns (accumulation, the stats after each call)."""
    prims, mats, env = spt.build_scene("cornell")
    with spt.Context(0) as ctx:
        ctx.set_tuning(**(tuning or {}))
        ctx.set_scene(prims, mats, env)
        if edit is not None:
            ctx.update_prims(*edit)
        ctx.configure(w, h, bounces, RR, flags, rank, world, 0)
        if camera is not None:
            ctx.set_camera(camera)
        if counters:
            ctx.set_profiling(False, counters=True)
        if prelude is not None:
            prelude(ctx)
        stats, f = [], 0
        for n in calls:
            ctx.render(f, n)
            f += n
            st = ctx.stats()
            assert st.schedule == spt.SCHEDULE_PERSISTENT
            stats.append(st)
        return ctx.read_accum(), stats


def plain(spt, **kw):
    """The same renders by a ctx that never caches the view; computed once per case, read only."""
    key = repr(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _plain:
        tuning = dict(kw.pop("tuning", None) or {}, view_cache=-1)
        acc, stats = render_calls(spt, tuning=tuning, **kw)
        assert all(st.view_cached == 0 and st.view_live_pixels == 0 for st in stats)
        acc.setflags(write=False)
        _plain[key] = (acc, stats)
    return _plain[key]


def assert_cached(stats, pixels, mixed=True):
    assert stats[0].view_cached == 0, "the first call after a change computes bounce 0 itself"
    for st in stats[1:]:
        assert st.view_cached == 1
    for st in stats:
        if mixed:
            assert 0 < st.view_live_pixels < pixels, (st.view_live_pixels, pixels)


@pytest.mark.parametrize("tuning", [{}, {"px_shift": 5}, {"specialize": -1}, {"specialize": 1}],
                         ids=["auto-chan", "px_shift5-pixel-lanes", "generic", "specialized"])
def test_mixed_view_odd_size(spt, ref, tuning):
    """Three calls of 5 frames under the automatic plan (small chunks at this size: the channel-lane
    kernel), with 32-pixel chunks (the pixel-lane kernel), and with the generic and the shape-specialized
    kernels. No counter names the instantiation that ran: tests/cpp/test_view_plan.cpp pins which one the
    launch plan picks for this image."""
    acc, stats = render_calls(spt, tuning=tuning)
    assert_cached(stats, W * H)
    if tuning.get("specialize") == 1:
        assert stats[-1].specialized == 1
    assert_same(acc, plain(spt, tuning=tuning)[0], f"view cache vs none, {tuning}")
    assert_same(acc, oracle(spt, ref, W, H, sum(CALLS), BOUNCES, 0), f"view cache vs the oracle, {tuning}")


def test_flat_nee(spt, ref):
    acc, stats = render_calls(spt, flags=spt.FLAG_NEE)
    assert_cached(stats, W * H)
    assert_same(acc, plain(spt, flags=spt.FLAG_NEE)[0], "NEE: view cache vs none")
    assert_same(acc, oracle(spt, ref, W, H, sum(CALLS), BOUNCES, ref.FLAG_NEE), "NEE: view cache vs the oracle")


@pytest.mark.parametrize("nee", [False, True])
def test_counters(spt, ref, nee):
    """The counting kernels over the lists: the same image and the same segments, radiance updates and
    shadow rays as the counting kernels of a ctx without the cache."""
    flags = spt.FLAG_NEE if nee else 0
    acc, stats = render_calls(spt, flags=flags, counters=True)
    assert_cached(stats, W * H)
    pacc, pstats = plain(spt, flags=flags, counters=True)
    assert_same(acc, pacc, "counters: view cache vs none")
    assert_same(acc, oracle(spt, ref, W, H, sum(CALLS), BOUNCES, ref.FLAG_NEE if nee else 0), "counters: vs the oracle")
    a, b = stats[-1], pstats[-1]
    assert list(a.segments) == list(b.segments)
    assert list(a.radiance_updates) == list(b.radiance_updates)
    assert a.shadow_rays == b.shadow_rays
    assert a.segments[0] == sum(CALLS) * W * H
    assert (a.shadow_rays > 0) == nee


def test_camera_to_an_all_sky_view(spt):
    """Cached under the reference camera, then a pose looking away from the box: no live pixel, sweep
    units only."""
    cam = spt.look_at((0.5, 0.25, 0.0), (-0.75, 1.0, -4.0), vfov=70.0)

    def prelude(ctx):
        ctx.render(0, 5)
        ctx.render(5, 5)
        assert ctx.stats().view_cached == 1
        ctx.set_camera(cam)

    acc, stats = render_calls(spt, prelude=prelude)
    assert_cached(stats, W * H, mixed=False)
    assert stats[-1].view_live_pixels == 0
    assert_same(acc, plain(spt, camera=cam)[0], "all-sky pose after a cached view vs a fresh ctx")
    assert np.all(bits(acc)[:, 3] == np.float32(sum(CALLS)).view(np.uint32))


def test_camera_to_an_all_live_view(spt):
    """... and a pose inside the box looking at its back wall: every pixel live, no sweep unit."""
    cam = spt.look_at((0.0, 0.0, 4.0), (0.0, 0.0, 8.0), vfov=60.0)

    def prelude(ctx):
        ctx.render(0, 5)
        ctx.render(5, 5)
        ctx.set_camera(cam)

    acc, stats = render_calls(spt, prelude=prelude)
    assert_cached(stats, W * H, mixed=False)
    assert stats[-1].view_live_pixels == W * H
    assert_same(acc, plain(spt, camera=cam)[0], "all-live pose after a cached view vs a fresh ctx")


def test_update_prims_between_calls(spt):
    """spt_update_prims moving a sphere between calls: the lists are built again for the edited scene."""
    prims, _, _ = spt.build_scene("cornell")
    sphere = int(np.flatnonzero(prims["type"] == spt.PRIM_SPHERE)[0])
    moved = prims[sphere:sphere + 1].copy()
    moved["p0"][0, :3] += np.array([0.6, 0.9, -0.5], dtype=np.float32)

    def prelude(ctx):
        ctx.render(0, 5)
        ctx.render(5, 5)
        ctx.update_prims([sphere], moved)
        ctx.reset()

    acc, stats = render_calls(spt, prelude=prelude)
    assert_cached(stats, W * H)
    assert_same(acc, plain(spt, edit=([sphere], moved))[0], "a moved sphere after a cached view vs a fresh ctx")
    assert not np.array_equal(bits(acc), bits(plain(spt)[0]))


def test_max_bounces_1(spt, ref):
    """max_bounces = 1 after a cached 8-bounce view: every pixel is constant, a hit's Lc is bounce 0's
    emission."""
    def prelude(ctx):
        ctx.render(0, 5)
        ctx.render(5, 5)
        ctx.configure(W, H, 1, RR, 0, 0, 1, 0)

    acc, stats = render_calls(spt, bounces=8, prelude=prelude)
    assert_cached(stats, W * H, mixed=False)
    assert stats[-1].view_live_pixels == 0
    assert_same(acc, plain(spt, bounces=1)[0], "max_bounces 1 after a cached view vs a fresh ctx")
    assert_same(acc, oracle(spt, ref, W, H, sum(CALLS), 1, 0), "max_bounces 1 vs the oracle")


def test_row_shard(spt, ref):
    """Rank 1 of 3: the lists are the shard's, its image the whole image's rows 1, 4, 7, ..."""
    acc, stats = render_calls(spt, rank=1, world=3)
    rows = len(range(1, H, 3))
    assert_cached(stats, rows * W)
    whole = oracle(spt, ref, W, H, sum(CALLS), BOUNCES, 0)
    assert_same(acc, whole[1::3], "shard 1 of 3 vs its rows of the whole image")
    assert_same(acc, plain(spt, rank=1, world=3)[0], "shard 1 of 3: view cache vs none")


def test_workload_size(spt, ref):
    """1920x1080, three calls of 4 frames: bounce 0 in the chunks, then the recorded launch over the
    lists, then the ordered one — the smallest shape whose automatic plan has a 32-pixel first tier and
    an order (8 x the resident waves x 32 pixels)."""
    w, h, calls = 1920, 1080, (4, 4, 4)
    acc, stats = render_calls(spt, calls=calls, w=w, h=h, tuning={"specialize": 1})
    assert_cached(stats, w * h)
    assert_same(acc, oracle(spt, ref, w, h, sum(calls), BOUNCES, 0), "1080p: view cache vs the oracle")
    assert_same(acc, plain(spt, calls=calls, w=w, h=h, tuning={"specialize": 1})[0], "1080p: view cache vs none")
