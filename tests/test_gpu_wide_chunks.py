"""Flat k_paths over a view's live list in 64-pixel chunks (spt_tuning.wide_chunks, the kWide kernel), bit for bit.

The wide form changes which wave traces a path and where a pixel's bounce-0 record is read from, never a
result: every case compares the accumulation's bits with a ctx that never caches the view (view_cache = -1:
the narrow kernel computing bounce 0 itself) and, under the reference camera, with the oracle, and asserts
through spt_get_view_wide (Context.stats().view_wide) that the wide kernel ran. The automatic rule never fires at these sizes, so the
cases force wide_chunks = 1. Cornell 70x37: the live count is no multiple of 64 or of 16, so the first tier
(64 pixels), the 32- and 16-pixel tiers and a partial last chunk all run; tests/cpp/test_wide_plan.cpp pins
the plans.
"""
import pytest

from test_gpu_view_cache import BOUNCES, CALLS, H, W, assert_same, oracle, plain, render_calls

pytestmark = pytest.mark.gpu

WIDE = {"wide_chunks": 1}


def assert_wide(stats, on=True):
    """The first call computes bounce 0 itself and builds the lists (never wide); the calls behind it run over
    them, wide or not."""
    assert stats[0].view_wide == 0
    for st in stats[1:]:
        assert st.view_cached == 1
        assert st.view_wide == (1 if on else 0)


@pytest.mark.parametrize("specialize", [1, -1], ids=["specialized", "generic"])
def test_wide_mixed_view(spt, ref, specialize):
    tuning = dict(WIDE, specialize=specialize)
    acc, stats = render_calls(spt, tuning=tuning)
    assert_wide(stats)
    live = stats[-1].view_live_pixels
    print(f"live pixels {live} of {W * H}")
    assert live > 4 * 64 and live % 64 != 0 and live % 16 != 0, "full 64-pixel chunks and a partial last chunk"
    assert stats[-1].specialized == (1 if specialize == 1 else 0)
    assert stats[-1].view_split == 0
    assert_same(acc, plain(spt, tuning=tuning)[0], f"wide vs no view cache, specialize {specialize}")
    assert_same(acc, oracle(spt, ref, W, H, sum(CALLS), BOUNCES, 0), f"wide vs the oracle, specialize {specialize}")


def test_wide_split_streams(spt, ref):
    """Two halves on two streams, each with its own wide plan; the cut falls on a multiple of 64."""
    tuning = dict(WIDE, split_streams=1, specialize=1)
    acc, stats = render_calls(spt, tuning=tuning)
    assert_wide(stats)
    assert stats[-1].view_split == 1
    assert_same(acc, plain(spt, tuning=tuning)[0], "wide, split vs no view cache")
    assert_same(acc, oracle(spt, ref, W, H, sum(CALLS), BOUNCES, 0), "wide, split vs the oracle")


def test_wide_counters(spt, ref):
    """The counting form: the same image, segments and radiance updates as the narrow counting kernel."""
    acc, stats = render_calls(spt, tuning=WIDE, counters=True)
    assert_wide(stats)
    pacc, pstats = plain(spt, tuning=WIDE, counters=True)
    assert_same(acc, pacc, "wide counters vs no view cache")
    assert_same(acc, oracle(spt, ref, W, H, sum(CALLS), BOUNCES, 0), "wide counters vs the oracle")
    assert list(stats[-1].segments) == list(pstats[-1].segments)
    assert list(stats[-1].radiance_updates) == list(pstats[-1].radiance_updates)


def test_wide_counters_specialized(spt):
    """The counting wide form compiled for the shape (Cornell has wall pairs): it runs, with the generic one's bits.
    Cornell 64x48, 8 frames in two calls (the second runs over the view's lists)."""
    w, h, calls = 64, 48, (4, 4)
    acc, stats = render_calls(spt, calls=calls, w=w, h=h, tuning=dict(WIDE, specialize=1), counters=True)
    assert_wide(stats)
    assert stats[-1].specialized == 1
    gen, gstats = render_calls(spt, calls=calls, w=w, h=h, tuning=dict(WIDE, specialize=-1), counters=True)
    assert_wide(gstats)
    assert gstats[-1].specialized == 0
    assert_same(acc, gen, "wide counters: specialized vs generic")
    assert list(stats[-1].segments) == list(gstats[-1].segments)


def test_wide_fewer_than_64_live(spt, ref):
    """A view whose whole live list is shorter than one wide chunk: the wide kernel runs its small tiers only."""
    w, h = 11, 7
    acc, stats = render_calls(spt, w=w, h=h, tuning=WIDE)
    assert_wide(stats)
    assert 0 < stats[-1].view_live_pixels < 64, stats[-1].view_live_pixels
    assert_same(acc, plain(spt, w=w, h=h, tuning=WIDE)[0], "wide, < 64 live vs no view cache")
    assert_same(acc, oracle(spt, ref, w, h, sum(CALLS), BOUNCES, 0), "wide, < 64 live vs the oracle")


def test_wide_camera_outside_the_box(spt):
    """A posed camera beside the box, looking at it from outside: another live list, sky on both sides."""
    cam = spt.look_at((3.5, 1.0, 0.5), (0.0, 0.0, 5.5), vfov=55.0)
    acc, stats = render_calls(spt, tuning=WIDE, camera=cam)
    assert_wide(stats)
    assert 64 < stats[-1].view_live_pixels < W * H, stats[-1].view_live_pixels
    assert_same(acc, plain(spt, tuning=WIDE, camera=cam)[0], "wide, camera outside vs no view cache")


def test_wide_more_than_512_frames(spt, ref):
    """One call of 600 frames: wide launches take at most 512 (the ring's done byte holds the slot's lap, 128
    at most), so the call runs two, and a 64-pixel chunk of the first reaches lap 128."""
    w, h, calls = 24, 16, (5, 600)
    acc, stats = render_calls(spt, calls=calls, w=w, h=h, tuning=WIDE)
    assert_wide(stats)
    assert stats[-1].view_live_pixels >= 100, "at least one 64-pixel chunk in the first tier"
    assert_same(acc, plain(spt, calls=calls, w=w, h=h, tuning=WIDE)[0], "wide, 600 frames vs no view cache")
    assert_same(acc, oracle(spt, ref, w, h, sum(calls), BOUNCES, 0), "wide, 600 frames vs the oracle")


def test_wide_never(spt, ref):
    tuning = {"wide_chunks": -1}
    acc, stats = render_calls(spt, tuning=tuning)
    assert_wide(stats, on=False)
    assert_same(acc, oracle(spt, ref, W, H, sum(CALLS), BOUNCES, 0), "wide_chunks -1 vs the oracle")


def test_wide_automatic_is_off_at_this_size(spt):
    _, stats = render_calls(spt)
    assert_wide(stats, on=False)


def test_wide_not_for_a_row_shard(spt, ref):
    """Rank 1 of 2 with wide_chunks = 1: a shard keeps its small chunks (not eligible), the same bits as before."""
    acc, stats = render_calls(spt, tuning=WIDE, rank=1, world=2)
    assert_wide(stats, on=False)
    whole = oracle(spt, ref, W, H, sum(CALLS), BOUNCES, 0)
    assert_same(acc, whole[1::2], "shard 1 of 2 vs its rows of the whole image")
    assert_same(acc, plain(spt, tuning=WIDE, rank=1, world=2)[0], "shard 1 of 2 vs no view cache")


def test_wide_not_with_nee(spt, ref):
    acc, stats = render_calls(spt, tuning=WIDE, flags=spt.FLAG_NEE)
    assert_wide(stats, on=False)
    assert_same(acc, plain(spt, tuning=WIDE, flags=spt.FLAG_NEE)[0], "NEE: view cache vs none")
    assert_same(acc, oracle(spt, ref, W, H, sum(CALLS), BOUNCES, ref.FLAG_NEE), "NEE vs the oracle")


def test_tuning_range(spt):
    with spt.Context(0) as ctx:
        with pytest.raises(Exception):
            ctx.set_tuning(wide_chunks=2)
        ctx.set_tuning(wide_chunks=1)
