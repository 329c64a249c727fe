"""Split k_paths launches (spt_tuning.split_streams): a view's lists in two halves on two streams, bit for bit.

Once a flat scene's view lists are built (behind the first persistent call), every k_paths launch runs as
two, over the two halves of the lists, on two streams of the ctx's own; nothing orders the halves against
each other, each pixel's frames stay in order on its half's stream, and the ctx stream waits on both halves
before spt_render returns. Every case runs the same calls with the knob forced on (1) and off (-1), asserts
that the last persistent launch was split / was not (spt_stats.view_split), and compares the accumulation as
uint32 between the two and with the oracle. 96x64, 8 bounces, 8 frames per call, as the wall-pair tests.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """test_stream_contract takes a stream and a tensor from torch, whose copy of the HIP runtime finds the GPU
    only if it looks before the library's copy has opened it (as in bench.py, which sets torch's device first):
    so torch looks before this module's first ctx."""
    torch.cuda.is_available()


W, H, BOUNCES, RR, FRAMES = 96, 64, 8, 2, 8
LEFT_WALL = 3  # scenes.cpp cornell_walls: floor, ceiling, back, left, right, light; then the two spheres


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def assert_same(got, want, what):
    g, r = bits(got), bits(want)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bad = np.flatnonzero(np.any(g != r, axis=1))
    print(f"{what}: {bad.size} of {g.shape[0]} pixels differ")
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} pixels differ, first {bad[:5]}"


def run(spt, split, script, scene="cornell", flags=0, cam=None, rank=0, world=1, w=W, h=H, specialize=-1,
        profiling=False):
    """A fresh ctx with the knob forced to `split`; script(ctx) makes the calls and returns what it read (or
    None: the accumulation is read here). Returns (image, stats after the script)."""
    prims, mats, env = spt.build_scene(scene) if isinstance(scene, str) else scene
    with spt.Context(0) as ctx:
        ctx.set_tuning(specialize=specialize, split_streams=split)
        ctx.set_scene(prims, mats, env)
        ctx.configure(w, h, BOUNCES, RR, flags, rank, world)
        if cam is not None:
            ctx.set_camera(cam)
        ctx.specialize_scene()
        if profiling:
            ctx.set_profiling(True)
        out = script(ctx)
        st = ctx.stats()
        return (ctx.read_accum() if out is None else out), st


def both(spt, script, last_split=1, knob=1, **kw):
    """script with the knob on (or `knob`) and off: the same bits, view_split as forced. Returns (image, stats on,
    stats off)."""
    on, st_on = run(spt, knob, script, **kw)
    off, st_off = run(spt, -1, script, **kw)
    assert st_on.schedule == st_off.schedule
    assert st_on.view_split == last_split, "the last persistent launch was not split with split_streams = 1"
    assert st_off.view_split == 0, "a launch was split with split_streams = -1"
    assert st_on.frames == st_off.frames and st_on.paths == st_off.paths
    assert st_on.persistent_launches == st_off.persistent_launches
    assert_same(on, off, "split against unsplit")
    return on, st_on, st_off


def three_calls(ctx):
    for k in range(3):  # nothing between them: the second split launch forks without a wait
        ctx.render(k * FRAMES, FRAMES)


_oracle = {}


def oracle(spt, ref, frames, scene="cornell", flags=0, **kw):
    """Frames [0, frames) of the 96x64 image by the oracle; the named scene's images are computed once."""
    key = (scene, frames, flags, repr(sorted(kw.items()))) if isinstance(scene, str) else None
    if key in _oracle:
        return _oracle[key]
    prims, mats, env = spt.build_scene(scene) if isinstance(scene, str) else scene
    acc = ref.RefScene(prims, mats, env).render(W, H, 0, frames, BOUNCES, RR, flags, **kw)
    acc.setflags(write=False)
    if key is not None:
        _oracle[key] = acc
    return acc


def test_three_consecutive_calls(spt, ref):
    """The recording launch of each half, the ordered launches, progressive frames; the specialized kernels
    (the benchmark's launch path), with per-launch events: a split call counts as one persistent launch."""
    img, st_on, st_off = both(spt, three_calls, specialize=1, profiling=True)
    assert st_on.specialized == 1 and st_on.schedule == spt.SCHEDULE_PERSISTENT
    assert st_on.persistent_launches == 3 and st_on.view_cached == 1
    assert st_on.persistent_ms > 0.0
    assert_same(img, oracle(spt, ref, 3 * FRAMES), "three split calls against the oracle")


def test_three_calls_generic_kernels(spt, ref):
    img, st_on, _ = both(spt, three_calls)
    assert st_on.specialized == 0
    assert_same(img, oracle(spt, ref, 3 * FRAMES), "three split calls (generic kernels) against the oracle")


def test_render_render_read(spt, ref):
    def script(ctx):
        ctx.render(0, FRAMES)
        ctx.render(FRAMES, FRAMES)
        return ctx.read_accum()  # (on the ctx stream, behind the join)
    img, _, _ = both(spt, script)
    assert_same(img, oracle(spt, ref, 2 * FRAMES), "render, render, read_accum")


def test_reset_between_renders(spt, ref):
    def script(ctx):
        ctx.render(0, FRAMES)
        ctx.render(FRAMES, FRAMES)  # split
        ctx.reset()                 # (zeroes the sums on the ctx stream: the next split launch forks behind it)
        ctx.render(0, FRAMES)       # split: the view's lists are kept
    img, _, _ = both(spt, script)
    assert_same(img, oracle(spt, ref, FRAMES), "render, reset, render")


def test_one_frame_call_between_renders(spt, ref):
    def script(ctx):
        ctx.render(0, FRAMES)
        ctx.render(FRAMES, FRAMES)          # split
        ctx.render(2 * FRAMES, 1)           # k_frame, on the ctx stream behind the join
        ctx.render(2 * FRAMES + 1, FRAMES)  # split again, forked behind k_frame
    img, st_on, _ = both(spt, script)
    assert st_on.schedule == spt.SCHEDULE_PERSISTENT
    assert_same(img, oracle(spt, ref, 3 * FRAMES + 1), "render, one-frame call, render")


def test_update_prims_between_renders(spt, ref):
    """An edit between split renders: the fork waits for it, the view is rebuilt (by an unsplit launch), and the
    launches after that are split over the new lists."""
    prims, mats, env = spt.build_scene("cornell")
    moved = prims.copy()
    moved[LEFT_WALL]["p0"][0] = 4.0  # the left wall to the right of the right one

    def script(ctx):
        ctx.render(0, FRAMES)
        ctx.render(FRAMES, FRAMES)  # split
        ctx.update_prims([LEFT_WALL], moved[[LEFT_WALL]])  # (resets the accumulation)
        ctx.render(0, FRAMES)       # whole: builds the new view's lists
        ctx.render(FRAMES, FRAMES)  # split over them
    img, _, _ = both(spt, script)
    assert_same(img, oracle(spt, ref, 2 * FRAMES, scene=(moved, mats, env)), "update_prims between split renders")


def test_cornell_nee(spt, ref):
    img, _, _ = both(spt, three_calls, flags=spt.FLAG_NEE)
    assert_same(img, oracle(spt, ref, 3 * FRAMES, flags=spt.FLAG_NEE), "NEE: three split calls against the oracle")


def test_posed_camera(spt, ref):
    """Right of the box, looking into its open front: another view, other lists (4 frames per call)."""
    cam = spt.look_at((4.0, 0.5, -1.0), (0.5, -1.0, 5.5), vfov=60.0)

    def script(ctx):
        ctx.render(0, 4)
        ctx.render(4, 4)
    img, _, _ = both(spt, script, cam=cam)
    # the oracle's pieces behind the camera's rays (spt_camera_ray: the function the kernels compile)
    prims, mats, env = spt.build_scene("cornell")
    rs = ref.RefScene(prims, mats, env)
    lib, slib = ref.load(), spt.load_library()
    cfg = ref.RefConfig(W, H, BOUNCES, RR, 0)
    f3 = ctypes.c_float * 3
    o, d, out = f3(), f3(), (ctypes.c_float * 4)()
    state = ctypes.c_uint32()
    acc = np.zeros((H, W, 4), dtype=np.float32)
    for f in range(8):
        frame = np.zeros((H, W, 4), dtype=np.float32)
        for y in range(H):
            for x in range(W):
                state.value = lib.ref_rng_seed(x, y, W, f + 1)
                assert slib.spt_camera_ray(ctypes.byref(cam), W, H, x, y, 0.0, 0.0, o, d) == 0
                lib.ref_trace_ray(rs.h, ctypes.byref(cfg), o, d, ctypes.byref(state), out)
                frame[y, x] = out[:]
        acc = acc + frame
    assert_same(img, acc, "posed camera: split against the oracle")


def test_rank_1_of_2(spt, ref):
    img, _, _ = both(spt, three_calls, rank=1, world=2)
    assert_same(img, oracle(spt, ref, 3 * FRAMES, row_step=2, row_offset=1), "rank 1 of 2: split against the oracle")


def sky_scene(spt):
    """One small sphere straight ahead under the gradient sky: all but a few pixels are constant."""
    return spt.sphere_prims([(0.0, 0.0, 5.0, 0.4)]), spt.reference_materials(), spt.reference_env(True)


@pytest.mark.parametrize("w,h", [(16, 8), (8, 4)], ids=["16x8", "8x4"])
def test_nearly_all_sky(spt, ref, w, h):
    """Fewer live pixels than half a chunk: half A has no live record (16x8: it keeps one sweep unit of constant
    pixels; 8x4: fewer constant pixels than half a sweep unit too, so half A is empty and is not launched)."""
    scene = sky_scene(spt)
    img, st_on, _ = both(spt, three_calls, scene=scene, w=w, h=h)
    assert 0 < st_on.view_live_pixels < 16, st_on.view_live_pixels
    r = ref.RefScene(*scene).render(w, h, 0, 3 * FRAMES, BOUNCES, RR, 0)
    assert_same(img, r, f"{w}x{h} nearly all sky: split against the oracle")


def test_long_call_is_split_or_whole_as_one(spt, ref):
    """The automatic rule on a call of more than 1024 frames: 1024 frames of 320x180 (22 K live pixels) reach the
    threshold, the remainder of 8 alone would not. Both launches of the call are split — a whole launch for the
    remainder would run on the ctx stream while the halves before it still add to the same pixels."""
    w, h = 320, 180

    def script(ctx):
        ctx.render(0, FRAMES)          # whole: builds the lists; 8 frames are below the threshold anyway
        ctx.render(FRAMES, 1024 + 8)   # two launches, 1024 frames and 8
    img, st_on, _ = both(spt, script, knob=0, w=w, h=h)
    assert 16384 < st_on.view_live_pixels < (1 << 24) // 8
    prims, mats, env = spt.build_scene("cornell")
    r = ref.RefScene(prims, mats, env).render(w, h, 0, FRAMES + 1024 + 8, BOUNCES, RR, 0)
    assert_same(img, r, "a 1032-frame call under the automatic rule against the oracle")


def test_accum_pointer_handed_out(spt, ref):
    """Once spt_accum_device_ptr has handed the sums out, every split launch waits for the ctx stream first
    (the caller may read them there): still split, the same bits."""
    def script(ctx):
        assert ctx.accum_device_ptr()[0] != 0
        three_calls(ctx)
    img, _, _ = both(spt, script)
    assert_same(img, oracle(spt, ref, 3 * FRAMES), "split launches after accum_device_ptr against the oracle")


def test_stream_contract(spt, ref):
    """The caller's contract stays: after spt_render, synchronizing the ctx's stream alone (not the device) is
    enough, and a copy enqueued on that stream sees the finished render. The last two calls are 1024 frames each,
    long enough that a copy not ordered behind them would read unfinished sums."""
    torch.cuda.set_device(0)  # (initializes torch's side: Stream() alone does not)

    def script(ctx):
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            dst = torch.zeros(ctx.shard_pixels * 4, dtype=torch.float32, device="cuda")
        stream.synchronize()
        ctx.render(0, FRAMES)
        ctx.render(FRAMES, 1024)
        ctx.render(FRAMES + 1024, 1024)
        stream.synchronize()  # the ctx's stream only
        ctx.copy_accum_device(dst.data_ptr())
        stream.synchronize()
        out = dst.cpu().numpy().reshape(-1, 4).copy()
        ctx.set_stream(0)  # (back to the ctx's own before the torch stream goes)
        return out
    img, _, _ = both(spt, script)
    assert_same(img, oracle(spt, ref, FRAMES + 2048), "stream contract: copy_accum_device behind a stream synchronize")
