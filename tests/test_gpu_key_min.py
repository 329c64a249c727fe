"""The flat closest hit's key minimum where ties decide the image, bit for bit, in every flat form.

closest_flat keeps the running closest hit as a key, (t bits << 32) | original index, so that equal t go to the lower
original index. The wide ranged k_paths and k_frame take the keys' minimum as one v_min_f64 (spt_device.h key_min);
the other specialized k_paths forms keep the integer compare. Every case waits for the shape-specialized kernels, asserts the form that ran, and compares the
accumulation as uint32 with the generic kernels (spt_tuning.specialize = -1) and with the oracle.

64x48, 8 bounces, RR depth 2, two calls of 8 frames continuing one accumulation (k_frame: the same 16 frames in calls
of 3, 3 and 2, twice). The forms:
  wide, wide-split   wide_chunks = 1, the halves on one stream or two (the benchmark's form)
  narrow             wide_chunks = -1 with 32-pixel chunks: the pixel-lane kernel
  shard              rank 3 of 8 by rows under the automatic plan: the channel-lane kernel
  nee                SPT_FLAG_NEE: the inline shadow rays' searches start from (smax, kMiss)
  frame              calls below four frames: k_frame
The scenes are the Cornell box, with an exact duplicate of the left wall or of a sphere under another material at a
lower or at a higher original index than its twin (every hit on either is a tie on t: the lower index's albedo must
show), and the box seen by a camera whose middle row of primary rays runs into the floor / back-wall edge (the two
walls' t have the same bits there). test_oracle_sees_the_index_order (no GPU) checks that the oracle's images of
the two index orders differ: the tie is exercised.
"""
import numpy as np
import pytest

from brute_ref import render as camera_render

gpu = pytest.mark.gpu

W, H, BOUNCES, RR = 64, 48, 8, 2
FRAMES = 16
WHITE, RED, GREEN, LIGHT = 0, 1, 2, 3  # scenes.cpp cornell_walls' materials
LEFT_WALL, SPHERE_A = 3, 6  # its quads: floor, ceiling, back, left, right, light; then the two spheres
RANK, WORLD = 3, 8
FORMS = {
    "wide": dict(tuning={"wide_chunks": 1, "split_streams": -1}, wide=1, split=0),
    "wide-split": dict(tuning={"wide_chunks": 1, "split_streams": 1}, wide=1, split=1),
    "narrow": dict(tuning={"wide_chunks": -1, "px_shift": 5}, wide=0),
    "shard": dict(tuning={}, wide=0, rank=RANK, world=WORLD),
    "nee": dict(tuning={}, nee=True),
    "frame": dict(tuning={}, calls=(3, 3, 2, 3, 3, 2), frame=True),
}
SCENES = ["cornell", "wall_twin_low", "wall_twin_high", "sphere_twin_low", "sphere_twin_high", "edge_camera"]
# (the eye 4.5 above the floor and 4.5 in front of the back wall, looking at the middle of their edge)
EDGE_EYE, EDGE_TARGET, EDGE_VFOV = (0.0, 2.0, 3.5), (0.0, -2.5, 8.0), 70.0

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
    """(prims, mats, env, camera or None)"""
    prims, mats, env = spt.build_scene("cornell")
    prims, cam = prims.copy(), None
    if name.startswith(("wall_twin", "sphere_twin")):
        twin = prims[LEFT_WALL if name.startswith("wall") else SPHERE_A].copy()
        twin["material"] = GREEN if name.startswith("wall") else RED
        twin = np.array([twin], dtype=prims.dtype)
        prims = np.concatenate([twin, prims] if name.endswith("low") else [prims, twin])
    elif name == "edge_camera":
        cam = spt.look_at(EDGE_EYE, EDGE_TARGET, vfov=EDGE_VFOV)
    else:
        assert name == "cornell", name
    return prims, mats, env, cam


def oracle(spt, ref, name, flags=0):
    """The whole image after FRAMES frames, computed once per scene and flags, read only; a shard takes its rows."""
    if (name, flags) not in _oracle:
        prims, mats, env, cam = scene(spt, name)
        rs = ref.RefScene(prims, mats, env, brute=True)
        if cam is None:
            acc = rs.render(W, H, 0, FRAMES, BOUNCES, RR, flags)
        else:
            acc = camera_render(spt, ref, rs, W, H, cam, FRAMES, BOUNCES, RR, flags)
        acc.setflags(write=False)
        _oracle[name, flags] = acc
    return _oracle[name, flags]


def render(spt, name, form, specialize=1):
    """A fresh ctx; the form's calls continuing one accumulation. Returns (accumulation, stats after the last call)."""
    f = FORMS[form]
    prims, mats, env, cam = scene(spt, name)
    with spt.Context(0) as ctx:
        ctx.set_tuning(specialize=specialize, **f["tuning"])
        ctx.set_scene(prims, mats, env)
        ctx.configure(W, H, BOUNCES, RR, spt.FLAG_NEE if f.get("nee") else 0, f.get("rank", 0), f.get("world", 1), 0)
        if cam is not None:
            ctx.set_camera(cam)
        ctx.specialize_scene()
        first = 0
        for n in f.get("calls", (8, 8)):
            ctx.render(first, n)
            first += n
        assert first == FRAMES
        return ctx.read_accum(), ctx.stats()


def check_stats(spt, st, form, specialized):
    f = FORMS[form]
    assert st.schedule == (spt.SCHEDULE_FRAME if f.get("frame") else spt.SCHEDULE_PERSISTENT)
    assert st.specialized == (1 if specialized else 0)
    if "wide" in f:
        assert st.view_cached == 1 and st.view_wide == f["wide"]
    if specialized and f.get("wide"):
        assert st.flat_ranges == 1, "the wide kernel ran without the range bit: not the form with key_min"
    if "split" in f:
        assert st.view_split == f["split"]


def generic(spt, name, form):
    if (name, form) not in _generic:
        acc, st = render(spt, name, form, specialize=-1)
        check_stats(spt, st, form, False)
        acc.setflags(write=False)
        _generic[name, form] = acc
    return _generic[name, form]


def test_oracle_sees_the_index_order(spt, ref):
    """No GPU. The oracle's images of a twin at the lower and at the higher index differ (so the tie decides
    pixels), the brute-force oracle agrees with the default one, and the edge camera's middle row of rays has
    d.y = -d.z, which with the eye's equal distances gives the floor and the back wall the same t bits."""
    for kind in ("wall", "sphere"):
        low, high = oracle(spt, ref, f"{kind}_twin_low"), oracle(spt, ref, f"{kind}_twin_high")
        differ = int(np.count_nonzero(np.any(bits(low) != bits(high), axis=1)))
        print(f"{kind} twin: {differ} of {W * H} pixels differ between the two index orders")
        assert differ > W * H // 50
        # the twin at the higher index never shows: the image is the plain box's
        assert_same(high, oracle(spt, ref, "cornell"), f"{kind} twin at the higher index against the plain box")
        prims, mats, env, _ = scene(spt, f"{kind}_twin_low")
        assert_same(ref.RefScene(prims, mats, env).render(W, H, 0, FRAMES, BOUNCES, RR, 0), low,
                    f"{kind} twin at the lower index: the default oracle against the brute-force one")
    prims, mats, env, cam = scene(spt, "edge_camera")
    rs = ref.RefScene(prims, mats, env, brute=True)
    ties = 0
    for x in range(W):
        o, d = spt.camera_ray(cam, W, H, x, H // 2)
        assert d[1] == -d[2] and d[1] < 0.0, (x, d)
        t_floor, t_back = np.float32(-2.5 - o[1]) / d[1], np.float32(8.0 - o[2]) / d[2]
        assert t_floor == t_back
        hit = rs.intersect(o, d)
        if hit is not None and np.float32(hit[0]) == t_floor:
            assert hit[1] == 0, "equal t: the floor (index 0) before the back wall (index 2)"
            ties += 1
    print(f"edge camera: {ties} of {W} rays of the middle row hit the edge at the two walls' common t")
    assert ties > W // 4


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", SCENES)
def test_scene(spt, ref, name, form):
    acc, st = render(spt, name, form)
    check_stats(spt, st, form, True)
    assert_same(acc, generic(spt, name, form), f"{name}, {form}: specialized against generic")
    want = oracle(spt, ref, name, spt.FLAG_NEE if FORMS[form].get("nee") else 0)
    if "world" in FORMS[form]:
        want = want[RANK::WORLD]
    assert_same(acc, want, f"{name}, {form}: specialized against the oracle")
