"""Expected images from the oracle in either of its closest-hit modes (tests/test_oracle_brute.py,
tests/test_gpu_bvh_brute.py): RefScene(brute=True) tests every primitive in index order and keeps the
smallest t, the lowest index on a tie; RefScene() walks the oracle's own BVH above 64 primitives.
Test infrastructure only.

With a camera the image is test_gpu_camera.frame_radiance's composition: the seed (ref_rng_seed), the ray
from spt_camera_ray (the host build of the function the kernels compile), ref_trace_ray from that ray and
RNG state, float32 adds into RGBA in frame order. Without one it is ref_render itself.
"""
import ctypes

import numpy as np

F = np.float32
MISS = 0xFFFFFFFF


def frame_radiance(spt, ref, rs, w, h, cam, frames, bounces=4, rr=2, flags=0, rect=None):
    """[frames, rows, cols, 4] float32: trace_ray's (L, 1) of every pixel of the rectangle `rect` of the w x h
    image, for frames 0 .. frames - 1, through `cam` (None: the reference's camera, ref_render frame by frame)."""
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, w, h)
    img = np.zeros((frames, y1 - y0, x1 - x0, 4), dtype=F)
    if cam is None:
        for f in range(frames):
            img[f] = rs.render(w, h, f, 1, bounces, rr, flags, rect=rect)
        return img
    lib, slib = ref.load(), spt.load_library()
    cfg = ref.RefConfig(w, h, bounces, rr, flags)
    f3 = ctypes.c_float * 3
    o, d, out = f3(), f3(), (ctypes.c_float * 4)()
    state = ctypes.c_uint32()
    for y in range(y0, y1):
        for x in range(x0, x1):
            assert slib.spt_camera_ray(ctypes.byref(cam), w, h, x, y, 0.0, 0.0, o, d) == 0
            for f in range(frames):
                state.value = lib.ref_rng_seed(x, y, w, f + 1)
                lib.ref_trace_ray(rs.h, ctypes.byref(cfg), o, d, ctypes.byref(state), out)
                img[f, y - y0, x - x0] = out[:]
    return img


def accumulate(frames, first, n):
    """The accumulation buffer after frames [first, first + n), added in frame order in float32."""
    acc = np.zeros(frames.shape[1:], dtype=F)
    for f in range(first, first + n):
        acc = acc + frames[f]
    return acc


def render(spt, ref, rs, w, h, cam, frames, bounces=4, rr=2, flags=0, rect=None):
    """The accumulation buffer [rows, cols, 4] float32 after frames 0 .. frames - 1."""
    return accumulate(frame_radiance(spt, ref, rs, w, h, cam, frames, bounces, rr, flags, rect), 0, frames)


def first_hits(spt, ref, rs, w, h, cam, rect=None):
    """(t [rows, cols] float32, +inf for a miss; prim [rows, cols] uint32, MISS for a miss) of the pixels'
    corner rays, from rs.intersect (tmin 0.001)."""
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, w, h)
    t = np.full((y1 - y0, x1 - x0), np.inf, dtype=F)
    k = np.full((y1 - y0, x1 - x0), MISS, dtype=np.uint32)
    for y in range(y0, y1):
        for x in range(x0, x1):
            o, d = (np.zeros(3, dtype=F), ref.primary_dir(x, y, w, h)) if cam is None else spt.camera_ray(cam, w, h, x, y)
            got = rs.intersect(o, d)
            if got is not None:
                t[y - y0, x - x0], k[y - y0, x - x0] = got[0], got[1]
    return t, k


def bits(a):
    return np.ascontiguousarray(a, dtype=F).reshape(-1, a.shape[-1] if a.ndim > 1 else 1).view(np.uint32)


def assert_same(got, want, what):
    """Bit for bit, every pixel."""
    g, r = bits(np.asarray(got)), bits(np.asarray(want))
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bad = np.flatnonzero(np.any(g != r, axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} pixels differ, first {bad[:5].tolist()}"
