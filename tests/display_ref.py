"""The luminance meter, the exposure from its histogram and the display transform, restated in numpy from the
text of include/spt.h ("exposure and tone mapping") alone: the checker of tests/test_display_host.py, which ties
the library's host functions to it bit for bit. Nothing here calls the library.

fp32 values stay np.float32 throughout, one numpy operation per stated operation (numpy rounds each once and
never contracts a multiply with an add); the exposure runs in float64 in the stated order."""
import numpy as np

F = np.float32
BINS = 256
KEY_BASE = 888
CLAMP, REINHARD, ACES = 0, 1, 2


def pixels(rgba):
    return np.ascontiguousarray(rgba, dtype=F).reshape(-1, 4)


def luminance(rgba, divisor=1.0):
    p, f = pixels(rgba), F(divisor)
    with np.errstate(all="ignore"):
        r, g, b = p[:, 0] / f, p[:, 1] / f, p[:, 2] / f
        return (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b


def meter_bin(lum):
    lum = np.ascontiguousarray(lum, dtype=F)
    with np.errstate(invalid="ignore"):
        positive = lum > 0
    key = np.where(positive, lum.view(np.uint32) >> 20, 0).astype(np.int64)
    return np.minimum(np.maximum(key, KEY_BASE) - KEY_BASE, BINS - 1)


def histogram(rgba, divisor=1.0):
    return np.bincount(meter_bin(luminance(rgba, divisor)), minlength=BINS).astype(np.uint32)


def bin_centre(b):
    """log2 of the centre of bin b (1..255)."""
    key = KEY_BASE + int(b)
    e, k = (key >> 3) - 127, key & 7
    return np.float64(e) + np.log2(np.float64(1.0) + (np.float64(k) + 0.5) / 8.0)


def exposure(counts, target=0.18, low=0.1, high=0.02, lo_limit=0.015625, hi_limit=64.0):
    """Steps 1-5; the parameters are taken as the floats the struct holds."""
    target, low, high, lo_limit, hi_limit = (np.float64(F(v)) for v in (target, low, high, lo_limit, hi_limit))
    counts = np.asarray(counts, dtype=np.uint32)
    n = np.float64(int(counts[1:].astype(np.uint64).sum()))
    if n == 0:
        return F(1.0)
    lo, hi = low * n, (np.float64(1.0) - high) * n
    c0 = sw = sl = np.float64(0.0)
    for b in range(1, BINS):
        c1 = c0 + np.float64(counts[b])
        w = max(np.float64(0.0), min(c1, hi) - max(c0, lo))
        sw = sw + w
        sl = sl + w * bin_centre(b)
        c0 = c1
    x = target / np.exp2(sl / sw)
    return F(min(max(x, lo_limit), hi_limit))


def unit_u8(c):
    """clamp to [0, 1], NaN becomes 0, (uint8)(c * 255.0f)"""
    with np.errstate(invalid="ignore"):
        c = np.where(c < 0, F(0), np.where(F(1) < c, F(1), c)).astype(F)
        c = np.where(c != c, F(0), c).astype(F)
        return (c * F(255)).astype(np.uint8).astype(np.uint32)


def display(rgba, tonemap, exposure_value=1.0, divisor=1.0):
    p, f, ex = pixels(rgba), F(divisor), F(exposure_value)
    with np.errstate(all="ignore"):
        x = (p[:, :3] / f) * ex
        if tonemap == CLAMP:
            rgb = unit_u8(x)
        else:
            x = np.where(x > 0, np.minimum(x, F(65536.0)), F(0)).astype(F)
            if tonemap == REINHARD:
                y = x / (F(1) + x)
            else:
                y = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
            assert y.dtype == F
            rgb = unit_u8(y)
        a = unit_u8(p[:, 3] / f)
    return (rgb[:, 0] << 24) | (rgb[:, 1] << 16) | (rgb[:, 2] << 8) | a


def resolve_rgba8(rgba, frames, exposure_value=1.0):
    """The plain resolve as csrc/spt_kernels.hip states it (to_u8 and rgba8), written from that text: what
    SPT_TONEMAP_CLAMP has to equal."""
    p, f, ex = pixels(rgba), F(frames), F(exposure_value)

    def to_u8(v, with_exposure):
        with np.errstate(all="ignore"):
            c = v / f
            if with_exposure:
                c = c * ex
            c = np.where(c < 0, F(0), np.where(F(1) < c, F(1), c)).astype(F)
            c = np.where(np.isnan(c), F(0), c).astype(F)
            return (c * F(255)).astype(np.uint8).astype(np.uint32)

    return (to_u8(p[:, 0], True) << 24) | (to_u8(p[:, 1], True) << 16) | (to_u8(p[:, 2], True) << 8) | to_u8(p[:, 3], False)


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------
def key_boundaries():
    """Every key boundary of the float format (bits = key << 20, key 0..4095 with the sign bit) with its two
    neighbours in bit order, as float32."""
    keys = np.arange(4096, dtype=np.uint64) << 20
    bits = np.stack([keys - 1, keys, keys + 1], axis=1).reshape(-1) & 0xFFFFFFFF
    return bits.astype(np.uint32).view(F)


def special_values():
    bits = np.array([0x00000000, 0x80000000, 0xBF800000, 0xFF7FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001,
                     0x7F800000, 0xFF800000, 0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x00800000, 0x7F7FFFFF],
                    dtype=np.uint32)
    return bits.view(F)


def random_bits(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(F)


def random_image(n, seed):
    """n RGBA pixels, log-uniform over the meter's range and beyond on both sides, some of them black."""
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-20.0, 18.0, size=(n, 4))).astype(F)
    img[rng.random(n) < 0.1, :3] = 0
    return img


def grey(values):
    """One RGBA pixel per value: (v, v, v, 1)."""
    v = np.ascontiguousarray(values, dtype=F).reshape(-1)
    return np.stack([v, v, v, np.ones_like(v)], axis=1)
