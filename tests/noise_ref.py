"""The noise estimate of include/spt.h ("noise estimate") restated in numpy, from the header's text: the checker of
tests/test_noise_host.py (against the library's host functions) and, through those, of tests/test_gpu_noise.py.

Every step is one fp32 numpy operation on arrays, so each `+ - * /` rounds once, as the definition says; nothing
here shares code with csrc/spt_noise.h."""
import math

import numpy as np

F = np.float32
BINS = 256
KEY_BASE = 792  # the key (bits >> 20) of 2^-28
MAX_FRAMES = 2.0 ** 24


def luminance(accum):
    a = np.asarray(accum, dtype=F)
    return (F(0.2126) * a[..., 0] + F(0.7152) * a[..., 1]) + F(0.0722) * a[..., 2]


def update(accum, batch_frames, frames_before, moments=None):
    """The moments after a batch of batch_frames frames on top of frames_before; the first batch (frames_before
    0) starts from a zeroed state."""
    a = np.asarray(accum, dtype=F)
    m = np.zeros_like(a) if frames_before == 0 else np.asarray(moments, dtype=F)
    w = F(batch_frames)
    wn = F(frames_before) + w
    r = w / wn
    with np.errstate(all="ignore"):
        L = luminance(a)
        d = (L - m[..., 2]) / w
        delta = d - m[..., 0]
        mean = m[..., 0] + r * delta
        m2 = m[..., 1] + (w * delta) * (d - mean)
    return np.stack([mean, m2, L, np.zeros_like(L)], axis=-1).astype(F)


def pooled(moments, radius):
    """(s_mean, s_m2) of a (height, width, 4) image: the window's in-image taps summed from 0.0f, rows outer and
    columns inner, then divided by their number."""
    m = np.asarray(moments, dtype=F)
    if radius == 0:
        return m[..., 0].copy(), m[..., 1].copy()
    h, w = m.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    s_mean, s_m2 = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
    count = np.zeros((h, w), dtype=np.int64)
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                ty, tx = ys + dy, xs + dx
                inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                cy, cx = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
                # (a tap outside the image adds nothing: the sum it would have joined is kept as it is)
                s_mean = np.where(inside, s_mean + m[cy, cx, 0], s_mean)
                s_m2 = np.where(inside, s_m2 + m[cy, cx, 1], s_m2)
                count += inside
        n = count.astype(F)
        return s_mean / n, s_m2 / n


def e2_image(moments, batches, frames, radius=1, dark_floor=0.01):
    assert batches >= 2
    inv = F(1.0) / (F(batches - 1) * F(frames))
    s_mean, s_m2 = pooled(moments, radius)
    with np.errstate(all="ignore"):
        v = s_m2 * inv
        t = s_mean + F(dark_floor)
        return (v / (t * t)).astype(F)


def noise_bin(e2):
    e = np.asarray(e2, dtype=F)
    key = (e.view(np.uint32) >> 20).astype(np.int64)
    with np.errstate(invalid="ignore"):
        b = np.where(e > 0, np.minimum(np.maximum(key, KEY_BASE) - KEY_BASE, BINS - 1), 0)
    return np.where(np.isnan(e), BINS - 1, b)


def histogram(e2):
    return np.bincount(noise_bin(e2).reshape(-1), minlength=BINS).astype(np.uint32)


def bin_lower_edge(b):
    """The least float of bin b (1..255): bits (792 + b) << 20."""
    return np.array([(KEY_BASE + b) << 20], dtype=np.uint32).view(F)[0]


def from_histogram(counts, quantile=0.95):
    """The stop rule, in double."""
    total = int(np.sum(np.asarray(counts, dtype=np.uint64)))
    if total == 0:
        return 0.0
    need = float(quantile) * float(total)
    cum = 0
    for b in range(BINS):
        cum += int(counts[b])
        if float(cum) >= need:
            break
    if b == 0:
        return 0.0
    if b == BINS - 1:
        return math.inf
    return math.sqrt(float(bin_lower_edge(b + 1)))


def fold(accums, frame_counts):
    """The moments after folding a sequence of accumulations taken at frame_counts (rising): (moments, B, W)."""
    m, before = None, 0
    for a, fc in zip(accums, frame_counts):
        m = update(a, fc - before, before, m)
        before = fc
    return m, len(frame_counts), float(before)


def quality_ratio(e2, mean, truth, dark_floor=0.01, least=1.0e-3):
    """R: the actual relative RMS error of each pixel's mean luminance (against `truth`, a long render's mean,
    relative to truth + dark_floor) over the estimated one (sqrt(e2), per pixel or pooled), both taken over the
    pixels whose estimate exceeds `least`; in double."""
    est = np.sqrt(np.maximum(np.asarray(e2, dtype=np.float64), 0.0))
    t = np.asarray(truth, dtype=np.float64)
    rel = (np.asarray(mean, dtype=np.float64) - t) / (t + dark_floor)
    sel = est > least
    return float(np.sqrt(np.mean(rel[sel] ** 2)) / np.sqrt(np.mean(est[sel] ** 2)))
