"""The checker of the variance-guided a-trous denoiser (tests/test_guided_host.py, tests/test_gpu_guided.py): a
numpy restatement of include/spt.h's definition ("variance-guided denoiser") — float32 arrays, one elementwise
operation per arithmetic step, written from that text and not from the product's code. Test infrastructure only.
"""
import numpy as np

F = np.float32
MISS = 0xFFFFFFFF
H5 = [F(1.0 / 16.0), F(1.0 / 4.0), F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0)]
G3 = [F(0.25), F(0.5), F(0.25)]
DEFAULTS = {"levels": 5, "sigma_variance": 4.0, "sigma_plane": 0.05, "normal_power_log2": 5, "variance_floor": 1e-8,
            "prefilter": 1}


def lum(c):
    """Linear luminance of an (..., >=3) float32 array."""
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def variance0(moments, batches, frame_count):
    """v0 = fmaxf(m2 * inv, 0) of (h, w, 4) moments."""
    assert batches >= 2 and frame_count >= 1
    inv = F(1.0) / (F(batches - 1) * F(frame_count))
    m = np.asarray(moments, dtype=F)
    with np.errstate(all="ignore"):
        return np.fmax(m[..., 1] * inv, F(0.0)).astype(F)


def prefilter(v0):
    """The 3 x 3 binomial of the in-image taps, rows outer and columns inner, both sums from 0.0f."""
    h, w = v0.shape
    ys, xs = np.mgrid[0:h, 0:w]
    s, sg = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
    with np.errstate(all="ignore"):
        for j in range(3):
            for i in range(3):
                ty, tx = ys + (j - 1), xs + (i - 1)
                inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                cy, cx = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
                g = G3[j] * G3[i]
                prod = g * v0[cy, cx]
                # (a tap outside the image adds nothing: the sums it would have joined are kept as they are)
                s = np.where(inside, s + prod, s)
                sg = np.where(inside, sg + g, sg)
        return (s / sg).astype(F)


def guided_level(c, v, feat_a, feat_b, level, sigma_variance, sigma_plane, normal_power_log2, variance_floor):
    """One pass at step 1 << level over (h, w, 4) colour and (h, w) variance: (colour, variance)."""
    h, w, _ = c.shape
    s = 1 << level
    s2 = F(sigma_variance) * F(sigma_variance)
    inv_z = F(1.0) / (F(sigma_plane) * F(s))
    mat = np.ascontiguousarray(feat_a[..., 3]).view(np.uint32)
    P, N = feat_a[..., :3], feat_b[..., :3]
    L = lum(c)
    iv = F(1.0) / (s2 * v + F(variance_floor))
    acc = np.zeros((h, w, 3), dtype=F)
    acc_w = np.zeros((h, w), dtype=F)
    acc_v = np.zeros((h, w), dtype=F)
    for j in range(5):
        dy = (j - 2) * s
        for i in range(5):
            dx = (i - 2) * s
            # the pixels p whose tap q = p + (dx, dy) is inside the image
            y0, y1 = max(0, -dy), min(h, h - dy)
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            p = (slice(y0, y1), slice(x0, x1))
            q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            dl = L[q] - L[p]
            x2 = (dl * dl) * iv[p]
            r = F(1.0) / (F(1.0) + x2)
            wc = (H5[j] * H5[i]) * (r * r)
            dn = np.fmax(dot(N[p], N[q]), F(0.0))
            for _ in range(normal_power_log2):
                dn = dn * dn
            e = P[q] - P[p]
            pd = dot(N[p], e) * inv_z
            rz = F(1.0) / (F(1.0) + pd * pd)
            geo = dn * (rz * rz)
            wt = wc * geo
            wt = np.where(mat[q] == mat[p], wt, F(0.0))
            for ch in range(3):
                prod = wt * c[q][..., ch]
                acc[p][..., ch] = acc[p][..., ch] + prod
            acc_w[p] = acc_w[p] + wt
            acc_v[p] = acc_v[p] + (wt * wt) * v[q]
    out = c.copy()
    hit = mat != MISS
    for ch in range(3):
        out[..., ch] = np.where(hit, acc[..., ch] / acc_w, c[..., ch])
    out_v = np.where(hit, acc_v / (acc_w * acc_w), v).astype(F)
    return out, out_v


def guided(c, moments, feat_a, feat_b, batches, frame_count, **kw):
    """The whole filter: (colour (h, w, 4), variance (h, w))."""
    p = {**DEFAULTS, **kw}
    c = np.ascontiguousarray(c, dtype=F)
    feat_a = np.ascontiguousarray(feat_a, dtype=F)
    feat_b = np.ascontiguousarray(feat_b, dtype=F)
    v = variance0(moments, batches, frame_count)
    if p["prefilter"]:
        v = prefilter(v)
    with np.errstate(all="ignore"):  # (a missed pixel's sums are computed and discarded)
        for level in range(p["levels"]):
            c, v = guided_level(c, v, feat_a, feat_b, level, p["sigma_variance"], p["sigma_plane"],
                                p["normal_power_log2"], p["variance_floor"])
    return c, v


def rms(img, truth):
    """RMS error over RGB and pixels."""
    d = img[..., :3].astype(np.float64) - truth[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=F).view(np.uint32),
                          np.ascontiguousarray(b, dtype=F).view(np.uint32))
