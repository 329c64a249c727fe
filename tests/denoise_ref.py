"""The checker of the first-hit features and the a-trous denoiser (tests/test_denoise_host.py,
tests/test_gpu_denoise.py): a numpy restatement of include/spt.h's definition — float32 arrays, one
elementwise operation per arithmetic step, written from that text and not from the product's code — and
the expected feature images from the oracle's closest hit. Test infrastructure only.
"""
import numpy as np

F = np.float32
MISS = 0xFFFFFFFF
H5 = [F(1.0 / 16.0), F(1.0 / 4.0), F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0)]


def lum(c):
    """Compressed luminance L / (1 + L) of an (..., >=3) float32 array."""
    L = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]
    return L / (F(1.0) + L)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def atrous_level(c, feat_a, feat_b, level, sigma_color, sigma_plane, normal_power_log2):
    """One pass at step 1 << level over (h, w, 4) float32 arrays."""
    h, w, _ = c.shape
    s = 1 << level
    inv_c = F(1.0) / (F(sigma_color) * F(2.0 ** -level))
    inv_z = F(1.0) / (F(sigma_plane) * F(s))
    mat = np.ascontiguousarray(feat_a[..., 3]).view(np.uint32)
    P, N = feat_a[..., :3], feat_b[..., :3]
    lum_all = lum(c)
    acc = np.zeros((h, w, 3), dtype=F)
    acc_w = np.zeros((h, w), dtype=F)
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
            k = H5[j] * H5[i]
            dl = (lum_all[q] - lum_all[p]) * inv_c
            r = F(1.0) / (F(1.0) + dl * dl)
            wc = k * (r * r)
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
    out = c.copy()
    hit = mat != MISS
    with np.errstate(all="ignore"):
        for ch in range(3):
            out[..., ch] = np.where(hit, acc[..., ch] / acc_w, c[..., ch])
    return out


def atrous(c, feat_a, feat_b, levels=5, sigma_color=1.0, sigma_plane=0.05, normal_power_log2=5):
    """The whole filter: `levels` passes, each reading the one before."""
    c = np.ascontiguousarray(c, dtype=F)
    feat_a = np.ascontiguousarray(feat_a, dtype=F)
    feat_b = np.ascontiguousarray(feat_b, dtype=F)
    with np.errstate(all="ignore"):  # (a missed pixel's sums are computed and discarded)
        for level in range(levels):
            c = atrous_level(c, feat_a, feat_b, level, sigma_color, sigma_plane, normal_power_log2)
    return c


def oracle_features(spt, ref, prims, mats, env, w, h, cam=None, jitter=False, rows=None, scene=None):
    """(feat_a, feat_b, albedo), each (len(rows), w, 4) float32, from the oracle: the camera ray of every
    pixel (ref.primary_dir, or spt.camera_ray through the corner / the centre with jitter), RefScene.intersect's
    closest hit, and the shading normal, position, material, albedo and primitive of include/spt.h. `scene`: a
    RefScene of (prims, mats, env) to use instead of a new one (one in brute-force mode, say)."""
    scene = ref.RefScene(prims, mats, env) if scene is None else scene
    rows = list(range(h)) if rows is None else list(rows)
    a = np.zeros((len(rows), w, 4), dtype=F)
    b = np.zeros((len(rows), w, 4), dtype=F)
    alb = np.zeros((len(rows), w, 4), dtype=F)
    au, albu = a.view(np.uint32), alb.view(np.uint32)
    j = 0.5 if jitter else 0.0
    for r, y in enumerate(rows):
        for x in range(w):
            if cam is None:
                o, d = np.zeros(3, dtype=F), ref.primary_dir(x, y, w, h)
            else:
                o, d = spt.camera_ray(cam, w, h, x, y, j, j)
            got = scene.intersect(o, d)
            if got is None:
                au[r, x, 3] = MISS
                b[r, x, 3] = np.inf
                albu[r, x, 3] = MISS
                continue
            t, prim, ng = got
            t = F(t)
            a[r, x, :3] = o + t * d
            au[r, x, 3] = prims[prim]["material"]
            inv = F(1.0) / np.sqrt((ng[0] * ng[0] + ng[1] * ng[1]) + ng[2] * ng[2])
            b[r, x, :3] = ng * inv
            b[r, x, 3] = t
            alb[r, x, :3] = mats[prims[prim]["material"]]["albedo"]
            albu[r, x, 3] = prim
    return a, b, alb


def rms(img, truth):
    """RMS error over RGB and pixels."""
    d = img[..., :3].astype(np.float64) - truth[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=F).view(np.uint32),
                          np.ascontiguousarray(b, dtype=F).view(np.uint32))
