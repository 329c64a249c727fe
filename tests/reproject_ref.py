"""The checker of temporal reprojection (tests/test_reproject_host.py, tests/test_gpu_reproject.py): a numpy
restatement of include/spt.h's definition — float32 arrays, one elementwise operation per arithmetic step,
float64 for the basis, written from that text and not from the product's code — with the count of every class
of pixel and tap the definition tells apart, and the oracle's mean image through a posed camera. Test
infrastructure only.
"""
import ctypes

import numpy as np

from denoise_ref import MISS, F, dot

D = np.float64
DEFAULTS = dict(max_history=32.0, normal_min=0.9, plane_tolerance=0.01, min_weight=0.01)


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=D)


def basis(cam):
    """(rows (3, 3) float32 = ru, rv, rw; origin (3,) float32; j') of a captured camera; None: the reference's."""
    if cam is None:
        return np.eye(3, dtype=F), np.zeros(3, dtype=F), F(0.0)
    u, v, w = (np.array(list(x), dtype=F).astype(D) for x in (cam.u, cam.v, cam.w))
    c = cross(v, w)
    det = (u[0] * c[0] + u[1] * c[1]) + u[2] * c[2]
    if det == 0.0 or not np.isfinite(det):
        rows = np.zeros((3, 3), dtype=F)
    else:
        with np.errstate(all="ignore"):
            rows = np.stack([cross(v, w) / det, cross(w, u) / det, cross(u, v) / det]).astype(F)
    return rows, np.array(list(cam.origin), dtype=F), F(0.5 if cam.flags & 1 else 0.0)


def reproject(prev_cam, cur_a, cur_b, hc, ha, hb, reusable=None, counts=None, **kw):
    """The history (h, w, 4) of the view with features cur_a / cur_b from the captured view (hc, ha, hb) of
    prev_cam. reusable: per material, falsy for METAL / DIELECTRIC (None: all). counts: a dict that receives
    how many pixels / taps took each branch."""
    p = {k: F(v) for k, v in {**DEFAULTS, **kw}.items()}
    cur_a, cur_b, hc, ha, hb = (np.ascontiguousarray(x, dtype=F) for x in (cur_a, cur_b, hc, ha, hb))
    h, w, _ = cur_a.shape
    rows, o, j = basis(prev_cam)
    mat = np.ascontiguousarray(cur_a[..., 3]).view(np.uint32)
    hmat = np.ascontiguousarray(ha[..., 3]).view(np.uint32)
    P, N, t = cur_a[..., :3], cur_b[..., :3], cur_b[..., 3]
    Wf, Hf = F(w), F(h)
    aspect = Wf / Hf
    with np.errstate(all="ignore"):
        miss = mat == MISS
        if reusable is None:
            eye_dep = np.zeros((h, w), dtype=bool)
        else:
            table = np.asarray(reusable).astype(bool)
            idx = np.minimum(mat, len(table) - 1)
            eye_dep = ~miss & ((mat >= len(table)) | ~table[idx])
        e = P - o
        a, b, c = dot(rows[0], e), dot(rows[1], e), dot(rows[2], e)
        front = c > F(0.0)
        sx, sy = a / c, b / c
        fx = ((sx / aspect + F(1.0)) * F(0.5)) * Wf - j
        fy = (F(1.0) - (sy + F(1.0)) * F(0.5)) * Hf - j
        inside = (fx > F(-1.0)) & (fx < Wf) & (fy > F(-1.0)) & (fy < Hf)
        live = ~miss & ~eye_dep & front & inside
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
        x0 = np.where(live, x0f, F(0.0)).astype(np.int64)
        y0 = np.where(live, y0f, F(0.0)).astype(np.int64)
        bound = p["plane_tolerance"] * t
        s = np.zeros((h, w, 4), dtype=F)
        sw = np.zeros((h, w), dtype=F)
        n_valid = np.zeros((h, w), dtype=np.int64)
        tally = dict(tap_outside=0, tap_material=0, tap_normal=0, tap_plane=0)
        for jj in (0, 1):
            for ii in (0, 1):
                qx, qy = x0 + ii, y0 + jj
                ok_in = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                ok_mat = hmat[cy, cx] == mat
                ok_n = dot(N, hb[cy, cx, :3]) >= p["normal_min"]
                ok_p = np.abs(dot(N, ha[cy, cx, :3] - P)) <= bound
                valid = live & ok_in & ok_mat & ok_n & ok_p
                tally["tap_outside"] += int(np.sum(live & ~ok_in))
                tally["tap_material"] += int(np.sum(live & ok_in & ~ok_mat))
                tally["tap_normal"] += int(np.sum(live & ok_in & ok_mat & ~ok_n))
                tally["tap_plane"] += int(np.sum(live & ok_in & ok_mat & ok_n & ~ok_p))
                k = (ax if ii else F(1.0) - ax) * (ay if jj else F(1.0) - ay)
                for ch in range(4):
                    prod = k * hc[cy, cx, ch]
                    s[..., ch] = np.where(valid, s[..., ch] + prod, s[..., ch])
                sw = np.where(valid, sw + k, sw)
                n_valid += valid
        keep = live & (sw >= p["min_weight"])
        out = np.zeros((h, w, 4), dtype=F)
        for ch in range(3):
            out[..., ch] = np.where(keep, s[..., ch] / sw, F(0.0))
        out[..., 3] = np.where(keep, np.fmin(s[..., 3] / sw, p["max_history"]), F(0.0))
    if counts is not None:
        counts.update(tally, miss=int(miss.sum()), eye_dependent=int(eye_dep.sum()),
                      behind=int(np.sum(~miss & ~eye_dep & ~front)),
                      off_image=int(np.sum(~miss & ~eye_dep & front & ~inside)),
                      no_valid_tap=int(np.sum(live & (n_valid == 0))),
                      partial=int(np.sum(live & (n_valid > 0) & (n_valid < 4))),
                      full=int(np.sum(live & (n_valid == 4))), kept=int(keep.sum()))
    return out


def blend(accum, frame_count, hist=None, length=False):
    """The blend of the history `hist` (None: no active history) with the sums `accum` of frame_count frames;
    length: alpha is the result's length (what a capture stores), else the mean's alpha."""
    accum = np.ascontiguousarray(accum, dtype=F)
    f = F(frame_count)
    m = accum / f
    out = m.copy()
    if hist is not None:
        hist = np.ascontiguousarray(hist, dtype=F)
    ha = np.zeros(accum.shape[:-1], dtype=F) if hist is None else hist[..., 3]
    if hist is not None:
        with np.errstate(all="ignore"):
            n = ha + f
            for ch in range(3):
                mixed = (hist[..., ch] * ha + m[..., ch] * f) / n
                out[..., ch] = np.where(ha > F(0.0), mixed, m[..., ch])
    if length:
        out[..., 3] = ha + f
    return out


def oracle_sum(spt, ref, prims, mats, env, w, h, cam, first, n, bounces, rr=2, flags=0):
    """(h, w, 4) float32: the accumulation of frames [first, first + n) through `cam` (None: the reference's
    camera), added in frame order, composed from the oracle's pieces as tests/test_gpu_camera.py
    frame_radiance does."""
    if cam is None:
        return ref.RefScene(prims, mats, env).render(w, h, first, n, bounces, rr, flags)
    rs = ref.RefScene(prims, mats, env)
    lib, slib = ref.load(), spt.load_library()
    cfg = ref.RefConfig(w, h, bounces, rr, flags)
    f3 = ctypes.c_float * 3
    o, d, out = f3(), f3(), (ctypes.c_float * 4)()
    state = ctypes.c_uint32()
    jitter = bool(cam.flags & spt.CAMERA_JITTER)
    acc = np.zeros((h, w, 4), dtype=F)
    one = np.zeros((h, w, 4), dtype=F)
    for f in range(first, first + n):
        for y in range(h):
            for x in range(w):
                state.value = lib.ref_rng_seed(x, y, w, f + 1)
                jx = jy = 0.0
                if jitter:
                    jx = lib.ref_random_float(ctypes.byref(state))
                    jy = lib.ref_random_float(ctypes.byref(state))
                slib.spt_camera_ray(ctypes.byref(cam), w, h, x, y, jx, jy, o, d)
                lib.ref_trace_ray(rs.h, ctypes.byref(cfg), o, d, ctypes.byref(state), out)
                one[y, x] = out[:]
        acc = acc + one
    return acc
