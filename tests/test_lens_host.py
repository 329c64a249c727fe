"""The thin lens's host side, without a GPU: spt_camera_lens_ray (the host build of the function the kernels
compile, spt_device.h camera_lens_ray), spt_camera_focus_at_hit, spt_lens's layout, the argument checks, and
the launch plan of a lens camera (a host program compiled here).

Geometry bounds (float64 arithmetic on the float32 results), eps = 2^-23: a lens ray passes the focus point
O + f p within 32 eps max(|O|, f |p|); its origin lies within radius + 8 eps max(|O|, 1) of O and within
8 eps max(|O|, 1) of the plane through O across the view direction."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
D = np.float64
EPS = 2.0 ** -23
W, H = 37, 23
EYE, TARGET, VFOV = (1.5, 0.75, -2.0), (0.0, -1.0, 5.0), 55.0  # the camera of tests/test_gpu_camera.py
LENSES = [(0.1, 6.0), (0.5, 2.5), (0.02, 40.0)]


def camera(spt, jitter=False):
    return spt.look_at(EYE, TARGET, vfov=VFOV, jitter=jitter)


def vec(a, dtype=D):
    return np.array(list(a), dtype=dtype)


def plane_vector(cam, w, h, x, y, jx=0.0, jy=0.0):
    """p of pixel (x + jx, y + jy) in float64 from the camera's float fields."""
    sx = ((D(x) + D(jx)) / w * 2.0 - 1.0) * (D(w) / D(h))
    sy = (1.0 - (D(y) + D(jy)) / h) * 2.0 - 1.0
    return sx * vec(cam.u) + sy * vec(cam.v) + vec(cam.w)


def distance_to_line(point, o, d):
    o, d = np.asarray(o, dtype=D), np.asarray(d, dtype=D)
    d = d / np.linalg.norm(d)
    v = point - o
    return float(np.linalg.norm(v - np.dot(v, d) * d))


def samples(n, seed):
    """(x, y, u1, u2) of n inputs: the ends u1 = 1, u2 = 1, u1 = 2^-32 and u1 = 0 first, then random ones."""
    rng = np.random.default_rng(seed)
    xs, ys = rng.integers(0, W, n), rng.integers(0, H, n)
    u1, u2 = rng.random(n).astype(F), rng.random(n).astype(F)
    u1[:6] = (1.0, 1.0, 2.0 ** -32, 2.0 ** -32, 0.0, 1.0)
    u2[:6] = (1.0, 0.0, 1.0, 0.5, 0.25, 0.75)
    xs[:4], ys[:4] = (0, W - 1, 0, W - 1), (0, 0, H - 1, H - 1)
    return [(int(x), int(y), F(a), F(b)) for x, y, a, b in zip(xs, ys, u1, u2)]


# ---- layout ------------------------------------------------------------------------------------------
def test_lens_struct_layout_matches_c(spt, tmp_path):
    assert ctypes.sizeof(spt.SptLens) == 16
    src = tmp_path / "lens.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spt.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(spt_lens), offsetof(spt_lens, radius),'
                   ' offsetof(spt_lens, focus_distance), offsetof(spt_lens, reserved), sizeof(spt_camera),'
                   ' SPT_ABI_VERSION); return 0;}\n')
    exe = tmp_path / "lens"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    c = spt.SptLens
    assert got == [16, c.radius.offset, c.focus_distance.offset, c.reserved.offset, ctypes.sizeof(spt.SptCamera), 3]
    assert got[:4] == [16, 0, 4, 8]


# ---- validation --------------------------------------------------------------------------------------
def test_lens_ray_rejects_invalid_arguments(spt):
    lib = spt.load_library()
    cam = camera(spt)
    o, d = (ctypes.c_float * 3)(), (ctypes.c_float * 3)()

    def call(lens, cam_p=ctypes.byref(cam), w=W, h=H, o_p=o, d_p=d):
        return lib.spt_camera_lens_ray(cam_p, ctypes.byref(lens) if lens is not None else None, w, h, 1, 2, 0.0, 0.0,
                                       0.25, 0.5, o_p, d_p)

    def lens(radius, focus, reserved=(0, 0)):
        l = spt.SptLens()
        l.radius, l.focus_distance = radius, focus
        l.reserved[:] = reserved
        return l

    good = lens(0.1, 6.0)
    assert call(good) == 0
    assert call(lens(0.0, 6.0)) == 0  # (radius 0 is a valid lens: the pinhole)
    assert call(None) == -1 and call(good, cam_p=None) == -1
    assert call(good, o_p=None) == -1 and call(good, d_p=None) == -1
    assert call(good, w=0) == -1 and call(good, h=0) == -1
    for radius in (-0.1, float("nan"), float("inf"), -float("inf")):
        assert call(lens(radius, 6.0)) == -1, radius
    for focus in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(lens(0.1, focus)) == -1, focus
    assert call(lens(0.1, 6.0, (1, 0))) == -1 and call(lens(0.1, 6.0, (0, 7))) == -1
    # the aperture sample is a pair of random_float values, in [0, 1]
    fp = ctypes.POINTER(ctypes.c_float)
    for u1, u2, want in ((0.0, 0.0, 0), (1.0, 1.0, 0), (-0.0, 0.5, 0), (1.0000001, 0.5, -1), (0.5, 1.0000001, -1),
                         (-1e-9, 0.5, -1), (0.5, -1e-9, -1), (float("nan"), 0.5, -1), (0.5, float("nan"), -1),
                         (float("inf"), 0.5, -1), (0.5, float("inf"), -1)):
        rc = lib.spt_camera_lens_ray(ctypes.byref(cam), ctypes.byref(good), W, H, 1, 2, 0.0, 0.0, u1, u2,
                                     ctypes.cast(o, fp), ctypes.cast(d, fp))
        assert rc == want, (u1, u2, rc)
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        spt.camera_lens_ray(cam, (-1.0, 6.0), W, H, 0, 0)
    # spt_set_camera_lens on no ctx (its other checks need one: tests/test_gpu_lens.py)
    assert lib.spt_set_camera_lens(None, ctypes.byref(good)) == -1
    assert lib.spt_set_camera_lens(None, None) == -1


def test_focus_at_hit_rejects_invalid_arguments(spt):
    lib = spt.load_library()
    cam = camera(spt)
    f = ctypes.c_float()

    def call(t, cam_p=ctypes.byref(cam), w=W, h=H, out=ctypes.byref(f)):
        return lib.spt_camera_focus_at_hit(cam_p, w, h, 3, 4, 0.0, 0.0, t, out)

    assert call(5.0) == 0 and f.value > 0.0
    for t in (0.0, -2.0, float("nan"), float("inf"), -float("inf")):
        assert call(t) == -1, t
    assert call(5.0, cam_p=None) == -1 and call(5.0, out=None) == -1
    assert call(5.0, w=0) == -1 and call(5.0, h=0) == -1
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        spt.camera_focus_at_hit(cam, W, H, 3, 4, float("inf"))


# ---- geometry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,focus", LENSES)
@pytest.mark.parametrize("jitter", [False, True])
def test_lens_rays_meet_in_the_focus_plane(spt, radius, focus, jitter):
    cam = camera(spt)
    O, Fw = vec(cam.origin), vec(cam.w)
    worst = [0.0, 0.0, 0.0]
    for i, (x, y, u1, u2) in enumerate(samples(1500, 0x1e45 + int(radius * 1000))):
        jx, jy = ((u2, u1) if i % 2 else (F(0.5), F(0.5))) if jitter else (F(0), F(0))
        o, d = spt.camera_lens_ray(cam, (radius, focus), W, H, x, y, jx, jy, u1, u2)
        p = plane_vector(cam, W, H, x, y, jx, jy)
        P = O + D(F(focus)) * p
        bound = 32 * EPS * max(np.linalg.norm(O), D(F(focus)) * np.linalg.norm(p))
        dist = distance_to_line(P, o, d)
        assert dist <= bound, (x, y, u1, u2, dist, bound)
        off = o.astype(D) - O
        slack = 8 * EPS * max(np.linalg.norm(O), 1.0)
        assert np.linalg.norm(off) <= D(F(radius)) + slack, (x, y, u1, u2, np.linalg.norm(off))
        assert abs(np.dot(off, Fw)) <= slack, (x, y, u1, u2, np.dot(off, Fw))
        assert abs(np.linalg.norm(d.astype(D)) - 1.0) <= 4 * EPS
        worst = [max(worst[0], dist / bound), max(worst[1], (np.linalg.norm(off) - D(F(radius))) / slack),
                 max(worst[2], abs(np.dot(off, Fw)) / slack)]
    print(f"lens ({radius}, {focus}) jitter={jitter}: worst fractions of the bounds {worst}")


def test_aperture_is_sampled_uniformly(spt):
    """Over the 64 x 64 grid of cell centres of (u1, u2), mean |o - O|^2 / radius^2 = 1/2 (the disc's)."""
    cam = camera(spt)
    radius, focus = 0.5, 2.5
    O = vec(cam.origin)
    total, seen = 0.0, set()
    for i in range(64):
        for j in range(64):
            o, _ = spt.camera_lens_ray(cam, (radius, focus), W, H, 18, 11, 0.0, 0.0, (i + 0.5) / 64, (j + 0.5) / 64)
            off = o.astype(D) - O
            total += float(np.dot(off, off)) / float(D(F(radius))) ** 2
            seen.add((int(np.sign(np.dot(off, vec(cam.u)))), int(np.sign(np.dot(off, vec(cam.v))))))
    mean = total / 4096
    print(f"mean |o - O|^2 / radius^2 = {mean:.8f}")
    assert abs(mean - 0.5) <= 1e-4
    assert {(1, 1), (1, -1), (-1, 1), (-1, -1)} <= seen  # every quadrant of the aperture


# ---- the stated expressions, restated ------------------------------------------------------------------
def lens_scalars_np(cam, radius):
    def length(v):
        x, y, z = (D(c) for c in v)
        return np.sqrt((x * x + y * y) + z * z)
    return F(D(F(radius)) / length(cam.u)), F(D(F(radius)) / length(cam.v))


def lens_ray_np(cam, radius, focus, w, h, x, y, jx, jy, u1, u2):
    """The expressions of spt.h / DESIGN.md, one np.float32 operation per step (sin and cos: numpy's fp64)."""
    O, U, V, Wv = (vec(a, F) for a in (cam.origin, cam.u, cam.v, cam.w))
    a, b = lens_scalars_np(cam, radius)
    f = F(focus)
    inv_w, inv_h, aspect = F(1.0) / F(w), F(1.0) / F(h), F(w) / F(h)
    px = F(x) + F(jx)
    py = F(y) + F(jy)
    u = px * inv_w
    v = F(1.0) - py * inv_h
    sx = (u * F(2.0) - F(1.0)) * aspect
    sy = v * F(2.0) - F(1.0)
    p = [(sx * U[c] + sy * V[c]) + Wv[c] for c in range(3)]
    r = np.sqrt(F(u1))
    phi = (F(2.0) * F(np.pi)) * F(u2)
    assert r.dtype == F and phi.dtype == F
    cp, sp = np.cos(D(phi)), np.sin(D(phi))
    lx, ly = F(D(r) * cp), F(D(r) * sp)
    ax, ay = lx * a, ly * b
    off = [ax * U[c] + ay * V[c] for c in range(3)]
    o = [O[c] + off[c] for c in range(3)]
    t = [f * p[c] - off[c] for c in range(3)]
    ln = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    assert ln.dtype == F
    return np.array(o, dtype=F), np.array([t[c] / ln for c in range(3)], dtype=F)


def ulps_apart(a, b):
    def order(x):
        i = np.ascontiguousarray(x, dtype=F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(order(a) - order(b))


@pytest.mark.parametrize("radius,focus", LENSES)
def test_lens_ray_is_the_stated_formula(spt, radius, focus):
    cam = camera(spt)
    quarter = [F(0.0), F(0.25), F(0.5), F(0.75), F(1.0)]
    n_exact = 0
    for i, (x, y, u1, u2) in enumerate(samples(1200, 0xf0c5)):
        jx, jy = (F(0), F(0)) if i % 3 else (u2, u1)
        if i % 2:  # phi a multiple of pi / 2 (in fp32): sin and cos are 0 and +-1 to within the fp64 rounding
            u2 = quarter[(i // 2) % 5]
        o, d = spt.camera_lens_ray(cam, (radius, focus), W, H, x, y, jx, jy, u1, u2)
        wo, wd = lens_ray_np(cam, radius, focus, W, H, x, y, jx, jy, u1, u2)
        what = (x, y, jx, jy, u1, u2, o, wo, d, wd)
        assert o.view(np.uint32).tolist() == wo.view(np.uint32).tolist(), what
        if u2 in quarter:
            assert d.view(np.uint32).tolist() == wd.view(np.uint32).tolist(), what
            n_exact += 1
        else:
            assert int(ulps_apart(d, wd).max()) <= 2, what
    assert n_exact >= 600


def test_radius_zero_is_the_pinhole_ray_up_to_the_focus_scale(spt):
    """radius 0: the origin is the camera's, and with focus distance 1 the direction is spt_camera_ray's bits
    (t = 1 * p - 0)."""
    cam = camera(spt)
    for x, y, u1, u2 in samples(200, 0x91):
        o, d = spt.camera_lens_ray(cam, (0.0, 1.0), W, H, x, y, u1, u2, u1, u2)
        po, pd = spt.camera_ray(cam, W, H, x, y, u1, u2)
        assert o.view(np.uint32).tolist() == po.view(np.uint32).tolist()
        assert d.view(np.uint32).tolist() == pd.view(np.uint32).tolist()


# ---- focus picking -----------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True])
def test_focus_at_hit_puts_the_point_in_focus(spt, jitter):
    cam = camera(spt, jitter)
    O = vec(cam.origin)
    j = 0.5 if jitter else 0.0
    rng = np.random.default_rng(0xf0c)
    for k in range(60):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        t = float(F((0.3, 2.5, 6.0, 40.0, 700.0)[k % 5] * (1.0 + rng.random())))
        f = spt.camera_focus_at_hit(cam, W, H, x, y, t, j, j)
        p = plane_vector(cam, W, H, x, y, j, j)
        assert f == F(D(t) / np.linalg.norm(p))
        co, cd = spt.camera_ray(cam, W, H, x, y, j, j)  # the chief ray
        Q = co.astype(D) + D(t) * cd.astype(D)
        bound = 32 * EPS * max(np.linalg.norm(O), D(f) * np.linalg.norm(p))
        for u1, u2 in ((1.0, 0.0), (1.0, 0.37), (0.5, 0.5), (0.25, 0.81), (2.0 ** -32, 1.0)):
            o, d = spt.camera_lens_ray(cam, (0.2, f), W, H, x, y, j, j, u1, u2)
            dist = distance_to_line(Q, o, d)
            assert dist <= bound, (x, y, t, f, u1, u2, dist, bound)


# ---- the launch plan ---------------------------------------------------------------------------------
def test_launch_plan_of_a_lens_camera(spt, tmp_path):
    csrc = os.path.join(os.path.dirname(spt.LIB_PATH), "csrc")
    src = os.path.join(ROOT, "tests", "cpp", "test_lens_plan.cpp")  # (built here, not by tests/cpp/Makefile)
    exe = tmp_path / "test_lens_plan"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", f"-I{csrc}", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_device_lens_inputs_reach_their_branches(spt):
    """tests/cpp/test_device_lens --host (no kernel runs): its inputs reach both sides of every gate term."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_device_lens")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/test_device_lens"], check=True)
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout and "not reached" not in r.stdout, r.stdout + r.stderr
