"""The camera's host side, without a GPU: spt_camera_look_at, spt_camera_ray (the host build of the
function the kernels compile, spt_device.h camera_ray_dir), the struct's layout, spt_set_camera's
argument checks, and the launch plan of a jittered camera (a host program compiled here)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_look_at_identity_is_the_reference_camera(spt):
    cam = spt.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0), 90.0)
    assert list(cam.origin) == [0.0, 0.0, 0.0]
    assert list(cam.u) == [1.0, 0.0, 0.0] and list(cam.v) == [0.0, 1.0, 0.0] and list(cam.w) == [0.0, 0.0, 1.0]
    assert cam.flags == 0 and list(cam.reserved) == [0, 0, 0]
    assert spt.look_at((0, 0, 0), (0, 0, 1), jitter=True).flags == spt.CAMERA_JITTER


def test_look_at_rejects_degenerate_input(spt):
    with pytest.raises(spt.SptError):
        spt.look_at((1, 2, 3), (1, 2, 3))  # eye == target
    with pytest.raises(spt.SptError):
        spt.look_at((0, 0, 0), (0, 2, 0), up=(0, 1, 0))  # up parallel to the view direction
    with pytest.raises(spt.SptError):
        spt.look_at((0, 0, 0), (0, -2, 0), up=(0, 3, 0))  # ... and anti-parallel
    for vfov in (0.0, 180.0, -10.0, 200.0, float("nan")):
        with pytest.raises(spt.SptError):
            spt.look_at((0, 0, 0), (0, 0, 1), vfov=vfov)


@pytest.mark.parametrize("eye,target,up,vfov", [
    ((1.5, 0.75, -2.0), (0.0, -1.0, 5.0), (0, 1, 0), 55.0),
    ((0, 0, 0), (-3.0, 0.5, -1.0), (0.2, 1.0, 0.1), 30.0),
    ((10, -4, 2), (9, -4.5, 7), (0, 0, 1), 120.0),
])
def test_look_at_basis_is_orthogonal(spt, eye, target, up, vfov):
    cam = spt.look_at(eye, target, up, vfov)
    u, v, w = (np.array(list(a), dtype=np.float64) for a in (cam.u, cam.v, cam.w))
    h = np.tan(np.radians(vfov) / 2)
    assert abs(np.linalg.norm(w) - 1) < 1e-6 and abs(np.linalg.norm(u) - h) < 1e-6 * max(1, h)
    assert abs(np.linalg.norm(v) - h) < 1e-6 * max(1, h)
    for a, b in ((u, v), (u, w), (v, w)):
        assert abs(np.dot(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b)) < 1e-6
    f = np.array(target, dtype=np.float64) - np.array(eye, dtype=np.float64)
    assert np.allclose(w, f / np.linalg.norm(f), atol=1e-6)
    assert np.dot(v, np.array(up, dtype=np.float64)) > 0  # v is on up's side
    assert np.allclose(np.cross(w, u / h), v / h, atol=1e-6)  # t = cross(f, r)
    assert list(cam.origin) == [F(c) for c in eye]


def test_set_camera_null_ctx(spt):
    lib = spt.load_library()
    cam = spt.look_at((0, 0, 0), (0, 0, 1))
    assert lib.spt_set_camera(None, ctypes.byref(cam)) == -1
    assert lib.spt_set_camera(None, None) == -1
    o, d = (ctypes.c_float * 3)(), (ctypes.c_float * 3)()
    assert lib.spt_camera_ray(None, 4, 4, 0, 0, 0.0, 0.0, o, d) == -1
    assert lib.spt_camera_ray(ctypes.byref(cam), 0, 4, 0, 0, 0.0, 0.0, o, d) == -1


def test_camera_struct_layout_matches_c(spt, tmp_path):
    assert ctypes.sizeof(spt.SptCamera) == 64
    src = tmp_path / "cam.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spt.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %u\\n", sizeof(spt_camera), offsetof(spt_camera, u), offsetof(spt_camera, w),'
                   ' offsetof(spt_camera, flags), offsetof(spt_camera, reserved), SPT_CAMERA_JITTER); return 0;}\n')
    exe = tmp_path / "cam"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    c = spt.SptCamera
    assert got == [ctypes.sizeof(c), c.u.offset, c.w.offset, c.flags.offset, c.reserved.offset, spt.CAMERA_JITTER]


def camera_ray_np(cam, w, h, x, y, jx, jy):
    """The formula of spt.h / DESIGN.md, one np.float32 operation per step."""
    U, V, W = (np.array(list(a), dtype=F) for a in (cam.u, cam.v, cam.w))
    inv_w, inv_h, aspect = F(1.0) / F(w), F(1.0) / F(h), F(w) / F(h)
    px = F(x) + F(jx)
    py = F(y) + F(jy)
    u = px * inv_w
    v = F(1.0) - py * inv_h
    sx = (u * F(2.0) - F(1.0)) * aspect
    sy = v * F(2.0) - F(1.0)
    p = [(sx * U[c] + sy * V[c]) + W[c] for c in range(3)]
    ln = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
    assert ln.dtype == F
    return np.array([p[c] / ln for c in range(3)], dtype=F)


def basis_camera(spt, u, v, w):
    cam = spt.SptCamera()
    cam.u[:], cam.v[:], cam.w[:] = u, v, w
    return cam


def ulps_apart(a, b):
    """The distance of two float32 arrays in representable values, per element (-0 and +0: 0)."""
    def order(x):
        i = np.ascontiguousarray(x, dtype=F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(order(a) - order(b))


@pytest.mark.parametrize("w,h", [(37, 23), (64, 64), (256, 144)])
def test_identity_camera_ray_is_the_reference_primary_dir(spt, ref, w, h):
    """Every pixel: the identity camera gives ref.primary_dir; so do, turned, the cameras whose p keeps
    the reference's summation order in |p|^2 = (p.x^2 + p.y^2) + p.z^2 — a half turn about y, (-d.x, d.y,
    -d.z), and x and y swapped (the first sum commutes).

    The quarter turn about y, U = (0,0,-1), V = (0,1,0), F = (1,0,0), gives (d.z, d.y, -d.x) of the
    reference direction only up to rounding: its |p|^2 is (1 + sy^2) + sx^2 where the reference adds
    (sx^2 + sy^2) + 1, and float addition does not associate — at 37x23, pixel (17, 0), 0.70411825
    against 0.7041183. Each sum rounds twice (<= 2u off the exact sum, u = 2^-24), so the two lengths
    differ by <= 4u relative (sqrt halves the 4u and rounds once each), and each quotient rounds once
    more: <= 6u relative, which is <= 6 representable values. What holds to the bit is the stated
    formula, checked for this camera as for the generic one (camera_ray_np)."""
    ident = spt.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0), 90.0)
    half = basis_camera(spt, (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0))
    swapped = basis_camera(spt, (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    quarter = basis_camera(spt, (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))
    worst = 0
    for y in range(h):
        for x in range(w):
            want = ref.primary_dir(x, y, w, h)
            o, d = spt.camera_ray(ident, w, h, x, y, 0.0, 0.0)
            assert np.array_equal(d, want) and not o.any(), (x, y, d, want)  # (+-0 compare equal)
            _, dh = spt.camera_ray(half, w, h, x, y)
            assert np.array_equal(dh, np.array([-want[0], want[1], -want[2]], dtype=F)), (x, y, dh, want)
            _, ds = spt.camera_ray(swapped, w, h, x, y)
            assert np.array_equal(ds, np.array([want[1], want[0], want[2]], dtype=F)), (x, y, ds, want)
            _, dq = spt.camera_ray(quarter, w, h, x, y)
            assert np.array_equal(dq.view(np.uint32), camera_ray_np(quarter, w, h, x, y, 0.0, 0.0).view(np.uint32))
            apart = int(ulps_apart(dq, np.array([want[2], want[1], -want[0]], dtype=F)).max())
            worst = max(worst, apart)
            assert apart <= 6, (x, y, dq, want)
    print(f"quarter turn {w}x{h}: at most {worst} representable values from (d.z, d.y, -d.x)")


def test_camera_ray_is_the_stated_formula(spt, ref):
    cam = spt.look_at((1.5, 0.75, -2.0), (0.0, -1.0, 5.0), vfov=55.0)
    rng = np.random.default_rng(0xca3e5a)
    n = 1000
    jit, _ = ref.random_floats(ref.rng_seed(3, 5, 256, 1), 2 * n)
    assert jit.dtype == F and 0.0 <= jit.min() and jit.max() <= 1.0
    jit[:6] = (1.0, 1.0, 1.0, 0.0, 0.0, 1.0)  # random_float can return 1.0f: the footprint's far edges
    for i in range(n):
        w, h = ((37, 23), (256, 144), (1920, 1080))[i % 3]
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        jx, jy = jit[2 * i], jit[2 * i + 1]
        o, d = spt.camera_ray(cam, w, h, x, y, jx, jy)
        want = camera_ray_np(cam, w, h, x, y, jx, jy)
        assert d.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (w, h, x, y, jx, jy, d, want)
        assert o.tolist() == [F(1.5), F(0.75), F(-2.0)]




def test_launch_plan_of_a_jittered_camera(spt, tmp_path):
    csrc = os.path.join(os.path.dirname(spt.LIB_PATH), "csrc")
    src = os.path.join(ROOT, "tests", "cpp", "test_camera_plan.cpp")  # (built here, not by tests/cpp/Makefile)
    exe = tmp_path / "test_camera_plan"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", f"-I{csrc}", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
