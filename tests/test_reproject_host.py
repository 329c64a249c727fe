"""Temporal reprojection without a GPU: spt_reproject_host — the host build of the function the kernels compile
(csrc/spt_reproject.h) — against the numpy restatement of include/spt.h's definition (tests/reproject_ref.py),
bit for bit, on the oracle's images and first-hit features; every branch of the definition reached; the
parameters' validation and the struct's layout; the dual basis; and the definition's quality: what reusing 32
frames of the old view is worth at the new one, and that it does not ghost."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import reproject_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
E, T, I, I_AT, VFOV = (1.5, 0.75, -2.0), (0.0, -1.0, 5.0), (0.0, 0.0, 4.0), (0.0, -1.0, 8.0), 55.0
QUALITY_BOUNCES = 4

_views = {}
_sums = {}


def cam_of(spt, name):
    return {"E": lambda: spt.look_at(E, T, vfov=VFOV), "I": lambda: spt.look_at(I, I_AT, vfov=VFOV),
            "Ej": lambda: spt.look_at(E, T, vfov=VFOV, jitter=True), "B": lambda: spt.look_at((1.35, 0.8, -1.9), T, vfov=VFOV),
            "S": lambda: spt.look_at((2.0, 0.5, 0.0), T, vfov=VFOV), "ref": lambda: None}[name]()


def view(spt, ref, scene, w, h, cam, frames=2):
    """(captured image with lengths, feat_a, feat_b) of `scene` through camera `cam` from the oracle; cached."""
    key = (scene, w, h, cam, frames)
    if key not in _views:
        prims, mats, env = spt.build_scene(scene)
        c = cam_of(spt, cam)
        acc = rr.oracle_sum(spt, ref, prims, mats, env, w, h, c, 0, frames, 4)
        a, b, _ = dr.oracle_features(spt, ref, prims, mats, env, w, h, c, jitter=cam.endswith("j"))
        got = (rr.blend(acc, frames, length=True), a, b)
        for arr in got:
            arr.setflags(write=False)
        _views[key] = got
    return _views[key]


def check_equal(spt, prev_cam, cur, old, reusable=None, counts=None, **kw):
    got = spt.reproject_host(prev_cam, cur[1], cur[2], *old, spt.ReprojectParams(**kw) if kw else None, reusable)
    want = rr.reproject(prev_cam, cur[1], cur[2], *old, reusable=reusable, counts=counts, **kw)
    assert got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0][:2])], want[tuple(bad[0][:2])])
    return got


def test_cornell_97x53_every_branch(spt, ref):
    """History from I, current view from E: pixels that miss, lie behind the old camera, project off its image,
    lose taps to the border, the material, the normal and the plane test, keep none, some or all four."""
    counts = {}
    got = check_equal(spt, cam_of(spt, "I"), view(spt, ref, "cornell", 97, 53, "E"), view(spt, ref, "cornell", 97, 53, "I"),
                      counts=counts)
    print(counts)
    for k in ("miss", "behind", "off_image", "tap_outside", "tap_material", "tap_normal", "tap_plane", "no_valid_tap",
              "partial", "full", "kept"):
        assert counts[k] > 0, (k, counts)
    assert counts["kept"] == int(np.sum(got[..., 3] > 0)) and np.all(got[got[..., 3] == 0] == 0)
    assert np.all(got[..., 3][got[..., 3] > 0] == F(2.0))  # (every tap's length is 2: so is their weighted mean)


def test_cornell_97x53_reverse_pair(spt, ref):
    counts = {}
    check_equal(spt, cam_of(spt, "E"), view(spt, ref, "cornell", 97, 53, "I"), view(spt, ref, "cornell", 97, 53, "E"),
                counts=counts)
    print(counts)
    assert counts["no_valid_tap"] > 0 and counts["partial"] > 0 and counts["full"] > 0


def test_c1_reference_camera_to_posed(spt, ref):
    counts = {}
    check_equal(spt, None, view(spt, ref, "c1", 20, 12, "S"), view(spt, ref, "c1", 20, 12, "ref"), counts=counts)
    assert counts["miss"] > 0 and counts["kept"] > 0, counts


def test_one_pixel(spt, ref):
    """1 x 1: the pixel's own history through the same camera (fx = fy = 0: the first tap alone carries weight)."""
    prims, mats, env = spt.sphere_prims([(-3.0, 3.0, 3.0, 1.0)]), spt.reference_materials(), spt.reference_env(True)
    acc = ref.RefScene(prims, mats, env).render(1, 1, 0, 3, 4, 2, 0)
    a, b, _ = dr.oracle_features(spt, ref, prims, mats, env, 1, 1)
    assert a.view(np.uint32)[0, 0, 3] == 0
    old = (rr.blend(acc, 3, length=True), a, b)
    got = check_equal(spt, None, (None, a, b), old)
    assert got[0, 0, 3] == F(3.0)


def test_old_camera_with_jitter(spt, ref):
    """j' = 0.5: the captured features' rays went through the pixels' centres."""
    cur, old = view(spt, ref, "cornell", 97, 53, "E"), view(spt, ref, "cornell", 97, 53, "Ej")
    cam = cam_of(spt, "Ej")
    assert spt.reproject_basis(cam)[2] == 0.5
    got = check_equal(spt, cam, cur, old)
    plain = spt.look_at(E, T, vfov=VFOV)
    assert not dr.bits_equal(got, spt.reproject_host(plain, cur[1], cur[2], *old))
    # the same view half a pixel apart: nearly every hit pixel finds its history
    assert np.sum(got[..., 3] > 0) > 0.9 * np.sum(cur[1].view(np.uint32)[..., 3] != dr.MISS)


def test_degenerate_basis_reuses_nothing(spt, ref):
    cam = spt.look_at(E, T, vfov=VFOV)
    for k in range(3):
        cam.v[k] = cam.u[k]
    rows, _, _ = spt.reproject_basis(cam)
    assert np.all(rows == 0) and np.all(rr.basis(cam)[0] == 0)
    cur, old = view(spt, ref, "cornell", 97, 53, "E"), view(spt, ref, "cornell", 97, 53, "I")
    assert np.all(check_equal(spt, cam, cur, old) == 0)


def test_metal_and_glass_get_no_history(spt, ref):
    cur, old = view(spt, ref, "cornell", 97, 53, "E"), view(spt, ref, "cornell", 97, 53, "I")
    _, mats, _ = spt.build_scene("cornell")
    all_of = check_equal(spt, cam_of(spt, "I"), cur, old)
    mat = cur[1].view(np.uint32)[..., 3]
    # the materials whose pixels receive history: the first a mirror, the second glass, the others diffuse
    with_history = [int(m) for m in np.unique(mat[all_of[..., 3] > 0])]
    assert len(with_history) >= 3, with_history
    metal, glass = with_history[:2]
    reusable = np.ones(len(mats), dtype=np.uint32)
    reusable[[metal, glass]] = 0
    got = check_equal(spt, cam_of(spt, "I"), cur, old, reusable=reusable)
    barred = (mat == metal) | (mat == glass)
    assert np.any(all_of[barred][:, 3] > 0) and np.all(got[barred] == 0)
    assert dr.bits_equal(got[~barred], all_of[~barred]) and np.any(got[..., 3] > 0)
    # a table shorter than the materials in the image: the ones beyond it are not reusable
    short = check_equal(spt, cam_of(spt, "I"), cur, old, reusable=reusable[:1])
    assert np.all(short[mat >= 1] == 0)


def test_max_history_caps_the_length(spt, ref):
    cur, old = view(spt, ref, "cornell", 97, 53, "E"), view(spt, ref, "cornell", 97, 53, "I")
    long = (old[0].copy(), old[1], old[2])
    long[0][..., 3] = F(40.0)
    got = check_equal(spt, cam_of(spt, "I"), cur, long)
    assert set(np.unique(got[..., 3])) == {F(0.0), F(32.0)}
    got = check_equal(spt, cam_of(spt, "I"), cur, long, max_history=64.0)
    kept = got[..., 3][got[..., 3] > 0]  # (a weighted mean of 40s, rounded: 40 to a few ulp, under the cap)
    assert kept.size and np.all(np.abs(kept - F(40.0)) < 1e-4)


@pytest.mark.parametrize("kw", [{"max_history": 1.0}, {"normal_min": 0.9999}, {"normal_min": -1.0}, {"plane_tolerance": 0.0},
                                {"plane_tolerance": 1.0}, {"min_weight": 0.9}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_parameters_reach_the_result(spt, ref, kw):
    cur, old = view(spt, ref, "cornell", 97, 53, "E"), view(spt, ref, "cornell", 97, 53, "I")
    got = check_equal(spt, cam_of(spt, "I"), cur, old, **kw)
    assert not dr.bits_equal(got, spt.reproject_host(cam_of(spt, "I"), cur[1], cur[2], *old))


def test_defaults(spt):
    p = spt.ReprojectParams()
    assert (p.max_history, p.normal_min, p.plane_tolerance, p.min_weight) == (32.0, float(F(0.9)), float(F(0.01)),
                                                                            float(F(0.01)))
    assert list(p.reserved) == [0, 0, 0, 0]
    assert spt.load_library().spt_reproject_params_default(None) == -1


@pytest.mark.parametrize("kw", [{"max_history": 0.5}, {"max_history": float("nan")}, {"max_history": float("inf")},
                                {"normal_min": float("nan")}, {"normal_min": float("inf")}, {"plane_tolerance": -0.01},
                                {"plane_tolerance": float("nan")}, {"plane_tolerance": float("inf")}, {"min_weight": 0.0},
                                {"min_weight": -1.0}, {"min_weight": float("nan")}, {"min_weight": float("inf")}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_parameters(spt, kw):
    z = np.zeros((2, 2, 4), dtype=F)
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        spt.reproject_host(None, z, z, z, z, z, spt.ReprojectParams(**kw))


def test_invalid_reserved_camera_and_null_pointers(spt):
    lib = spt.load_library()
    z = np.zeros((2, 2, 4), dtype=F)
    out = np.zeros((2, 2, 4), dtype=F)
    P = ctypes.c_void_p
    for word in range(4):
        p = spt.ReprojectParams()
        p.reserved[word] = 1
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            spt.reproject_host(None, z, z, z, z, z, p)
    bad = spt.look_at(E, T, vfov=VFOV)
    bad.u[0] = float("nan")
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        spt.reproject_host(bad, z, z, z, z, z)
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        spt.reproject_basis(bad)
    zp = P(z.ctypes.data)
    ok = [None, None, 2, 2, zp, zp, zp, zp, zp, None, 0, P(out.ctypes.data)]
    assert lib.spt_reproject_host(*ok) == 0
    for k in (4, 5, 6, 7, 8, 11):
        args = list(ok)
        args[k] = None
        assert lib.spt_reproject_host(*args) == -1
    for k in (2, 3):
        args = list(ok)
        args[k] = 0
        assert lib.spt_reproject_host(*args) == -1
    rows, origin, j = (ctypes.c_float * 9)(), (ctypes.c_float * 3)(), ctypes.c_float()
    assert lib.spt_reproject_basis(None, rows, origin, ctypes.byref(j)) == 0
    assert lib.spt_reproject_basis(None, None, origin, ctypes.byref(j)) == -1
    assert lib.spt_reproject_basis(None, rows, None, ctypes.byref(j)) == -1
    assert lib.spt_reproject_basis(None, rows, origin, None) == -1
    # the ctx calls refuse a null ctx before anything else
    assert lib.spt_history_capture(None, 1) == -1
    assert lib.spt_reproject(None, None) == -1
    assert lib.spt_history_clear(None) == -1
    assert lib.spt_read_history(None, None) == -1
    assert lib.spt_history_device_ptr(None, None, None) == -1
    assert lib.spt_history_blend(None, 1) == -1
    assert lib.spt_read_blended(None, None) == -1
    assert lib.spt_blended_device_ptr(None, None, None) == -1
    assert lib.spt_resolve_blended_rgba8(None, 1.0, None) == -1
    assert lib.spt_denoise_blended(None, None) == -1
    assert lib.spt_set_history_layout(None, -1) == -1


def test_struct_layout_matches_c(spt, tmp_path):
    src = tmp_path / "rp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spt.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(spt_reproject_params),'
                   ' offsetof(spt_reproject_params, max_history), offsetof(spt_reproject_params, normal_min),'
                   ' offsetof(spt_reproject_params, plane_tolerance), offsetof(spt_reproject_params, min_weight),'
                   ' offsetof(spt_reproject_params, reserved)); return 0;}\n')
    exe = tmp_path / "rp"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = spt.ReprojectParams
    assert got == [ctypes.sizeof(R), R.max_history.offset, R.normal_min.offset, R.plane_tolerance.offset,
                   R.min_weight.offset, R.reserved.offset]
    assert got[0] == 32


def test_basis(spt):
    """The float64 restatement's bits; the dual of a look_at camera's orthogonal (u, v, w); the defaults."""
    rows, origin, j = spt.reproject_basis(None)
    assert np.array_equal(rows, np.eye(3, dtype=F)) and np.all(origin == 0) and j == 0.0
    for eye, target, vfov, jitter in ((E, T, VFOV, False), (I, I_AT, 35.0, True), ((2.0, 0.5, 0.0), T, 110.0, False)):
        cam = spt.look_at(eye, target, vfov=vfov, jitter=jitter)
        rows, origin, j = spt.reproject_basis(cam)
        want = rr.basis(cam)
        assert dr.bits_equal(rows, want[0]) and dr.bits_equal(origin, want[1]) and j == float(want[2])
        u, v, w = (np.array(list(x), dtype=np.float64) for x in (cam.u, cam.v, cam.w))
        got = rows.astype(np.float64) @ np.stack([u, v, w]).T
        assert np.allclose(got, np.eye(3), rtol=0.0, atol=1e-6), got
    # a skewed basis is still inverted exactly enough
    cam = spt.look_at(E, T, vfov=VFOV)
    cam.u[1] += 0.25
    cam.w[0] -= 0.5
    assert dr.bits_equal(spt.reproject_basis(cam)[0], rr.basis(cam)[0])


# ---- quality -------------------------------------------------------------------------------------------
def mean_at(spt, ref, scene, w, h, cam, first, n):
    key = (scene, w, h, cam, first, n)
    if key not in _sums:
        prims, mats, env = spt.build_scene(scene)
        m = rr.oracle_sum(spt, ref, prims, mats, env, w, h, cam_of(spt, cam), first, n, QUALITY_BOUNCES) / F(n)
        m.setflags(write=False)
        _sums[key] = m
    return _sums[key]


def feats_at(spt, ref, scene, w, h, cam):
    key = (scene, w, h, cam, "features")
    if key not in _sums:
        prims, mats, env = spt.build_scene(scene)
        _sums[key] = dr.oracle_features(spt, ref, prims, mats, env, w, h, cam_of(spt, cam))[:2]
    return _sums[key]


def history(spt, ref, scene, w, h, old, new, frames=32, **kw):
    """`frames` frames of the old view, captured and reprojected into the new one."""
    hc = mean_at(spt, ref, scene, w, h, old, 0, frames).copy()
    hc[..., 3] = F(frames)
    ha, hb = feats_at(spt, ref, scene, w, h, old)
    ca, cb = feats_at(spt, ref, scene, w, h, new)
    params = spt.ReprojectParams(**kw) if kw else None
    return spt.reproject_host(cam_of(spt, old), ca, cb, hc, ha, hb, params)


@pytest.mark.parametrize("scene,w,h", [("cornell", 96, 54), ("app", 64, 64)])
def test_quality_blend_after_a_small_move(spt, ref, scene, w, h):
    """32 frames at E, the eye moves to (1.35, .8, -1.9), one frame there: the blend's RMS error against 256
    frames of the new view (from frame 1000) is at most a quarter of the one-sample image's (the definition
    measured 0.14 and 0.17 when it was written; the margin covers the truth's own noise)."""
    hist = history(spt, ref, scene, w, h, "E", "B")
    one = mean_at(spt, ref, scene, w, h, "B", 0, 1)
    truth = mean_at(spt, ref, scene, w, h, "B", 1000, 256)
    blended = rr.blend(one, 1, hist)
    noisy, reused = dr.rms(one, truth), dr.rms(blended, truth)
    print(f"{scene} {w}x{h}: 1 spp rms {noisy:.4f}, blended with 32 reprojected frames {reused:.4f}, "
          f"ratio {reused / noisy:.3f}; pixels with history {np.mean(hist[..., 3] > 0):.3f}")
    assert reused <= 0.25 * noisy


@pytest.mark.parametrize("scene,w,h,old,new", [("cornell", 97, 53, "E", "I"), ("cornell", 97, 53, "I", "E"),
                                               ("app", 64, 64, "ref", "S")])
def test_quality_no_ghosting(spt, ref, scene, w, h, old, new):
    """On the pixels that received history, 32 reprojected frames of the old view are no further from the truth
    (256 frames of the new view from frame 1000) than 32 independent frames of the new view (from frame 5000):
    measured 0.143 vs 0.192, 0.161 vs 0.205 and 0.0210 vs 0.0248 when the definition was written."""
    hist = history(spt, ref, scene, w, h, old, new)
    got = hist[..., 3] > 0
    assert got.any()
    truth = mean_at(spt, ref, scene, w, h, new, 1000, 256)
    fresh = mean_at(spt, ref, scene, w, h, new, 5000, 32)
    reused, independent = dr.rms(hist[got], truth[got]), dr.rms(fresh[got], truth[got])
    print(f"{scene} {old}->{new}: history rms {reused:.4f} vs independent 32 frames {independent:.4f} on "
          f"{int(got.sum())} pixels")
    assert reused <= independent
