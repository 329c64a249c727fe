"""The a-trous denoiser without a GPU: spt_atrous_host — the host build of the function the filter kernels
compile (csrc/spt_atrous.h) — against the numpy restatement of include/spt.h's definition
(tests/denoise_ref.py), bit for bit, on the oracle's images and first-hit features; the parameters'
validation; the definition's quality on the oracle's one-sample images; the parameter struct's layout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

_inputs = {}


def oracle_inputs(spt, ref, scene, w, h, bounces):
    """(mean colour of frame 0, feat_a, feat_b) of a built-in scene from the oracle; computed once."""
    key = (scene, w, h, bounces)
    if key not in _inputs:
        prims, mats, env = spt.build_scene(scene)
        c = ref.RefScene(prims, mats, env).render(w, h, 0, 1, bounces, 2, 0) / F(1.0)
        a, b, _ = dr.oracle_features(spt, ref, prims, mats, env, w, h)
        for arr in (c, a, b):
            arr.setflags(write=False)
        _inputs[key] = (c, a, b)
    return _inputs[key]


def check_equal(spt, c, a, b, **kw):
    got = spt.atrous_host(c, a, b, spt.DenoiseParams(**kw))
    want = dr.atrous(c, a, b, **{"levels": 5, "sigma_color": 1.0, "sigma_plane": 0.05, "normal_power_log2": 5, **kw})
    assert got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0][:2])], want[tuple(bad[0][:2])])


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_cornell_97x53_levels(spt, ref, levels):
    """Width and height are multiples of no tile; every step 1..16."""
    check_equal(spt, *oracle_inputs(spt, ref, "cornell", 97, 53, 8), levels=levels)


def test_image_smaller_than_a_tap_offset(spt, ref):
    """20 x 12 at 5 levels: the last step's taps (2 * 16 = 32 pixels away) nearly all fall outside."""
    check_equal(spt, *oracle_inputs(spt, ref, "cornell", 20, 12, 8), levels=5)


def test_one_pixel(spt, ref):
    """A 1 x 1 image whose only ray (through the pixel's corner: up and to the left) hits a sphere: the
    centre tap alone, out = (w * c) / w."""
    prims, mats, env = spt.sphere_prims([(-3.0, 3.0, 3.0, 1.0)]), spt.reference_materials(), spt.reference_env(True)
    c = ref.RefScene(prims, mats, env).render(1, 1, 0, 1, 4, 2, 0) / F(1.0)
    a, b, _ = dr.oracle_features(spt, ref, prims, mats, env, 1, 1)
    assert a.view(np.uint32)[0, 0, 3] == 0 and np.isfinite(b[0, 0, 3])
    check_equal(spt, c, a, b)


@pytest.mark.parametrize("kw", [{"normal_power_log2": 0}, {"normal_power_log2": 7}, {"sigma_color": 0.25},
                                {"sigma_color": 4.0}, {"sigma_plane": 0.005}, {"sigma_plane": 0.5}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_parameters_reach_the_weights(spt, ref, kw):
    c, a, b = oracle_inputs(spt, ref, "cornell", 97, 53, 8)
    check_equal(spt, c, a, b, **kw)
    assert not dr.bits_equal(spt.atrous_host(c, a, b, spt.DenoiseParams(**kw)), spt.atrous_host(c, a, b))


def test_spheres_and_sky(spt, ref):
    """C1 64 x 64: sphere normals (never flipped), sky pixels beside hits."""
    c, a, b = oracle_inputs(spt, ref, "c1", 64, 64, 4)
    miss = a.view(np.uint32)[..., 3] == dr.MISS
    assert miss.any() and not miss.all()
    check_equal(spt, c, a, b)
    assert dr.bits_equal(spt.atrous_host(c, a, b)[miss], c[miss])  # the sky passes through


def test_all_miss_image_is_unchanged(spt):
    rng = np.random.default_rng(7)
    c = rng.uniform(0.0, 2.0, size=(9, 13, 4)).astype(F)
    a = np.zeros((9, 13, 4), dtype=F)
    a.view(np.uint32)[..., 3] = dr.MISS
    b = np.zeros((9, 13, 4), dtype=F)
    b[..., 3] = np.inf
    got = spt.atrous_host(c, a, b)
    assert dr.bits_equal(got, c)
    assert dr.bits_equal(dr.atrous(c, a, b), c)


def test_output_may_alias_the_input(spt, ref):
    c, a, b = oracle_inputs(spt, ref, "cornell", 20, 12, 8)
    want = spt.atrous_host(c, a, b)
    buf = c.copy()
    fp = ctypes.c_void_p
    rc = spt.load_library().spt_atrous_host(fp(buf.ctypes.data), fp(a.ctypes.data), fp(b.ctypes.data), 20, 12, None,
                                            fp(buf.ctypes.data))
    assert rc == 0 and dr.bits_equal(buf, want)


def test_defaults(spt):
    p = spt.DenoiseParams()
    assert (p.levels, p.sigma_color, p.sigma_plane, p.normal_power_log2) == (5, 1.0, float(F(0.05)), 5)
    assert list(p.reserved) == [0, 0, 0, 0]
    assert spt.load_library().spt_denoise_params_default(None) == -1


@pytest.mark.parametrize("kw", [{"levels": 0}, {"levels": 7}, {"sigma_color": 0.0}, {"sigma_color": -1.0},
                                {"sigma_color": float("nan")}, {"sigma_color": float("inf")}, {"sigma_plane": 0.0},
                                {"sigma_plane": -0.05}, {"sigma_plane": float("nan")}, {"sigma_plane": float("inf")},
                                {"normal_power_log2": 8}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_parameters(spt, kw):
    z = np.zeros((2, 2, 4), dtype=F)
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        spt.atrous_host(z, z, z, spt.DenoiseParams(**kw))


def test_invalid_reserved_and_null_pointers(spt):
    lib = spt.load_library()
    z = np.zeros((2, 2, 4), dtype=F)
    out = np.zeros((2, 2, 4), dtype=F)
    P = ctypes.c_void_p
    for word in range(4):
        p = spt.DenoiseParams()
        p.reserved[word] = 1
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            spt.atrous_host(z, z, z, p)
    ok = [P(z.ctypes.data), P(z.ctypes.data), P(z.ctypes.data), 2, 2, None, P(out.ctypes.data)]
    assert lib.spt_atrous_host(*ok) == 0
    for k in (0, 1, 2, 6):
        args = list(ok)
        args[k] = None
        assert lib.spt_atrous_host(*args) == -1
    for k in (3, 4):
        args = list(ok)
        args[k] = 0
        assert lib.spt_atrous_host(*args) == -1
    # the ctx calls refuse a null ctx before anything else
    assert lib.spt_render_features(None) == -1
    assert lib.spt_read_features(None, None, None, None) == -1
    assert lib.spt_features_device_ptr(None, None, None, None, None) == -1
    assert lib.spt_denoise(None, 1, None) == -1
    assert lib.spt_set_denoise_form(None, -1) == -1
    assert lib.spt_read_denoised(None, None) == -1
    assert lib.spt_denoised_device_ptr(None, None, None) == -1
    assert lib.spt_resolve_denoised_rgba8(None, 1.0, None) == -1


@pytest.mark.parametrize("scene,w,h,bounces,cap", [("cornell", 96, 54, 8, 0.5), ("c1", 64, 64, 4, 0.6),
                                                   ("app", 64, 64, 4, 0.75)])
def test_quality_at_one_sample(spt, ref, scene, w, h, bounces, cap):
    """The definition on the oracle's one-frame image, default parameters: RMS error over RGB and pixels
    against the mean of frames 1000..3047, denoised over noisy, at most `cap` (include/spt.h's definition
    measured 0.252 / 0.335 / 0.480 when it was written)."""
    c, a, b = oracle_inputs(spt, ref, scene, w, h, bounces)
    prims, mats, env = spt.build_scene(scene)
    truth = ref.RefScene(prims, mats, env).render(w, h, 1000, 2048, bounces, 2, 0) / F(2048.0)
    noisy = dr.rms(c, truth)
    restated = dr.rms(dr.atrous(c, a, b), truth)
    product = dr.rms(spt.atrous_host(c, a, b), truth)
    print(f"{scene} {w}x{h}: noisy rms {noisy:.4f}, denoised {product:.4f}, ratio {product / noisy:.3f}")
    assert product == restated
    assert product / noisy <= cap


def test_struct_layout_matches_c(spt, tmp_path):
    src = tmp_path / "dn.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spt.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(spt_denoise_params), offsetof(spt_denoise_params, levels),'
                   ' offsetof(spt_denoise_params, sigma_color), offsetof(spt_denoise_params, sigma_plane),'
                   ' offsetof(spt_denoise_params, normal_power_log2), offsetof(spt_denoise_params, reserved));'
                   ' return 0;}\n')
    exe = tmp_path / "dn"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = spt.DenoiseParams
    assert got == [ctypes.sizeof(D), D.levels.offset, D.sigma_color.offset, D.sigma_plane.offset,
                   D.normal_power_log2.offset, D.reserved.offset]
    assert got[0] == 32
