"""The variance-guided a-trous denoiser without a GPU: spt_atrous_guided_host — the host build of the functions
the guided kernels compile (csrc/spt_atrous_guided.h) — against the numpy restatement of include/spt.h's
definition (tests/guided_ref.py), bit for bit in colour and variance, on the oracle's accumulations, the moments
tests/noise_ref.py folds from them and the oracle's first-hit features; the parameters' validation; the struct's
layout; the host function under the sanitizers; and the definition's quality after 8 batches of 8 frames.

Quality figures of this definition on the oracle (RMS over RGB against the mean of frames 1000..3047; noisy mean /
plain spt_denoise / guided, and guided over noisy): see test_quality_after_eight_batches's docstring."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import guided_ref as gr
import host_program
import noise_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

_cache = {}


def one_sphere(spt):
    """The 1 x 1 one-sphere image of test_denoise_host.py: its only ray (up and to the left) hits the sphere."""
    return spt.sphere_prims([(-3.0, 3.0, 3.0, 1.0)]), spt.reference_materials(), spt.reference_env(True)


def scene_of(spt, name):
    return one_sphere(spt) if name == "one_sphere" else spt.build_scene(name)


def inputs(spt, ref, name, w, h, bounces, frame_counts):
    """(mean colour, moments, feat_a, feat_b, B, frame_count) from the oracle: the accumulation after each of
    frame_counts frames folded as one batch each (noise_ref.fold); computed once per sequence."""
    key = (name, w, h, bounces, tuple(frame_counts))
    if key not in _cache:
        prims, mats, env = scene_of(spt, name)
        rs = ref.RefScene(prims, mats, env)
        accums = [rs.render(w, h, 0, fc, bounces, 2, 0, threads=8) for fc in frame_counts]
        m, B, W = nr.fold(accums, frame_counts)
        f = int(frame_counts[-1])
        assert B == len(frame_counts) and W == f
        c = (accums[-1] / F(f)).astype(F)
        a, b, _ = dr.oracle_features(spt, ref, prims, mats, env, w, h)
        for arr in (c, m, a, b):
            arr.setflags(write=False)
        _cache[key] = (c, m, a, b, B, f)
    return _cache[key]


def check_equal(spt, c, m, a, b, B, f, **kw):
    got, got_v = spt.atrous_guided_host(c, m, a, b, B, f, spt.GuidedParams(**kw))
    want, want_v = gr.guided(c, m, a, b, B, f, **kw)
    assert got.shape == want.shape and got_v.shape == want_v.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0][:2])], want[tuple(bad[0][:2])])
    bad = np.argwhere(got_v.view(np.uint32) != want_v.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:4], got_v[tuple(bad[0])], want_v[tuple(bad[0])])
    return got, got_v


FOUR_BY_TWO = (2, 4, 6, 8)  # 4 batches of 2 frames


# ---- bit equality -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_cornell_97x53_levels(spt, ref, levels):
    """Width and height are multiples of no tile; every step 1..16."""
    check_equal(spt, *inputs(spt, ref, "cornell", 97, 53, 8, FOUR_BY_TWO), levels=levels)


def test_image_smaller_than_a_tap_offset(spt, ref):
    """20 x 12 at 5 levels: the last step's taps (2 * 16 = 32 pixels away) nearly all fall outside."""
    check_equal(spt, *inputs(spt, ref, "cornell", 20, 12, 8, FOUR_BY_TWO), levels=5)


def test_one_pixel(spt, ref):
    """A single pixel with B = 2: the centre tap alone at every level, the prefilter's one tap."""
    c, m, a, b, B, f = inputs(spt, ref, "one_sphere", 1, 1, 4, (1, 2))
    assert a.view(np.uint32)[0, 0, 3] == 0 and np.isfinite(b[0, 0, 3]) and B == 2
    check_equal(spt, c, m, a, b, B, f)


def test_spheres_and_sky_unequal_batches(spt, ref):
    """C1 64 x 64, B = 3 with batches of 1, 2 and 5 frames: sky pixels beside hits."""
    c, m, a, b, B, f = inputs(spt, ref, "c1", 64, 64, 4, (1, 3, 8))
    miss = a.view(np.uint32)[..., 3] == dr.MISS
    assert miss.any() and not miss.all() and (B, f) == (3, 8)
    got, got_v = check_equal(spt, c, m, a, b, B, f)
    # the sky passes through: its colour, and its (prefiltered) variance
    assert gr.bits_equal(got[miss], c[miss])
    assert gr.bits_equal(got_v[miss], gr.prefilter(gr.variance0(m, B, f))[miss])


def test_all_miss_image_is_unchanged(spt):
    rng = np.random.default_rng(7)
    c = rng.uniform(0.0, 2.0, size=(9, 13, 4)).astype(F)
    m = np.zeros((9, 13, 4), dtype=F)
    m[..., 0] = rng.uniform(0.0, 2.0, size=(9, 13))
    m[..., 1] = rng.uniform(-0.1, 0.5, size=(9, 13))  # (some negative: v0 clamps them)
    a = np.zeros((9, 13, 4), dtype=F)
    a.view(np.uint32)[..., 3] = dr.MISS
    b = np.zeros((9, 13, 4), dtype=F)
    b[..., 3] = np.inf
    for prefilter in (0, 1):
        got, got_v = check_equal(spt, c, m, a, b, 3, 7, prefilter=prefilter)
        v = gr.variance0(m, 3, 7)
        assert (v >= 0).all() and (v == 0).any()
        assert gr.bits_equal(got, c)
        assert gr.bits_equal(got_v, gr.prefilter(v) if prefilter else v)


# ---- the remaining host checks ------------------------------------------------------------------------------
def test_prefilter_on_and_off(spt, ref):
    args = inputs(spt, ref, "cornell", 97, 53, 8, FOUR_BY_TWO)
    on, on_v = check_equal(spt, *args, prefilter=1)
    off, off_v = check_equal(spt, *args, prefilter=0)
    assert not gr.bits_equal(on_v, off_v) and not gr.bits_equal(on, off)


@pytest.mark.parametrize("kw", [{"normal_power_log2": 0}, {"normal_power_log2": 7}, {"sigma_variance": 2.0},
                                {"sigma_variance": 8.0}, {"sigma_plane": 0.005}, {"sigma_plane": 0.5},
                                {"variance_floor": 1e-3}, {"levels": 6}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_parameters_reach_the_weights(spt, ref, kw):
    args = inputs(spt, ref, "cornell", 97, 53, 8, FOUR_BY_TWO)
    got, _ = check_equal(spt, *args, **kw)
    assert not gr.bits_equal(got, spt.atrous_guided_host(*args)[0])


def test_output_may_alias_the_input_and_variance_may_be_null(spt, ref):
    c, m, a, b, B, f = inputs(spt, ref, "cornell", 20, 12, 8, FOUR_BY_TWO)
    want, _ = spt.atrous_guided_host(c, m, a, b, B, f)
    buf = c.copy()
    fp = ctypes.c_void_p
    rc = spt.load_library().spt_atrous_guided_host(fp(buf.ctypes.data), fp(m.ctypes.data), fp(a.ctypes.data),
                                                   fp(b.ctypes.data), 20, 12, B, f, None, fp(buf.ctypes.data), None)
    assert rc == 0 and gr.bits_equal(buf, want)


def test_defaults(spt):
    p = spt.GuidedParams()
    assert (p.levels, p.sigma_variance, p.sigma_plane, p.normal_power_log2, p.variance_floor, p.prefilter) == \
        (5, 4.0, float(F(0.05)), 5, float(F(1e-8)), 1)
    assert list(p.reserved) == [0, 0]
    assert spt.load_library().spt_guided_params_default(None) == -1
    with pytest.raises(TypeError):
        spt.GuidedParams(no_such_field=1)


def test_struct_layout_matches_c(spt, tmp_path):
    src = tmp_path / "gd.c"
    fields = ["levels", "sigma_variance", "sigma_plane", "normal_power_log2", "variance_floor", "prefilter", "reserved"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spt.h"\nint main(void){'
                   'printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(spt_guided_params)'
                   + "".join(f", offsetof(spt_guided_params, {k})" for k in fields) + '); return 0;}\n')
    exe = tmp_path / "gd"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    G = spt.GuidedParams
    assert got == [ctypes.sizeof(G)] + [getattr(G, k).offset for k in fields]
    assert got == [32, 0, 4, 8, 12, 16, 20, 24]


INVALID = [{"levels": 0}, {"levels": 7}, {"sigma_variance": 0.0}, {"sigma_variance": -1.0},
           {"sigma_variance": float("nan")}, {"sigma_variance": float("inf")}, {"sigma_plane": 0.0},
           {"sigma_plane": -0.05}, {"sigma_plane": float("nan")}, {"sigma_plane": float("inf")},
           {"normal_power_log2": 8}, {"variance_floor": 0.0}, {"variance_floor": -1e-8},
           {"variance_floor": float("nan")}, {"variance_floor": float("inf")}, {"prefilter": 2}]


@pytest.mark.parametrize("kw", INVALID, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_parameters(spt, kw):
    z = np.zeros((2, 2, 4), dtype=F)
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        spt.atrous_guided_host(z, z, z, z, 2, 1, spt.GuidedParams(**kw))


@pytest.mark.parametrize("kw", [{"levels": 1}, {"levels": 6}, {"normal_power_log2": 0}, {"normal_power_log2": 7},
                                {"prefilter": 0}, {"prefilter": 1}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_range_ends_are_valid(spt, kw):
    z = np.zeros((2, 2, 4), dtype=F)
    spt.atrous_guided_host(z, z, z, z, 2, 1, spt.GuidedParams(**kw))


def test_invalid_reserved_counts_and_null_pointers(spt):
    lib = spt.load_library()
    z = np.zeros((2, 2, 4), dtype=F)
    out = np.zeros((2, 2, 4), dtype=F)
    var = np.zeros((2, 2), dtype=F)
    P = ctypes.c_void_p
    for word in range(2):
        p = spt.GuidedParams()
        p.reserved[word] = 1
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            spt.atrous_guided_host(z, z, z, z, 2, 1, p)
    for batches, frames in ((1, 1), (0, 1), (2, 0)):
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            spt.atrous_guided_host(z, z, z, z, batches, frames)
    zp = P(z.ctypes.data)
    ok = [zp, zp, zp, zp, 2, 2, 2, 1, None, P(out.ctypes.data), P(var.ctypes.data)]
    assert lib.spt_atrous_guided_host(*ok) == 0
    for k in (0, 1, 2, 3, 9):
        args = list(ok)
        args[k] = None
        assert lib.spt_atrous_guided_host(*args) == -1
    for k in (4, 5):
        args = list(ok)
        args[k] = 0
        assert lib.spt_atrous_guided_host(*args) == -1
    # the ctx calls refuse a null ctx before anything else
    assert lib.spt_denoise_guided(None, 1, None) == -1
    assert lib.spt_read_denoised_variance(None, None) == -1


def test_declared_functions_are_exported(spt):
    """include/spt.h's new declarations are in EXPORTED_SYMBOLS and in the library (test_capi_symbols.py checks
    the whole list; this names the new ones)."""
    lib = spt.load_library()
    for name in ("spt_guided_params_default", "spt_denoise_guided", "spt_read_denoised_variance", "spt_atrous_guided_host"):
        assert name in spt.EXPORTED_SYMBOLS and getattr(lib, name) is not None


# ---- the host function under the sanitizers -----------------------------------------------------------------
def test_host_function_under_sanitizers(spt, ref, tmp_path):
    """tests/cpp/guided_host_check.cpp with csrc/spt_host.cpp, built with AddressSanitizer and
    UndefinedBehaviorSanitizer into a program of its own (tests/host_program.py), over the 20 x 12 and the 1 x 1
    inputs; its results are the library's."""
    exe = host_program.build("guided_host_check", tmp_path)
    cases = [("small", inputs(spt, ref, "cornell", 20, 12, 8, FOUR_BY_TWO)),
             ("pixel", inputs(spt, ref, "one_sphere", 1, 1, 4, (1, 2)))]
    for name, (c, m, a, b, B, f) in cases:
        h, w = c.shape[:2]
        inp, out = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
        with open(inp, "wb") as fh:
            np.array([w, h, B, f], dtype=np.uint32).tofile(fh)
            for arr in (c, m, a, b):
                np.ascontiguousarray(arr, dtype=F).tofile(fh)
        r = subprocess.run([str(exe), str(inp), str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
        raw = np.fromfile(out, dtype=np.uint32)
        want, want_v = spt.atrous_guided_host(c, m, a, b, B, f)
        n = w * h
        assert raw.size == 5 * n
        assert np.array_equal(raw[:4 * n], want.view(np.uint32).reshape(-1))
        assert np.array_equal(raw[4 * n:], want_v.view(np.uint32).reshape(-1))


# ---- the definition's quality -------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,w,h,bounces,cap", [("cornell", 96, 54, 8, 0.6), ("c1", 64, 64, 4, 0.75),
                                                   ("app", 64, 64, 4, 0.8)])
def test_quality_after_eight_batches(spt, ref, scene, w, h, bounces, cap):
    """The definition after 8 batches of 8 frames from the oracle, default parameters: RMS error over RGB and
    pixels against the mean of frames 1000..3047. The guided image beats the plain filter's, and guided over noisy
    is at most `cap`. Measured when this was written (noisy / plain / guided, ratio):
    cornell 96x54 0.0661 / 0.0384 / 0.0284, 0.429;  c1 64x64 0.0079 / 0.0196 / 0.0045, 0.579;
    app 64x64 0.0105 / 0.0202 / 0.0067, 0.634."""
    c, m, a, b, B, f = inputs(spt, ref, scene, w, h, bounces, tuple(range(8, 65, 8)))
    assert (B, f) == (8, 64)
    prims, mats, env = spt.build_scene(scene)
    truth = ref.RefScene(prims, mats, env).render(w, h, 1000, 2048, bounces, 2, 0, threads=8) / F(2048.0)
    noisy = gr.rms(c, truth)
    plain = gr.rms(spt.atrous_host(c, a, b), truth)
    restated = gr.rms(gr.guided(c, m, a, b, B, f)[0], truth)
    product = gr.rms(spt.atrous_guided_host(c, m, a, b, B, f)[0], truth)
    print(f"{scene} {w}x{h}, 8 batches of 8: noisy rms {noisy:.4f}, plain {plain:.4f}, guided {product:.4f}, "
          f"guided / noisy {product / noisy:.3f}")
    assert product == restated
    assert product < plain
    assert product / noisy <= cap
