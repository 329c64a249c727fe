"""The noise estimate on the host (no GPU): the library's host functions (spt_noise_update_host,
spt_noise_meter_host, spt_noise_from_histogram: compiled from csrc/spt_noise.h, the header the kernels compile)
against the numpy restatement of include/spt.h's definition (tests/noise_ref.py), bit for bit, on the CPU oracle's
accumulations and on crafted moments; then the definition's quality against a 2048-frame render.

Quality figures of this restatement on the oracle (R: actual over estimated relative RMS error, noise_ref.py
quality_ratio): C1 0.97 per pixel / 1.03 pooled 3x3, the App's scene 0.98 / 1.09, Cornell 64 batches 1.30 / 1.07."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import host_program
import noise_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
RADII = [0, 1, 2]

_cache = {}


def app_spheres():
    """App::App's scene (src/App.cpp:101-123), as tests/cpp/display_backend.cpp builds it."""
    s = [(0.0, -1.0, 5.0, 1.0), (0.0, -102.0, 5.0, 100.0)]
    for x in range(-5, 6, 2):
        for y in range(-5, 6, 2):
            s.append((float(x), float(y), 10.0, 0.5))
    return s


def ref_scene(spt, ref, name):
    if ("scene", name) not in _cache:
        if name == "app":
            prims, mats, env = spt.sphere_prims(app_spheres()), spt.reference_materials(), spt.reference_env(True)
        else:
            prims, mats, env = spt.build_scene(name)
        _cache[("scene", name)] = ref.RefScene(prims, mats, env)
    return _cache[("scene", name)]


def accumulations(spt, ref, name, w, h, bounces, frame_counts):
    """The oracle's accumulation after each of frame_counts frames (computed once per sequence)."""
    key = (name, w, h, bounces, tuple(frame_counts))
    if key not in _cache:
        rs = ref_scene(spt, ref, name)
        _cache[key] = [rs.render(w, h, 0, fc, bounces, 2, 0, threads=8) for fc in frame_counts]
    return _cache[key]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=F).view(np.uint32), np.ascontiguousarray(b, dtype=F).view(np.uint32))


def lib_fold(spt, accums, frame_counts):
    m, before = None, 0
    for a, fc in zip(accums, frame_counts):
        m = spt.noise_update_host(a, fc - before, before, m)
        before = fc
    return m


def check_meter(spt, moments, batches, frames, radius, dark_floor=0.01):
    counts, e2 = spt.noise_meter_host(moments, batches, frames, spt.NoiseParams(radius=radius, dark_floor=dark_floor))
    want = nr.e2_image(moments, batches, frames, radius, dark_floor)
    assert same_bits(e2, want), (radius, np.argwhere(e2.view(np.uint32) != want.view(np.uint32))[:4])
    assert np.array_equal(counts, nr.histogram(want))
    assert int(counts.sum()) == want.size
    return counts, e2


SEQUENCES = [("cornell", 97, 53, 8, (1, 2, 3, 4, 5, 6)),  # six one-frame batches
             ("cornell", 97, 53, 8, (1, 4, 8)),           # batches of 1, 3 and 4 frames: unequal weights
             ("c1", 64, 64, 4, (1, 2, 3, 4))]             # sky beside hits


# ---- update and meter on the oracle's accumulations -----------------------------------------------------
@pytest.mark.parametrize("name,w,h,bounces,frame_counts", SEQUENCES)
def test_update_and_meter_on_oracle_sequences(spt, ref, name, w, h, bounces, frame_counts):
    accums = accumulations(spt, ref, name, w, h, bounces, frame_counts)
    m_lib, m_ref, before = None, None, 0
    for k, (a, fc) in enumerate(zip(accums, frame_counts)):
        m_lib = spt.noise_update_host(a, fc - before, before, m_lib)
        m_ref = nr.update(a, fc - before, before, m_ref)
        assert same_bits(m_lib, m_ref), (name, k)
        before = fc
        if k >= 1:
            for radius in RADII:
                check_meter(spt, m_lib, k + 1, float(fc), radius)
    assert np.all(m_lib[..., 3] == 0) and same_bits(m_lib[..., 2], nr.luminance(accums[-1]))
    # West's update is the weighted mean and sum of squares of the batch means (in double, to rounding)
    L = [nr.luminance(a).astype(np.float64) for a in accums]
    ws = np.diff(np.array((0,) + tuple(frame_counts), dtype=np.float64))
    ds = [(L[k] - (L[k - 1] if k else 0.0)) / ws[k] for k in range(len(L))]
    mean = sum(w_ * d for w_, d in zip(ws, ds)) / ws.sum()
    m2 = sum(w_ * (d - mean) ** 2 for w_, d in zip(ws, ds))
    assert np.allclose(m_lib[..., 0], mean, rtol=1e-5, atol=1e-6)
    assert np.allclose(m_lib[..., 1], m2, rtol=1e-3, atol=1e-6)


def test_sky_pixels_have_no_noise(spt, ref):
    """C1's sky pixels take the same value every frame: their error is the sums' rounding, a relative 1e-7 at the
    most (e2 below 1e-13), far below any pixel that scatters."""
    accums = accumulations(spt, ref, "c1", 64, 64, 4, (1, 2, 3, 4))
    m = lib_fold(spt, accums, (1, 2, 3, 4))
    counts, e2 = spt.noise_meter_host(m, 4, 4.0, spt.NoiseParams(radius=0))
    first = accums[0].astype(np.float64)
    still = np.all([np.abs(accums[k] / (k + 1.0) - first) <= 1e-6 * first for k in (1, 2, 3)], axis=0).all(axis=-1)
    assert 0 < still.sum() < still.size
    assert np.all(e2[still] < 1e-13) and np.median(e2[~still]) > 1e-4


@pytest.mark.parametrize("w,h", [(2, 2), (1, 1), (5, 3)])
def test_clipped_windows(spt, w, h):
    """2 x 2 at radius 2: every window is clipped to the whole image; 1 x 1: one tap."""
    rng = np.random.default_rng(w * 10 + h)
    m = np.zeros((h, w, 4), dtype=F)
    m[..., 0] = rng.uniform(0.05, 2.0, (h, w))
    m[..., 1] = rng.uniform(0.0, 0.5, (h, w))
    for radius in RADII:
        _, e2 = check_meter(spt, m, 3, 7.0, radius)
    if (w, h) == (2, 2):  # every pixel pools the same four taps in the same order
        assert np.unique(e2.view(np.uint32)).size == 1


# ---- crafted moments --------------------------------------------------------------------------------------
def moments_with_e2(values):
    """Moments whose radius-0 e2 is exactly `values` with B = 2, W = 1 and dark_floor 0: inv = 1, mean = 1."""
    v = np.asarray(values, dtype=F)
    m = np.zeros((1, v.size, 4), dtype=F)
    m[0, :, 0] = 1.0
    m[0, :, 1] = v
    return m


def test_every_bin_edge(spt):
    edges = np.array([nr.bin_lower_edge(b) for b in range(1, nr.BINS)], dtype=F)
    below = np.nextafter(edges, F(0))
    values = np.concatenate([edges, below])
    counts, e2 = spt.noise_meter_host(moments_with_e2(values), 2, 1.0, spt.NoiseParams(radius=0, dark_floor=0.0))
    assert same_bits(e2.reshape(-1), values)
    want_bins = np.concatenate([np.arange(1, nr.BINS), np.arange(0, nr.BINS - 1)])
    assert np.array_equal(nr.noise_bin(values), want_bins)
    assert np.array_equal(counts, np.bincount(want_bins, minlength=nr.BINS))
    # by hand: bin 0 ends below 2^-28 * 1.125, bin 255 starts at 15
    assert nr.bin_lower_edge(1) == F(2.0 ** -28 * 1.125) and nr.bin_lower_edge(255) == F(15.0)
    assert nr.bin_lower_edge(0) == F(2.0 ** -28)


def test_special_values(spt):
    nan, inf = float("nan"), float("inf")
    #            mean   m2
    cases = [(1.0, nan), (nan, 1.0), (1.0, inf), (1.0, -inf), (inf, 1.0), (inf, inf), (1.0, 0.0), (1.0, -0.0),
             (1.0, -0.25), (-1.0, 0.25), (-0.01, 1.0), (0.0, 0.0), (1.0, 1e-45), (1e-30, 1e-30), (1.0, 3.0e38)]
    m = np.zeros((3, 5, 4), dtype=F)
    m.reshape(-1, 4)[:, :2] = np.array(cases, dtype=F)
    for radius in RADII:
        counts, e2 = check_meter(spt, m, 2, 1.0, radius)
    counts, e2 = spt.noise_meter_host(m, 2, 1.0, spt.NoiseParams(radius=0))
    bins = nr.noise_bin(e2).reshape(-1)
    # NaN and +inf: the last bin; zero and negatives: bin 0; a negative mean below -dark_floor is squared away;
    # mean = -dark_floor divides by zero: +inf
    assert list(bins[:6]) == [255, 255, 255, 0, 0, 255]
    assert list(bins[6:9]) == [0, 0, 0] and bins[10] == 255
    t = F(-1.0) + F(0.01)
    assert bins[9] == nr.noise_bin(F(0.25) / (t * t)) and bins[9] > 0
    assert np.isnan(e2.reshape(-1)[[0, 1, 5]]).all()


def test_random_moments(spt):
    rng = np.random.default_rng(5)
    for w, h in ((17, 33), (33, 17), (64, 16), (65, 17)):
        m = np.zeros((h, w, 4), dtype=F)
        m[..., 0] = np.exp2(rng.uniform(-12, 4, (h, w)))
        m[..., 1] = np.exp2(rng.uniform(-40, 8, (h, w))) * (rng.random((h, w)) > 0.1)
        for radius in RADII:
            check_meter(spt, m, 9, 36.0, radius, dark_floor=0.25)


# ---- the stop rule --------------------------------------------------------------------------------------
def test_from_histogram(spt):
    z = np.zeros(nr.BINS, dtype=np.uint32)
    assert spt.noise_from_histogram(z) == 0.0 == nr.from_histogram(z)
    c = z.copy()
    c[0] = 1000
    assert spt.noise_from_histogram(c) == 0.0 == nr.from_histogram(c)
    c = z.copy()
    c[255] = 1000
    assert spt.noise_from_histogram(c) == math.inf == nr.from_histogram(c)
    c = z.copy()
    c[100], c[140] = 950, 50  # the quantile is reached exactly at the end of bin 100
    lo, hi = math.sqrt(float(nr.bin_lower_edge(101))), math.sqrt(float(nr.bin_lower_edge(141)))
    assert spt.noise_from_histogram(c, 0.95) == lo == nr.from_histogram(c, 0.95)
    c[100], c[140] = 949, 51  # one pixel short: the upper bin decides
    assert spt.noise_from_histogram(c, 0.95) == hi == nr.from_histogram(c, 0.95)
    assert spt.noise_from_histogram(c, 0.5) == lo and spt.noise_from_histogram(c, 1.0) == hi
    # the upper edge: every e2 of the bin is at most the result squared
    assert abs(lo ** 2 - float(nr.bin_lower_edge(101))) <= 1e-12 * lo ** 2
    rng = np.random.default_rng(3)
    for _ in range(50):
        c = (rng.integers(0, 1000, nr.BINS) * (rng.random(nr.BINS) > 0.5)).astype(np.uint32)
        q = float(rng.uniform(0.01, 1.0))
        assert spt.noise_from_histogram(c, q) == nr.from_histogram(c, q)
    for q in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            spt.noise_from_histogram(z, q)


# ---- validation ---------------------------------------------------------------------------------------------
def test_defaults_and_struct_size(spt, tmp_path):
    p = spt.NoiseParams()
    assert (p.radius, p.dark_floor, list(p.reserved)) == (1, F(0.01), [0, 0]) and spt.NOISE_BINS == 256
    with pytest.raises(TypeError):
        spt.NoiseParams(no_such_field=1)
    # the struct as the C compiler lays it out
    src, exe = tmp_path / "size.c", tmp_path / "size"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spt.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(spt_noise_params), offsetof(spt_noise_params, radius),\n'
                   '         offsetof(spt_noise_params, dark_floor), offsetof(spt_noise_params, reserved));\n'
                   '  return 0;\n}\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(p), spt.NoiseParams.radius.offset, spt.NoiseParams.dark_floor.offset,
                   spt.NoiseParams.reserved.offset] == [16, 0, 4, 8]


def test_validation(spt):
    m = np.ones((3, 4, 4), dtype=F)
    ok = spt.NoiseParams()
    assert spt.noise_meter_host(m, 2, 2.0, ok)[0].sum() == 12
    bad_reserved = spt.NoiseParams()
    bad_reserved.reserved[1] = 1
    for p in (spt.NoiseParams(radius=3), spt.NoiseParams(dark_floor=-0.5), spt.NoiseParams(dark_floor=float("nan")),
              spt.NoiseParams(dark_floor=float("inf")), bad_reserved):
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            spt.noise_meter_host(m, 2, 2.0, p)
    for batches, frames in ((1, 2.0), (0, 2.0), (2, 0.0), (2, 2.5), (2, 2.0 ** 24 + 2), (2, float("nan")), (2, -1.0)):
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            spt.noise_meter_host(m, batches, frames, ok)
    assert spt.noise_meter_host(m, 2, 2.0 ** 24, ok)[0].sum() == 12
    a = np.ones((3, 4, 4), dtype=F)
    for w, before in ((0.0, 0.0), (0.5, 0.0), (1.5, 1.0), (-1.0, 2.0), (1.0, 0.5), (1.0, 2.0 ** 24), (2.0 ** 24, 1.0),
                      (float("nan"), 0.0)):
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            spt.noise_update_host(a, w, before, a)
    assert spt.noise_update_host(a, 1.0, 2.0 ** 24 - 1, a).shape == a.shape
    with pytest.raises(ValueError):
        spt.noise_update_host(a, 1.0, 1.0)  # moments are needed after the first batch
    # the first batch ignores what the moments held
    assert same_bits(spt.noise_update_host(a, 2.0, 0.0, np.full_like(a, 7.0)), spt.noise_update_host(a, 2.0))


# ---- the definition's quality ---------------------------------------------------------------------------------
def quality(spt, ref, name, w, h, bounces, batches):
    fcs = tuple(range(1, batches + 1))
    accums = accumulations(spt, ref, name, w, h, bounces, fcs)
    m = lib_fold(spt, accums, fcs)
    truth = nr.luminance(ref_scene(spt, ref, name).render(w, h, 0, 2048, bounces, 2, 0, threads=8)).astype(np.float64) / 2048
    out = []
    for radius in (0, 1):
        _, e2 = spt.noise_meter_host(m, batches, float(batches), spt.NoiseParams(radius=radius))
        out.append(nr.quality_ratio(e2, m[..., 0], truth))
    print(f"noise quality {name} {w}x{h}, {batches} one-frame batches: R per pixel {out[0]:.3f}, pooled 3x3 {out[1]:.3f}")
    return out


@pytest.mark.parametrize("name", ["c1", "app"])
def test_quality_sphere_scenes(spt, ref, name):
    per_pixel, pooled = quality(spt, ref, name, 64, 64, 4, 32)
    assert 0.7 <= per_pixel <= 1.4 and 0.7 <= pooled <= 1.4


def test_quality_cornell(spt, ref):
    per_pixel, pooled = quality(spt, ref, "cornell", 96, 54, 8, 64)
    assert per_pixel <= 1.6 and pooled <= 1.3


# ---- the host functions under the sanitizers --------------------------------------------------------------
def test_host_functions_under_sanitizers(spt, ref, tmp_path):
    """tests/cpp/noise_host_check.cpp with csrc/spt_host.cpp, built with AddressSanitizer and
    UndefinedBehaviorSanitizer into a program of its own (tests/host_program.py), over a 2 x 2 image and a
    97 x 53 sequence of the oracle's; its results are the library's."""
    exe = host_program.build("noise_host_check", tmp_path)
    rng = np.random.default_rng(1)
    small = [np.cumsum(rng.uniform(0.0, 1.0, (2, 2, 4)).astype(F), axis=0, dtype=F) * F(k + 1) for k in range(3)]
    cases = [("small", small, (1, 2, 3)),
             ("cornell", accumulations(spt, ref, "cornell", 97, 53, 8, (1, 4, 8)), (1, 4, 8))]
    for name, accums, fcs in cases:
        h, w = accums[0].shape[:2]
        inp, out = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
        with open(inp, "wb") as f:
            np.array([w, h, len(fcs)] + list(fcs), dtype=np.uint32).tofile(f)
            for a in accums:
                np.ascontiguousarray(a, dtype=F).tofile(f)
        r = subprocess.run([str(exe), str(inp), str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
        raw = np.fromfile(out, dtype=np.uint32)
        m = lib_fold(spt, accums, fcs)
        n = w * h
        assert np.array_equal(raw[:4 * n], m.view(np.uint32).reshape(-1))
        at = 4 * n
        for radius in RADII:
            counts, e2 = spt.noise_meter_host(m, len(fcs), float(fcs[-1]), spt.NoiseParams(radius=radius))
            assert np.array_equal(raw[at:at + 256], counts)
            assert np.array_equal(raw[at + 256:at + 256 + n], e2.view(np.uint32).reshape(-1))
            at += 256 + n
        assert at == raw.size
