"""The luminance meter, the exposure from its histogram and the display transform on the host (no GPU): the
library's host functions (compiled from csrc/spt_display.h, the header the kernels compile) against the numpy
restatement of include/spt.h's definition (tests/display_ref.py). Bins, histograms and display bytes bit for bit;
the exposure to one unit in the last place of the float result (its double-precision log2 / exp2 may differ
between libm and numpy by parts in 10^15, which can move only the single final rounding)."""
import ctypes

import numpy as np
import pytest

import display_ref as dr

F = np.float32
OPERATORS = [dr.CLAMP, dr.REINHARD, dr.ACES]


def lib_bins(spt, values):
    lib, out = spt.load_library(), ctypes.c_uint32(0)
    got = np.empty(values.size, dtype=np.int64)
    for i, b in enumerate(values.view(np.uint32).tolist()):
        assert lib.spt_meter_bin(ctypes.c_float.from_buffer_copy(b.to_bytes(4, "little")), ctypes.byref(out)) == 0
        got[i] = out.value
    return got


def ulps(a, b):
    return abs(int(np.array(a, dtype=F).view(np.int32)) - int(np.array(b, dtype=F).view(np.int32)))


# ---- the bin ------------------------------------------------------------------------------------------
def test_meter_bin_boundaries_and_special_values(spt):
    values = np.concatenate([dr.key_boundaries(), dr.special_values()])
    want = dr.meter_bin(values)
    assert np.array_equal(lib_bins(spt, values), want)
    assert np.array_equal(np.unique(want), np.arange(dr.BINS))  # every bin is produced
    # by hand: bin 1 starts at 2^-16 * 1.125, bin 255 at 2^15 * 1.875; 0.18 = 2^-3 * 1.44 is key 995
    assert spt.meter_bin(F(2.0 ** -16 * 1.125)) == 1 and spt.meter_bin(np.nextafter(F(2.0 ** -16 * 1.125), F(0))) == 0
    assert spt.meter_bin(F(2.0 ** 15 * 1.875)) == 255 and spt.meter_bin(np.nextafter(F(2.0 ** 15 * 1.875), F(0))) == 254
    assert spt.meter_bin(0.18) == 995 - 888
    for v in (0.0, -0.0, -1.0, float("nan"), -float("nan"), -float("inf"), 1e-45, 1e-39):
        assert spt.meter_bin(v) == 0, v
    assert spt.meter_bin(float("inf")) == 255


def test_meter_bin_random_bit_patterns(spt):
    values = dr.random_bits(1 << 20, 11)
    assert np.array_equal(lib_bins(spt, values), dr.meter_bin(values))


# ---- the histogram --------------------------------------------------------------------------------------
@pytest.mark.parametrize("divisor", [1.0, 7.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5141])
def test_histogram_random_images(spt, n, divisor):
    for img in (dr.random_image(n, n), dr.random_bits(4 * n, n + 1).reshape(n, 4)):
        want = dr.histogram(img, divisor)
        assert int(want.sum()) == n
        assert np.array_equal(spt.luminance_histogram_host(img, divisor), want)


def test_histogram_black_repeated_and_special(spt):
    black = np.zeros((300, 4), dtype=F)
    got = spt.luminance_histogram_host(black)
    assert got[0] == 300 and got[1:].sum() == 0 and np.array_equal(got, dr.histogram(black))
    same = np.tile(np.array([[0.3, 0.5, 0.1, 1.0]], dtype=F), (777, 1))
    got = spt.luminance_histogram_host(same, 3.0)
    assert got.max() == 777 and np.array_equal(got, dr.histogram(same, 3.0))
    for values in (dr.key_boundaries(), dr.special_values()):
        img = dr.grey(values)
        assert np.array_equal(spt.luminance_histogram_host(img), dr.histogram(img))
    assert spt.luminance_histogram_host(np.zeros((4, 5, 4), dtype=F)).sum() == 20  # any leading shape


# ---- the display transform --------------------------------------------------------------------------------
def display_inputs():
    ramp = np.concatenate([np.linspace(0.0, 2.0, 8193), np.geomspace(2.0, 1.0e5, 8192)]).astype(F)
    thresholds = (np.arange(257, dtype=np.float64) / 255.0).astype(F)  # CLAMP's steps with their neighbours
    steps = np.concatenate([np.nextafter(thresholds, F(-1)), thresholds, np.nextafter(thresholds, F(2))])
    return {"random": dr.random_image(5141, 5), "bits": dr.random_bits(4 * 5141, 6).reshape(-1, 4),
            "ramp": dr.grey(np.concatenate([ramp, steps])), "special": dr.grey(dr.special_values()),
            "special alpha": np.stack([dr.special_values()] * 4, axis=1)}


@pytest.mark.parametrize("exposure", [0.0, 1.0, 3.5])
@pytest.mark.parametrize("tonemap", OPERATORS)
def test_display_host_matches_the_restatement(spt, tonemap, exposure):
    for name, img in display_inputs().items():
        for divisor in (1.0, 7.0):
            got = spt.display_host(img, spt.Display(tonemap, exposure), divisor)
            want = dr.display(img, tonemap, exposure, divisor)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (name, divisor, bad[:5], [hex(int(v)) for v in got[bad[:5]]],
                                   [hex(int(v)) for v in want[bad[:5]]], img[bad[:5]])


def test_display_ramp_crosses_every_threshold(spt):
    ramp = display_inputs()["ramp"]
    for tonemap, top in ((dr.CLAMP, 255), (dr.ACES, 255), (dr.REINHARD, 254)):  # 65536 / 65537 stays below 1
        red = spt.display_host(ramp, spt.Display(tonemap, 1.0)) >> 24
        assert np.array_equal(np.unique(red), np.arange(top + 1)), tonemap


@pytest.mark.parametrize("exposure", [1.0, 2.5])
def test_clamp_is_the_plain_resolve(spt, exposure):
    for name, img in display_inputs().items():
        for frames in (1.0, 7.0):
            got = spt.display_host(img, spt.Display(spt.TONEMAP_CLAMP, exposure), frames)
            assert np.array_equal(got, dr.resolve_rgba8(img, frames, exposure)), (name, frames)


# ---- the exposure -----------------------------------------------------------------------------------------
def counts_of(**bins):
    c = np.zeros(dr.BINS, dtype=np.uint32)
    for b, n in bins.items():
        c[int(b[1:])] = n
    return c


def test_exposure_one_bin_by_hand(spt):
    b = spt.meter_bin(0.18)  # key 995: e = -3, k = 3: the centre is 2^-3 * (1 + 3.5 / 8)
    got = spt.exposure_from_histogram(counts_of(**{f"b{b}": 1000}))
    assert ulps(got, F(0.18) / F(0.125 * (1.0 + 3.5 / 8.0))) <= 1
    assert ulps(got, dr.exposure(counts_of(**{f"b{b}": 1000}))) <= 1
    # a black border does not count
    assert got == spt.exposure_from_histogram(counts_of(b0=123456, **{f"b{b}": 1000}))


def test_exposure_cuts_inside_bins(spt):
    counts = counts_of(b100=50, b120=50)  # lo = 10 and hi = 98 fall inside the two bins: weights 40 and 48
    want = F(0.18 / 2.0 ** ((40 * dr.bin_centre(100) + 48 * dr.bin_centre(120)) / 88.0))
    got = spt.exposure_from_histogram(counts)
    assert ulps(got, want) <= 1 and ulps(got, dr.exposure(counts)) <= 1
    spread = np.random.default_rng(3).integers(0, 5000, size=dr.BINS).astype(np.uint32)
    for kw in ({}, {"low_fraction": 0.0, "high_fraction": 0.0}, {"low_fraction": 0.45, "high_fraction": 0.45},
               {"target_luminance": 0.5}):
        got = spt.exposure_from_histogram(spread, spt.ExposureParams(**kw))
        want = dr.exposure(spread, kw.get("target_luminance", 0.18), kw.get("low_fraction", 0.1), kw.get("high_fraction", 0.02))
        assert ulps(got, want) <= 1, kw
    big = np.full(dr.BINS, 0xFFFFFFFF, dtype=np.uint32)  # the sum needs more than 32 bits
    assert ulps(spt.exposure_from_histogram(big), dr.exposure(big)) <= 1


def test_exposure_black_and_limits(spt):
    assert spt.exposure_from_histogram(np.zeros(dr.BINS, dtype=np.uint32)) == 1.0
    assert spt.exposure_from_histogram(counts_of(b0=99)) == 1.0
    assert spt.exposure_from_histogram(counts_of(b250=10)) == 0.015625 == float(dr.exposure(counts_of(b250=10)))
    assert spt.exposure_from_histogram(counts_of(b3=10)) == 64.0 == float(dr.exposure(counts_of(b3=10)))
    p = spt.ExposureParams(min_exposure=0.5, max_exposure=2.0)
    assert spt.exposure_from_histogram(counts_of(b250=10), p) == 0.5
    assert spt.exposure_from_histogram(counts_of(b3=10), p) == 2.0


def test_defaults(spt):
    p = spt.ExposureParams()
    assert (p.target_luminance, p.low_fraction, p.high_fraction, p.min_exposure, p.max_exposure) == \
        (F(0.18), F(0.1), F(0.02), 0.015625, 64.0)
    assert list(p.reserved) == [0, 0, 0] and ctypes.sizeof(p) == 32
    d = spt.Display()
    assert (d.tonemap, d.exposure, list(d.reserved)) == (spt.TONEMAP_CLAMP, 1.0, [0, 0]) and ctypes.sizeof(d) == 16
    assert (spt.TONEMAP_CLAMP, spt.TONEMAP_REINHARD, spt.TONEMAP_ACES) == (0, 1, 2)
    assert (spt.IMAGE_ACCUM, spt.IMAGE_DENOISED, spt.IMAGE_BLENDED) == (0, 1, 2) and spt.METER_BINS == 256
    with pytest.raises(TypeError):
        spt.ExposureParams(no_such_field=1)


def test_invalid_arguments(spt):
    lib = spt.load_library()
    counts = counts_of(b100=5)
    nan, inf = float("nan"), float("inf")
    bad = [{"target_luminance": 0.0}, {"target_luminance": -1.0}, {"target_luminance": nan}, {"target_luminance": inf},
           {"min_exposure": 0.0}, {"max_exposure": 0.0}, {"min_exposure": -1.0}, {"max_exposure": inf},
           {"min_exposure": 2.0, "max_exposure": 1.0}, {"low_fraction": -0.1}, {"high_fraction": -0.1},
           {"low_fraction": nan}, {"high_fraction": inf}, {"low_fraction": 0.5, "high_fraction": 0.5},
           {"low_fraction": 0.75, "high_fraction": 0.5}]
    for kw in bad:
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            spt.exposure_from_histogram(counts, spt.ExposureParams(**kw))
    p = spt.ExposureParams()
    p.reserved[2] = 1
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        spt.exposure_from_histogram(counts, p)
    e = ctypes.c_float(0.0)
    assert lib.spt_exposure_from_histogram(None, None, ctypes.byref(e)) == -1
    assert lib.spt_exposure_from_histogram(counts.ctypes.data_as(ctypes.c_void_p), None, None) == -1
    assert lib.spt_exposure_params_default(None) == -1
    assert lib.spt_meter_bin(1.0, None) == -1

    img = np.ones((3, 4), dtype=F)
    out = np.zeros(3, dtype=np.uint32)
    hist = np.zeros(dr.BINS, dtype=np.uint32)
    ip, op, hp = (ctypes.c_void_p(a.ctypes.data) for a in (img, out, hist))
    assert lib.spt_luminance_histogram_host(None, 3, 1.0, hp) == -1
    assert lib.spt_luminance_histogram_host(ip, 3, 1.0, None) == -1
    assert lib.spt_luminance_histogram_host(ip, 0, 1.0, hp) == -1
    for divisor in (0.0, -1.0, nan, inf):
        assert lib.spt_luminance_histogram_host(ip, 3, divisor, hp) == -1
        assert lib.spt_display_host(ip, 3, divisor, ctypes.byref(spt.Display()), op) == -1
    d = spt.Display()
    assert lib.spt_display_host(None, 3, 1.0, ctypes.byref(d), op) == -1
    assert lib.spt_display_host(ip, 3, 1.0, None, op) == -1
    assert lib.spt_display_host(ip, 3, 1.0, ctypes.byref(d), None) == -1
    assert lib.spt_display_host(ip, 0, 1.0, ctypes.byref(d), op) == -1
    assert lib.spt_display_host(ip, 3, 1.0, ctypes.byref(d), op) == 0
    for tonemap, exposure in ((3, 1.0), (0xFFFFFFFF, 1.0), (0, -1.0), (1, nan), (2, inf)):
        assert lib.spt_display_host(ip, 3, 1.0, ctypes.byref(spt.Display(tonemap, exposure)), op) == -1
    d.reserved[1] = 7
    assert lib.spt_display_host(ip, 3, 1.0, ctypes.byref(d), op) == -1
    # the ctx entry points refuse a null ctx before anything else
    assert lib.spt_meter_luminance(None, 0, 1, hp) == -1
    assert lib.spt_meter_device_image(None, ip, 3, 1.0, hp) == -1
    assert lib.spt_resolve_display_rgba8(None, 0, 1, ctypes.byref(spt.Display()), op) == -1
    assert lib.spt_resolve_display_device_image(None, ip, 3, 1.0, ctypes.byref(spt.Display()), op) == -1
    assert lib.spt_set_meter_form(None, 0) == -1


# ---- the settings mirror ----------------------------------------------------------------------------------
def test_render_settings_auto_exposure(spt):
    s = spt.RenderSettings()
    assert s.getAutoExposure() is False and s.getTargetLuminance() == 0.18
    s.clearDirty()
    s.setAutoExposure(False)  # nothing changes: not dirty
    assert not s.isDirty()
    s.setAutoExposure(True)
    assert s.isDirty() and s.getAutoExposure() is True and s.getTargetLuminance() == 0.18
    s.clearDirty()
    s.setAutoExposure(True, 0.18)
    assert not s.isDirty()
    s.setAutoExposure(True, 0.25)
    assert s.isDirty() and s.getTargetLuminance() == 0.25
    s.clearDirty()
    s.setAutoExposure(False, 0.25)
    assert s.isDirty() and s.getAutoExposure() is False and s.getTargetLuminance() == 0.25
