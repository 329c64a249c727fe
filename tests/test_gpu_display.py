"""The luminance meter and the display resolve on the GPU, bit for bit against the library's host functions
(spt_luminance_histogram_host / spt_display_host, compiled from the header the kernels compile), which
tests/test_display_host.py ties to the numpy restatement of include/spt.h's definition.

Kernels (csrc/spt_display.hip): k_meter runs blocks of four waves, a thread taking four pixels 256 apart per step
(1024 pixels a block), on a grid capped at 256 blocks: 1 and 63 pixels are a partial wave, 65, 255 and 257 a
partial run of 256, 5141 = 5 * 1024 + 21 several blocks with a partial one, and 1920 x 1080 (2025 blocks' worth)
runs the stride loop; both forms of the LDS sum are run. k_display runs 256-pixel blocks."""
import os
import subprocess

import numpy as np
import pytest

import display_ref as dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FORMS = [0, 1]
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5141]
BOUNCES = {"cornell": 8}

_scenes = {}


def scene_of(spt, name):
    if name not in _scenes:
        if name == "one_sphere":  # the 1x1 image's only ray (its pixel's corner: up and left) hits it
            _scenes[name] = (spt.sphere_prims([(-3.0, 3.0, 3.0, 1.0)]), spt.reference_materials(), spt.reference_env(True))
        else:
            _scenes[name] = spt.build_scene(name)
    return _scenes[name]


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """The crafted device images are torch tensors, and torch's copy of the HIP runtime finds the GPU only if it
    looks before the library's copy has opened it (as in tests/test_gpu_split_streams.py): so torch looks before
    this module's first ctx."""
    import torch

    torch.cuda.is_available()


@pytest.fixture(scope="module")
def ctx(spt, torch_first):
    c = spt.Context(0)
    yield c
    c.close()


def on_device(img):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(img, dtype=F).reshape(-1, 4)).cuda()
    torch.cuda.synchronize()
    return t


def bin_value(b):
    """A luminance in the middle of bin b (1..255)."""
    return F(2.0 ** dr.bin_centre(b))


def crafted(n, kind):
    if kind == "special":  # every special value and key boundary, repeated over the image
        v = np.concatenate([dr.special_values(), dr.key_boundaries()])
        return dr.grey(np.resize(v, n))
    if kind == "repeated":  # the worst contention: every lane of every wave in one bin
        return np.tile(np.array([[0.3, 0.5, 0.1, 1.0]], dtype=F), (n, 1))
    if kind == "bits":
        return dr.random_bits(4 * n, n).reshape(n, 4)
    if kind == "two_bins":  # each wave holds exactly two bins, other ones from wave to wave
        i = np.arange(n)
        b = 1 + (2 * (i // 64) + (i % 64) // 32) % 255
        return dr.grey(np.array([bin_value(k) for k in range(256)], dtype=F)[b])
    if kind == "all_differ":  # the lanes of every wave in 64 bins of their own (64 peel rounds)
        i = np.arange(n)
        b = 1 + (i % 64) * 3 + (i // 64) % 3
        return dr.grey(np.array([bin_value(k) for k in range(256)], dtype=F)[b])
    raise KeyError(kind)


def check_meter(spt, ctx, img, divisor, what):
    want = spt.luminance_histogram_host(img, divisor)
    t = on_device(img)
    for form in FORMS:
        ctx.set_meter_form(form)
        got = ctx.meter_device_image(t.data_ptr(), t.shape[0], divisor)
        assert np.array_equal(got, want), (what, form, np.flatnonzero(got != want)[:8])
    ctx.set_meter_form(-1)
    assert np.array_equal(ctx.meter_device_image(t.data_ptr(), t.shape[0], divisor), want), (what, "default")
    return want


# ---- k_meter on crafted images -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["special", "repeated", "bits", "two_bins"])
@pytest.mark.parametrize("n", SIZES)
def test_meter_device_image(spt, ctx, n, kind):
    img = crafted(n, kind)
    divisor = 3.0 if kind in ("special", "repeated") else 1.0
    want = check_meter(spt, ctx, img, divisor, (kind, n))
    assert int(want.sum()) == n
    if kind == "two_bins":
        bins = dr.meter_bin(dr.luminance(img, divisor))
        for w in range(0, n, 64):
            assert np.unique(bins[w:w + 64]).size == (2 if n - w > 32 else 1)


def test_meter_partial_last_wave_all_lanes_differ(spt, ctx):
    """64 * 5 + 37 pixels: the last wave is partial and every lane of every wave holds a bin of its own, so the
    peel form runs as many rounds as the wave has active lanes."""
    n = 64 * 5 + 37
    img = crafted(n, "all_differ")
    bins = dr.meter_bin(dr.luminance(img, 1.0))
    for w in range(0, n, 64):
        assert np.unique(bins[w:w + 64]).size == min(64, n - w)
    check_meter(spt, ctx, img, 1.0, "all_differ")


def test_meter_1080p_runs_the_stride_loop(spt, ctx):
    n = 1920 * 1080  # 2025 blocks' worth of pixels on a grid of 256
    img = dr.random_image(n, 7)
    want = check_meter(spt, ctx, img, 1.0, "1080p")
    assert int(want.sum()) == n and np.count_nonzero(want) == dr.BINS


def test_meter_device_image_errors(spt, ctx):
    t = on_device(np.ones((4, 4), dtype=F))
    for n, divisor in ((0, 1.0), (4, 0.0), (4, -1.0), (4, float("nan")), (4, float("inf"))):
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            ctx.meter_device_image(t.data_ptr(), n, divisor)
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            ctx.resolve_display_device_image(t.data_ptr(), n, spt.Display(), divisor)
    with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
        ctx.meter_device_image(0, 4, 1.0)
    for form in (2, -2):
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            ctx.set_meter_form(form)


# ---- the ctx's images ----------------------------------------------------------------------------------
def meter_both(spt, ctx, frame_count, image, img, divisor, what):
    want = spt.luminance_histogram_host(img, divisor)
    for form in FORMS + [-1]:
        ctx.set_meter_form(form)
        got = ctx.meter_luminance(frame_count, image)
        assert np.array_equal(got, want), (what, form, np.flatnonzero(got != want)[:8])
    return want


def check_display(spt, ctx, frame_count, image, img, divisor, what):
    n = ctx.shard_pixels
    reg = np.zeros(n, dtype=np.uint32)
    for tonemap in (spt.TONEMAP_CLAMP, spt.TONEMAP_REINHARD, spt.TONEMAP_ACES):
        d = spt.Display(tonemap, 1.75)
        want = spt.display_host(img, d, divisor)
        got = ctx.resolve_display_rgba8(frame_count, d, image)  # through the ctx's staging image
        assert np.array_equal(got, want), (what, tonemap, "staging")
        ctx.register_host_output(reg)
        try:
            reg[:] = 0
            out = ctx.resolve_display_rgba8(frame_count, d, image, out=reg)  # the kernel writes host memory
            assert out is reg and np.array_equal(reg, want), (what, tonemap, "registered")
        finally:
            ctx.register_host_output(None)


@pytest.mark.parametrize("name,w,h", [("cornell", 97, 53), ("cornell", 64, 64), ("one_sphere", 1, 1)])
def test_rendered_images(spt, ctx, name, w, h):
    """The accumulation after 1 and 8 frames, the denoised and the blended image: metered in both forms and
    resolved with the three operators, through staging and through the registered buffer."""
    prims, mats, env = scene_of(spt, name)
    ctx.set_scene(prims, mats, env)
    ctx.configure(w, h, BOUNCES.get(name, 4), 2, 0)
    ctx.set_camera(None)
    ctx.render(0, 1)
    acc = ctx.read_accum()
    meter_both(spt, ctx, 1, spt.IMAGE_ACCUM, acc, 1.0, (name, w, h, "1 frame"))
    ctx.render(1, 7)
    acc = ctx.read_accum()
    hist = meter_both(spt, ctx, 8, spt.IMAGE_ACCUM, acc, 8.0, (name, w, h, "8 frames"))
    assert int(hist.sum()) == w * h
    check_display(spt, ctx, 8, spt.IMAGE_ACCUM, acc, 8.0, (name, w, h, "accum"))
    for exposure in (1.0, 2.5):  # CLAMP is the plain resolve, byte for byte
        assert np.array_equal(ctx.resolve_display_rgba8(8, spt.Display(spt.TONEMAP_CLAMP, exposure)),
                              ctx.resolve_rgba8(8, exposure))
    ctx.denoise(8)
    den = ctx.read_denoised()
    meter_both(spt, ctx, 0, spt.IMAGE_DENOISED, den, 1.0, (name, w, h, "denoised"))  # (the frame count is ignored)
    check_display(spt, ctx, 0, spt.IMAGE_DENOISED, den, 1.0, (name, w, h, "denoised"))
    ctx.history_blend(8)
    ble = ctx.read_blended()
    meter_both(spt, ctx, 8, spt.IMAGE_BLENDED, ble, 1.0, (name, w, h, "blended"))
    check_display(spt, ctx, 8, spt.IMAGE_BLENDED, ble, 1.0, (name, w, h, "blended"))


def test_ctx_image_errors(spt):
    with spt.Context(0) as c:
        with pytest.raises(spt.SptError, match="SPT_ERR_NOT_CONFIGURED"):
            c.meter_luminance(1)
        prims, mats, env = scene_of(spt, "cornell")
        c.set_scene(prims, mats, env)
        c.configure(20, 12, 4, 2, 0)
        c.render(0, 1)
        out = np.zeros(20 * 12, dtype=np.uint32)
        for image in (spt.IMAGE_DENOISED, spt.IMAGE_BLENDED, 3):  # none exists yet; 3 is no image
            with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
                c.meter_luminance(1, image)
            with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
                c.resolve_display_rgba8(1, spt.Display(), image, out=out)
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            c.meter_luminance(0)
        with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
            c.resolve_display_rgba8(0, spt.Display(), out=out)
        bad = spt.Display()
        bad.reserved[0] = 1
        for d in (spt.Display(3, 1.0), spt.Display(1, -1.0), spt.Display(2, float("nan")), spt.Display(0, float("inf")), bad):
            with pytest.raises(spt.SptError, match="SPT_ERR_INVALID"):
                c.resolve_display_rgba8(1, d, out=out)
        assert c.resolve_display_rgba8(1, spt.Display(spt.TONEMAP_ACES, 0.0), out=out) is out


def test_shards_add_up(spt, ctx):
    """Two contexts that render the two row shards of a 97 x 53 Cornell: their counts sum to the whole image's."""
    prims, mats, env = scene_of(spt, "cornell")
    w, h, frames = 97, 53, 2
    ctx.set_scene(prims, mats, env)
    ctx.configure(w, h, 8, 2, 0)
    ctx.set_camera(None)
    ctx.render(0, frames)
    whole = ctx.meter_luminance(frames)
    total = np.zeros(dr.BINS, dtype=np.uint64)
    for rank in range(2):
        with spt.Context(0) as c:
            c.set_scene(prims, mats, env)
            c.configure(w, h, 8, 2, 0, shard_rank=rank, shard_count=2)
            c.render(0, frames)
            part = c.meter_luminance(frames)
            assert np.array_equal(part, spt.luminance_histogram_host(c.read_accum(), float(frames)))
            total += part
    assert int(total.sum()) == w * h and np.array_equal(total, whole.astype(np.uint64))


def test_black_scene_meters_black(spt, ctx):
    """No sky and no emitter: every pixel lands in bin 0 and the exposure is 1."""
    prims = spt.sphere_prims([(0.0, 0.0, 5.0, 1.0)])
    env = spt.reference_env(False)
    ctx.set_scene(prims, spt.reference_materials(), env)
    ctx.configure(33, 17, 4, 2, 0)
    ctx.set_camera(None)
    ctx.render(0, 2)
    counts = ctx.meter_luminance(2)
    assert counts[0] == 33 * 17 and counts[1:].sum() == 0
    assert spt.exposure_from_histogram(counts) == 1.0


# ---- the device-image resolve ----------------------------------------------------------------------------
def test_resolve_display_device_image(spt, ctx):
    v = np.concatenate([dr.special_values(), dr.key_boundaries()[::7], np.linspace(0.0, 12.0, 777).astype(F)])
    images = {"grey": dr.grey(v), "channels": np.stack([v, v[::-1], np.roll(v, 5), np.roll(v, 11)], axis=1),
              "bits": dr.random_bits(4 * 5141, 9).reshape(-1, 4)}
    for name, img in images.items():
        t = on_device(img)
        for tonemap in (spt.TONEMAP_CLAMP, spt.TONEMAP_REINHARD, spt.TONEMAP_ACES):
            for exposure, divisor in ((1.0, 1.0), (3.5, 7.0)):
                d = spt.Display(tonemap, exposure)
                got = ctx.resolve_display_device_image(t.data_ptr(), t.shape[0], d, divisor)
                assert np.array_equal(got, spt.display_host(img, d, divisor)), (name, tonemap, exposure)


# ---- the backends ---------------------------------------------------------------------------------------
def test_backend_auto_exposure_and_tonemap(spt, ctx, tmp_path):
    """tests/cpp/display_backend.cpp drives render::HIPPathTracer in settings mode: with setAutoExposure(true,
    0.18f), setExposure(1.5f) and set_tonemap(ACES), get_render_result() is display_host of the accumulation at
    1.5 times the exposure of its host histogram; with both off it is the plain resolve; with the denoiser on
    the meter reads the denoised image. The backend builds its scene from the Scene's spheres (it has no other
    geometry), so this is the App's scene at 64 x 64, not Cornell."""
    pkg = os.path.join(ROOT, "software-path-tracer_amd")
    exe, out = tmp_path / "display_backend", tmp_path / "out.bin"
    subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "display_backend.cpp"), "-L", pkg, "-lspt_render", "-lspt_hip",
                    f"-Wl,-rpath,{pkg}"], check=True)
    w, h, spp = 64, 64, 2
    r = subprocess.run([str(exe), str(w), str(h), str(spp), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(out, dtype=np.uint32)
    assert tuple(raw[:2]) == (w, h)
    n, px = int(raw[2]), w * h
    spheres = raw[3:3 + 4 * n].view(F).reshape(n, 4)
    at = 3 + 4 * n
    accum = raw[at:at + 4 * px].view(F).reshape(px, 4)
    img_a, img_b, img_c, img_b_metered = (raw[at + 4 * px + k * px:at + 4 * px + (k + 1) * px] for k in range(4))
    assert n == 38 and img_b_metered.size == px

    # the same frames in a Context: the backend's scene in the order it uploaded it, its settings-mode configuration
    ctx.set_scene(spt.sphere_prims([tuple(s) for s in spheres]), spt.reference_materials(), spt.reference_env(True))
    ctx.configure(w, h, 4, 2, 0, frames_in_flight=1)
    ctx.set_camera(None)
    ctx.render(0, spp)
    acc = ctx.read_accum()
    assert np.array_equal(acc.view(np.uint32), accum.view(np.uint32))

    def shown(img, divisor):  # (1.5: the settings' exposure, the compensation)
        metered = spt.exposure_from_histogram(spt.luminance_histogram_host(img, divisor),
                                              spt.ExposureParams(target_luminance=0.18))
        exposure = float(F(metered) * F(1.5))
        return spt.display_host(img, spt.Display(spt.TONEMAP_ACES, exposure), divisor), exposure

    want_a, exposure_a = shown(acc, float(spp))
    assert np.array_equal(img_a, want_a)
    want_b = ctx.resolve_rgba8(spp, 1.5)  # what the backend gives without the feature
    assert np.array_equal(img_b, want_b) and not np.array_equal(img_a, img_b)
    ctx.denoise(spp)
    den = ctx.read_denoised()
    want_c, exposure_c = shown(den, 1.0)
    assert np.array_equal(img_c, want_c)
    # the accumulation's meter gives another exposure and other bytes: the backend metered the denoised image
    assert exposure_c != exposure_a
    assert not np.array_equal(img_c, spt.display_host(den, spt.Display(spt.TONEMAP_ACES, exposure_a)))
    # auto-exposure switched on after B without a render(): B's frames metered, through CLAMP (the driver checked
    # that switching it off again gave B, not what this resolve left in the result buffer)
    assert np.array_equal(img_b_metered, spt.display_host(acc, spt.Display(spt.TONEMAP_CLAMP, exposure_a), float(spp)))
    assert not np.array_equal(img_b_metered, img_b)

    # the Python mirror of the backend: the same switches, the same three images
    pt = spt.HIPPathTracer(settings_mode=True)
    scene = spt.Scene()
    for x, y, z, rad in spheres:
        node = scene.CreateNode(spt.SphereObject, "sphere")
        node.SetPosition((x, y, z))
        node.SetRadius(rad)
    settings = spt.RenderSettings()
    settings.setResolution(w, h)
    settings.setMaxBounces(4)
    settings.setRussianRouletteDepth(2)
    settings.setSamplesPerPixel(spp)
    settings.setExposure(1.5)
    pt.set_scene(scene)
    pt.set_settings(settings)
    settings.setAutoExposure(True, 0.18)
    pt.set_tonemap(spt.TONEMAP_ACES)
    pt.render()
    assert np.array_equal(pt.get_render_result().image_buffer, want_a)
    settings.setAutoExposure(False)
    pt.set_tonemap(spt.TONEMAP_CLAMP)
    pt.render()
    assert np.array_equal(pt.get_render_result().image_buffer, want_b)
    pt.set_denoise(spt.DenoiseParams())
    settings.setAutoExposure(True, 0.18)
    pt.set_tonemap(spt.TONEMAP_ACES)
    pt.render()
    assert np.array_equal(pt.get_render_result().image_buffer, want_c)
