"""The host functions of the a-trous filter, the reprojection, the luminance meter and the display transform under
AddressSanitizer and UndefinedBehaviorSanitizer (no GPU): tests/cpp/filters_host_check.cpp with csrc/spt_host.cpp in
a program of its own (tests/host_program.py), over oracle renders at 1 x 1, 7 x 5 and 20 x 12 made as
tests/test_denoise_host.py and tests/test_reproject_host.py make theirs. Every word the program writes is the
library's own (which those tests pin to the numpy restatements)."""
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import host_program
import reproject_ref as rr

F = np.float32
FRAMES, EXPOSURE = 2, 1.75
E, T, I, I_AT, VFOV = (1.5, 0.75, -2.0), (0.0, -1.0, 5.0), (0.0, 0.0, 4.0), (0.0, -1.0, 8.0), 55.0  # test_reproject_host.py's


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build("filters_host_check", tmp_path_factory.mktemp("filters"))


def views(spt, ref, w, h):
    """(the previous view's camera, material table, sums, mean, cur_a, cur_b, hist, hist_a, hist_b): the current
    view's sums of FRAMES frames with its features, and the previous view's captured image with its features."""
    if (w, h) == (1, 1):  # the one-sphere pixel of both tests' test_one_pixel: its only ray hits the sphere
        prims, mats, env = spt.sphere_prims([(-3.0, 3.0, 3.0, 1.0)]), spt.reference_materials(), spt.reference_env(True)
        cur_cam, prev_cam = None, None
    else:  # Cornell seen from E, its history from I
        prims, mats, env = spt.build_scene("cornell")
        cur_cam, prev_cam = spt.look_at(E, T, vfov=VFOV), spt.look_at(I, I_AT, vfov=VFOV)
    sums = rr.oracle_sum(spt, ref, prims, mats, env, w, h, cur_cam, 0, FRAMES, 4)
    cur_a, cur_b, _ = dr.oracle_features(spt, ref, prims, mats, env, w, h, cur_cam)
    hist = rr.blend(rr.oracle_sum(spt, ref, prims, mats, env, w, h, prev_cam, 0, FRAMES, 4), FRAMES, length=True)
    hist_a, hist_b, _ = dr.oracle_features(spt, ref, prims, mats, env, w, h, prev_cam)
    reusable = np.ones(len(mats), dtype=np.uint32)
    reusable[::2] = 0  # every other material barred
    posed = prev_cam if prev_cam is not None else spt.look_at((0.25, 0.0, -0.5), (-3.0, 3.0, 3.0), vfov=VFOV)
    return posed, reusable, sums, (sums / F(FRAMES)).astype(F), cur_a, cur_b, hist, hist_a, hist_b


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (20, 12)])
def test_filters_under_sanitizers(spt, ref, program, tmp_path, w, h):
    cam, reusable, sums, mean, cur_a, cur_b, hist, hist_a, hist_b = views(spt, ref, w, h)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        np.array([w, h, FRAMES, reusable.size], dtype=np.uint32).tofile(f)
        np.array([EXPOSURE], dtype=F).tofile(f)
        f.write(bytes(cam))
        reusable.tofile(f)
        for arr in (sums, mean, cur_a, cur_b, hist, hist_a, hist_b):
            assert arr.shape == (h, w, 4)
            np.ascontiguousarray(arr, dtype=F).tofile(f)
    r = subprocess.run([program, str(inp), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(out, dtype=np.uint32)
    n, at = w * h, 0

    def take(count):
        nonlocal at
        at += count
        assert at <= raw.size
        return raw[at - count:at]

    for levels in range(1, 7):
        want = spt.atrous_host(mean, cur_a, cur_b, spt.DenoiseParams(levels=levels))
        assert np.array_equal(take(4 * n), want.view(np.uint32).reshape(-1)), levels
    for table in (None, reusable):
        for prev in (None, cam):
            want = spt.reproject_host(prev, cur_a, cur_b, hist, hist_a, hist_b, None, table)
            assert np.array_equal(take(4 * n), want.view(np.uint32).reshape(-1)), (table is not None, prev is not None)
    counts = spt.luminance_histogram_host(sums, float(FRAMES))
    assert np.array_equal(take(spt.METER_BINS), counts) and int(counts.sum()) == n
    assert take(1)[0] == np.array([spt.exposure_from_histogram(counts)], dtype=F).view(np.uint32)[0]
    for tonemap in (spt.TONEMAP_CLAMP, spt.TONEMAP_REINHARD, spt.TONEMAP_ACES):
        want = spt.display_host(sums, spt.Display(tonemap, EXPOSURE), float(FRAMES))
        assert np.array_equal(take(n), want.reshape(-1)), tonemap
    assert at == raw.size
