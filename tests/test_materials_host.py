"""Material models without a GPU: spt_bsdf_sample (the host build of the scattering step the kernels
compile) against the independent restatement tests/cpp/ref_materials.c, closed cases, the restatement
against the oracle and in a furnace, argument checks, and the launch plan (tests/cpp/test_bsdf_plan.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import material_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def same_bits(a, b):
    return np.asarray(a, dtype=F).view(np.uint32).tolist() == np.asarray(b, dtype=F).view(np.uint32).tolist()


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(F)


# ---- spt_bsdf_sample against the restatement, bit for bit -------------------------------------------
def test_bsdf_sample_matches_the_restatement(spt):
    """120,000 pseudo-random (d, n, model, rng) inputs: every kind, both `entering` values, grazing incidence
    (|d . n| down to 1e-7), total internal reflection (inside glass beyond the critical angle), fuzz 0 and
    > 0, SPT_FLAG_ABS_FLOAT on and off; direction, flags and the RNG state afterwards compared."""
    lib, rlib = spt.load_library(), mr.load()
    rng = np.random.default_rng(0x6d617473)
    n_cases = 120_000
    f3 = ctypes.c_float * 3
    FP = ctypes.POINTER(ctypes.c_float)
    seen = {"tir": 0, "transmit": 0, "reflect_glass": 0, "absorbed": 0, "grazing": 0}
    kinds = [0, 0, 0]
    for i in range(n_cases):
        n = unit(rng.normal(size=3))
        entering = bool(i & 1)
        mode = i % 5
        if mode == 0:  # grazing: d almost in the tangent plane, on the side `entering` names (or just past it)
            t = unit(np.cross(n, rng.normal(size=3)))
            eps = 10.0 ** rng.uniform(-7, -1) * (1 if i % 10 else -1)
            d = unit(t.astype(np.float64) + (-eps if entering else eps) * n.astype(np.float64))
            seen["grazing"] += 1
        else:  # any direction on the side `entering` names
            d = unit(rng.normal(size=3))
            if (float(np.dot(d, n)) < 0) != entering:
                d = -d
        kind = i % 3
        kinds[kind] += 1
        param = [0.0, float(F(rng.uniform(0, 1))) if (i // 3) % 4 else (0.0 if (i // 12) % 2 else 1.0),
                 float(F(rng.choice([1.0, 1.33, 1.5, 2.4, 0.75, rng.uniform(0.3, 3.0)])))][kind]
        flags = spt.FLAG_ABS_FLOAT if (i // 7) % 2 else 0
        state = int(rng.integers(0, 2 ** 32))
        m = spt.material_models([(kind, param)])
        out_a, out_b = np.zeros(3, dtype=F), np.zeros(3, dtype=F)
        sa, sb = ctypes.c_uint32(state), ctypes.c_uint32(state)
        ta, tb, aa, ab = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = lib.spt_bsdf_sample(m.ctypes.data, f3(*d), f3(*n), int(entering), flags, ctypes.byref(sa),
                                 out_a.ctypes.data_as(FP), ctypes.byref(ta), ctypes.byref(aa))
        assert rc == 0
        rlib.mat_bsdf_sample(m.ctypes.data, f3(*d), f3(*n), int(entering), flags, ctypes.byref(sb),
                             out_b.ctypes.data_as(FP), ctypes.byref(tb), ctypes.byref(ab))
        assert same_bits(out_a, out_b) and (ta.value, aa.value, sa.value) == (tb.value, ab.value, sb.value), \
            (i, kind, param, d, n, entering, flags, state, out_a, out_b, ta.value, tb.value, aa.value, ab.value)
        if kind == 2:
            sin2 = 1.0 - float(np.dot(d, n)) ** 2
            eta = 1.0 / param if entering else param
            if eta * eta * sin2 > 1.0 + 1e-5:  # (clear of the fp32 rounding of k)
                seen["tir"] += 1
                assert not ta.value
            seen["transmit" if ta.value else "reflect_glass"] += 1
        seen["absorbed"] += aa.value
    assert min(kinds) >= n_cases // 3
    assert seen["tir"] > 1000 and seen["transmit"] > 10000 and seen["reflect_glass"] > 1000, seen
    assert seen["absorbed"] > 100 and seen["grazing"] == n_cases // 5, seen


# ---- closed cases -----------------------------------------------------------------------------------
def test_glass_at_normal_incidence_goes_straight_through(spt, ref):
    d, n = (0.0, -1.0, 0.0), (0.0, 1.0, 0.0)
    through = 0
    for state in range(1, 400):
        u = float(ref.random_floats(state, 1)[0][0])
        out, transmitted, absorbed, after = spt.bsdf_sample(spt.MAT_DIELECTRIC, 1.5, d, n, True, state)
        assert after == int(ref.random_floats(state, 1)[1][0])  # exactly one draw
        assert not absorbed
        r0 = F(F(F(1.0) - F(1.5)) / F(F(1.0) + F(1.5))) ** 2  # R at ci = 1 is r0 + (1 - r0) * 0
        if F(r0) > F(u):
            assert not transmitted and same_bits(out, (0.0, 1.0, 0.0))
        else:
            assert transmitted and same_bits(out, (0.0, -1.0, 0.0))
            through += 1
    assert through > 300


def test_mirror_at_normal_incidence(spt):
    out, transmitted, absorbed, after = spt.bsdf_sample(spt.MAT_METAL, 0.0, (0.0, -1.0, 0.0), (0.0, 1.0, 0.0), True, 77)
    assert same_bits(out, (0.0, 1.0, 0.0)) and not transmitted and not absorbed
    assert after == 77  # fuzz 0 draws nothing


def test_total_internal_reflection_for_any_u(spt, ref):
    """Inside glass of 1.5 at 60 degrees from the normal (the critical angle is 41.8): always reflected."""
    n = (0.0, 1.0, 0.0)  # the outward normal: the ray travels with it
    d = unit((np.sin(np.pi / 3), np.cos(np.pi / 3), 0.0))
    for state in range(1, 300):
        out, transmitted, absorbed, after = spt.bsdf_sample(spt.MAT_DIELECTRIC, 1.5, d, n, False, state)
        assert not transmitted and not absorbed
        assert after == int(ref.random_floats(state, 1)[1][0])
        assert out[1] < 0 and abs(float(out[0]) - float(d[0])) < 1e-6 and abs(float(out[1]) + float(d[1])) < 1e-6


def test_fuzzy_metal_reports_absorption(spt):
    """METAL(1) at grazing incidence: `absorbed` exactly where dot(r, nf) <= 0 for the direction returned."""
    n = np.array((0.0, 1.0, 0.0), dtype=F)
    got = {True: 0, False: 0}
    for state in range(1, 600):
        # the last two arrive from below the surface: absorbed when the fuzz direction's cosine (squared: uniform)
        # is below d . n, about 8 % and 45 % of their 120 states each
        eps = (1e-3, 1e-5, 0.0, -0.3, -0.9)[state % 5]
        d = unit((1.0, -eps, 0.0))
        out, transmitted, absorbed, after = spt.bsdf_sample(spt.MAT_METAL, 1.0, d, n, True, state)
        dot = F(F(out[0] * n[0]) + F(out[1] * n[1])) + F(out[2] * n[2])
        assert absorbed == (not dot > 0), (state, d, out)
        assert not transmitted and after != state  # fuzz > 0: two draws
        got[absorbed] += 1
    assert got[True] > 20 and got[False] > 300, got


# ---- the restatement itself ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cornell", "app"])
@pytest.mark.parametrize("nee", [False, True])
def test_restatement_without_models_is_the_oracle(spt, ref, scene, nee):
    w, h, frames = 37, 23, 4
    flags = spt.FLAG_NEE if nee else 0
    prims, mats, env = spt.build_scene(scene)
    ms = mr.MatScene(spt, ref, prims, mats, env)
    want = ms.rs.render(w, h, 0, frames, mr.BOUNCES, mr.RR, flags)
    mr.assert_same(mr.accumulate(ms.frames(w, h, 0, frames, flags), 0, frames), want, f"{scene} nee={nee}")
    diffuse = mr.MatScene(spt, ref, prims, mats, env, [(spt.MAT_DIFFUSE, 0.0)] * len(mats))
    mr.assert_same(mr.accumulate(diffuse.frames(w, h, 0, frames, flags), 0, frames), want, f"{scene} all-DIFFUSE")


def test_furnace(spt, ref):
    """A white sky all around, no emitters, albedo 1: a glass sphere and a fuzzy metal sphere neither create
    nor lose energy — every path returns the sky's 1 or was stopped (0) by the bounce limit or a fuzz
    absorption. Cap on the zeros: METAL's fuzz direction lies in nf's hemisphere, so r . nf <= 0 needs both
    cosines to round to zero: none expected. A path stopped by the limit of 32 stayed inside the glass for
    ~30 reflections at one internal angle (a sphere repeats it), which takes a Schlick reflectance R >= 0.5,
    else R^30 < 1e-9: (1 - cos)^5 >= 0.48, cos <= 0.14, the outer 2 % of the sphere's disc, at most 0.5 %
    of the image here; a path there enters with 1 - R and survives with R^30, at most 1.2 % (R = 30/31).
    0.5 % x 1.2 % = 6e-5 of the paths: the cap is 1e-3 (16 of the 16,384 paths)."""
    w = h = 64
    frames = 4
    prims = spt.sphere_prims([(-0.9, 0.0, 4.0, 0.8), (0.9, 0.0, 4.0, 0.8)])
    mats = np.zeros(2, dtype=spt.MATERIAL_DTYPE)
    mats["albedo"] = 1.0
    prims[1]["material"] = 1
    env = spt.reference_env(True)
    env.horizon[:] = [1.0, 1.0, 1.0]
    env.zenith[:] = [1.0, 1.0, 1.0]
    ms = mr.MatScene(spt, ref, prims, mats, env, [(spt.MAT_DIELECTRIC, 1.5), (spt.MAT_METAL, 0.3)])
    img = ms.frames(w, h, 0, frames, 0, bounces=32, rr=2)
    rgb = img[..., :3]
    zero = np.all(rgb == 0.0, axis=-1)
    one = np.all(np.abs(rgb.astype(np.float64) - 1.0) <= 2.0 ** -22, axis=-1)
    assert np.all(zero | one), np.argwhere(~(zero | one))[:5]
    assert zero.mean() <= 1e-3, zero.mean()
    # the spheres are in view: a disc of radius 0.8 at z = 4 covers pi * 0.2^2 of the image plane's 2 x 2, 3.1 %,
    # a little more off axis; with one bounce allowed their pixels are the black ones
    plain = mr.MatScene(spt, ref, prims, mats, env).frames(w, h, 0, 1, 0, bounces=1, rr=2)
    assert 0.05 < np.all(plain[0, ..., :3] == 0.0, axis=-1).mean() < 0.08


# ---- argument checks that need no device -------------------------------------------------------------------
def test_argument_checks(spt, tmp_path):
    lib = spt.load_library()
    m = spt.material_models([(spt.MAT_METAL, 0.5)])
    assert lib.spt_set_material_models(None, m.ctypes.data, 1) == -1  # SPT_ERR_INVALID
    assert lib.spt_set_material_models(None, None, 0) == -1
    assert spt.MATERIAL_MODEL_DTYPE.itemsize == 16
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spt.h"\nint main(void){'
                   'printf("%zu %zu %zu %d %d %d\\n", sizeof(spt_material_model), offsetof(spt_material_model, param),'
                   ' offsetof(spt_material_model, reserved), SPT_MAT_DIFFUSE, SPT_MAT_METAL, SPT_MAT_DIELECTRIC);'
                   ' return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = spt.MATERIAL_MODEL_DTYPE
    assert got == [dt.itemsize, dt.fields["param"][1], dt.fields["reserved"][1], spt.MAT_DIFFUSE, spt.MAT_METAL,
                   spt.MAT_DIELECTRIC]
    assert spt.load_library().spt_abi_version() == 3
    # spt_bsdf_sample refuses what spt_set_material_models refuses
    f3 = ctypes.c_float * 3
    FP = ctypes.POINTER(ctypes.c_float)
    out = np.zeros(3, dtype=F)
    st, tr, ab = ctypes.c_uint32(1), ctypes.c_int(), ctypes.c_int()

    def call(model):
        return lib.spt_bsdf_sample(model.ctypes.data, f3(0, -1, 0), f3(0, 1, 0), 1, 0, ctypes.byref(st),
                                   out.ctypes.data_as(FP), ctypes.byref(tr), ctypes.byref(ab))

    assert call(m) == 0
    assert call(spt.material_models([(spt.MAT_METAL, -0.0)])) == 0 and same_bits(out, (0.0, 1.0, 0.0))  # a mirror
    for kind, param in ((spt.MAT_METAL, 1.5), (spt.MAT_METAL, -0.1), (spt.MAT_DIELECTRIC, 0.0),
                        (spt.MAT_DIELECTRIC, float("inf")), (spt.MAT_DIFFUSE, 0.5), (3, 0.0), (spt.MAT_METAL, float("nan"))):
        assert call(spt.material_models([(kind, param)])) == -1, (kind, param)
    bad = spt.material_models([(spt.MAT_METAL, 0.5)])
    bad[0]["reserved"][1] = 1
    assert call(bad) == -1
    assert lib.spt_bsdf_sample(None, f3(), f3(), 1, 0, ctypes.byref(st), out.ctypes.data_as(FP), ctypes.byref(tr),
                               ctypes.byref(ab)) == -1


def test_launch_plan_of_material_models(spt, tmp_path):
    csrc = os.path.join(os.path.dirname(spt.LIB_PATH), "csrc")
    src = os.path.join(ROOT, "tests", "cpp", "test_bsdf_plan.cpp")  # (built here, as test_camera_plan.cpp is)
    exe = tmp_path / "test_bsdf_plan"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", f"-I{csrc}", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
