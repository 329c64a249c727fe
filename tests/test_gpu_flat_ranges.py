"""The guard-free forms of the shape-specialized flat k_paths (spt_kernels.h kShapeRanges), bit for bit.

A flat scene that passes scene.cpp flat_ranges_ok carries a bit in its shape key, and the k_paths compiled for
it runs Russian roulette's divisions, the shading normal's inverse root and the path start's emission without
their per-lane range tests (spt_get_flat_ranges, Context.stats().flat_ranges). Every case waits for the
specialized kernels, asserts that they ran and what the bit was, and compares the accumulation as uint32 with
the generic kernels (spt_tuning.specialize = -1) and with the oracle.

96x64, 8 bounces, RR depth 2, 16 frames in two calls of 8, once with wide_chunks = 1 (the first call runs the
automatic plan's channel-lane kernel and builds the view's lists, the second the wide pixel-lane kernel over them)
and once with wide_chunks = -1 and 32-pixel chunks (the narrow pixel-lane kernel, the benchmark's before the wide
one): the three specialized forms that read the bit. tests/cpp/test_device_ranges (run below) checks the forms
themselves over their whole ranges.
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, BOUNCES, RR = 96, 64, 8, 2
CALLS = (8, 8)
WHITE, RED, GREEN, LIGHT = 0, 1, 2, 3  # scenes.cpp cornell_walls' materials
LEFT_WALL = 3  # ... and its quads: floor, ceiling, back, left, right, light; then the two spheres
FORMS = {"wide": {"wide_chunks": 1}, "narrow": {"wide_chunks": -1, "px_shift": 5}}

_oracle = {}
_generic = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def assert_same(got, want, what):
    g, r = bits(got), bits(want)
    bad = np.flatnonzero(np.any(g != r, axis=1))
    print(f"{what}: {bad.size} of {g.shape[0]} pixels differ")
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} pixels differ, first {bad[:5]}"


def scene(spt, name):
    """(prims, mats, env) of a case's scene: the Cornell box with one thing changed. The changed albedo is the
    white material's green component (the floor, ceiling, back wall and both spheres), so red and blue stay
    nonzero in every material."""
    prims, mats, env = spt.build_scene("cornell")
    prims, mats = prims.copy(), mats.copy()
    albedo = {"albedo_zero": 0.0, "albedo_2^-5": 2.0 ** -5, "albedo_2^-6": 2.0 ** -6, "albedo_1.5": 1.5}
    if name in albedo:
        mats[WHITE]["albedo"][1] = albedo[name]
    elif name == "emission_zero_flagged":
        # The emission flag (DevMaterial emission.w) is derived from the components, so a flagged light of
        # exactly zero emission cannot be set; the nearest: two components +0 and the third 2^-60, small enough
        # to add nothing visible and large enough that no product with a throughput (>= 2^-40) is denormal.
        # The +0 components go through the flagged light's products and the path start's select-free read.
        mats[LIGHT]["emission"][:] = (0.0, 0.0, 2.0 ** -60)
    elif name == "tiny_sphere":
        prims = np.concatenate([prims, spt.sphere_prims([(0.0, 0.0, 5.0, 2.0 ** -46)], material=WHITE)])
    elif name in ("spare_material", "spare_material_used"):
        # a fifth material outside the albedo range; unused, it does not count (the predicate sees the
        # materials the primitives use), and spt_update_prims puts the left wall on it and back
        bad = np.zeros(1, dtype=spt.MATERIAL_DTYPE)
        bad[0]["albedo"][:] = (0.65, 1.5, 0.05)
        mats = np.concatenate([mats, bad])
        if name == "spare_material_used":
            prims[LEFT_WALL]["material"] = len(mats) - 1
    else:
        assert name == "cornell", name
    return prims, mats, env


def oracle(spt, ref, name):
    if name not in _oracle:
        prims, mats, env = scene(spt, name)
        acc = ref.RefScene(prims, mats, env).render(W, H, 0, sum(CALLS), BOUNCES, RR, 0)
        acc.setflags(write=False)
        _oracle[name] = acc
    return _oracle[name]


def render_calls(ctx):
    """CALLS continuing one accumulation from frame 0; (accumulation, stats after the last call)."""
    f = 0
    for n in CALLS:
        ctx.render(f, n)
        f += n
    return ctx.read_accum(), ctx.stats()


def render(spt, name, form, specialize=1):
    prims, mats, env = scene(spt, name)
    with spt.Context(0) as ctx:
        ctx.set_tuning(specialize=specialize, **FORMS[form])
        ctx.set_scene(prims, mats, env)
        ctx.configure(W, H, BOUNCES, RR, 0)
        ctx.specialize_scene()
        return render_calls(ctx)


def generic(spt, name, form):
    if (name, form) not in _generic:
        acc, st = render(spt, name, form, specialize=-1)
        assert st.specialized == 0 and st.flat_ranges == 0
        acc.setflags(write=False)
        _generic[name, form] = acc
    return _generic[name, form]


def check_stats(spt, st, form, want):
    assert st.schedule == spt.SCHEDULE_PERSISTENT
    assert st.specialized == 1, "the shape-specialized kernel did not run"
    assert st.view_wide == (1 if form == "wide" else 0)
    assert st.flat_ranges == want, (st.flat_ranges, want)


CASES = [("cornell", 1), ("albedo_zero", 1), ("albedo_2^-5", 1), ("albedo_2^-6", 0), ("albedo_1.5", 0),
         ("emission_zero_flagged", 1), ("tiny_sphere", 0)]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name,want", CASES, ids=[c[0] for c in CASES])
def test_scene(spt, ref, name, want, form):
    acc, st = render(spt, name, form)
    check_stats(spt, st, form, want)
    assert_same(acc, generic(spt, name, form), f"{name}, {form}: specialized against generic")
    assert_same(acc, oracle(spt, ref, name), f"{name}, {form}: specialized against the oracle")


@pytest.mark.parametrize("form", list(FORMS))
def test_material_changed_through_the_update_path(spt, ref, form):
    """The left wall is put on a material with an albedo of 1.5 and back (spt_update_prims prepares a flat scene
    again, with the materials its primitives then use): the bit goes 1, 0, 1, and each state renders its oracle."""
    prims, mats, env = scene(spt, "spare_material")
    used = scene(spt, "spare_material_used")[0]
    with spt.Context(0) as ctx:
        ctx.set_tuning(specialize=1, **FORMS[form])
        ctx.set_scene(prims, mats, env)
        ctx.configure(W, H, BOUNCES, RR, 0)
        for state, want, wall in (("spare_material", 1, None), ("spare_material_used", 0, used), ("spare_material", 1, prims)):
            if wall is not None:
                ctx.update_prims([LEFT_WALL], wall[[LEFT_WALL]])
            ctx.specialize_scene()
            acc, st = render_calls(ctx)
            check_stats(spt, st, form, want)
            assert_same(acc, oracle(spt, ref, state), f"{state}, {form}: specialized against the oracle")
            assert_same(acc, generic(spt, state, form), f"{state}, {form}: specialized against generic")


def test_more_bounces_than_the_proof_covers(spt, ref):
    """10 bounces: a throughput may pass below 2^-40 before its last roulette, so the kernel compiled for this
    configuration keeps the guarded forms whatever the scene's bit says (spt_kernels.h kRangesMaxBounces)."""
    prims, mats, env = scene(spt, "cornell")
    with spt.Context(0) as ctx:
        ctx.set_tuning(specialize=1, **FORMS["narrow"])
        ctx.set_scene(prims, mats, env)
        ctx.configure(W, H, 10, RR, 0)
        ctx.specialize_scene()
        acc, st = render_calls(ctx)
    assert st.specialized == 1 and st.flat_ranges == 0
    want = ref.RefScene(prims, mats, env).render(W, H, 0, sum(CALLS), 10, RR, 0)
    assert_same(acc, want, "10 bounces: specialized against the oracle")


def test_two_frames_run_k_frame_without_the_forms(spt, ref):
    """k_frame has no guard-free forms: it runs specialized for the key with the bit and reports 0."""
    prims, mats, env = scene(spt, "cornell")
    with spt.Context(0) as ctx:
        ctx.set_tuning(specialize=1)
        ctx.set_scene(prims, mats, env)
        ctx.configure(W, H, BOUNCES, RR, 0)
        ctx.specialize_scene()
        ctx.render(0, 2)
        acc, st = ctx.read_accum(), ctx.stats()
    assert st.schedule == spt.SCHEDULE_FRAME and st.specialized == 1 and st.flat_ranges == 0
    want = ref.RefScene(prims, mats, env).render(W, H, 0, 2, BOUNCES, RR, 0)
    assert_same(acc, want, "k_frame: specialized against the oracle")


def test_guard_free_forms_over_their_ranges(spt):
    """tests/cpp/test_device_ranges on the GPU: inv_sqrt_ranged on every float of [2^-96, 2^96), rr_divide_ranged on
    every divisor of [2^-40, 1], the emission identity on every value >= +0, bounce_tangent_ranged on 2^26 normals,
    each against '/', sqrtf and the guarded form."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_device_ranges")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/test_device_ranges"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "mismatches: inv_sqrt 0, rr_divide 0, emission 0, tangent 0" in r.stdout
    # a sphere of the smallest admitted radius, hit centrally from anywhere in the scene: the shading normal's bound
    assert "hits, 0 with |Ng|^2 below r^2 / 17 or outside the window" in r.stdout
