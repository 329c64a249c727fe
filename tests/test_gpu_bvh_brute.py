"""Every form of the GPU's BVH traversal against a brute-force closest hit, bit for bit.

The expected values come from the oracle in brute-force mode (RefScene(brute=True): every primitive in index
order, the smallest t, the lowest index on a tie), so neither BVH — the product's quantized 4-wide tree nor
the oracle's own — is trusted: a box culled that an exact test would hit, on either side or on both, shows.
No tolerance anywhere: the primitive records, t, the normals and the images are the same fp32 formulas on
both sides.

Two checks per (scene, camera):
  first hits   spt_render_features against denoise_ref.oracle_features over the brute scene: position and
               material, normal and t, albedo and primitive index (closest_tree with the private stack);
  whole paths  spt_render, 4 frames, max_bounces 4, rr_depth 2, against brute_ref.frame_radiance (seed,
               spt_camera_ray, ref_trace_ray, float32 adds in frame order), on every schedule the BVH kernels
               have: one-frame calls (k_frame), one call of 4 frames (k_paths: LDS top nodes, global 4-byte
               stack entries), the counting instantiations (set_profiling), FLAG_WAVEFRONT | FLAG_SPLIT_KERNELS,
               FLAG_SORTED_RAYS, and — in scenes with emitters — FLAG_NEE (any-hit shadow traversal) on k_frame,
               k_paths, the counting kernels and the split schedule. stalled_waves == 0 throughout.

Scenes (numpy, fixed seeds; each the smallest that can still go wrong):
  hf       24 x 24 cells of two right triangles with axis-aligned edges, all coordinates multiples of 1/32
           (the quantized boxes then add no slack of their own: the padding alone covers the slab test's
           rounding); every third row of cells exactly flat (zero-thickness boxes); every fifth triangle emits
  ties     a 300-primitive mixed scene twice over, the copy with another material, plus stacks of coplanar
           overlapping axis-aligned quads, shuffled: the lower index wins every exact tie, whichever leaf the
           traversal reaches first
  tmin     coplanar overlapping quads exactly kTNear = 0.001 in front of the reference camera: the centre
           ray's hit has t == tmin, the value every entry distance is clamped to, so every stack entry of the
           other quads has t0 == best_t (a pop must keep t0 <= best_t, not t0 < best_t); tmin_r is the same
           scene in reverse index order, so in one of the two the leaf the traversal reaches first does not
           hold the lowest index
  mixed    200 spheres, 200 quads, 400 triangles; nested spheres (a camera inside the outer one), tangent spheres
  scale    clusters of primitives of extent 2^-10 beside primitives of extent 2^6: the padding exceeds whole
           clusters, every box overlaps its siblings
  offset   hf translated by (1000, -2000, 500): the magnitude far above the extent
  sizes    trees of at most 5, 6..53, 54..64 and just above 64 device nodes (see SIZES below)
  refit    hf after spt_update_prims moved a tenth of its triangles, one beyond the old coordinate magnitude

Cameras: the reference camera; one posed close in front; one inside the geometry; one whose rays run along
cell edges (hf: from above, every second pixel's ray through a grid line or vertex of the flat cells and the
centre row and column in the planes of a row of edges); and far ones, R = |origin| / (scene magnitude) = 8,
32, 128, 1000 with a field of view that makes the scene fill the image (hf and mixed). DESIGN.md §3.3 counts the
roundings: a padding of 1e-5 x the scene's magnitude alone covers quads and triangles to R of about 10 and
a sphere's test at no R at all (small spheres fail inside the scene: scale's shadow rays), which is why the
padding follows the camera and spheres' boxes carry a term of their own; with that the argument has no R in
it, and R = 1000 is the largest tested.

Which traversal form a tree size reaches (spt_launch_plan.h paths_variant, spt_kernels.h frame_small_scene,
spt_kernels.hip kBvhTopNodes / kBvhTopNodes8 / kFrameTopNodes): k_paths without statistics or NEE on a scene
of at most 256 K primitives is the 8-wave kernel, whose LDS holds the first min(5, D) device nodes; with
counters or NEE the 7-wave kernel, min(53, D); k_frame holds min(64, D), and a scene of at most 64 nodes, 64
primitives and 16 stack entries without emitters whole, decoded (kSmall). D is the number of 4-wide device
nodes: spt_stats.bvh_nodes counts the binary tree (two per leaf, so never below 6 for a BVH scene), and D =
(scene_bytes - 64 n_prims - 32 n_materials - 80 n_emitters) / 64 by spt_stats.scene_bytes' definition.
The sizes sit on both sides of each boundary:
  size_5   33 triangles, 3 per leaf, D = 5: every node in LDS in every kernel; k_frame kSmall
  size_6   34 triangles, 3 per leaf, D = 6: k_paths' 8-wave kernel reads node 5 from global memory, the 7-wave
           kernel and k_frame (kSmall) none
  size_53  108 triangles, D = 53: the 7-wave kernel's LDS copy is exactly the tree (k_frame: not kSmall from
           here on, more than 64 primitives; its 4-float4 LDS copy holds the whole tree)
  size_54  109 triangles, D = 54: the 7-wave kernel reads node 53 from global memory, k_frame none
  size_64  119 triangles, D = 64: k_frame's LDS copy is exactly the tree
  size_65  121 triangles, D = 65: every kernel reads its last nodes from global memory
"""
import math

import numpy as np
import pytest

import brute_ref as br
import denoise_ref as dr

pytestmark = pytest.mark.gpu

F = np.float32
FRAMES, BOUNCES, RR = 4, 4, 2
W, H = 64, 48
OFFSET = (1000.0, -2000.0, 500.0)
FAR_R = (8, 32, 128, 1000)

_scenes = {}
_want = {}
_mag = {}


# ---- materials and primitive records ------------------------------------------------------------------
def materials(spt):
    m = np.zeros(6, dtype=spt.MATERIAL_DTYPE)
    m["albedo"] = [(0.7, 0.7, 0.7), (0.6, 0.6, 0.6), (0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.3, 0.3, 0.8), (0.9, 0.8, 0.2)]
    m["emission"][1] = (5.0, 4.0, 3.0)
    return m


def tri(spt, p, k, a, b, c, mat):
    p[k]["type"], p[k]["material"] = spt.PRIM_TRIANGLE, mat
    p[k]["p0"][:3], p[k]["p1"][:3], p[k]["p2"][:3] = a, b, c


def quad(spt, p, k, q, u, v, mat):
    p[k]["type"], p[k]["material"] = spt.PRIM_QUAD, mat
    p[k]["p0"][:3], p[k]["p1"][:3], p[k]["p2"][:3] = q, u, v


def sphere(spt, p, k, c, r, mat):
    p[k]["type"], p[k]["material"] = spt.PRIM_SPHERE, mat
    p[k]["p0"] = (c[0], c[1], c[2], r)


def random_prims(spt, rng, n_s, n_q, n_t, lo, hi, mats=(0, 2, 3, 4, 5), emit_every=7):
    """n_s spheres, n_q quads, n_t triangles with centres uniform in the box [lo, hi]."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    p = np.zeros(n_s + n_q + n_t, dtype=spt.PRIM_DTYPE)
    for k in range(len(p)):
        c = lo + (hi - lo) * rng.random(3)
        mat = 1 if emit_every and k % emit_every == 0 else mats[k % len(mats)]
        if k < n_s:
            sphere(spt, p, k, c, 0.1 + 0.25 * rng.random(), mat)
        elif k < n_s + n_q:
            quad(spt, p, k, c, rng.normal(size=3) * 0.35, rng.normal(size=3) * 0.35, mat)
        else:
            tri(spt, p, k, c, c + rng.normal(size=3) * 0.4, c + rng.normal(size=3) * 0.4, mat)
    return p


# ---- scenes ----------------------------------------------------------------------------------------------
def height_field(spt, offset=(0.0, 0.0, 0.0)):
    """1152 triangles over x in [-3, 3], z in [3, 9], heights in [-2, -1]; rows j % 3 == 0 flat at y = -1."""
    n, cell = 24, 0.25
    rng = np.random.default_rng(7)
    hgt = -1.0 - rng.integers(0, 33, size=(n + 1, n + 1)) / 32.0
    for j in range(0, n, 3):
        hgt[j, :] = hgt[j + 1, :] = -1.0
    off = np.asarray(offset, dtype=np.float64)
    p = np.zeros(2 * n * n, dtype=spt.PRIM_DTYPE)
    k = 0
    for j in range(n):
        for i in range(n):
            x0, x1, z0, z1 = -3.0 + cell * i, -3.0 + cell * (i + 1), 3.0 + cell * j, 3.0 + cell * (j + 1)
            v00, v10 = off + (x0, hgt[j, i], z0), off + (x1, hgt[j, i + 1], z0)
            v01, v11 = off + (x0, hgt[j + 1, i], z1), off + (x1, hgt[j + 1, i + 1], z1)
            for a, b, c in ((v00, v10, v01), (v11, v01, v10)):
                tri(spt, p, k, a, b, c, 1 if k % 5 == 0 else (0, 2, 3, 4)[k % 4])
                k += 1
    flat = sum(1 for q in p if q["p0"][1] == q["p1"][1] == q["p2"][1])
    assert flat >= 2 * n * n // 3
    return p


def ties_scene(spt):
    """Every primitive of a 300-primitive mixed scene twice (the copy with the next material), and 6 stacks of
    8 coplanar overlapping axis-aligned quads (two per axis; stack 2 lies in the plane z = 4 around (-0.5, 0)),
    in a fixed shuffle."""
    rng = np.random.default_rng(11)
    base = random_prims(spt, rng, 100, 100, 100, (-3.0, -2.0, 4.0), (3.0, 2.0, 8.0))
    copy = base.copy()
    copy["material"] = (copy["material"] + 1) % 6
    stacks = np.zeros(48, dtype=spt.PRIM_DTYPE)
    k = 0
    for s in range(6):
        ax = s % 3
        u, v = [(1, 2), (0, 2), (0, 1)][ax]
        centre = np.array((-2.0 + 0.75 * s, -1.0 + 0.5 * (s % 3), 3.5 + 0.25 * s))
        for _ in range(8):
            # edges of 0.5, 1 or 2: the stored normal's length is a power of two, so its normalization is exact
            # (a z normal of 0.99999994 would send the reference's abs(int) pole test to a NaN tangent)
            q, eu, ev = centre.copy(), np.zeros(3), np.zeros(3)
            eu[u], ev[v] = rng.choice((0.5, 1.0, 2.0), size=2)
            q[u] -= eu[u] * (0.25 + 0.5 * rng.random())
            q[v] -= ev[v] * (0.25 + 0.5 * rng.random())
            quad(spt, stacks, k, q, eu, ev, k % 6)
            k += 1
    p = np.concatenate([base, copy, stacks])
    perm = rng.permutation(len(p))
    where = np.empty(len(p), dtype=np.int64)
    where[perm] = np.arange(len(p))
    assert np.median(np.abs(where[:300] - where[300:600])) > 100  # (the copies lie far apart)
    return p[perm]


def tmin_ties_scene(spt):
    """12 coplanar overlapping quads in the plane z = 0.001f (kTNear from the reference camera's origin, so the
    centre ray hits them at t == tmin exactly), and 40 primitives behind them: 52 primitives, 5 materials."""
    rng = np.random.default_rng(19)
    back = random_prims(spt, rng, 14, 13, 13, (-3.0, -2.0, 4.0), (3.0, 2.0, 8.0), mats=(0, 2, 3, 4), emit_every=0)
    front = np.zeros(12, dtype=spt.PRIM_DTYPE)
    z = float(F(0.001))
    for k in range(12):  # (edges of 0.5, 1 or 2 around the axis: as ties_scene's stacks)
        eu, ev = rng.choice((0.5, 1.0, 2.0), size=2)
        quad(spt, front, k, (-eu * (0.25 + 0.5 * rng.random()), -ev * (0.25 + 0.5 * rng.random()), z),
             (eu, 0.0, 0.0), (0.0, ev, 0.0), (0, 2, 3, 4)[k % 4])
    p = np.concatenate([back, front])
    return p[rng.permutation(len(p))]


def mixed_scene(spt):
    """200 spheres, 200 quads, 400 triangles: 191 + 200 + 400 random ones, three nested spheres around
    (2.5, 0, 6) and three pairs of tangent spheres (dyadic centres and radii: the contact is exact)."""
    rng = np.random.default_rng(13)
    p = random_prims(spt, rng, 191, 200, 400, (-4.0, -3.0, 3.0), (4.0, 3.0, 11.0))
    extra = np.zeros(9, dtype=spt.PRIM_DTYPE)
    for k, r in enumerate((1.25, 0.625, 0.25)):
        sphere(spt, extra, k, (2.5, 0.0, 6.0), r, (2, 1, 4)[k])
    for k in range(3):
        c = (-2.0 + k, 1.5, 4.0 + k)
        sphere(spt, extra, 3 + 2 * k, c, 0.25, 3)
        sphere(spt, extra, 4 + 2 * k, (c[0] + 0.75, c[1], c[2]), 0.5, 5)
    p = np.concatenate([p[:191], extra, p[191:]])
    assert [int((p["type"] == t).sum()) for t in (0, 1, 2)] == [200, 200, 400]
    return p


def scale_scene(spt):
    """12 clusters of 40 primitives of extent 2^-10 within 2^-7 of their centres, beside 24 primitives of
    extent 2^6: the padding (1e-5 x a magnitude above 100) exceeds a cluster's primitives."""
    rng = np.random.default_rng(17)
    big = np.zeros(24, dtype=spt.PRIM_DTYPE)
    quad(spt, big, 0, (-32.0, -4.0, -16.0), (64.0, 0.0, 0.0), (0.0, 0.0, 64.0), 0)  # a floor
    for k in range(1, 24):
        c = np.array((rng.uniform(-40, 40), rng.uniform(-2, 40), rng.uniform(40, 100)))
        if k % 3 == 0:
            sphere(spt, big, k, c, 32.0, (2, 3, 4, 1)[k % 4])
        elif k % 3 == 1:
            quad(spt, big, k, c, rng.normal(size=3) * 32.0, rng.normal(size=3) * 32.0, (2, 3, 4, 1)[k % 4])
        else:
            tri(spt, big, k, c, c + rng.normal(size=3) * 32.0, c + rng.normal(size=3) * 32.0, (2, 3, 4, 1)[k % 4])
    parts = [big]
    for c in cluster_centres():
        s = 2.0 ** -10
        q = np.zeros(40, dtype=spt.PRIM_DTYPE)
        for k in range(40):
            a = c + rng.uniform(-1, 1, size=3) * 2.0 ** -7
            mat = 1 if k % 9 == 0 else (0, 2, 3, 4, 5)[k % 5]
            if k % 3 == 0:
                sphere(spt, q, k, a, s / 2, mat)
            elif k % 3 == 1:
                quad(spt, q, k, a, rng.normal(size=3) * s / 2, rng.normal(size=3) * s / 2, mat)
            else:
                tri(spt, q, k, a, a + rng.normal(size=3) * s / 2, a + rng.normal(size=3) * s / 2, mat)
        parts.append(q)
    p = np.concatenate(parts)
    return p[rng.permutation(len(p))]


def cluster_centres():
    rng = np.random.default_rng(23)
    c = [np.array((0.0, 0.0, 4.0)), np.array((0.01, 0.005, 4.02))]  # two beside each other, on the reference camera's axis
    while len(c) < 12:
        c.append(np.array((rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 6))))
    return c


def sized_scene(spt, n, seed):
    """n random triangles without an emitter (so a small one is k_frame's kSmall scene)."""
    return random_prims(spt, np.random.default_rng(seed), 0, 0, n, (-2.0, -1.5, 3.0), (2.0, 1.5, 7.0), emit_every=0)


# name -> (primitives, seed, spt_tuning.bvh_max_leaf, the device nodes D the tree has)
SIZES = {"size_5": (33, 1, 3, 5), "size_6": (34, 1, 3, 6), "size_53": (108, 1, 0, 53), "size_54": (109, 1, 0, 54),
         "size_64": (119, 1, 0, 64), "size_65": (121, 1, 0, 65)}


def moved_height_field(spt):
    """(indices, records): every tenth triangle of hf translated by a multiple of 1/32 per axis; the first
    of them to x around 20, beyond hf's coordinate magnitude of 9."""
    rng = np.random.default_rng(29)
    base = height_field(spt)
    idx = np.arange(3, len(base), 10, dtype=np.uint32)
    rec = base[idx].copy()
    for k in range(len(idx)):
        d = np.array((23.0, 0.5, 0.0)) if k == 0 else rng.integers(-16, 17, size=3) / 32.0
        for f in ("p0", "p1", "p2"):
            rec[k][f][:3] = rec[k][f][:3] + d.astype(F)
    return idx, rec


def build(spt, name):
    if name == "hf":
        return height_field(spt)
    if name == "offset":
        return height_field(spt, OFFSET)
    if name == "refit":
        p = height_field(spt)
        idx, rec = moved_height_field(spt)
        p[idx] = rec
        return p
    if name in SIZES:
        return sized_scene(spt, *SIZES[name][:2])
    if name == "tmin_r":
        return tmin_ties_scene(spt)[::-1].copy()
    return {"ties": ties_scene, "tmin": tmin_ties_scene, "mixed": mixed_scene, "scale": scale_scene}[name](spt)


def scene_of(spt, ref, name):
    """(prims, mats, env, RefScene in brute-force mode), built once; read only."""
    if name not in _scenes:
        prims, mats, env = build(spt, name), materials(spt), spt.reference_env(True)
        prims.setflags(write=False)
        _scenes[name] = (prims, mats, env, ref.RefScene(prims, mats, env, brute=True))
    return _scenes[name]


def magnitude(prims):
    """The scene's coordinate magnitude (the largest |coordinate| of a primitive's bounds, at least 1)."""
    m = 1.0
    for q in prims:
        if q["type"] == 0:
            pts = [q["p0"][:3] - q["p0"][3], q["p0"][:3] + q["p0"][3]]
        elif q["type"] == 1:
            pts = [q["p0"][:3], q["p0"][:3] + q["p1"][:3], q["p0"][:3] + q["p2"][:3], q["p0"][:3] + q["p1"][:3] + q["p2"][:3]]
        else:
            pts = [q["p0"][:3], q["p1"][:3], q["p2"][:3]]
        m = max(m, float(np.max(np.abs(pts))))
    return m


# ---- cameras ---------------------------------------------------------------------------------------------
# scene -> (centre, radius) the far cameras look at
LOOK = {"hf": ((0.0, -1.5, 6.0), 4.4), "mixed": ((0.0, 0.0, 7.0), 6.5)}
# the direction a far camera lies in, |.|_inf = 1
FAR_DIR = {"hf": (0.35, 1.0, -0.6), "mixed": (-0.45, 0.3, -1.0)}


def camera_of(spt, ref, scene, kind):
    """(camera or None, image width, height)."""
    off = np.array(OFFSET if scene == "offset" else (0.0, 0.0, 0.0))
    if kind == "ref":
        return None, W, H
    if kind.startswith("far"):
        r = int(kind[3:])
        centre, radius = LOOK[scene]
        if scene not in _mag:
            _mag[scene] = magnitude(scene_of(spt, ref, scene)[0])
        mag = _mag[scene]
        eye = np.array(FAR_DIR[scene]) * (r * mag)
        dist = float(np.linalg.norm(eye - np.array(centre)))
        return spt.look_at(tuple(eye), centre, vfov=2.0 * math.degrees(math.atan(radius / dist))), W, H
    if scene in ("hf", "offset", "refit"):
        if kind == "posed":
            return spt.look_at(tuple(off + (1.0, 0.5, 1.5)), tuple(off + (0.0, -1.5, 6.0)), vfov=60.0), W, H
        if kind == "inside":  # between the terrain's lowest and highest points
            return spt.look_at(tuple(off + (0.125, -1.4375, 6.125)), tuple(off + (2.0, -1.6, 8.0)), vfov=75.0), W, H
        # edges: 4 above the flat rows, straight down: pixel (x, y) meets y = -1 at (x / 8 - 4, 10 - y / 8)
        eye = off + (0.0, 3.0, 6.0)
        return spt.look_at(tuple(eye), tuple(eye - (0.0, 1.0, 0.0)), up=(0.0, 0.0, 1.0), vfov=90.0), 64, 64
    if scene == "ties":
        if kind == "posed":
            return spt.look_at((0.5, 0.5, 2.0), (0.0, 0.0, 6.0), vfov=70.0), W, H
        if kind == "inside":
            return spt.look_at((0.2, -0.1, 6.0), (-1.0, 0.5, 4.0), vfov=80.0), W, H
        # edges: exactly along +z at the centre of the stack in the plane z = 4 (all its quads tie there)
        return spt.look_at((-0.5, 0.0, 1.0), (-0.5, 0.0, 2.0), vfov=90.0), 64, 64
    if scene == "mixed":
        if kind == "posed":
            return spt.look_at((-1.0, 1.0, 1.0), (0.5, -0.5, 7.0), vfov=65.0), W, H
        if kind == "inside":  # inside the outer nested sphere, outside the middle one
            return spt.look_at((2.5, 0.9, 6.0), (2.4, -1.0, 6.2), vfov=100.0), W, H
        # edges: the centre ray through the point where the first two tangent spheres touch
        return spt.look_at((-1.75, 1.5, 1.0), (-1.75, 1.5, 2.0), vfov=90.0), 64, 64
    if scene == "scale":
        c0 = cluster_centres()[0]
        if kind == "posed":  # close in front of the first cluster: it fills the image
            return spt.look_at(tuple(c0 - (0.0, 0.0, 2.0 ** -5)), tuple(c0), vfov=40.0), W, H
        if kind == "inside":  # inside it
            return spt.look_at(tuple(c0), tuple(c0 + (0.3, 0.1, 1.0)), vfov=90.0), W, H
        return spt.look_at((0.0, 0.0, 3.5), (0.0, 0.0, 4.5), vfov=3.0), 64, 64  # along +z at both axis clusters
    raise KeyError((scene, kind))


def tmin_camera(spt, kind):
    """The reference camera, or test_gpu_axis_rays' uv0 (u = v = 0: every pixel gets the centre ray (0, 0, 1))."""
    if kind == "ref":
        return None
    cam = spt.SptCamera()
    cam.origin[:] = (0.0, 0.0, 0.0)
    cam.w[:] = (0.0, 0.0, 1.0)
    return cam


BASIC = ("ref", "posed", "inside", "edges")
CASES = ([("hf", k) for k in BASIC + tuple(f"far{r}" for r in FAR_R)] + [("ties", k) for k in BASIC] +
         [("tmin", "ref"), ("tmin", "uv0"), ("tmin_r", "ref"), ("tmin_r", "uv0")] + [("mixed", k) for k in BASIC + tuple(f"far{r}" for r in FAR_R)] +
         [("scale", k) for k in BASIC] + [("offset", k) for k in BASIC] + [(s, "ref") for s in SIZES] +
         [("refit", "ref"), ("refit", "posed"), ("refit", "edges")])


def case_camera(spt, ref, scene, kind):
    if scene in ("tmin", "tmin_r"):
        return tmin_camera(spt, kind), W, H
    if scene in SIZES:
        return None, W, H
    return camera_of(spt, ref, scene, kind)


# ---- expected values, computed once -------------------------------------------------------------------------
def want_features(spt, ref, scene, kind):
    key = (scene, kind, "features")
    if key not in _want:
        prims, mats, env, rs = scene_of(spt, ref, scene)
        cam, w, h = case_camera(spt, ref, scene, kind)
        got = dr.oracle_features(spt, ref, prims, mats, env, w, h, cam, scene=rs)
        for a in got:
            a.setflags(write=False)
        _want[key] = got
    return _want[key]


def want_frames(spt, ref, scene, kind, flags):
    key = (scene, kind, flags)
    if key not in _want:
        rs = scene_of(spt, ref, scene)[3]
        cam, w, h = case_camera(spt, ref, scene, kind)
        img = br.frame_radiance(spt, ref, rs, w, h, cam, FRAMES, BOUNCES, RR, flags)
        assert not np.isnan(img).any()  # (the scenes avoid NaN: its bits are not the same on every machine)
        img.setflags(write=False)
        _want[key] = img
    return _want[key]


# ---- the GPU side ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(spt):
    """One context for these tests (not the session's: a camera outlives spt_configure)."""
    c = spt.Context(0)
    yield c
    c.close()


def device_nodes(st, prims, mats, n_emit):
    """The 4-wide device tree's node count from spt_stats.scene_bytes (64-B primitive and node records, 32-B
    materials, 80-B emitters)."""
    rest = int(st.scene_bytes) - 64 * len(prims) - 32 * len(mats) - 80 * n_emit
    assert rest > 0 and rest % 64 == 0, (int(st.scene_bytes), len(prims), len(mats), n_emit)
    return rest // 64


def setup(spt, ref, ctx, scene, kind, flags):
    """The scene (refit: hf, then spt_update_prims), configuration and camera; returns (w, h, brute scene)."""
    prims, mats, env, rs = scene_of(spt, ref, scene)
    cam, w, h = case_camera(spt, ref, scene, kind)
    ctx.set_camera(None)
    ctx.set_tuning(bvh_max_leaf=SIZES[scene][2] if scene in SIZES else 0)  # (read by the next spt_set_scene)
    if scene == "refit":
        ctx.set_scene(height_field(spt), mats, env)
        ctx.update_prims(*moved_height_field(spt))
    else:
        ctx.set_scene(prims, mats, env)
    ctx.set_tuning()
    ctx.configure(w, h, BOUNCES, RR, flags)
    ctx.set_camera(cam)
    st = ctx.stats()
    assert st.bvh_nodes > 0 and int(st.emitters) == rs.emitter_count()
    return w, h, rs


@pytest.mark.parametrize("scene,kind", CASES)
def test_first_hits_equal_brute_force(spt, ref, ctx, scene, kind):
    want = want_features(spt, ref, scene, kind)
    prim = want[2].view(np.uint32)[..., 3]
    hit = prim != dr.MISS
    if not (scene == "offset" and kind == "ref"):  # (the reference camera looks past the translated field)
        assert hit.any(), "the camera sees nothing"
    setup(spt, ref, ctx, scene, kind, 0)
    ctx.render_features()
    for got, exp, lane in zip(ctx.read_features(), want, ("feat_a", "feat_b", "albedo")):
        br.assert_same(got, exp, f"{scene} camera {kind}: {lane}")
    print(f"{scene} camera {kind}: {int(hit.sum())} of {hit.size} pixels hit, {len(np.unique(prim[hit]))} primitives seen")


def run_schedules(spt, ref, ctx, scene, kind, nee):
    flags = spt.FLAG_NEE if nee else 0
    frames = want_frames(spt, ref, scene, kind, flags)
    what = f"{scene} camera {kind} nee={nee}"
    w, h, _ = setup(spt, ref, ctx, scene, kind, flags)
    # one-frame calls: k_frame (the first stores the camera hits, the later ones read them)
    for f in range(3):
        ctx.render(f, 1)
        assert int(ctx.stats().schedule) == spt.SCHEDULE_FRAME
        if f != 1:
            br.assert_same(ctx.read_accum(), br.accumulate(frames, 0, f + 1), f"{what}: one-frame call {f}")
    # one call: k_paths
    ctx.reset()
    ctx.render(0, FRAMES)
    assert int(ctx.stats().schedule) == spt.SCHEDULE_PERSISTENT
    br.assert_same(ctx.read_accum(), br.accumulate(frames, 0, FRAMES), f"{what}: k_paths")
    # the counting instantiations of both
    try:
        ctx.set_profiling(False, counters=True)
        ctx.reset()
        ctx.render(0, FRAMES)
        br.assert_same(ctx.read_accum(), br.accumulate(frames, 0, FRAMES), f"{what}: counting k_paths")
        ctx.reset()
        ctx.render(0, 1)
        br.assert_same(ctx.read_accum(), br.accumulate(frames, 0, 1), f"{what}: counting k_frame")
        assert int(ctx.stats().stalled_waves) == 0
    finally:
        ctx.set_profiling(False)
    # the wavefront schedules: split kernels, and sorted ray queues
    for fl in (spt.FLAG_WAVEFRONT | spt.FLAG_SPLIT_KERNELS,) + (() if nee else (spt.FLAG_SORTED_RAYS,)):
        setup(spt, ref, ctx, scene, kind, flags | fl)
        ctx.render(0, 2)
        ctx.render(2, FRAMES - 2)
        assert int(ctx.stats().schedule) in (spt.SCHEDULE_FUSED, spt.SCHEDULE_SPLIT)
        br.assert_same(ctx.read_accum(), br.accumulate(frames, 0, FRAMES), f"{what}: wavefront flags {fl:#x}")
    assert int(ctx.stats().stalled_waves) == 0


@pytest.mark.parametrize("scene,kind", CASES)
def test_whole_paths_equal_brute_force(spt, ref, ctx, scene, kind):
    run_schedules(spt, ref, ctx, scene, kind, False)
    if scene_of(spt, ref, scene)[3].emitter_count() > 0:
        run_schedules(spt, ref, ctx, scene, kind, True)


def test_tree_sizes_bracket_the_lds_copies(spt, ref, ctx):
    """The sizes' trees have the device node counts the module docstring says, so the set holds a tree of at
    most 5 nodes, one of 6..53, one of 54..64 and one just above 64 (the LDS top-of-tree copies hold 5, 53 or 64
    nodes; k_frame's small-tree form takes 64)."""
    seen = {}
    for scene, (n, _, leaf, want) in SIZES.items():
        prims, mats, _, rs = scene_of(spt, ref, scene)
        setup(spt, ref, ctx, scene, "ref", 0)
        st = ctx.stats()
        d = device_nodes(st, prims, mats, rs.emitter_count())
        print(f"{scene}: {n} primitives, {leaf or 1} per leaf: bvh_nodes {int(st.bvh_nodes)} (binary), "
              f"{d} device nodes, stack need {int(st.stack_need)}")
        assert d <= int(st.bvh_nodes) // 2 - 1  # (no more device nodes than binary interior nodes)
        assert d == want, (scene, d, want)
        seen[scene] = d
    ds = sorted(seen.values())
    assert any(d <= 5 for d in ds) and any(6 <= d <= 53 for d in ds) and any(54 <= d <= 64 for d in ds)
    assert any(64 < d <= 68 for d in ds)


def test_edge_camera_rays_run_along_cell_edges(spt, ref):
    """hf's edges camera: the centre row's rays have d.z == 0 and the centre column's d.x == 0 exactly (they lie
    in the planes z = 6 and x = 0 of two rows of cell edges), and every second pixel's exact ray meets the flat
    rows' plane y = -1 on a grid line."""
    cam, w, h = camera_of(spt, ref, "hf", "edges")
    for x in range(w):
        o, d = spt.camera_ray(cam, w, h, x, h // 2)
        assert d[2] == 0.0 and tuple(o) == (0.0, 3.0, 6.0)
    for y in range(h):
        assert spt.camera_ray(cam, w, h, w // 2, y)[1][0] == 0.0
    assert tuple(cam.u) == (1.0, 0.0, 0.0) and tuple(cam.v) == (0.0, 0.0, 1.0) and tuple(cam.w) == (0.0, -1.0, 0.0)
