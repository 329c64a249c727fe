"""The checker of the material tests: ctypes binding of tests/cpp/libref_materials.so (ref_materials.c, the
oracle's integrator restated with material models) and the two test scenes. Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "cpp", "libref_materials.so")
BOUNCES, RR = 5, 2
SIZES = [(37, 23), (48, 32)]

_lib = None


class _Env(ctypes.Structure):  # == spt_env
    _fields_ = [("sky_enabled", ctypes.c_uint32), ("horizon", ctypes.c_float * 3), ("zenith", ctypes.c_float * 3)]


class _MatScene(ctypes.Structure):  # == ref_materials.c mat_scene
    _fields_ = [("scene", ctypes.c_void_p), ("prims", ctypes.c_void_p), ("mats", ctypes.c_void_p),
                ("models", ctypes.c_void_p), ("env", _Env), ("env_map", ctypes.c_void_p),
                ("env_w", ctypes.c_uint32), ("env_h", ctypes.c_uint32)]


def load():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "cpp", "ref_materials.c")
        if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(src):
            subprocess.run(["make", "-s", "-C", ROOT, "oracle"], check=True)
        lib = ctypes.CDLL(LIB_PATH)
        P, U32, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        FP = ctypes.POINTER(ctypes.c_float)
        lib.mat_trace_ray.argtypes = [P, P, FP, FP, ctypes.POINTER(U32), FP]
        lib.mat_trace_ray.restype = None
        lib.mat_render_frames.argtypes = [P, P, U32, U32, P]
        lib.mat_render_frames.restype = None
        lib.mat_bsdf_sample.argtypes = [P, FP, FP, I, U32, ctypes.POINTER(U32), FP, ctypes.POINTER(I), ctypes.POINTER(I)]
        lib.mat_bsdf_sample.restype = None
        _lib = lib
    return _lib


class MatScene:
    """A scene of the restatement: the oracle's RefScene plus the caller's arrays and the models (or None)."""

    def __init__(self, spt, ref, prims, mats, env, models=None, env_map=None):
        self.lib = load()
        self.ref = ref
        self.prims = np.ascontiguousarray(prims)
        self.mats = np.ascontiguousarray(mats)
        self.models = None if models is None else spt.material_models(models)
        self.env = env
        self.rs = ref.RefScene(self.prims, self.mats, env)
        self.env_map = None if env_map is None else np.ascontiguousarray(env_map, dtype=np.float32)
        if self.env_map is not None:
            self.rs.set_env_map(self.env_map)
        m = _MatScene()
        m.scene = self.rs.h
        m.prims = self.prims.ctypes.data
        m.mats = self.mats.ctypes.data
        m.models = None if self.models is None else self.models.ctypes.data
        m.env.sky_enabled = env.sky_enabled
        m.env.horizon[:] = list(env.horizon)
        m.env.zenith[:] = list(env.zenith)
        if self.env_map is not None:
            m.env_map = self.env_map.ctypes.data
            m.env_w, m.env_h = self.env_map.shape[1], self.env_map.shape[0]
        self.c = m

    def frames(self, w, h, first, n, flags=0, bounces=BOUNCES, rr=RR):
        """[n, h, w, 4] float32: trace_ray's (L, 1) per pixel of frames first .. first + n - 1, the reference's camera."""
        cfg = self.ref.RefConfig(w, h, bounces, rr, flags)
        out = np.zeros((n, h, w, 4), dtype=np.float32)
        self.lib.mat_render_frames(ctypes.byref(self.c), ctypes.byref(cfg), first, n, out.ctypes.data)
        out.setflags(write=False)
        return out

    def trace(self, cfg, o, d, state):
        """mat_trace_ray from the ray (o, d: ctypes float[3]) and RNG state (ctypes uint32, advanced): (L, 1)."""
        out = (ctypes.c_float * 4)()
        self.lib.mat_trace_ray(ctypes.byref(self.c), ctypes.byref(cfg), o, d, ctypes.byref(state), out)
        return out[:]


def bsdf_sample(spt, kind, param, d, n, entering, state, flags=0):
    """The restatement's step with spt_bsdf_sample's interface: (direction, transmitted, absorbed, state)."""
    m = spt.material_models([(kind, param)])
    f3 = ctypes.c_float * 3
    out = np.zeros(3, dtype=np.float32)
    st, tr, ab = ctypes.c_uint32(state), ctypes.c_int(0), ctypes.c_int(0)
    load().mat_bsdf_sample(m.ctypes.data, f3(*d), f3(*n), int(bool(entering)), flags, ctypes.byref(st),
                           out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(tr), ctypes.byref(ab))
    return out, bool(tr.value), bool(ab.value), st.value


def accumulate(frames, first, n):
    """The accumulation buffer after frames [first, first + n), added in frame order in float32."""
    acc = np.zeros(frames.shape[1:], dtype=np.float32)
    for f in range(first, first + n):
        acc = acc + frames[f]
    return acc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def assert_same(got, want, what):
    g, r = bits(got), bits(want)
    bad = np.flatnonzero(np.any(g != r, axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} pixels differ, first {bad[:5]}"


# ---- the test scenes ----------------------------------------------------------------------------------
def _append_material(spt, mats, albedo, emission=(0.0, 0.0, 0.0)):
    m = np.zeros(1, dtype=spt.MATERIAL_DTYPE)
    m[0]["albedo"] = albedo
    m[0]["emission"] = emission
    return np.concatenate([mats, m])


def cornell_materials(spt):
    """Cornell (a flat scene) with its spheres METAL(0) and DIELECTRIC(1.5) on material entries of their own
    and a METAL(0.4) back wall: (prims, mats, env, models)."""
    prims, mats, env = spt.build_scene("cornell")
    prims = prims.copy()
    spheres = [i for i in range(len(prims)) if prims[i]["type"] == 0]
    back = [i for i in range(len(prims)) if prims[i]["type"] == 1 and prims[i]["p0"][2] == 8.0]
    assert len(spheres) == 2 and len(back) == 1
    models = [(spt.MAT_DIFFUSE, 0.0)] * len(mats)
    for i, (albedo, model) in zip(spheres + back, [((0.9, 0.85, 0.8), (spt.MAT_METAL, 0.0)),
                                                    ((0.95, 0.95, 0.95), (spt.MAT_DIELECTRIC, 1.5)),
                                                    ((0.73, 0.73, 0.73), (spt.MAT_METAL, 0.4))]):
        mats = _append_material(spt, mats, albedo)
        prims[i]["material"] = len(mats) - 1
        models.append(model)
    return prims, mats, env, models


def app_materials(spt):
    """The App scene (38 spheres: a BVH scene) with every third grid sphere METAL(0.2) or DIELECTRIC(1.33) in
    turn, one grid sphere an emitter (so SPT_FLAG_NEE has something to sample), and a small closed tetrahedron
    of DIELECTRIC(1.5) triangles wound outward in front of the first sphere: (prims, mats, env, models)."""
    prims, mats, env = spt.build_scene("app")
    prims = prims.copy()
    models = [(spt.MAT_DIFFUSE, 0.0)] * len(mats)
    mats = _append_material(spt, mats, (0.8, 0.8, 0.9))
    models.append((spt.MAT_METAL, 0.2))
    mats = _append_material(spt, mats, (0.95, 1.0, 0.95))
    models.append((spt.MAT_DIELECTRIC, 1.33))
    mats = _append_material(spt, mats, (0.7, 0.7, 0.7), (6.0, 5.0, 4.0))
    models.append((spt.MAT_DIFFUSE, 0.0))
    mats = _append_material(spt, mats, (1.0, 0.95, 0.9))
    models.append((spt.MAT_DIELECTRIC, 1.5))
    metal, glass, light, tetra = len(mats) - 4, len(mats) - 3, len(mats) - 2, len(mats) - 1
    for j, i in enumerate(range(2, len(prims), 3)):  # (prims 0 and 1 are C1's two spheres; then the 6 x 6 grid)
        prims[i]["material"] = metal if j % 2 == 0 else glass
    prims[len(prims) - 15]["material"] = light
    # a tetrahedron around (0.9, 0.3, 3.0), faces wound so that cross(v1 - v0, v2 - v0) points outward
    a, b, c, d = (np.array(v, dtype=np.float32) for v in ((0.5, 0.0, 3.3), (1.3, 0.0, 3.3), (0.9, 0.0, 2.6), (0.9, 0.7, 3.05)))
    centre = (a + b + c + d) / 4
    tris = np.zeros(4, dtype=spt.PRIM_DTYPE)
    for t, (v0, v1, v2) in enumerate(((a, b, c), (a, b, d), (b, c, d), (c, a, d))):
        if np.dot(np.cross(v1 - v0, v2 - v0), v0 - centre) < 0:
            v1, v2 = v2, v1
        tris[t]["type"] = 2
        tris[t]["material"] = tetra
        tris[t]["p0"][:3], tris[t]["p1"][:3], tris[t]["p2"][:3] = v0, v1, v2
    return np.concatenate([prims, tris]), mats, env, models
