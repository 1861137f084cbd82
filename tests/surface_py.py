"""TEST INFRASTRUCTURE -- ctypes binding of tests/surface/libsurface.so, the checker of xrt_surface_hits.

surface_ref.cpp: the CPU oracle (oracle/oracle.cpp, included unmodified through tests/castray/castray_ref.cpp) plus orc_surface_hits, what its
CastRay computes at a hit without asking the scene anything -- fragment normal (RT:520-531), surface colour (RT:568-581, the oracle's own
SurfaceColor), the reflected ray (RT:547-550) and the Snell refraction (RT:656-694) -- on an IntersectionResult built from an xrt_hit.
tests/test_surface_cpu.py pins the restatement against orc_cast_rays and orc_paths_run."""
import ctypes as C
import os
import subprocess

import numpy as np

import castray_py
import lights_py as lp
import shade_hits_py as sh

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")
LIB = os.path.join(_HERE, "surface", "libsurface.so")
SRC = os.path.join(_HERE, "surface", "surface_ref.cpp")
DEPS = [SRC, os.path.join(_HERE, "castray", "castray_ref.cpp"), os.path.join(_ROOT, "oracle", "oracle.cpp"), os.path.join(_ROOT, "oracle", "xna_math.h"),
        os.path.join(_ROOT, "include", "xrt.h")]
COUNTS = ("live", "interpolated", "textured", "transparent", "index_equal", "index_differs", "cos_nonneg", "cos_neg", "nan_direction")
SURFACE_DTYPE = np.dtype([("normal", np.float32, 3), ("reflectiveness", np.float32), ("color", np.float32, 3), ("alpha", np.float32),
                          ("uv", np.float32, 2), ("refraction_index", np.float32), ("next_ref_index", np.float32), ("flags", np.int32),
                          ("reserved", np.int32, 3)])
assert SURFACE_DTYPE.itemsize == 64
SURF_HIT, SURF_TRANSPARENT, SURF_INTERPOLATED, SURF_TEXTURED = 1, 2, 4, 8
FLOAT_FIELDS = ("normal", "reflectiveness", "color", "alpha", "uv", "refraction_index", "next_ref_index")
_lib = None

bits, same_bits, same_floats = sh.bits, sh.same_bits, lp.same_floats


def same_surface(a, b):
    """Two arrays of surface records: the float fields bit for bit but NaN == NaN of any payload, flags and reserved words equal."""
    if a.shape != b.shape:
        return False
    return all(same_floats(a[f], b[f]) for f in FLOAT_FIELDS) and np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["reserved"], b["reserved"])


def same_rays(a, b):
    """Two arrays of ray records: origin and direction as same_floats, the ignore pair equal."""
    if a.shape != b.shape:
        return False
    return same_floats(a["o"], b["o"]) and same_floats(a["d"], b["d"]) and np.array_equal(a["ignore_mesh"], b["ignore_mesh"]) and \
        np.array_equal(a["ignore_tri"], b["ignore_tri"])


def same_outputs(got, want):
    """(surface, reflect, refract) against (surface, reflect, refract)."""
    return same_surface(got[0], want[0]) and same_rays(got[1], want[1]) and same_rays(got[2], want[2])


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return
    subprocess.check_call(["g++"] + castray_py.FLAGS + ["-shared", "-o", LIB, SRC])


def build_checked():
    """xrt_surface_hits' host program on a host-only scene under ASan + UBSan (csrc/Makefile `hostcheck_surface`)."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "hostcheck_surface"])
    return os.path.join(CSRC, "hostcheck_surface")


def lib():
    global _lib
    if _lib is None:
        build()
        from oracle import oracle_py as orc
        l = C.CDLL(LIB)
        castray_py._bind_scene(l, orc)
        l.orc_cast_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_surface_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_scene_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def refraction_cases(rays, hits, surf):
    """The batches that take CastRay's refraction (RT:656-694) through every branch, from the hits of a scene with Transparent bodies: the
    Transparent entries as they were traced (the ray arrives from outside: cos1 >= 0) and with the direction reversed (from inside: cos1 < 0),
    each with current_ref_index = the first such entry's RefractionIndex (RT:658: equal) and = 1.0 (RT:663: not equal; n1 / n2 is then the
    material's index, and a ray that grazes the surface refracts into the square root of a negative number: a NaN direction).
    -> [(what, rays, hits, current_ref_index)]"""
    t = np.flatnonzero((surf["flags"] & SURF_TRANSPARENT) != 0)
    assert len(t) > 0, "no Transparent entry"
    index = float(surf["refraction_index"][t[0]])
    assert index != 1.0
    inside = rays[t].copy()
    inside["d"] = -inside["d"]
    out = []
    for what, r in (("outside", rays[t].copy()), ("inside", inside)):
        for cur in (index, 1.0):
            out.append(("%s, current index %g" % (what, cur), r, hits[t].copy(), cur))
    return out


class SurfaceScene(sh.ShadeHitsScene):
    """The oracle scene of a spec inside libsurface.so: the query, CastRay, and the surface terms and next rays behind a given query result."""

    def __init__(self, spec):
        sh_lib = sh.lib
        sh.lib = lib          # (ShadeHitsScene builds and uses its scene in whichever library `lib()` names)
        try:
            super().__init__(spec)
        finally:
            sh.lib = sh_lib

    def _call(self, fn):
        sh_lib = sh.lib
        sh.lib = lib
        try:
            return fn()
        finally:
            sh.lib = sh_lib

    def __del__(self):
        try:
            if self.h:
                lib().orc_scene_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def intersect(self, rays):
        return self._call(lambda: sh.ShadeHitsScene.intersect(self, rays))

    def cast_rays(self, rays, **kw):
        return self._call(lambda: sh.ShadeHitsScene.cast_rays(self, rays, **kw))

    def render(self, max_reflections=None):
        return self._call(lambda: sh.ShadeHitsScene.render(self, max_reflections))

    def surface_hits(self, hits, rays=None, ref_index=1.0, address_mode=None, filtering=None):
        """-> (surface SURFACE_DTYPE[n], reflect RAY_DTYPE[n], refract RAY_DTYPE[n], counts dict of COUNTS).  Without rays the ray outputs
        are None and the refraction counts 0."""
        hits = np.ascontiguousarray(hits, dtype=self.orc.HIT_DTYPE)
        n = hits.shape[0]
        opts = self._opts(None)
        if address_mode is not None:
            opts.address_mode = int(address_mode)
        if filtering is not None:
            opts.filtering = int(filtering)
        surf = np.zeros(n, dtype=SURFACE_DTYPE)
        counts = np.zeros(len(COUNTS), dtype=np.uint64)
        refl = refr = None
        if rays is not None:
            rays = np.ascontiguousarray(rays, dtype=self.orc.RAY_DTYPE)
            assert rays.shape[0] == n
            refl, refr = np.zeros(n, dtype=self.orc.RAY_DTYPE), np.zeros(n, dtype=self.orc.RAY_DTYPE)
        rc = lib().orc_surface_hits(self.h, C.byref(opts), rays.ctypes.data if rays is not None else None, hits.ctypes.data, n, float(ref_index),
                                    surf.ctypes.data, refl.ctypes.data if rays is not None else None, refr.ctypes.data if rays is not None else None,
                                    counts.ctypes.data)
        if rc != 0:
            raise RuntimeError("orc_surface_hits failed: %d" % rc)
        return surf, refl, refr, dict(zip(COUNTS, (int(v) for v in counts)))
