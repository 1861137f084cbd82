"""TEST INFRASTRUCTURE -- ctypes binding of tests/shade_hits/libshade_hits.so, the checker of xrt_shade_hits.

shade_hits_ref.cpp: the CPU oracle (oracle/oracle.cpp, included unmodified through tests/castray/castray_ref.cpp) plus orc_shade_hits, one
level of its CastRay (RT:514-737) on an IntersectionResult built from an xrt_hit, with the oracle's own IsLightPathObstructed and CastRay
below.  tests/test_shade_hits_cpu.py pins the restatement against orc_cast_rays of the same library."""
import ctypes as C
import os
import subprocess

import numpy as np

import castray_py

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB = os.path.join(_HERE, "shade_hits", "libshade_hits.so")
SRC = os.path.join(_HERE, "shade_hits", "shade_hits_ref.cpp")
DEPS = [SRC, os.path.join(_HERE, "castray", "castray_ref.cpp"), os.path.join(_ROOT, "oracle", "oracle.cpp"), os.path.join(_ROOT, "oracle", "xna_math.h"),
        os.path.join(_ROOT, "include", "xrt.h")]
# the reference work counters of xrt_stats (what collect_stats fills), and the four that are always filled
WORK = ("scene_node_tests", "instance_visits", "mesh_aabb_tests", "mesh_queries", "node_tests", "leaf_refs", "tri_tests", "hits_shadow")
RAYS = ("rays_closest", "hits_closest", "rays_shadow", "shaded_hits")
_lib = None


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return
    subprocess.check_call(["g++"] + castray_py.FLAGS + ["-shared", "-o", LIB, SRC])


def lib():
    global _lib
    if _lib is None:
        build()
        from oracle import oracle_py as orc
        l = C.CDLL(LIB)
        castray_py._bind_scene(l, orc)
        l.orc_cast_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_shade_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_scene_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def bits(a):
    """The raw 32-bit words of an array of 4-byte items or of a structured array made of them (NaNs compare by pattern)."""
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


class ShadeHitsScene(castray_py.CastRayScene):
    """The oracle scene of a spec inside libshade_hits.so: the query, CastRay, and CastRay behind a given query result."""

    def __init__(self, spec):
        castray_py_lib = castray_py.lib
        castray_py.lib = lib          # (CastRayScene builds its scene in whichever library `lib()` names)
        try:
            super().__init__(spec)
        finally:
            castray_py.lib = castray_py_lib

    def __del__(self):
        try:
            if self.h:
                lib().orc_scene_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _opts(self, max_reflections):
        opts = self.orc.opts_abi(self.spec)
        if max_reflections is not None:
            opts.max_reflections = max_reflections
        return opts

    def _spec_lights(self, lights):
        src = self.spec.lights if lights is None else lights
        arr = (self.orc.abi.xrt_light * max(len(src), 1))()
        for i, l in enumerate(src):
            arr[i] = self.orc.light_abi(l)
        return arr, len(src)

    def render(self, max_reflections=None):
        spec = self.spec
        cam, opts = self.orc.camera_abi(spec), self._opts(max_reflections)
        rgba, rgbf, st = np.zeros(spec.width * spec.height, dtype=np.uint32), np.zeros((spec.width * spec.height, 3), dtype=np.float32), self.orc.abi.xrt_stats()
        larr, nl = self._spec_lights(None)
        rc = lib().orc_render(self.h, C.byref(cam), larr, nl, C.byref(opts), rgba.ctypes.data, rgbf.ctypes.data, C.byref(st), 1, 0, spec.height)
        if rc != 0:
            raise RuntimeError("oracle render failed: %d" % rc)
        return rgba, rgbf, st.as_dict()

    def intersect(self, rays):
        """GetRayIntersection on every ray -> (hits HIT_DTYPE[n], stats dict: the counters of the n queries)."""
        rays = np.ascontiguousarray(rays, dtype=self.orc.RAY_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=self.orc.HIT_DTYPE)
        st = self.orc.abi.xrt_stats()
        rc = lib().orc_scene_intersect(self.h, rays.ctypes.data, rays.shape[0], hits.ctypes.data, C.byref(st))
        if rc != 0:
            raise RuntimeError("orc_scene_intersect failed: %d" % rc)
        return hits, st.as_dict()

    def cast_rays(self, rays, iteration=0, ref_index=1.0, max_reflections=None, lights=None):
        rays = np.ascontiguousarray(rays, dtype=self.orc.RAY_DTYPE)
        opts = self._opts(max_reflections)
        n = rays.shape[0]
        rgba, rgbf, st = np.zeros(n, dtype=np.uint32), np.zeros((n, 3), dtype=np.float32), self.orc.abi.xrt_stats()
        larr, nl = self._spec_lights(lights)
        rc = lib().orc_cast_rays(self.h, larr, nl, C.byref(opts), rays.ctypes.data, n, int(iteration), float(ref_index), rgba.ctypes.data,
                                 rgbf.ctypes.data, C.byref(st))
        if rc != 0:
            raise RuntimeError("orc_cast_rays failed: %d" % rc)
        return rgba, rgbf, st.as_dict()

    def shade_hits(self, rays, hits, iteration=0, ref_index=1.0, max_reflections=None, lights=None):
        """CastRay behind "the query returned hits[i]" -> (rgba uint32[n], rgb float32[n, 3], stats dict)."""
        rays = np.ascontiguousarray(rays, dtype=self.orc.RAY_DTYPE)
        hits = np.ascontiguousarray(hits, dtype=self.orc.HIT_DTYPE)
        assert hits.shape[0] == rays.shape[0]
        opts = self._opts(max_reflections)
        n = rays.shape[0]
        rgba, rgbf, st = np.zeros(n, dtype=np.uint32), np.zeros((n, 3), dtype=np.float32), self.orc.abi.xrt_stats()
        larr, nl = self._spec_lights(lights)
        rc = lib().orc_shade_hits(self.h, larr, nl, C.byref(opts), rays.ctypes.data, hits.ctypes.data, n, int(iteration), float(ref_index),
                                  rgba.ctypes.data, rgbf.ctypes.data, C.byref(st))
        if rc != 0:
            raise RuntimeError("orc_shade_hits failed: %d" % rc)
        return rgba, rgbf, st.as_dict()
