"""TEST INFRASTRUCTURE -- ctypes binding of tests/lights/liblights.so, the checker of xrt_light_hits.

lights_ref.cpp: the CPU oracle (oracle/oracle.cpp, included unmodified through tests/castray/castray_ref.cpp) plus orc_light_hits, the light
loop of its CastRay (RT:520-542) on an IntersectionResult built from an xrt_hit, with the oracle's own IsLightPathObstructed and
GetLightForFragment.  tests/test_lights_cpu.py pins the restatement against orc_cast_rays of the same library."""
import ctypes as C
import os
import subprocess

import numpy as np

import castray_py
import shade_hits_py as sh

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")
LIB = os.path.join(_HERE, "lights", "liblights.so")
SRC = os.path.join(_HERE, "lights", "lights_ref.cpp")
DEPS = [SRC, os.path.join(_HERE, "castray", "castray_ref.cpp"), os.path.join(_ROOT, "oracle", "oracle.cpp"), os.path.join(_ROOT, "oracle", "xna_math.h"),
        os.path.join(_ROOT, "include", "xrt.h")]
COUNTS = ("obstructed", "transparent", "beyond", "live")
_lib = None

bits, same_bits = sh.bits, sh.same_bits


def same_floats(a, b):
    """Bit for bit, but a NaN equals a NaN of any payload."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return
    subprocess.check_call(["g++"] + castray_py.FLAGS + ["-shared", "-o", LIB, SRC])


def build_checked():
    """The chunk planner's host program under ASan + UBSan (csrc/Makefile `hostcheck_lights`)."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "hostcheck_lights"])
    return os.path.join(CSRC, "hostcheck_lights")


def lib():
    global _lib
    if _lib is None:
        build()
        from oracle import oracle_py as orc
        l = C.CDLL(LIB)
        castray_py._bind_scene(l, orc)
        l.orc_cast_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_light_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_scene_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


class LightsScene(sh.ShadeHitsScene):
    """The oracle scene of a spec inside liblights.so: the query, CastRay, and the light loop behind a given query result."""

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

    def light_hits(self, hits, lights=None, want_color=False):
        """-> (light float32[n, 3], amounts float32[n, n_lights], counts dict of COUNTS[, surface colour float32[n, 3]])."""
        hits = np.ascontiguousarray(hits, dtype=self.orc.HIT_DTYPE)
        n = hits.shape[0]
        larr, nl = self._spec_lights(lights)
        opts = self._opts(None)
        light, amounts = np.zeros((n, 3), dtype=np.float32), np.zeros((n, nl), dtype=np.float32)
        counts = np.zeros(4, dtype=np.uint64)
        color = np.zeros((n, 3), dtype=np.float32) if want_color else None
        rc = lib().orc_light_hits(self.h, larr, nl, C.byref(opts), hits.ctypes.data, n, light.ctypes.data, amounts.ctypes.data, counts.ctypes.data,
                                  color.ctypes.data if want_color else None)
        if rc != 0:
            raise RuntimeError("orc_light_hits failed: %d" % rc)
        out = (light, amounts, dict(zip(COUNTS, (int(v) for v in counts))))
        return out + (color,) if want_color else out
