"""TEST INFRASTRUCTURE -- ctypes binding of tests/castray/libcastray.so, the checker of xrt_cast_rays: the CPU oracle's
RayTracer.CastRay (RT:506-737) on caller-given rays (tests/castray/castray_ref.cpp includes oracle/oracle.cpp unmodified).
Scenes are built with the library's own orc_scene_* exports from the same specs as oracle_py.OracleScene."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB = os.path.join(_HERE, "castray", "libcastray.so")
SRC = os.path.join(_HERE, "castray", "castray_ref.cpp")
DEPS = [SRC, os.path.join(_ROOT, "oracle", "oracle.cpp"), os.path.join(_ROOT, "oracle", "xna_math.h"), os.path.join(_ROOT, "include", "xrt.h")]
FLAGS = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-associative-math", "-pthread"]   # the oracle Makefile's
_lib = None


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return
    subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", LIB, SRC])


def lib():
    global _lib
    if _lib is None:
        build()
        from oracle import oracle_py as orc
        l = C.CDLL(LIB)
        _bind_scene(l, orc)
        l.orc_cast_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def _bind_scene(l, orc):
    abi = orc.abi
    _F = C.POINTER(C.c_float)
    l.orc_scene_create.restype = C.c_void_p
    l.orc_scene_destroy.argtypes = [C.c_void_p]
    l.orc_last_error.restype = C.c_char_p
    l.orc_last_error.argtypes = [C.c_void_p]
    l.orc_scene_add_mesh.argtypes = [C.c_void_p, _F, _F, _F, _F, _F, C.c_int32, C.POINTER(abi.xrt_material), _F]
    l.orc_scene_add_object.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, _F, _F, _F, _F]
    l.orc_scene_build.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    l.orc_generate_primary_rays.argtypes = [C.POINTER(abi.xrt_camera), C.c_void_p]
    l.orc_render.argtypes = [C.c_void_p, C.POINTER(abi.xrt_camera), C.POINTER(abi.xrt_light), C.c_int32,
                             C.POINTER(abi.xrt_render_opts), C.c_void_p, C.c_void_p, C.POINTER(abi.xrt_stats),
                             C.c_int32, C.c_int32, C.c_int32]


class CastRayScene:
    """The oracle scene of a spec inside the checker's library, and CastRay on it."""

    def __init__(self, spec):
        from oracle import oracle_py as orc
        self.orc, self.spec = orc, spec
        L = lib()
        xna = orc.xna
        _fp = orc._fp
        self.h = C.c_void_p(L.orc_scene_create())
        for data, m in spec.meshes:
            a, keep = orc.material_abi(m)
            sn = np.ascontiguousarray(data.surface_normal, dtype=np.float32)
            rc = L.orc_scene_add_mesh(self.h, _fp(data.v), _fp(data.n), _fp(data.uv), _fp(sn), _fp(data.color), data.ntri,
                                      C.byref(a), _fp(np.ascontiguousarray(data.bbox, dtype=np.float32)))
            assert rc >= 0, L.orc_last_error(self.h)
        for ids, pos, rot, scale in spec.objects:
            bb = np.zeros(6, dtype=np.float32)
            for i in ids:
                bb[:3] = np.minimum(bb[:3], spec.meshes[i][0].bbox[:3])
                bb[3:] = np.maximum(bb[3:], spec.meshes[i][0].bbox[3:])
            world, inv, wbb = xna.build_world(scale, rot, pos, bb)
            idarr = np.array(ids, dtype=np.int32)
            rc = L.orc_scene_add_object(self.h, idarr.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), _fp(xna.as_array(world)),
                                        _fp(xna.as_array(inv)), _fp(bb), _fp(xna.as_array(wbb)))
            assert rc >= 0, L.orc_last_error(self.h)
        rc = L.orc_scene_build(self.h, spec.mesh_threshold, spec.scene_threshold)
        if rc != 0:
            raise RuntimeError(L.orc_last_error(self.h).decode())

    def __del__(self):
        try:
            if self.h:
                lib().orc_scene_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _lights(self):
        lights = (self.orc.abi.xrt_light * max(len(self.spec.lights), 1))()
        for i, l in enumerate(self.spec.lights):
            lights[i] = self.orc.light_abi(l)
        return lights

    def cast_rays(self, rays, iteration=0, ref_index=1.0, max_reflections=None):
        """CastRay on every ray -> (rgba uint32[n], rgb float32[n, 3], stats dict)."""
        rays = np.ascontiguousarray(rays, dtype=self.orc.RAY_DTYPE)
        opts = self.orc.opts_abi(self.spec)
        if max_reflections is not None:
            opts.max_reflections = max_reflections
        n = rays.shape[0]
        rgba = np.zeros(n, dtype=np.uint32)
        rgbf = np.zeros((n, 3), dtype=np.float32)
        st = self.orc.abi.xrt_stats()
        rc = lib().orc_cast_rays(self.h, self._lights(), len(self.spec.lights), C.byref(opts), rays.ctypes.data, n, int(iteration),
                                 float(ref_index), rgba.ctypes.data, rgbf.ctypes.data, C.byref(st))
        if rc != 0:
            raise RuntimeError("orc_cast_rays failed: %d" % rc)
        return rgba, rgbf, st.as_dict()

    def primary_rays(self):
        cam = self.orc.camera_abi(self.spec)
        rays = np.zeros(self.spec.width * self.spec.height, dtype=self.orc.RAY_DTYPE)
        assert lib().orc_generate_primary_rays(C.byref(cam), rays.ctypes.data) == 0
        return rays

    def render(self, max_reflections=None):
        """orc_render of the spec's camera (MS as in the spec) in this library -> (rgba, rgbf, stats)."""
        spec = self.spec
        cam, opts = self.orc.camera_abi(spec), self.orc.opts_abi(spec)
        if max_reflections is not None:
            opts.max_reflections = max_reflections
        rgba = np.zeros(spec.width * spec.height, dtype=np.uint32)
        rgbf = np.zeros((spec.width * spec.height, 3), dtype=np.float32)
        st = self.orc.abi.xrt_stats()
        rc = lib().orc_render(self.h, C.byref(cam), self._lights(), len(spec.lights), C.byref(opts), rgba.ctypes.data, rgbf.ctypes.data,
                              C.byref(st), 1, 0, spec.height)
        if rc != 0:
            raise RuntimeError("oracle render failed: %d" % rc)
        return rgba, rgbf, st.as_dict()
