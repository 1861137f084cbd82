"""TEST INFRASTRUCTURE -- ctypes binding of tests/paths/libpaths.so, the checker of xrt_cast_rays_paths.

paths_ref.cpp: the CPU oracle (oracle/oracle.cpp, included unmodified through tests/castray/castray_ref.cpp) plus orc_paths_run, its CastRay
with the list RayTracer.points kept (RT:543, 701, 740-747) and the `ref Ray ray` handed back (RT:692-694).  The oracle's CastRay has no hook
for the list, so orc_paths_run restates the recursion; PathsScene.cast_rays_paths pins the restatement on EVERY batch it is used for: its
colours, colour vectors and counters must equal orc_cast_rays' of the same library bit for bit, else it raises.
paths_order.cpp: the library's own ordering rule (csrc/paths.h) compiled for the CPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import castray_py

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")
LIB = os.path.join(_HERE, "paths", "libpaths.so")
SRCS = [os.path.join(_HERE, "paths", "paths_ref.cpp"), os.path.join(_HERE, "paths", "paths_order.cpp")]
DEPS = SRCS + [os.path.join(_HERE, "castray", "castray_ref.cpp"), os.path.join(_ROOT, "oracle", "oracle.cpp"), os.path.join(_ROOT, "oracle", "xna_math.h"),
               os.path.join(_ROOT, "include", "xrt.h"), os.path.join(_CSRC, "paths.h"), os.path.join(_CSRC, "xrt_core.h")]
VERTEX_DTYPE = np.dtype([("position", np.float32, (3,)), ("color", np.uint32)])   # xrt_path_vertex / VertexPositionColor
WHITE, RED = 0xFFFFFFFF, 0xFF0000FF
_lib = None


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return
    subprocess.check_call(["g++"] + castray_py.FLAGS + ["-shared", "-o", LIB] + SRCS)


def lib():
    global _lib
    if _lib is None:
        build()
        from oracle import oracle_py as orc
        l = C.CDLL(LIB)
        castray_py._bind_scene(l, orc)
        l.orc_cast_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_paths_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_paths_sizes.argtypes = [C.c_void_p]
        l.orc_paths_sizes.restype = None
        l.orc_paths_copy.argtypes = [C.c_void_p] * 6
        l.orc_paths_copy.restype = None
        l.xrt_paths_order_cpu.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        l.xrt_paths_order_cpu.restype = C.c_int64
        l.xrt_paths_node.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        l.xrt_paths_node.restype = C.c_int32
        l.xrt_paths_bound.argtypes = [C.c_int32, C.c_int32]
        l.xrt_paths_bound.restype = C.c_int64
        _lib = l
    return _lib


def bits(a):
    """The raw 32-bit words of an array of 4-byte items or of a structured array made of them (NaNs compare by pattern)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(-1)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


class PathsResult:
    def __init__(self, rgba, rgbf, stats, vertices, vertex_start, rays_back, recs, tree):
        self.rgba, self.rgbf, self.stats, self.vertices, self.vertex_start, self.rays_back = rgba, rgbf, stats, vertices, vertex_start, rays_back
        self.recs, self.tree = recs, tree   # recs: (ray int64[], node int32[], kind int32[], v float32[, 3]) -- the recursion trees
        self.n_vertices = int(vertices.shape[0])


class PathsScene(castray_py.CastRayScene):
    """The oracle scene of a spec inside libpaths.so; CastRay with the list kept."""

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

    def cast_rays_paths(self, rays, iteration=0, ref_index=1.0, max_reflections=None):
        rays = np.ascontiguousarray(rays, dtype=self.orc.RAY_DTYPE)
        opts = self.orc.opts_abi(self.spec)
        if max_reflections is not None:
            opts.max_reflections = max_reflections
        n = rays.shape[0]
        L = lib()
        lights = self._lights()
        out = []
        for fn in ("paths", "plain"):
            rgba = np.zeros(n, dtype=np.uint32)
            rgbf = np.zeros((n, 3), dtype=np.float32)
            st = self.orc.abi.xrt_stats()
            if fn == "paths":
                back = np.zeros(n, dtype=self.orc.RAY_DTYPE)
                rc = L.orc_paths_run(self.h, lights, len(self.spec.lights), C.byref(opts), rays.ctypes.data, n, int(iteration), float(ref_index),
                                     rgba.ctypes.data, rgbf.ctypes.data, back.ctypes.data, C.byref(st))
            else:
                rc = L.orc_cast_rays(self.h, lights, len(self.spec.lights), C.byref(opts), rays.ctypes.data, n, int(iteration), float(ref_index),
                                     rgba.ctypes.data, rgbf.ctypes.data, C.byref(st))
            if rc != 0:
                raise RuntimeError("checker failed: %d" % rc)
            out.append((rgba, rgbf, st.as_dict()))
        # the restatement is the oracle's CastRay: colours, colour vectors and counters bit for bit
        (rgba, rgbf, st), (o_rgba, o_rgbf, o_st) = out
        if not (np.array_equal(rgba, o_rgba) and same_bits(rgbf, o_rgbf)):
            raise AssertionError("tests/paths/paths_ref.cpp is no longer the oracle's CastRay: colours differ")
        for k, v in o_st.items():
            if not k.startswith("ms_") and st[k] != v:
                raise AssertionError("tests/paths/paths_ref.cpp is no longer the oracle's CastRay: %s %r != %r" % (k, st[k], v))
        sizes = (C.c_int64 * 3)()
        L.orc_paths_sizes(sizes)
        nv, nr, tree = int(sizes[0]), int(sizes[1]), bool(sizes[2])
        vertices = np.zeros(nv, dtype=VERTEX_DTYPE)
        vstart = np.zeros(n + 1, dtype=np.int64)
        rec_ray, rec_node, rec_kind = np.zeros(nr, dtype=np.int64), np.zeros(nr, dtype=np.int32), np.zeros(nr, dtype=np.int32)
        rec_v = np.zeros((nr, 3), dtype=np.float32)
        L.orc_paths_copy(vertices.ctypes.data, vstart.ctypes.data, rec_ray.ctypes.data, rec_node.ctypes.data, rec_kind.ctypes.data, rec_v.ctypes.data)
        return PathsResult(rgba, rgbf, st, vertices, vstart, back, (rec_ray, rec_node, rec_kind, rec_v), tree)


def order_cpu(rays, depth, tree, recs, capacity=None):
    """csrc/paths.h on the CPU: node records -> (n_vertices, vertices, vertex_start, rays_back)."""
    from oracle import oracle_py as orc
    rays = np.ascontiguousarray(rays, dtype=orc.RAY_DTYPE)
    n = rays.shape[0]
    rec_ray, rec_node, rec_kind, rec_v = (np.ascontiguousarray(a) for a in recs)
    L = lib()
    vstart = np.zeros(n + 1, dtype=np.int64)
    back = np.zeros(n, dtype=orc.RAY_DTYPE)
    if capacity is None:
        capacity = int(L.xrt_paths_bound(int(depth), int(tree))) * n
    vertices = np.zeros(max(capacity, 1), dtype=VERTEX_DTYPE)
    need = L.xrt_paths_order_cpu(rays.ctypes.data, n, int(depth), int(tree), rec_ray.shape[0], rec_ray.ctypes.data, rec_node.ctypes.data, rec_kind.ctypes.data,
                                 rec_v.ctypes.data, vertices.ctypes.data, int(capacity), vstart.ctypes.data, back.ctypes.data)
    return int(need), vertices[:min(int(need), capacity & ~1)], vstart, back
