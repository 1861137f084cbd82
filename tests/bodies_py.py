"""TEST INFRASTRUCTURE -- the checkers of xrt_scene_set_bodies (tests/test_bodies_cpu.py, tests/test_gpu_bodies.py).

tests/bodies/libemulbodies.so: tests/emul (included unmodified) plus emu_set_bodies, which calls the product's own host-side list edit
(HostScene::set_bodies), and emu_compare, a memcmp of everything two HostScenes hold after a build.
A scene under edit is described by a SceneSpec whose `meshes` are in the order the edited scene numbers them (order of addition; meshes
no body uses included) and whose `objects` are the current list: that spec is what a from-scratch scene and the oracle are given."""
import copy
import ctypes as C
import importlib
import os
import subprocess

import numpy as np

from poses_py import body_box, hits_equal, pose_arrays   # noqa: F401  (hits_equal: for the tests)

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")
EMU_LIB = os.path.join(_HERE, "bodies", "libemulbodies.so")
EMU_SRCS = [os.path.join(_HERE, "bodies", "emul_bodies.cpp"), os.path.join(_CSRC, "scene_build.cpp"), os.path.join(_CSRC, "scene_host.cpp")]
EMU_DEPS = EMU_SRCS + [os.path.join(_HERE, "emul", "emul.cpp"), os.path.join(_ROOT, "include", "xrt.h")] + \
    [os.path.join(_CSRC, h) for h in ("traverse.h", "xrt_core.h", "scene_host.h", "scene_build.h", "pose.h")]
EMUL_FLAGS = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]   # tests/emul_py.py's
_pkg = importlib.import_module("xna-ray-trace_amd")
abi, xna = _pkg.abi, _pkg.xna
RAY_DTYPE, HIT_DTYPE, NODE_DTYPE = _pkg.RAY_DTYPE, _pkg.HIT_DTYPE, _pkg.NODE_DTYPE
_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
_emu = None


def build():
    if not (os.path.exists(EMU_LIB) and all(os.path.getmtime(EMU_LIB) >= os.path.getmtime(d) for d in EMU_DEPS)):
        subprocess.check_call(["g++"] + EMUL_FLAGS + ["-shared", "-o", EMU_LIB] + EMU_SRCS)


def emu_lib():
    global _emu
    if _emu is None:
        build()
        l = C.CDLL(EMU_LIB)
        l.emu_create.restype = C.c_void_p
        l.emu_destroy.argtypes = [C.c_void_p]
        l.emu_error.restype = C.c_char_p
        l.emu_error.argtypes = [C.c_void_p]
        l.emu_add_mesh.argtypes = [C.c_void_p, _F, _F, _F, _F, _F, C.c_int, C.POINTER(abi.xrt_material), _F]
        l.emu_add_object.argtypes = [C.c_void_p, _I, C.c_int, _F, _F, _F, _F]
        l.emu_build.argtypes = [C.c_void_p, C.c_int, C.c_int]
        l.emu_intersect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        l.emu_set_bodies.argtypes = [C.c_void_p, C.c_int, _I, _I, _F, _F, _F, _F, C.c_int, _I]
        l.emu_set_materials.argtypes = [C.c_void_p, _I, C.c_int, C.POINTER(abi.xrt_material)]
        l.emu_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
        _emu = l
    return _emu


def _fp(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(_F)


def edited(spec, meshes=None, objects=None):
    """A copy of spec with `meshes` appended to its mesh list and `objects` as its body list."""
    s = copy.copy(spec)
    s.meshes = list(spec.meshes) + list(meshes or [])
    s.objects = list(spec.objects if objects is None else objects)
    return s


class BodyArrays:
    """The arrays xrt_scene_set_bodies takes for the bodies of a spec (kept alive by this object)."""

    def __init__(self, spec):
        n = len(spec.objects)
        self.n = n
        self.start = np.zeros(n + 1, dtype=np.int32)
        ids, w, iw, bb, wbb = [], [], [], [], []
        for b, (m, pos, rot, scale) in enumerate(spec.objects):
            self.start[b + 1] = self.start[b] + len(m)
            ids += list(m)
            a = pose_arrays(spec, b, pos, rot, scale)
            w.append(a[0]), iw.append(a[1]), wbb.append(a[2]), bb.append(body_box(spec, m))
        self.ids = np.array(ids + [0], dtype=np.int32)   # (never an empty array)
        cat = lambda parts, k: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(k), dtype=np.float32)
        self.world, self.inv, self.bbox, self.wbb = cat(w, 16), cat(iw, 16), cat(bb, 6), cat(wbb, 6)

    def args(self):
        return (self.n, self.start.ctypes.data_as(_I), self.ids.ctypes.data_as(_I), _fp(self.world), _fp(self.inv), _fp(self.bbox), _fp(self.wbb))


def _add_meshes(add_mesh, spec, first=0):
    from oracle import oracle_py as orc
    for data, m in spec.meshes[first:]:
        a, keep = orc.material_abi(m)
        assert add_mesh(_fp(data.v), _fp(data.n), _fp(data.uv), _fp(data.surface_normal), _fp(data.color), data.ntri, C.byref(a), _fp(data.bbox)) >= 0


class BodiesEmul:
    """The product's host-side scene (HostScene) of a spec, built once, then edited with HostScene::set_bodies; single-stepped on the CPU."""

    def __init__(self, spec):
        L = emu_lib()
        self.h = C.c_void_p(L.emu_create())
        self.n_meshes = len(spec.meshes)
        self.mesh_threshold = spec.mesh_threshold
        _add_meshes(lambda *a: L.emu_add_mesh(self.h, *a), spec)
        for b, (ids, pos, rot, scale) in enumerate(spec.objects):
            w, iw, wbb = pose_arrays(spec, b, pos, rot, scale)
            idarr = np.array(list(ids) + [0], dtype=np.int32)
            assert L.emu_add_object(self.h, idarr.ctypes.data_as(_I), len(ids), _fp(w), _fp(iw), _fp(body_box(spec, ids)), _fp(wbb)) >= 0
        if L.emu_build(self.h, spec.mesh_threshold, spec.scene_threshold) != 0:
            raise RuntimeError(L.emu_error(self.h).decode())

    def __del__(self):
        try:
            emu_lib().emu_destroy(self.h)
        except Exception:
            pass

    def set_bodies(self, spec):
        """The list of spec; meshes of spec this scene has not seen are added first.  Returns meshes_built."""
        L = emu_lib()
        _add_meshes(lambda *a: L.emu_add_mesh(self.h, *a), spec, self.n_meshes)
        self.n_meshes = len(spec.meshes)
        built = C.c_int32(-1)
        rc = L.emu_set_bodies(self.h, *BodyArrays(spec).args(), spec.scene_threshold, C.byref(built))
        assert rc == 0, (rc, L.emu_error(self.h))
        return built.value

    def differs_from(self, other):
        """None when both scenes hold the same bytes, else the name of the first part that differs."""
        what = C.create_string_buffer(96)
        return what.value.decode() if emu_lib().emu_compare(self.h, other.h, what, 96) else None

    def intersect(self, rays):
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        assert emu_lib().emu_intersect(self.h, 0, 0, rays.ctypes.data, rays.shape[0], hits.ctypes.data, None) == 0
        return hits


def add_meshes(xrt, handle, spec, first):
    """xrt_scene_add_mesh for meshes [first, ..) of spec on a library scene."""
    lib = xrt.abi.lib()

    def add(*a):
        mid = C.c_int32(-1)
        return -1 if lib.xrt_scene_add_mesh(handle, *a, C.byref(mid)) != 0 else mid.value
    _add_meshes(add, spec, first)


def set_bodies(xrt, handle, spec, n_known=None):
    """xrt_scene_set_bodies(handle, the bodies of spec) after adding the meshes [n_known, ..) of spec; returns (code, meshes_built)."""
    if n_known is not None:
        add_meshes(xrt, handle, spec, n_known)
    built = C.c_int32(-1)
    rc = xrt.abi.lib().xrt_scene_set_bodies(handle, *BodyArrays(spec).args(), spec.scene_threshold, C.byref(built))
    return rc, built.value


def get_tree(xrt, handle, mesh_id):
    lib = xrt.abi.lib()
    nn, nr = C.c_int64(0), C.c_int64(0)
    assert lib.xrt_scene_get_tree(handle, mesh_id, None, C.byref(nn), None, C.byref(nr)) == 0
    nodes = np.zeros(nn.value, dtype=NODE_DTYPE)
    refs = np.zeros(max(nr.value, 1), dtype=np.int32)
    assert lib.xrt_scene_get_tree(handle, mesh_id, nodes.ctypes.data_as(C.POINTER(abi.xrt_node_info)), C.byref(nn), refs.ctypes.data_as(_I), C.byref(nr)) == 0
    return nodes.tobytes(), refs[: nr.value].tobytes()


def sphere_mesh(xrt):
    z = np.load(os.path.join(xrt.fixtures._GOLDEN, "sphere_mesh.npz"))
    return xrt.fixtures.MeshData(z["v"], z["n"], z["uv"], z["color"])


def random_rays(xrt, n, seed, spread=150.0, aim=60.0):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3)) * spread
    d = rng.uniform(-aim, aim, size=(n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return xrt.rays_array(o.astype(np.float32), d.astype(np.float32))
