"""TEST INFRASTRUCTURE -- the checkers of xrt_scene_set_mesh_triangles (tests/test_mesh_edit_cpu.py, tests/test_gpu_mesh_edit.py).

tests/mesh_edit/libemulmeshedit.so: tests/bodies/emul_bodies.cpp (tests/emul included unmodified, emu_set_bodies, emu_compare) plus
emu_set_mesh_triangles, which calls the product's own host-side edit (HostScene::set_mesh_triangles), the counter of mesh octrees built and
the host-side pose / shading edits a replay needs.  csrc/hostcheck_mesh_edit_plain: the stand-alone program of the sanitizer check
(tests/mesh_edit/host_mesh_edit.cpp), built without a sanitizer against libxrt.so (the sanitizer build: `make -C csrc hostcheck_mesh_edit`).

The call does not touch the bodies' BoundingBox / WorldBoundingBox (the reference computes them once, SO:126-132), and every helper of this
suite (the oracle included) derives a spec's body boxes from its mesh boxes.  So a replacement is described by a spec whose BODY boxes are
those of the original: `fitted` scales a mesh into a given box and gives it a Mesh.MeshBoundingBox of the test's choice -- the old mesh's
box, or a smaller box with the same hull together with the origin (SO:131 merges the mesh boxes into default(BoundingBox)), which changes
the pre-cull records and nothing of the bodies."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np

import bodies_py
from bodies_py import BodiesEmul, EMUL_FLAGS, _CSRC, _HERE, _ROOT, _fp, _F, _I, abi
from poses_py import pose_arrays

EMU_LIB = os.path.join(_HERE, "mesh_edit", "libemulmeshedit.so")
EMU_SRCS = [os.path.join(_HERE, "mesh_edit", "emul_mesh_edit.cpp"), os.path.join(_CSRC, "scene_build.cpp"), os.path.join(_CSRC, "scene_host.cpp")]
EMU_DEPS = EMU_SRCS + [os.path.join(_HERE, "bodies", "emul_bodies.cpp"), os.path.join(_HERE, "emul", "emul.cpp"), os.path.join(_ROOT, "include", "xrt.h")] + \
    [os.path.join(_CSRC, h) for h in ("traverse.h", "xrt_core.h", "scene_host.h", "scene_build.h", "pose.h")]
HOST_PLAIN = os.path.join(_CSRC, "hostcheck_mesh_edit_plain")
HOST_SANITIZED = os.path.join(_CSRC, "hostcheck_mesh_edit")
_emu = None


def _stale(out, deps):
    return not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps))


def build():
    if _stale(EMU_LIB, EMU_DEPS):
        subprocess.check_call(["g++"] + EMUL_FLAGS + ["-shared", "-o", EMU_LIB] + EMU_SRCS)
    subprocess.check_call(["make", "-s", "-C", _CSRC, "hostcheck_mesh_edit_plain"])   # (the stand-alone program of the sanitizer check, without a sanitizer)


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
        l.emu_get_tree.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64)]
        l.emu_set_materials.argtypes = [C.c_void_p, _I, C.c_int, C.POINTER(abi.xrt_material)]
        l.emu_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
        l.emu_set_mesh_triangles.argtypes = [C.c_void_p, C.c_int, _F, _F, _F, _F, _F, C.c_int, _F]
        l.emu_mesh_trees_built.argtypes = [C.c_void_p]
        l.emu_arrays_bytes.argtypes = [C.c_void_p]
        l.emu_arrays_bytes.restype = C.c_longlong
        l.emu_edit_pose.argtypes = [C.c_void_p, C.c_int, _F, _F, _F]
        l.emu_edit_triangle_shading.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _F, _F, _F]
        _emu = l
    return _emu


def fitted(xrt, data, box, bbox=None, shift=(0.0, 0.0, 0.0)):
    """A copy of the MeshData `data` scaled (uniformly) and moved into the middle of `box` (6 floats), moved on by `shift` times the room
    left, with Mesh.MeshBoundingBox `bbox` (default: box)."""
    box = np.asarray(box, dtype=np.float64)
    v = data.v.astype(np.float64)
    if data.ntri:
        lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
        ext = np.where(hi - lo > 0, hi - lo, 1.0)
        f = 0.98 * float(((box[3:] - box[:3]) / ext).min())
        room = (box[3:] - box[:3]) - f * (hi - lo)
        v = (v - 0.5 * (lo + hi)) * f + 0.5 * (box[:3] + box[3:]) + 0.45 * room * np.asarray(shift)
    out = xrt.fixtures.MeshData(v, data.n, data.uv, data.color)
    out.bbox = np.asarray(box if bbox is None else bbox, dtype=np.float32)
    return out


def moved_vertices(xrt, data, seed, amount=0.02):
    """`data` with every vertex moved by up to `amount` of the mesh's extent (the same triangle count, another octree), inside the same
    Mesh.MeshBoundingBox."""
    rng = np.random.default_rng(seed)
    ext = float((data.bbox[3:] - data.bbox[:3]).max())
    v = data.v.astype(np.float64) + rng.uniform(-amount * ext, amount * ext, size=data.v.shape)
    v = np.clip(v, data.bbox[:3].astype(np.float64), data.bbox[3:].astype(np.float64))
    out = xrt.fixtures.MeshData(v, data.n, data.uv, data.color)
    out.bbox = data.bbox.copy()
    return out


def empty_mesh(xrt, bbox):
    out = xrt.fixtures.MeshData(np.zeros((0, 3, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3, 2)), np.zeros((0, 4)))
    out.surface_normal = np.zeros((0, 3), dtype=np.float32)
    out.bbox = np.asarray(bbox, dtype=np.float32)
    return out


def replaced(spec, k, data):
    """A copy of spec with `data` as the triangles of mesh k (its material stays)."""
    s = copy.copy(spec)
    s.meshes = list(spec.meshes)
    s.meshes[k] = (data, spec.meshes[k][1])
    s.objects = list(spec.objects)
    return s


class TriArgs:
    """The arrays xrt_scene_set_mesh_triangles takes for a MeshData (kept alive by this object); a mesh without triangles gets arrays of one record."""

    def __init__(self, data):
        e = data.ntri == 0
        arr = lambda a, k: np.zeros(k, dtype=np.float32) if e else np.ascontiguousarray(a, dtype=np.float32)
        self.v, self.n, self.uv, self.sn, self.color = arr(data.v, 9), arr(data.n, 9), arr(data.uv, 6), arr(data.surface_normal, 3), arr(data.color, 4)
        self.bbox = np.ascontiguousarray(data.bbox, dtype=np.float32)
        self.ntri = int(data.ntri)

    def args(self):
        return (_fp(self.v), _fp(self.n), _fp(self.uv), _fp(self.sn), _fp(self.color), self.ntri, _fp(self.bbox))


class MeshEditEmul(BodiesEmul):
    """The product's host-side scene (HostScene) of a spec, built once, then edited with HostScene::set_mesh_triangles; single-stepped on the CPU."""

    def __init__(self, spec):
        self.spec = spec
        L = emu_lib()
        self.h = C.c_void_p(L.emu_create())
        self.n_meshes = len(spec.meshes)
        bodies_py._add_meshes(lambda *a: L.emu_add_mesh(self.h, *a), spec)
        for b, (ids, pos, rot, scale) in enumerate(spec.objects):
            w, iw, wbb = pose_arrays(spec, b, pos, rot, scale)
            idarr = np.array(list(ids) + [0], dtype=np.int32)
            assert L.emu_add_object(self.h, idarr.ctypes.data_as(_I), len(ids), _fp(w), _fp(iw), _fp(bodies_py.body_box(spec, ids)), _fp(wbb)) >= 0
        if L.emu_build(self.h, spec.mesh_threshold, spec.scene_threshold) != 0:
            raise RuntimeError(L.emu_error(self.h).decode())

    def __del__(self):
        try:
            emu_lib().emu_destroy(self.h)
        except Exception:
            pass

    def set_mesh_triangles(self, k, data):
        return emu_lib().emu_set_mesh_triangles(self.h, int(k), *TriArgs(data).args())

    def error(self):
        return emu_lib().emu_error(self.h).decode()

    def trees_built(self):
        return int(emu_lib().emu_mesh_trees_built(self.h))

    def bytes(self):
        return int(emu_lib().emu_arrays_bytes(self.h))

    def differs_from(self, other):
        what = C.create_string_buffer(96)
        return what.value.decode() if emu_lib().emu_compare(self.h, other.h, what, 96) else None

    def intersect(self, rays):
        rays = np.ascontiguousarray(rays, dtype=bodies_py.RAY_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=bodies_py.HIT_DTYPE)
        assert emu_lib().emu_intersect(self.h, 0, 0, rays.ctypes.data, rays.shape[0], hits.ctypes.data, None) == 0
        return hits

    def set_pose(self, spec, body, pos, rot, scale):
        w, iw, wbb = pose_arrays(spec, body, pos, rot, scale)
        assert emu_lib().emu_edit_pose(self.h, body, _fp(w), _fp(iw), _fp(wbb)) == 0

    def set_material(self, mesh, struct):
        ids = np.array([mesh], dtype=np.int32)
        assert emu_lib().emu_set_materials(self.h, ids.ctypes.data_as(_I), 1, C.byref(struct)) == 0

    def set_triangle_shading(self, mesh, first, normals, uv, color):
        n = len(color)
        f = lambda a: _fp(np.ascontiguousarray(a, dtype=np.float32))
        assert emu_lib().emu_edit_triangle_shading(self.h, mesh, first, n, f(normals), f(uv), f(color)) == 0

    def leaf_sizes(self, mesh):
        nn, nr = C.c_int64(0), C.c_int64(0)
        emu_lib().emu_get_tree(self.h, mesh, None, C.byref(nn), None, C.byref(nr))
        nodes = np.zeros(nn.value, dtype=bodies_py.NODE_DTYPE)
        refs = np.zeros(max(nr.value, 1), dtype=np.int32)
        emu_lib().emu_get_tree(self.h, mesh, nodes.ctypes.data, C.byref(nn), refs.ctypes.data, C.byref(nr))
        return nodes["count"][nodes["is_leaf"] != 0]


def set_mesh_triangles(xrt, handle, k, data):
    """xrt_scene_set_mesh_triangles(handle, mesh k, the triangles and box of data); returns the code."""
    return xrt.abi.lib().xrt_scene_set_mesh_triangles(handle, int(k), *TriArgs(data).args())


def shading_values(data, first, n, seed):
    """Normals, UVs and colours for triangles [first, first + n) of a mesh, and the MeshData that holds them."""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3, 3)).astype(np.float32)
    uv = rng.uniform(0, 1, size=(n, 3, 2)).astype(np.float32)
    col = rng.uniform(0.2, 1, size=(n, 4)).astype(np.float32)
    out = copy.copy(data)
    out.n, out.uv, out.color = data.n.copy(), data.uv.copy(), data.color.copy()
    out.n[first:first + n], out.uv[first:first + n], out.color[first:first + n] = nrm, uv, col
    return nrm, uv, col, out
