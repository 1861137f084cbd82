"""TEST INFRASTRUCTURE -- the checkers of xrt_scene_set_poses / xrt_scene_build_tree.

tests/poses/libposesref.so: the CPU oracle (oracle/oracle.cpp, included unmodified through tests/castray/castray_ref.cpp) with two more
entry points, orc_scene_set_pose (SceneObject World / InverseWorld / WorldBoundingBox after a move, SO:51-88, 183-199) and
orc_scene_build_tree (OctreeSpatialManager.Build alone, OSM:64-99): the reference with bodies moved between frames.
tests/poses/libemulposes.so: tests/emul (included unmodified) plus emu_set_pose / emu_build_tree, which call the product's own host-side
pose update (HostScene::set_pose / build_tree) -- the CPU single-stepper of the traversal on the records the library writes."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")
REF_LIB = os.path.join(_HERE, "poses", "libposesref.so")
EMU_LIB = os.path.join(_HERE, "poses", "libemulposes.so")
REF_SRC = os.path.join(_HERE, "poses", "poses_ref.cpp")
EMU_SRCS = [os.path.join(_HERE, "poses", "emul_poses.cpp"), os.path.join(_CSRC, "scene_build.cpp"), os.path.join(_CSRC, "scene_host.cpp")]
REF_DEPS = [REF_SRC, os.path.join(_HERE, "castray", "castray_ref.cpp"), os.path.join(_ROOT, "oracle", "oracle.cpp"),
            os.path.join(_ROOT, "oracle", "xna_math.h"), os.path.join(_ROOT, "include", "xrt.h")]
EMU_DEPS = EMU_SRCS + [os.path.join(_HERE, "emul", "emul.cpp"), os.path.join(_ROOT, "include", "xrt.h")] + \
    [os.path.join(_CSRC, h) for h in ("traverse.h", "xrt_core.h", "scene_host.h", "scene_build.h", "pose.h")]
ORACLE_FLAGS = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-associative-math", "-pthread"]   # the oracle Makefile's
EMUL_FLAGS = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]                                         # tests/emul_py.py's
_pkg = importlib.import_module("xna-ray-trace_amd")
abi, xna = _pkg.abi, _pkg.xna
RAY_DTYPE, HIT_DTYPE, NODE_DTYPE = _pkg.RAY_DTYPE, _pkg.HIT_DTYPE, _pkg.NODE_DTYPE
_F = C.POINTER(C.c_float)
_ref = None
_emu = None


def _stale(lib, deps):
    return not (os.path.exists(lib) and all(os.path.getmtime(lib) >= os.path.getmtime(d) for d in deps))


def build():
    if _stale(REF_LIB, REF_DEPS):
        subprocess.check_call(["g++"] + ORACLE_FLAGS + ["-shared", "-o", REF_LIB, REF_SRC])
    if _stale(EMU_LIB, EMU_DEPS):
        subprocess.check_call(["g++"] + EMUL_FLAGS + ["-shared", "-o", EMU_LIB] + EMU_SRCS)


def _fp(a):
    return a.ctypes.data_as(_F)


def ref_lib():
    global _ref
    if _ref is None:
        build()
        import castray_py
        from oracle import oracle_py as orc
        l = C.CDLL(REF_LIB)
        castray_py._bind_scene(l, orc)
        l.orc_cast_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_scene_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        l.orc_scene_get_tree.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64)]
        l.orc_scene_set_pose.argtypes = [C.c_void_p, C.c_int32, _F, _F, _F]
        l.orc_scene_build_tree.argtypes = [C.c_void_p, C.c_int32]
        _ref = l
    return _ref


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
        l.emu_add_object.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int, _F, _F, _F, _F]
        l.emu_build.argtypes = [C.c_void_p, C.c_int, C.c_int]
        l.emu_get_tree.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64)]
        l.emu_intersect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        l.emu_set_pose.argtypes = [C.c_void_p, C.c_int, _F, _F, _F]
        l.emu_build_tree.argtypes = [C.c_void_p, C.c_int]
        l.emu_cull_record.argtypes = [C.c_void_p, C.c_int, _F]
        _emu = l
    return _emu


def body_box(spec, ids):
    """SceneObject.BoundingBox: default(BoundingBox) merged with every mesh box (SO:131)."""
    bb = np.zeros(6, dtype=np.float32)
    for i in ids:
        bb[:3] = np.minimum(bb[:3], spec.meshes[i][0].bbox[:3])
        bb[3:] = np.maximum(bb[3:], spec.meshes[i][0].bbox[3:])
    return bb


def pose_arrays(spec, body, pos, rot, scale):
    """SceneObject.BuildWorld (SO:183-199) of body `body` of spec at (pos, rot, scale) -> (world[16], inv[16], wbb[6]) float32."""
    world, inv, wbb = xna.build_world(scale, rot, pos, body_box(spec, spec.objects[body][0]))
    return xna.as_array(world), xna.as_array(inv), xna.as_array(wbb)


def moved(spec, poses):
    """A copy of spec whose bodies stand at poses {body: (pos, rot, scale)} (what a fresh build of the moved scene is given)."""
    import copy
    s = copy.copy(spec)
    s.objects = list(spec.objects)
    for b, (pos, rot, scale) in poses.items():
        s.objects[b] = (s.objects[b][0], tuple(pos), tuple(rot), tuple(scale))
    return s


def _add_scene(add_mesh, add_object, spec):
    from oracle import oracle_py as orc
    for data, m in spec.meshes:
        a, keep = orc.material_abi(m)
        sn = np.ascontiguousarray(data.surface_normal, dtype=np.float32)
        assert add_mesh(_fp(data.v), _fp(data.n), _fp(data.uv), _fp(sn), _fp(data.color), data.ntri, C.byref(a),
                        _fp(np.ascontiguousarray(data.bbox, dtype=np.float32))) >= 0
    for b, (ids, pos, rot, scale) in enumerate(spec.objects):
        w, iw, wbb = pose_arrays(spec, b, pos, rot, scale)
        idarr = np.array(ids, dtype=np.int32)
        assert add_object(idarr.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), _fp(w), _fp(iw), _fp(body_box(spec, ids)), _fp(wbb)) >= 0


class PoseOracle:
    """The oracle scene of a spec whose bodies can be moved (orc_scene_set_pose) and filed again (orc_scene_build_tree)."""

    def __init__(self, spec):
        from oracle import oracle_py as orc
        self.orc, self.spec = orc, spec
        L = ref_lib()
        self.h = C.c_void_p(L.orc_scene_create())
        _add_scene(lambda *a: L.orc_scene_add_mesh(self.h, *a), lambda *a: L.orc_scene_add_object(self.h, *a), spec)
        if L.orc_scene_build(self.h, spec.mesh_threshold, spec.scene_threshold) != 0:
            raise RuntimeError(L.orc_last_error(self.h).decode())

    def __del__(self):
        try:
            if self.h:
                ref_lib().orc_scene_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_pose(self, body, pos, rot, scale=(1.0, 1.0, 1.0)):
        w, iw, wbb = pose_arrays(self.spec, body, pos, rot, scale)
        assert ref_lib().orc_scene_set_pose(self.h, body, _fp(w), _fp(iw), _fp(wbb)) == 0

    def set_pose_arrays(self, body, w, iw, wbb):
        assert ref_lib().orc_scene_set_pose(self.h, body, _fp(np.ascontiguousarray(w, dtype=np.float32)), _fp(np.ascontiguousarray(iw, dtype=np.float32)),
                                            _fp(np.ascontiguousarray(wbb, dtype=np.float32))) == 0

    def build_tree(self):
        assert ref_lib().orc_scene_build_tree(self.h, self.spec.scene_threshold) == 0

    def tree(self):
        nn, nr = C.c_int64(0), C.c_int64(0)
        assert ref_lib().orc_scene_get_tree(self.h, -1, None, C.byref(nn), None, C.byref(nr)) == 0
        nodes = np.zeros(nn.value, dtype=NODE_DTYPE)
        refs = np.zeros(max(nr.value, 1), dtype=np.int32)
        assert ref_lib().orc_scene_get_tree(self.h, -1, nodes.ctypes.data, C.byref(nn), refs.ctypes.data, C.byref(nr)) == 0
        return nodes, refs[: nr.value]

    def intersect(self, rays):
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        st = abi.xrt_stats()
        assert ref_lib().orc_scene_intersect(self.h, rays.ctypes.data, rays.shape[0], hits.ctypes.data, C.byref(st)) == 0
        return hits

    def _lights(self):
        lights = (abi.xrt_light * max(len(self.spec.lights), 1))()
        for i, l in enumerate(self.spec.lights):
            lights[i] = self.orc.light_abi(l)
        return lights

    def render(self, nthreads=16, camera=None, lights=None):
        """orc_render of the spec's camera -> (rgba uint32[H*W], rgb float32[H*W, 3]).  camera / lights: replacements (spec dicts)."""
        spec = self.spec
        if camera is not None or lights is not None:
            import copy
            spec = copy.copy(spec)
            spec.camera = camera or spec.camera
            spec.lights = lights or spec.lights
        cam, opts = self.orc.camera_abi(spec), self.orc.opts_abi(spec)
        ls = (abi.xrt_light * max(len(spec.lights), 1))()
        for i, l in enumerate(spec.lights):
            ls[i] = self.orc.light_abi(l)
        rgba = np.zeros(spec.width * spec.height, dtype=np.uint32)
        rgbf = np.zeros((spec.width * spec.height, 3), dtype=np.float32)
        st = abi.xrt_stats()
        rc = ref_lib().orc_render(self.h, C.byref(cam), ls, len(spec.lights), C.byref(opts), rgba.ctypes.data, rgbf.ctypes.data, C.byref(st),
                                  int(nthreads), 0, spec.height)
        if rc != 0:
            raise RuntimeError("oracle render failed: %d" % rc)
        return rgba, rgbf

    def cast_rays(self, rays, iteration=0, ref_index=1.0):
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        opts = self.orc.opts_abi(self.spec)
        n = rays.shape[0]
        rgba = np.zeros(n, dtype=np.uint32)
        rgbf = np.zeros((n, 3), dtype=np.float32)
        st = abi.xrt_stats()
        rc = ref_lib().orc_cast_rays(self.h, self._lights(), len(self.spec.lights), C.byref(opts), rays.ctypes.data, n, int(iteration),
                                     float(ref_index), rgba.ctypes.data, rgbf.ctypes.data, C.byref(st))
        assert rc == 0, rc
        return rgba, rgbf


class PoseEmul:
    """The product's host-side scene (HostScene) of a spec, single-stepped on the CPU, with HostScene::set_pose / build_tree."""

    def __init__(self, spec):
        L = emu_lib()
        self.spec = spec
        self.h = C.c_void_p(L.emu_create())
        _add_scene(lambda *a: L.emu_add_mesh(self.h, *a), lambda *a: L.emu_add_object(self.h, *a), spec)
        if L.emu_build(self.h, spec.mesh_threshold, spec.scene_threshold) != 0:
            raise RuntimeError(L.emu_error(self.h).decode())

    def __del__(self):
        try:
            emu_lib().emu_destroy(self.h)
        except Exception:
            pass

    def set_pose(self, body, pos, rot, scale=(1.0, 1.0, 1.0)):
        w, iw, wbb = pose_arrays(self.spec, body, pos, rot, scale)
        assert emu_lib().emu_set_pose(self.h, body, _fp(w), _fp(iw), _fp(wbb)) == 0

    def set_pose_arrays(self, body, w, iw, wbb):
        assert emu_lib().emu_set_pose(self.h, body, _fp(np.ascontiguousarray(w, dtype=np.float32)), _fp(np.ascontiguousarray(iw, dtype=np.float32)),
                                      _fp(np.ascontiguousarray(wbb, dtype=np.float32))) == 0

    def build_tree(self):
        assert emu_lib().emu_build_tree(self.h, self.spec.scene_threshold) == 0, emu_lib().emu_error(self.h)

    def cull_record(self, body):
        out = np.zeros(10, dtype=np.float32)
        emu_lib().emu_cull_record(self.h, body, _fp(out))
        return out

    def tree(self):
        nn, nr = C.c_int64(0), C.c_int64(0)
        emu_lib().emu_get_tree(self.h, -1, None, C.byref(nn), None, C.byref(nr))
        nodes = np.zeros(nn.value, dtype=NODE_DTYPE)
        refs = np.zeros(max(nr.value, 1), dtype=np.int32)
        emu_lib().emu_get_tree(self.h, -1, nodes.ctypes.data, C.byref(nn), refs.ctypes.data, C.byref(nr))
        return nodes, refs[: nr.value]

    def intersect(self, rays):
        """Scene queries (mode 0), one lane at a time."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        assert emu_lib().emu_intersect(self.h, 0, 0, rays.ctypes.data, rays.shape[0], hits.ctypes.data, None) == 0
        return hits


HIT_FIELDS = ("hit", "object", "mesh", "tri", "leaf", "u", "v", "d", "w")


def hits_equal(a, b):
    """Bit-identical answers (hit, object, mesh, tri, leaf, u, v, d, w): None, or a message naming the first ray that differs."""
    for k in HIT_FIELDS:
        x, y = a[k], b[k]
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        bad = np.nonzero((x != y).reshape(len(a), -1).any(axis=1))[0]
        if len(bad):
            i = int(bad[0])
            return "%d rays differ in %s (first: ray %d, %r vs %r)" % (len(bad), k, i, a[i], b[i])
    return None
