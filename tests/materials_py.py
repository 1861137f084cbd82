"""TEST INFRASTRUCTURE for xrt_scene_set_materials (tests/test_materials_cpu.py, tests/test_gpu_materials.py): specs with changed material
dicts -- the frame the reference renders after Material's setters ran is the oracle's frame of that spec (oracle_py.OracleScene) --,
generated textures, and the C-ABI calls on a bare scene handle."""
import copy
import ctypes as C

import numpy as np

from oracle import oracle_py as orc

abi = orc.abi
_F = C.POINTER(C.c_float)


def _fp(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(_F)


def with_materials(spec, changes):
    """A copy of spec whose mesh m has its material dict updated by changes[m] (keys of configs.material; 'texture' also sets
    'use_texture' unless the change names it)."""
    s = copy.copy(spec)
    s.meshes = []
    for i, (data, m) in enumerate(spec.meshes):
        m = dict(m)
        ch = dict(changes.get(i, {}))
        if "texture" in ch and "use_texture" not in ch:
            ch["use_texture"] = ch["texture"] is not None
        if "texture" in ch and "texture_pargb" not in ch:
            ch["texture_pargb"] = None
        if "texture" in ch:
            m.pop("texture_file", None)
        m.update(ch)
        s.meshes.append((data, m))
    return s


def gen_texture(w, h, seed, alpha=True):
    """(argb, pargb): a w x h Format32bppArgb bitmap of random colours -- with alpha, and then with the premultiplied copy the reference's
    RayTracerTexture makes of it (TEX:24-33: every channel times alpha / 255, truncated) -- as uint32 arrays of shape (h, w)."""
    rng = np.random.default_rng(seed)
    ch = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint32)   # a, r, g, b
    if not alpha:
        ch[..., 0] = 255
    argb = (ch[..., 0] << 24) | (ch[..., 1] << 16) | (ch[..., 2] << 8) | ch[..., 3]
    if not alpha:
        return np.ascontiguousarray(argb, dtype=np.uint32), None
    pm = ch[..., 1:] * ch[..., :1] // 255
    pargb = (ch[..., 0] << 24) | (pm[..., 0] << 16) | (pm[..., 1] << 8) | pm[..., 2]
    return np.ascontiguousarray(argb, dtype=np.uint32), np.ascontiguousarray(pargb, dtype=np.uint32)


def material_struct(m, texels=True):
    """xrt_material of a material dict; texels=False: NULL texels and size 0 (the library keeps the texels the mesh has).  Returns
    (struct, what must stay alive)."""
    if texels:
        return orc.material_abi(m)
    a = abi.xrt_material()
    a.reflectiveness, a.transparent, a.refraction_index = m["reflectiveness"], int(m["transparent"]), m["refraction_index"]
    a.interpolate_normals, a.use_texture = int(m["interpolate_normals"]), int(m["use_texture"])
    return a, None


def set_materials(xrt, handle, entries):
    """xrt_scene_set_materials(handle, ..): entries = [(mesh id, xrt_material)], returns the code."""
    ids = np.array([e[0] for e in entries], dtype=np.int32)
    arr = (abi.xrt_material * max(len(entries), 1))()
    for i, e in enumerate(entries):
        arr[i] = e[1]
    return xrt.abi.lib().xrt_scene_set_materials(handle, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(entries), arr)


class RawScene:
    """A host-only library scene made from a spec by the C-ABI alone; `before_build(handle)` runs between the last add and the build."""

    def __init__(self, xrt, spec, before_build=None, device=-1):
        from poses_py import body_box, pose_arrays
        lib = xrt.abi.lib()
        self.lib, self.handle = lib, C.c_void_p()
        assert lib.xrt_scene_create(device, C.byref(self.handle)) == 0
        for data, m in spec.meshes:
            a, keep = orc.material_abi(m)
            mid = C.c_int32()
            assert lib.xrt_scene_add_mesh(self.handle, _fp(data.v), _fp(data.n), _fp(data.uv), _fp(data.surface_normal), _fp(data.color), data.ntri, C.byref(a),
                                          _fp(data.bbox), C.byref(mid)) == 0
        for b, (ids, pos, rot, scale) in enumerate(spec.objects):
            w, iw, bb = pose_arrays(spec, b, pos, rot, scale)
            oid = C.c_int32()
            idarr = np.array(ids, dtype=np.int32)
            assert lib.xrt_scene_add_object(self.handle, idarr.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), _fp(w), _fp(iw), _fp(body_box(spec, ids)), _fp(bb),
                                            C.byref(oid)) == 0
        if before_build is not None:
            before_build(self.handle)
        assert lib.xrt_scene_build(self.handle, spec.mesh_threshold, spec.scene_threshold) == 0

    def saved(self, path):
        assert self.lib.xrt_scene_save(self.handle, str(path).encode()) == 0, self.lib.xrt_last_error()
        return path.read_bytes()

    def close(self):
        if self.handle:
            self.lib.xrt_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
