"""TEST INFRASTRUCTURE for xrt_scene_set_triangle_shading (tests/test_triangles_cpu.py, tests/test_gpu_triangles.py): specs with edited
MeshData -- the frame the reference renders after a host wrote Triangle.n1..n3 / uv1..uv3 / color is the oracle's frame of that spec
(oracle_py.OracleScene) -- and the C-ABI call on a bare scene handle."""
import copy
import ctypes as C

import numpy as np

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


def with_triangle_shading(spec, edits):
    """A copy of spec in which mesh m has, for every entry i of edits[m] = dict(ids=.., normals=.., uv=.., color=..), the given values in
    its MeshData (ids: a `range` with step 1 or a list of triangle ids, entries applied in order; a missing or None field stays).  The
    vertices, surface normals and boxes are shared with spec: nothing may derive from the edited fields."""
    s = copy.copy(spec)
    s.meshes = []
    for m, (data, mat) in enumerate(spec.meshes):
        e = edits.get(m)
        if e is not None:
            ids = np.asarray(list(e["ids"]), dtype=np.int64)
            data = copy.copy(data)
            for field, shape in (("n", (-1, 3, 3)), ("uv", (-1, 3, 2)), ("color", (-1, 4))):
                vals = e.get({"n": "normals"}.get(field, field))
                if vals is None:
                    continue
                arr = getattr(data, field).copy()
                vals = np.asarray(vals, dtype=np.float32).reshape(shape)
                for i, t in enumerate(ids):   # (one by one: of a triangle listed twice the last entry counts)
                    arr[t] = vals[i]
                setattr(data, field, arr)
        s.meshes.append((data, mat))
    return s


def set_triangle_shading(xrt, handle, mesh, ids, normals=None, uv=None, color=None, first=None):
    """xrt_scene_set_triangle_shading(handle, ..) as the C-ABI takes it; ids: a `range` with step 1 (NULL tri_ids, first_tri = its start)
    or a list (first_tri 0 unless `first` overrides it).  Returns the code."""
    def fp(a):
        return None if a is None else np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(_F)
    if isinstance(ids, range):
        arr, start, n = None, ids.start, len(ids)
    else:
        arr, start = np.ascontiguousarray(ids, dtype=np.int32), 0
        n = arr.shape[0]
    if first is not None:
        start = first
    keep = [fp(normals), fp(uv), fp(color)]
    return xrt.abi.lib().xrt_scene_set_triangle_shading(handle, int(mesh), None if arr is None else arr.ctypes.data_as(_I), int(start), int(n), *keep)


def apply_edits(xrt, handle, edits):
    for m, e in edits.items():
        rc = set_triangle_shading(xrt, handle, m, e["ids"], e.get("normals"), e.get("uv"), e.get("color"))
        assert rc == 0, xrt.abi.lib().xrt_last_error()


def push(scene, edits, device=False):
    """The edits of with_triangle_shading through the mirror (OctreeSpatialManager.SetTriangleShading[Device])."""
    for m, e in edits.items():
        ids = e["ids"]
        if not device:
            scene.SetTriangleShading(m, ids if isinstance(ids, range) else list(ids), e.get("normals"), e.get("uv"), e.get("color"))
            continue
        import torch

        def t(a, dt=torch.float32):
            return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda").contiguous()
        scene.SetTriangleShadingDevice(m, ids if isinstance(ids, range) else t(list(ids), torch.int32), t(e.get("normals")), t(e.get("uv")), t(e.get("color")))
