"""Host-side mirror of the reference's API surface for the hot path, forwarding to libxrt through the
C-ABI (include/xrt.h).  Same names, argument meaning and error behaviour as the C# classes:

    Material (RayTracerTypeLibrary/Material.cs:25), Mesh (Mesh.cs:9), MeshOctree (MeshOctree.cs:9),
    SceneObject (RayTraceProject/SceneObject.cs:12), ISpatialManager / OctreeSpatialManager
    (Spatial/ISpatialManager.cs:10, OctreeSpatialManager.cs:35), Camera (Camera.cs), SpotLight,
    DirectionalLight (SpotLight.cs:10, DirectionalLight.cs:10), RayTracer (RayTracer.cs:13).

The real host is C#; its P/Invoke shim is in csharp/ and INTEGRATION.md.  This mirror exists because the
image has no .NET toolchain; it contains no arithmetic of the path itself — all of that runs in HIP.
"""
import ctypes as C
import threading
import numpy as np

from . import _abi as abi
from . import xna

f32 = np.float32


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _material_property(name, convert, texels=False):
    """A reference property of Material with a public setter (MAT:39, 234-268): setting it bumps the serial the spatial manager compares
    (and, for the texel arrays, the serial that says the library's texels are behind)."""
    attr = "_" + name

    def get(self):
        return getattr(self, attr)

    def set_(self, value):
        setattr(self, attr, convert(value))
        self._serial = getattr(self, "_serial", 0) + 1
        if texels:
            self._tex_serial = getattr(self, "_tex_serial", 0) + 1
    return property(get, set_)


def _texel_array(value):
    return None if value is None else np.ascontiguousarray(value, dtype=np.uint32)


class Material:
    """Material.cs:25-269 (shading inputs; texels as the Format32bppArgb lock of MAT:65).  Reflectiveness, Transparent, RefractionIndex,
    InterpolateNormals, UseTexture and Texture / TexturePArgb may be set after the scene is built: the OctreeSpatialManager the material's
    meshes are in hands the change to the library before its next query or frame (xrt_scene_set_materials)."""
    Reflectiveness = _material_property("Reflectiveness", float)
    UseTexture = _material_property("UseTexture", bool)
    Transparent = _material_property("Transparent", bool)
    RefractionIndex = _material_property("RefractionIndex", float)
    InterpolateNormals = _material_property("InterpolateNormals", bool)
    Texture = _material_property("Texture", _texel_array, texels=True)
    TexturePArgb = _material_property("TexturePArgb", _texel_array, texels=True)

    def __init__(self, reflectiveness=0.0, useTexture=False, transparent=False, refractionIndex=0.0, texture=None, texture_pargb=None, textureFilePath=None):
        self.Reflectiveness = float(reflectiveness)
        self.UseTexture = bool(useTexture)
        self.Transparent = bool(transparent)
        self.RefractionIndex = float(refractionIndex)
        self.InterpolateNormals = False
        self.Texture = None if texture is None else np.ascontiguousarray(texture, dtype=np.uint32)
        # Material.Texture.ColorData: the premultiplied Format32bppPArgb copy the bilinear filter reads (TEX:24-33, MAT:186-189)
        self.TexturePArgb = None if texture_pargb is None else np.ascontiguousarray(texture_pargb, dtype=np.uint32)
        self.TextureFilePath = textureFilePath   # MAT:45-53; TracerModelProcessor.CreateMaterial passes its TextureFilePath parameter (TMP:121-131)

    def Init(self):
        """Material.Init (MAT:59-69): Bitmap.FromFile(textureFilePath) locked as Format32bppArgb.  Files without an alpha channel
        (24-bpp BMP, what the reference's content uses) need no separate premultiplied copy."""
        if self.UseTexture and self.Texture is None:
            if not self.TextureFilePath:
                raise ValueError("UseTexture without a texture file")   # Bitmap.FromFile(null) throws, MAT:63
            from . import fixtures
            self.Texture = fixtures.load_bmp_argb(self.TextureFilePath)

    def _to_abi(self):
        m = abi.xrt_material()
        m.reflectiveness = self.Reflectiveness
        m.transparent = int(self.Transparent)
        m.refraction_index = self.RefractionIndex
        m.interpolate_normals = int(self.InterpolateNormals)
        m.use_texture = int(self.UseTexture)
        if self.UseTexture:
            if self.Texture is None:
                self.Init()
            m.tex_height, m.tex_width = self.Texture.shape
            m.tex_argb = self.Texture.ctypes.data_as(C.POINTER(C.c_uint32))
            if self.TexturePArgb is not None:
                if self.TexturePArgb.shape != self.Texture.shape:
                    raise ValueError("Texture.ColorData must have the size of the bitmap")
                m.tex_pargb = self.TexturePArgb.ctypes.data_as(C.POINTER(C.c_uint32))
        return m

    def _to_abi_update(self, texels):
        """The xrt_material of an xrt_scene_set_materials entry: with the texel arrays, or with NULL texels (the library keeps the ones it has)."""
        m = abi.xrt_material()
        m.reflectiveness, m.transparent, m.refraction_index = self.Reflectiveness, int(self.Transparent), self.RefractionIndex
        m.interpolate_normals, m.use_texture = int(self.InterpolateNormals), int(self.UseTexture)
        if texels:
            if self.Texture is None:
                self.Init()   # (UseTexture without a bitmap: the file, or ValueError as Bitmap.FromFile(null), MAT:63)
            if self.Texture is not None:
                m.tex_height, m.tex_width = self.Texture.shape
                m.tex_argb = self.Texture.ctypes.data_as(C.POINTER(C.c_uint32))
                if self.TexturePArgb is not None:
                    if self.TexturePArgb.shape != self.Texture.shape:
                        raise ValueError("Texture.ColorData must have the size of the bitmap")
                    m.tex_pargb = self.TexturePArgb.ctypes.data_as(C.POINTER(C.c_uint32))
        return m


class _Scene:
    """Owner of one xrt_scene handle."""

    def __init__(self, device=0):
        self.handle = C.c_void_p()
        abi.check(abi.lib().xrt_scene_create(int(device), C.byref(self.handle)))

    def close(self):
        """xrt_scene_destroy now; returns its code (XRT_OK for a scene already closed).  The handle is given up either way."""
        rc = abi.XRT_OK
        if self.handle:
            rc = abi.lib().xrt_scene_destroy(self.handle)
            self.handle = C.c_void_p()
        return rc

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_mesh(self, mesh):
        d = mesh.data
        mat = mesh.MeshMaterial._to_abi()
        mid = C.c_int32(-1)
        sn = np.ascontiguousarray(d.surface_normal, dtype=np.float32)
        bbox = np.ascontiguousarray(mesh.MeshBoundingBox, dtype=np.float32)
        abi.check(abi.lib().xrt_scene_add_mesh(self.handle, _fp(d.v), _fp(d.n), _fp(d.uv), _fp(sn), _fp(d.color),
                                               d.ntri, C.byref(mat), _fp(bbox), C.byref(mid)))
        return mid.value


def rays_array(origins, directions, ignore_mesh=None, ignore_tri=None):
    """Pack (n,3) origins / directions into an xrt_ray array."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    n = o.shape[0]
    dt = np.dtype([("o", np.float32, 3), ("d", np.float32, 3), ("ignore_mesh", np.int32), ("ignore_tri", np.int32)])
    r = np.zeros(n, dtype=dt)
    r["o"], r["d"] = o, d
    r["ignore_mesh"] = -1 if ignore_mesh is None else ignore_mesh
    r["ignore_tri"] = -1 if ignore_tri is None else ignore_tri
    return r


RAY_DTYPE = np.dtype([("o", np.float32, 3), ("d", np.float32, 3), ("ignore_mesh", np.int32), ("ignore_tri", np.int32)])
HIT_DTYPE = np.dtype([("hit", np.int32), ("object", np.int32), ("mesh", np.int32), ("tri", np.int32), ("leaf", np.int32),
                      ("u", np.float32), ("v", np.float32), ("d", np.float32), ("w", np.float32, 3), ("reserved", np.int32)])
NODE_DTYPE = np.dtype([("bmin", np.float32, 3), ("bmax", np.float32, 3), ("is_leaf", np.int32), ("count", np.int32),
                       ("dfs_index", np.int32), ("depth", np.int32), ("first_ref", np.int32), ("reserved", np.int32)])
VERTEX_DTYPE = np.dtype([("position", np.float32, 3), ("color", np.uint32)])   # xrt_path_vertex: VertexPositionColor of RayTracer.points
assert VERTEX_DTYPE.itemsize == C.sizeof(abi.xrt_path_vertex)
SURFACE_DTYPE = np.dtype(abi.SURFACE_DTYPE)   # xrt_surface
assert SURFACE_DTYPE.itemsize == C.sizeof(abi.xrt_surface) == 64
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 48 and NODE_DTYPE.itemsize == C.sizeof(abi.xrt_node_info)


class MeshOctree:
    """MeshOctree.cs:9-355.  Bodies = the mesh's triangles; Build() builds the tree natively with the
    MO:56-96/204-236 semantics; GetRayIntersection is MO:259-326."""

    def __init__(self, mesh):
        self._mesh = mesh
        self._scene = None
        self._mesh_id = -1
        self.itemTreshold = 50   # MO:42

    @property
    def Bodies(self):
        return self._mesh.data

    def Build(self):
        self._scene = _Scene(self._mesh.device)
        self._mesh_id = self._scene.add_mesh(self._mesh)
        abi.check(abi.lib().xrt_scene_build(self._scene.handle, self.itemTreshold, 0))

    def IntersectBatch(self, rays):
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        abi.check(abi.lib().xrt_mesh_intersect(self._scene.handle, self._mesh_id,
                                               rays.ctypes.data_as(C.POINTER(abi.xrt_ray)), rays.shape[0],
                                               hits.ctypes.data_as(C.POINTER(abi.xrt_hit))))
        return hits

    def GetRayIntersection(self, ray, ignoreTriangle=None):
        """ray = (position, direction); ignoreTriangle = triangle index or None.
        Returns (found, result) with result = dict(triangle, u, v, d, objectSpacePosition) or None."""
        r = rays_array([ray[0]], [ray[1]], self._mesh_id if ignoreTriangle is not None else -1,
                       -1 if ignoreTriangle is None else int(ignoreTriangle))
        h = self.IntersectBatch(r)[0]
        if not h["hit"]:
            return False, None
        return True, dict(triangle=int(h["tri"]), u=h["u"], v=h["v"], d=h["d"], objectSpacePosition=h["w"].copy(), leaf=int(h["leaf"]))

    def tree(self):
        return _get_tree(self._scene, self._mesh_id)


def _get_tree(scene, mesh_id):
    nn, nr = C.c_int64(0), C.c_int64(0)
    abi.check(abi.lib().xrt_scene_get_tree(scene.handle, mesh_id, None, C.byref(nn), None, C.byref(nr)))
    nodes = np.zeros(nn.value, dtype=NODE_DTYPE)
    refs = np.zeros(max(nr.value, 1), dtype=np.int32)
    abi.check(abi.lib().xrt_scene_get_tree(scene.handle, mesh_id, nodes.ctypes.data_as(C.POINTER(abi.xrt_node_info)),
                                           C.byref(nn), refs.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nr)))
    return nodes, refs[: nr.value]


class Mesh:
    """Mesh.cs:9-40: Triangles[] (as arrays), MeshMaterial, MeshBoundingBox, Octree, Init(), RayIntersects().  Triangles and
    MeshBoundingBox have public setters (MESH:12-14); a host that assigns them calls Init(), as in the reference, and every built
    OctreeSpatialManager that holds the mesh hands the new triangles to the library before its next query or frame."""

    def __init__(self, triangles, material, boundingBox=None, device=0):
        self.data = triangles            # fixtures.MeshData
        self.MeshMaterial = material
        self.MeshBoundingBox = np.asarray(triangles.bbox if boundingBox is None else boundingBox, dtype=np.float32)
        self.Octree = None
        self.device = device
        self._geom_serial = 0            # counts the Init() calls that followed an assignment: what a spatial manager compares
        self._geom_assigned = False

    @property
    def Triangles(self):
        return self.data

    @Triangles.setter
    def Triangles(self, triangles):   # MESH:12
        self.data = triangles
        self._geom_assigned = True

    @property
    def MeshBoundingBox(self):
        return self._bbox

    @MeshBoundingBox.setter
    def MeshBoundingBox(self, box):   # MESH:14
        self._bbox = np.asarray(box, dtype=np.float32)
        self._geom_assigned = True

    def Init(self):   # MESH:27-32
        """A fresh MeshOctree over whatever Triangles holds.  After an assignment to Triangles or MeshBoundingBox it also marks the mesh for
        the spatial managers that hold it.  (The mirror cannot see writes INTO the arrays of a MeshData: assign Triangles again, or call
        OctreeSpatialManager.SetMeshTriangles.)"""
        if self._geom_assigned:
            self._geom_serial += 1
            self._geom_assigned = False
        self.Octree = MeshOctree(self)
        self.Octree.Build()


class SceneObject:
    """SceneObject.cs:12 — transform + shared mesh list (SO:126-127); BuildWorld is SO:183-199.  Position / Rotation / Scale mark the
    body dirty (SO:52-89): the OctreeSpatialManager it is in hands the new pose to the library before its next query or frame."""

    def __init__(self, meshes, pos=(0, 0, 0), rot=(0, 0, 0), name=None):
        self.Meshes = list(meshes)
        self._pose_serial = 0
        self.Position = tuple(pos)
        self.Rotation = tuple(rot)
        self.Scale = (1.0, 1.0, 1.0)
        self.Name = name
        bb = np.zeros(6, dtype=np.float32)   # default(BoundingBox) merged with every mesh box (SO:131)
        for m in self.Meshes:
            bb[:3] = np.minimum(bb[:3], m.MeshBoundingBox[:3])
            bb[3:] = np.maximum(bb[3:], m.MeshBoundingBox[3:])
        self.BoundingBox = bb

    @property
    def Position(self):
        return self._position

    @Position.setter
    def Position(self, value):   # SO:51-62
        self._position = tuple(value)
        self._pose_serial += 1

    @property
    def Rotation(self):
        return self._rotation

    @Rotation.setter
    def Rotation(self, value):   # SO:64-75
        self._rotation = tuple(value)
        self._pose_serial += 1

    @property
    def Scale(self):
        return self._scale

    @Scale.setter
    def Scale(self, value):   # SO:77-88
        self._scale = tuple(value)
        self._pose_serial += 1

    def _build_world(self):
        world, inv, wbb = xna.build_world(self.Scale, self.Rotation, self.Position, self.BoundingBox)
        return xna.as_array(world), xna.as_array(inv), xna.as_array(wbb)

    @property
    def World(self):
        return self._build_world()[0]

    @property
    def InverseWorld(self):
        return self._build_world()[1]

    @property
    def WorldBoundingBox(self):
        return self._build_world()[2]


class ISpatialManager:
    """Spatial/ISpatialManager.cs:10-16."""

    def Build(self):
        raise NotImplementedError

    def GetRayIntersection(self, ray, ignoreTriangle=None, ignoreObject=None):
        raise NotImplementedError


class OctreeSpatialManager(ISpatialManager):
    """OctreeSpatialManager.cs:35 — the GPU implementation of the reference's plug-in seam."""

    def __init__(self, device=0):
        self.Bodies = []
        self.itemTreshold = 20          # OSM:50
        self.meshItemTreshold = 50      # MO:42
        self.device = device
        self._scene = None
        self._mesh_ids = {}
        self.meshes = []
        self._built_key = None   # the bodies and meshes of the last Build
        self._pushed = []        # per body: the pose serial the library has
        self._pushed_mats = []   # per mesh: (its Material, the material's serial) the library has
        self._pushed_tex = []    # per mesh: (Material, texel serial) of the texels the library has, or None
        self._pushed_geom = []   # per mesh: the geometry serial (Mesh.Init calls) of the triangles the library has
        self.last_build_meshes = 0   # mesh octrees the last Build() built (xrt_scene_set_bodies' meshes_built_out; a full build: all)

    def _key(self):
        return (self.meshItemTreshold, tuple((id(b), tuple(id(m) for m in b.Meshes)) for b in self.Bodies))

    def Build(self):   # OSM:64-99 (+ Mesh.Init of every distinct mesh, SO:132)
        if self._scene is not None and self._built_key == self._key():
            # same bodies and meshes: OctreeSpatialManager.Build alone over the current poses (xrt_scene_build_tree)
            self._push_poses()
            self._push_meshes()
            self._push_materials()
            abi.check(abi.lib().xrt_scene_build_tree(self._scene.handle, self.itemTreshold))
            return
        if self._scene is not None and self._built_key is not None and self._built_key[0] == self.meshItemTreshold:
            # a scene of this manager's own Build, the mesh threshold unchanged: the list alone changes (xrt_scene_set_bodies).  Meshes the
            # library has keep their ids and their octrees; only those it has not seen are added (and built by the call).
            self._push_meshes()
            self._push_materials()
            for body in self.Bodies:
                for m in body.Meshes:
                    if id(m) not in self._mesh_ids:
                        self._mesh_ids[id(m)] = self._scene.add_mesh(m)
                        self.meshes.append(m)
                        self._pushed_mats.append((m.MeshMaterial, m.MeshMaterial._serial))
                        self._pushed_tex.append((m.MeshMaterial, m.MeshMaterial._tex_serial) if m.MeshMaterial.UseTexture else None)
                        self._pushed_geom.append(m._geom_serial)
            poses = [b._build_world() for b in self.Bodies]
            self.last_build_meshes = self.SetBodies([[self._mesh_ids[id(m)] for m in b.Meshes] for b in self.Bodies],
                                                    [p[0] for p in poses], [p[1] for p in poses], [b.BoundingBox for b in self.Bodies],
                                                    [p[2] for p in poses], self.itemTreshold)
            self._built_key = self._key()
            self._pushed = [b._pose_serial for b in self.Bodies]
            return
        self._scene = _Scene(self.device)
        self._mesh_ids = {}
        self.meshes = []
        for body in self.Bodies:
            for m in body.Meshes:
                if id(m) not in self._mesh_ids:
                    self._mesh_ids[id(m)] = self._scene.add_mesh(m)
                    self.meshes.append(m)
        for body in self.Bodies:
            ids = np.array([self._mesh_ids[id(m)] for m in body.Meshes], dtype=np.int32)
            world, inv, wbb = body._build_world()
            bb = np.ascontiguousarray(body.BoundingBox, dtype=np.float32)
            oid = C.c_int32(-1)
            abi.check(abi.lib().xrt_scene_add_object(self._scene.handle, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids),
                                                     _fp(world), _fp(inv), _fp(bb), _fp(wbb), C.byref(oid)))
        abi.check(abi.lib().xrt_scene_build(self._scene.handle, self.meshItemTreshold, self.itemTreshold))
        self.last_build_meshes = len(self.meshes)
        self._built_key = self._key()
        self._pushed = [b._pose_serial for b in self.Bodies]
        self._pushed_mats = [(m.MeshMaterial, m.MeshMaterial._serial) for m in self.meshes]
        self._pushed_tex = [(m.MeshMaterial, m.MeshMaterial._tex_serial) if m.MeshMaterial.UseTexture else None for m in self.meshes]
        self._pushed_geom = [m._geom_serial for m in self.meshes]

    def SetBodies(self, body_meshes, world, inv, bbox, wbb, scene_threshold=0):
        """xrt_scene_set_bodies: the body list becomes len(body_meshes) bodies; body i has the mesh ids body_meshes[i] and world[i] (16
        floats), inv[i] (16), bbox[i] (6), wbb[i] (6).  The scene octree is built over the new list; meshes added since the last build get
        their octrees.  Returns the number of mesh octrees the call built (last_build_meshes holds it also when the call raises)."""
        n = len(body_meshes)
        start = np.zeros(n + 1, dtype=np.int32)
        start[1:] = np.cumsum([len(m) for m in body_meshes], dtype=np.int64)
        ids = np.ascontiguousarray([i for m in body_meshes for i in m] or [0], dtype=np.int32)
        w = np.ascontiguousarray(world, dtype=np.float32).reshape(-1)
        iw = np.ascontiguousarray(inv, dtype=np.float32).reshape(-1)
        bb = np.ascontiguousarray(bbox, dtype=np.float32).reshape(-1)
        wb = np.ascontiguousarray(wbb, dtype=np.float32).reshape(-1)
        if w.size != 16 * n or iw.size != 16 * n or bb.size != 6 * n or wb.size != 6 * n:
            raise ValueError("SetBodies: 16 + 16 + 6 + 6 floats per body")
        built = C.c_int32(0)
        rc = abi.lib().xrt_scene_set_bodies(self.handle, n, start.ctypes.data_as(C.POINTER(C.c_int32)), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                            _fp(w), _fp(iw), _fp(bb), _fp(wb), int(scene_threshold), C.byref(built))
        self.last_build_meshes = built.value   # (this call's own count, also when the scene octree could not be built: those octrees stay built)
        abi.check(rc)
        return built.value

    def _push_poses(self):
        """The poses of the bodies moved since the last push, in one xrt_scene_set_poses (before every query and frame)."""
        if self._scene is None or self._built_key is None:
            return
        moved = [i for i, b in enumerate(self.Bodies) if b._pose_serial != self._pushed[i]]
        if moved:
            self.SetPoses(moved, *zip(*(self.Bodies[i]._build_world() for i in moved)))
            for i in moved:
                self._pushed[i] = self.Bodies[i]._pose_serial

    def SetPoses(self, ids, world, inv, wbb):
        """xrt_scene_set_poses: body ids[i] takes world[i] (16 floats), inv[i] (16) and wbb[i] (6); the scene octree stays as built."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        w = np.ascontiguousarray(world, dtype=np.float32).reshape(-1)
        iw = np.ascontiguousarray(inv, dtype=np.float32).reshape(-1)
        bb = np.ascontiguousarray(wbb, dtype=np.float32).reshape(-1)
        n = ids.shape[0]
        if w.size != 16 * n or iw.size != 16 * n or bb.size != 6 * n:
            raise ValueError("SetPoses: 16 + 16 + 6 floats per id")
        abi.check(abi.lib().xrt_scene_set_poses(self.handle, ids.ctypes.data_as(C.POINTER(C.c_int32)), n, _fp(w), _fp(iw), _fp(bb)))

    def _push_meshes(self):
        """The meshes whose Init() ran since the last push (Mesh.Triangles / MeshBoundingBox assigned, MESH:12-14, 27-32), each in one
        xrt_scene_set_mesh_triangles (before every query, frame, Save and Build).  A mesh shared by several managers reaches each."""
        if self._scene is None or self._built_key is None:
            return
        for i, mesh in enumerate(self.meshes):
            if self._pushed_geom[i] != mesh._geom_serial:
                self.SetMeshTriangles(i, mesh.data, mesh.MeshBoundingBox)

    def SetMeshTriangles(self, mesh_or_id, triangles, boundingBox=None):
        """xrt_scene_set_mesh_triangles: the mesh (a Mesh of this manager or a mesh id) takes the triangles of `triangles` (a MeshData) and
        boundingBox (default: the triangles' own box) under its id and with its material.  Its octree alone is built; the body list, the
        bodies' boxes and the scene octree stay.  The mirror's Mesh follows, so that a later from-scratch Build() and Save() agree."""
        mid = mesh_or_id if isinstance(mesh_or_id, (int, np.integer)) else self.mesh_id(mesh_or_id)
        d = triangles
        bbox = np.ascontiguousarray(d.bbox if boundingBox is None else boundingBox, dtype=np.float32)
        arr = lambda a, k: np.ascontiguousarray(a, dtype=np.float32) if d.ntri else np.zeros(k, dtype=np.float32)   # (an empty array has no address)
        abi.check(abi.lib().xrt_scene_set_mesh_triangles(self.handle, int(mid), _fp(arr(d.v, 9)), _fp(arr(d.n, 9)), _fp(arr(d.uv, 6)),
                                                         _fp(arr(d.surface_normal, 3)), _fp(arr(d.color, 4)), int(d.ntri), _fp(bbox)))
        if 0 <= mid < len(self.meshes):   # (else a loaded scene: its geometry lives in the library alone)
            mesh = self.meshes[mid]
            if mesh.data is not d:   # a direct call: the other managers that hold the mesh see an Init()
                mesh.data = d
                mesh._geom_serial += 1
            mesh._bbox = bbox
            self._pushed_geom[mid] = mesh._geom_serial

    def _push_materials(self):
        """The materials changed since the last push -- a property set, or another Material assigned to Mesh.MeshMaterial -- in one
        xrt_scene_set_materials (before every query, frame, Save and Build).  A Material shared by several meshes goes to each of them
        (TMP:121-131).  Texels travel only when the library's are behind."""
        if self._scene is None or self._built_key is None:
            return
        ids, mats, done = [], [], []
        for i, mesh in enumerate(self.meshes):
            mat = mesh.MeshMaterial
            had, serial = self._pushed_mats[i]
            if had is mat and serial == mat._serial:
                continue
            tex = self._pushed_tex[i]
            need_tex = (mat.UseTexture or mat.Texture is not None) and not (tex is not None and tex[0] is mat and tex[1] == mat._tex_serial)
            ids.append(i)
            mats.append(mat._to_abi_update(need_tex))
            done.append((i, mat, need_tex))
        if ids:
            self.SetMaterials(ids, mats)
            for i, mat, sent in done:
                self._pushed_mats[i] = (mat, mat._serial)
                if sent:
                    self._pushed_tex[i] = (mat, mat._tex_serial)

    def SetMaterials(self, mesh_ids, materials):
        """xrt_scene_set_materials: mesh mesh_ids[i] takes materials[i] -- a Material (its texels travel when it has any; without them the
        library keeps the ones the mesh has) or an abi.xrt_material as the C-ABI takes it.  Nothing is rebuilt."""
        ids = np.ascontiguousarray(mesh_ids, dtype=np.int32).reshape(-1)
        materials = list(materials)
        if len(materials) != ids.shape[0]:
            raise ValueError("SetMaterials: one material per mesh id")
        arr = (abi.xrt_material * max(len(materials), 1))()
        for i, m in enumerate(materials):   # (the Materials own the texel arrays the structs point into)
            arr[i] = m if isinstance(m, abi.xrt_material) else m._to_abi_update(m.Texture is not None)
        abi.check(abi.lib().xrt_scene_set_materials(self.handle, ids.ctypes.data_as(C.POINTER(C.c_int32)), ids.shape[0], arr))

    def SetPosesDevice(self, ids, world, inv, wbb, stream=None):
        """xrt_scene_set_poses_device on CUDA tensors (int32 ids; float32 world / inv with 16 and wbb with 6 values per id, contiguous),
        ordered after `stream` (a torch stream; default: the current one)."""
        import torch
        n = ids.numel()
        for t, k, dt in ((ids, 1, torch.int32), (world, 16, torch.float32), (inv, 16, torch.float32), (wbb, 6, torch.float32)):
            if not t.is_cuda or not t.is_contiguous() or t.dtype != dt or t.numel() != k * n:
                raise ValueError("SetPosesDevice: contiguous CUDA tensors, int32 ids and float32 poses (16 + 16 + 6 per id)")
        s = stream if stream is not None else torch.cuda.current_stream(ids.device)
        abi.check(abi.lib().xrt_scene_set_poses_device(self.handle, C.c_void_p(ids.data_ptr()), n, C.c_void_p(world.data_ptr()),
                                                       C.c_void_p(inv.data_ptr()), C.c_void_p(wbb.data_ptr()), C.c_void_p(s.cuda_stream)))

    @staticmethod
    def _tri_selection(tri_ids_or_range):
        """(ids array or None, first, n) of a `range` with step 1 (triangles first .. first + n - 1) or a list of triangle ids."""
        if isinstance(tri_ids_or_range, range):
            r = tri_ids_or_range
            if r.step != 1:
                raise ValueError("SetTriangleShading: a range of triangles has step 1")
            return None, int(r.start), len(r)
        ids = np.ascontiguousarray(tri_ids_or_range, dtype=np.int32).reshape(-1)
        return ids, 0, int(ids.shape[0])

    def _mirror_triangle_shading(self, mesh_id, ids, first, n, normals, uv, color):
        if not (0 <= mesh_id < len(self.meshes)):
            return   # (a loaded scene: its geometry lives in the library alone)
        d = self.meshes[mesh_id].data
        sel = slice(first, first + n) if ids is None else np.asarray(ids, dtype=np.int64)
        if ids is not None and np.unique(sel).size != sel.size:   # of a triangle listed twice the last entry counts
            last = {int(t): i for i, t in enumerate(sel)}
            keep = np.array(sorted(last.values()), dtype=np.int64)
            sel = sel[keep]
            normals, uv, color = (None if a is None else a[keep] for a in (normals, uv, color))
        for have, new in ((d.n, normals), (d.uv, uv), (d.color, color)):
            if new is not None:
                have[sel] = new

    def SetTriangleShading(self, mesh_id, tri_ids_or_range, normals=None, uv=None, color=None):
        """xrt_scene_set_triangle_shading: Triangle.n1..n3 / uv1..uv3 / color (TRI:17-23) of the listed triangles of mesh `mesh_id` --
        a `range` with step 1 or a list of triangle ids -- take normals[i] (3 x 3 floats), uv[i] (3 x 2) and color[i] (4); None leaves
        a field as it is.  Nothing is rebuilt; surface normals and vertices are not settable.  The mirror's MeshData.n / uv / color are
        updated too, so that a later from-scratch Build() and Save() agree.  There is NO implicit push: the mirror cannot see writes
        into the numpy arrays of a MeshData, so a host that edits them calls this with the new values."""
        ids, first, n = self._tri_selection(tri_ids_or_range)
        arrs = []
        for a, per, shape in ((normals, 9, (n, 3, 3)), (uv, 6, (n, 3, 2)), (color, 4, (n, 4))):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.size != per * n:
                    raise ValueError("SetTriangleShading: 9 / 6 / 4 floats per triangle")
                a = a.reshape(shape)
            arrs.append(a)
        abi.check(abi.lib().xrt_scene_set_triangle_shading(self.handle, int(mesh_id), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                           first, n, *(None if a is None else _fp(a) for a in arrs)))
        self._mirror_triangle_shading(int(mesh_id), ids, first, n, *arrs)

    def SetTriangleShadingDevice(self, mesh_id, tri_ids_or_range, normals=None, uv=None, color=None, stream=None):
        """xrt_scene_set_triangle_shading_device on CUDA tensors (a `range` with step 1 or an int32 tensor of DISTINCT ids; float32 normals
        / uv / color with 9 / 6 / 4 values per entry, contiguous, None to leave a field), ordered after `stream` (a torch stream; default:
        the current one).  Ids out of range are skipped.  The mirror's MeshData follows (one copy to the host)."""
        import torch
        if isinstance(tri_ids_or_range, range):
            ids, (_, first, n) = None, self._tri_selection(tri_ids_or_range)
        else:
            ids, first, n = tri_ids_or_range, 0, tri_ids_or_range.numel()
        for t, k, dt in ((ids, 1, torch.int32), (normals, 9, torch.float32), (uv, 6, torch.float32), (color, 4, torch.float32)):
            if t is not None and (not t.is_cuda or not t.is_contiguous() or t.dtype != dt or t.numel() != k * n):
                raise ValueError("SetTriangleShadingDevice: contiguous CUDA tensors, int32 ids and float32 values (9 + 6 + 4 per entry)")
        some = next((t for t in (ids, normals, uv, color) if t is not None), None)
        s = stream if stream is not None else torch.cuda.current_stream(some.device if some is not None else None)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        abi.check(abi.lib().xrt_scene_set_triangle_shading_device(self.handle, int(mesh_id), ptr(ids), first, n, ptr(normals), ptr(uv), ptr(color),
                                                                  C.c_void_p(s.cuda_stream)))
        if 0 <= mesh_id < len(self.meshes):
            hids = np.arange(first, first + n, dtype=np.int64) if ids is None else ids.detach().cpu().numpy()
            keep = (hids >= 0) & (hids < self.meshes[mesh_id].data.ntri)   # (the others are the entries the kernel skips)
            host = lambda t, shape: None if t is None else t.detach().cpu().numpy().reshape(shape)[keep]
            self._mirror_triangle_shading(int(mesh_id), hids[keep], 0, int(keep.sum()), host(normals, (n, 3, 3)), host(uv, (n, 3, 2)),
                                          host(color, (n, 4)))

    def Save(self, path):
        """xrt_scene_save: the built scene's meshes, materials, texels and bodies as one file (the reference's .xnb content)."""
        self._push_meshes()
        self._push_materials()
        abi.check(abi.lib().xrt_scene_save(self.handle, str(path).encode()))

    @classmethod
    def Load(cls, path, device=0):
        """xrt_scene_load + xrt_scene_build: a spatial manager whose geometry lives only in the library (Bodies stays empty;
        meshes are known by id).  What a game does at start-up with the file its content build wrote."""
        sm = cls(device)
        sm._scene = _Scene.__new__(_Scene)
        sm._scene.handle = C.c_void_p()
        abi.check(abi.lib().xrt_scene_load(int(device), str(path).encode(), C.byref(sm._scene.handle)))
        abi.check(abi.lib().xrt_scene_build(sm._scene.handle, sm.meshItemTreshold, sm.itemTreshold))
        return sm

    @property
    def handle(self):
        if self._scene is None:
            raise RuntimeError("scene not built")
        return self._scene.handle

    def mesh_id(self, mesh):
        return self._mesh_ids[id(mesh)]

    def SplitStats(self, reset=True):
        """xrt_split_stats: (subtrees handed over, taken, packets split, packets written by a taker) -- diagnostics of the split walks of long packets."""
        out = (C.c_uint64 * 4)()
        abi.check(abi.lib().xrt_split_stats(self.handle, out, 1 if reset else 0))
        return tuple(int(x) for x in out)

    def EndCounts(self):
        """xrt_debug_end_counts: the last finished frame's paths coloured by k_raygen, coloured by k_shade, left on k_compose's list (all zero: not engaged)."""
        out = (C.c_uint64 * 3)()
        abi.check(abi.lib().xrt_debug_end_counts(self.handle, out))
        return tuple(int(x) for x in out)

    def PacketTable(self):
        """xrt_debug_packet_table: the last finished one-chunk frame's packet table, an (entries, 2) array of (first slot, rays), and its live list, the
        path of the ray in every slot (no entries: the frame's first traversal launch took no table)."""
        counts = (C.c_uint64 * 2)()
        abi.check(abi.lib().xrt_debug_packet_table(self.handle, counts, None, 0, None, 0))
        entries = np.zeros((int(counts[0]), 2), dtype=np.uint32)
        paths = np.zeros(int(counts[1]), dtype=np.int32)
        abi.check(abi.lib().xrt_debug_packet_table(self.handle, counts, entries.ctypes.data_as(C.POINTER(C.c_uint32)), entries.shape[0],
                                                   paths.ctypes.data_as(C.POINTER(C.c_int32)), paths.shape[0]))
        return entries, paths

    def ScreenTable(self, host_eval=False):
        """xrt_debug_screen_table: the last finished one-chunk frame's table of screen boxes, an (entries, 2) array of (x0 | x1 << 16, y0 | y1 << 16) per leaf
        reference (no entries: the frame took no table); host_eval: evaluated by the host's build of the same functions instead of copied from the device."""
        count = C.c_uint64(0)
        abi.check(abi.lib().xrt_debug_screen_table(self.handle, 1 if host_eval else 0, C.byref(count), None, 0))
        entries = np.zeros((int(count.value), 2), dtype=np.uint32)
        if entries.shape[0]:
            abi.check(abi.lib().xrt_debug_screen_table(self.handle, 1 if host_eval else 0, C.byref(count), entries.ctypes.data_as(C.POINTER(C.c_uint32)), entries.shape[0]))
        return entries

    def IntersectBatch(self, rays, stats=False):
        """Batched ISpatialManager.GetRayIntersection (ISM:15): xrt_ray array -> xrt_hit array."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        st = abi.xrt_stats()
        self._push_poses()
        self._push_meshes()
        self._push_materials()
        abi.check(abi.lib().xrt_scene_intersect(self.handle, rays.ctypes.data_as(C.POINTER(abi.xrt_ray)), None, rays.shape[0],
                                                hits.ctypes.data_as(C.POINTER(abi.xrt_hit)), C.byref(st) if stats else None))
        return (hits, st.as_dict()) if stats else hits

    def GetRayIntersection(self, ray, ignoreTriangle=None, ignoreObject=None):
        """Single-ray signature of ISM:15, forwarded as a batch of one (correct, slow).
        ignoreTriangle = (mesh, triangle index) or None; ignoreObject is dead in the reference (OSM:343)."""
        im, it = (-1, -1) if ignoreTriangle is None else (self.mesh_id(ignoreTriangle[0]), int(ignoreTriangle[1]))
        h = self.IntersectBatch(rays_array([ray[0]], [ray[1]], im, it))[0]
        if not h["hit"]:
            return False, None
        return True, dict(mesh=self.meshes[h["mesh"]], triangle=int(h["tri"]), u=h["u"], v=h["v"], d=h["d"],
                          worldPosition=h["w"].copy(), object=int(h["object"]), leaf=int(h["leaf"]))

    def tree(self, mesh=None):
        return _get_tree(self._scene, -1 if mesh is None else self.mesh_id(mesh))


class Camera:
    """Camera.cs: LookAt view + perspective projection (CAM:40-54), rebuilt on every access."""

    def __init__(self, position, target, up, fieldOfView, aspectRatio, nearClippingPlane, farClippingPlane):
        self.Position, self.Target, self.Up = position, target, up
        self.FieldOfView, self.AspectRatio = fieldOfView, aspectRatio
        self.NearClippingPlane, self.FarClippingPlane = nearClippingPlane, farClippingPlane

    @property
    def View(self):
        return xna.as_array(xna.create_look_at(self.Position, self.Target, self.Up))

    @property
    def Projection(self):
        return xna.as_array(xna.create_perspective_fov(self.FieldOfView, self.AspectRatio, self.NearClippingPlane, self.FarClippingPlane))


class SpotLight:
    """SpotLight.cs:10-63."""
    IsPositionable = True

    def __init__(self):
        self.Position = (0.0, 0.0, 0.0)
        self.Direction = (0.0, -1.0, 0.0)
        self.Color = (1.0, 1.0, 1.0)
        self.DecayExponent = 1.3   # SPOT:33
        self.Intensity = 1.0       # SPOT:34
        self.SpotAngle = 0.0

    def _to_abi(self):
        l = abi.xrt_light()
        l.kind = abi.LIGHT_SPOT
        l.position[:] = self.Position
        l.direction[:] = self.Direction
        l.color[:] = self.Color
        l.intensity, l.spot_angle, l.decay_exponent = self.Intensity, self.SpotAngle, self.DecayExponent
        return l


class DirectionalLight:
    """DirectionalLight.cs:10-31."""
    IsPositionable = False

    def __init__(self):
        self.Direction = (0.0, -1.0, 0.0)
        self.Color = (1.0, 1.0, 1.0)
        self.Intensity = 1.0   # DIR:20

    def _to_abi(self):
        l = abi.xrt_light()
        l.kind = abi.LIGHT_DIRECTIONAL
        l.direction[:] = self.Direction
        l.color[:] = self.Color
        l.intensity = self.Intensity
        l.decay_exponent = 1.3
        return l


class RenderTarget:
    """Stand-in for RenderTarget2D: Width, Height and the Color[] the tracer fills (RT:29,123)."""

    def __init__(self, width, height):
        self.Width, self.Height = int(width), int(height)
        self.data = None


class RayTracer:
    """RayTracer.cs:13 — the properties of RT:19-46 and RenderAsync / Render; the body of
    RenderInternal (RT:105-120) is one call into libxrt."""

    def __init__(self):
        self.CurrentScene = None
        self.CurrentCamera = None
        self._target = None
        self.MaxReflections = 0
        self.IsBusy = False
        self.RenderCompleted = None
        self.TextureFiltering = abi.FILTER_POINT
        self.AddressMode = abi.ADDRESS_WRAP
        self.Lights = []
        self.UseMultisampling = False
        self.MultisampleQuality = 0
        self.MultisampleMode = None     # None: ADAPTIVE when UseMultisampling (the reference); or abi.MS_FIXED16
        self.renderTargetData = None
        self.last_stats = None
        self.collect_stats = False
        # RT:504: the debugging list of ray paths (VERTEX_DTYPE records, two per segment).  Off by default: CastRay / CastRays cost and return
        # what they did; with RecordPoints they append to it.  Render* clears it (RT:61) and records nothing -- the reference's frame appends every
        # pixel's segments under one lock.
        self.points = []
        self.RecordPoints = False
        self.last_ray = None            # with RecordPoints: (position, direction) as the last CastRay left its `ref Ray ray` (RT:692-694)
        self.last_n_vertices = 0        # vertices the last recording call needed
        self.NumGpus = 1                # xrt_render_opts.n_gpus: one process, the frame's tiles dealt to this many devices
        self.BalanceTiles = False       # xrt_render_opts.balance_tiles (with NumGpus > 1): tiles dealt by the last frame's costs instead of round-robin

    @property
    def CurrentTarget(self):
        return self._target

    @CurrentTarget.setter
    def CurrentTarget(self, value):
        if self.IsBusy:
            raise RuntimeError("Can not change RenderTarget while RayTracer is busy.")   # RT:26-27
        self._target = value
        self.renderTargetData = np.zeros(value.Width * value.Height, dtype=np.uint32)     # RT:29

    def _scene_handle(self):
        """The current scene's handle, after the bodies moved and the materials changed since the last frame have been handed over
        (SO:52-89; MAT:39, 234-268)."""
        sc = self.CurrentScene
        if hasattr(sc, "_push_poses"):
            sc._push_poses()
        if hasattr(sc, "_push_meshes"):
            sc._push_meshes()
        if hasattr(sc, "_push_materials"):
            sc._push_materials()
        return sc.handle

    @property
    def Progress(self):   # RT:43-46
        return float(abi.lib().xrt_progress(self.CurrentScene.handle))

    def _camera_abi(self):
        cam = abi.xrt_camera()
        cam.view[:] = [float(x) for x in self.CurrentCamera.View]
        cam.proj[:] = [float(x) for x in self.CurrentCamera.Projection]
        cam.vp_x, cam.vp_y, cam.vp_width, cam.vp_height = 0, 0, self._target.Width, self._target.Height
        cam.vp_min_depth, cam.vp_max_depth = 0.0, 1.0
        return cam

    def _opts_abi(self, shard_rank=0, shard_count=1):
        o = abi.xrt_render_opts()
        o.max_reflections = int(self.MaxReflections)
        if self.UseMultisampling:
            o.use_multisampling = abi.MS_ADAPTIVE if self.MultisampleMode is None else self.MultisampleMode
        else:
            o.use_multisampling = abi.MS_OFF
        o.multisample_quality = int(self.MultisampleQuality)
        o.address_mode, o.filtering = int(self.AddressMode), int(self.TextureFiltering)
        o.shard_rank, o.shard_count = shard_rank, shard_count
        o.collect_stats = int(self.collect_stats)
        o.n_gpus = int(self.NumGpus) if shard_count <= 1 else 0
        o.balance_tiles = 1 if (self.BalanceTiles and o.n_gpus > 1) else 0
        return o

    def _lights_abi(self):
        arr = (abi.xrt_light * max(len(self.Lights), 1))()
        for i, l in enumerate(self.Lights):
            arr[i] = l._to_abi()
        return arr

    def Render(self, want_float=False):
        """Blocking RenderInternal (RT:103-126).  Returns the packed Color[] (and the float colorVector)."""
        cam, opts, lights = self._camera_abi(), self._opts_abi(), self._lights_abi()
        st = abi.xrt_stats()
        self.points.clear()   # RT:61
        rgbf = np.zeros(self._target.Width * self._target.Height * 3, dtype=np.float32) if want_float else None
        abi.check(abi.lib().xrt_render(self._scene_handle(), C.byref(cam), lights, len(self.Lights), C.byref(opts),
                                       self.renderTargetData.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       _fp(rgbf) if want_float else None, C.byref(st)))
        self.last_stats = st.as_dict()
        self._target.data = self.renderTargetData
        return (self.renderTargetData, rgbf.reshape(-1, 3)) if want_float else self.renderTargetData

    def RenderAsync(self):   # RT:59-79
        if self.IsBusy:
            raise RuntimeError("Current render operation not finished.")   # RT:62-63
        self.IsBusy = True

        def run():
            try:
                self.Render()
            finally:
                self.IsBusy = False                     # RT:433
                if self.RenderCompleted is not None:    # RT:435-436
                    self.RenderCompleted(self)

        t = threading.Thread(target=run, name="RenderDispatcherThread", daemon=True)   # RT:76-77
        t.start()
        return t

    def RenderDevice(self, d_rgba_ptr, stream=None, shard_rank=0, shard_count=1):
        """xrt_render_device: output stays in HBM (a torch tensor's data_ptr())."""
        return self.PrepareDevice(d_rgba_ptr, stream, shard_rank, shard_count)()

    def PrepareDevice(self, d_rgba_ptr, stream=None, shard_rank=0, shard_count=1):
        """Marshal camera / lights / options once (what the C# host does with its own XNA matrices) and return a
        callable that renders one frame into HBM per call and returns the xrt_stats dict."""
        cam, opts, lights = self._camera_abi(), self._opts_abi(shard_rank, shard_count), self._lights_abi()
        st = abi.xrt_stats()
        fn, handle, n = abi.lib().xrt_render_device, self.CurrentScene.handle, len(self.Lights)
        args = (handle, C.byref(cam), lights, n, C.byref(opts), C.c_void_p(d_rgba_ptr), C.c_void_p(stream or 0), C.byref(st))

        def frame():
            self._scene_handle()
            self.points.clear()   # RT:61
            abi.check(fn(*args))
            self.last_stats = st.as_dict()
            return self.last_stats
        frame.keepalive = (cam, opts, lights, st)

        # pipelined form: begin() enqueues a frame and returns its ticket, end(ticket) waits for it (two may be open)
        lib = abi.lib()
        ticket = C.c_int32(0)
        bargs = args[:-1] + (C.byref(ticket),)

        def begin():
            self._scene_handle()
            self.points.clear()   # RT:61
            abi.check(lib.xrt_render_device_begin(*bargs))
            return ticket.value

        def end(t):
            abi.check(lib.xrt_render_device_end(handle, t, C.byref(st)))
            self.last_stats = st.as_dict()
            return self.last_stats
        frame.begin, frame.end = begin, end
        return frame

    # ---- cost-aware tile assignment (xrt.h: the static counterpart of the reference's dynamic row stealing, RT:48-52) ----
    def TileCosts(self, reset=True):
        """xrt_scene_tile_costs: ticks per tile (row-major tile order) of the frames of the current target's size rendered since the last reset."""
        w, h = self._target.Width, self._target.Height
        tx, ty = (w + abi.TILE_W - 1) // abi.TILE_W, (h + abi.TILE_H - 1) // abi.TILE_H
        cost = np.zeros(tx * ty, dtype=np.float32)
        abi.check(abi.lib().xrt_scene_tile_costs(self.CurrentScene.handle, w, h, _fp(cost), 1 if reset else 0))
        return cost

    def SetTileTable(self, shard_count, tiles_per_rank, table):
        """xrt_scene_set_tile_table for frames of the current target's size (table None: back to round-robin)."""
        w, h = self._target.Width, self._target.Height
        if table is None:
            abi.check(abi.lib().xrt_scene_set_tile_table(self.CurrentScene.handle, w, h, 0, 0, None))
            return
        t = np.ascontiguousarray(table, dtype=np.int32)
        abi.check(abi.lib().xrt_scene_set_tile_table(self.CurrentScene.handle, w, h, int(shard_count), int(tiles_per_rank), t.ctypes.data_as(C.POINTER(C.c_int32))))

    def PrepareHost(self, host_array):
        """Pipelined host-output frames (xrt_render_begin / xrt_render_end): RenderAsync with the frame ending in the host's
        Color[] (RT:122-123).  `host_array`: a uint32 numpy array of W*H elements, ideally registered with
        xrt_host_register so that the device-to-host copy of frame i runs under the rendering of frame i+1."""
        cam, opts, lights = self._camera_abi(), self._opts_abi(), self._lights_abi()
        st, ticket, lib = abi.xrt_stats(), C.c_int32(0), abi.lib()
        handle, n = self.CurrentScene.handle, len(self.Lights)
        ptr = host_array.ctypes.data_as(C.POINTER(C.c_uint32))

        def begin():
            self._scene_handle()
            self.points.clear()   # RT:61
            abi.check(lib.xrt_render_begin(handle, C.byref(cam), lights, n, C.byref(opts), ptr, C.byref(ticket)))
            return ticket.value

        def end(t):
            abi.check(lib.xrt_render_end(handle, t, C.byref(st)))
            self.last_stats = st.as_dict()
            return self.last_stats
        begin.keepalive = (cam, opts, lights, st, host_array)
        begin.begin, begin.end = begin, end
        return begin

    # ---- GetColorForQuadrant / the body of Render's inner loop (RT:215-311, 412-425) on caller-chosen pixels: xrt_render_pixels ----
    def RenderPixels(self, centers, want_float=False, device=False, stream=None, coherent=False):
        """The colour of every screen position of a list, by the tracer's camera, lights and options as in Render (all three multisampling
        modes; an integer centre gets the frame's pixel bit for bit).  Host form: `centers` an (n, 2) float32 array -> uint32 colours (and
        float32 (n, 3) with want_float).  device=True: `centers` a contiguous CUDA tensor of n float32 pairs -> torch tensors on its device
        (int32 holding the packed colours; float32 (n, 3)), enqueued on `stream` (a torch stream, default: the current one).
        coherent=True (xrt_render_opts.list_order = XRT_LIST_COHERENT): consecutive centres are neighbours on screen -- a row-major rectangle,
        a frame's tile order -- and the list is traced as a frame would be.  Scheduling only: the colours and counters are the same."""
        cam, opts, lights = self._camera_abi(), self._opts_abi(shard_count=0), self._lights_abi()
        opts.n_gpus = 0
        opts.list_order = int(coherent)   # (False / True are XRT_LIST_UNORDERED / XRT_LIST_COHERENT; the library refuses any other value)
        st, lib = abi.xrt_stats(), abi.lib()
        if device:
            import torch
            if centers.dtype != torch.float32 or not centers.is_contiguous() or centers.numel() % 2:
                raise ValueError("centers: a contiguous float32 tensor of (x, y) pairs")
            n = centers.numel() // 2
            rgba = torch.empty(n, dtype=torch.int32, device=centers.device)
            rgbf = torch.empty((n, 3), dtype=torch.float32, device=centers.device) if want_float else None
            s = stream if stream is not None else torch.cuda.current_stream(centers.device)
            abi.check(lib.xrt_render_pixels_device(self._scene_handle(), C.byref(cam), lights, len(self.Lights), C.byref(opts),
                                                   C.c_void_p(centers.data_ptr()), n, C.c_void_p(rgba.data_ptr()),
                                                   C.c_void_p(rgbf.data_ptr()) if want_float else None, C.c_void_p(s.cuda_stream), C.byref(st)))
        else:
            centers = np.ascontiguousarray(centers, dtype=np.float32).reshape(-1, 2)
            n = centers.shape[0]
            rgba = np.zeros(n, dtype=np.uint32)
            rgbf = np.zeros((n, 3), dtype=np.float32) if want_float else None
            abi.check(lib.xrt_render_pixels(self._scene_handle(), C.byref(cam), lights, len(self.Lights), C.byref(opts), _fp(centers), n,
                                            rgba.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(rgbf) if want_float else None, C.byref(st)))
        self.last_stats = st.as_dict()
        return (rgba, rgbf) if want_float else rgba

    # ---- the first level of RenderPixels alone: the ray of RT:412-421 and the IntersectionResult of RT:512 per listed pixel: xrt_trace_pixels ----
    def TracePixels(self, centers, want_rays=True, want_hits=True, fixed16=False, device=False, stream=None, coherent=False):
        """The primary ray and its closest hit for every screen position of a list, by the tracer's camera; nothing is shaded and no light is
        read.  fixed16=True: the sixteen level-1 positions around every centre as RenderPixels takes them with MultisampleMode MS_FIXED16
        (record i * 16 + s is sample s of entry i); the tracer's own multisampling settings are not read.  Host form: `centers` an (n, 2)
        float32 array -> a RAY_DTYPE array and a HIT_DTYPE array (the one that is wanted alone, or both as a pair).  device=True: `centers` a
        contiguous CUDA tensor of n float32 pairs -> int32 tensors of 8 words per ray record and 12 words per hit record on its device,
        enqueued on `stream` (a torch stream, default: the current one).  want_hits=False traces nothing.  coherent=True
        (xrt_render_opts.list_order = XRT_LIST_COHERENT): consecutive centres are neighbours on screen and the list is traced as a frame's
        primary rays would be.  Scheduling only: the records and counters are the same."""
        if not want_rays and not want_hits:
            raise ValueError("TracePixels: nothing is wanted")
        cam, opts = self._camera_abi(), self._opts_abi(shard_count=0)
        opts.n_gpus = 0
        opts.use_multisampling = abi.MS_FIXED16 if fixed16 else abi.MS_OFF
        opts.list_order = int(coherent)   # (False / True are XRT_LIST_UNORDERED / XRT_LIST_COHERENT; the library refuses any other value)
        samples = 16 if fixed16 else 1
        st, lib = abi.xrt_stats(), abi.lib()
        if device:
            import torch
            if centers.dtype != torch.float32 or not centers.is_contiguous() or centers.numel() % 2:
                raise ValueError("centers: a contiguous float32 tensor of (x, y) pairs")
            n = centers.numel() // 2
            rays = torch.empty((n * samples, 8), dtype=torch.int32, device=centers.device) if want_rays else None
            hits = torch.empty((n * samples, 12), dtype=torch.int32, device=centers.device) if want_hits else None
            s = stream if stream is not None else torch.cuda.current_stream(centers.device)
            abi.check(lib.xrt_trace_pixels_device(self._scene_handle(), C.byref(cam), C.byref(opts), C.c_void_p(centers.data_ptr()), n,
                                                  C.c_void_p(rays.data_ptr()) if want_rays else None, C.c_void_p(hits.data_ptr()) if want_hits else None,
                                                  C.c_void_p(s.cuda_stream), C.byref(st)))
        else:
            centers = np.ascontiguousarray(centers, dtype=np.float32).reshape(-1, 2)
            n = centers.shape[0]
            rays = np.zeros(n * samples, dtype=RAY_DTYPE) if want_rays else None
            hits = np.zeros(n * samples, dtype=HIT_DTYPE) if want_hits else None
            abi.check(lib.xrt_trace_pixels(self._scene_handle(), C.byref(cam), C.byref(opts), _fp(centers), n,
                                           rays.ctypes.data_as(C.POINTER(abi.xrt_ray)) if want_rays else None,
                                           hits.ctypes.data_as(C.POINTER(abi.xrt_hit)) if want_hits else None, C.byref(st)))
        self.last_stats = st.as_dict()
        if want_rays and want_hits:
            return rays, hits
        return rays if want_rays else hits

    # ---- RayTracer.CastRay (RT:506-737) on caller-given rays: xrt_cast_rays, xrt_cast_rays_paths ----
    def CastRays(self, rays, iteration=0, currentRefIndex=1.0, want_float=False, device=False, stream=None, paths=False, vertex_capacity=None, coherent=False):
        """CastRay(ref rays[i], out color, iteration, origin_i, null, currentRefIndex) for every ray of a batch, origin_i = the ray's
        (ignore_mesh, ignore_tri).  Host form: `rays` an xrt_ray array (RAY_DTYPE) -> uint32 colours (and float32 (n, 3) colour vectors
        with want_float).  device=True: `rays` a contiguous CUDA tensor of n 32-byte records (e.g. (n, 8) float32) -> torch tensors on
        its device (int32 holding the packed colours; float32 (n, 3)), enqueued on `stream` (a torch stream, default: the current one).

        paths=True (xrt_cast_rays_paths): additionally returns (vertices, vertex_start, rays_back) -- the segments every call appends to
        RayTracer.points (RT:543, 701), vertices[vertex_start[i]:vertex_start[i + 1]] being ray i's, and every ray as CastRay leaves its
        `ref ray` (RT:692-694).  Host form: a VERTEX_DTYPE array (`position`, `color`), int64[n + 1], RAY_DTYPE[n]; device form: torch tensors
        (float32 (m, 4) whose last column holds the colour's bits, int64 (n + 1), float32 (n, 8)).  How the vertex array is sized: with
        vertex_capacity=None a first call counts (no vertex array) and a second call of exactly that capacity fills it -- the batch is traced
        twice; a caller who knows a bound passes vertex_capacity and gets one call, the array cut to what fitted; last_n_vertices is what
        the batch needs either way.
        With RecordPoints the segments are also appended to `points` and last_ray is the last ray's (position, direction) as left.

        coherent=True (xrt_render_opts.list_order = XRT_LIST_COHERENT): consecutive rays are neighbours in space (a frame's primary rays in
        screen order), and the batch is traced as a frame would be.  Scheduling only: every output is the same."""
        opts, lights = self._opts_abi(shard_count=0), self._lights_abi()
        opts.n_gpus = 0
        opts.list_order = int(coherent)   # (False / True are XRT_LIST_UNORDERED / XRT_LIST_COHERENT; the library refuses any other value)
        st, lib = abi.xrt_stats(), abi.lib()
        record = paths or self.RecordPoints
        need = C.c_int64(0)
        if device:
            import torch
            if not rays.is_contiguous() or rays.numel() * rays.element_size() % 32:
                raise ValueError("rays: a contiguous tensor of 32-byte xrt_ray records")
            n = rays.numel() * rays.element_size() // 32
            rgba = torch.empty(n, dtype=torch.int32, device=rays.device)
            rgbf = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if want_float else None
            s = stream if stream is not None else torch.cuda.current_stream(rays.device)
            if not record:
                abi.check(lib.xrt_cast_rays_device(self._scene_handle(), C.c_void_p(rays.data_ptr()), n, int(iteration), float(currentRefIndex),
                                                   lights, len(self.Lights), C.byref(opts), C.c_void_p(rgba.data_ptr()),
                                                   C.c_void_p(rgbf.data_ptr()) if want_float else None, C.c_void_p(s.cuda_stream), C.byref(st)))
            else:
                vstart = torch.empty(n + 1, dtype=torch.int64, device=rays.device)
                back = torch.empty((n, 8), dtype=torch.float32, device=rays.device)

                def call(verts, cap):
                    abi.check(lib.xrt_cast_rays_paths_device(self._scene_handle(), C.c_void_p(rays.data_ptr()), n, int(iteration), float(currentRefIndex),
                                                             lights, len(self.Lights), C.byref(opts), C.c_void_p(rgba.data_ptr()),
                                                             C.c_void_p(rgbf.data_ptr()) if want_float else None, C.c_void_p(back.data_ptr()),
                                                             C.c_void_p(vstart.data_ptr()), C.c_void_p(verts.data_ptr()) if cap > 0 else None, cap,
                                                             C.c_void_p(s.cuda_stream), C.byref(need), C.byref(st)))
                cap = vertex_capacity
                if cap is None:
                    call(None, 0)
                    cap = need.value
                vertices = torch.empty((max(int(cap), 1), 4), dtype=torch.float32, device=rays.device)
                call(vertices, int(cap))
                vertices = vertices[:min(need.value, int(cap) & ~1)]
        else:
            rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
            n = rays.shape[0]
            rgba = np.zeros(n, dtype=np.uint32)
            rgbf = np.zeros((n, 3), dtype=np.float32) if want_float else None
            if not record:
                abi.check(lib.xrt_cast_rays(self._scene_handle(), rays.ctypes.data_as(C.POINTER(abi.xrt_ray)), n, int(iteration), float(currentRefIndex),
                                            lights, len(self.Lights), C.byref(opts), rgba.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            _fp(rgbf) if want_float else None, C.byref(st)))
            else:
                vstart = np.zeros(n + 1, dtype=np.int64)
                back = np.zeros(n, dtype=RAY_DTYPE)

                def call(verts, cap):
                    abi.check(lib.xrt_cast_rays_paths(self._scene_handle(), rays.ctypes.data_as(C.POINTER(abi.xrt_ray)), n, int(iteration), float(currentRefIndex),
                                                      lights, len(self.Lights), C.byref(opts), rgba.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                      _fp(rgbf) if want_float else None, back.ctypes.data_as(C.POINTER(abi.xrt_ray)),
                                                      vstart.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      verts.ctypes.data_as(C.POINTER(abi.xrt_path_vertex)) if cap > 0 else None, cap, C.byref(need), C.byref(st)))
                cap = vertex_capacity
                if cap is None:
                    call(None, 0)
                    cap = need.value
                vertices = np.zeros(max(int(cap), 1), dtype=VERTEX_DTYPE)
                call(vertices, int(cap))
                vertices = vertices[:min(need.value, int(cap) & ~1)]
        self.last_stats = st.as_dict()
        if record:
            self.last_n_vertices = need.value
            if self.RecordPoints:   # RT:740-747: the public list grows call by call
                host_v = np.ascontiguousarray(vertices.cpu().numpy()).view(VERTEX_DTYPE).reshape(-1) if device else vertices
                self.points.extend(host_v)
                if n > 0:
                    b = back[n - 1].cpu().numpy() if device else np.frombuffer(back[n - 1].tobytes(), dtype=np.float32)
                    self.last_ray = (b[0:3].copy(), b[3:6].copy())
        out = (rgba, rgbf) if want_float else (rgba,)
        if paths:
            out = out + (vertices, vstart, back)
        return out if len(out) > 1 else out[0]

    # ---- what CastRay does with an IntersectionResult (RT:514-737) on caller-given hits: xrt_shade_hits ----
    def ShadeHits(self, rays, hits, iteration=0, currentRefIndex=1.0, want_float=False, device=False, stream=None):
        """CastRay(ref rays[i], out color, iteration, origin, null, currentRefIndex) for every ray of a batch with its closest-hit query
        (RT:512) replaced by "the query returned hits[i]": nothing is traced for the first level, everything below it is.  Host form:
        `rays` an xrt_ray array (RAY_DTYPE), `hits` the structured array OctreeSpatialManager.IntersectBatch returns (HIT_DTYPE) -> uint32
        colours (and float32 (n, 3) colour vectors with want_float).  device=True: `rays` a contiguous CUDA tensor of n 32-byte records
        and `hits` one of n x 12 32-bit words on the same device -> torch tensors on it (int32 holding the packed colours; float32 (n, 3)),
        enqueued on `stream` (a torch stream, default: the current one)."""
        opts, lights = self._opts_abi(shard_count=0), self._lights_abi()
        opts.n_gpus = 0
        st, lib = abi.xrt_stats(), abi.lib()
        if device:
            import torch
            if not rays.is_contiguous() or rays.numel() * rays.element_size() % 32:
                raise ValueError("rays: a contiguous tensor of 32-byte xrt_ray records")
            n = rays.numel() * rays.element_size() // 32
            if not hits.is_contiguous() or hits.element_size() != 4 or hits.numel() != 12 * n or hits.device != rays.device:
                raise ValueError("hits: a contiguous tensor of n x 12 32-bit words (xrt_hit records) on the rays' device")
            rgba = torch.empty(n, dtype=torch.int32, device=rays.device)
            rgbf = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if want_float else None
            s = stream if stream is not None else torch.cuda.current_stream(rays.device)
            abi.check(lib.xrt_shade_hits_device(self._scene_handle(), C.c_void_p(rays.data_ptr()), C.c_void_p(hits.data_ptr()), n, int(iteration),
                                                float(currentRefIndex), lights, len(self.Lights), C.byref(opts), C.c_void_p(rgba.data_ptr()),
                                                C.c_void_p(rgbf.data_ptr()) if want_float else None, C.c_void_p(s.cuda_stream), C.byref(st)))
        else:
            rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
            hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
            n = rays.shape[0]
            if hits.shape[0] != n:
                raise ValueError("hits: one xrt_hit per ray")
            rgba = np.zeros(n, dtype=np.uint32)
            rgbf = np.zeros((n, 3), dtype=np.float32) if want_float else None
            abi.check(lib.xrt_shade_hits(self._scene_handle(), rays.ctypes.data_as(C.POINTER(abi.xrt_ray)), hits.ctypes.data_as(C.POINTER(abi.xrt_hit)), n,
                                         int(iteration), float(currentRefIndex), lights, len(self.Lights), C.byref(opts),
                                         rgba.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(rgbf) if want_float else None, C.byref(st)))
        self.last_stats = st.as_dict()
        return (rgba, rgbf) if want_float else rgba

    # ---- CastRay's light loop alone (RT:534-542) on caller-given hits, in fp32: xrt_light_hits ----
    def LightHits(self, hits, want_amounts=False, want_light=True, device=False, stream=None):
        """For every hit the light sum of RT:534-542 -- GetLightForFragment * (1 - lightAmount) over self.Lights, nothing quantised -- as
        float32 (n, 3), and with want_amounts IsLightPathObstructed's amount per light (RT:465-502) as float32 (n, len(Lights)); an entry
        with hit == 0 gives zeros.  Host form: `hits` the structured array IntersectBatch returns (HIT_DTYPE).  device=True: a contiguous
        CUDA tensor of n x 12 32-bit words -> torch tensors on its device, enqueued on `stream` (a torch stream, default: the current
        one).  want_light=False returns the amounts alone."""
        if not want_light and not want_amounts:
            raise ValueError("LightHits: nothing is wanted")
        lights, nl = self._lights_abi(), len(self.Lights)
        st, lib = abi.xrt_stats(), abi.lib()
        if device:
            import torch
            if not hits.is_contiguous() or hits.element_size() != 4 or hits.numel() % 12:
                raise ValueError("hits: a contiguous tensor of n x 12 32-bit words (xrt_hit records)")
            n = hits.numel() // 12
            light = torch.empty((n, 3), dtype=torch.float32, device=hits.device) if want_light else None
            amounts = torch.empty((n, nl), dtype=torch.float32, device=hits.device) if want_amounts else None
            s = stream if stream is not None else torch.cuda.current_stream(hits.device)
            abi.check(lib.xrt_light_hits_device(self._scene_handle(), C.c_void_p(hits.data_ptr()), n, lights, nl,
                                                C.c_void_p(light.data_ptr()) if want_light else None,
                                                C.c_void_p(amounts.data_ptr()) if want_amounts else None, C.c_void_p(s.cuda_stream), C.byref(st)))
        else:
            hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
            n = hits.shape[0]
            light = np.zeros((n, 3), dtype=np.float32) if want_light else None
            amounts = np.zeros((n, nl), dtype=np.float32) if want_amounts else None
            abi.check(lib.xrt_light_hits(self._scene_handle(), hits.ctypes.data_as(C.POINTER(abi.xrt_hit)), n, lights, nl,
                                         _fp(light) if want_light else None, _fp(amounts) if want_amounts else None, C.byref(st)))
        self.last_stats = st.as_dict()
        if want_light and want_amounts:
            return light, amounts
        return light if want_light else amounts

    # ---- what CastRay computes at a hit without asking the scene anything, and the rays it casts next: xrt_surface_hits ----
    def SurfaceHits(self, hits, rays=None, currentRefIndex=1.0, want_surface=True, want_reflect=False, want_refract=False, device=False, stream=None):
        """For every hit the surface record (SURFACE_DTYPE: fragment normal RT:520-531, surface colour with its texture lookup RT:568-581,
        color.W, Reflectiveness, RefractionIndex, uv, the refraction index below the surface, flags), the reflected ray (RT:547-559) and the
        Snell refraction (RT:656-694, the record of a miss where the material is not Transparent); an entry with hit == 0 gives the zero
        record and rays of o = d = 0, ignore (-1, -1).  `rays` (the rays that produced the hits; only their directions are read) is needed
        for the ray outputs alone.  Host form: structured arrays (HIT_DTYPE, RAY_DTYPE) -> SURFACE_DTYPE / RAY_DTYPE arrays.  device=True:
        contiguous CUDA tensors of n x 12 words (hits) and n 32-byte records (rays) -> torch tensors on their device, float32 (n, 16) for
        the surface records and (n, 8) for each ray list, enqueued on `stream` (a torch stream, default: the current one).  Returns the
        outputs that are wanted, in the order (surface, reflect, refract): one alone, or a tuple."""
        if not (want_surface or want_reflect or want_refract):
            raise ValueError("SurfaceHits: nothing is wanted")
        want_rays = want_reflect or want_refract
        if want_rays and rays is None:
            raise ValueError("SurfaceHits: the ray outputs need the rays that produced the hits")
        opts = self._opts_abi()
        st, lib = abi.xrt_stats(), abi.lib()
        if device:
            import torch
            if not hits.is_contiguous() or hits.element_size() != 4 or hits.numel() % 12:
                raise ValueError("hits: a contiguous tensor of n x 12 32-bit words (xrt_hit records)")
            n = hits.numel() // 12
            if want_rays and (not rays.is_contiguous() or rays.numel() * rays.element_size() != 32 * n or rays.device != hits.device):
                raise ValueError("rays: a contiguous tensor of n 32-byte xrt_ray records on the hits' device")
            surf = torch.empty((n, 16), dtype=torch.float32, device=hits.device) if want_surface else None
            refl = torch.empty((n, 8), dtype=torch.float32, device=hits.device) if want_reflect else None
            refr = torch.empty((n, 8), dtype=torch.float32, device=hits.device) if want_refract else None
            s = stream if stream is not None else torch.cuda.current_stream(hits.device)
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            abi.check(lib.xrt_surface_hits_device(self._scene_handle(), ptr(rays) if want_rays else None, ptr(hits), n, float(currentRefIndex), C.byref(opts),
                                                  ptr(surf), ptr(refl), ptr(refr), C.c_void_p(s.cuda_stream), C.byref(st)))
        else:
            hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
            n = hits.shape[0]
            if want_rays:
                rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
                if rays.shape[0] != n:
                    raise ValueError("rays: one xrt_ray per hit")
            surf = np.zeros(n, dtype=SURFACE_DTYPE) if want_surface else None
            refl = np.zeros(n, dtype=RAY_DTYPE) if want_reflect else None
            refr = np.zeros(n, dtype=RAY_DTYPE) if want_refract else None
            rp = lambda a: a.ctypes.data_as(C.POINTER(abi.xrt_ray)) if a is not None else None
            abi.check(lib.xrt_surface_hits(self._scene_handle(), rp(rays) if want_rays else None, hits.ctypes.data_as(C.POINTER(abi.xrt_hit)), n,
                                           float(currentRefIndex), C.byref(opts), surf.ctypes.data_as(C.POINTER(abi.xrt_surface)) if want_surface else None,
                                           rp(refl), rp(refr), C.byref(st)))
        self.last_stats = st.as_dict()
        out = tuple(o for o, w in ((surf, want_surface), (refl, want_reflect), (refr, want_refract)) if w)
        return out[0] if len(out) == 1 else out

    # ---- the way back up CastRay, one level (RT:584, 699, 705, 726, 732), on caller-given terms: xrt_compose_hits ----
    def ComposeHits(self, surface, light, reflect=None, refract=None, want_float=False, device=False, stream=None):
        """For every entry the colour CastRay returns from its surface record (SurfaceHits), its light sum (LightHits) and the packed colours
        its two nested calls returned (CastRays on the reflected and the refracted rays): without `reflect` RT:726 (light * colour: the
        caller's iteration >= MaxReflections), with it RT:584, and with `refract` RT:699 on the Transparent entries; an entry without
        SURF_HIT is black (RT:732).  Host form: SURFACE_DTYPE (n), float32 (n, 3), uint32 (n) -> uint32 (n), and with want_float the vector
        handed to `new Color` as float32 (n, 3).  device=True: contiguous CUDA tensors on one device -- float32 (n, 16), float32 (n, 3),
        int32 (n) -> int32 (n) and float32 (n, 3) --, enqueued on `stream` (a torch stream, default: the current one)."""
        if refract is not None and reflect is None:
            raise ValueError("ComposeHits: refract without reflect")
        st, lib = abi.xrt_stats(), abi.lib()
        if device:
            import torch
            if surface.dtype != torch.float32 or surface.dim() != 2 or surface.shape[1] != 16 or not surface.is_contiguous() or not surface.is_cuda:
                raise ValueError("surface: a contiguous float32 CUDA tensor (n, 16) of xrt_surface records")
            n = surface.shape[0]
            if light.dtype != torch.float32 or tuple(light.shape) != (n, 3) or not light.is_contiguous() or light.device != surface.device:
                raise ValueError("light: a contiguous float32 tensor (n, 3) on the surface records' device")
            for name, t in (("reflect", reflect), ("refract", refract)):
                if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous() or t.device != surface.device):
                    raise ValueError("%s: a contiguous int32 tensor (n) of packed colours on the surface records' device" % name)
            rgba = torch.empty(n, dtype=torch.int32, device=surface.device)
            rgbf = torch.empty((n, 3), dtype=torch.float32, device=surface.device) if want_float else None
            s = stream if stream is not None else torch.cuda.current_stream(surface.device)
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            abi.check(lib.xrt_compose_hits_device(self._scene_handle(), ptr(surface), ptr(light), ptr(reflect), ptr(refract), n, ptr(rgba), ptr(rgbf),
                                                  C.c_void_p(s.cuda_stream), C.byref(st)))
        else:
            surface = np.ascontiguousarray(surface)
            if surface.dtype != SURFACE_DTYPE or surface.ndim != 1:
                raise ValueError("surface: an array of SURFACE_DTYPE records")
            n = surface.shape[0]
            light = np.ascontiguousarray(light)
            if light.dtype != np.float32 or light.shape != (n, 3):
                raise ValueError("light: float32 (n, 3)")
            cols = []
            for name, a in (("reflect", reflect), ("refract", refract)):
                if a is not None:
                    a = np.ascontiguousarray(a)
                    if a.dtype != np.uint32 or a.shape != (n,):
                        raise ValueError("%s: uint32 (n) packed colours" % name)
                cols.append(a)
            rgba = np.zeros(n, dtype=np.uint32)
            rgbf = np.zeros((n, 3), dtype=np.float32) if want_float else None
            up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)) if a is not None else None
            abi.check(lib.xrt_compose_hits(self._scene_handle(), surface.ctypes.data_as(C.POINTER(abi.xrt_surface)), _fp(light), up(cols[0]), up(cols[1]), n,
                                           up(rgba), _fp(rgbf) if want_float else None, C.byref(st)))
        self.last_stats = st.as_dict()
        return (rgba, rgbf) if want_float else rgba

    # ---- RT:309 on caller-given colours: xrt_fold_samples ----
    def FoldSamples(self, colors, samples=16, want_float=False, device=False, stream=None):
        """The mean of four packed colours, re-quantised (samples=4), or the mean of four such means (samples=16, the record order of
        TracePixels / RenderPixels with sixteen samples) of every entry: n * samples colours -> n colours, and with want_float their
        ToVector3() as float32 (n, 3).  Host form: a uint32 array; device=True: a contiguous int32 CUDA tensor."""
        if samples not in (4, 16):
            raise ValueError("FoldSamples: samples is 4 or 16")
        st, lib = abi.xrt_stats(), abi.lib()
        if device:
            import torch
            if colors.dtype != torch.int32 or not colors.is_contiguous() or not colors.is_cuda or colors.numel() % samples:
                raise ValueError("colors: a contiguous int32 CUDA tensor of n * samples packed colours")
            n = colors.numel() // samples
            rgba = torch.empty(n, dtype=torch.int32, device=colors.device)
            rgbf = torch.empty((n, 3), dtype=torch.float32, device=colors.device) if want_float else None
            s = stream if stream is not None else torch.cuda.current_stream(colors.device)
            abi.check(lib.xrt_fold_samples_device(self._scene_handle(), C.c_void_p(colors.data_ptr()), n, int(samples), C.c_void_p(rgba.data_ptr()),
                                                  C.c_void_p(rgbf.data_ptr()) if want_float else None, C.c_void_p(s.cuda_stream), C.byref(st)))
        else:
            colors = np.ascontiguousarray(colors)
            if colors.dtype != np.uint32 or colors.size % samples:
                raise ValueError("colors: uint32, n * samples packed colours")
            n = colors.size // samples
            rgba = np.zeros(n, dtype=np.uint32)
            rgbf = np.zeros((n, 3), dtype=np.float32) if want_float else None
            abi.check(lib.xrt_fold_samples(self._scene_handle(), colors.ctypes.data_as(C.POINTER(C.c_uint32)), n, int(samples),
                                           rgba.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(rgbf) if want_float else None, C.byref(st)))
        self.last_stats = st.as_dict()
        return (rgba, rgbf) if want_float else rgba

    def CastRay(self, ray, iteration=0, origin=None, currentRefIndex=1.0, want_float=False):
        """RT:506: one ray = (position, direction) -> the packed Color (and its float colour vector with want_float).  origin: the
        triangle the ray leaves, (mesh, index in Mesh.Triangles[]) as GetRayIntersection's ignoreTriangle, or None.
        With RecordPoints the call appends its segments to `points` and leaves the ray as the reference's `ref Ray ray` holds it
        afterwards in last_ray = (position, direction)."""
        im, it = (-1, -1) if origin is None else (self.CurrentScene.mesh_id(origin[0]), int(origin[1]))
        out = self.CastRays(rays_array([ray[0]], [ray[1]], im, it), iteration, currentRefIndex, want_float)
        return (int(out[0][0]), out[1][0]) if want_float else int(out[0])

    def GeneratePrimaryRays(self):
        """The rays of RT:410-421 for the whole target."""
        cam = self._camera_abi()
        rays = np.zeros(self._target.Width * self._target.Height, dtype=RAY_DTYPE)
        abi.check(abi.lib().xrt_generate_primary_rays(self._scene_handle(), C.byref(cam), rays.ctypes.data_as(C.POINTER(abi.xrt_ray))))
        return rays
