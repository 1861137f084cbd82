"""xrt_scene_set_bodies without a GPU: the bindings; the host-side list edit (HostScene::set_bodies) -- after any sequence of edits every
array the library uploads, the scene tree and the mesh trees are byte for byte what a scene made from scratch with the same meshes (in id
order) and bodies holds --; the same through the C-ABI (xrt_scene_get_tree, xrt_scene_save); the traversal single-stepped on the edited
scene against the oracle; meshes_built_out, the materials that stay, the error table, and the Python mirror's Build().
(tests/bodies/host_bodies.cpp walks the same edits as a program of its own for the sanitizer build, `make -C csrc hostcheck_bodies`.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bodies_py
from bodies_py import BodiesEmul, BodyArrays, edited, hits_equal, set_bodies
from materials_py import RawScene, gen_texture, material_struct, set_materials, with_materials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORT = "xrt_scene_set_bodies"
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def test_export_is_bound_everywhere(xrt):
    hdr = open(os.path.join(ROOT, "include", "xrt.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "XrtNative.cs")).read()
    src = open(os.path.join(ROOT, "xna-ray-trace_amd", "_abi.py")).read()
    assert re.search(r"\bint %s\(" % EXPORT, hdr)
    assert re.search(r"public static extern int %s\(" % EXPORT, cs)
    assert getattr(xrt.abi.lib(), EXPORT) is not None
    assert '"%s"' % EXPORT in src
    assert re.search(r"#define XRT_VERSION 203\b", hdr) and xrt.abi.lib().xrt_version() == 203 == xrt.abi.XRT_VERSION
    assert EXPORT in open(os.path.join(ROOT, "csharp", "GpuSpatialManager.cs")).read()


def _meshes(xrt):
    f, mat = xrt.fixtures, xrt.configs.material
    return dict(crate1=(f.crate(1), mat(0.5, texture=gen_texture(4, 3, 7, alpha=False)[0])), crate3=(f.crate(3), mat(0.25)),
                sphere=(bodies_py.sphere_mesh(xrt), mat(0.7, interpolate_normals=True)), heightfield=(f.heightfield(32), mat(0.3)))


def _unit(xrt):
    return float(2.0 * max(float((m.bbox[3:] - m.bbox[:3]).max()) for m, _ in _meshes(xrt).values()))


def _base(xrt, kind, scene_threshold):
    """Five bodies of one mesh on a line, every mesh opaque.  The spacing u is twice the largest mesh's extent: with scene_threshold 2 no
    three world boxes of any list of _sequence may share a point (OSM:101-113 would not terminate)."""
    s = xrt.configs.SceneSpec("bodies_" + kind)
    s.meshes = [_meshes(xrt)[kind]]
    u = _unit(xrt)
    s.objects = [([0], (-2 * u + u * i, 0.0, 0.125 * u * i), (0.0, 0.1 * i, 0.0), ONE) for i in range(5)]
    s.camera = xrt.configs.camera((0, 120, 260), (0, 0, 0))
    s.lights = [xrt.configs.spot((0, 200, 300))]
    s.max_reflections = 2
    s.scene_threshold = scene_threshold
    return s.with_size(64, 36)


def _sequence(xrt, spec, kind):
    """[(what, spec after the step, meshes the step must build)]: bodies removed from the middle, the list reordered, bodies of known meshes
    added, a body of a new mesh, a new Transparent mesh in an opaque scene, the empty list, the list refilled (with a body of two meshes and
    one of none; the first mesh unused)."""
    others = [m for k, m in _meshes(xrt).items() if k != kind]
    glass = (bodies_py.sphere_mesh(xrt), xrt.configs.material(0.7, transparent=True, refraction_index=float(np.float32(1.32)), interpolate_normals=True))
    b = spec.objects
    u = _unit(xrt)
    steps = []
    s = edited(spec, objects=[b[0], b[3], b[4]])
    steps.append(("bodies removed from the middle", s, 0))
    s = edited(s, objects=[b[4], b[0], b[3]])
    steps.append(("reordered", s, 0))
    s = edited(s, objects=s.objects + [([0], (0.75 * u, 12.0, -1.5 * u), (0.4, 0.0, 0.2), (1.5, 0.5, 1.0)), ([0], (-0.75 * u, -5.0, 1.75 * u), ZERO, ONE)])
    steps.append(("bodies of a known mesh added", s, 0))
    s = edited(s, meshes=[others[0]], objects=s.objects + [([1], (0.0, 1.5 * u, 0.0), (0.0, 0.5, 0.0), ONE)])
    steps.append(("a body of a new mesh", s, 1))
    s = edited(s, meshes=[glass], objects=s.objects[:2] + [([2], (0.25 * u, 8.0, 3.5 * u), ZERO, (3.0, 3.0, 3.0))] + s.objects[2:])
    steps.append(("a new Transparent mesh", s, 1))
    s = edited(s, objects=[])
    steps.append(("the empty list", s, 0))
    s = edited(s, meshes=[others[1], others[2]],
               objects=[([3, 1], (0.0, 0.0, 0.0), ZERO, ONE), ([], (5.0, 5.0, 5.0), ZERO, ONE), ([2], (-u, 10.0, 0.5 * u), ZERO, (2.0, 2.0, 2.0)), ([4], (1.5 * u, 0.0, -0.5 * u), (0.0, 1.0, 0.0), ONE)])
    steps.append(("refilled", s, 2))
    return steps


@pytest.mark.parametrize("scene_threshold", [2, 20])
@pytest.mark.parametrize("kind", ["crate1", "crate3", "sphere", "heightfield"])
def test_an_edited_scene_holds_the_bytes_of_a_fresh_one(xrt, kind, scene_threshold, tmp_path):
    spec = _base(xrt, kind, scene_threshold)
    emu = BodiesEmul(spec)
    raw = RawScene(xrt, spec)
    known = len(spec.meshes)
    for what, after, n_new in _sequence(xrt, spec, kind):
        assert emu.set_bodies(after) == n_new, what
        fresh = BodiesEmul(after)
        diff = emu.differs_from(fresh)
        assert diff is None, "%s: %s differs from a scene made from scratch" % (what, diff)
        # ... and through the C-ABI on a host-only scene: the trees and the scene file
        rc, built = set_bodies(xrt, raw.handle, after, known)
        assert (rc, built) == (0, n_new), (what, rc, built, xrt.abi.lib().xrt_last_error())
        known = len(after.meshes)
        fresh_raw = RawScene(xrt, after)
        for m in range(-1, known):
            assert bodies_py.get_tree(xrt, raw.handle, m) == bodies_py.get_tree(xrt, fresh_raw.handle, m), (what, m)
        assert raw.saved(tmp_path / "edited.xrts") == fresh_raw.saved(tmp_path / "fresh.xrts"), what
        fresh_raw.close()
    raw.close()


def test_build_is_unchanged_after_edits_and_rebuilds_everything(xrt):
    """xrt_scene_build on an edited scene (the old way: add_object after a build, then build) still gives the fresh scene's bytes."""
    spec = _base(xrt, "crate3", 2)
    emu = BodiesEmul(spec)
    steps = _sequence(xrt, spec, "crate3")
    emu.set_bodies(steps[3][1])
    L = bodies_py.emu_lib()
    assert L.emu_build(emu.h, spec.mesh_threshold, spec.scene_threshold) == 0
    assert emu.differs_from(BodiesEmul(steps[3][1])) is None


@pytest.mark.parametrize("scene_threshold", [2, 20])
def test_single_stepped_traversal_of_the_edited_grid_equals_the_oracle(xrt, orc, scene_threshold):
    spec = xrt.configs.crate_grid_scene(64, 36, n=3, grid=3)
    spec.scene_threshold = scene_threshold
    emu = BodiesEmul(spec)
    rays = np.concatenate([orc.OracleScene(spec).primary_rays(), bodies_py.random_rays(xrt, 3000, 5)])
    b = spec.objects
    sphere = (bodies_py.sphere_mesh(xrt), xrt.configs.material(0.7, interpolate_normals=True))
    s1 = edited(spec, objects=[b[0], b[2], b[5], b[7], b[8]])
    s2 = edited(s1, objects=s1.objects + [([0], (15.0, 25.0, 10.0), (0.3, 0.9, -0.4), (1.5, 0.6, 1.0)), ([0], (-90.0, 0.0, 100.0), (0.0, 2.0, 0.0), ONE)])
    s3 = edited(s2, meshes=[sphere], objects=s2.objects[:3] + [([1], (0.0, 20.0, 60.0), ZERO, (6.0, 6.0, 6.0))] + s2.objects[3:])
    s4 = edited(s3, objects=list(reversed(s3.objects)))
    s5 = edited(s4, objects=[])
    s6 = edited(s5, objects=[b[4], ([1, 0], (40.0, 0.0, 40.0), ZERO, (2.0, 2.0, 2.0))])
    for what, after, n_new in (("four removed", s1, 0), ("two added", s2, 0), ("a sphere of a new mesh", s3, 1), ("reversed", s4, 0), ("empty", s5, 0), ("refilled", s6, 0)):
        assert emu.set_bodies(after) == n_new, what
        want = orc.OracleScene(after).intersect(rays)
        msg = hits_equal(emu.intersect(rays), want)
        assert msg is None, "%s: %s" % (what, msg)
        if after.objects:
            assert want["hit"].any() and int(want["object"].max()) < len(after.objects)


def _textured_pair(xrt):
    """Two bodies: a textured crate and a plain one (two meshes)."""
    s = xrt.configs.SceneSpec("pair")
    tex = gen_texture(5, 3, 3)
    s.meshes = [(xrt.fixtures.crate(1), xrt.configs.material(0.5, texture=tex[0], texture_pargb=tex[1])), (xrt.fixtures.crate(3), xrt.configs.material(0.25))]
    s.objects = [([0], (-20.0, 0.0, 0.0), ZERO, ONE), ([1], (20.0, 0.0, 0.0), ZERO, ONE)]
    s.camera = xrt.configs.camera((0, 32, 64), (0, 8, 0))
    s.lights = [xrt.configs.spot((0, 40, 60))]
    return s.with_size(32, 32)


def test_count_of_built_meshes_and_materials_that_stay(xrt, tmp_path):
    spec = _textured_pair(xrt)
    scene = RawScene(xrt, spec)
    assert set_bodies(xrt, scene.handle, edited(spec, objects=spec.objects[::-1])) == (0, 0)
    # the texture of mesh 0 switched off: the texels stay in the library ...
    off = with_materials(spec, {0: dict(use_texture=False)})
    assert set_materials(xrt, scene.handle, [(0, material_struct(off.meshes[0][1], False)[0])]) == 0
    # ... across a set_bodies that adds two meshes (one of them textured: the arena is packed again) ...
    tex2 = gen_texture(2, 2, 9, alpha=False)[0]
    more = [(bodies_py.sphere_mesh(xrt), xrt.configs.material(0.7, texture=tex2)), (xrt.fixtures.crate(1), xrt.configs.material(0.1))]
    after_off = edited(off, meshes=more, objects=spec.objects + [([2, 3], (0.0, 20.0, 0.0), ZERO, ONE)])
    assert set_bodies(xrt, scene.handle, after_off, 2) == (0, 2)
    assert set_bodies(xrt, scene.handle, after_off, 4) == (0, 0)       # nothing new: nothing built
    assert scene.saved(tmp_path / "a.xrts") == RawScene(xrt, after_off).saved(tmp_path / "b.xrts")
    # ... and use_texture = 1 with NULL texels brings them back
    assert set_materials(xrt, scene.handle, [(0, material_struct(spec.meshes[0][1], False)[0])]) == 0
    after_on = edited(spec, meshes=more, objects=after_off.objects)
    assert scene.saved(tmp_path / "a.xrts") == RawScene(xrt, after_on).saved(tmp_path / "b.xrts")
    # a mesh added and never named by a body is built all the same and stays
    unused = edited(after_on, meshes=[(xrt.fixtures.crate(3), xrt.configs.material(0.9))])
    assert set_bodies(xrt, scene.handle, unused, 4) == (0, 1)
    assert scene.saved(tmp_path / "a.xrts") == RawScene(xrt, unused).saved(tmp_path / "b.xrts")
    scene.close()


def test_materials_that_stay_in_the_arrays(xrt):
    """The same on HostScene itself: the arrays after set_materials + set_bodies are a fresh scene's, except that the fresh scene was never
    given the texels of the mesh whose texture is off -- so the comparison is made with the texture on again."""
    spec = _textured_pair(xrt)
    emu = BodiesEmul(spec)
    L = bodies_py.emu_lib()

    def set_mat(mesh, m):
        ids = np.array([mesh], dtype=np.int32)
        st = material_struct(m, False)[0]
        assert L.emu_set_materials(emu.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), 1, C.byref(st)) == 0
    set_mat(0, with_materials(spec, {0: dict(use_texture=False)}).meshes[0][1])
    changed = with_materials(spec, {1: dict(reflectiveness=0.75, transparent=True, refraction_index=1.5)})
    set_mat(1, changed.meshes[1][1])
    after = edited(changed, meshes=[(xrt.fixtures.heightfield(32), xrt.configs.material(0.3))], objects=spec.objects + [([2], (0.0, -10.0, 0.0), ZERO, ONE)])
    assert emu.set_bodies(after) == 1
    set_mat(0, spec.meshes[0][1])
    assert emu.differs_from(BodiesEmul(after)) is None


def test_error_table(xrt, tmp_path):
    abi, lib = xrt.abi, xrt.abi.lib()
    spec = _textured_pair(xrt)
    a = BodyArrays(spec)
    n, start, ids, w, iw, bb, wbb = a.args()
    # before the first build
    h = C.c_void_p()
    assert lib.xrt_scene_create(-1, C.byref(h)) == 0
    bodies_py.add_meshes(xrt, h, spec, 0)
    assert lib.xrt_scene_set_bodies(h, n, start, ids, w, iw, bb, wbb, 0, None) == abi.XRT_E_NOT_BUILT
    lib.xrt_scene_destroy(h)
    scene = RawScene(xrt, spec)
    before = scene.saved(tmp_path / "before.xrts")
    built = C.c_int32(-7)
    bad = [
        ("null scene", lambda: lib.xrt_scene_set_bodies(None, n, start, ids, w, iw, bb, wbb, 0, None)),
        ("n_bodies < 0", lambda: lib.xrt_scene_set_bodies(scene.handle, -1, start, ids, w, iw, bb, wbb, 0, None)),
        ("null mesh_start", lambda: lib.xrt_scene_set_bodies(scene.handle, n, None, ids, w, iw, bb, wbb, 0, None)),
        ("null mesh_start, no bodies", lambda: lib.xrt_scene_set_bodies(scene.handle, 0, None, None, None, None, None, None, 0, None)),
        ("null mesh_ids", lambda: lib.xrt_scene_set_bodies(scene.handle, n, start, None, w, iw, bb, wbb, 0, None)),
        ("null world", lambda: lib.xrt_scene_set_bodies(scene.handle, n, start, ids, None, iw, bb, wbb, 0, None)),
        ("null inv_world", lambda: lib.xrt_scene_set_bodies(scene.handle, n, start, ids, w, None, bb, wbb, 0, None)),
        ("null bbox", lambda: lib.xrt_scene_set_bodies(scene.handle, n, start, ids, w, iw, None, wbb, 0, None)),
        ("null world_bbox", lambda: lib.xrt_scene_set_bodies(scene.handle, n, start, ids, w, iw, bb, None, 0, C.byref(built))),
    ]

    def with_start(values):
        s = np.array(values, dtype=np.int32)
        return lambda: lib.xrt_scene_set_bodies(scene.handle, n, s.ctypes.data_as(C.POINTER(C.c_int32)), ids, w, iw, bb, wbb, 0, None)

    def with_ids(values):
        i = np.array(values, dtype=np.int32)
        return lambda: lib.xrt_scene_set_bodies(scene.handle, n, start, i.ctypes.data_as(C.POINTER(C.c_int32)), w, iw, bb, wbb, 0, None)
    bad += [("mesh_start[0] != 0", with_start([1, 1, 2])), ("a decreasing mesh_start", with_start([0, 2, 1])), ("a mesh id too large", with_ids([0, 2])),
            ("a negative mesh id", with_ids([-1, 1]))]
    for what, call in bad:
        assert call() == abi.XRT_E_INVALID_ARG, what
        assert scene.saved(tmp_path / "after.xrts") == before, what
    assert built.value == -7
    # the legal edge cases: no bodies (the id array is not needed), a body without meshes
    one = np.zeros(1, dtype=np.int32)
    assert lib.xrt_scene_set_bodies(scene.handle, 0, one.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None, None, 0, C.byref(built)) == 0
    assert built.value == 0 and scene.saved(tmp_path / "after.xrts") == RawScene(xrt, edited(spec, objects=[])).saved(tmp_path / "fresh.xrts")
    none = edited(spec, objects=[([], ZERO, ZERO, ONE)])
    assert set_bodies(xrt, scene.handle, none) == (0, 0)
    assert scene.saved(tmp_path / "after.xrts") == RawScene(xrt, none).saved(tmp_path / "fresh.xrts")
    # (XRT_E_UNSUPPORTED: test_a_list_the_scene_octree_cannot_hold_and_its_repair; XRT_E_BUSY needs a ticket: tests/test_gpu_bodies.py)
    # the older calls behave as before
    oid = C.c_int32(-1)
    assert lib.xrt_scene_add_object(scene.handle, ids, 1, w, iw, bb, wbb, C.byref(oid)) == 0 and oid.value == 1
    assert lib.xrt_scene_build(scene.handle, 0, 0) == 0
    scene.close()


def test_a_list_the_scene_octree_cannot_hold_and_its_repair(xrt, tmp_path):
    """XRT_E_UNSUPPORTED: three bodies with one world box at scene_threshold 2 (OSM:101-113 would not terminate).  The list is applied, the
    scene is left as xrt_scene_build_tree leaves it -- not built: no trees, nothing to trace; the file holds the new list --, the count of
    the octrees the call built is reported all the same, and the next legal call repairs the scene: a fresh scene's file and trees."""
    abi, lib = xrt.abi, xrt.abi.lib()
    spec = _textured_pair(xrt)
    spec.scene_threshold = 2
    scene = RawScene(xrt, spec)
    same = ([0], (5.0, 0.0, 0.0), ZERO, ONE)

    def refused(after, n_known, n_new):
        assert set_bodies(xrt, scene.handle, after, n_known) == (abi.XRT_E_UNSUPPORTED, n_new)
        nn, nr = C.c_int64(0), C.c_int64(0)
        assert lib.xrt_scene_get_tree(scene.handle, -1, None, C.byref(nn), None, C.byref(nr)) == abi.XRT_E_NOT_BUILT
        assert lib.xrt_scene_build_tree(scene.handle, 2) == abi.XRT_E_NOT_BUILT
        unbuilt = RawScene(xrt, edited(after, objects=[]))             # (the file of the refused list: a fresh scene cannot build it either)
        for ids, pos, rot, scale in after.objects:
            a = BodyArrays(edited(after, objects=[(ids, pos, rot, scale)]))
            oid = C.c_int32(-1)
            assert lib.xrt_scene_add_object(unbuilt.handle, a.ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), *a.args()[3:], C.byref(oid)) == 0
        assert scene.saved(tmp_path / "a.xrts") == unbuilt.saved(tmp_path / "b.xrts")
        unbuilt.close()

    def repaired(after, n_known):
        assert set_bodies(xrt, scene.handle, after, n_known) == (0, 0)   # (what the refused call built stays built)
        fresh = RawScene(xrt, after)
        for m in range(-1, len(after.meshes)):
            assert bodies_py.get_tree(xrt, scene.handle, m) == bodies_py.get_tree(xrt, fresh.handle, m), m
        assert scene.saved(tmp_path / "a.xrts") == fresh.saved(tmp_path / "b.xrts")
        fresh.close()
    # without a new mesh
    refused(edited(spec, objects=[same, same, same, spec.objects[1]]), 2, 0)
    repaired(edited(spec, objects=[spec.objects[1], same]), 2)
    # with a new mesh added before the refused call: its octree is built and counted by that call
    ball = (bodies_py.sphere_mesh(xrt), xrt.configs.material(0.7, interpolate_normals=True))
    more = edited(spec, meshes=[ball], objects=[same, ([2], (0.0, 30.0, 0.0), ZERO, ONE), same, same])
    refused(more, 2, 1)
    repaired(edited(more, objects=[more.objects[1], spec.objects[0], same]), 3)
    scene.close()
    # the same on HostScene: the arrays after the repair are a fresh scene's
    emu = BodiesEmul(spec)
    L = bodies_py.emu_lib()
    L.emu_add_mesh.restype = C.c_int
    bodies_py._add_meshes(lambda *a: L.emu_add_mesh(emu.h, *a), more, 2)
    emu.n_meshes = 3
    built = C.c_int32(-1)
    assert L.emu_set_bodies(emu.h, *BodyArrays(more).args(), 2, C.byref(built)) == abi.XRT_E_UNSUPPORTED and built.value == 1
    legal = edited(more, objects=[more.objects[1], spec.objects[0], same])
    assert emu.set_bodies(legal) == 0
    assert emu.differs_from(BodiesEmul(legal)) is None
    # the mirror: the Build() that fails has built the new Mesh's octree and says so; the next one repairs the same library scene
    msm, _ = xrt.configs.build_product(spec, device=-1)
    handle = msm.handle.value
    crate = msm.meshes[0]
    new = xrt.api.Mesh(ball[0], xrt.api.Material(0.7), device=-1)
    keep = list(msm.Bodies)
    msm.Bodies[:] = [xrt.api.SceneObject([crate], (5.0, 0.0, 0.0)) for _ in range(3)] + [xrt.api.SceneObject([new], (0.0, 30.0, 0.0))]
    with pytest.raises(abi.XrtError) as e:
        msm.Build()
    assert e.value.code == abi.XRT_E_UNSUPPORTED and msm.last_build_meshes == 1
    msm.Bodies[:] = keep + [msm.Bodies[3]]
    msm.Build()
    assert msm.handle.value == handle and msm.last_build_meshes == 0 and msm.mesh_id(new) == 2
    msm.Save(tmp_path / "a.xrts")
    want = edited(spec, meshes=[(ball[0], xrt.configs.material(0.7))], objects=spec.objects + [([2], (0.0, 30.0, 0.0), ZERO, ONE)])
    assert (tmp_path / "a.xrts").read_bytes() == RawScene(xrt, want).saved(tmp_path / "b.xrts")


def test_python_build_edits_the_list_on_the_same_scene(xrt, tmp_path):
    api = xrt.api
    spec = xrt.configs.crate_grid_scene(64, 36, n=2, grid=2)
    scene, _ = xrt.configs.build_product(spec, device=-1)
    assert scene.last_build_meshes == 1
    handle = scene.handle.value
    crate = scene.meshes[0]
    # a SceneObject appended, one removed
    scene.Bodies.append(api.SceneObject([crate], (0.0, 30.0, 0.0), (0.0, 0.5, 0.0)))
    del scene.Bodies[1]
    scene.Build()
    assert scene.handle.value == handle and scene.last_build_meshes == 0
    want = edited(spec, objects=[spec.objects[0]] + spec.objects[2:] + [([0], (0.0, 30.0, 0.0), (0.0, 0.5, 0.0), ONE)])
    scene.Save(tmp_path / "a.xrts")
    assert (tmp_path / "a.xrts").read_bytes() == RawScene(xrt, want).saved(tmp_path / "b.xrts")
    # a body of a new Mesh, with a material changed on the known one in the same Build
    crate.MeshMaterial.Reflectiveness = 0.125
    tex = gen_texture(3, 2, 4, alpha=False)[0]
    ball = api.Mesh(bodies_py.sphere_mesh(xrt), api.Material(0.7, True, False, 0.0, tex), device=-1)
    scene.Bodies.insert(1, api.SceneObject([ball, crate], (10.0, 5.0, 0.0)))
    scene.Build()
    assert scene.handle.value == handle and scene.last_build_meshes == 1 and scene.mesh_id(ball) == 1
    assert len(scene._pushed) == len(scene.Bodies) and len(scene._pushed_mats) == len(scene._pushed_tex) == len(scene.meshes) == 2
    want = with_materials(want, {0: dict(reflectiveness=0.125)})
    want = edited(want, meshes=[(ball.data, xrt.configs.material(0.7, texture=tex))], objects=want.objects[:1] + [([1, 0], (10.0, 5.0, 0.0), ZERO, ONE)] + want.objects[1:])
    scene.Save(tmp_path / "a.xrts")
    assert (tmp_path / "a.xrts").read_bytes() == RawScene(xrt, want).saved(tmp_path / "b.xrts")
    # setters after the edit reach the bodies at their new positions, materials the new mesh
    scene.Bodies[1].Position = (12.0, 5.0, 1.0)
    ball.MeshMaterial.Reflectiveness = 0.5
    scene.Save(tmp_path / "a.xrts")                       # (pushes materials; the pose travels with the next query, frame or Build)
    scene.Build()                                         # same list: xrt_scene_build_tree
    assert scene.handle.value == handle
    want = with_materials(want, {1: dict(reflectiveness=0.5)})
    want.objects[1] = ([1, 0], (12.0, 5.0, 1.0), ZERO, ONE)
    scene.Save(tmp_path / "a.xrts")
    assert (tmp_path / "a.xrts").read_bytes() == RawScene(xrt, want).saved(tmp_path / "b.xrts")
    # another mesh threshold: the full way, a new scene
    scene.meshItemTreshold = 64
    scene.Build()
    assert scene.handle.value != handle and scene.last_build_meshes == 2

