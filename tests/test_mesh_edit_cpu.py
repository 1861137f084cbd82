"""xrt_scene_set_mesh_triangles without a GPU: the bindings; the host-side replacement (HostScene::set_mesh_triangles) -- after any
sequence of replacements every array the library uploads, the scene tree and the mesh trees are byte for byte what a scene made from
scratch with the replaced mesh holds, and exactly one mesh octree was built per call --; the same through the C-ABI on a host-only scene
(xrt_scene_get_tree, xrt_scene_save); leaves stored in runs; the replay of pose, material and shading edits; the traversal single-stepped on
the edited scene against the oracle; the error table, all or nothing; the Python mirror's Mesh.Triangles / Init(); and
tests/mesh_edit/host_mesh_edit.cpp, the same walk as a program of its own, plain and under ASan + UBSan.

The bodies' boxes are not touched by the call (SO:126-132), so every replacement here lies in the box of the mesh the scene was built with
(mesh_edit_py.fitted): the replaced spec then describes the same bodies, and a fresh scene or the oracle made from it is the scene the
header promises."""
import os
import re
import subprocess

import numpy as np
import pytest

import bodies_py
import mesh_edit_py
import tree_shapes
from bodies_py import hits_equal
from materials_py import RawScene, material_struct, with_materials
from mesh_edit_py import MeshEditEmul, empty_mesh, fitted, moved_vertices, replaced, set_mesh_triangles, shading_values
from poses_py import moved

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORT = "xrt_scene_set_mesh_triangles"
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
LEAF_RUN_MIN = 16   # xrt_core.h XRT_LEAF_RUN_MIN


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


def _kinds(xrt):
    f = xrt.fixtures
    return dict(crate1=f.crate(1), crate3=f.crate(3), sphere=bodies_py.sphere_mesh(xrt), heightfield=f.heightfield(32))


def _base(xrt, scene_threshold):
    """Three meshes, six bodies: five of one mesh each on a line, one of two meshes above them.  The spacing is twice the largest mesh's
    extent: with scene_threshold 2 no three world boxes share a point (OSM:101-113 would not terminate)."""
    k, mat = _kinds(xrt), xrt.configs.material
    s = xrt.configs.SceneSpec("mesh_edit")
    # (the heightfield in the octant of positive coordinates, its box with a corner at the origin: see "a smaller box" below)
    s.meshes = [(k["crate3"], mat(0.25)), (fitted(xrt, k["heightfield"], (0.0, 0.0, 0.0, 48.0, 16.0, 48.0)), mat(0.3)), (k["sphere"], mat(0.7, interpolate_normals=True))]
    u = float(2.0 * max(float((m.bbox[3:] - m.bbox[:3]).max()) for m, _ in s.meshes))
    s.objects = [([i % 3], (-2 * u + u * i, 0.0, 0.125 * u * i), (0.0, 0.1 * i, 0.0), ONE) for i in range(5)]
    s.objects.append(([2, 0], (0.0, 2.5 * u, 0.0), (0.2, 0.0, 0.1), (1.5, 1.0, 0.5)))
    s.camera = xrt.configs.camera((0, 120, 260), (0, 0, 0))
    s.lights = [xrt.configs.spot((0, 200, 300))]
    s.max_reflections = 2
    s.scene_threshold = scene_threshold
    return s.with_size(64, 36)


def _sequence(xrt, spec, k):
    """[(what, the MeshData mesh k takes)]: the four kinds (another kind and another triangle count; crate(1): the root is a leaf;
    heightfield(32): a real octree), the same mesh with its vertices moved, no triangles, a real mesh again.  Every one lies in the box of
    the mesh the scene was built with, and is given that box, except "a smaller box": the mesh box shrinks towards its far corner, the hull
    of box and origin -- the bodies' BoundingBox (SO:131) -- stays, and the pre-cull records change."""
    box = spec.meshes[k][0].bbox
    steps = [(name, fitted(xrt, data, box, shift=(0.3, -0.2, 0.1))) for name, data in _kinds(xrt).items()]
    steps.append(("vertices moved", moved_vertices(xrt, steps[-1][1], 11 + k)))
    steps.append(("no triangles", empty_mesh(xrt, box)))
    steps.append(("a real mesh again", fitted(xrt, _kinds(xrt)["sphere" if k != 2 else "crate3"], box)))
    if not box[:3].any() and float(box[3:].min()) > 0.0:
        small = np.concatenate([0.5 * box[3:], box[3:]])
        steps.append(("a smaller box", fitted(xrt, _kinds(xrt)["crate3"], small)))
    return steps


@pytest.mark.parametrize("scene_threshold", [2, 20])
def test_a_replaced_mesh_leaves_the_bytes_of_a_fresh_scene(xrt, scene_threshold, tmp_path):
    spec = _base(xrt, scene_threshold)
    emu = MeshEditEmul(spec)
    raw = RawScene(xrt, spec)
    now = spec
    for k in (0, 1, 2):   # the first, the middle and the last mesh
        for what, data in _sequence(xrt, spec, k):
            what = "mesh %d: %s" % (k, what)
            before = emu.trees_built()
            assert emu.set_mesh_triangles(k, data) == 0, (what, emu.error())
            assert emu.trees_built() == before + 1, what          # this mesh's octree and no other
            now = replaced(now, k, data)
            assert [bodies_py.body_box(now, o[0]).tolist() for o in now.objects] == [bodies_py.body_box(spec, o[0]).tolist() for o in spec.objects], what
            diff = emu.differs_from(MeshEditEmul(now))
            assert diff is None, "%s: %s differs from a scene made from scratch" % (what, diff)
            # ... and through the C-ABI on a host-only scene: the trees and the scene file
            assert set_mesh_triangles(xrt, raw.handle, k, data) == 0, (what, xrt.abi.lib().xrt_last_error())
            fresh = RawScene(xrt, now)
            for m in range(-1, len(now.meshes)):
                assert bodies_py.get_tree(xrt, raw.handle, m) == bodies_py.get_tree(xrt, fresh.handle, m), (what, m)
            assert raw.saved(tmp_path / "edited.xrts") == fresh.saved(tmp_path / "fresh.xrts"), what
            fresh.close()
    raw.close()


def test_the_pre_cull_records_follow_the_new_box(xrt):
    """The step "a smaller box" of _sequence exists for some mesh, and it changes the records of the bodies that name the mesh."""
    spec = _base(xrt, 20)
    ks = [k for k in range(3) if _sequence(xrt, spec, k)[-1][0] == "a smaller box"]
    assert ks
    k = ks[0]
    emu, same_box = MeshEditEmul(spec), MeshEditEmul(spec)
    data = _sequence(xrt, spec, k)[-1][1]
    assert emu.set_mesh_triangles(k, data) == 0
    kept = fitted(xrt, data, spec.meshes[k][0].bbox)
    kept.v, kept.surface_normal = data.v, data.surface_normal     # the same triangles under the old box
    assert same_box.set_mesh_triangles(k, kept) == 0
    assert emu.differs_from(same_box) in ("arrays.scull", "arrays.meshes", "arrays.objects")


def test_runs_and_the_parts_behind_them(xrt):
    """At mesh threshold 50 heightfield(32) has leaves of LEAF_RUN_MIN references and more: stored in runs (spatial_runs, runTB), and the
    meshes behind it, one of them with runs of its own, move (runBase, the run offsets of lrec)."""
    spec = _base(xrt, 20)
    assert spec.mesh_threshold == 50
    emu = MeshEditEmul(spec)
    assert int(emu.leaf_sizes(1).max()) >= LEAF_RUN_MIN            # mesh 1, behind the replaced one, has runs
    data = fitted(xrt, _kinds(xrt)["heightfield"], spec.meshes[0][0].bbox)
    assert emu.set_mesh_triangles(0, data) == 0
    assert int(emu.leaf_sizes(0).max()) >= LEAF_RUN_MIN
    now = replaced(spec, 0, data)
    assert emu.differs_from(MeshEditEmul(now)) is None
    raw = RawScene(xrt, spec)
    assert set_mesh_triangles(xrt, raw.handle, 0, data) == 0
    nodes = np.frombuffer(bodies_py.get_tree(xrt, raw.handle, 0)[0], dtype=bodies_py.NODE_DTYPE)
    assert int(nodes["count"][nodes["is_leaf"] != 0].max()) >= LEAF_RUN_MIN
    # ... and back to a mesh without runs: the runs of mesh 1 move the other way
    small = fitted(xrt, _kinds(xrt)["crate1"], spec.meshes[0][0].bbox)
    assert emu.set_mesh_triangles(0, small) == 0
    assert emu.differs_from(MeshEditEmul(replaced(spec, 0, small))) is None
    raw.close()


def test_replay_equivalence(xrt):
    """A body that names the mesh moved after the build, a material set, triangle values of another mesh set, then the mesh replaced: the
    scene equals fresh + the same replay.  The scene tree is NOT rebuilt: it still holds the build-time filing."""
    spec = _base(xrt, 2)
    pose = ((33.0, 9.0, -21.0), (0.3, 0.2, 0.1), (1.25, 0.75, 1.0))
    mat = with_materials(spec, {0: dict(reflectiveness=0.875, transparent=True, refraction_index=1.5)})
    nrm, uv, col, shaded = shading_values(spec.meshes[2][0], 5, 40, 3)

    def replay(e, s):
        e.set_pose(s, 0, *pose)                                   # body 0 names mesh 0
        e.set_material(0, material_struct(mat.meshes[0][1], False)[0])
        e.set_triangle_shading(2, 5, nrm, uv, col)
    emu = MeshEditEmul(spec)
    replay(emu, spec)
    data = fitted(xrt, _kinds(xrt)["heightfield"], spec.meshes[0][0].bbox)
    assert emu.set_mesh_triangles(0, data) == 0
    now = replaced(spec, 0, data)
    fresh = MeshEditEmul(now)
    replay(fresh, now)
    assert emu.differs_from(fresh) is None
    # a scene BUILT with the moved pose files body 0 elsewhere: the edited scene does not equal it
    rebuilt = MeshEditEmul(replaced(moved(mat, {0: pose}), 0, data))
    rebuilt.set_triangle_shading(2, 5, nrm, uv, col)
    assert emu.differs_from(rebuilt) is not None


@pytest.mark.parametrize("scene_threshold", [2, 20])
def test_single_stepped_traversal_of_the_edited_scene_equals_the_oracle(xrt, orc, scene_threshold):
    spec = _base(xrt, scene_threshold)
    emu = MeshEditEmul(spec)
    rays = np.concatenate([orc.OracleScene(spec).primary_rays(), bodies_py.random_rays(xrt, 3000, 5, spread=400.0, aim=250.0)])
    now = spec
    for k, kind in ((0, "heightfield"), (2, "crate1"), (1, "sphere"), (0, None)):
        data = empty_mesh(xrt, spec.meshes[k][0].bbox) if kind is None else fitted(xrt, _kinds(xrt)[kind], spec.meshes[k][0].bbox)
        assert emu.set_mesh_triangles(k, data) == 0
        now = replaced(now, k, data)
        oracle = orc.OracleScene(now)
        want = oracle.intersect(rays)
        msg = hits_equal(emu.intersect(rays), want)
        assert msg is None, "mesh %d <- %s: %s" % (k, kind, msg)
        assert want["hit"].any()
        # ... and again with every ray that hit ignoring the triangle it hit: ids of the NEW arrays
        again = rays.copy()
        hit = want["hit"] != 0
        again["ignore_mesh"][hit], again["ignore_tri"][hit] = want["mesh"][hit], want["tri"][hit]
        if kind is not None:
            assert (want["mesh"][hit] == k).any() and int(want["tri"][hit][want["mesh"][hit] == k].max()) < data.ntri
        msg = hits_equal(emu.intersect(again), oracle.intersect(again))
        assert msg is None, "mesh %d <- %s, with ignore_tri: %s" % (k, kind, msg)


def _coincident(xrt, n):
    """n triangles with the same three vertices: above the threshold MeshOctree.BuildTree would not terminate (MO:84-96)."""
    one = xrt.fixtures.crate(1)
    return xrt.fixtures.MeshData(np.repeat(one.v[:1], n, axis=0), np.repeat(one.n[:1], n, axis=0), np.repeat(one.uv[:1], n, axis=0), np.repeat(one.color[:1], n, axis=0))


def test_error_table_all_or_nothing(xrt, tmp_path):
    abi, lib = xrt.abi, xrt.abi.lib()
    spec = _base(xrt, 20)
    scene, emu, untouched = RawScene(xrt, spec), MeshEditEmul(spec), MeshEditEmul(spec)
    good = mesh_edit_py.TriArgs(fitted(xrt, _kinds(xrt)["crate1"], spec.meshes[1][0].bbox))
    v, n, uv, sn, col, ntri, bbox = good.args()
    call = lib.xrt_scene_set_mesh_triangles
    heap = _coincident(xrt, spec.mesh_threshold + 1)
    bad = [
        ("null scene", abi.XRT_E_INVALID_ARG, lambda: call(None, 1, v, n, uv, sn, col, ntri, bbox)),
        ("a mesh id too large", abi.XRT_E_INVALID_ARG, lambda: call(scene.handle, 3, v, n, uv, sn, col, ntri, bbox)),
        ("a negative mesh id", abi.XRT_E_INVALID_ARG, lambda: call(scene.handle, -1, v, n, uv, sn, col, ntri, bbox)),
        ("ntri < 0", abi.XRT_E_INVALID_ARG, lambda: call(scene.handle, 1, v, n, uv, sn, col, -1, bbox)),
        ("null v", abi.XRT_E_INVALID_ARG, lambda: call(scene.handle, 1, None, n, uv, sn, col, ntri, bbox)),
        ("null surf_n", abi.XRT_E_INVALID_ARG, lambda: call(scene.handle, 1, v, n, uv, None, col, ntri, bbox)),
        ("null bbox", abi.XRT_E_INVALID_ARG, lambda: call(scene.handle, 1, v, n, uv, sn, col, ntri, None)),
        ("too many triangles", abi.XRT_E_INVALID_ARG, lambda: call(scene.handle, 1, v, n, uv, sn, col, 1 << 28, bbox)),
        ("more coincident triangles than the threshold", abi.XRT_E_UNSUPPORTED, lambda: set_mesh_triangles(xrt, scene.handle, 1, heap)),
    ]
    before = scene.saved(tmp_path / "before.xrts")
    trees = [bodies_py.get_tree(xrt, scene.handle, m) for m in range(-1, 3)]
    for what, code, f in bad:
        assert f() == code, what
        assert scene.saved(tmp_path / "after.xrts") == before, what
        assert [bodies_py.get_tree(xrt, scene.handle, m) for m in range(-1, 3)] == trees, what
    # the same codes from the host-side edit, whose arrays are compared byte for byte with an untouched scene's
    L = mesh_edit_py.emu_lib()
    for what, code, args in (("id", abi.XRT_E_INVALID_ARG, (3, v, n, uv, sn, col, ntri, bbox)), ("ntri", abi.XRT_E_INVALID_ARG, (1, v, n, uv, sn, col, -1, bbox)),
                             ("v", abi.XRT_E_INVALID_ARG, (1, None, n, uv, sn, col, ntri, bbox)), ("many", abi.XRT_E_INVALID_ARG, (1, v, n, uv, sn, col, 1 << 28, bbox))):
        assert L.emu_set_mesh_triangles(emu.h, *args) == code, what
        assert emu.differs_from(untouched) is None, what
    assert emu.set_mesh_triangles(1, heap) == abi.XRT_E_UNSUPPORTED
    assert emu.differs_from(untouched) is None
    # NULL n / uv / color: the defaults of xrt_scene_add_mesh
    assert call(scene.handle, 1, v, None, None, sn, None, ntri, bbox) == 0
    d = fitted(xrt, _kinds(xrt)["crate1"], spec.meshes[1][0].bbox)
    d.n, d.uv, d.color = np.zeros_like(d.n), np.zeros_like(d.uv), np.ones_like(d.color)
    assert scene.saved(tmp_path / "after.xrts") == RawScene(xrt, replaced(spec, 1, d)).saved(tmp_path / "fresh.xrts")
    scene.close()


def test_a_tree_too_deep_for_the_stack_is_refused_and_nothing_changes(xrt, tmp_path):
    """tests/tree_shapes.py's 41-word scene: nineteen nested bodies (scene depth 19) of the depth-20 staircase.  Built with the depth-6
    staircase (27 words) it is accepted; the depth-20 staircase in its place needs (19 + 1) + (20 + 1) = 41 > 40 words."""
    abi = xrt.abi
    c = tree_shapes.REFUSED
    assert c["words"] == 41
    shallow = tree_shapes.nested_bodies(xrt, c["arg"], tree_shapes.staircase(xrt, 6), mesh_threshold=1, p=2.0 * tree_shapes.S)
    deep = tree_shapes.staircase(xrt, c["md"])
    assert np.array_equal(deep.bbox, shallow.meshes[0][0].bbox)
    scene, emu, untouched = RawScene(xrt, shallow), MeshEditEmul(shallow), MeshEditEmul(shallow)
    before = scene.saved(tmp_path / "before.xrts")
    nodes = np.frombuffer(bodies_py.get_tree(xrt, scene.handle, -1)[0], dtype=bodies_py.NODE_DTYPE)
    assert int(nodes["depth"].max()) == c["sd"]
    assert set_mesh_triangles(xrt, scene.handle, 0, deep) == abi.XRT_E_UNSUPPORTED
    assert "stack" in xrt.abi.lib().xrt_last_error().decode()
    assert scene.saved(tmp_path / "after.xrts") == before
    assert emu.set_mesh_triangles(0, deep) == abi.XRT_E_UNSUPPORTED and emu.differs_from(untouched) is None
    # one level less fits: 40 words, the last size accepted
    ok = tree_shapes.staircase(xrt, c["md"] - 1)
    assert set_mesh_triangles(xrt, scene.handle, 0, ok) == 0
    assert scene.saved(tmp_path / "after.xrts") == RawScene(xrt, replaced(shallow, 0, ok)).saved(tmp_path / "fresh.xrts")
    scene.close()


def test_a_call_before_the_first_build_edits_what_the_build_uses(xrt, tmp_path):
    lib = xrt.abi.lib()
    spec = _base(xrt, 20)
    data = fitted(xrt, _kinds(xrt)["heightfield"], spec.meshes[0][0].bbox)
    def before_build(h):
        assert set_mesh_triangles(xrt, h, 0, data) == 0
    edited = RawScene(xrt, spec, before_build=before_build)
    assert edited.saved(tmp_path / "a.xrts") == RawScene(xrt, replaced(spec, 0, data)).saved(tmp_path / "b.xrts")
    # ... also for a mesh added after a build and not built yet
    more = bodies_py.edited(spec, meshes=[(_kinds(xrt)["crate1"], xrt.configs.material(0.1))])
    bodies_py.add_meshes(xrt, edited.handle, more, 3)
    other = fitted(xrt, _kinds(xrt)["sphere"], more.meshes[3][0].bbox)
    assert set_mesh_triangles(xrt, edited.handle, 3, other) == 0
    now = replaced(replaced(more, 0, data), 3, other)
    assert bodies_py.set_bodies(xrt, edited.handle, now) == (0, 1)
    assert edited.saved(tmp_path / "a.xrts") == RawScene(xrt, now).saved(tmp_path / "b.xrts")
    edited.close()


def test_python_mirror_pushes_an_initialised_mesh_once(xrt, tmp_path, monkeypatch):
    api = xrt.api
    spec = _base(xrt, 20)
    a, _ = xrt.configs.build_product(spec, device=-1)
    assert a.last_build_meshes == 3
    crate = a.meshes[0]
    b = api.OctreeSpatialManager(device=-1)                       # a second manager that shares the mesh
    b.Bodies = [api.SceneObject([crate], (0.0, 0.0, 0.0)), api.SceneObject([crate], (90.0, 0.0, 0.0))]
    b.Build()
    calls = []
    real = api.OctreeSpatialManager.SetMeshTriangles
    monkeypatch.setattr(api.OctreeSpatialManager, "SetMeshTriangles", lambda self, *args, **kw: (calls.append(self), real(self, *args, **kw))[1])
    handle = a.handle.value
    data = fitted(xrt, _kinds(xrt)["heightfield"], spec.meshes[0][0].bbox)
    crate.Triangles = data
    crate.Init()
    assert calls == [] and crate.Octree is not None               # its own MeshOctree, as ever; nothing travels before the next query, frame, Save or Build
    crate.Init()                                                  # (no assignment since: the mesh is not marked again)
    a.Save(tmp_path / "a.xrts")
    assert calls == [a] and a.last_build_meshes == 3 and a.handle.value == handle
    now = replaced(spec, 0, data)
    assert (tmp_path / "a.xrts").read_bytes() == RawScene(xrt, now).saved(tmp_path / "b.xrts")
    a.Save(tmp_path / "a.xrts")
    a.Build()                                                     # same list: xrt_scene_build_tree, nothing to push
    assert calls == [a] and a.handle.value == handle
    b.Save(tmp_path / "c.xrts")                                   # the shared mesh reaches the other manager too, once
    b.Save(tmp_path / "c.xrts")
    assert calls == [a, b]
    # the direct call with a Mesh; MeshBoundingBox assigned with the triangles
    small = np.concatenate([0.5 * spec.meshes[1][0].bbox[3:], spec.meshes[1][0].bbox[3:]])   # (mesh 1's box has its corner at the origin: the bodies' boxes stay)
    other = fitted(xrt, _kinds(xrt)["crate3"], small)
    a.SetMeshTriangles(a.meshes[1], other, other.bbox)
    assert a.meshes[1].Triangles is other and np.array_equal(a.meshes[1].MeshBoundingBox, other.bbox)
    now = replaced(now, 1, other)
    a.Save(tmp_path / "a.xrts")
    assert calls == [a, b, a]
    assert (tmp_path / "a.xrts").read_bytes() == RawScene(xrt, now).saved(tmp_path / "b.xrts")
    # the mirror's copy of shading values follows the new triangles
    nrm, uv, col, shaded = shading_values(data, 3, 9, 8)
    a.SetTriangleShading(0, range(3, 12), nrm, uv, col)
    assert crate.Triangles is data and np.array_equal(data.color[3:12], col)
    # Save / Load round trip
    a.Save(tmp_path / "a.xrts")
    loaded = api.OctreeSpatialManager.Load(tmp_path / "a.xrts", device=-1)
    loaded.Save(tmp_path / "d.xrts")
    assert (tmp_path / "a.xrts").read_bytes() == (tmp_path / "d.xrts").read_bytes()
    for m in range(3):
        t0, t1 = a.tree(a.meshes[m]), api._get_tree(loaded._scene, m)
        assert t0[0].tobytes() == t1[0].tobytes() and t0[1].tobytes() == t1[1].tobytes()
    # Init() without an assignment, and on a mesh no manager holds, behaves as before: its own MeshOctree, nothing pushed
    a.meshes[2].Init()
    a.Save(tmp_path / "a.xrts")
    lone = api.Mesh(_kinds(xrt)["crate1"], api.Material(0.5), device=-1)
    lone.Triangles = _kinds(xrt)["crate3"]
    lone.Init()
    assert lone.Octree is not None and a.meshes[2].Octree is not None and calls == [a, b, a]


def test_sanitizer_program(xrt):
    """tests/mesh_edit/host_mesh_edit.cpp walks the replacements and the error table on host-only scenes, once as built plainly against
    the library and once with the library's sources under ASan + UBSan (csrc/Makefile `hostcheck_mesh_edit`)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "xna-ray-trace_amd", "csrc"), "hostcheck_mesh_edit"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for prog in (mesh_edit_py.HOST_PLAIN, mesh_edit_py.HOST_SANITIZED):
        p = subprocess.run([prog], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert p.returncode == 0 and p.stdout.strip() == "host_mesh_edit: ok" and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (prog, p.stdout, p.stderr[-2000:])
