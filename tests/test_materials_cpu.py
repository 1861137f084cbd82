"""xrt_scene_set_materials without a GPU: the bindings, the host-side update (HostScene::set_materials) seen through the scene file --
after any sequence of updates xrt_scene_save writes byte for byte what a scene made from scratch with the final materials writes --,
updates before and after the build, the error codes, all-or-nothing, duplicates, and the Python mirror's push of changed Materials."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from materials_py import RawScene, gen_texture, material_struct, set_materials, with_materials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORT = "xrt_scene_set_materials"


def test_export_is_bound_everywhere(xrt):
    hdr = open(os.path.join(ROOT, "include", "xrt.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "XrtNative.cs")).read()
    src = open(os.path.join(ROOT, "xna-ray-trace_amd", "_abi.py")).read()
    assert re.search(r"\bint %s\(" % EXPORT, hdr)
    assert re.search(r"public static extern int %s\(" % EXPORT, cs)
    assert getattr(xrt.abi.lib(), EXPORT) is not None
    assert '"%s"' % EXPORT in src
    assert re.search(r"#define XRT_VERSION 203\b", hdr) and xrt.abi.lib().xrt_version() == 203 == xrt.abi.XRT_VERSION
    assert "PushMaterials" in open(os.path.join(ROOT, "csharp", "GpuSpatialManager.cs")).read()


# content_scene: 0 textured ground plane, 1 glass monkey, 2 torus, 3 glass sphere, 4 cube
TEX_A = gen_texture(5, 3, 1)              # another size than the checkers, with alpha and a premultiplied copy
TEX_B = gen_texture(7, 2, 2, alpha=False)


def _sequence(spec):
    """[(entries of one call as (mesh, material dict, send texels), spec after the call)]: scalars, a texture replaced by another size,
    use_texture off and on again with NULL texels, a texture given to a mesh that had none."""
    steps = []
    s1 = with_materials(spec, {2: dict(reflectiveness=0.25), 4: dict(interpolate_normals=False), 1: dict(refraction_index=1.5, transparent=False)})
    steps.append(([(m, s1.meshes[m][1], False) for m in (2, 4, 1)], s1))
    s2 = with_materials(s1, {0: dict(texture=TEX_A[0], texture_pargb=TEX_A[1])})
    steps.append(([(0, s2.meshes[0][1], True)], s2))
    s3 = with_materials(s2, {0: dict(use_texture=False)})
    steps.append(([(0, s3.meshes[0][1], False)], s3))
    steps.append(([(0, s2.meshes[0][1], False)], s2))          # on again, NULL texels: TEX_A is back
    s5 = with_materials(s2, {4: dict(texture=TEX_B[0]), 3: dict(transparent=False, reflectiveness=0.0)})
    steps.append(([(4, s5.meshes[4][1], True), (3, s5.meshes[3][1], False)], s5))
    return steps


def _apply(xrt, handle, entries):
    structs = [material_struct(m, texels) for _, m, texels in entries]   # (kept alive until the call returns)
    rc = set_materials(xrt, handle, [(e[0], st[0]) for e, st in zip(entries, structs)])
    assert rc == 0, xrt.abi.lib().xrt_last_error()


@pytest.fixture(scope="module")
def spec(xrt):
    return xrt.configs.content_scene(96, 54, max_reflections=3)


def test_updates_after_the_build_are_what_save_writes(xrt, spec, tmp_path):
    scene = RawScene(xrt, spec)
    for k, (entries, after) in enumerate(_sequence(spec)):
        _apply(xrt, scene.handle, entries)
        got = scene.saved(tmp_path / "updated.xrts")
        fresh = RawScene(xrt, after)
        assert got == fresh.saved(tmp_path / "fresh.xrts"), "step %d" % k
        fresh.close()
    # the file loads, builds, and saves itself again
    h = C.c_void_p()
    lib = xrt.abi.lib()
    assert lib.xrt_scene_load(-1, str(tmp_path / "updated.xrts").encode(), C.byref(h)) == 0
    assert lib.xrt_scene_build(h, spec.mesh_threshold, spec.scene_threshold) == 0
    assert lib.xrt_scene_save(h, str(tmp_path / "again.xrts").encode()) == 0
    lib.xrt_scene_destroy(h)
    assert (tmp_path / "again.xrts").read_bytes() == got
    scene.close()


def test_updates_before_the_build_are_what_the_build_uses(xrt, spec, tmp_path):
    steps = _sequence(spec)

    def before(handle):
        for entries, _ in steps:
            _apply(xrt, handle, entries)
    scene = RawScene(xrt, spec, before_build=before)
    fresh = RawScene(xrt, steps[-1][1])
    assert scene.saved(tmp_path / "a.xrts") == fresh.saved(tmp_path / "b.xrts")
    # ... and updates on both sides of the build
    half = RawScene(xrt, spec, before_build=lambda h: [_apply(xrt, h, e) for e, _ in steps[:2]])
    for entries, _ in steps[2:]:
        _apply(xrt, half.handle, entries)
    assert half.saved(tmp_path / "c.xrts") == (tmp_path / "b.xrts").read_bytes()
    for s in (scene, fresh, half):
        s.close()


def test_error_codes_and_all_or_nothing(xrt, spec, tmp_path):
    abi, lib = xrt.abi, xrt.abi.lib()
    scene = RawScene(xrt, spec)
    mats = [m for _, m in spec.meshes]
    ok = material_struct(mats[2], False)[0]
    one = np.zeros(1, dtype=np.int32)
    ids = one.ctypes.data_as(C.POINTER(C.c_int32))
    assert set_materials(xrt, scene.handle, [(5, ok)]) == abi.XRT_E_INVALID_ARG        # five meshes: ids 0 .. 4
    assert set_materials(xrt, scene.handle, [(-1, ok)]) == abi.XRT_E_INVALID_ARG
    assert lib.xrt_scene_set_materials(scene.handle, ids, -1, C.byref(ok)) == abi.XRT_E_INVALID_ARG
    assert lib.xrt_scene_set_materials(scene.handle, None, 1, C.byref(ok)) == abi.XRT_E_INVALID_ARG
    assert lib.xrt_scene_set_materials(scene.handle, ids, 1, None) == abi.XRT_E_INVALID_ARG
    assert lib.xrt_scene_set_materials(None, ids, 1, C.byref(ok)) == abi.XRT_E_INVALID_ARG
    assert lib.xrt_scene_set_materials(scene.handle, None, 0, None) == abi.XRT_OK       # n == 0 does nothing
    wants_texels = material_struct(dict(mats[2], use_texture=True), False)[0]
    assert set_materials(xrt, scene.handle, [(2, wants_texels)]) == abi.XRT_E_INVALID_ARG   # the torus never had texels
    kept = material_struct(mats[0], False)[0]
    h, w = mats[0]["texture"].shape
    kept.tex_width, kept.tex_height = w, h
    assert set_materials(xrt, scene.handle, [(0, kept)]) == abi.XRT_OK                  # the stored size is accepted ...
    kept.tex_width = w + 1
    assert set_materials(xrt, scene.handle, [(0, kept)]) == abi.XRT_E_INVALID_ARG       # ... another is not
    kept.tex_width, kept.tex_height = w, 0
    assert set_materials(xrt, scene.handle, [(0, kept)]) == abi.XRT_E_INVALID_ARG
    # what xrt_scene_add_mesh rejects: texels without a size
    sized, keep = material_struct(mats[0], True)
    sized.tex_width = 0
    assert set_materials(xrt, scene.handle, [(0, sized)]) == abi.XRT_E_INVALID_ARG
    # a call of three entries whose last one is bad applies nothing
    before = scene.saved(tmp_path / "before.xrts")
    e0 = material_struct(dict(mats[2], reflectiveness=0.125), False)[0]
    e1, keep1 = material_struct(dict(mats[4], use_texture=True, texture=TEX_B[0]), True)
    assert set_materials(xrt, scene.handle, [(2, e0), (4, e1), (3, wants_texels)]) == abi.XRT_E_INVALID_ARG
    assert scene.saved(tmp_path / "after.xrts") == before
    assert set_materials(xrt, scene.handle, [(2, e0), (4, e1)]) == abi.XRT_OK           # (the two good ones alone do change it)
    assert scene.saved(tmp_path / "after.xrts") != before
    scene.close()


def test_a_mesh_listed_twice_takes_its_last_entry(xrt, spec, tmp_path):
    scene = RawScene(xrt, spec)
    first = with_materials(spec, {2: dict(reflectiveness=0.9, transparent=True), 0: dict(texture=TEX_B[0])})
    last = with_materials(spec, {2: dict(reflectiveness=0.1), 0: dict(texture=TEX_A[0], texture_pargb=TEX_A[1])})
    _apply(xrt, scene.handle, [(2, first.meshes[2][1], False), (0, first.meshes[0][1], True), (0, last.meshes[0][1], True), (2, last.meshes[2][1], False)])
    fresh = RawScene(xrt, last)
    assert scene.saved(tmp_path / "a.xrts") == fresh.saved(tmp_path / "b.xrts")
    scene.close()
    fresh.close()


def test_python_materials_are_pushed_before_save_and_build(xrt, tmp_path):
    """The mirror: a property set on a Material (shared by two meshes: pushed for each), another Material assigned to Mesh.MeshMaterial, a
    Texture replaced; Build() with the same bodies stays on the same library scene."""
    spec = xrt.configs.crate_grid_scene(64, 36, n=2, grid=2)
    spec.meshes.append((xrt.fixtures.crate(1), spec.meshes[0][1]))
    spec.objects.append(([1], (0.0, 30.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    scene, _ = xrt.configs.build_product(spec, device=-1)
    shared = scene.meshes[0].MeshMaterial
    scene.meshes[1].MeshMaterial = shared                      # one Material for both meshes (TMP:121-131)
    serial = shared._serial
    shared.Reflectiveness = 0.875
    shared.InterpolateNormals = True
    assert shared._serial == serial + 2
    handle = scene.handle.value
    scene.Build()
    assert scene.handle.value == handle                        # xrt_scene_build_tree, not a new build
    scene.Save(tmp_path / "a.xrts")
    want = with_materials(spec, {m: dict(reflectiveness=0.875, interpolate_normals=True) for m in (0, 1)})
    xrt.configs.build_product(want, device=-1)[0].Save(tmp_path / "b.xrts")
    assert (tmp_path / "a.xrts").read_bytes() == (tmp_path / "b.xrts").read_bytes()
    # a new Texture on the shared Material, and another Material on mesh 1
    shared.Texture, shared.TexturePArgb = TEX_A
    scene.meshes[1].MeshMaterial = xrt.api.Material(0.25, False, True, 1.5)
    scene.Save(tmp_path / "a.xrts")
    want = with_materials(want, {0: dict(texture=TEX_A[0], texture_pargb=TEX_A[1]),
                                 1: dict(reflectiveness=0.25, transparent=True, refraction_index=1.5, interpolate_normals=False, use_texture=False, texture=None)})
    xrt.configs.build_product(want, device=-1)[0].Save(tmp_path / "b.xrts")
    assert (tmp_path / "a.xrts").read_bytes() == (tmp_path / "b.xrts").read_bytes()
    # UseTexture off and on again: the texels do not travel a second time, the library kept them
    shared.UseTexture = False
    scene.Save(tmp_path / "off.xrts")
    shared.UseTexture = True
    assert scene._pushed_tex[0] == (shared, shared._tex_serial)
    scene.Save(tmp_path / "a.xrts")
    assert (tmp_path / "a.xrts").read_bytes() == (tmp_path / "b.xrts").read_bytes() != (tmp_path / "off.xrts").read_bytes()
    # the explicit form
    scene.SetMaterials([0], [xrt.api.Material(0.5, False)])
    scene.Save(tmp_path / "a.xrts")
    want = with_materials(want, {0: dict(reflectiveness=0.5, interpolate_normals=False, use_texture=False, texture=None)})
    xrt.configs.build_product(want, device=-1)[0].Save(tmp_path / "b.xrts")
    assert (tmp_path / "a.xrts").read_bytes() == (tmp_path / "b.xrts").read_bytes()
