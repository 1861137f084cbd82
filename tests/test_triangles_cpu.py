"""xrt_scene_set_triangle_shading without a GPU: the bindings, the host-side edit (HostScene::set_triangle_shading) seen through the scene
file -- after any sequence of calls xrt_scene_save writes byte for byte what a scene made from scratch with the final values writes --,
calls before, after and on both sides of the build, the error codes, all-or-nothing, duplicates, xrt_scene_set_bodies with a new mesh, and
the Python mirror's MeshData.  (tests/triangles/host_triangles.cpp walks such a sequence as a program of its own for the sanitizer build,
`make -C csrc hostcheck_triangles`, and compares the shading records in memory as well.)"""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from materials_py import RawScene
from triangles_py import apply_edits, set_triangle_shading, with_triangle_shading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xna-ray-trace_amd", "csrc")
EXPORTS = ("xrt_scene_set_triangle_shading", "xrt_scene_set_triangle_shading_device")


def test_exports_are_bound_everywhere(xrt):
    hdr = open(os.path.join(ROOT, "include", "xrt.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "XrtNative.cs")).read()
    src = open(os.path.join(ROOT, "xna-ray-trace_amd", "_abi.py")).read()
    for export in EXPORTS:
        assert re.search(r"\bint %s\(" % export, hdr)
        assert re.search(r"public static extern int %s\(" % export, cs)
        assert getattr(xrt.abi.lib(), export) is not None
        assert '"%s"' % export in src
    assert re.search(r"#define XRT_VERSION 203\b", hdr) and xrt.abi.lib().xrt_version() == 203 == xrt.abi.XRT_VERSION
    assert "PushTriangleShading" in open(os.path.join(ROOT, "csharp", "GpuSpatialManager.cs")).read()


def _f(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _vals(rng, n):
    return dict(normals=rng.normal(size=(n, 3, 3)).astype(np.float32), uv=rng.uniform(-2, 2, size=(n, 3, 2)).astype(np.float32),
                color=rng.uniform(0, 1, size=(n, 4)).astype(np.float32))


def _sequence(spec):
    """[(the edits of one call, spec after the call)] on content_scene (0 plane, 1 monkey, 2 torus, 3 sphere, 4 cube): a range on mesh 0,
    an unsorted id list on mesh 2, one field at a time, special values, a triangle listed twice."""
    rng = np.random.default_rng(7)
    nt = [d.ntri for d, _ in spec.meshes]
    calls = [{0: dict(ids=range(0, nt[0]), **_vals(rng, nt[0]))}]
    ids = rng.permutation(nt[2])[:37]
    assert not np.array_equal(ids, np.sort(ids))
    calls.append({2: dict(ids=ids, **_vals(rng, 37))})
    calls.append({2: dict(ids=ids[5:20], normals=_vals(rng, 15)["normals"])})
    calls.append({2: dict(ids=range(3, 40), uv=_vals(rng, 37)["uv"])})
    calls.append({4: dict(ids=range(nt[4] - 3, nt[4]), color=_vals(rng, 3)["color"])})
    odd = _vals(rng, 2)
    odd["normals"].reshape(-1)[[0, 4, 8, 17]] = _f([0x7fc12345, 0xffa00001, 0x80000000, 0x7f800000])   # NaN payloads (quiet, signalling), -0.0, +inf
    odd["uv"].reshape(-1)[[0, 2, 5, 11]] = _f([0x7f812345, 0xff800000, 0x80000000, 0xffc00001])
    odd["color"].reshape(-1)[[3, 4, 7]] = _f([0x7fc00100, 0x80000000, 0xff800000])
    calls.append({3: dict(ids=[0, nt[3] - 1], **odd)})
    calls.append({1: dict(ids=[6, 1, 6], **_vals(rng, 3))})
    steps, cur = [], spec
    for c in calls:
        cur = with_triangle_shading(cur, c)
        steps.append((c, cur))
    return steps


@pytest.fixture(scope="module")
def spec(xrt):
    return xrt.configs.content_scene(96, 54, max_reflections=3)


@pytest.fixture(scope="module")
def steps(spec):
    return _sequence(spec)


def test_special_values_reach_the_spec_bit_for_bit(steps):
    want = _f([0x7fc12345, 0xffa00001, 0x80000000, 0x7f800000]).view(np.uint32)
    got = steps[-1][1].meshes[3][0].n[0].reshape(-1)[[0, 4, 8]].view(np.uint32)
    assert np.array_equal(got, want[:3])


def test_edits_after_the_build_are_what_save_writes(xrt, spec, steps, tmp_path):
    scene = RawScene(xrt, spec)
    before = scene.saved(tmp_path / "start.xrts")
    for k, (call, after) in enumerate(steps):
        apply_edits(xrt, scene.handle, call)
        got = scene.saved(tmp_path / "edited.xrts")
        fresh = RawScene(xrt, after)
        assert got == fresh.saved(tmp_path / "fresh.xrts"), "step %d" % k
        assert got != before, "step %d changed nothing" % k
        before = got
        fresh.close()
    # the file loads, builds, and saves itself again
    h = C.c_void_p()
    lib = xrt.abi.lib()
    assert lib.xrt_scene_load(-1, str(tmp_path / "edited.xrts").encode(), C.byref(h)) == 0
    assert lib.xrt_scene_build(h, spec.mesh_threshold, spec.scene_threshold) == 0
    assert lib.xrt_scene_save(h, str(tmp_path / "again.xrts").encode()) == 0
    lib.xrt_scene_destroy(h)
    assert (tmp_path / "again.xrts").read_bytes() == got
    scene.close()


def test_edits_before_the_build_are_what_the_build_uses(xrt, spec, steps, tmp_path):
    scene = RawScene(xrt, spec, before_build=lambda h: [apply_edits(xrt, h, c) for c, _ in steps])
    fresh = RawScene(xrt, steps[-1][1])
    assert scene.saved(tmp_path / "a.xrts") == fresh.saved(tmp_path / "b.xrts")
    # ... and edits on both sides of the build
    half = RawScene(xrt, spec, before_build=lambda h: [apply_edits(xrt, h, c) for c, _ in steps[:3]])
    for c, _ in steps[3:]:
        apply_edits(xrt, half.handle, c)
    assert half.saved(tmp_path / "c.xrts") == (tmp_path / "b.xrts").read_bytes()
    for s in (scene, fresh, half):
        s.close()


def test_error_codes_and_all_or_nothing(xrt, spec, tmp_path):
    abi, lib = xrt.abi, xrt.abi.lib()
    scene = RawScene(xrt, spec)
    nt = spec.meshes[2][0].ntri
    v = _vals(np.random.default_rng(1), 3)
    before = scene.saved(tmp_path / "before.xrts")
    E = abi.XRT_E_INVALID_ARG
    assert set_triangle_shading(xrt, scene.handle, 5, range(0, 3), **v) == E             # five meshes: ids 0 .. 4
    assert set_triangle_shading(xrt, scene.handle, -1, range(0, 3), **v) == E
    assert set_triangle_shading(xrt, scene.handle, 2, range(-1, 2), **v) == E            # first_tri < 0
    assert set_triangle_shading(xrt, scene.handle, 2, range(nt - 2, nt + 1), **v) == E   # a range past the end: its first two entries are good
    assert set_triangle_shading(xrt, scene.handle, 2, [0, 1, nt], **v) == E              # an id past the end, behind two good ones
    assert set_triangle_shading(xrt, scene.handle, 2, [0, -1, 1], **v) == E
    assert set_triangle_shading(xrt, scene.handle, 2, [0, 1, 2], first=1, **v) == E      # tri_ids with first_tri
    assert set_triangle_shading(xrt, scene.handle, 2, [0, 1, 2]) == E                    # all three arrays NULL with n > 0
    assert set_triangle_shading(xrt, scene.handle, 2, range(0, 3)) == E
    one = np.zeros(12, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert lib.xrt_scene_set_triangle_shading(scene.handle, 2, None, 0, -1, one, None, None) == E
    assert lib.xrt_scene_set_triangle_shading(None, 2, None, 0, 1, one, None, None) == E
    assert scene.saved(tmp_path / "after.xrts") == before                                # nothing was applied
    assert lib.xrt_scene_set_triangle_shading(scene.handle, 2, None, 0, 0, None, None, None) == abi.XRT_OK   # n == 0 does nothing
    assert lib.xrt_scene_set_triangle_shading(scene.handle, 2, None, nt, 0, one, None, None) == abi.XRT_OK
    assert scene.saved(tmp_path / "after.xrts") == before
    assert set_triangle_shading(xrt, scene.handle, 2, range(nt - 3, nt), **v) == abi.XRT_OK                  # (the last three do change it)
    assert scene.saved(tmp_path / "after.xrts") != before
    # the device form has no device here
    assert lib.xrt_scene_set_triangle_shading_device(scene.handle, 2, None, 0, 1, None, None, None, None) == abi.XRT_E_NO_DEVICE
    scene.close()


def test_edits_survive_set_bodies_with_a_new_mesh(xrt, spec, steps, tmp_path):
    import bodies_py
    scene = RawScene(xrt, spec)
    for c, _ in steps:
        apply_edits(xrt, scene.handle, c)
    crate = (xrt.fixtures.crate(1), xrt.configs.material(0.5))
    grown = bodies_py.edited(steps[-1][1], meshes=[crate], objects=list(spec.objects) + [([5], (0.0, 9.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    rc, built = bodies_py.set_bodies(xrt, scene.handle, grown, n_known=5)
    assert (rc, built) == (0, 1), xrt.abi.lib().xrt_last_error()
    fresh = RawScene(xrt, grown)
    assert scene.saved(tmp_path / "a.xrts") == fresh.saved(tmp_path / "b.xrts")
    # ... and the new mesh can be edited
    call = {5: dict(ids=[11, 0], **_vals(np.random.default_rng(3), 2))}
    apply_edits(xrt, scene.handle, call)
    again = RawScene(xrt, with_triangle_shading(grown, call))
    assert scene.saved(tmp_path / "a.xrts") == again.saved(tmp_path / "b.xrts")
    for s in (scene, fresh, again):
        s.close()


def test_the_mirror_keeps_meshdata_in_step(xrt, spec, steps, tmp_path):
    from triangles_py import push
    mine = copy.copy(spec)   # (the mirror edits the MeshData it was given: this test brings its own)
    mine.meshes = [(copy.deepcopy(d), m) for d, m in spec.meshes]
    scene, _ = xrt.configs.build_product(mine, device=-1)
    for call, _ in steps:
        push(scene, call)
    final = steps[-1][1]
    for m, (want, _) in enumerate(final.meshes):
        have = scene.meshes[m].data
        assert have is mine.meshes[m][0]
        for field in ("n", "uv", "color"):
            assert np.array_equal(getattr(have, field).view(np.uint32), getattr(want, field).view(np.uint32)), (m, field)
    scene.Save(tmp_path / "a.xrts")
    xrt.configs.build_product(final, device=-1)[0].Save(tmp_path / "b.xrts")
    assert (tmp_path / "a.xrts").read_bytes() == (tmp_path / "b.xrts").read_bytes()
    # a from-scratch Build() of the mirror (another mesh threshold: a new library scene) reads the mirror's arrays
    scene.meshItemTreshold += 1
    handle = scene.handle.value
    scene.Build()
    assert scene.handle.value != handle
    scene.Save(tmp_path / "c.xrts")
    assert (tmp_path / "c.xrts").read_bytes() == (tmp_path / "b.xrts").read_bytes()
    with pytest.raises(ValueError):
        scene.SetTriangleShading(2, range(0, 4, 2), color=np.zeros((2, 4)))
    with pytest.raises(ValueError):
        scene.SetTriangleShading(2, [0, 1], color=np.zeros((3, 4)))


def test_host_program_under_the_sanitizers():
    """tests/triangles/host_triangles.cpp, host code under ASan and UBSan, a program of its own (nothing is preloaded, no GPU)."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "hostcheck_triangles"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(CSRC, "hostcheck_triangles")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0 and "host_triangles: ok" in p.stdout, p.stdout + p.stderr
