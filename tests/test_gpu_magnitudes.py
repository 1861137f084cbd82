"""Parity across magnitudes on the MI355X: the cells of tests/magnitudes.py -- scenes scaled by 2^k, ray directions of length 2^j, on
both sides of the guard of every shortcut of the hot path (DESIGN.md §3 "Range of validity") -- through the kernels, bit for bit against the
CPU oracle: hits at the scene seam and the mesh seam in three builds (per-lane kernel, packet kernel, packet kernel with every ray's normal
boxes), the counting pass, secondary rays, frames, CastRays on unnormalised rays and k_pose.  What only the device can get wrong is here:
binary32 subnormals, v_rcp_f32, the sqrtf and division expansions, the restatements of packet.hip, k_pose's eigenvalue.  A cell that fails
here and passes in tests/test_magnitudes_cpu.py is a fault of the device-only code."""
import ctypes as C
import functools

import numpy as np
import pytest

import castray_py
import poses_py
from magnitudes import (CELLS, FLOOR, FRAME_FLOOR, FRAMES, POSES, SECONDARY, cell_floors, cell_id, cell_spec_and_rays, frame_id, oracle_frame, oracle_of,
                        pose_floors, pose_id, secondary_case, secondary_id)
from util import hits_equal, magnitude_frame_spec, magnitude_pose_case, scaled_rays

pytestmark = pytest.mark.gpu

BUILDS = {"default": {}, "packet": {"XRT_PACKET": "31"}, "packet_cull2": {"XRT_PACKET": "31", "XRT_NODE_CULL": "2"}}
WORK = ("node_tests", "leaf_refs", "tri_tests", "mesh_aabb_tests")
FRAME_COUNTS = ("rays_closest", "rays_shadow", "hits_shadow", "shaded_hits")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def product(xrt, monkeypatch, spec, build):
    """The scene and tracer of spec under a build's switches (xrt_scene_create reads them)."""
    for k, v in BUILDS[build].items():
        monkeypatch.setenv(k, v)
    return xrt.configs.build_product(spec)


def mesh_octree(scene, spec):
    """MESH:27-32: the mesh's own octree, with the scene's leaf threshold (the oracle's mesh tree has it)."""
    mesh = scene.meshes[0]
    mesh.Init()
    if mesh.Octree.itemTreshold != spec.mesh_threshold:
        mesh.Octree.itemTreshold = spec.mesh_threshold
        mesh.Octree.Build()
    return mesh.Octree


@functools.lru_cache(maxsize=None)
def wanted(xrt, orc, cell):
    """The oracle's answers of a cell, computed once: (hits, work counters) at the scene seam -- None where that seam is dead -- and the hits at
    the mesh seam."""
    spec, rays = cell_spec_and_rays(xrt, cell)
    o = oracle_of(xrt, orc, cell[0], cell[1])
    return (o.intersect(rays, stats=True) if cell[4] is not None else None), o.mesh_intersect(0, rays)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_hits(xrt, orc, monkeypatch, cell, build):
    """scene.IntersectBatch and mesh.Octree.IntersectBatch of the cell's 4000 rays are the oracle's, and the oracle alone reaches the floors."""
    spec, rays = cell_spec_and_rays(xrt, cell)
    want_scene, want_mesh = wanted(xrt, orc, cell)
    floor_scene, floor_mesh = cell_floors(cell)
    scene, tracer = product(xrt, monkeypatch, spec, build)
    if want_scene is not None:
        assert int(want_scene[0]["hit"].sum()) >= floor_scene
        assert hits_equal(want_scene[0], scene.IntersectBatch(rays)) == {}
    assert int(want_mesh["hit"].sum()) >= floor_mesh
    assert hits_equal(want_mesh, mesh_octree(scene, spec).IntersectBatch(rays)) == {}


def packets_split(xrt, handle):
    """xrt_split_stats: the packets of the packet kernel that handed subtrees over on the scene's device since the last call (0 unless that kernel
    ran with split walks)."""
    out = (C.c_uint64 * 4)()
    xrt.abi.check(xrt.abi.lib().xrt_split_stats(handle, out, 1))
    return int(out[2])


@pytest.mark.parametrize("name", ["soup", "hf"])
def test_the_packet_builds_run_the_packet_kernel(xrt, orc, monkeypatch, name):
    """XRT_PACKET=31 asks for the packet kernel, and the library answers with the per-lane kernel where a tree is too deep for it or a mesh root is a
    leaf.  Not for these fixtures: with split walks on and a zero budget (every packet with pending subtrees hands some over, xrt_split_stats counts
    them) batches at both seams and a frame report split packets; the default build reports none.  Same answers."""
    cell = next(c for c in CELLS if c[:4] == (name, 0, 0, False))
    spec, rays = cell_spec_and_rays(xrt, cell)
    want_scene, want_mesh = wanted(xrt, orc, cell)
    fspec, o_rgba, _, _ = oracle_frame(xrt, orc, name, 10)
    for build in ("default", "packet"):
        if build == "packet":
            for k, v in {"XRT_PK_SPLIT": "1", "XRT_PK_BUDGET": "0", "XRT_PK_BUDGET_ITEM": "0"}.items():
                monkeypatch.setenv(k, v)
        scene, tracer = product(xrt, monkeypatch, spec, build)
        octree = mesh_octree(scene, spec)
        fscene, ftracer = xrt.configs.build_product(fspec)
        packets_split(xrt, scene.handle)   # (the counters are the device's: read, and thereby reset, after every step)
        assert hits_equal(want_scene[0], scene.IntersectBatch(rays)) == {}
        counts = [packets_split(xrt, scene.handle)]
        assert hits_equal(want_mesh, octree.IntersectBatch(rays)) == {}
        counts.append(packets_split(xrt, octree._scene.handle))
        assert np.array_equal(ftracer.Render(), o_rgba)
        counts.append(packets_split(xrt, fscene.handle))
        print("%s %s: split packets of the scene batch, the mesh batch, the frame: %r" % (name, build, counts))
        if build == "default":
            assert counts == [0, 0, 0]
        else:
            assert min(counts) > 0, counts


STATS_CELLS = [c for c in CELLS if c[0] == "soup" and not c[3] and (c[1], c[2]) in ((-40, 0), (-31, 0), (31, 19), (0, 64))]


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("cell", STATS_CELLS, ids=cell_id)
def test_counting_pass(xrt, orc, monkeypatch, cell, build):
    """k_count at magnitude: the reference's work counters of the cell's rays."""
    assert len(STATS_CELLS) == 4
    spec, rays = cell_spec_and_rays(xrt, cell)
    want, want_st = wanted(xrt, orc, cell)[0]
    scene, tracer = product(xrt, monkeypatch, spec, build)
    hits, st = scene.IntersectBatch(rays, stats=True)
    assert hits_equal(want, hits) == {}
    assert want_st["tri_tests"] > 0
    for k in WORK:
        assert st[k] == want_st[k], (k, st[k], want_st[k])


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("case", SECONDARY, ids=secondary_id)
def test_secondary_rays(xrt, orc, monkeypatch, case, build):
    """Origins on the surface and an ignore triangle: where the normal boxes and "answered at emission" decide."""
    spec, rays, floor = secondary_case(xrt, orc, case)
    want = oracle_of(xrt, orc, case[0], case[1]).intersect(rays)
    assert len(rays) >= FLOOR and int(want["hit"].sum()) >= floor
    scene, tracer = product(xrt, monkeypatch, spec, build)
    assert hits_equal(want, scene.IntersectBatch(rays)) == {}


def frames_equal(tracer, o_rgba, o_rgbf, o_st, what):
    tracer.collect_stats = True
    rgba, rgbf = tracer.Render(want_float=True)
    bad = int((rgba != o_rgba).sum())
    assert bad == 0, "%s: %d of %d RGBA8 pixels differ" % (what, bad, rgba.size)
    assert np.array_equal(_bits(rgbf).reshape(-1), _bits(o_rgbf).reshape(-1)), what + ": fp32 colours"
    for k in FRAME_COUNTS:
        assert tracer.last_stats[k] == o_st[k], (what, k, tracer.last_stats[k], o_st[k])


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("case", FRAMES, ids=frame_id)
def test_frames(xrt, orc, monkeypatch, case, build):
    """48 x 48 frames of the scaled scenes (MaxReflections 2; the soup also as glass of index 1.32): RGBA8, the fp32 colours and the ray accounting."""
    spec, o_rgba, o_rgbf, o_st = oracle_frame(xrt, orc, *case)
    assert o_st["shaded_hits"] >= FRAME_FLOOR
    scene, tracer = product(xrt, monkeypatch, spec, build)
    frames_equal(tracer, o_rgba, o_rgbf, o_st, frame_id(case))


@pytest.mark.parametrize("k", [-40, 10])
@pytest.mark.parametrize("mode", ["fixed16", "adaptive1"])
@pytest.mark.parametrize("name", ["soup", "hf"])
def test_supersampled_frames(xrt, orc, name, mode, k):
    ms, q = (xrt.abi.MS_FIXED16, 0) if mode == "fixed16" else (xrt.abi.MS_ADAPTIVE, 1)
    spec, o_rgba, _, o_st = oracle_frame(xrt, orc, name, k, False, ms, q)
    assert o_st["shaded_hits"] >= FRAME_FLOOR
    scene, tracer = xrt.configs.build_product(spec)
    rgba = tracer.Render()
    assert np.array_equal(rgba, o_rgba), "%d of %d RGBA8 pixels differ" % (int((rgba != o_rgba).sum()), rgba.size)


@pytest.mark.parametrize("j", [-19, 19, 40])
@pytest.mark.parametrize("k", [0, -40])
def test_cast_rays_on_unnormalised_rays(xrt, k, j):
    """RT:506 never normalises the caller's ray: the camera rays of the soup scene with directions x 2^j through xrt_cast_rays against the
    checker (tests/castray), colours and colour vectors."""
    spec = magnitude_frame_spec(xrt, "soup", k)
    cs = castray_py.CastRayScene(spec)
    rays = scaled_rays(cs.primary_rays(), 0, j)
    o_rgba, o_rgbf, o_st = cs.cast_rays(rays)
    assert o_st["hits_closest"] >= FLOOR
    scene, tracer = xrt.configs.build_product(spec)
    rgba, rgbf = tracer.CastRays(rays, want_float=True)
    bad = int((rgba != o_rgba).sum())
    assert bad == 0, "%d of %d colours differ" % (bad, len(rays))
    assert np.array_equal(_bits(rgbf), _bits(o_rgbf))
    for key in ("rays_closest", "rays_shadow", "hits_closest", "shaded_hits"):
        assert tracer.last_stats[key] == o_st[key], (key, tracer.last_stats[key], o_st[key])


@pytest.mark.filterwarnings("ignore::RuntimeWarning")   # (the inverse of a singular world matrix: infinities and NaNs, as in the reference)
@pytest.mark.parametrize("case", POSES, ids=pose_id)
def test_poses(xrt, case):
    """k_pose at magnitude: body 0 turned and scaled through the SceneObject setters (xrt_scene_set_poses), queried with the stale scene octree
    against the checker with the same pose, then after scene.Build() (xrt_scene_build_tree) against the checker's rebuilt tree and a fresh scene
    built with those poses."""
    spec, pose0, rays0, rays1 = magnitude_pose_case(xrt, case[0], case[1])
    scene, tracer = xrt.configs.build_product(spec)
    ref = poses_py.PoseOracle(spec)
    scene.Bodies[0].Rotation, scene.Bodies[0].Scale = pose0[1], pose0[2]
    ref.set_pose(0, *pose0)
    floors = pose_floors(case)
    for i, tree in enumerate(("stale", "built")):
        if tree == "built":
            scene.Build()
            ref.build_tree()
            fresh, _ = xrt.configs.build_product(poses_py.moved(spec, {0: pose0}))
        for b, rays in enumerate((rays0, rays1)):
            want = ref.intersect(rays)
            assert int(want["hit"].sum()) >= floors[2 * i + b], (tree, b, int(want["hit"].sum()))
            msg = poses_py.hits_equal(want, scene.IntersectBatch(rays))
            assert msg is None, "%s tree, body %d: %s" % (tree, b, msg)
            if tree == "built":
                msg = poses_py.hits_equal(want, fresh.IntersectBatch(rays))
                assert msg is None, "fresh scene, body %d: %s" % (b, msg)
