"""The mesh-level test "every triangle faces away from this ray" bounds the normals in a diagonal frame as well as in their axis-aligned box (traverse.h
mesh_faces_away): k_shade answers more reflections and shadow rays at emission, the walks skip more meshes.  Nothing a caller can see
may change: every frame here -- 96 x 54 pixels, 16 sub-rays per pixel, MaxReflections 3 -- is compared bit for bit with the oracle.

Which rays the device answered shows in the frame's end counts (xrt_debug_end_counts, tests/test_gpu_end_early.py): the paths left on k_compose's list are
the generation-0 hits that emitted a shadow ray or a reflection.  The test computes that number from the ORACLE's generation-0 hits with the host build of
the very function the kernels call (tests/normal_diag_py.py: scene_host.cpp's mesh record, traverse.h mesh_faces_away, the object-space direction formed as
shade_math.h faces_away_single forms it), which tests/test_normal_diag_cpu.py proves sound; the two numbers must be equal.

The sub-rays of a pixel are the oracle's primary rays of a viewport 8 times as wide and high, moved by 4: sub-sample offsets are odd multiples of 1/8, so
pixel 8 x + 4 + k of that viewport is screen position x + k / 8 of the frame's, with (sx - vp_x) / vp_width the same quotient bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest

import normal_diag_py

pytestmark = pytest.mark.gpu

W, H = 96, 54
SLOTS = ((W + 63) // 64) * ((H + 7) // 8) * 512


def base_spec(xrt, name, mesh, obj, cam, light, threshold=50):
    s = xrt.configs.SceneSpec(name)
    s.meshes.append((mesh, xrt.configs.material(0.3)))
    s.objects.append(obj)
    s.camera = xrt.configs.camera(*cam)
    s.lights = [xrt.configs.spot(light)]
    s.max_reflections = 3
    s.multisampling = xrt.abi.MS_FIXED16
    s.multisample_quality = 1
    s.mesh_threshold = threshold
    return s.with_size(W, H)


def turned(xrt, mesh, up):
    """`mesh` turned so that +y goes to `up` (evaluated in double, rounded once per coordinate; normals, uv and colours recomputed or kept)"""
    Y = np.array(up, dtype=np.float64) / np.linalg.norm(up)
    X = np.cross([0.0, 1.0, 0.0], Y) if abs(Y[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    X = X / np.linalg.norm(X)
    Z = np.cross(X, Y)
    v = mesh.v.astype(np.float64)
    v = (v[..., 0:1] * X + v[..., 1:2] * Y + v[..., 2:3] * Z).astype(np.float32)
    sn = xrt.fixtures.surface_normals(np.ascontiguousarray(v))
    return xrt.fixtures.MeshData(v, np.repeat(sn[:, None, :], 3, axis=1), mesh.uv, mesh.color)


def ground(xrt, y=-30.0, half=400.0):
    """two triangles facing up"""
    a, b, c, d = (-half, y, -half), (half, y, -half), (half, y, half), (-half, y, half)
    v = np.array([(a, b, c), (a, c, d)], dtype=np.float32)
    sn = xrt.fixtures.surface_normals(v)
    assert (sn[:, 1] > 0.99).all()
    return xrt.fixtures.MeshData(v, np.repeat(sn[:, None, :], 3, axis=1), np.zeros((2, 3, 2), dtype=np.float32), np.ones((2, 4), dtype=np.float32))


def sub_rays(xrt, orc, spec):
    """the 16 W H generation-0 rays of the frame (see the module's docstring), in no particular order"""
    big = copy.deepcopy(spec).with_size(8 * W, 8 * H)
    cam = orc.camera_abi(big)
    cam.vp_x, cam.vp_y = 4, 4
    rays = np.zeros(64 * W * H, dtype=xrt.RAY_DTYPE)
    assert orc.lib().orc_generate_primary_rays(C.byref(cam), rays.ctypes.data) == 0
    return np.ascontiguousarray(rays.reshape(8 * H, 8 * W)[1::2, 1::2]).reshape(-1)


def expected_listed(xrt, orc, spec):
    """(hits of generation 0, those among them that emit a shadow ray or a reflection, the mesh record's axis, can-face-away) by the host copy of the test"""
    o = orc.OracleScene(spec)
    rays = sub_rays(xrt, orc, spec)
    hits = o.intersect(rays)
    hit = hits["hit"] != 0
    assert (hits["mesh"][hit] == 0).all()
    mesh = spec.meshes[0][0]
    ids, pos, rot, scale = spec.objects[0]
    _, inv, _ = xrt.xna.build_world(scale, rot, pos, np.zeros(6, dtype=np.float32))
    inv = xrt.xna.as_array(inv)
    w, d, n = hits["w"][hit], rays["d"][hit], mesh.surface_normal[hits["tri"][hit]]
    refl, axis, can = normal_diag_py.answers(mesh.v, spec.mesh_threshold, inv, "hits", np.concatenate([w, d, n], axis=1))
    emits = ~refl
    for l in spec.lights:
        lp = np.broadcast_to(np.array(l["position"], dtype=np.float32), w.shape)
        shadow, _, _ = normal_diag_py.answers(mesh.v, spec.mesh_threshold, inv, "light", np.concatenate([w, lp], axis=1))
        emits |= ~shadow
    return int(hit.sum()), int(emits.sum()), int((~refl).sum()), axis, can


def frame(xrt, orc, spec):
    """the product's frame against the oracle's, bit for bit; returns the end counts"""
    o_rgba, _, o_st = orc.OracleScene(spec).render(nthreads=8, want_float=False)
    scene, tracer = xrt.configs.build_product(copy.deepcopy(spec))
    rgba = tracer.Render().copy()
    assert np.array_equal(rgba, o_rgba), "%s: %d RGBA8 pixels differ from the oracle" % (spec.name, int((rgba != o_rgba).sum()))
    for k in ("rays_closest", "rays_shadow", "shaded_hits", "pixels"):
        assert tracer.last_stats[k] == o_st[k], (spec.name, k, tracer.last_stats[k], o_st[k])
    return scene.EndCounts()


def pinned(xrt, orc, spec, want_axis):
    h0, listed, traced, axis, can = expected_listed(xrt, orc, spec)
    counts = frame(xrt, orc, spec)
    print(spec.name, "generation-0 hits", h0, "reflections not answered", traced, "listed (expected)", listed, "end counts", counts, "axis", axis)
    assert can and (axis == want_axis if want_axis else axis in (1, 2, 3)), (axis, can)
    assert sum(counts) == SLOTS * 16
    assert h0 > 10000 and 0 < traced < h0       # the test answers, and not everything
    assert counts[2] == listed, (counts, listed)
    return h0, traced


def test_heightfield_benchmark_camera(xrt, orc):
    """The benchmark's scene in small: the 64 x 64-quad terrain, camera (0, 60, 110) -> origin, spot light at (0, 120, 160)."""
    spec = base_spec(xrt, "heightfield_m64", xrt.fixtures.heightfield(64), ([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0, 60, 110), (0, 0, 0)), (0, 120, 160))
    h0, traced = pinned(xrt, orc, spec, 2)
    assert traced < 0.26 * h0   # (the axis-aligned box alone leaves about 30 % of this view's reflections to be traced, tests/test_normal_diag_cpu.py; both bounds about 21 %)


def test_heightfield_turned_and_scaled_body(xrt, orc):
    """The same mesh in a body turned about x and z and scaled unevenly: object space is not world space, the test runs on the object-space direction."""
    spec = base_spec(xrt, "heightfield_m64_turned", xrt.fixtures.heightfield(64), ([0], (3.0, -2.0, 5.0), (0.3, 0.0, 0.45), (1.3, 0.8, 1.1)), ((0, 60, 110), (0, 0, 0)), (0, 120, 160))
    pinned(xrt, orc, spec, 2)


def test_cone_about_111(xrt, orc):
    """Normals in a cone about (1, 1, 1): every axis interval excludes 0, the box is loose, the diagonal box answers more.  One body: the counts are pinned."""
    mesh = turned(xrt, xrt.fixtures.heightfield(64), (1.0, 1.0, 1.0))
    spec = base_spec(xrt, "cone111", mesh, ([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((115, 30, -55), (0, 0, 0)), (90, 140, 40))
    pinned(xrt, orc, spec, None)


def test_cone_about_111_over_a_ground_plane(xrt, orc):
    """... and over a ground plane, a second body: the frame takes the two-level walk, which asks the same question per mesh (packet.hip); nothing is answered at
    emission, nothing ends early."""
    mesh = turned(xrt, xrt.fixtures.heightfield(64), (1.0, 1.0, 1.0))
    spec = base_spec(xrt, "cone111_ground", mesh, ([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((115, 30, -55), (0, 0, 0)), (90, 140, 40))
    spec.meshes.append((ground(xrt), xrt.configs.material(0.4)))
    spec.objects.append(([1], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    assert frame(xrt, orc, spec) == (0, 0, 0)


def test_crate_takes_the_old_path(xrt, orc):
    """A crate has normals of every direction: neither box excludes the origin, nothing is answered at emission (the frame plan decides it from both boxes)."""
    spec = base_spec(xrt, "crate_n7", xrt.fixtures.crate(7), ([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0, 32, 64), (0, 8, 0)), (0, 40, 60))
    _, axis, can = normal_diag_py.answers(spec.meshes[0][0].v, spec.mesh_threshold, np.eye(4, dtype=np.float32), "rays", np.zeros((0, 6), dtype=np.float32))
    assert (axis, can) == (0, False)
    assert frame(xrt, orc, spec) == (0, 0, 0)
