"""xrt_scene_set_mesh_triangles on the MI355X: frames, seam-1 answers and ray batches of scenes one of whose meshes takes new triangles
between frames, bit for bit (RGBA8 words, the uint32 view of the fp32 colour vectors, every hit field) against the oracle of the replaced
spec.  Every replacement lies in the box of the mesh the scene was built with (mesh_edit_py.fitted): the bodies' boxes, which the call does
not touch, are then those of the replaced spec."""
import numpy as np
import pytest

import bodies_py
import tree_shapes
from bodies_py import edited, hits_equal
from materials_py import with_materials
from mesh_edit_py import TriArgs, empty_mesh, fitted, moved_vertices, replaced, shading_values
from poses_py import PoseOracle, pose_arrays
from triangles_py import with_triangle_shading

pytestmark = pytest.mark.gpu
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
LEAF_RUN_MIN = 16   # xrt_core.h XRT_LEAF_RUN_MIN


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle(orc, spec):
    rgba, rgbf, _ = orc.OracleScene(spec).render(nthreads=16)
    return rgba, rgbf


def frame_equal(got_rgba, got_f, want, what):
    rgba, rgbf = want
    bad = int((np.asarray(got_rgba).reshape(-1) != rgba).sum())
    assert bad == 0, "%s: %d of %d pixels differ" % (what, bad, rgba.size)
    if got_f is not None and rgbf is not None:
        assert np.array_equal(_bits(got_f).reshape(-1), _bits(rgbf).reshape(-1)), what


def render(tracer):
    rgba, rgbf = tracer.Render(want_float=True)
    return rgba.copy(), rgbf.copy()


def check_frame(orc, tracer, spec, what):
    got = render(tracer)
    frame_equal(*got, oracle(orc, spec), what + " vs the oracle")
    return got


def depth_and_leaf(scene, mesh_id=0):
    nodes, _ = scene.tree(scene.meshes[mesh_id])
    return int(nodes["depth"].max()), int(nodes["count"][nodes["is_leaf"] != 0].max())


@pytest.mark.parametrize("multisampling", ["plain", "fixed16"])
def test_grid(xrt, orc, multisampling):
    """The mirror's way: mesh.Triangles = ..; mesh.Init(); the next frame shows the new mesh in all nine bodies."""
    spec = xrt.configs.crate_grid_scene(96, 54, n=3, grid=3)
    spec.scene_threshold = 2
    if multisampling == "fixed16":
        spec.multisampling, spec.multisample_quality = xrt.abi.MS_FIXED16, 1
    scene, tracer = xrt.configs.build_product(spec)
    handle = scene.handle.value
    last = render(tracer)
    crate = spec.meshes[0][0]
    rays = np.concatenate([tracer.GeneratePrimaryRays()[::5], bodies_py.random_rays(xrt, 4096, 3)])[:4096]
    now = spec
    for what, data in (("the sphere", fitted(xrt, bodies_py.sphere_mesh(xrt), crate.bbox)), ("the crate with moved vertices", moved_vertices(xrt, crate, 4, amount=0.05))):
        scene.meshes[0].Triangles = data
        scene.meshes[0].Init()
        now = replaced(now, 0, data)
        got = check_frame(orc, tracer, now, what)
        assert scene.handle.value == handle and scene.last_build_meshes == 1
        assert not np.array_equal(got[0], last[0]), what
        last = got
        ref = PoseOracle(now)
        msg = hits_equal(scene.IntersectBatch(rays), ref.intersect(rays))
        assert msg is None, "%s: %s" % (what, msg)
        ms, tracer.UseMultisampling = tracer.UseMultisampling, False    # (CastRay is one ray, one colour)
        rgba, rgbf = tracer.CastRays(rays, want_float=True)
        tracer.UseMultisampling = ms
        ref.spec = edited(now)
        ref.spec.multisampling = xrt.abi.MS_OFF
        o_rgba, o_rgbf = ref.cast_rays(rays)
        assert np.array_equal(rgba, o_rgba), what
        assert np.array_equal(_bits(rgbf), _bits(o_rgbf)), what


@pytest.mark.parametrize("multisampling", ["plain", "fixed16"])
def test_modes_and_stack_on_one_scene(xrt, orc, multisampling):
    """One body.  crate(1), a single leaf (the one-body walk of a mesh without an octree) -> heightfield(32): a real octree, the packet kernel,
    leaves stored in runs (mesh threshold 16) -> the heightfield deformed -> a staircase of depth 7: 9 stack words, the 12-word instantiation
    of k_intersect where the others take the 8-word one -> crate(1) again.  The scene's first frame was a larger one."""
    spec = xrt.configs.crate_scene(64, 36, max_reflections=2)
    spec.mesh_threshold = 16
    if multisampling == "fixed16":
        spec.multisampling, spec.multisample_quality = xrt.abi.MS_FIXED16, 1
    scene, tracer = xrt.configs.build_product(spec)
    tracer.CurrentTarget = xrt.api.RenderTarget(256, 144)     # work buffers and hints of a bigger frame meet the smaller scenes
    tracer.Render()
    tracer.CurrentTarget = xrt.api.RenderTarget(64, 36)
    single = check_frame(orc, tracer, spec, "one crate")
    assert depth_and_leaf(scene) == (0, 12)
    box = spec.meshes[0][0].bbox
    terrain = fitted(xrt, xrt.fixtures.heightfield(32), box)
    steps = (("a heightfield", terrain, lambda d, l: 0 < d <= 6 and l >= LEAF_RUN_MIN), ("the heightfield deformed", moved_vertices(xrt, terrain, 9, amount=0.01), lambda d, l: 0 < d <= 6),
             ("a staircase of depth 7", fitted(xrt, tree_shapes.staircase(xrt, 7, 16), box), lambda d, l: d == 7), ("the crate again", spec.meshes[0][0], lambda d, l: (d, l) == (0, 12)))
    rays = np.concatenate([tracer.GeneratePrimaryRays(), bodies_py.random_rays(xrt, 1500, 8, spread=60.0, aim=12.0)])
    last = single
    for what, data, shape_ok in steps:
        scene.SetMeshTriangles(0, data)
        now = replaced(spec, 0, data)
        assert shape_ok(*depth_and_leaf(scene)), (what, depth_and_leaf(scene))
        got = check_frame(orc, tracer, now, what)
        assert not np.array_equal(got[0], last[0]), what
        last = got
        msg = hits_equal(scene.IntersectBatch(rays), orc.OracleScene(now).intersect(rays))
        assert msg is None, "%s: %s" % (what, msg)
    frame_equal(*last, single, "the crate again vs the first frame")


def test_what_survives(xrt, orc):
    """Poses and triangle values set from device arrays, and a material set before, survive the call; the triangle values of the replaced
    mesh itself are what the call gives; a Transparent material on the replaced mesh keeps the frame on the ray-tree pipeline."""
    import torch
    spec = xrt.configs.SceneSpec("survivors")
    mat = xrt.configs.material
    spec.meshes = [(xrt.fixtures.crate(3), mat(0.4, transparent=True, refraction_index=float(np.float32(1.32)))), (bodies_py.sphere_mesh(xrt), mat(0.7, interpolate_normals=True))]
    spec.objects = [([0], (-14.0, 0.0, 0.0), ZERO, ONE), ([1], (16.0, 10.0, -6.0), ZERO, (5.0, 5.0, 5.0)), ([0], (0.0, 0.0, -50.0), (0.0, 0.4, 0.0), ONE)]
    spec.camera = xrt.configs.camera((0, 32, 80), (0, 8, 0))
    spec.lights = [xrt.configs.spot((0, 40, 60))]
    spec.max_reflections = 3
    spec.with_size(64, 36)
    scene, tracer = xrt.configs.build_product(spec)
    first = check_frame(orc, tracer, spec, "as built")
    # a material on the other mesh, by the host
    changed = with_materials(spec, {1: dict(reflectiveness=0.2)})
    scene.meshes[1].MeshMaterial.Reflectiveness = 0.2
    # poses of bodies 0 (names the mesh to be replaced) and 1 from device arrays
    moves = {0: ((-12.0, 3.0, 6.0), (0.0, 0.5, 0.0), ONE), 1: ((14.0, 12.0, -4.0), (0.3, 0.0, 0.0), (5.0, 5.0, 5.0))}
    ids = sorted(moves)
    w, iw, bb = zip(*(pose_arrays(spec, b, *moves[b]) for b in ids))
    t = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda").contiguous()
    scene._push_materials()
    scene.SetPosesDevice(t(ids, torch.int32), t(np.concatenate(w)), t(np.concatenate(iw)), t(np.concatenate(bb)))
    # triangle values from device arrays: of the other mesh (they stay) and of the mesh to be replaced (they go)
    n1, uv1, c1, _ = shading_values(spec.meshes[1][0], 100, 300, 21)
    n0, uv0, c0, _ = shading_values(spec.meshes[0][0], 0, 60, 22)
    scene.SetTriangleShadingDevice(1, range(100, 400), t(n1), t(uv1), t(c1))
    scene.SetTriangleShadingDevice(0, range(0, 60), t(n0), t(uv0), t(c0))
    torch.cuda.synchronize()

    def reference(s):
        ref = PoseOracle(s)
        for b in ids:
            ref.set_pose(b, *moves[b])
        return ref.render()
    shaded = with_triangle_shading(changed, {1: dict(ids=range(100, 400), normals=n1, uv=uv1, color=c1)})
    before = render(tracer)
    frame_equal(*before, reference(with_triangle_shading(shaded, {0: dict(ids=range(0, 60), normals=n0, uv=uv0, color=c0)})), "before the replacement")
    assert not np.array_equal(before[0], first[0])
    data = fitted(xrt, xrt.fixtures.heightfield(32), spec.meshes[0][0].bbox)
    assert xrt.abi.lib().xrt_scene_set_mesh_triangles(scene.handle, 0, *TriArgs(data).args()) == 0   # (the C-ABI alone: the mirror's arrays stay behind)
    got = render(tracer)
    frame_equal(*got, reference(replaced(shaded, 0, data)), "after the replacement")
    assert not np.array_equal(got[0], before[0])
    tracer.collect_stats = True
    tracer.Render()
    assert tracer.last_stats["rays_closest"] > spec.width * spec.height    # (the glass splits rays: a ray tree, not a chain)


def test_busy_while_a_ticket_is_open(xrt, orc):
    spec = xrt.configs.crate_grid_scene(64, 36, n=3, grid=3)
    spec.scene_threshold = 2
    scene, tracer = xrt.configs.build_product(spec)
    data = fitted(xrt, bodies_py.sphere_mesh(xrt), spec.meshes[0][0].bbox)
    args = TriArgs(data)
    lib, abi = xrt.abi.lib(), xrt.abi
    host = np.zeros(spec.width * spec.height, dtype=np.uint32)
    fr = tracer.PrepareHost(host)
    t = fr.begin()
    assert lib.xrt_scene_set_mesh_triangles(scene.handle, 0, *args.args()) == abi.XRT_E_BUSY
    fr.end(t)
    frame_equal(host, None, oracle(orc, spec), "the frame in flight during the refused call")
    assert lib.xrt_scene_set_mesh_triangles(scene.handle, 0, *args.args()) == abi.XRT_OK
    t = fr.begin()
    fr.end(t)
    frame_equal(host, None, oracle(orc, replaced(spec, 0, data)), "the frame after the call")


def test_empty_and_back(xrt, orc):
    spec = xrt.configs.crate_scene(64, 36, max_reflections=2)
    scene, tracer = xrt.configs.build_product(spec)
    full = check_frame(orc, tracer, spec, "the crate")
    rays = tracer.GeneratePrimaryRays()
    none = empty_mesh(xrt, spec.meshes[0][0].bbox)
    scene.SetMeshTriangles(0, none)
    got = check_frame(orc, tracer, replaced(spec, 0, none), "no triangles")
    frame_equal(*got, oracle(orc, edited(spec, objects=[])), "no triangles vs the frame of the empty list")
    assert len(np.unique(got[0])) == 1                                  # the background
    assert not scene.IntersectBatch(rays)["hit"].any()
    scene.SetMeshTriangles(0, spec.meshes[0][0])
    frame_equal(*check_frame(orc, tracer, spec, "the crate again"), full, "the crate again vs the first frame")
    msg = hits_equal(scene.IntersectBatch(rays), orc.OracleScene(spec).intersect(rays))
    assert msg is None, msg


def test_two_gpus_after_a_replacement(xrt, orc, monkeypatch):
    """n_gpus = 2 under the switch tests/test_gpu_parity.py::test_in_library_multi_gpu uses (XRT_FAKE_GPUS=1: both replicas on the one
    device): the replicas of the old triangles are dropped, the frame after the call equals the one-GPU frame and the oracle's."""
    monkeypatch.setenv("XRT_FAKE_GPUS", "1")
    spec = xrt.configs.crate_grid_scene(96, 54, n=3, grid=3)
    scene, tracer = xrt.configs.build_product(spec)
    tracer.NumGpus = 2
    frame_equal(tracer.Render().copy(), None, oracle(orc, spec), "two GPUs, as built")
    data = fitted(xrt, bodies_py.sphere_mesh(xrt), spec.meshes[0][0].bbox)
    scene.SetMeshTriangles(0, data)
    two = tracer.Render().copy()
    assert tracer.last_stats["pieces"] == 2
    tracer.NumGpus = 1
    one = tracer.Render().copy()
    assert np.array_equal(two, one)
    frame_equal(two, None, oracle(orc, replaced(spec, 0, data)), "two GPUs after the replacement")
