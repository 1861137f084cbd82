"""xrt_scene_set_bodies on the MI355X: frames, seam-1 answers and ray batches of scenes whose body list is edited between frames, bit for bit
(RGBA8 words, the uint32 view of the fp32 colour vectors, every hit field) against the oracle of a spec that holds the scene's meshes in id
order and the current bodies, and against a library scene made from scratch of that spec.  The edits go through the mirror's Build(), which
keeps the library scene and calls xrt_scene_set_bodies once."""
import ctypes as C

import numpy as np
import pytest

import bodies_py
from bodies_py import BodyArrays, edited, hits_equal
from materials_py import RawScene, with_materials
from poses_py import PoseOracle

pytestmark = pytest.mark.gpu
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


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


class Edited:
    """A product scene (the mirror) under edit: `meshes` are the mirror's Mesh objects in id order; apply(spec) makes the mirror's Bodies
    those of spec (new SceneObjects, new Meshes for the meshes of spec the scene has not seen) and calls Build()."""

    def __init__(self, xrt, spec):
        self.xrt = xrt
        self.scene, self.tracer = xrt.configs.build_product(spec)
        self.meshes = list(self.scene.meshes)
        self.handle = self.scene.handle.value

    def apply(self, spec, n_new):
        api = self.xrt.api
        for data, m in spec.meshes[len(self.meshes):]:
            mat = api.Material(m["reflectiveness"], m["use_texture"], m["transparent"], m["refraction_index"], m["texture"], m.get("texture_pargb"))
            mat.InterpolateNormals = m["interpolate_normals"]
            self.meshes.append(api.Mesh(data, mat))
        bodies = []
        for ids, pos, rot, scale in spec.objects:
            o = api.SceneObject([self.meshes[i] for i in ids], pos, rot)
            o.Scale = scale
            bodies.append(o)
        self.scene.Bodies[:] = bodies
        self.scene.Build()
        assert self.scene.handle.value == self.handle and self.scene.last_build_meshes == n_new
        assert [self.scene.mesh_id(m) for m in self.meshes[:len(self.scene.meshes)]] == list(range(len(self.scene.meshes)))

    def fresh_frame(self, spec):
        """The tracer's frame of a library scene made from scratch of spec: its meshes in spec's order, its bodies, one xrt_scene_build."""
        api = self.xrt.api
        raw = RawScene(self.xrt, spec, device=0)
        sm = api.OctreeSpatialManager(0)
        sm._scene = api._Scene.__new__(api._Scene)
        sm._scene.handle, raw.handle = raw.handle, C.c_void_p()
        mine = self.tracer.CurrentScene
        self.tracer.CurrentScene = sm
        try:
            return render(self.tracer)
        finally:
            self.tracer.CurrentScene = mine

    def check_frame(self, orc, spec, what):
        got = render(self.tracer)
        frame_equal(*got, oracle(orc, spec), what + " vs the oracle")
        frame_equal(*got, self.fresh_frame(spec), what + " vs a scene made from scratch")
        return got


def _sphere(xrt, **kw):
    return (bodies_py.sphere_mesh(xrt), xrt.configs.material(0.7, interpolate_normals=True, **kw))


@pytest.mark.parametrize("multisampling", ["plain", "fixed16"])
def test_grid_edits(xrt, orc, multisampling):
    spec = xrt.configs.crate_grid_scene(96, 54, n=3, grid=3)
    spec.scene_threshold = 2
    if multisampling == "fixed16":
        spec.multisampling, spec.multisample_quality = xrt.abi.MS_FIXED16, 1
    e = Edited(xrt, spec)
    b = spec.objects
    s1 = edited(spec, objects=[b[0], b[2], b[3], b[6], b[8]])
    s2 = edited(s1, objects=s1.objects[:2] + [([0], (15.0, 45.0, 10.0), (0.3, 0.9, -0.4), (1.5, 0.6, 1.0))] + s1.objects[2:] + [([0], (0.0, 0.0, 0.0), (0.0, 2.0, 0.0), ONE)])
    s3 = edited(s2, meshes=[_sphere(xrt)], objects=s2.objects[:4] + [([1], (0.0, 10.0, 70.0), ZERO, (6.0, 6.0, 6.0))] + s2.objects[4:])
    first = render(e.tracer)
    rays = np.concatenate([e.tracer.GeneratePrimaryRays(), bodies_py.random_rays(xrt, 2000, 3)])
    last = first
    for what, after, n_new in (("four bodies removed", s1, 0), ("two added at new poses", s2, 0), ("a sphere body of a new mesh", s3, 1)):
        e.apply(after, n_new)
        got = e.check_frame(orc, after, what)
        assert not np.array_equal(got[0], last[0]), what
        last = got
        ref = PoseOracle(after)
        msg = hits_equal(e.scene.IntersectBatch(rays), ref.intersect(rays))
        assert msg is None, "%s: %s" % (what, msg)
        batch = rays[::3]
        ms, e.tracer.UseMultisampling = e.tracer.UseMultisampling, False    # (CastRay is one ray, one colour)
        rgba, rgbf = e.tracer.CastRays(batch, want_float=True)
        e.tracer.UseMultisampling = ms
        ref.spec = edited(after)
        ref.spec.multisampling = xrt.abi.MS_OFF
        o_rgba, o_rgbf = ref.cast_rays(batch)
        assert np.array_equal(rgba, o_rgba), what
        assert np.array_equal(_bits(rgbf), _bits(o_rgbf)), what


@pytest.mark.parametrize("multisampling", ["plain", "fixed16"])
def test_mode_and_stack_changes_on_one_scene(xrt, orc, multisampling):
    """One crate(1) body (one body, one mesh that is a single leaf) -> a second body (two-level walk) -> a heightfield with a real octree (a
    deeper stack) -> the single crate again, all on one library scene whose first frame was a larger one."""
    spec = xrt.configs.crate_scene(64, 36, max_reflections=2)
    if multisampling == "fixed16":
        spec.multisampling, spec.multisample_quality = xrt.abi.MS_FIXED16, 1
    e = Edited(xrt, spec)
    e.tracer.CurrentTarget = xrt.api.RenderTarget(256, 144)     # work buffers and hints of a bigger frame meet the smaller scenes
    e.tracer.Render()
    e.tracer.CurrentTarget = xrt.api.RenderTarget(64, 36)
    single = e.check_frame(orc, spec, "one crate")
    two = edited(spec, objects=spec.objects + [([0], (30.0, 0.0, -20.0), (0.0, 0.6, 0.0), ONE)])
    e.apply(two, 0)
    e.check_frame(orc, two, "two crates")
    terrain = edited(two, meshes=[(xrt.fixtures.heightfield(32), xrt.configs.material(0.3))], objects=two.objects + [([1], (0.0, -6.0, 0.0), ZERO, ONE)])
    e.apply(terrain, 1)
    got = e.check_frame(orc, terrain, "two crates on a terrain")
    assert not np.array_equal(got[0], single[0])
    back = edited(terrain, objects=spec.objects)
    e.apply(back, 0)
    frame_equal(*e.check_frame(orc, back, "the single crate again"), single, "the single crate again vs the first frame")


@pytest.mark.parametrize("kind", ["crate", "terrain"])
def test_modes_go_there_and_back_on_one_scene(xrt, orc, kind):
    """One body of one mesh -> two bodies -> the one body again, the scene holding one mesh throughout: the one-body walk, its refill and
    long-ray settings and the blocks per CU are left and taken again (crate: a mesh that is one leaf), and with a heightfield that has a real
    octree the wave-packet kernel is left and taken again."""
    spec = xrt.configs.crate_scene(64, 36, max_reflections=2) if kind == "crate" else xrt.configs.heightfield_scene(64, 36, m=32)
    e = Edited(xrt, spec)
    e.tracer.collect_stats = True
    one = e.check_frame(orc, spec, "one body")
    stats = dict(e.tracer.last_stats)
    second = ([0], (30.0, 0.0, -20.0), (0.0, 0.6, 0.0), ONE) if kind == "crate" else ([0], (10.0, 25.0, -30.0), (0.2, 0.5, 0.0), (0.5, 0.5, 0.5))
    two = edited(spec, objects=spec.objects + [second])
    e.apply(two, 0)
    got = e.check_frame(orc, two, "two bodies")
    assert not np.array_equal(got[0], one[0])
    e.apply(spec, 0)
    frame_equal(*e.check_frame(orc, spec, "one body again"), one, "one body again vs the first frame")
    for k in ("rays_closest", "rays_shadow", "node_tests", "leaf_refs", "tri_tests"):
        assert e.tracer.last_stats[k] == stats[k], k
    rays = e.tracer.GeneratePrimaryRays()
    msg = hits_equal(e.scene.IntersectBatch(rays), orc.OracleScene(spec).intersect(rays))
    assert msg is None, msg


def test_pipeline_switch_and_restarted_versions(xrt, orc):
    import torch
    spec = xrt.configs.crate_scene(48, 27, max_reflections=3)
    e = Edited(xrt, spec)
    opaque = e.check_frame(orc, spec, "the opaque crate")
    glass = edited(spec, meshes=[_sphere(xrt, transparent=True, refraction_index=float(np.float32(1.32)))],
                   objects=spec.objects + [([1], (-6.0, 14.0, 30.0), ZERO, (4.0, 4.0, 4.0))])
    e.apply(glass, 1)
    got = e.check_frame(orc, glass, "a glass sphere in front of the crate")
    assert not np.array_equal(got[0], opaque[0])
    # one set_poses and one set_materials while a ticket is open: the frame in flight shows the old state, the next one the new one
    px = spec.width * spec.height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    f0, f1 = e.tracer.PrepareDevice(outs[0].data_ptr()), e.tracer.PrepareDevice(outs[1].data_ptr())
    t0 = f0.begin()
    e.scene.Bodies[1].Position = (8.0, 12.0, 28.0)
    e.meshes[0].MeshMaterial.Reflectiveness = 0.125
    t1 = f1.begin()
    f0.end(t0)
    f1.end(t1)
    moved = with_materials(edited(glass, objects=[glass.objects[0], ([1], (8.0, 12.0, 28.0), ZERO, (4.0, 4.0, 4.0))]), {0: dict(reflectiveness=0.125)})
    frame_equal(outs[0].cpu().numpy().view(np.uint32), None, (got[0], None), "the ticket opened before the setters")
    ref = PoseOracle(with_materials(glass, {0: dict(reflectiveness=0.125)}))   # (a moved body stays filed where the last Build filed it, OSM:64-99)
    ref.set_pose(1, (8.0, 12.0, 28.0), ZERO, (4.0, 4.0, 4.0))
    frame_equal(outs[1].cpu().numpy().view(np.uint32), None, ref.render(), "the ticket opened after the setters")
    assert not np.array_equal(outs[0].cpu().numpy(), outs[1].cpu().numpy())
    # the glass removed again: the plain pipeline, the crate with its new reflectiveness
    alone = with_materials(edited(moved, objects=spec.objects), {0: dict(reflectiveness=0.125)})
    e.apply(alone, 0)
    e.check_frame(orc, alone, "the glass sphere removed")


def test_busy_while_a_ticket_is_open(xrt, orc):
    spec = xrt.configs.crate_grid_scene(64, 36, n=3, grid=3)
    spec.scene_threshold = 2
    scene, tracer = xrt.configs.build_product(spec)
    after = edited(spec, objects=spec.objects[:2] + spec.objects[5:])
    arrays = BodyArrays(after)
    lib, abi = xrt.abi.lib(), xrt.abi
    host = np.zeros(spec.width * spec.height, dtype=np.uint32)
    fr = tracer.PrepareHost(host)
    t = fr.begin()
    assert lib.xrt_scene_set_bodies(scene.handle, *arrays.args(), spec.scene_threshold, None) == abi.XRT_E_BUSY
    fr.end(t)
    frame_equal(host, None, oracle(orc, spec), "the frame in flight during the refused call")
    built = C.c_int32(-1)
    assert lib.xrt_scene_set_bodies(scene.handle, *arrays.args(), spec.scene_threshold, C.byref(built)) == abi.XRT_OK and built.value == 0
    t = fr.begin()
    fr.end(t)
    frame_equal(host, None, oracle(orc, after), "the frame after the call")


def test_empty_and_back(xrt, orc):
    spec = xrt.configs.crate_grid_scene(64, 36, n=3, grid=3)
    e = Edited(xrt, spec)
    full = e.check_frame(orc, spec, "the grid")
    rays = e.tracer.GeneratePrimaryRays()
    empty = edited(spec, objects=[])
    e.apply(empty, 0)
    got = e.check_frame(orc, empty, "no bodies")
    assert len(np.unique(got[0])) == 1                                  # the background
    assert not e.scene.IntersectBatch(rays)["hit"].any()
    e.apply(spec, 0)
    frame_equal(*e.check_frame(orc, spec, "refilled"), full, "refilled vs the first frame")
    msg = hits_equal(e.scene.IntersectBatch(rays), orc.OracleScene(spec).intersect(rays))
    assert msg is None, msg
