"""Tree shapes on the MI355X: the cases of tests/tree_shapes.py through the kernels, bit for bit against the CPU oracle -- mesh octrees of 6 .. 20
levels on both sides of every compiled per-lane stack capacity (k_intersect<8 | 12 | 16 | 24 | 40>), scene octrees of 10, 11 and 24 levels on both
sides of the seam between the packet kernel and the per-lane kernel (packet.hip packet_supported), both at once up to the 40 stack words a scene
may need, and scene leaves of 32, 33 and 65 bodies (the 32-body chunks of the scene packet walk), in the builds `default` and `packet`
(XRT_PACKET=31: batches through the packet kernel too).  tests/test_tree_shapes_cpu.py shows on the CPU that the trees have these shapes, that the
oracle's answers reach their deep levels, and that the walk stays inside the stack the device gives it; a case that fails here and passes there is
a fault of the device-only code."""
import ctypes as C

import numpy as np
import pytest

import castray_py
from tree_shapes import CASE_IDS, DEEPEST, all_rays, case, case_spec, oracle_frame, wanted, wanted_mesh
from util import hits_equal

pytestmark = pytest.mark.gpu

BUILDS = {"default": {}, "packet": {"XRT_PACKET": "31"}}
SPLIT = {"XRT_PK_SPLIT": "1", "XRT_PK_BUDGET": "0", "XRT_PK_BUDGET_ITEM": "0"}   # split walks, every packet with pending subtrees hands some over
WORK = ("node_tests", "leaf_refs", "tri_tests", "mesh_aabb_tests", "scene_node_tests", "instance_visits", "mesh_queries")
FRAME_COUNTS = ("rays_closest", "rays_shadow", "hits_shadow", "shaded_hits")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def product(xrt, monkeypatch, spec, build, more=None):
    """The scene and tracer of spec under a build's switches (xrt_scene_create reads them)."""
    for k, v in dict(BUILDS[build], **(more or {})).items():
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


def packets_split(xrt, handle):
    """xrt_split_stats: the packets of the packet kernel that handed subtrees over on the scene's device since the last call."""
    out = (C.c_uint64 * 4)()
    xrt.abi.check(xrt.abi.lib().xrt_split_stats(handle, out, 1))
    return int(out[2])


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", CASE_IDS)
def test_hits(xrt, orc, monkeypatch, name, build):
    """scene.IntersectBatch of every ray family, and mesh.Octree.IntersectBatch of the one-body cases: hit, object, mesh, triangle, leaf, u, v, d and
    the world position."""
    spec, rays = case_spec(xrt, name), all_rays(xrt, orc, name)
    scene, tracer = product(xrt, monkeypatch, spec, build)
    assert hits_equal(wanted(xrt, orc, name)[0], scene.IntersectBatch(rays)) == {}
    if case(name)["kind"] == "mesh":
        assert hits_equal(wanted_mesh(xrt, orc, name), mesh_octree(scene, spec).IntersectBatch(rays)) == {}


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", CASE_IDS)
def test_counting_pass(xrt, orc, monkeypatch, name, build):
    """k_count, which carries a stack of its own: the reference's work counters of the same rays."""
    spec, rays = case_spec(xrt, name), all_rays(xrt, orc, name)
    want, want_st = wanted(xrt, orc, name)
    scene, tracer = product(xrt, monkeypatch, spec, build)
    hits, st = scene.IntersectBatch(rays, stats=True)
    assert hits_equal(want, hits) == {}
    assert want_st["tri_tests"] > 0
    for k in WORK:
        assert st[k] == want_st[k], (k, st[k], want_st[k])


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", CASE_IDS)
def test_frames(xrt, orc, monkeypatch, name, build):
    """A 32 x 32 frame at MaxReflections 2: RGBA8, the fp32 colours and the ray accounting at one sample, RGBA8 at sixteen (k_raygen's root-box
    answers, shadow and reflection rays, the generation-0 tiles)."""
    spec, o_rgba, o_rgbf, o_st = oracle_frame(xrt, orc, name)
    assert o_st["shaded_hits"] > 0
    scene, tracer = product(xrt, monkeypatch, spec, build)
    tracer.collect_stats = True
    rgba, rgbf = tracer.Render(want_float=True)
    bad = int((rgba != o_rgba).sum())
    assert bad == 0, "%d of %d RGBA8 pixels differ" % (bad, rgba.size)
    assert np.array_equal(_bits(rgbf).reshape(-1), _bits(o_rgbf).reshape(-1))
    for k in FRAME_COUNTS:
        assert tracer.last_stats[k] == o_st[k], (k, tracer.last_stats[k], o_st[k])
    spec16, o_rgba, _, o_st = oracle_frame(xrt, orc, name, True)
    assert o_st["shaded_hits"] > 0
    scene, tracer = product(xrt, monkeypatch, spec16, build)
    rgba = tracer.Render()
    assert np.array_equal(rgba, o_rgba), "sixteen samples: %d of %d RGBA8 pixels differ" % (int((rgba != o_rgba).sum()), rgba.size)


@pytest.mark.parametrize("name", DEEPEST)
def test_list_calls(xrt, orc, name):
    """xrt_cast_rays on the camera rays against the checker of tests/castray, and xrt_trace_pixels, unhinted and as a coherent list, against the
    oracle's rays and hits: the list calls share the traversal launch."""
    from test_gpu_trace_pixels import TraceCase
    spec = case_spec(xrt, name)
    cs = castray_py.CastRayScene(spec)
    rays = cs.primary_rays()
    o_rgba, o_rgbf, o_st = cs.cast_rays(rays)
    assert o_st["shaded_hits"] > 0
    tc = TraceCase(xrt, orc, spec)
    rgba, rgbf = tc.tracer.CastRays(rays, want_float=True)
    assert np.array_equal(rgba, o_rgba) and np.array_equal(_bits(rgbf), _bits(o_rgbf))
    for key in ("rays_closest", "rays_shadow", "hits_closest", "shaded_hits"):
        assert tc.tracer.last_stats[key] == o_st[key], (key, tc.tracer.last_stats[key], o_st[key])
    tc.check(np.arange(spec.width * spec.height), False, name)
    tc.check(np.arange(spec.width * spec.height), True, name + " at sixteen samples")


@pytest.mark.parametrize("name", ["scene_sd10", "scene_sd11", "scene_sd24"])
def test_which_kernel_ran(xrt, orc, monkeypatch, capsys, name):
    """Both sides of packet_supported, observed: after a blocking frame xrt_debug_packet_table reports the packet table of the frame's first
    traversal launch, and none where another kernel took that launch.  At scene depth 10 the packet kernel runs (sceneDepth + 1 < PK_SLEVELS); at 11
    and 24 the library answers XRT_PACKET=31 with the per-lane kernel -- and the frame is the oracle's either way."""
    spec, o_rgba, _, _ = oracle_frame(xrt, orc, name)
    scene, tracer = product(xrt, monkeypatch, spec, "packet")
    assert np.array_equal(tracer.Render(), o_rgba)
    entries, paths = scene.PacketTable()
    with capsys.disabled():   # (what was observed belongs in the run's output, passed or not)
        print("\n%s under XRT_PACKET=31: %d packet table entries, %d live rays -> the %s kernel traced the primary rays"
              % (name, entries.shape[0], paths.shape[0], "packet" if entries.shape[0] else "per-lane"))
    if case(name)["sd"] <= 10:
        assert entries.shape[0] > 0 and paths.shape[0] > 0
    else:
        assert entries.shape[0] == 0 and paths.shape[0] == 0


@pytest.mark.parametrize("name", ["mesh_md20", "scene_sd10"])
def test_split_walks(xrt, orc, monkeypatch, name):
    """XRT_PK_SPLIT=1 with a zero budget: packets hand their pending subtrees to other waves at every block they enter -- twenty levels down on the
    deepest mesh tree -- and the answers do not change.  On the one-body case xrt_split_stats also says that the packet kernel ran on that tree and
    did hand subtrees over (the scene walk of a multi-body scene has no split variant: there the switch must simply change nothing)."""
    spec, rays = case_spec(xrt, name), all_rays(xrt, orc, name)
    scene, tracer = product(xrt, monkeypatch, spec, "packet", SPLIT)
    packets_split(xrt, scene.handle)
    assert hits_equal(wanted(xrt, orc, name)[0], scene.IntersectBatch(rays)) == {}
    counts = [packets_split(xrt, scene.handle)]
    if case(name)["kind"] == "mesh":
        octree = mesh_octree(scene, spec)
        assert hits_equal(wanted_mesh(xrt, orc, name), octree.IntersectBatch(rays)) == {}
        counts.append(packets_split(xrt, octree._scene.handle))
    _, o_rgba, _, _ = oracle_frame(xrt, orc, name)
    assert np.array_equal(tracer.Render(), o_rgba)
    print("%s: split packets of the scene batch%s: %r" % (name, ", the mesh batch" if len(counts) > 1 else "", counts))
    if case(name)["kind"] == "mesh":
        assert min(counts) > 0, counts
