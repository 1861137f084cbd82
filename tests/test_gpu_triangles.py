"""xrt_scene_set_triangle_shading[_device] on the MI355X: frames and ray batches of scenes whose triangle normals, texture coordinates and
colours change between frames, bit for bit (RGBA8 words and the uint32 view of the fp32 colour vectors) against the oracle of the spec with
the edited MeshData -- the frame the reference renders after a host wrote Triangle.n1..n3 / uv1..uv3 / color -- and against a product
scene built from scratch of that spec.  Colours, alpha, normals, UVs, the kernel's shapes, the device form against the host form, tickets
that render their own values (three versions), a pipelined loop, ray batches and their paths, seam 1 (which must not notice), replicas,
the paths that upload the scene again, and the scene file."""
import copy

import numpy as np
import pytest

from materials_py import RawScene
from poses_py import hits_equal
from triangles_py import push, with_triangle_shading

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle(orc, spec):
    rgba, rgbf, _ = orc.OracleScene(spec).render(nthreads=16)
    return rgba, rgbf


def frame_equal(got_rgba, got_f, want, what):
    rgba, rgbf = want
    bad = int((np.asarray(got_rgba).reshape(-1) != np.asarray(rgba).reshape(-1)).sum())
    assert bad == 0, "%s: %d of %d pixels differ" % (what, bad, np.asarray(rgba).size)
    if got_f is not None and rgbf is not None:
        assert np.array_equal(_bits(got_f).reshape(-1), _bits(rgbf).reshape(-1)), what


def render(tracer):
    rgba, rgbf = tracer.Render(want_float=True)
    return rgba.copy(), rgbf.copy()


def product(xrt, spec):
    """build_product of a spec with MeshData of its own: the mirror edits the arrays it was given, the spec of the test stays as it is."""
    mine = copy.copy(spec)
    mine.meshes = [(copy.deepcopy(d), m) for d, m in spec.meshes]
    return xrt.configs.build_product(mine)


def check(xrt, orc, tracer, spec, what):
    got = render(tracer)
    frame_equal(*got, oracle(orc, spec), what + " vs the oracle")
    frame_equal(*got, render(xrt.configs.build_product(spec)[1]), what + " vs a scene built from scratch")
    return got


def saved(scene, path):
    scene.Save(path)
    return path.read_bytes()


def fresh_file(xrt, spec, path):
    raw = RawScene(xrt, spec)
    try:
        return raw.saved(path)
    finally:
        raw.close()


def colors(rng, n, alpha=None):
    c = rng.uniform(0.0, 1.0, size=(n, 4)).astype(np.float32)
    if alpha is not None:
        c[:, 3] = np.float32(alpha)
    return c


def test_colours_on_the_reference_content(xrt, orc):
    spec = xrt.configs.content_scene(96, 54, max_reflections=3)   # 0 plane, 1 monkey, 2 torus, 3 sphere, 4 cube
    scene, tracer = product(xrt, spec)
    f0 = render(tracer)
    rng = np.random.default_rng(1)
    nt = [d.ntri for d, _ in spec.meshes]
    edits = {2: dict(ids=range(0, nt[2]), color=colors(rng, nt[2])), 4: dict(ids=range(2, nt[4] - 3), color=colors(rng, nt[4] - 5))}
    push(scene, edits)
    f1 = check(xrt, orc, tracer, with_triangle_shading(spec, edits), "torus and part of the cube recoloured")
    assert not np.array_equal(f0[0], f1[0])


def test_alpha_of_the_glass_spheres(xrt, orc):
    spec = xrt.configs.default_game_scene(64, 64, 4)
    scene, tracer = product(xrt, spec)
    f0 = render(tracer)
    data = spec.meshes[0][0]
    c = data.color.copy()
    c[:, 3] = np.float32(0.875)                                   # color.W alone: the shadow through the occluder (RT:491) and the blend (RT:699)
    edits = {0: dict(ids=range(0, data.ntri), color=c)}
    push(scene, edits)
    f1 = check(xrt, orc, tracer, with_triangle_shading(spec, edits), "alpha 0.875")
    assert not np.array_equal(f0[0], f1[0])
    floor = f0[0].reshape(64, 64) != f1[0].reshape(64, 64)
    assert floor.any()


def test_normals_then_a_uv_only_call(xrt, orc):
    spec = xrt.configs.content_scene(96, 54, max_reflections=3)
    scene, tracer = product(xrt, spec)
    f0 = render(tracer)
    hits = scene.IntersectBatch(tracer.GeneratePrimaryRays())
    torus = hits[(hits["hit"] != 0) & (hits["mesh"] == 2)]["tri"]
    assert torus.size > 10                                       # (the torus is a few dozen pixels of this frame)
    seen = int(np.bincount(torus).argmax())                      # the torus triangle most pixels see
    rng = np.random.default_rng(2)
    data = spec.meshes[2][0]
    ids = np.unique(np.concatenate([rng.permutation(data.ntri)[: data.ntri // 2], [seen]]))
    n = data.n[ids] + rng.normal(scale=0.35, size=(ids.size, 3, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    s = np.float32(np.sqrt(np.float32(3.0)) / np.float32(2.0))
    n[list(ids).index(seen)] = [[1.0, 0.0, 0.0], [-0.5, s, 0.0], [-0.5, -s, 0.0]]   # n1 + n2 + n3 = 0: no normal at the centroid
    assert np.all(n[list(ids).index(seen)].sum(axis=0) == 0)
    e1 = {2: dict(ids=ids, normals=n.astype(np.float32))}
    push(scene, e1)
    s1 = with_triangle_shading(spec, e1)
    f1 = check(xrt, orc, tracer, s1, "new normals on half the torus")
    assert not np.array_equal(f0[0], f1[0])
    e2 = {2: dict(ids=ids, uv=rng.uniform(-3, 3, size=(ids.size, 3, 2)).astype(np.float32))}
    push(scene, e2)
    f2 = check(xrt, orc, tracer, with_triangle_shading(s1, e2), "a uv-only call on the same triangles")
    frame_equal(*f2, f1, "the uv-only call left the normals")


@pytest.mark.parametrize("filtering", ["point", "bilinear"])
@pytest.mark.parametrize("address", ["wrap", "mirror"])
def test_uvs_then_a_normals_only_call(xrt, orc, filtering, address):
    spec = xrt.configs.crate_scene(64, 48, 2)
    spec.filtering = xrt.abi.FILTER_POINT if filtering == "point" else xrt.abi.FILTER_BILINEAR
    spec.address_mode = xrt.abi.ADDRESS_WRAP if address == "wrap" else xrt.abi.ADDRESS_MIRROR
    scene, tracer = product(xrt, spec)
    f0 = render(tracer)
    data = spec.meshes[0][0]
    ids = range(0, data.ntri)
    e1 = {0: dict(ids=ids, uv=data.uv + np.float32(0.71875))}    # uv in [0, 1] before: the shifted ones cross 1.0, a period boundary of both modes
    assert (e1[0]["uv"] > 1).any() and (e1[0]["uv"] < 1).any()
    push(scene, e1)
    s1 = with_triangle_shading(spec, e1)
    f1 = check(xrt, orc, tracer, s1, "uv shifted")
    assert not np.array_equal(f0[0], f1[0])
    rng = np.random.default_rng(3)
    e2 = {0: dict(ids=ids, normals=rng.normal(size=(data.ntri, 3, 3)).astype(np.float32))}
    push(scene, e2)
    f2 = check(xrt, orc, tracer, with_triangle_shading(s1, e2), "a normals-only call on the same triangles")
    frame_equal(*f2, f1, "the normals-only call left the uv")


@pytest.fixture(scope="module")
def spheres(xrt, orc):
    spec = xrt.configs.default_game_scene(48, 48, 2)
    return spec, oracle(orc, spec)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("first,n", [(7, 1), (100, 63), (0, 64), (300, 65), (5, 255), (650, 257), (960 - 130, 130)])
def test_kernel_shapes_on_the_sphere(xrt, orc, spheres, tmp_path, first, n, device):
    """Ranges of 1, 63, 64, 65, 255 and 257 triangles (5 n work-items: below, at and above a wave and a block), and one that ends at the
    mesh's last triangle.  Every word of every record is seen through the file: the values of the device form are read back for it."""
    spec, before = spheres
    assert spec.meshes[0][0].ntri == 960
    scene, tracer = product(xrt, spec)
    rng = np.random.default_rng(first + n)
    edits = {0: dict(ids=range(first, first + n), normals=rng.normal(size=(n, 3, 3)).astype(np.float32), uv=rng.uniform(size=(n, 3, 2)).astype(np.float32),
                     color=colors(rng, n))}
    push(scene, edits, device=device)
    after = with_triangle_shading(spec, edits)
    got = check(xrt, orc, tracer, after, "triangles %d .. %d" % (first, first + n))
    assert saved(scene, tmp_path / "a.xrts") == fresh_file(xrt, after, tmp_path / "b.xrts")
    if n > 60:
        assert not np.array_equal(got[0], before[0])


def test_first_triangle_of_a_mesh_behind_another(xrt, orc, tmp_path):
    spec = xrt.configs.content_scene(96, 54, max_reflections=3)
    scene, tracer = product(xrt, spec)
    rng = np.random.default_rng(5)
    for device in (False, True):                                  # mesh 1 (the monkey) lies behind the plane's triangles in `shade`: triBase != 0
        edits = {1: dict(ids=range(0, 1), normals=rng.normal(size=(1, 3, 3)).astype(np.float32), uv=rng.uniform(size=(1, 3, 2)).astype(np.float32),
                         color=colors(rng, 1))}
        push(scene, edits, device=device)
        spec = with_triangle_shading(spec, edits)
        # the plane's last triangle (the record in front) and the monkey's second are as they were: in the frame, and word for word in the file
        check(xrt, orc, tracer, spec, "first triangle of mesh 1")
        assert saved(scene, tmp_path / "a.xrts") == fresh_file(xrt, spec, tmp_path / "b.xrts")


def test_device_ids_out_of_range_are_skipped(xrt, orc, spheres, tmp_path):
    import torch
    spec, _ = spheres
    scene, tracer = product(xrt, spec)
    rng = np.random.default_rng(6)
    ids = np.array([400, -1, 3, 960, 959, 0, 77, 2 ** 31 - 1, -2 ** 31, 500], dtype=np.int32)
    n = ids.size
    vals = dict(normals=rng.normal(size=(n, 3, 3)).astype(np.float32), uv=rng.uniform(size=(n, 3, 2)).astype(np.float32), color=colors(rng, n))
    t = {k: torch.tensor(v, device="cuda") for k, v in vals.items()}
    scene.SetTriangleShadingDevice(0, torch.tensor(ids, device="cuda"), t["normals"], t["uv"], t["color"])
    ok = (ids >= 0) & (ids < 960)
    after = with_triangle_shading(spec, {0: dict(ids=ids[ok], **{k: v[ok] for k, v in vals.items()})})
    check(xrt, orc, tracer, after, "an unsorted id list with -1 and ntri")
    assert saved(scene, tmp_path / "a.xrts") == fresh_file(xrt, after, tmp_path / "b.xrts")
    # what the device form rejects on the host
    lib, E = xrt.abi.lib(), xrt.abi.XRT_E_INVALID_ARG
    p = lambda x, off=0: xrt.api.C.c_void_p(x.data_ptr() + off)
    assert lib.xrt_scene_set_triangle_shading_device(scene.handle, 0, None, 0, 4, p(t["normals"], 4), None, None, None) == E   # not 16-byte aligned
    assert lib.xrt_scene_set_triangle_shading_device(scene.handle, 0, None, 0, 4, None, None, None, None) == E
    assert lib.xrt_scene_set_triangle_shading_device(scene.handle, 1, None, 0, 4, p(t["normals"]), None, None, None) == E     # one mesh
    assert lib.xrt_scene_set_triangle_shading_device(scene.handle, 0, p(t["uv"]), 1, 4, p(t["normals"]), None, None, None) == E
    assert lib.xrt_scene_set_triangle_shading_device(scene.handle, 0, None, -1, 4, p(t["normals"]), None, None, None) == E
    assert lib.xrt_scene_set_triangle_shading_device(scene.handle, 0, None, 0, 0, None, None, None, None) == xrt.abi.XRT_OK
    assert saved(scene, tmp_path / "a.xrts") == (tmp_path / "b.xrts").read_bytes()
    fresh = xrt.api.OctreeSpatialManager(0)
    fresh._scene = xrt.api._Scene(0)
    assert lib.xrt_scene_set_triangle_shading_device(fresh.handle, 0, None, 0, 4, p(t["normals"]), None, None, None) == xrt.abi.XRT_E_NOT_BUILT


def test_the_device_form_equals_the_host_form(xrt, tmp_path):
    spec = xrt.configs.content_scene(96, 54, max_reflections=3)
    rng = np.random.default_rng(8)
    nt = [d.ntri for d, _ in spec.meshes]
    ids = rng.permutation(nt[1])[:301]
    calls = [{2: dict(ids=range(10, 10 + 257), normals=rng.normal(size=(257, 3, 3)).astype(np.float32), color=colors(rng, 257))},
             {1: dict(ids=ids, uv=rng.uniform(size=(301, 3, 2)).astype(np.float32), color=colors(rng, 301, alpha=0.5))},
             {4: dict(ids=range(0, nt[4]), normals=rng.normal(size=(nt[4], 3, 3)).astype(np.float32))}]
    frames, files = [], []
    for device in (False, True):
        scene, tracer = product(xrt, spec)
        for c in calls:
            push(scene, c, device=device)
        frames.append(render(tracer))
        files.append(saved(scene, tmp_path / ("dev.xrts" if device else "host.xrts")))
    frame_equal(*frames[1], frames[0], "device form vs host form")
    assert files[0] == files[1]
    after = spec
    for c in calls:
        after = with_triangle_shading(after, c)
    assert files[0] == fresh_file(xrt, after, tmp_path / "fresh.xrts")


def _recolour(spec, seed, mesh=0):
    data = spec.meshes[mesh][0]
    c = colors(np.random.default_rng(seed), data.ntri)
    c[:, 3] = data.color[:, 3]
    return {mesh: dict(ids=range(0, data.ntri), color=c)}


def _ticket_scene(xrt):
    spec = xrt.configs.crate_scene(64, 48, 1, textured=False)    # untextured: the crate shows its triangle colours
    return spec


def test_pipelined_tickets_render_their_own_values(xrt, orc):
    import torch
    spec = _ticket_scene(xrt)
    scene, tracer = product(xrt, spec)
    px = spec.width * spec.height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    f0, f1 = tracer.PrepareDevice(outs[0].data_ptr()), tracer.PrepareDevice(outs[1].data_ptr())
    e = _recolour(spec, 1)
    t0 = f0.begin()                                               # the values as built
    push(scene, e)
    t1 = f1.begin()                                               # an edit while ticket 0 is open, then the new values
    f0.end(t0)
    f1.end(t1)
    frame_equal(outs[0].cpu().numpy().view(np.uint32), None, oracle(orc, spec), "ticket of the old values")
    frame_equal(outs[1].cpu().numpy().view(np.uint32), None, oracle(orc, with_triangle_shading(spec, e)), "ticket of the new values")
    assert not np.array_equal(outs[0].cpu().numpy(), outs[1].cpu().numpy())


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_two_open_tickets_and_two_edits_bring_in_the_third_version(xrt, orc, device):
    import torch
    spec = _ticket_scene(xrt)
    scene, tracer = product(xrt, spec)
    px = spec.width * spec.height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    f0, f1 = tracer.PrepareDevice(outs[0].data_ptr()), tracer.PrepareDevice(outs[1].data_ptr())
    ea, eb, ec = _recolour(spec, 2), _recolour(spec, 3), {0: dict(ids=[3, 1], uv=np.full((2, 3, 2), 0.25, dtype=np.float32), color=np.full((2, 4), 0.5, dtype=np.float32))}
    sa = with_triangle_shading(spec, ea)
    sb = with_triangle_shading(sa, eb)
    sc = with_triangle_shading(sb, ec)
    t0 = f0.begin()                                               # version 0
    push(scene, ea, device=device)                                # -> version 1
    t1 = f1.begin()
    push(scene, eb, device=device)                                # both open: -> version 2
    push(scene, ec, device=device)                                # version 2 is read by no ticket: written in place
    f0.end(t0)
    f1.end(t1)
    frame_equal(outs[0].cpu().numpy().view(np.uint32), None, oracle(orc, spec), "ticket 0")
    frame_equal(outs[1].cpu().numpy().view(np.uint32), None, oracle(orc, sa), "ticket 1")
    got = check(xrt, orc, tracer, sc, "the frame after both")
    assert len({outs[0].cpu().numpy().tobytes(), outs[1].cpu().numpy().tobytes(), got[0].tobytes()}) == 3


def test_a_loop_of_recolourings_with_two_frames_in_flight(xrt, orc):
    import torch
    spec = _ticket_scene(xrt)
    scene, tracer = product(xrt, spec)
    px = spec.width * spec.height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    fr = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
    palette = [_recolour(spec, 10 + i) for i in range(4)]
    wants = [oracle(orc, with_triangle_shading(spec, e))[0] for e in palette]
    assert len({w.tobytes() for w in wants}) == 4
    open_ = {}
    for k in range(12):
        push(scene, palette[k % 4], device=k % 3 == 2)
        slot = k % 2
        if slot in open_:
            kk, t = open_.pop(slot)
            fr[slot].end(t)
            frame_equal(outs[slot].cpu().numpy().view(np.uint32), None, (wants[kk % 4], None), "frame %d" % kk)
        open_[slot] = (k, fr[slot].begin())
    for slot, (kk, t) in sorted(open_.items(), key=lambda x: x[1][0]):
        fr[slot].end(t)
        frame_equal(outs[slot].cpu().numpy().view(np.uint32), None, (wants[kk % 4], None), "frame %d" % kk)


def test_cast_rays_and_their_paths_after_an_edit(xrt):
    import castray_py
    import paths_py
    spec = xrt.configs.default_game_scene(32, 32, max_reflections=4)
    scene, tracer = product(xrt, spec)
    rays = tracer.GeneratePrimaryRays()
    data = spec.meshes[0][0]
    rng = np.random.default_rng(12)
    n = data.n + rng.normal(scale=0.2, size=data.n.shape).astype(np.float32)
    edits = {0: dict(ids=range(0, data.ntri), normals=n.astype(np.float32), color=colors(rng, data.ntri, alpha=0.625))}
    before = tracer.CastRays(rays, want_float=True)
    push(scene, edits)
    after = with_triangle_shading(spec, edits)
    rgba, rgbf = tracer.CastRays(rays, want_float=True)
    o_rgba, o_rgbf, _ = castray_py.CastRayScene(after).cast_rays(rays)
    assert np.array_equal(rgba, o_rgba) and np.array_equal(_bits(rgbf), _bits(o_rgbf))
    assert not np.array_equal(rgba, before[0])
    rgba, rgbf, vertices, vstart, back = tracer.CastRays(rays, want_float=True, paths=True)
    want = paths_py.PathsScene(after).cast_rays_paths(rays)
    assert np.array_equal(rgba, want.rgba) and np.array_equal(_bits(rgbf), _bits(want.rgbf))
    assert np.array_equal(vstart, want.vertex_start) and paths_py.same_bits(vertices, want.vertices) and paths_py.same_bits(back, want.rays_back)
    assert len(vertices) > 0


def test_seam_1_does_not_notice(xrt):
    spec = xrt.configs.content_scene(96, 54, max_reflections=3)
    scene, tracer = product(xrt, spec)
    rng = np.random.default_rng(3)
    o = rng.normal(size=(4000, 3)) * 30.0
    d = rng.uniform(-10, 10, size=(4000, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([tracer.GeneratePrimaryRays(), xrt.rays_array(o.astype(np.float32), d.astype(np.float32))])
    before = scene.IntersectBatch(rays)
    for m in range(5):
        nt = spec.meshes[m][0].ntri
        push(scene, {m: dict(ids=range(0, nt), normals=rng.normal(size=(nt, 3, 3)).astype(np.float32), uv=rng.normal(size=(nt, 3, 2)).astype(np.float32),
                             color=colors(rng, nt))}, device=m % 2 == 1)
    after = scene.IntersectBatch(rays)
    assert hits_equal(before, after) is None, hits_equal(before, after)
    assert (before["hit"] != 0).sum() > 1000


def test_replicas_render_the_edited_values(xrt, monkeypatch):
    monkeypatch.setenv("XRT_FAKE_GPUS", "1")
    spec = xrt.configs.crate_grid_scene(200, 120, textured=False)
    scene, tracer = product(xrt, spec)
    tracer.NumGpus = 2
    before = tracer.Render().copy()      # (the replicas exist before the edit)
    tracer.NumGpus = 1
    push(scene, _recolour(spec, 20))
    want = tracer.Render().copy()
    assert not np.array_equal(want, before)
    for n in (2, 3):
        tracer.NumGpus = n
        assert np.array_equal(tracer.Render(), want), "n_gpus %d" % n
    # ... and an edit from device arrays, with the replicas in place; then replicas made after a Build()
    tracer.NumGpus = 1
    push(scene, _recolour(spec, 21), device=True)
    want = tracer.Render().copy()
    for n in (3, 2):
        tracer.NumGpus = n
        assert np.array_equal(tracer.Render(), want), "n_gpus %d after a device edit" % n
    scene.Build()                        # (xrt_scene_build_tree: the replicas go)
    assert np.array_equal(tracer.Render(), want), "n_gpus 2 after build_tree"
    tracer.NumGpus = 1
    assert np.array_equal(tracer.Render(), want)


def test_device_edits_survive_the_uploads(xrt, orc, tmp_path):
    """Build() with the same bodies (xrt_scene_build_tree) and with one more body of a new mesh (xrt_scene_set_bodies, which builds the crate and
    sends every scene array again): the values set from device arrays are still rendered, and still in the file."""
    spec = xrt.configs.content_scene(96, 54, max_reflections=3)
    scene, tracer = product(xrt, spec)
    handle = scene.handle.value
    rng = np.random.default_rng(30)
    nt = [d.ntri for d, _ in spec.meshes]
    edits = {2: dict(ids=range(0, nt[2]), color=colors(rng, nt[2])), 4: dict(ids=rng.permutation(nt[4])[:7], normals=rng.normal(size=(7, 3, 3)).astype(np.float32))}
    push(scene, edits, device=True)
    after = with_triangle_shading(spec, edits)
    for d in scene.meshes:               # the mirror's arrays are put back: only the library holds the edits now
        i = scene.mesh_id(d)
        d.data.n[...], d.data.color[...] = spec.meshes[i][0].n, spec.meshes[i][0].color
    want = check(xrt, orc, tracer, after, "device edits")
    scene.Build()
    assert scene.handle.value == handle
    frame_equal(*render(tracer), want, "after xrt_scene_build_tree")
    api = xrt.api
    crate = (xrt.fixtures.crate(1), xrt.configs.material(0.5))
    body = api.SceneObject([api.Mesh(crate[0], api.Material(0.5, False))], (0.0, 9.0, 0.0), (0.0, 0.0, 0.0))
    scene.Bodies.append(body)
    scene.Build()
    assert scene.handle.value == handle and scene.last_build_meshes == 1
    grown = copy.copy(after)
    grown.meshes = list(after.meshes) + [crate]
    grown.objects = list(after.objects) + [([5], (0.0, 9.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))]
    check(xrt, orc, tracer, grown, "after xrt_scene_set_bodies with a crate")
    assert saved(scene, tmp_path / "a.xrts") == fresh_file(xrt, grown, tmp_path / "b.xrts")


def test_save_load_after_edits(xrt, tmp_path):
    spec = xrt.configs.content_scene(96, 54, max_reflections=3)
    scene, tracer = product(xrt, spec)
    rng = np.random.default_rng(40)
    nt = [d.ntri for d, _ in spec.meshes]
    edits = {0: dict(ids=range(0, nt[0]), uv=spec.meshes[0][0].uv * np.float32(1.5)), 2: dict(ids=range(5, 200), color=colors(rng, 195)),
             3: dict(ids=[0, 959, 17], normals=rng.normal(size=(3, 3, 3)).astype(np.float32), color=colors(rng, 3, alpha=0.25))}
    push(scene, {0: edits[0], 2: edits[2]})
    push(scene, {3: edits[3]}, device=True)
    scene.Save(tmp_path / "edited.xrts")
    tracer.CurrentScene = xrt.api.OctreeSpatialManager.Load(tmp_path / "edited.xrts")
    got = render(tracer)
    frame_equal(*got, render(xrt.configs.build_product(with_triangle_shading(spec, edits))[1]), "loaded")
