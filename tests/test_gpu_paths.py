"""xrt_cast_rays_paths / xrt_cast_rays_paths_device on the MI355X: RayTracer.points (RT:543, 701) and CastRay's `ref Ray ray` (RT:692-694), bit
for bit against the checker (tests/paths: the oracle's CastRay with the list kept) -- vertices, vertex_start, the vertex count, rays_back -- and
colours / colour vectors / counters against xrt_cast_rays of the same call.  Every ray of every batch is compared, on raw 32-bit words."""
import ctypes as C

import numpy as np
import pytest

import paths_py
from paths_py import RED, WHITE, same_bits
from test_gpu_cast_rays import COUNTS, one_sphere_glass, scenes
from test_paths_cpu import pane_scene
from util import random_rays, secondary_rays

pytestmark = pytest.mark.gpu


def check(ps, tracer, rays, iteration=0, ref=1.0, what=""):
    """One paths call (counted, then filled) == the checker, and its colours / counters == xrt_cast_rays'."""
    rgba, rgbf, v, vs, back = tracer.CastRays(rays, iteration=iteration, currentRefIndex=ref, want_float=True, paths=True)
    st = dict(tracer.last_stats)
    need = tracer.last_n_vertices
    r = ps.cast_rays_paths(rays, iteration=iteration, ref_index=ref, max_reflections=tracer.MaxReflections)
    print("%s: %d rays, %d vertices (%d red)" % (what, len(rays), r.n_vertices, int((r.vertices["color"] == RED).sum())))
    assert need == r.n_vertices and need % 2 == 0, (what, need, r.n_vertices)
    assert np.array_equal(vs, r.vertex_start), "%s: vertex_start differs for %d rays" % (what, int((vs != r.vertex_start).sum()))
    assert v.shape == r.vertices.shape
    bad = paths_py.bits(v).reshape(-1, 4) != paths_py.bits(r.vertices).reshape(-1, 4)
    assert not bad.any(), "%s: %d of %d vertices differ, first at %d" % (what, int(bad.any(axis=1).sum()), len(v), int(np.argmax(bad.any(axis=1))))
    badr = paths_py.bits(back).reshape(-1, 8) != paths_py.bits(r.rays_back).reshape(-1, 8)
    assert not badr.any(), "%s: rays_back differs for %d rays" % (what, int(badr.any(axis=1).sum()))
    p_rgba, p_rgbf = tracer.CastRays(rays, iteration=iteration, currentRefIndex=ref, want_float=True)   # xrt_cast_rays
    p_st = tracer.last_stats
    assert np.array_equal(rgba, p_rgba) and same_bits(rgbf, p_rgbf), what
    assert np.array_equal(rgba, r.rgba) and same_bits(rgbf, r.rgbf), what
    for k in COUNTS:
        assert st[k] == p_st[k] == r.stats[k], (what, k, st[k], p_st[k], r.stats[k])
    return r


def g1(xrt, max_reflections=8):
    return xrt.configs.default_game_scene(512, 512, max_reflections=max_reflections)


def test_g1_screen_centre_ray_and_primary_grid(xrt):
    """The reference's four glass spheres at MaxReflections 8: the ray Game1 casts on a click -- screen (W / 2, H / 2 - 5), iteration 1 (G1:296-325) --
    through CastRay with RecordPoints, and every ray of a coarse primary grid at iteration 0, 1 and at / above MaxReflections."""
    spec = g1(xrt)
    ps = paths_py.PathsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    prim = tracer.GeneratePrimaryRays()
    assert same_bits(prim, ps.primary_rays())
    centre = prim[(spec.height // 2 - 5) * spec.width + spec.width // 2: (spec.height // 2 - 5) * spec.width + spec.width // 2 + 1].copy()
    r = check(ps, tracer, centre, iteration=1, what="G1 screen centre")
    grid = prim.reshape(spec.height, spec.width)[2::8, 3::8].reshape(-1).copy()
    r0 = check(ps, tracer, grid, iteration=0, what="G1 grid iteration 0")
    assert (r0.vertices["color"] == RED).sum() >= 50 and np.diff(r0.vertex_start).max() >= 10, "the spheres are not in view"
    # ... and through the Python mirror of the reference's surface: CastRay appends to `points` and leaves the ray in last_ray; Render clears the list
    busiest = int(np.argmax(np.diff(r0.vertex_start)))
    tracer.RecordPoints = True
    total = []
    for one in (centre, grid[busiest:busiest + 1]):
        r = ps.cast_rays_paths(one, iteration=1)
        col = tracer.CastRay((one[0]["o"], one[0]["d"]), iteration=1)
        total.append(r.vertices)
        assert col == int(r.rgba[0]) and tracer.last_n_vertices == r.n_vertices
        assert same_bits(tracer.last_ray[0], r.rays_back[0]["o"]) and same_bits(tracer.last_ray[1], r.rays_back[0]["d"])
    tracer.RecordPoints = False
    total = np.concatenate(total)
    assert len(total) >= 4 and len(tracer.points) == len(total) and same_bits(np.array(tracer.points, dtype=xrt.VERTEX_DTYPE), total)
    tracer.CastRay((centre[0]["o"], centre[0]["d"]), iteration=1)
    assert len(tracer.points) == len(total)   # (RecordPoints off: nothing is appended)
    tracer.Render()
    assert tracer.points == []   # RT:61
    check(ps, tracer, grid, iteration=1, what="G1 grid iteration 1")
    for it in (8, 11):
        r = check(ps, tracer, grid, iteration=it, what="G1 grid iteration %d" % it)
        assert (r.vertices["color"] == WHITE).all() and same_bits(r.rays_back, grid)
    inside = spec.meshes[0][1]["refraction_index"]
    check(ps, tracer, grid, iteration=2, ref=inside, what="G1 grid from inside the glass")


def test_opaque_chains(xrt):
    """Plain reflection chains: the crates at depth 3, the C2 crate 24 generations deep, and two facing mirrors whose chains really are that long."""
    spec = xrt.configs.crate_grid_scene(64, 40, max_reflections=3, n=5, grid=4)
    ps = paths_py.PathsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rays = ps.primary_rays()
    r = check(ps, tracer, rays, what="crates depth 3")
    assert not r.tree and np.diff(r.vertex_start).max() >= 4
    check(ps, tracer, rays, iteration=2, what="crates iteration 2")
    spec = xrt.configs.crate_scene(64, 40, max_reflections=24)
    ps = paths_py.PathsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    check(ps, tracer, ps.primary_rays(), what="crate, 24 generations")
    spec = pane_scene(xrt, glass=False, max_reflections=24)
    ps = paths_py.PathsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rng = np.random.default_rng(3)
    o = np.concatenate([rng.uniform(-0.9, 0.9, size=(500, 2)), np.full((500, 1), 5.0)], axis=1).astype(np.float32)
    d = np.concatenate([rng.uniform(-0.02, 0.02, size=(500, 2)), np.full((500, 1), -1.0)], axis=1).astype(np.float32)
    d[:20, :2] = 0.0   # straight on: these bounce between the mirrors until the depth limit
    r = check(ps, tracer, xrt.rays_array(o, d), what="facing mirrors")
    assert np.diff(r.vertex_start).max() == 2 * 25, "no chain runs the whole depth"


def mixed_batch(xrt, ps, scene, seed):
    """Primary rays, rays that miss everything, rays that cannot reach the root box, rays leaving a surface (origin triangle set), duplicates: shuffled."""
    prim = ps.primary_rays()
    sec = secondary_rays(xrt, scene.IntersectBatch(prim), seed=seed)
    assert len(sec) > 50
    far = random_rays(xrt, 300, seed + 1, radius=5000.0)
    far["d"] = -far["d"]                                 # pointing away from the scene: no root box
    up = prim[:200].copy(); up["d"] = (0.0, 1.0, 0.0)    # inside the box's shadow, hitting nothing
    rays = np.concatenate([prim, sec, far, up, prim[::3], sec[::2]])
    return rays[np.random.default_rng(seed).permutation(len(rays))]


@pytest.mark.parametrize("name", ["glass", "crate_grid"])
def test_shuffled_batch_follows_the_callers_order(xrt, name):
    spec = scenes(xrt)[name]
    ps = paths_py.PathsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rays = mixed_batch(xrt, ps, scene, 11)
    r = check(ps, tracer, rays, what=name + " mixed")
    counts = np.diff(r.vertex_start)
    assert (counts == 0).sum() >= 400 and (counts > 0).sum() >= 100
    check(ps, tracer, rays, iteration=1, what=name + " mixed iteration 1")


def raw_call(xrt, scene, tracer, rays, cap, vbuf, iteration=0, vstart=None, back=None):
    lib, abi = xrt.abi.lib(), xrt.abi
    opts, lights = tracer._opts_abi(shard_count=0), tracer._lights_abi()
    opts.n_gpus = 0
    n = len(rays)
    rgba = np.zeros(max(n, 1), dtype=np.uint32)
    need = C.c_int64(-1)
    rc = lib.xrt_cast_rays_paths(scene.handle, rays.ctypes.data_as(C.POINTER(abi.xrt_ray)), n, iteration, 1.0, lights, len(tracer.Lights), C.byref(opts),
                                 rgba.ctypes.data_as(C.POINTER(C.c_uint32)), None, back.ctypes.data_as(C.POINTER(abi.xrt_ray)) if back is not None else None,
                                 vstart.ctypes.data_as(C.POINTER(C.c_int64)) if vstart is not None else None,
                                 vbuf.ctypes.data_as(C.POINTER(abi.xrt_path_vertex)) if vbuf is not None else None, cap, C.byref(need), None)
    return rc, need.value, rgba


def test_capacity(xrt):
    """vertices NULL, 0, one segment, need - 2, need - 1, need, need + 2: the count is always what the batch needs, vertex_start is complete, whole
    segments up to the capacity are written and the guard pattern behind the capacity survives.  rays_back may be the rays themselves."""
    spec = scenes(xrt)["glass"]
    ps = paths_py.PathsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rays = ps.primary_rays()
    r = ps.cast_rays_paths(rays)
    need = r.n_vertices
    assert need > 100
    GUARD = 0xA5C3F00D
    rc, got, _ = raw_call(xrt, scene, tracer, rays, 0, None)
    assert rc == 0 and got == need
    for cap in (0, 2, 3, need - 2, need - 1, need, need + 2):
        vbuf = np.zeros(need + 64, dtype=xrt.VERTEX_DTYPE)
        vbuf.view(np.uint32)[:] = GUARD
        vstart = np.full(len(rays) + 1, -7, dtype=np.int64)
        rc, got, rgba = raw_call(xrt, scene, tracer, rays, cap, vbuf, vstart=vstart)
        wrote = min(need, cap & ~1)
        assert rc == 0 and got == need, (cap, rc, got)
        assert np.array_equal(vstart, r.vertex_start), cap
        assert same_bits(vbuf[:wrote], r.vertices[:wrote]), cap
        assert (vbuf[wrote:].view(np.uint32) == GUARD).all(), "capacity %d: something was written behind it" % cap
        assert np.array_equal(rgba, r.rgba)
    alias = rays.copy()
    vbuf = np.zeros(need, dtype=xrt.VERTEX_DTYPE)
    rc, got, _ = raw_call(xrt, scene, tracer, alias, need, vbuf, back=alias)
    assert rc == 0 and same_bits(alias, r.rays_back) and same_bits(vbuf, r.vertices)
    # n = 0
    vstart = np.full(1, -7, dtype=np.int64)
    rc, got, _ = raw_call(xrt, scene, tracer, rays[:0].copy(), 4, np.zeros(4, dtype=xrt.VERTEX_DTYPE), vstart=vstart)
    assert rc == 0 and got == 0 and vstart[0] == 0


def test_device_form_on_a_stream_busy_and_frames(xrt):
    """Torch tensors on a non-default stream give the host form's bits, nothing is written behind the capacity on the device either; XRT_E_BUSY while
    a ticket is open; the frame rendered before and after a paths call is the oracle's."""
    import torch
    spec = scenes(xrt)["glass"]
    ps = paths_py.PathsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    o_rgba, o_rgbf, _ = ps.render()
    f_rgba, f_rgbf = tracer.Render(want_float=True)
    assert np.array_equal(f_rgba, o_rgba) and same_bits(f_rgbf, o_rgbf)
    rays = ps.primary_rays()
    r = check(ps, tracer, rays, iteration=1, what="glass host form")
    f_rgba, f_rgbf = tracer.Render(want_float=True)
    assert np.array_equal(f_rgba, o_rgba) and same_bits(f_rgbf, o_rgbf), "the frame after a paths call"
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda")
        d_rgba, d_rgbf, d_v, d_vs, d_back = tracer.CastRays(d_rays, iteration=1, want_float=True, device=True, stream=s, paths=True)
        assert tracer.last_n_vertices == r.n_vertices
        cap = r.n_vertices - 6
        guard = torch.full((r.n_vertices + 8, 4), 123.0, dtype=torch.float32, device="cuda")
        tracer.CastRays(d_rays, iteration=1, device=True, stream=s, paths=True, vertex_capacity=cap)   # (sized by the caller: one call)
        lib, abi = xrt.abi.lib(), xrt.abi
        opts, lights = tracer._opts_abi(shard_count=0), tracer._lights_abi()
        opts.n_gpus = 0
        need = C.c_int64(0)
        rgba2 = torch.empty(len(rays), dtype=torch.int32, device="cuda")
        rc = lib.xrt_cast_rays_paths_device(scene.handle, C.c_void_p(d_rays.data_ptr()), len(rays), 1, 1.0, lights, len(tracer.Lights), C.byref(opts),
                                            C.c_void_p(rgba2.data_ptr()), None, None, None, C.c_void_p(guard.data_ptr()), cap, C.c_void_p(s.cuda_stream),
                                            C.byref(need), None)
        assert rc == 0 and need.value == r.n_vertices
        rc = lib.xrt_cast_rays_paths_device(scene.handle, C.c_void_p(d_rays.data_ptr()), len(rays), 1, 1.0, lights, len(tracer.Lights), C.byref(opts),
                                            C.c_void_p(rgba2.data_ptr()), None, C.c_void_p(d_rays.data_ptr()), None, None, 0, C.c_void_p(s.cuda_stream),
                                            C.byref(need), None)
        assert rc == abi.XRT_E_INVALID_ARG   # rays_back must not be the rays in the device form
        rc = lib.xrt_cast_rays_paths_device(scene.handle, C.c_void_p(d_rays.data_ptr()), len(rays), 1, 1.0, lights, len(tracer.Lights), C.byref(opts),
                                            C.c_void_p(rgba2.data_ptr()), None, None, None, C.c_void_p(guard.data_ptr() + 4), cap, C.c_void_p(s.cuda_stream),
                                            C.byref(need), None)
        assert rc == abi.XRT_E_INVALID_ARG   # alignment
    s.synchronize()
    assert np.array_equal(d_rgba.cpu().numpy().view(np.uint32), r.rgba) and same_bits(d_rgbf.cpu().numpy(), r.rgbf)
    assert same_bits(d_v.cpu().numpy(), r.vertices) and np.array_equal(d_vs.cpu().numpy(), r.vertex_start) and same_bits(d_back.cpu().numpy(), r.rays_back)
    g = guard.cpu().numpy()
    assert same_bits(g[:cap], r.vertices[:cap]) and (g[cap:] == 123.0).all(), "the device form wrote behind the capacity"
    # a begin / end ticket open: busy; afterwards the frame is right and the next paths call works
    frame = np.zeros(spec.width * spec.height, dtype=np.uint32)
    pipe = tracer.PrepareHost(frame)
    t = pipe.begin()
    rc, _, _ = raw_call(xrt, scene, tracer, rays, 0, None)
    assert rc == xrt.abi.XRT_E_BUSY
    pipe.end(t)
    assert np.array_equal(frame, o_rgba)
    check(ps, tracer, rays, what="glass after the ticket")


@pytest.mark.parametrize("guard", ["0", "1"])
def test_chunked_and_redone_batches(xrt, monkeypatch, guard):
    """A batch of many chunks (XRT_CHUNK_PATHS) and a ray-tree batch whose chunks overflow and are redone (XRT_HEAP_RAY_CAP): the running offsets
    cross the chunks, and a generation that is redone leaves nothing of its first attempt behind -- with and without the buffer guards."""
    monkeypatch.setenv("XRT_GUARD", guard)
    try:
        spec = scenes(xrt)["crate_grid"]
        ps = paths_py.PathsScene(spec)
        monkeypatch.setenv("XRT_CHUNK_PATHS", "8192")
        scene, tracer = xrt.configs.build_product(spec)
        monkeypatch.delenv("XRT_CHUNK_PATHS")
        rays = random_rays(xrt, 30000, 17, radius=300.0)
        rays["o"] += np.array([0.0, 40.0, 0.0], dtype=np.float32)
        r = check(ps, tracer, rays, what="4 chunks")
        assert r.n_vertices > 1000

        glass = one_sphere_glass(xrt)
        gs = paths_py.PathsScene(glass)
        rays = gs.primary_rays()
        rays = np.concatenate([rays, rays[np.random.default_rng(8).permutation(len(rays))]])
        scene, tracer = xrt.configs.build_product(glass)
        check(gs, tracer, rays, what="ray tree with room")
        roomy = dict(tracer.last_stats)
        monkeypatch.setenv("XRT_HEAP_RAY_CAP", "1024")
        scene, tracer = xrt.configs.build_product(glass)
        monkeypatch.delenv("XRT_HEAP_RAY_CAP")
        check(gs, tracer, rays, what="ray-tree redo")
        assert tracer.last_stats["intersect_launches"] > roomy["intersect_launches"], "no chunk was split"
        check(gs, tracer, rays, ref=glass.meshes[0][1]["refraction_index"], what="ray-tree redo inside")
        f_rgba = tracer.Render()
        assert np.array_equal(f_rgba, gs.render()[0]), "the frame after redone paths calls"
    finally:
        monkeypatch.delenv("XRT_GUARD")
        xrt.configs.build_product(xrt.configs.crate_scene(32, 32, 0))   # (xrt_scene_create reads the switch)
