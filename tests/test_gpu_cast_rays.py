"""xrt_cast_rays / xrt_cast_rays_device on the MI355X: RayTracer.CastRay (RT:506-737) on caller-given rays, bit for bit against the
checker (tests/castray: the oracle's own CastRay) -- RGBA8, the fp32 colour vector and the ray counts."""
import copy
import ctypes as C

import numpy as np
import pytest

import castray_py
from util import random_rays, secondary_rays, triangle_soup

pytestmark = pytest.mark.gpu

COUNTS = ("rays_closest", "rays_shadow", "hits_closest", "shaded_hits", "pixels")
WORK = ("rays_closest", "rays_shadow", "hits_closest", "hits_shadow", "scene_node_tests", "instance_visits", "mesh_aabb_tests", "mesh_queries",
        "node_tests", "leaf_refs", "tri_tests", "shaded_hits", "pixels", "algorithmic_bytes")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(cs, tracer, rays, iteration=0, ref=1.0, collect=False, what=""):
    """GPU batch == checker: colours, colour vectors, counters (all of them with the counting pass)."""
    tracer.collect_stats = collect
    rgba, rgbf = tracer.CastRays(rays, iteration=iteration, currentRefIndex=ref, want_float=True)
    st = tracer.last_stats
    o_rgba, o_rgbf, o_st = cs.cast_rays(rays, iteration=iteration, ref_index=ref, max_reflections=tracer.MaxReflections)
    bad = int((rgba != o_rgba).sum())
    assert bad == 0, "%s: %d of %d colours differ" % (what, bad, len(rays))
    assert np.array_equal(_bits(rgbf), _bits(o_rgbf)), what
    for k in (WORK if collect else COUNTS):
        assert st[k] == o_st[k], (what, k, st[k], o_st[k])
    return rgba, rgbf


def soup_spec(xrt, n, seed, threshold, size):
    s = xrt.configs.SceneSpec("soup")
    s.meshes.append((triangle_soup(n, seed, size), xrt.configs.material(0.5)))
    s.objects.append(([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    s.camera = xrt.configs.camera((0, 3, 3), (0, 0, 0))
    s.lights = [xrt.configs.spot((0, 5, 5))]
    s.mesh_threshold = threshold
    s.max_reflections = 3
    return s.with_size(48, 48)


def two_mesh_spec(xrt):
    s = xrt.configs.SceneSpec("inst")
    s.meshes.append((xrt.fixtures.crate(3), xrt.configs.material(0.5, texture=xrt.fixtures.crate_texture())))
    s.meshes.append((triangle_soup(80, 11, 0.4), xrt.configs.material(0.2, interpolate_normals=True)))
    k = 0
    for ix in range(5):
        for iz in range(5):
            s.objects.append(([0] if (k % 3) else [0, 1], (-60.0 + 30.0 * ix, 2.0 * (k % 2), -60.0 + 30.0 * iz),
                              (0.1 * ix, 0.37 * iz, 0.05 * (ix + iz)), (1.0 + 0.1 * ix, 1.0, 0.8 + 0.1 * iz)))
            k += 1
    s.camera = xrt.configs.camera((0, 80, 160), (0, 0, 0))
    s.lights = [xrt.configs.spot((0, 100, 100)), xrt.configs.directional((0.3, 0.8, 0.5), (0.4, 0.5, 0.6), 0.7)]
    s.max_reflections = 3
    return s.with_size(96, 54)


def one_sphere_glass(xrt, size=96):
    """A glass sphere scaled by 4 filling the view (one body): most paths refract as well as reflect, generation 1 holds about twice the
    rays of generation 0 -- the geometry under which a ray-tree chunk overflows a small XRT_HEAP_RAY_CAP."""
    spec = xrt.configs.default_game_scene(size, size, max_reflections=4)
    spec.objects = [([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (4.0, 4.0, 4.0))]
    spec.camera = xrt.configs.camera((0, 0, 14), (0, 0, 0))
    return spec


def scenes(xrt):
    cfg = xrt.configs
    return {"crate": cfg.crate_scene(64, 40, max_reflections=2), "crate_grid": cfg.crate_grid_scene(64, 40),
            "glass": cfg.default_game_scene(48, 48, 4), "heightfield": cfg.heightfield_scene(64, 36, m=48),
            "content": cfg.content_scene(64, 36)}


def world_boxes(spec, xrt):
    out = []
    for ids, pos, rot, scale in spec.objects:
        bb = np.zeros(6, dtype=np.float32)
        for i in ids:
            bb[:3] = np.minimum(bb[:3], spec.meshes[i][0].bbox[:3]); bb[3:] = np.maximum(bb[3:], spec.meshes[i][0].bbox[3:])
        out.append(np.asarray(xrt.xna.build_world(scale, rot, pos, bb)[2], dtype=np.float32).reshape(-1)[:6])
    return out


@pytest.mark.parametrize("name", ["crate", "crate_grid", "glass", "heightfield", "content"])
def test_camera_rays_as_a_batch(xrt, name):
    """The camera's primary rays, row-major and shuffled (colours put back in place), are the checker's and xrt_render's frame."""
    spec = scenes(xrt)[name]
    cs = castray_py.CastRayScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rays = cs.primary_rays()
    rgba, rgbf = check(cs, tracer, rays, what=name)
    f_rgba, f_rgbf = tracer.Render(want_float=True)
    assert np.array_equal(rgba, f_rgba) and np.array_equal(_bits(rgbf), _bits(f_rgbf)), name
    perm = np.random.default_rng(5).permutation(len(rays))
    p_rgba, p_rgbf = check(cs, tracer, rays[perm], what=name + " shuffled")
    back = np.empty_like(p_rgba); back[perm] = p_rgba
    backf = np.empty_like(p_rgbf); backf[perm] = p_rgbf
    assert np.array_equal(back, f_rgba) and np.array_equal(_bits(backf), _bits(f_rgbf))


@pytest.mark.parametrize("name", ["crate", "glass", "crate_grid"])
def test_iteration(xrt, name):
    """CastRay from iteration 1 (Game1's call, G1:307/325), 2, MaxReflections and MaxReflections + 1."""
    spec = scenes(xrt)[name]
    cs = castray_py.CastRayScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rays = cs.primary_rays()
    M = spec.max_reflections
    for k in (1, 2, M, M + 1):
        check(cs, tracer, rays, iteration=k, what="%s iteration %d" % (name, k))
    # the single-ray surface: the screen centre's ray (G1:296-307)
    c = rays[(spec.height // 2) * spec.width + spec.width // 2]
    col, vec = tracer.CastRay((c["o"], c["d"]), iteration=1, want_float=True)
    o_rgba, o_rgbf, _ = cs.cast_rays(rays[(spec.height // 2) * spec.width + spec.width // 2:][:1], iteration=1)
    assert col == int(o_rgba[0]) and np.array_equal(_bits(vec), _bits(o_rgbf[0]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100003])
def test_arbitrary_rays(xrt, n):
    """Unnormalised directions (x 0.25 .. 8), origins inside the bodies' boxes, rays that miss the root box."""
    spec = scenes(xrt)["crate_grid"]
    cs = castray_py.CastRayScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rng = np.random.default_rng(n)
    boxes = world_boxes(spec, xrt)
    lo = np.min([b[:3] for b in boxes], axis=0); hi = np.max([b[3:] for b in boxes], axis=0)
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    rays = random_rays(xrt, n, n, radius=radius)
    rays["o"] += centre.astype(np.float32)
    third = n // 3
    rays["d"][:third] *= rng.uniform(0.25, 8.0, size=(third, 1)).astype(np.float32)
    b = [boxes[i] for i in rng.integers(0, len(boxes), size=n)]
    for i in range(third, 2 * third):   # origins inside a body's box
        rays["o"][i] = rng.uniform(b[i][:3], b[i][3:]).astype(np.float32)
    for i in range(2 * third, n, 5):    # far outside, pointing away: they cannot reach the root box
        rays["o"][i] = (centre + 4 * radius * np.array([1.0, 0.5, 0.25])).astype(np.float32)
        rays["d"][i] = np.array([1.0, 0.2, 0.1], dtype=np.float32)
    check(cs, tracer, rays, what="arbitrary n=%d" % n)


def test_rays_with_an_origin_triangle(xrt):
    """Secondary rays off hits (ignore = the hit triangle) of a soup, of rotated / scaled bodies with two meshes, and of the glass scene
    with currentRefIndex 1 and the glass's refraction index (RT:658: "inside")."""
    for spec in (soup_spec(xrt, 300, 5, 4, 0.5), two_mesh_spec(xrt), scenes(xrt)["glass"]):
        cs = castray_py.CastRayScene(spec)
        scene, tracer = xrt.configs.build_product(spec)
        rays = secondary_rays(xrt, scene.IntersectBatch(cs.primary_rays()), seed=3)
        assert len(rays) > 50
        refs = [1.0] + [m["refraction_index"] for _, m in spec.meshes if m["transparent"]][:1]
        for ref in refs:
            check(cs, tracer, rays, ref=ref, what="%s origin ref %r" % (spec.name, ref))
            check(cs, tracer, rays, iteration=1, ref=ref, what="%s origin ref %r iteration 1" % (spec.name, ref))


@pytest.mark.parametrize("guard", ["0", "1"])
def test_large_batches(xrt, monkeypatch, guard):
    """Many chunks, ray-tree overflow and redo, 128 lights under a small shadow budget -- each with and without the guards."""
    monkeypatch.setenv("XRT_GUARD", guard)
    try:
        spec = scenes(xrt)["crate_grid"]
        cs = castray_py.CastRayScene(spec)
        monkeypatch.setenv("XRT_CHUNK_PATHS", "8192")
        scene, tracer = xrt.configs.build_product(spec)
        rays = random_rays(xrt, 50000, 17, radius=300.0)
        rays["o"] += np.array([0.0, 40.0, 0.0], dtype=np.float32)
        check(cs, tracer, rays, what="chunks")
        monkeypatch.delenv("XRT_CHUNK_PATHS")

        glass = one_sphere_glass(xrt)
        gs = castray_py.CastRayScene(glass)
        rays = gs.primary_rays()
        rays = np.concatenate([rays, rays[np.random.default_rng(8).permutation(len(rays))]])   # 18,432 rays, the second half shuffled
        scene, tracer = xrt.configs.build_product(glass)
        check(gs, tracer, rays, what="ray tree with room")
        roomy = dict(tracer.last_stats)
        assert roomy["rays_closest"] > 3 * len(rays), "the sphere does not fill the view"
        monkeypatch.setenv("XRT_HEAP_RAY_CAP", "1024")
        scene, tracer = xrt.configs.build_product(glass)
        monkeypatch.delenv("XRT_HEAP_RAY_CAP")
        check(gs, tracer, rays, what="ray-tree redo")
        check(gs, tracer, rays, ref=glass.meshes[0][1]["refraction_index"], what="ray-tree redo inside")
        assert tracer.last_stats["intersect_launches"] > roomy["intersect_launches"], "no chunk was split"

        lit = copy.deepcopy(scenes(xrt)["crate_grid"])
        lit.lights = [xrt.configs.spot((300.0 * np.cos(0.37 * i), 150.0 + 2.0 * i, 300.0 * np.sin(0.37 * i))) for i in range(128)]
        for l in lit.lights:
            l["intensity"] = 0.02
        ls = castray_py.CastRayScene(lit)
        monkeypatch.setenv("XRT_SHADOW_BYTES", str(84 * 128 * 8192))
        scene, tracer = xrt.configs.build_product(lit)
        check(ls, tracer, np.concatenate([ls.primary_rays()] * 6), what="128 lights")
    finally:
        monkeypatch.delenv("XRT_GUARD")
        xrt.configs.build_product(xrt.configs.crate_scene(32, 32, 0))   # (xrt_scene_create reads the switch)


def test_collect_stats(xrt):
    """collect_stats = 1: every reference work counter equals the checker's (the culled rays included)."""
    for name in ("crate_grid", "glass"):
        spec = scenes(xrt)[name]
        cs = castray_py.CastRayScene(spec)
        scene, tracer = xrt.configs.build_product(spec)
        rays = cs.primary_rays()
        rays = np.concatenate([rays, secondary_rays(xrt, scene.IntersectBatch(rays), seed=4)])
        check(cs, tracer, rays, collect=True, what=name)
        check(cs, tracer, rays, iteration=1, collect=True, what=name + " iteration 1")


def test_device_variant(xrt):
    """Torch tensors on a non-default stream give the host variant's bits; a misaligned pointer is XRT_E_INVALID_ARG."""
    import torch
    spec = scenes(xrt)["crate_grid"]
    scene, tracer = xrt.configs.build_product(spec)
    cs = castray_py.CastRayScene(spec)
    rays = cs.primary_rays()
    h_rgba, h_rgbf = tracer.CastRays(rays, iteration=1, want_float=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda", non_blocking=False)
        d_rgba, d_rgbf = tracer.CastRays(d_rays, iteration=1, want_float=True, device=True, stream=s)
    s.synchronize()
    assert np.array_equal(d_rgba.cpu().numpy().view(np.uint32), h_rgba)
    assert np.array_equal(_bits(d_rgbf.cpu().numpy()), _bits(h_rgbf))
    lib, abi = xrt.abi.lib(), xrt.abi
    opts = tracer._opts_abi(shard_count=0)
    lights = tracer._lights_abi()
    raw = torch.zeros(64 * 8 + 4, dtype=torch.float32, device="cuda")
    out = torch.zeros(80, dtype=torch.int32, device="cuda")
    rc = lib.xrt_cast_rays_device(scene.handle, C.c_void_p(raw.data_ptr() + 4), 64, 0, 1.0, lights, len(tracer.Lights), C.byref(opts),
                                  C.c_void_p(out.data_ptr()), None, None, None)
    assert rc == abi.XRT_E_INVALID_ARG
    rc = lib.xrt_cast_rays_device(scene.handle, C.c_void_p(raw.data_ptr()), 64, 0, 1.0, lights, len(tracer.Lights), C.byref(opts),
                                  C.c_void_p(out.data_ptr() + 4), None, None, None)
    assert rc == abi.XRT_E_INVALID_ARG


def test_errors_and_busy(xrt):
    spec = scenes(xrt)["crate"]
    scene, tracer = xrt.configs.build_product(spec)
    cs = castray_py.CastRayScene(spec)
    lib, abi = xrt.abi.lib(), xrt.abi
    rays = cs.primary_rays()[:256].copy()
    out = np.zeros(len(rays), dtype=np.uint32)
    lights = tracer._lights_abi()

    def call(opts, n=len(rays), r=rays, iteration=0):
        return lib.xrt_cast_rays(scene.handle, r.ctypes.data_as(C.POINTER(abi.xrt_ray)), n, iteration, 1.0, lights, len(tracer.Lights), C.byref(opts),
                                 out.ctypes.data_as(C.POINTER(C.c_uint32)), None, None)

    def opts(**kw):
        o = tracer._opts_abi(shard_count=0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    assert call(opts(use_multisampling=abi.MS_FIXED16)) == abi.XRT_E_INVALID_ARG
    assert call(opts(use_multisampling=abi.MS_ADAPTIVE)) == abi.XRT_E_INVALID_ARG
    assert call(opts(shard_count=2)) == abi.XRT_E_INVALID_ARG
    assert call(opts(n_gpus=2)) == abi.XRT_E_INVALID_ARG
    assert call(opts(), n=-1) == abi.XRT_E_INVALID_ARG
    assert call(opts(max_reflections=70), iteration=2) == abi.XRT_E_INVALID_ARG
    assert call(opts(max_reflections=70), iteration=6) == abi.XRT_OK          # 64 generations are allowed
    assert call(opts(), n=0) == abi.XRT_OK
    for im, it in ((0, 10 ** 6), (57, 0), (-1, 3)):
        bad = rays.copy(); bad["ignore_mesh"][7], bad["ignore_tri"][7] = im, it
        assert call(opts(), r=bad) == abi.XRT_E_INVALID_ARG, (im, it)
    glass = scenes(xrt)["glass"]
    gscene, gtracer = xrt.configs.build_product(glass)
    gt = gtracer._opts_abi(shard_count=0); gt.max_reflections = 14
    gr = castray_py.CastRayScene(glass).primary_rays()[:64].copy()
    gout = np.zeros(64, dtype=np.uint32)
    assert lib.xrt_cast_rays(gscene.handle, gr.ctypes.data_as(C.POINTER(abi.xrt_ray)), 64, 1, 1.0, None, 0, C.byref(gt),
                             gout.ctypes.data_as(C.POINTER(C.c_uint32)), None, None) == abi.XRT_E_UNSUPPORTED
    assert lib.xrt_cast_rays(gscene.handle, gr.ctypes.data_as(C.POINTER(abi.xrt_ray)), 64, 2, 1.0, None, 0, C.byref(gt),
                             gout.ctypes.data_as(C.POINTER(C.c_uint32)), None, None) == abi.XRT_OK   # 12 generations
    # a begin/end ticket open: busy; the frame is still right afterwards and the next cast works
    frame = np.zeros(spec.width * spec.height, dtype=np.uint32)
    pipe = tracer.PrepareHost(frame)
    t = pipe.begin()
    assert call(opts()) == abi.XRT_E_BUSY
    pipe.end(t)
    o_rgba, _, _ = cs.render()
    assert np.array_equal(frame, o_rgba)
    check(cs, tracer, rays, what="after the ticket")


def test_both_generation0_kernels(xrt, monkeypatch):
    """Generation 0 of a batch goes to the per-lane kernel unless XRT_PACKET / XRT_PACKET_HEAP route it to the packets (bit 0): same bits.
    Which kernel ran is seen through the split walks of the packet kernel (one-body scenes, XRT_PK_SPLIT=1 with a zero budget: every
    packet with pending subtrees hands some over, xrt_split_stats counts them): none without the switch, some with bit 0 alone."""
    monkeypatch.setenv("XRT_PK_SPLIT", "1")
    monkeypatch.setenv("XRT_PK_BUDGET", "0")
    monkeypatch.setenv("XRT_PK_BUDGET_ITEM", "0")
    for name, var, spec in (("heightfield", "XRT_PACKET", scenes(xrt)["heightfield"]), ("one-sphere glass", "XRT_PACKET_HEAP", one_sphere_glass(xrt, 48))):
        cs = castray_py.CastRayScene(spec)
        rays = cs.primary_rays()
        perm = np.random.default_rng(2).permutation(len(rays))
        outs = {}
        for mask in (None, "1"):
            if mask is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, mask)
            scene, tracer = xrt.configs.build_product(spec)
            for order, r in (("row-major", rays), ("shuffled", rays[perm])):
                scene.SplitStats(reset=True)
                rgba, rgbf = check(cs, tracer, r, what="%s %s=%s %s" % (name, var, mask, order))
                packets = scene.SplitStats(reset=True)[2]
                if mask is None:
                    assert packets == 0, (name, order, "a packet launch ran without the switch")
                else:
                    assert packets > 0, (name, order, "generation 0 did not go to the packet kernel")
                outs[(mask, order)] = (rgba, _bits(rgbf))
        monkeypatch.delenv(var, raising=False)
        for order in ("row-major", "shuffled"):
            a, b = outs[(None, order)], outs[("1", order)]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, order)
    # a two-level scene: the packet kernel has no split walks there, the bits are compared only
    spec = scenes(xrt)["crate_grid"]
    cs = castray_py.CastRayScene(spec)
    rays = cs.primary_rays()
    for mask in (None, "31"):
        if mask is None:
            monkeypatch.delenv("XRT_PACKET", raising=False)
        else:
            monkeypatch.setenv("XRT_PACKET", mask)
        scene, tracer = xrt.configs.build_product(spec)
        check(cs, tracer, rays, what="crate_grid XRT_PACKET=%s" % mask)
    monkeypatch.delenv("XRT_PACKET", raising=False)
