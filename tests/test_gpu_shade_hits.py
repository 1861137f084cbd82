"""xrt_shade_hits / xrt_shade_hits_device on the MI355X: what CastRay does with an IntersectionResult (RT:514-737) on caller-given hits,
bit for bit against the checker (tests/shade_hits: one level of the oracle's CastRay on a given result, the oracle's own recursion
below), against xrt_cast_rays on the same rays and against xrt_render -- RGBA8, the fp32 colour vector and the counters."""
import copy
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import shade_hits_py as sh
from materials_py import material_struct, with_materials
from test_gpu_cast_rays import WORK, one_sphere_glass, scenes, world_boxes
from triangles_py import push, with_triangle_shading
from util import random_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the kernel's paths per block and group (csrc/hits.h): list sizes around it cross a group, a block and the grid-stride loop
S = int(re.search(r"INGEST_HITS_SPAN = (\d+);", open(os.path.join(ROOT, "xna-ray-trace_amd", "csrc", "hits.h")).read()).group(1))


def _same(a, b):
    return np.array_equal(a[0], b[0]) and sh.same_bits(a[1], b[1])


def shade(tracer, rays, hits, **kw):
    return tracer.ShadeHits(rays, hits, want_float=True, **kw)


def glass_index(xrt):
    return [m["refraction_index"] for _, m in scenes(xrt)["glass"].meshes if m["transparent"]][0]


def set_lights(xrt, tracer, lights):
    """The tracer's light list from light dicts (configs.build_product's loop)."""
    del tracer.Lights[:]
    for l in lights:
        if l["kind"] == xrt.abi.LIGHT_SPOT:
            L = xrt.api.SpotLight()
            L.Position, L.SpotAngle, L.DecayExponent = l["position"], l["spot_angle"], l["decay_exponent"]
        else:
            L = xrt.api.DirectionalLight()
        L.Direction, L.Color, L.Intensity = l["direction"], l["color"], l["intensity"]
        tracer.Lights.append(L)


def arbitrary_rays(xrt, spec, n):
    """The rays of test_gpu_cast_rays.test_arbitrary_rays: unnormalised directions, origins inside the bodies' boxes, rays that cannot
    reach the root box."""
    rng = np.random.default_rng(n)
    boxes = world_boxes(spec, xrt)
    lo = np.min([b[:3] for b in boxes], axis=0); hi = np.max([b[3:] for b in boxes], axis=0)
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    rays = random_rays(xrt, n, n, radius=radius)
    rays["o"] += centre.astype(np.float32)
    third = n // 3
    rays["d"][:third] *= rng.uniform(0.25, 8.0, size=(third, 1)).astype(np.float32)
    pick = rng.integers(0, len(boxes), size=n)
    for i in range(third, 2 * third):   # origins inside a body's box
        b = boxes[pick[i]]
        rays["o"][i] = rng.uniform(b[:3], b[3:]).astype(np.float32)
    for i in range(2 * third, n, 5):    # far outside, pointing away
        rays["o"][i] = (centre + 4 * radius * np.array([1.0, 0.5, 0.25])).astype(np.float32)
        rays["d"][i] = np.array([1.0, 0.2, 0.1], dtype=np.float32)
    return rays


@pytest.mark.parametrize("name", ["crate", "crate_grid", "glass", "heightfield", "content"])
def test_traced_hits(xrt, name):
    """ShadeHits(R, IntersectBatch(R)) is CastRays(R), the checker and, on the camera's rays, Render(); rows in order and shuffled."""
    spec = scenes(xrt)[name]
    cs = sh.ShadeHitsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rays = cs.primary_rays()
    hits = scene.IntersectBatch(rays)
    assert 0 < int(hits["hit"].sum()) < len(rays)
    got = shade(tracer, rays, hits)
    assert _same(got, tracer.CastRays(rays, want_float=True)), name
    assert _same(got, cs.shade_hits(rays, hits)[:2]), name
    assert _same(got, tracer.Render(want_float=True)), name
    perm = np.random.default_rng(5).permutation(len(rays))
    p = shade(tracer, rays[perm], hits[perm])
    assert _same(p, (got[0][perm], got[1][perm])), name + " shuffled"


@pytest.mark.parametrize("n", [1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1, 100003])
def test_sizes_at_the_kernels_edges(xrt, n):
    spec = scenes(xrt)["crate_grid"]
    cs = sh.ShadeHitsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rays = arbitrary_rays(xrt, spec, n)
    hits = scene.IntersectBatch(rays)
    got = shade(tracer, rays, hits)
    st = dict(tracer.last_stats)
    assert _same(got, cs.shade_hits(rays, hits)[:2]), n
    assert _same(got, tracer.CastRays(rays, want_float=True)), n
    cast = tracer.last_stats
    assert st["pixels"] == n and st["rays_closest"] == cast["rays_closest"] - n and st["hits_closest"] == cast["hits_closest"] - int(hits["hit"].sum())


def test_compaction_patterns(xrt):
    """2S + 1 entries that all carry a valid hit, `hit` overwritten: the kernel's ballots, its scan of the block's cells and its
    reservations under every pattern of live lanes."""
    spec = scenes(xrt)["crate_grid"]
    cs = sh.ShadeHitsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rays = cs.primary_rays()
    hits = scene.IntersectBatch(rays)
    live = np.flatnonzero(hits["hit"] == 1)
    assert len(live) > 64
    n = 2 * S + 1
    pick = np.resize(live, n)
    rays, hits = rays[pick].copy(), hits[pick].copy()
    i = np.arange(n)
    aligned, misaligned = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    aligned[S + 128:S + 192] = False
    misaligned[S + 129:S + 193] = False
    patterns = {"all misses": np.zeros(n, dtype=bool), "all hits": np.ones(n, dtype=bool), "alternating": i % 2 == 1,
                "one hit per wave": (i % 64) == ((i // 64) % 64), "last wave of each block": (i % 1024) >= 960,
                "64 misses aligned": aligned, "64 misses misaligned by one": misaligned}
    black = None
    for what, mask in patterns.items():
        h = hits.copy()
        h["hit"] = mask.astype(np.int32)
        got = shade(tracer, rays, h)
        assert _same(got, cs.shade_hits(rays, h)[:2]), what
        assert tracer.last_stats["shaded_hits"] >= int(mask.sum()), what
        if what == "all misses":
            black = got[0][0]
            assert (got[0] == black).all() and tracer.last_stats["shaded_hits"] == 0 and tracer.last_stats["rays_traversed"] == 0
        else:
            assert (got[0][~mask] == black).all(), what


@pytest.mark.parametrize("name", ["crate_grid", "glass", "content"])
def test_hits_that_are_not_the_rays(xrt, name):
    """The hits of R with random unnormalised directions and garbage origins: the checker's colours; with R's directions and garbage
    origins: CastRays(R) -- CastRay reads the direction alone."""
    spec = scenes(xrt)[name]
    cs = sh.ShadeHitsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rays = cs.primary_rays()
    hits = scene.IntersectBatch(rays)
    rng = np.random.default_rng(11)
    other = rays.copy()
    other["d"] = (rng.normal(size=other["d"].shape) * rng.uniform(0.01, 50.0, size=(len(rays), 1))).astype(np.float32)
    other["o"] = (rng.normal(size=other["o"].shape) * 1e7).astype(np.float32)
    other["o"][::3, 0] = np.nan
    other["o"][1::5] = np.array([np.inf, -np.inf, -0.0], dtype=np.float32)
    other["ignore_mesh"], other["ignore_tri"] = 10 ** 6, 7
    assert _same(shade(tracer, other, hits), cs.shade_hits(other, hits)[:2]), name
    back = other.copy()
    back["d"] = rays["d"]
    assert _same(shade(tracer, back, hits), tracer.CastRays(rays, want_float=True)), name


@pytest.mark.parametrize("name", ["glass", "crate_grid"])
def test_iteration_and_index(xrt, name):
    spec = scenes(xrt)[name]
    cs = sh.ShadeHitsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    rays = cs.primary_rays()
    hits = scene.IntersectBatch(rays)
    M, ref = spec.max_reflections, glass_index(xrt)
    for it in (1, M, M + 1):
        got = shade(tracer, rays, hits, iteration=it, currentRefIndex=ref)
        assert _same(got, cs.shade_hits(rays, hits, iteration=it, ref_index=ref)[:2]), (name, it)
        assert _same(got, tracer.CastRays(rays, iteration=it, currentRefIndex=ref, want_float=True)), (name, it)


@pytest.mark.parametrize("guard", ["0", "1"])
def test_chunks_and_redo(xrt, monkeypatch, guard):
    """Many chunks, a ray-tree chunk that overflows and is ingested again, 128 lights under a small shadow budget -- each with and
    without the guards."""
    monkeypatch.setenv("XRT_GUARD", guard)
    try:
        spec = scenes(xrt)["crate_grid"]
        cs = sh.ShadeHitsScene(spec)
        monkeypatch.setenv("XRT_CHUNK_PATHS", "8192")
        scene, tracer = xrt.configs.build_product(spec)
        rays = random_rays(xrt, 50000, 17, radius=300.0)
        rays["o"] += np.array([0.0, 40.0, 0.0], dtype=np.float32)
        hits = scene.IntersectBatch(rays)
        assert int(hits["hit"].sum()) > 1000
        got = shade(tracer, rays, hits)
        assert _same(got, cs.shade_hits(rays, hits)[:2]), "chunks"
        assert _same(got, tracer.CastRays(rays, want_float=True)), "chunks"
        monkeypatch.delenv("XRT_CHUNK_PATHS")

        glass = one_sphere_glass(xrt)
        gs = sh.ShadeHitsScene(glass)
        rays = gs.primary_rays()
        rays = np.concatenate([rays, rays[np.random.default_rng(8).permutation(len(rays))]])   # 18,432 rays, the second half shuffled
        scene, tracer = xrt.configs.build_product(glass)
        hits = scene.IntersectBatch(rays)
        want = gs.shade_hits(rays, hits)[:2]
        assert _same(shade(tracer, rays, hits), want), "ray tree with room"
        roomy = dict(tracer.last_stats)
        assert roomy["rays_closest"] > 2 * len(rays), "the sphere does not fill the view"
        monkeypatch.setenv("XRT_HEAP_RAY_CAP", "1024")
        scene, tracer = xrt.configs.build_product(glass)
        monkeypatch.delenv("XRT_HEAP_RAY_CAP")
        assert _same(shade(tracer, rays, hits), want), "ray-tree redo"
        assert tracer.last_stats["intersect_launches"] > roomy["intersect_launches"], "no chunk was split"
        for k in ("rays_closest", "hits_closest", "rays_shadow", "shaded_hits"):   # a chunk that was redone is counted once
            assert tracer.last_stats[k] == roomy[k], k

        lit = copy.deepcopy(scenes(xrt)["crate_grid"])
        lit.lights = [xrt.configs.spot((300.0 * np.cos(0.37 * i), 150.0 + 2.0 * i, 300.0 * np.sin(0.37 * i))) for i in range(128)]
        for l in lit.lights:
            l["intensity"] = 0.02
        ls = sh.ShadeHitsScene(lit)
        monkeypatch.setenv("XRT_SHADOW_BYTES", str(84 * 128 * 8192))
        scene, tracer = xrt.configs.build_product(lit)
        rays = np.concatenate([ls.primary_rays()] * 4)   # 10,240 rays: two chunks of 8192 under the budget
        hits = scene.IntersectBatch(rays)
        assert _same(shade(tracer, rays, hits), ls.shade_hits(rays, hits)[:2]), "128 lights"
    finally:
        monkeypatch.delenv("XRT_GUARD")
        xrt.configs.build_product(xrt.configs.crate_scene(32, 32, 0))   # (xrt_scene_create reads the switch)


def test_device_form(xrt):
    """Torch tensors on a non-default stream give the host form's bits; a misaligned pointer is XRT_E_INVALID_ARG; an entry whose mesh or
    triangle is out of range is shaded as a miss and touches no other entry."""
    import torch
    spec = scenes(xrt)["crate_grid"]
    scene, tracer = xrt.configs.build_product(spec)
    cs = sh.ShadeHitsScene(spec)
    rays = cs.primary_rays()
    hits = scene.IntersectBatch(rays)
    host = shade(tracer, rays, hits, iteration=1)
    s = torch.cuda.Stream()

    def on_device(r, h):
        with torch.cuda.stream(s):
            d_rays = torch.from_numpy(r.view(np.float32).reshape(-1, 8).copy()).to("cuda")
            d_hits = torch.from_numpy(h.view(np.int32).reshape(-1, 12).copy()).to("cuda")
            d_rgba, d_rgbf = tracer.ShadeHits(d_rays, d_hits, iteration=1, want_float=True, device=True, stream=s)
        s.synchronize()
        return d_rgba.cpu().numpy().view(np.uint32), d_rgbf.cpu().numpy()
    assert _same(on_device(rays, hits), host)
    # out-of-range entries: negative and huge mesh / tri, with any body
    live = np.flatnonzero(hits["hit"] == 1)
    bad = live[:: max(1, len(live) // 40)][:32]
    broken = hits.copy()
    values = [(-1, 0), (-2 ** 31, 0), (2 ** 31 - 1, 0), (len(spec.meshes), 0), (0, -1), (0, -2 ** 31), (0, 2 ** 31 - 1), (0, spec.meshes[0][0].ntri)]
    for k, at in enumerate(bad):
        broken["mesh"][at], broken["tri"][at] = values[k % len(values)]
        broken["object"][at] = (-7, 10 ** 6, 0)[k % 3]
    got = on_device(rays, broken)
    missed = hits.copy()
    missed["hit"][bad] = 0
    assert _same(got, shade(tracer, rays, missed, iteration=1))
    keep = np.ones(len(rays), dtype=bool); keep[bad] = False
    assert _same((got[0][keep], got[1][keep]), (host[0][keep], host[1][keep]))
    black = got[0][np.flatnonzero(hits["hit"] == 0)[0]]
    assert (got[0][bad] == black).all() and (sh.bits(got[1][bad]) == 0).all()
    # misaligned arrays
    lib, abi = xrt.abi.lib(), xrt.abi
    opts = tracer._opts_abi(shard_count=0)
    lights = tracer._lights_abi()
    raw_r = torch.zeros(64 * 8 + 4, dtype=torch.float32, device="cuda")
    raw_h = torch.zeros(64 * 12 + 4, dtype=torch.int32, device="cuda")
    out = torch.zeros(80, dtype=torch.int32, device="cuda")
    for dr, dh, do in ((4, 0, 0), (0, 8, 0), (0, 0, 4)):
        rc = lib.xrt_shade_hits_device(scene.handle, C.c_void_p(raw_r.data_ptr() + dr), C.c_void_p(raw_h.data_ptr() + dh), 64, 0, 1.0, lights, len(tracer.Lights),
                                       C.byref(opts), C.c_void_p(out.data_ptr() + do), None, None, None)
        assert rc == abi.XRT_E_INVALID_ARG, (dr, dh, do)
    rc = lib.xrt_shade_hits_device(scene.handle, C.c_void_p(raw_r.data_ptr()), C.c_void_p(raw_h.data_ptr()), 64, 0, 1.0, lights, len(tracer.Lights),
                                   C.byref(opts), C.c_void_p(out.data_ptr()), None, None, None)
    assert rc == abi.XRT_OK and (out[:64].cpu().numpy().view(np.uint32) == black).all()   # 64 misses on the scene's own stream


def test_relight_and_rematerial_a_still(xrt):
    """The hits of a still traced once: three positions of the turning light of the reference's video mode (G1:163-164), then new
    reflectiveness and new triangle colours -- each image is the checker's on that scene, and Render()'s with that light."""
    spec = scenes(xrt)["content"]
    scene, tracer = xrt.configs.build_product(spec)
    rays = sh.ShadeHitsScene(spec).primary_rays()
    hits = scene.IntersectBatch(rays)
    images = []
    for degrees in (30.0, 135.0, 250.0):
        rot = math.radians(degrees)
        lit = copy.copy(spec)
        lit.lights = list(spec.lights) + [xrt.configs.directional((float(np.float32(math.sin(rot))), -float(np.float32(math.cos(rot))), 0.0))]
        set_lights(xrt, tracer, lit.lights)
        got = shade(tracer, rays, hits)
        assert _same(got, sh.ShadeHitsScene(lit).shade_hits(rays, hits)[:2]), degrees
        assert _same(got, tracer.Render(want_float=True)), degrees
        images.append(got[0])
    assert not np.array_equal(images[0], images[1]) and not np.array_equal(images[1], images[2])
    # the last light stays; materials and triangle colours change, the geometry and the hits do not
    rng = np.random.default_rng(3)
    changes = {i: dict(reflectiveness=float(np.float32(rng.uniform(0.1, 0.9)))) for i in range(len(spec.meshes))}
    edits = {i: dict(ids=range(0, d.ntri), color=rng.uniform(0, 1, size=(d.ntri, 4)).astype(np.float32)) for i, (d, _) in enumerate(spec.meshes)}
    edited = with_triangle_shading(with_materials(lit, changes), edits)
    scene.SetMaterials(list(range(len(edited.meshes))), [material_struct(m, texels=False)[0] for _, m in edited.meshes])
    push(scene, edits)   # (SetTriangleShading)
    got = shade(tracer, rays, hits)
    assert _same(got, sh.ShadeHitsScene(edited).shade_hits(rays, hits)[:2])
    assert not np.array_equal(got[0], images[2])


def test_stats(xrt):
    for name in ("crate_grid", "glass"):
        spec = scenes(xrt)[name]
        cs = sh.ShadeHitsScene(spec)
        scene, tracer = xrt.configs.build_product(spec)
        rays = cs.primary_rays()
        hits = scene.IntersectBatch(rays)
        n, nhit = len(rays), int(hits["hit"].sum())
        for it in (0, 1):
            tracer.collect_stats = False
            tracer.CastRays(rays, iteration=it)
            cast = dict(tracer.last_stats)
            tracer.ShadeHits(rays, hits, iteration=it)
            st = dict(tracer.last_stats)
            assert st["pixels"] == n
            assert st["rays_closest"] == cast["rays_closest"] - n, (name, it)
            assert st["hits_closest"] == cast["hits_closest"] - nhit, (name, it)
            assert st["rays_shadow"] == cast["rays_shadow"] and st["shaded_hits"] == cast["shaded_hits"], (name, it)
            assert st["rays_traversed"] <= st["rays_closest"] + st["rays_shadow"]
            assert st["intersect_launches"] < cast["intersect_launches"] and st["pieces"] == 1
            tracer.collect_stats = True
            tracer.ShadeHits(rays, hits, iteration=it)
            o_st = cs.shade_hits(rays, hits, iteration=it)[2]
            for k in WORK:
                assert tracer.last_stats[k] == o_st[k], (name, it, k, tracer.last_stats[k], o_st[k])
            assert tracer.last_stats["rays_traversed"] == o_st["rays_closest"] + o_st["rays_shadow"]
        # no lights and no reflection: nothing is traced at all
        tracer.collect_stats = False
        kept = list(tracer.Lights)
        del tracer.Lights[:]
        M = spec.max_reflections
        got = shade(tracer, rays, hits, iteration=M)
        st = tracer.last_stats
        assert st["intersect_launches"] == 0 and st["rays_traversed"] == 0 and st["rays_closest"] == 0 and st["rays_shadow"] == 0 and st["shaded_hits"] == nhit
        assert _same(got, cs.shade_hits(rays, hits, iteration=M, lights=[])[:2])
        tracer.Lights.extend(kept)


def test_errors_and_busy(xrt):
    spec = scenes(xrt)["crate"]
    scene, tracer = xrt.configs.build_product(spec)
    cs = sh.ShadeHitsScene(spec)
    lib, abi = xrt.abi.lib(), xrt.abi
    rays = cs.primary_rays()
    hits = scene.IntersectBatch(rays)
    live = np.flatnonzero(hits["hit"] == 1)
    start = max(0, int(live[0]) - 100)
    at = int(live[0]) - start                                                     # the first entry that is a hit
    rays, hits = rays[start:start + 256].copy(), hits[start:start + 256].copy()   # misses, then hits
    out = np.zeros(len(rays), dtype=np.uint32)
    lights = tracer._lights_abi()

    def call(opts, n=len(rays), h=hits, iteration=0):
        return lib.xrt_shade_hits(scene.handle, rays.ctypes.data_as(C.POINTER(abi.xrt_ray)), h.ctypes.data_as(C.POINTER(abi.xrt_hit)), n, iteration, 1.0, lights,
                                  len(tracer.Lights), C.byref(opts), out.ctypes.data_as(C.POINTER(C.c_uint32)), None, None)

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
    for field, value in (("mesh", 57), ("mesh", -1), ("tri", 10 ** 6), ("tri", -1), ("object", 1), ("object", -1)):
        bad = hits.copy()
        bad[field][at] = value
        out[:] = 0x12345678
        assert call(opts(), h=bad) == abi.XRT_E_INVALID_ARG, (field, value)
        assert (b"hit %d " % at) in lib.xrt_last_error() and (out == 0x12345678).all(), (field, value)
        with pytest.raises(ValueError):
            tracer.ShadeHits(rays, bad)
    glass = scenes(xrt)["glass"]
    gscene, gtracer = xrt.configs.build_product(glass)
    gt = gtracer._opts_abi(shard_count=0); gt.max_reflections = 14
    gr = sh.ShadeHitsScene(glass).primary_rays()[:64].copy()
    gh = gscene.IntersectBatch(gr)
    gout = np.zeros(64, dtype=np.uint32)

    def gcall(iteration):
        return lib.xrt_shade_hits(gscene.handle, gr.ctypes.data_as(C.POINTER(abi.xrt_ray)), gh.ctypes.data_as(C.POINTER(abi.xrt_hit)), 64, iteration, 1.0, None, 0,
                                  C.byref(gt), gout.ctypes.data_as(C.POINTER(C.c_uint32)), None, None)
    assert gcall(1) == abi.XRT_E_UNSUPPORTED
    assert gcall(2) == abi.XRT_OK   # 12 generations
    # a begin/end ticket open: busy; the frame is still right afterwards and the next call works
    frame = np.zeros(spec.width * spec.height, dtype=np.uint32)
    pipe = tracer.PrepareHost(frame)
    t = pipe.begin()
    assert call(opts()) == abi.XRT_E_BUSY
    pipe.end(t)
    o_rgba, _, _ = cs.render()
    assert np.array_equal(frame, o_rgba)
    assert _same(shade(tracer, rays, hits), cs.shade_hits(rays, hits)[:2])
