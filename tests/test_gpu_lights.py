"""xrt_light_hits / xrt_light_hits_device on the MI355X: CastRay's light loop (RT:534-542) on caller-given hits -- the fp32 light sum and
IsLightPathObstructed's amount per light (RT:465-502) -- bit for bit against the checker (tests/lights: the loop written with the oracle's
own IsLightPathObstructed and GetLightForFragment) and against the colour vectors of xrt_cast_rays and xrt_shade_hits where the surface
colour is (1, 1, 1).  Every comparison is bit for bit; a NaN equals a NaN of any payload."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import lights_py as lp
from materials_py import material_struct, with_materials
from poses_py import moved, pose_arrays
from test_gpu_cast_rays import scenes, two_mesh_spec
from test_gpu_shade_hits import arbitrary_rays, set_lights
from triangles_py import push, with_triangle_shading

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the emission kernel's entries per block and round (csrc/lights.h): list sizes around it cross a round, a block and the grid-stride loop
B = int(re.search(r"LIGHT_EMIT_BLOCK = (\d+);", open(os.path.join(ROOT, "xna-ray-trace_amd", "csrc", "lights.h")).read()).group(1))
_CTX = {}


def specs(xrt):
    out = dict(scenes(xrt))
    out["two_mesh"] = two_mesh_spec(xrt)
    return out


def ctx(xrt, name):
    """(spec, checker scene, product scene, tracer, the camera's rays, their hits) of a scene, made once; the tests that edit a scene make
    their own."""
    if name not in _CTX:
        spec = specs(xrt)[name]
        cs = lp.LightsScene(spec)
        scene, tracer = xrt.configs.build_product(spec)
        rays = cs.primary_rays()
        _CTX[name] = (spec, cs, scene, tracer, rays, scene.IntersectBatch(rays))
    return _CTX[name]


def light_hits(tracer, hits, **kw):
    return tracer.LightHits(hits, want_amounts=True, **kw)


def same(got, want):
    return lp.same_floats(got[0], want[0]) and lp.same_floats(got[1], want[1])


def with_lights(xrt, tracer, lights, fn):
    kept = list(tracer.Lights)
    set_lights(xrt, tracer, lights)
    try:
        return fn()
    finally:
        del tracer.Lights[:]
        tracer.Lights.extend(kept)


@pytest.mark.parametrize("name", ["crate", "crate_grid", "glass", "heightfield", "content", "two_mesh"])
def test_traced_hits(xrt, name):
    """LightHits(IntersectBatch(primary rays)): both outputs are the checker's, rows in order and shuffled; each output alone is the same."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, name)
    nhit = int(hits["hit"].sum())
    assert 0 < nhit < len(rays)
    got = light_hits(tracer, hits)
    st = dict(tracer.last_stats)
    want = cs.light_hits(hits)
    assert same(got, want[:2]), name
    assert st["shaded_hits"] == nhit == want[2]["live"] and st["pixels"] == len(rays) and st["rays_shadow"] == nhit * len(spec.lights)
    perm = np.random.default_rng(5).permutation(len(rays))
    assert same(light_hits(tracer, hits[perm]), (got[0][perm], got[1][perm])), name + " shuffled"
    assert lp.same_floats(tracer.LightHits(hits), got[0]) and lp.same_floats(tracer.LightHits(hits, want_amounts=True, want_light=False), got[1])


def test_every_branch_of_the_obstruction_test(xrt):
    """RT:485-501: obstructed, free, a Transparent blocker, a blocker beyond the light (on scaled bodies too, where the object-space d differs
    from the world distance) -- asserted from the checker's counts, and the GPU's amounts are the checker's."""
    cfg = xrt.configs
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "crate_grid")
    lights = [cfg.spot((0, 5, 20), angle=6.0)] + list(spec.lights)
    want = cs.light_hits(hits, lights=lights)
    c = want[2]
    assert c["obstructed"] > 0 and c["beyond"] > 0 and c["live"] * len(lights) - c["obstructed"] > 0
    assert same(with_lights(xrt, tracer, lights, lambda: light_hits(tracer, hits)), want[:2])
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "content")
    want = cs.light_hits(hits)
    assert want[2]["transparent"] > 0
    got = light_hits(tracer, hits)
    assert same(got, want[:2])
    assert ((got[1] != 0) & (got[1] != 1)).any(), "no amount is a Transparent blocker's color.W"
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "two_mesh")
    lights = [cfg.spot((-15, 4, -15), angle=6.0)] + list(spec.lights)
    want = cs.light_hits(hits, lights=lights)
    assert want[2]["beyond"] > 0
    assert same(with_lights(xrt, tracer, lights, lambda: light_hits(tracer, hits)), want[:2])


@pytest.mark.parametrize("name", ["crate_grid", "heightfield", "glass"])
def test_identity_with_cast_rays_and_shade_hits(xrt, name):
    """Every colour (1, 1, 1, 1), textures off, MaxReflections 0: RT:726 multiplies the light sum by (1, 1, 1) and by nothing else, so the
    light sum is the colour vector of CastRays and of ShadeHits."""
    spec = specs(xrt)[name]
    scene, tracer = xrt.configs.build_product(spec)
    edits = {i: dict(ids=range(0, d.ntri), color=np.ones((d.ntri, 4), dtype=np.float32)) for i, (d, _) in enumerate(spec.meshes)}
    white = with_triangle_shading(with_materials(spec, {i: dict(use_texture=False) for i in range(len(spec.meshes))}), edits)
    scene.SetMaterials(list(range(len(white.meshes))), [material_struct(m, texels=False)[0] for _, m in white.meshes])
    push(scene, edits)
    tracer.MaxReflections = 0
    rays = ctx(xrt, name)[4]
    hits = scene.IntersectBatch(rays)
    light = tracer.LightHits(hits)
    assert (lp.bits(light) != 0).any()
    assert lp.same_floats(light, tracer.CastRays(rays, want_float=True)[1]), name
    assert lp.same_floats(light, tracer.ShadeHits(rays, hits, want_float=True)[1]), name
    assert lp.same_floats(light, lp.LightsScene(white).light_hits(hits)[0]), name


@pytest.mark.parametrize("n", [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, 100003])
def test_sizes_at_the_kernels_edges(xrt, n):
    spec, cs, scene, tracer, _, _ = ctx(xrt, "crate_grid")
    hits = scene.IntersectBatch(arbitrary_rays(xrt, spec, n))
    got = light_hits(tracer, hits)
    assert same(got, cs.light_hits(hits)[:2]), n
    assert tracer.last_stats["pixels"] == n and tracer.last_stats["shaded_hits"] == int(hits["hit"].sum())


def test_compaction_patterns(xrt):
    """2B + 1 entries that all carry a valid hit, `hit` overwritten: the kernel's ballots, its scan of the block's cells and its reservations
    under every pattern of live lanes."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "crate_grid")
    live = np.flatnonzero(hits["hit"] == 1)
    assert len(live) > 64
    n = 2 * B + 1
    hits = hits[np.resize(live, n)].copy()
    i = np.arange(n)
    rng = np.random.default_rng(9)
    patterns = {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "alternating": i % 2 == 1,
                "one per wave": (i % 64) == ((i // 64) % 64), "first and last lane": ((i % 64) == 0) | ((i % 64) == 63),
                "random": rng.random(n) < 0.37}
    full = None
    for what, mask in patterns.items():
        h = hits.copy()
        h["hit"] = mask.astype(np.int32)
        got = light_hits(tracer, h)
        st = tracer.last_stats
        assert same(got, cs.light_hits(h)[:2]), what
        assert st["shaded_hits"] == int(mask.sum()) and st["rays_shadow"] == int(mask.sum()) * len(spec.lights), what
        assert (lp.bits(got[0][~mask]) == 0).all() and (lp.bits(got[1][~mask]) == 0).all(), what
        if what == "none":
            assert st["rays_traversed"] == 0
        if what == "all":
            full = got
        elif full is not None:
            assert lp.same_floats(got[0][mask], full[0][mask]) and lp.same_floats(got[1][mask], full[1][mask]), what


@pytest.mark.parametrize("count", [0, 1, 2, 33, 128])
def test_light_counts(xrt, monkeypatch, count):
    """0, 1, 2, 33 and 128 lights; under a small shadow budget the list is split into several chunks and the answers are the unsplit call's."""
    cfg = xrt.configs
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "crate_grid")
    lights = [cfg.spot((300.0 * np.cos(0.37 * i), 150.0 + 2.0 * i, 300.0 * np.sin(0.37 * i))) if i % 3 else cfg.directional((0.1 * (i % 7) - 0.3, -1.0, 0.05 * (i % 5)))
              for i in range(count)]
    for l in lights:
        l["intensity"] = 0.02
    n = 2 * 64 + 1 if count == 128 else 2 * B + 1
    pick = np.concatenate([np.resize(np.flatnonzero(hits["hit"] == 1), n - n // 4), np.resize(np.flatnonzero(hits["hit"] == 0), n // 4)])   # three hits to a miss
    h = hits[np.random.default_rng(count).permutation(pick)].copy()
    assert len(h) == n
    want = cs.light_hits(h, lights=lights)
    got = with_lights(xrt, tracer, lights, lambda: light_hits(tracer, h))
    st = dict(tracer.last_stats)
    assert got[1].shape == (n, count) and same(got, want[:2]), count
    assert st["rays_shadow"] == want[2]["live"] * count
    if count == 0:
        assert st["intersect_launches"] == 0 and st["rays_traversed"] == 0 and (lp.bits(got[0]) == 0).all()
        return
    assert st["intersect_launches"] == 1
    monkeypatch.setenv("XRT_SHADOW_BYTES", str(1 << 20))   # (the smallest budget the switch takes: 11915 pairs)
    try:
        small_scene, small_tracer = cfg.build_product(spec)
    finally:
        monkeypatch.delenv("XRT_SHADOW_BYTES")
    big = np.concatenate([h] * (1 + 24000 // (n * count))) if n * count <= 24000 else h
    chunks = -(-len(big) // max(1, (1 << 20) // (88 * count)))
    assert chunks >= 2
    split = with_lights(xrt, small_tracer, lights, lambda: light_hits(small_tracer, big))
    assert small_tracer.last_stats["intersect_launches"] == chunks, count
    unsplit = with_lights(xrt, tracer, lights, lambda: light_hits(tracer, big))
    assert tracer.last_stats["intersect_launches"] == 1
    assert same(split, unsplit), count
    assert same((split[0][:n], split[1][:n]), want[:2]), count
    for k in ("pixels", "shaded_hits", "rays_shadow", "rays_traversed"):
        assert small_tracer.last_stats[k] == tracer.last_stats[k], k


def test_answered_at_emission_switch(xrt, monkeypatch):
    """XRT_AE=0 against the default on the heightfield (one body, one mesh): equal outputs; with it off every pair is traced, with it on no
    more than that."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "heightfield")
    on = light_hits(tracer, hits)
    st_on = dict(tracer.last_stats)
    monkeypatch.setenv("XRT_AE", "0")
    try:
        scene0, tracer0 = xrt.configs.build_product(spec)
    finally:
        monkeypatch.delenv("XRT_AE")
    off = light_hits(tracer0, hits)
    st_off = dict(tracer0.last_stats)
    assert same(on, off) and same(on, cs.light_hits(hits)[:2])
    assert st_off["shaded_hits"] == st_on["shaded_hits"] > 0
    assert st_off["rays_traversed"] == st_off["shaded_hits"] * len(spec.lights)
    assert st_on["rays_traversed"] <= st_off["rays_traversed"]
    for st in (st_on, st_off):
        assert st["rays_shadow"] == st["shaded_hits"] * len(spec.lights)


@pytest.mark.parametrize("name", ["crate_grid", "content", "two_mesh"])
def test_hits_that_are_not_traced_hits(xrt, name):
    """Positions off every surface, arbitrary u / v, a few non-finite entries among finite ones: the checker's answers, and the finite
    neighbours of the non-finite entries are what they are without them."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, name)
    rng = np.random.default_rng(21)
    n = 3000
    h = np.zeros(n, dtype=hits.dtype)
    h["hit"] = (rng.random(n) < 0.8).astype(np.int32) * rng.integers(1, 5, size=n).astype(np.int32)   # (any non-zero word is a hit)
    h["mesh"] = rng.integers(0, len(spec.meshes), size=n)
    h["tri"] = [rng.integers(0, spec.meshes[m][0].ntri) for m in h["mesh"]]
    seen = hits["w"][hits["hit"] == 1]   # (around what the camera sees: inside, between and above the bodies)
    h["w"] = rng.uniform(seen.min(axis=0) - 5.0, seen.max(axis=0) + 5.0, size=(n, 3)).astype(np.float32)
    h["u"], h["v"] = rng.uniform(-0.5, 1.5, size=n).astype(np.float32), rng.uniform(-0.5, 1.5, size=n).astype(np.float32)
    h["object"], h["leaf"], h["d"], h["reserved"] = -5, 10 ** 6, np.float32(np.nan), -1   # not read
    finite = light_hits(tracer, h)
    assert same(finite, cs.light_hits(h)[:2]), name
    odd = h.copy()
    at = np.flatnonzero(h["hit"] != 0)[5::97][:24]
    for k, i in enumerate(at):
        value = (np.nan, np.inf, -np.inf)[k % 3]
        if k % 5 < 3:
            odd["w"][i, k % 5] = value
        else:
            odd[("u", "v")[k % 5 - 3]][i] = value
    got = light_hits(tracer, odd)
    assert same(got, cs.light_hits(odd)[:2]), name
    keep = np.ones(n, dtype=bool); keep[at] = False
    assert same((got[0][keep], got[1][keep]), (finite[0][keep], finite[1][keep])), name


def test_after_edits(xrt):
    """SetPoses, SetMaterials (Transparent and InterpolateNormals toggled) and SetTriangleShading (color.W, normals): the call uses the latest
    values and equals a checker scene built with them."""
    spec = two_mesh_spec(xrt)
    scene, tracer = xrt.configs.build_product(spec)
    rays = ctx(xrt, "two_mesh")[4]
    before = light_hits(tracer, scene.IntersectBatch(rays))
    poses = {0: ((-55.0, 3.0, -58.0), (0.3, 0.1, 0.0), (1.3, 0.9, 1.1)), 7: ((-30.0, 6.0, 2.0), (0.0, 0.5, 0.2), (1.0, 1.4, 1.0)),
             12: ((4.0, 9.0, -3.0), (0.2, 0.2, 0.2), (0.7, 1.2, 1.5))}
    arrays = [pose_arrays(spec, b, *poses[b]) for b in poses]
    scene.SetPoses(list(poses), [a[0] for a in arrays], [a[1] for a in arrays], [a[2] for a in arrays])
    assert xrt.abi.lib().xrt_scene_build_tree(scene.handle, spec.scene_threshold) == 0
    rng = np.random.default_rng(4)
    changes = {0: dict(transparent=True, refraction_index=1.2, interpolate_normals=True), 1: dict(interpolate_normals=False)}
    edits = {}
    for i, (d, _) in enumerate(spec.meshes):
        color = d.color.copy()
        color[:, 3] = rng.uniform(0.05, 0.95, size=d.ntri).astype(np.float32)
        normals = d.n.reshape(d.ntri, 3, 3) + rng.normal(scale=0.2, size=(d.ntri, 3, 3)).astype(np.float32)
        edits[i] = dict(ids=range(0, d.ntri), color=color, normals=normals.astype(np.float32))
    edited = with_triangle_shading(with_materials(moved(spec, poses), changes), edits)
    scene.SetMaterials(list(range(len(edited.meshes))), [material_struct(m, texels=False)[0] for _, m in edited.meshes])
    push(scene, edits)
    hits = scene.IntersectBatch(rays)
    cs = lp.LightsScene(edited)
    o_hits, _ = cs.intersect(rays)
    assert np.array_equal(hits["hit"], o_hits["hit"]) and np.array_equal(hits["tri"], o_hits["tri"])
    got = light_hits(tracer, hits)
    want = cs.light_hits(hits)
    assert want[2]["transparent"] > 0, "no shadow ray meets the crate that became Transparent"
    assert same(got, want[:2])
    assert not lp.same_floats(got[0], before[0])


def test_device_form(xrt):
    """Torch tensors on a non-default stream give the host form's bits; an entry whose mesh or triangle is out of range is a miss and touches
    no other entry; misaligned pointers are XRT_E_INVALID_ARG; each output is nullable on its own."""
    import torch
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "crate_grid")
    host = light_hits(tracer, hits)
    s = torch.cuda.Stream()

    def on_device(h, **kw):
        with torch.cuda.stream(s):
            d_hits = torch.from_numpy(h.view(np.int32).reshape(-1, 12).copy()).to("cuda")
            out = tracer.LightHits(d_hits, device=True, stream=s, **kw)
        s.synchronize()
        return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()
    assert same(on_device(hits, want_amounts=True), host)
    assert lp.same_floats(on_device(hits), host[0])
    assert lp.same_floats(on_device(hits, want_amounts=True, want_light=False), host[1])
    live = np.flatnonzero(hits["hit"] == 1)
    bad = live[:: max(1, len(live) // 40)][:32]
    broken = hits.copy()
    values = [(-1, 0), (-2 ** 31, 0), (2 ** 31 - 1, 0), (len(spec.meshes), 0), (0, -1), (0, -2 ** 31), (0, 2 ** 31 - 1), (0, spec.meshes[0][0].ntri)]
    for k, at in enumerate(bad):
        broken["mesh"][at], broken["tri"][at] = values[k % len(values)]
        broken["object"][at] = (-7, 10 ** 6, 0)[k % 3]
    got = on_device(broken, want_amounts=True)
    st = dict(tracer.last_stats)
    missed = hits.copy()
    missed["hit"][bad] = 0
    assert same(got, light_hits(tracer, missed))
    assert st["shaded_hits"] == len(live) - len(bad) == tracer.last_stats["shaded_hits"]
    keep = np.ones(len(hits), dtype=bool); keep[bad] = False
    assert same((got[0][keep], got[1][keep]), (host[0][keep], host[1][keep]))
    assert (lp.bits(got[0][bad]) == 0).all() and (lp.bits(got[1][bad]) == 0).all()
    # misaligned arrays; the scene's own stream
    lib, abi = xrt.abi.lib(), xrt.abi
    lights, nl = tracer._lights_abi(), len(tracer.Lights)
    raw_h = torch.zeros(64 * 12 + 4, dtype=torch.int32, device="cuda")
    out = torch.full((64 * 3 + 4,), 5.0, dtype=torch.float32, device="cuda")
    amt = torch.full((64 * nl + 4,), 5.0, dtype=torch.float32, device="cuda")
    for dh, do, da in ((8, 0, 0), (0, 4, 0), (0, 0, 4)):
        rc = lib.xrt_light_hits_device(scene.handle, C.c_void_p(raw_h.data_ptr() + dh), 64, lights, nl, C.c_void_p(out.data_ptr() + do),
                                       C.c_void_p(amt.data_ptr() + da), None, None)
        assert rc == abi.XRT_E_INVALID_ARG, (dh, do, da)
    assert (out == 5.0).all() and (amt == 5.0).all()
    rc = lib.xrt_light_hits_device(scene.handle, C.c_void_p(raw_h.data_ptr()), 64, lights, nl, C.c_void_p(out.data_ptr()), C.c_void_p(amt.data_ptr()), None, None)
    assert rc == abi.XRT_OK
    assert (out[:192] == 0).all() and (out[192:] == 5.0).all() and (amt[:64 * nl] == 0).all() and (amt[64 * nl:] == 5.0).all()   # 64 misses


def test_errors_busy_and_stats(xrt):
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "crate")
    lib, abi = xrt.abi.lib(), xrt.abi
    lights, nl = tracer._lights_abi(), len(tracer.Lights)
    n, nhit = len(hits), int(hits["hit"].sum())
    out = np.zeros((n, 3), dtype=np.float32)

    def call(h=hits, count=n, n_lights=nl):
        return lib.xrt_light_hits(scene.handle, h.ctypes.data_as(C.POINTER(abi.xrt_hit)), count, lights, n_lights,
                                  out.ctypes.data_as(C.POINTER(C.c_float)), None, None)
    assert call(count=-1) == abi.XRT_E_INVALID_ARG and call(n_lights=-1) == abi.XRT_E_INVALID_ARG
    assert call(count=0) == abi.XRT_OK
    at = int(np.flatnonzero(hits["hit"] == 1)[0])
    for field, value in (("mesh", 57), ("mesh", -1), ("tri", 10 ** 6), ("tri", -1)):
        bad = hits.copy()
        bad[field][at] = value
        out[:] = 3.0
        assert call(h=bad) == abi.XRT_E_INVALID_ARG, (field, value)
        assert (b"hit %d " % at) in lib.xrt_last_error() and (out == 3.0).all(), (field, value)
    # every field of the stats
    light_hits(tracer, hits)
    st = dict(tracer.last_stats)
    want = dict.fromkeys(st, 0)
    want.update(pixels=n, shaded_hits=nhit, rays_shadow=nhit * nl, intersect_launches=1)
    for k, v in st.items():
        if k in ("ms_total", "ms_intersect"):
            assert v > 0, k
        elif k == "rays_traversed":
            assert 0 < v <= nhit * nl
        else:
            assert v == want[k], (k, v)
    assert st["ms_intersect"] <= st["ms_total"]
    got = with_lights(xrt, tracer, [], lambda: light_hits(tracer, hits))
    st = tracer.last_stats
    assert st["intersect_launches"] == 0 and st["rays_traversed"] == 0 and st["rays_shadow"] == 0 and st["shaded_hits"] == nhit and st["ms_intersect"] == 0
    assert got[1].shape == (n, 0) and (lp.bits(got[0]) == 0).all()
    # a begin/end ticket open: busy; the frame is still right afterwards and the next call works
    frame = np.zeros(spec.width * spec.height, dtype=np.uint32)
    pipe = tracer.PrepareHost(frame)
    t = pipe.begin()
    assert call() == abi.XRT_E_BUSY
    pipe.end(t)
    o_rgba, _, _ = cs.render()
    assert np.array_equal(frame, o_rgba)
    assert same(light_hits(tracer, hits), cs.light_hits(hits)[:2])
