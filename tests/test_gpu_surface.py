"""xrt_surface_hits / xrt_surface_hits_device on the MI355X: what CastRay computes at a hit without asking the scene anything -- the
fragment normal (RT:520-531), the surface colour with its texture lookup (RT:568-581), the material terms, the reflected ray (RT:547-559)
and the Snell refraction (RT:656-694) -- on caller-given hits, bit for bit against the checker (tests/surface: written with the oracle's
own Vector3 operations and SurfaceColor) and against what xrt_shade_hits, xrt_light_hits and xrt_cast_rays_paths compute from the same
hits.  Every comparison is bit for bit; a NaN equals a NaN of any payload."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surface_py as sp
from materials_py import material_struct, with_materials
from test_gpu_cast_rays import scenes, two_mesh_spec
from triangles_py import push, with_triangle_shading

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "xna-ray-trace_amd", "csrc", "surface.h")).read()
# the kernel's entries per block and the most blocks of a launch (csrc/surface.h): list sizes around B cross a wave, a block and, one entry
# past CAP * B, the grid-stride loop
B = int(re.search(r"SURFACE_BLOCK = (\d+);", _SRC).group(1))
CAP = int(re.search(r"SURFACE_MAX_BLOCKS = (\d+);", _SRC).group(1))
NAMES = ["crate", "crate_grid", "glass", "heightfield", "content", "two_mesh"]
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
        cs = sp.SurfaceScene(spec)
        scene, tracer = xrt.configs.build_product(spec)
        rays = cs.primary_rays()
        _CTX[name] = (spec, cs, scene, tracer, rays, scene.IntersectBatch(rays))
    return _CTX[name]


def surface_hits(tracer, hits, rays, cur=1.0, **kw):
    """All three outputs of one call."""
    return tracer.SurfaceHits(hits, rays, currentRefIndex=cur, want_surface=True, want_reflect=True, want_refract=True, **kw)


def to_device(a, words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1, words).copy()).to("cuda")


def to_host(t, dtype):
    return np.ascontiguousarray(t.cpu().numpy()).view(dtype).reshape(-1)


def on_device(xrt, tracer, hits, rays, cur=1.0, stream=None, want=(True, True, True)):
    """The device form on torch tensors -> the wanted outputs as the host form's structured arrays."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d_hits = to_device(hits, 12)
        d_rays = to_device(rays, 8).view(torch.float32) if rays is not None else None
        out = tracer.SurfaceHits(d_hits, d_rays, currentRefIndex=cur, want_surface=want[0], want_reflect=want[1], want_refract=want[2], device=True, stream=s)
    s.synchronize()
    out = out if isinstance(out, tuple) else (out,)
    kinds = [d for d, w in zip((xrt.SURFACE_DTYPE, xrt.RAY_DTYPE, xrt.RAY_DTYPE), want) if w]
    res = tuple(to_host(o, d) for o, d in zip(out, kinds))
    return res if len(res) > 1 else res[0]


def tiled(hits, rays, n, seed):
    """n entries drawn from a scene's (hit, ray) pairs: all of them in turn, then shuffled."""
    pick = np.random.default_rng(seed).permutation(np.resize(np.arange(len(hits)), n))
    return hits[pick].copy(), rays[pick].copy()


@pytest.mark.parametrize("name", NAMES)
def test_traced_hits(xrt, name):
    """SurfaceHits(IntersectBatch(primary rays)): the three outputs are the checker's, rows in order and shuffled; each output asked for alone
    is its part of the joint call."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, name)
    nhit = int((hits["hit"] != 0).sum())
    assert 0 < nhit < len(rays)
    got = surface_hits(tracer, hits, rays)
    st = dict(tracer.last_stats)
    want = cs.surface_hits(hits, rays)
    assert sp.same_outputs(got, want), name
    assert st["shaded_hits"] == nhit == want[3]["live"] and st["pixels"] == len(rays) and st["intersect_launches"] == 0
    perm = np.random.default_rng(5).permutation(len(rays))
    assert sp.same_outputs(surface_hits(tracer, hits[perm], rays[perm]), tuple(g[perm] for g in got)), name + " shuffled"
    assert sp.same_surface(tracer.SurfaceHits(hits), got[0])                                   # (no rays given: none are needed)
    assert sp.same_surface(tracer.SurfaceHits(hits, rays), got[0])
    assert sp.same_rays(tracer.SurfaceHits(hits, rays, want_surface=False, want_reflect=True), got[1])
    assert sp.same_rays(tracer.SurfaceHits(hits, rays, want_surface=False, want_refract=True), got[2])
    r, t = tracer.SurfaceHits(hits, rays, want_surface=False, want_reflect=True, want_refract=True)
    assert sp.same_rays(r, got[1]) and sp.same_rays(t, got[2])
    s, t = tracer.SurfaceHits(hits, rays, want_refract=True)
    assert sp.same_surface(s, got[0]) and sp.same_rays(t, got[2])


def test_the_scenes_cover_every_kind_of_entry(xrt):
    """From the checker's counts on the GPU's hits: the set as a whole has hits and misses, interpolated and flat normals, textured and
    untextured, Transparent and opaque entries."""
    total = dict.fromkeys(sp.COUNTS, 0)
    n = 0
    for name in NAMES:
        spec, cs, scene, tracer, rays, hits = ctx(xrt, name)
        n += len(rays)
        for k, v in cs.surface_hits(hits, rays)[3].items():
            total[k] += v
    assert 0 < total["live"] < n
    for k in ("interpolated", "textured", "transparent"):
        assert 0 < total[k] < total["live"], (k, total)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("filtering", [0, 1])
def test_address_modes_and_filters(xrt, mode, filtering):
    """The textured crate under the 3 address modes x 2 filters, with u, v as traced and pushed beyond the triangle so that uv leaves [0, 1]."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "crate")
    wide = hits.copy()
    wide["u"] = wide["u"] * np.float32(3.0) - np.float32(1.0)
    wide["v"] = wide["v"] * np.float32(-2.5) + np.float32(0.75)
    kept = tracer.AddressMode, tracer.TextureFiltering
    tracer.AddressMode, tracer.TextureFiltering = mode, filtering
    try:
        for h in (hits, wide):
            got = surface_hits(tracer, h, rays)
            want = cs.surface_hits(h, rays, address_mode=mode, filtering=filtering)
            assert (want[0]["flags"][h["hit"] != 0] & sp.SURF_TEXTURED).all()
            assert sp.same_outputs(got, want), (mode, filtering)
    finally:
        tracer.AddressMode, tracer.TextureFiltering = kept


@pytest.mark.parametrize("name", NAMES)
def test_identity_with_light_hits_and_shade_hits(xrt, name):
    """color * LightHits(hits) is the colour vector of ShadeHits(rays, hits) with MaxReflections <= iteration (RT:726)."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, name)
    kept = tracer.MaxReflections
    tracer.MaxReflections = 0
    try:
        rgbf = tracer.ShadeHits(rays, hits, want_float=True)[1]
    finally:
        tracer.MaxReflections = kept
    color = tracer.SurfaceHits(hits)["color"]
    assert (sp.bits(rgbf) != 0).any()
    assert sp.same_floats(color * tracer.LightHits(hits), rgbf), name


@pytest.mark.parametrize("name", ["crate_grid", "glass", "content", "two_mesh"])
def test_identity_with_the_rays_of_cast_rays_paths(xrt, name):
    """CastRays(paths=True) at MaxReflections 1: for a hit that is not Transparent the segments of its ray are (origin, hit) and, where the
    reflection hits, (hit, the reflection's hit) -- the position IntersectBatch finds for reflect_out; for a Transparent hit refract_out is the
    ray the call hands back."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, name)
    surf, refl, refr = surface_hits(tracer, hits, rays)
    kept = tracer.MaxReflections
    tracer.MaxReflections = 1
    try:
        _, vertices, vstart, back = tracer.CastRays(rays, paths=True)
    finally:
        tracer.MaxReflections = kept
    live = hits["hit"] != 0
    t = (surf["flags"] & sp.SURF_TRANSPARENT) != 0
    opaque = np.flatnonzero(live & ~t)
    r_hits = scene.IntersectBatch(refl[opaque])
    count = (vstart[1:] - vstart[:-1])[opaque]
    reached = r_hits["hit"] != 0
    assert np.array_equal(count, np.where(reached, 4, 2)), name
    assert t[live].all() if name == "glass" else reached.any(), name   # (the camera of `glass` sees the glass body alone)
    ends = vertices["position"][vstart[opaque[reached]] + 3]
    assert sp.same_floats(r_hits["w"][reached], ends), name
    assert sp.same_floats(vertices["position"][vstart[opaque[reached]] + 2], refl["o"][opaque[reached]])
    if name in ("glass", "content"):
        assert t.any()
    assert sp.same_floats(back["o"][t], refr["o"][t]) and sp.same_floats(back["d"][t], refr["d"][t]), name


@pytest.mark.parametrize("n", [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, CAP * B + 1])
def test_sizes_at_the_kernels_edges(xrt, n):
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "crate_grid")
    h, r = tiled(hits, rays, n, n)
    got = surface_hits(tracer, h, r)
    assert sp.same_outputs(got, cs.surface_hits(h, r)), n
    assert tracer.last_stats["pixels"] == n and tracer.last_stats["shaded_hits"] == int((h["hit"] != 0).sum())


def test_live_lane_patterns(xrt):
    """2B + 1 entries that all carry a valid hit, `hit` overwritten with 0: the miss path, the divergence within a wave and the wave
    reduction of the count under every pattern of live lanes."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "crate_grid")
    live = np.flatnonzero(hits["hit"] != 0)
    assert len(live) > 64
    n = 2 * B + 1
    pick = np.resize(live, n)
    h0, r = hits[pick].copy(), rays[pick].copy()
    i = np.arange(n)
    patterns = {"all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool), "every other": i % 2 == 1, "every 64th": i % 64 == 0,
                "first wave only": i < 64, "last lane only": i % 64 == 63}
    full = None
    for what, mask in patterns.items():
        h = h0.copy()
        h["hit"] = mask.astype(np.int32)
        got = surface_hits(tracer, h, r)
        assert sp.same_outputs(got, cs.surface_hits(h, r)), what
        assert tracer.last_stats["shaded_hits"] == int(mask.sum()), what
        assert (sp.bits(got[0][~mask]) == 0).all() and (sp.bits(got[1]["d"][~mask]) == 0).all() and (got[2]["ignore_tri"][~mask] == -1).all(), what
        if what == "all":
            full = got
        else:
            assert sp.same_outputs(tuple(g[mask] for g in got), tuple(g[mask] for g in full)), what


def odd_values(hits, rays):
    """Entries with NaN, +-inf and -0.0 in u, v, w and in the ray's direction among finite ones -> (hits, rays, the touched indices)."""
    h, r = hits.copy(), rays.copy()
    at = np.flatnonzero(h["hit"] != 0)[3::41][:40]
    values = (np.nan, np.inf, -np.inf, -0.0)
    for k, i in enumerate(at):
        value = np.float32(values[k % 4])
        where = (k // 4) % 8
        if where < 2:
            h[("u", "v")[where]][i] = value
        elif where < 5:
            h["w"][i, where - 2] = value
        else:
            r["d"][i, where - 5] = value
    return h, r, at


@pytest.mark.parametrize("name", ["crate_grid", "content", "two_mesh"])
def test_values_as_bits(xrt, name):
    """NaN, +-inf and -0.0 in u, v, w and in ray directions give the checker's records and leave every other entry as it is; `hit` values 2
    and -1 are hits; the fields that are not read may hold anything."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, name)
    base = surface_hits(tracer, hits, rays)
    h, r, at = odd_values(hits, rays)
    assert len(at) >= 16
    for filtering in (0, 1):
        kept = tracer.TextureFiltering
        tracer.TextureFiltering = filtering
        try:
            got = surface_hits(tracer, h, r)
            clean = base if filtering == 0 else surface_hits(tracer, hits, rays)
        finally:
            tracer.TextureFiltering = kept
        assert sp.same_outputs(got, cs.surface_hits(h, r, filtering=filtering)), (name, filtering)
        keep = np.ones(len(hits), dtype=bool); keep[at] = False
        assert sp.same_outputs(tuple(g[keep] for g in got), tuple(g[keep] for g in clean)), (name, filtering)
    words = hits.copy()
    live = np.flatnonzero(hits["hit"] != 0)
    words["hit"][live[0::2]], words["hit"][live[1::2]] = 2, -1
    words["object"], words["leaf"], words["d"], words["reserved"] = -9, 10 ** 6, np.float32(np.nan), -1
    junk = rays.copy()
    junk["o"], junk["ignore_mesh"], junk["ignore_tri"] = np.float32(np.nan), 12345, -7
    assert sp.same_outputs(surface_hits(tracer, words, junk), base), name


def test_device_form_range_check_and_guard_words(xrt):
    """The device form: an entry whose mesh or triangle is -1, n_meshes, ntri or INT_MAX is a miss and touches no other entry; nothing is
    written at or behind entry n of any output."""
    import torch
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "two_mesh")
    host = surface_hits(tracer, hits, rays)
    live = np.flatnonzero(hits["hit"] != 0)
    bad = live[:: max(1, len(live) // 40)][:32]
    broken = hits.copy()
    ntri = [d.ntri for d, _ in spec.meshes]
    values = [(-1, 0), (len(spec.meshes), 0), (2 ** 31 - 1, 0), (-2 ** 31, 0), (0, -1), (0, ntri[0]), (1, ntri[1]), (0, 2 ** 31 - 1), (1, -2 ** 31)]
    for k, at in enumerate(bad):
        broken["mesh"][at], broken["tri"][at] = values[k % len(values)]
    got = on_device(xrt, tracer, broken, rays)
    assert tracer.last_stats["shaded_hits"] == len(live) - len(bad)
    missed = hits.copy()
    missed["hit"][bad] = 0
    assert sp.same_outputs(got, surface_hits(tracer, missed, rays))
    keep = np.ones(len(hits), dtype=bool); keep[bad] = False
    assert sp.same_outputs(tuple(g[keep] for g in got), tuple(g[keep] for g in host))
    assert (sp.bits(got[0][bad]) == 0).all() and (got[1]["ignore_mesh"][bad] == -1).all() and (sp.bits(got[2]["o"][bad]) == 0).all()
    # guard words: the arrays hold n + 3 records, the call is told n
    lib, abi = xrt.abi.lib(), xrt.abi
    opts = tracer._opts_abi()
    n = len(hits)
    d_hits, d_rays = to_device(np.concatenate([hits, hits[:3]]), 12), to_device(np.concatenate([rays, rays[:3]]), 8)
    outs = [torch.full((n + 3, w), 0x5a5a5a5a, dtype=torch.int32, device="cuda") for w in (16, 8, 8)]
    for m in (n, n - 1, 1):
        for o in outs:
            o.fill_(0x5a5a5a5a)
        rc = lib.xrt_surface_hits_device(scene.handle, C.c_void_p(d_rays.data_ptr()), C.c_void_p(d_hits.data_ptr()), m, 1.0, C.byref(opts),
                                         *[C.c_void_p(o.data_ptr()) for o in outs], None, None)
        assert rc == abi.XRT_OK, lib.xrt_last_error()
        for o, dt, want in zip(outs, (xrt.SURFACE_DTYPE, xrt.RAY_DTYPE, xrt.RAY_DTYPE), host):
            assert bool((o[m:] == 0x5a5a5a5a).all()), m
            same = sp.same_surface if dt == xrt.SURFACE_DTYPE else sp.same_rays
            assert same(to_host(o[:m].view(torch.float32), dt), want[:m]), m


@pytest.mark.parametrize("name", ["glass", "content"])
def test_every_refraction_branch(xrt, name):
    """RT:656-694 on the Transparent hits: rays from outside and from inside, current_ref_index equal to the material's index and not equal,
    and total internal reflections -- asserted from the checker's counts, then parity."""
    spec, cs, scene, tracer, rays, hits = ctx(xrt, name)
    surf = tracer.SurfaceHits(hits)
    total = dict.fromkeys(sp.COUNTS, 0)
    for what, r, h, cur in sp.refraction_cases(rays, hits, surf):
        want = cs.surface_hits(h, r, ref_index=cur)
        for k, v in want[3].items():
            total[k] += v
        got = surface_hits(tracer, h, r, cur=cur)
        assert sp.same_outputs(got, want), (name, what)
        assert int(np.isnan(got[2]["d"]).any(axis=1).sum()) == want[3]["nan_direction"], what
        # (RT:656-667: n2 is the current index where it equals the material's, else 1 -- which is the current index of these batches)
        assert sp.same_floats(got[0]["next_ref_index"], np.full(len(h), cur, dtype=np.float32)), what
    for k in ("index_equal", "index_differs", "cos_nonneg", "cos_neg", "nan_direction"):
        assert total[k] > 0, (k, total)
    # an opaque hit hands the caller's index on
    cur = 1.75
    got = tracer.SurfaceHits(hits, currentRefIndex=cur)
    opaque = (got["flags"] & (sp.SURF_HIT | sp.SURF_TRANSPARENT)) == sp.SURF_HIT
    assert opaque.any() or name == "glass"   # (the camera of `glass` sees the glass body alone)
    assert (got["next_ref_index"][opaque] == np.float32(cur)).all()
    glassy = (got["flags"] & sp.SURF_TRANSPARENT) != 0
    assert glassy.any() and (got["next_ref_index"][glassy] == np.float32(1.0)).all()   # (1.75 is not the material's index: n2 = 1, RT:663-667)
    assert sp.same_surface(got, cs.surface_hits(hits, ref_index=cur)[0])


def test_after_edits(xrt):
    """SetMaterials (UseTexture off and on, InterpolateNormals, Transparent, RefractionIndex, Reflectiveness) and SetTriangleShading /
    SetTriangleShadingDevice (normals, uv, color): the call uses the latest values and equals a checker scene built with them; a rendered
    frame is the same before and after the call."""
    spec = two_mesh_spec(xrt)
    scene, tracer = xrt.configs.build_product(spec)
    rays = ctx(xrt, "two_mesh")[4]
    hits = scene.IntersectBatch(rays)
    frame = tracer.Render()
    before = surface_hits(tracer, hits, rays)
    assert np.array_equal(tracer.Render(), frame)
    assert sp.same_outputs(before, sp.SurfaceScene(spec).surface_hits(hits, rays))
    steps = [{0: dict(use_texture=False, transparent=True, refraction_index=1.4, reflectiveness=0.3, interpolate_normals=True),
              1: dict(interpolate_normals=False, reflectiveness=0.9)},
             {0: dict(use_texture=True, refraction_index=1.1, reflectiveness=0.65), 1: dict(transparent=True, refraction_index=1.0, reflectiveness=0.0)}]
    cur_spec = spec
    last = before
    for changes in steps:
        cur_spec = with_materials(cur_spec, changes)
        scene.SetMaterials(list(range(len(cur_spec.meshes))), [material_struct(m, texels=False)[0] for _, m in cur_spec.meshes])
        got = surface_hits(tracer, hits, rays)
        want = sp.SurfaceScene(cur_spec).surface_hits(hits, rays)
        assert sp.same_outputs(got, want), changes
        assert not np.array_equal(got[0]["flags"], last[0]["flags"]) and not sp.same_floats(got[0]["reflectiveness"], last[0]["reflectiveness"])
        last = got
    flags = last[0]["flags"][hits["mesh"] == 0]
    assert ((flags & sp.SURF_TEXTURED) != 0)[flags != 0].all() and ((last[0]["flags"] & sp.SURF_TRANSPARENT) != 0)[hits["hit"] != 0].all()
    rng = np.random.default_rng(4)
    for device in (False, True):
        edits = {}
        for i, (d, _) in enumerate(cur_spec.meshes):
            color = rng.uniform(0.05, 0.95, size=(d.ntri, 4)).astype(np.float32)
            normals = d.n.reshape(d.ntri, 3, 3) + rng.normal(scale=0.2, size=(d.ntri, 3, 3)).astype(np.float32)
            uv = rng.uniform(-0.5, 1.5, size=(d.ntri, 3, 2)).astype(np.float32)
            edits[i] = dict(ids=range(0, d.ntri), color=color, normals=normals.astype(np.float32), uv=uv)
        cur_spec = with_triangle_shading(cur_spec, edits)
        push(scene, edits, device=device)
        got = surface_hits(tracer, hits, rays)
        assert sp.same_outputs(got, sp.SurfaceScene(cur_spec).surface_hits(hits, rays)), device
        h = hits["hit"] != 0
        for f in ("normal", "uv", "color", "alpha"):
            assert not sp.same_floats(got[0][f][h], last[0][f][h]), (device, f)
        last = got
    frame = tracer.Render()
    surface_hits(tracer, hits, rays)
    assert np.array_equal(tracer.Render(), frame)


def test_device_form(xrt):
    """Torch tensors on the current and on a non-default stream give the host form's bits, each output alone too; misaligned pointers are
    XRT_E_INVALID_ARG and write nothing; the stats."""
    import torch
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "content")
    host = surface_hits(tracer, hits, rays)
    s = torch.cuda.Stream()
    assert sp.same_outputs(on_device(xrt, tracer, hits, rays), host)
    assert sp.same_outputs(on_device(xrt, tracer, hits, rays, stream=s), host)
    st = dict(tracer.last_stats)
    nhit = int((hits["hit"] != 0).sum())
    want = dict.fromkeys(st, 0)
    want.update(pixels=len(hits), shaded_hits=nhit, intersect_launches=0)
    for k, v in st.items():
        if k == "ms_total":
            assert v > 0
        else:
            assert v == want[k], (k, v)
    assert sp.same_surface(on_device(xrt, tracer, hits, None, stream=s, want=(True, False, False)), host[0])
    assert sp.same_rays(on_device(xrt, tracer, hits, rays, stream=s, want=(False, True, False)), host[1])
    assert sp.same_rays(on_device(xrt, tracer, hits, rays, stream=s, want=(False, False, True)), host[2])
    cur = float(host[0]["refraction_index"][(host[0]["flags"] & sp.SURF_TRANSPARENT) != 0][0])
    assert sp.same_outputs(on_device(xrt, tracer, hits, rays, cur=cur, stream=s), surface_hits(tracer, hits, rays, cur=cur))
    # misaligned arrays
    lib, abi = xrt.abi.lib(), xrt.abi
    opts = tracer._opts_abi()
    raw_h = torch.zeros(64 * 12 + 4, dtype=torch.int32, device="cuda")
    raw_r = torch.zeros(64 * 8 + 4, dtype=torch.float32, device="cuda")
    outs = [torch.full((64 * w + 4,), 5.0, dtype=torch.float32, device="cuda") for w in (16, 8, 8)]
    for k in range(5):
        off = [0] * 5
        off[k] = (4, 8, 12)[k % 3]
        rc = lib.xrt_surface_hits_device(scene.handle, C.c_void_p(raw_r.data_ptr() + off[0]), C.c_void_p(raw_h.data_ptr() + off[1]), 64, 1.0, C.byref(opts),
                                         *[C.c_void_p(o.data_ptr() + d) for o, d in zip(outs, off[2:])], None, None)
        assert rc == abi.XRT_E_INVALID_ARG and b"16-byte" in lib.xrt_last_error(), k
    assert all(bool((o == 5.0).all()) for o in outs)
    rc = lib.xrt_surface_hits_device(scene.handle, C.c_void_p(raw_r.data_ptr()), C.c_void_p(raw_h.data_ptr()), 64, 1.0, C.byref(opts),
                                     *[C.c_void_p(o.data_ptr()) for o in outs], None, None)   # the scene's own stream; 64 misses
    assert rc == abi.XRT_OK
    assert bool((outs[0][:64 * 16] == 0).all()) and bool((outs[0][64 * 16:] == 5.0).all())
    miss = to_host(outs[1][:64 * 8].reshape(64, 8), xrt.RAY_DTYPE)
    assert (sp.bits(miss["o"]) == 0).all() and (sp.bits(miss["d"]) == 0).all() and (miss["ignore_mesh"] == -1).all() and (miss["ignore_tri"] == -1).all()
    assert bool((outs[1][64 * 8:] == 5.0).all()) and bool((outs[2][64 * 8:] == 5.0).all())


def test_errors_and_busy(xrt):
    spec, cs, scene, tracer, rays, hits = ctx(xrt, "crate")
    lib, abi = xrt.abi.lib(), xrt.abi
    opts = tracer._opts_abi()
    n = len(hits)
    out = np.zeros(n, dtype=xrt.SURFACE_DTYPE)

    def call(h=hits, count=n, o=opts):
        return lib.xrt_surface_hits(scene.handle, None, h.ctypes.data_as(C.POINTER(abi.xrt_hit)), count, 1.0, C.byref(o) if o is not None else None,
                                    out.ctypes.data_as(C.POINTER(abi.xrt_surface)), None, None, None)
    assert call(count=-1) == abi.XRT_E_INVALID_ARG and call(o=None) == abi.XRT_E_INVALID_ARG
    assert call(count=0) == abi.XRT_OK
    at = int(np.flatnonzero(hits["hit"] != 0)[0])
    for field, value in (("mesh", 57), ("mesh", -1), ("tri", 10 ** 6), ("tri", -1)):
        bad = hits.copy()
        bad[field][at] = value
        out["flags"] = 3
        assert call(h=bad) == abi.XRT_E_INVALID_ARG, (field, value)
        assert (b"hit %d " % at) in lib.xrt_last_error() and (out["flags"] == 3).all(), (field, value)
    # a begin/end ticket open: busy; the frame is still right afterwards and the next call works
    frame = np.zeros(spec.width * spec.height, dtype=np.uint32)
    pipe = tracer.PrepareHost(frame)
    t = pipe.begin()
    assert call() == abi.XRT_E_BUSY
    pipe.end(t)
    o_rgba, _, _ = cs.render()
    assert np.array_equal(frame, o_rgba)
    assert sp.same_outputs(surface_hits(tracer, hits, rays), cs.surface_hits(hits, rays))
