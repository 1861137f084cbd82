"""xrt_compose_hits / xrt_fold_samples and their device forms on the MI355X: the return path of CastRay, one level (RT:584, 699, 705, 726,
732), and the RT:309 fold on caller-given terms, bit for bit against the checker (tests/compose: written with the oracle's own Lerp,
ColorFromVector3 and ColorToVector3) -- on the checkers' own arrays, on a synthetic table of edge values at the sizes where the kernel can go
wrong -- and in the identities the calls exist for: composed from the product's own SurfaceHits, LightHits and CastRays they are ShadeHits,
CastRays and RenderPixels, and the oracle's CastRay and frames.  Every comparison is bit for bit; a NaN equals a NaN of any payload."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import compose_py as cp
import lights_py as lp
import pixels_py as px
import surface_py as sp
from test_gpu_cast_rays import scenes, two_mesh_spec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "xna-ray-trace_amd", "csrc", "compose.h")).read()
# the kernel's entries per block and the most blocks of a launch (csrc/compose.h): list sizes around B cross a wave and a block and, one entry
# past CAP * B, the grid-stride loop
B = int(re.search(r"COMPOSE_BLOCK = (\d+);", _SRC).group(1))
CAP = int(re.search(r"COMPOSE_MAX_BLOCKS = (\d+);", _SRC).group(1))
NAMES = ["crate", "crate_grid", "glass", "heightfield", "content", "two_mesh"]
GUARD = 0x5a5a5a5a
_CTX = {}


def specs(xrt):
    out = dict(scenes(xrt))
    out["two_mesh"] = two_mesh_spec(xrt)
    return out


def ctx(xrt, name):
    """(spec, the surface checker's scene, the light checker's scene, product scene, tracer, the camera's rays) of a scene, made once."""
    if name not in _CTX:
        spec = specs(xrt)[name]
        cs = sp.SurfaceScene(spec)
        scene, tracer = xrt.configs.build_product(spec)
        _CTX[name] = (spec, cs, lp.LightsScene(spec), scene, tracer, cs.primary_rays())
    return _CTX[name]


def to_device(a, words=None):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32).reshape(-1).copy()).to("cuda")
    return t.reshape(-1, words) if words else t


def compose(xrt, scene, surf, light, reflect=None, refract=None, want=(True, True), device=False, stats=None):
    """xrt_compose_hits or, with device, xrt_compose_hits_device on fresh tensors, through ctypes -> (rgba or None, rgbf or None)."""
    lib, abi = xrt.abi.lib(), xrt.abi
    n = len(surf)
    st = abi.xrt_stats()
    if device:
        import torch
        d = [to_device(surf, 16).view(torch.float32), to_device(light, 3).view(torch.float32)] + [to_device(c) if c is not None else None for c in (reflect, refract)]
        rgba = torch.full((n,), GUARD, dtype=torch.int32, device="cuda") if want[0] else None
        rgbf = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda") if want[1] else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        rc = lib.xrt_compose_hits_device(scene.handle, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), n, ptr(rgba), ptr(rgbf), None, C.byref(st))
        assert rc == abi.XRT_OK, lib.xrt_last_error()
        out = (rgba.cpu().numpy().view(np.uint32) if want[0] else None, rgbf.cpu().numpy() if want[1] else None)
    else:
        surf, light = np.ascontiguousarray(surf, dtype=xrt.SURFACE_DTYPE), np.ascontiguousarray(light, dtype=np.float32)
        rgba = np.full(n, GUARD, dtype=np.uint32) if want[0] else None
        rgbf = np.full((n, 3), 7.0, dtype=np.float32) if want[1] else None
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)) if a is not None else None
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
        rc = lib.xrt_compose_hits(scene.handle, surf.ctypes.data_as(C.POINTER(abi.xrt_surface)), fp(light), up(reflect), up(refract), n, up(rgba), fp(rgbf), C.byref(st))
        assert rc == abi.XRT_OK, lib.xrt_last_error()
        out = (rgba, rgbf)
    if stats is not None:
        stats.update(st.as_dict())
    return out


def same(got, want):
    """(rgba or None, rgbf or None) against the checker's (rgba, rgbf, ...)."""
    return (got[0] is None or np.array_equal(got[0], want[0])) and (got[1] is None or cp.same_floats(got[1], want[1]))


class Recording(cp.OracleOps):
    """cast_by_hand on the checkers, keeping what it hands to the composition."""

    def compose(self, surface, light, reflect, refract):
        self.last = (surface, light, reflect, refract)
        return super().compose(surface, light, reflect, refract)


class ProductOps(cp.HandOps):
    """cast_by_hand on the product's host forms (tracer.MaxReflections is what CastRays is given)."""

    def __init__(self, scene, tracer, abi=None):
        self.scene, self.tracer, self.abi = scene, tracer, abi

    def intersect(self, rays): return self.scene.IntersectBatch(rays)
    def surface(self, hits, rays, ref_index): return self.tracer.SurfaceHits(hits, rays, currentRefIndex=ref_index, want_surface=True, want_reflect=True, want_refract=True)
    def light(self, hits): return self.tracer.LightHits(hits)
    def cast(self, rays, iteration, ref_index): return self.tracer.CastRays(rays, iteration, ref_index)
    def compose(self, surface, light, reflect, refract): return self.tracer.ComposeHits(surface, light, reflect, refract, want_float=True)


class DeviceOps(ProductOps):
    """The same on torch tensors: rays float32 (n, 8), hits int32 (n, 12), surface records float32 (n, 16), colours int32 (n)."""

    def intersect(self, rays):
        import torch
        lib = self.abi.lib()
        hits = torch.empty((len(rays), 12), dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream()
        assert lib.xrt_scene_intersect_device(self.scene.handle, C.c_void_p(rays.data_ptr()), len(rays), C.c_void_p(hits.data_ptr()), C.c_void_p(s.cuda_stream)) == 0
        s.synchronize()
        return hits

    def surface(self, hits, rays, ref_index):
        return self.tracer.SurfaceHits(hits, rays, currentRefIndex=ref_index, want_surface=True, want_reflect=True, want_refract=True, device=True)

    def light(self, hits): return self.tracer.LightHits(hits, device=True)
    def cast(self, rays, iteration, ref_index): return self.tracer.CastRays(rays, iteration, ref_index, device=True)
    def compose(self, surface, light, reflect, refract): return self.tracer.ComposeHits(surface, light, reflect, refract, want_float=True, device=True)

    def colors(self, n):
        import torch
        return torch.zeros(n, dtype=torch.int32, device="cuda")

    def flags(self, surface):
        import torch
        return surface[:, 12].contiguous().view(torch.int32)

    def next_index(self, surface): return surface[:, 11].contiguous()

    def where(self, mask):
        import torch
        return torch.nonzero(mask).reshape(-1)

    def values(self, x): return sorted(set(x.cpu().tolist()))


def host(pair):
    """(rgba, rgbf) of either path as numpy arrays."""
    rgba, rgbf = pair
    if not isinstance(rgba, np.ndarray):
        rgba, rgbf = rgba.cpu().numpy(), rgbf.cpu().numpy()
    return rgba.view(np.uint32), rgbf


@pytest.mark.parametrize("name", NAMES)
def test_checker_inputs(xrt, name):
    """Host and device forms on the arrays the checkers' own recursion hands to its composition (surface records, light sums, the colours of
    orc_cast_rays on the next rays) equal orc_compose_hits: RT:726, RT:584 without and with the refraction, each output alone and both."""
    spec, cs, ls, scene, tracer, rays = ctx(xrt, name)
    ops = Recording(spec, 2, cs, ls)
    cp.cast_by_hand(ops, rays, 0, 2)
    surf, light, reflect, refract = ops.last
    assert 0 < int(((surf["flags"] & cp.SURF_HIT) != 0).sum()) < len(rays)
    for a, b in ((None, None), (reflect, None), (reflect, refract)):
        want = cp.compose_hits(surf, light, a, b)
        for device in (False, True):
            for outs in ((True, True), (True, False), (False, True)):
                assert same(compose(xrt, scene, surf, light, a, b, want=outs, device=device), want), (name, a is not None, b is not None, device, outs)
    if name in ("glass", "content"):
        assert cp.compose_hits(surf, light, reflect, refract)[2]["refracted"] > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, CAP * B + 1])
def test_edge_table_at_the_kernels_edges(xrt, n):
    """The synthetic table (every flag combination, NaN / inf / -0.0 / out-of-range channels, products on the RGBA8 halves, all byte values of
    the colours), tiled to n entries and shuffled: every branch equals the checker; a permuted list gives permuted answers."""
    spec, cs, ls, scene, tracer, rays = ctx(xrt, "crate")
    surf, light, reflect, refract = cp.tiled_table(n, seed=n)
    big = n > 4 * B
    for a, b in ((reflect, refract),) if big else ((None, None), (reflect, None), (reflect, refract)):
        want = cp.compose_hits(surf, light, a, b)
        st = {}
        got = compose(xrt, scene, surf, light, a, b, device=True, stats=st)
        assert same(got, want), (n, a is not None, b is not None)
        assert st["pixels"] == n and st["shaded_hits"] == want[2]["hit"] and st["intersect_launches"] == 0
        if not big:
            assert same(compose(xrt, scene, surf, light, a, b), want), n
        perm = np.random.default_rng(n + 1).permutation(n)
        again = compose(xrt, scene, surf[perm], light[perm], a[perm] if a is not None else None, b[perm] if b is not None else None, device=True)
        assert np.array_equal(again[0], got[0][perm]) and cp.same_floats(again[1], got[1][perm]), n


def test_whole_table_in_order(xrt):
    """The table as it is (its classes at known rows), both forms, through the Python binding too."""
    spec, cs, ls, scene, tracer, rays = ctx(xrt, "crate")
    surf, light, reflect, refract, classes = cp.edge_table()
    import torch
    side = torch.cuda.Stream()
    for a, b in ((None, None), (reflect, None), (reflect, refract)):
        want = cp.compose_hits(surf, light, a, b)
        assert same(tracer.ComposeHits(surf, light, a, b, want_float=True), want)
        assert np.array_equal(tracer.ComposeHits(surf, light, a, b), want[0])
        torch.cuda.synchronize()   # (the uploads below are made on the current stream, the call on another)
        d = tracer.ComposeHits(to_device(surf, 16).view(torch.float32), to_device(light, 3).view(torch.float32), to_device(a) if a is not None else None,
                               to_device(b) if b is not None else None, want_float=True, device=True, stream=side)
        assert same(host(d), want)
        for k, rows in classes.items():
            assert np.array_equal(host(d)[0][rows], want[0][rows]), k


def test_in_place_and_guard_words(xrt):
    """The device form with d_rgba_out being d_reflect_rgba, or d_refract_rgba, equals the out-of-place result; nothing is written at or
    behind entry n of either output, for n on and off the block size."""
    import torch
    spec, cs, ls, scene, tracer, rays = ctx(xrt, "crate")
    lib, abi = xrt.abi.lib(), xrt.abi
    n = 2 * B + 37
    surf, light, reflect, refract = cp.tiled_table(n + 3, seed=11)
    d_surf, d_light = to_device(surf, 16).view(torch.float32), to_device(light, 3).view(torch.float32)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    for m in (n, 2 * B, B - 1, 1):
        want = cp.compose_hits(surf[:m], light[:m], reflect[:m], refract[:m])
        for alias in (None, "reflect", "refract"):
            d_reflect, d_refract = to_device(reflect), to_device(refract)
            d_rgba = {None: torch.full((n + 3,), GUARD, dtype=torch.int32, device="cuda"), "reflect": d_reflect, "refract": d_refract}[alias]
            d_f32 = torch.full((n + 3, 3), 7.0, dtype=torch.float32, device="cuda")
            rc = lib.xrt_compose_hits_device(scene.handle, ptr(d_surf), ptr(d_light), ptr(d_reflect), ptr(d_refract), m, ptr(d_rgba), ptr(d_f32), None, None)
            assert rc == abi.XRT_OK, lib.xrt_last_error()
            got = d_rgba.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:m], want[0]) and cp.same_floats(d_f32.cpu().numpy()[:m], want[1]), (m, alias)
            behind = {None: np.full(n + 3 - m, GUARD, dtype=np.uint32), "reflect": reflect[m:], "refract": refract[m:]}[alias]
            assert np.array_equal(got[m:], behind) and bool((d_f32[m:] == 7.0).all()), (m, alias)
            if alias != "reflect":
                assert np.array_equal(d_reflect.cpu().numpy().view(np.uint32), reflect)     # (inputs are not written)
            if alias != "refract":
                assert np.array_equal(d_refract.cpu().numpy().view(np.uint32), refract)
    # the fold: n + 3 entries of sixteen, told n
    colours = np.resize(np.concatenate([reflect, refract]), 16 * (n + 3)).astype(np.uint32)
    d_in = to_device(colours)
    for samples in (4, 16):
        for m in (n, B, 1):
            d_rgba = torch.full((n + 3,), GUARD, dtype=torch.int32, device="cuda")
            d_f32 = torch.full((n + 3, 3), 7.0, dtype=torch.float32, device="cuda")
            rc = lib.xrt_fold_samples_device(scene.handle, ptr(d_in), m, samples, ptr(d_rgba), ptr(d_f32), None, None)
            assert rc == abi.XRT_OK, lib.xrt_last_error()
            want = cp.fold_samples(colours[:m * samples], samples)
            assert np.array_equal(d_rgba.cpu().numpy().view(np.uint32)[:m], want[0]) and cp.same_bits(d_f32.cpu().numpy()[:m], want[1]), (samples, m)
            assert bool((d_rgba[m:] == GUARD).all()) and bool((d_f32[m:] == 7.0).all()), (samples, m)


@pytest.mark.parametrize("name", NAMES)
def test_identity_with_shade_hits(xrt, name):
    """ComposeHits(SurfaceHits(h), LightHits(h)) is ShadeHits(rays, h) with MaxReflections <= iteration (RT:726), and the oracle's CastRay."""
    spec, cs, ls, scene, tracer, rays = ctx(xrt, name)
    hits = scene.IntersectBatch(rays)
    kept = tracer.MaxReflections
    tracer.MaxReflections = 0
    try:
        shaded = tracer.ShadeHits(rays, hits, want_float=True)
    finally:
        tracer.MaxReflections = kept
    got = tracer.ComposeHits(tracer.SurfaceHits(hits), tracer.LightHits(hits), want_float=True)
    st = dict(tracer.last_stats)
    assert np.array_equal(got[0], shaded[0]) and cp.same_floats(got[1], shaded[1]), name
    o_rgba, o_rgbf, _ = cs.cast_rays(rays, max_reflections=0)
    assert np.array_equal(got[0], o_rgba) and cp.same_floats(got[1], o_rgbf), name
    assert len(np.unique(o_rgba)) > 3
    # the stats: pixels, shaded_hits, a time, and nothing else
    want = dict.fromkeys(st, 0)
    want.update(pixels=len(rays), shaded_hits=int((hits["hit"] != 0).sum()), intersect_launches=0)
    for k, v in st.items():
        assert (v > 0) if k == "ms_total" else (v == want[k]), (k, v)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["glass", "content", "crate_grid", "two_mesh"])
def test_the_recursion_by_hand(xrt, name, device):
    """Product calls only: TracePixels / IntersectBatch, SurfaceHits, LightHits, CastRays on the next rays at iteration + 1 (the refraction
    grouped by next_ref_index), ComposeHits -- equals CastRays and the oracle's CastRay on the same rays.  On `glass` at MaxReflections 2 once
    more with no CastRays call at all."""
    import torch
    spec, cs, ls, scene, tracer, rays = ctx(xrt, name)
    kept = tracer.MaxReflections
    try:
        if device:
            ops = DeviceOps(scene, tracer, xrt.abi)
            centers = torch.from_numpy(px.grid_centers(spec.width, spec.height)).to("cuda")
            d_rays, d_hits = tracer.TracePixels(centers, device=True)
            d_rays = d_rays.view(torch.float32)
            rays = np.ascontiguousarray(d_rays.cpu().numpy()).view(xrt.RAY_DTYPE).reshape(-1)
        else:
            ops, d_rays, d_hits = ProductOps(scene, tracer), rays, None
        levels = [(0, 1, 1), (1, 3, 1)] + ([(0, 2, 99)] if name == "glass" else [])
        for iteration, m, hand_levels in levels:
            tracer.MaxReflections = m
            ops.cast_calls = 0
            got = host(cp.cast_by_hand(ops, d_rays, iteration, m, hand_levels=hand_levels, hits=d_hits if iteration == 0 else None))
            assert (ops.cast_calls == 0) == (hand_levels > 1)
            o_rgba, o_rgbf, _ = cs.cast_rays(rays, iteration=iteration, max_reflections=m)
            assert np.array_equal(got[0], o_rgba) and cp.same_floats(got[1], o_rgbf), (name, iteration, m, "oracle")
            p = tracer.CastRays(rays, iteration, want_float=True)
            assert np.array_equal(got[0], p[0]) and cp.same_floats(got[1], p[1]), (name, iteration, m, "CastRays")
            assert len(np.unique(o_rgba)) > 3
    finally:
        tracer.MaxReflections = kept


@pytest.mark.parametrize("name", ["crate_grid", "glass"])
def test_fold_is_render_pixels_fixed16(xrt, orc, name):
    """FoldSamples(ShadeHits(*TracePixels(c, fixed16=True))) is RenderPixels(c) with XRT_MS_FIXED16, in rgba and float, on pixels across an
    edge, and the oracle's frame there; samples = 4 against the checker; both forms."""
    import torch
    from test_compose_cpu import edge_pixels
    spec, cs, ls, scene, tracer, rays = ctx(xrt, name)
    osc = orc.OracleScene(spec)
    f16, f16f = px.oracle_frame(orc, osc, px.with_mode(spec, xrt.abi.MS_FIXED16))
    centers = edge_pixels(f16)
    colours = tracer.ShadeHits(*tracer.TracePixels(centers, fixed16=True))
    assert colours.shape == (16 * len(centers),)
    assert sum(len(set(colours[16 * i:16 * i + 16].tolist())) > 1 for i in range(len(centers))) >= 4
    got = tracer.FoldSamples(colours, want_float=True)
    assert tracer.last_stats["pixels"] == len(centers) and tracer.last_stats["shaded_hits"] == 0 and tracer.last_stats["intersect_launches"] == 0
    kept = tracer.UseMultisampling, tracer.MultisampleMode
    tracer.UseMultisampling, tracer.MultisampleMode = True, xrt.abi.MS_FIXED16
    try:
        want = tracer.RenderPixels(centers, want_float=True)
    finally:
        tracer.UseMultisampling, tracer.MultisampleMode = kept
    assert np.array_equal(got[0], want[0]) and cp.same_bits(got[1], want[1]), name
    x, y = centers[:, 0].astype(int), centers[:, 1].astype(int)
    assert np.array_equal(got[0], f16[y, x]) and cp.same_bits(got[1], f16f[y, x]), name
    assert np.array_equal(tracer.FoldSamples(colours), got[0])
    for samples in (4, 16):
        want = cp.fold_samples(colours, samples)
        h = tracer.FoldSamples(colours, samples=samples, want_float=True)
        d = tracer.FoldSamples(to_device(colours), samples=samples, want_float=True, device=True)
        assert np.array_equal(h[0], want[0]) and cp.same_bits(h[1], want[1]), samples
        assert np.array_equal(host(d)[0], want[0]) and cp.same_bits(host(d)[1], want[1]), samples


_PIX = open(os.path.join(ROOT, "xna-ray-trace_amd", "csrc", "pixels.hip")).read()
# the fold is k_pixel_resolve (csrc/pixels.hip): its block size, and the most blocks launch_pixel_resolve gives it
FB = int(re.search(r"constexpr int PIXEL_BLOCK = (\d+);", _PIX).group(1))
FCAP = int(re.search(r"void launch_pixel_resolve\(.*?if \(blocks > (\d+)\) blocks = \1;", _PIX, flags=re.S).group(1))


@pytest.mark.parametrize("n", [1, FB - 1, FB, FB + 1, FCAP * FB + 1])
def test_fold_sizes(xrt, n):
    """The fold of n entries of arbitrary colours (all byte values in every channel), samples 4 and 16, around its block size and one entry past
    its grid."""
    spec, cs, ls, scene, tracer, rays = ctx(xrt, "crate")
    samples = 4 if n > 10 ** 6 else 16
    i = np.arange(n * samples, dtype=np.uint32)
    colours = (i * np.uint32(2654435761)) ^ (i >> np.uint32(7))
    for k in ((samples,) if n > 10 ** 6 else (4, 16)):
        want = cp.fold_samples(colours[:n * k], k)
        got = tracer.FoldSamples(to_device(colours[:n * k]), samples=k, want_float=True, device=True)
        assert np.array_equal(host(got)[0], want[0]) and cp.same_bits(host(got)[1], want[1]), (n, k)
        assert tracer.last_stats["pixels"] == n


def test_errors_and_busy(xrt):
    """On a scene with a device: misaligned arrays in the device forms are XRT_E_INVALID_ARG and write nothing; with a begin / end ticket open
    every form is XRT_E_BUSY, the frame is right afterwards and the next call works."""
    import torch
    spec, cs, ls, scene, tracer, rays = ctx(xrt, "crate")
    lib, abi = xrt.abi.lib(), xrt.abi
    n = 64
    surf, light, reflect, refract = cp.tiled_table(n, seed=5)
    raw = [torch.zeros(n * w + 4, dtype=torch.int32, device="cuda") for w in (16, 3, 1, 1)]
    outs = [torch.full((n * w + 4,), GUARD, dtype=torch.int32, device="cuda") for w in (1, 3)]
    for k in range(6):
        off = [0] * 6
        off[k] = (4, 8, 12)[k % 3]
        p = [C.c_void_p(t.data_ptr() + d) for t, d in zip(raw + outs, off)]
        assert lib.xrt_compose_hits_device(scene.handle, p[0], p[1], p[2], p[3], n, p[4], p[5], None, None) == abi.XRT_E_INVALID_ARG, k
        assert b"16-byte" in lib.xrt_last_error(), k
    fold_in = torch.zeros(16 * n + 4, dtype=torch.int32, device="cuda")
    for k in range(3):
        off = [0] * 3
        off[k] = (4, 8, 12)[k]
        p = [C.c_void_p(t.data_ptr() + d) for t, d in zip([fold_in] + outs, off)]
        assert lib.xrt_fold_samples_device(scene.handle, p[0], n, 16, p[1], p[2], None, None) == abi.XRT_E_INVALID_ARG and b"16-byte" in lib.xrt_last_error(), k
    assert all(bool((o == GUARD).all()) for o in outs)
    colours = np.zeros(16 * n, dtype=np.uint32)
    frame = np.zeros(spec.width * spec.height, dtype=np.uint32)
    pipe = tracer.PrepareHost(frame)
    t = pipe.begin()
    for call in (lambda: tracer.ComposeHits(surf, light), lambda: tracer.ComposeHits(surf, light, reflect, refract), lambda: tracer.FoldSamples(colours),
                 lambda: tracer.ComposeHits(to_device(surf, 16).view(torch.float32), to_device(light, 3).view(torch.float32), device=True),
                 lambda: tracer.FoldSamples(to_device(colours), device=True)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "busy" in str(e.value)
    pipe.end(t)
    o_rgba, _, _ = cs.render()
    assert np.array_equal(frame, o_rgba)
    assert same(tracer.ComposeHits(surf, light, reflect, refract, want_float=True), cp.compose_hits(surf, light, reflect, refract))
