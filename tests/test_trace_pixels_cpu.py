"""xrt_trace_pixels (the ray of RT:412-421 and the IntersectionResult of RT:512 for caller-chosen pixels, nothing shaded) without a GPU: the exports in
every binding, the order of the argument errors on a host-only scene, the expectation of the GPU test pinned on the oracle alone (tests/trace_py.py: the
k-times frame and the shifted viewport give the ray of any listed centre; the oracle's CastRay on those rays is the oracle frames' pixels), the conditions
the GPU test's lists must meet, and the chunk plan (csrc/trace_plan.h) at its edges in a host program under ASan and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import castray_py
import pixels_py as px
import trace_py as tp
from test_gpu_packet_quads import hf_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("xrt_trace_pixels", "xrt_trace_pixels_device")
_F = C.POINTER(C.c_float)


def test_exports_are_in_the_library_the_header_and_every_binding(xrt):
    hdr = open(os.path.join(ROOT, "include", "xrt.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "XrtNative.cs")).read()
    raw = C.CDLL(xrt.abi.LIB_PATH)
    for name in EXPORTS:
        assert hasattr(raw, name), name
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in xrt.abi.SYMBOLS, name
        assert re.search(r"CallingConvention = CallingConvention\.Cdecl\)\] public static extern (?:unsafe )?int %s\(" % name, cs), name
    assert "#define XRT_VERSION 203" in hdr and xrt.abi.lib().xrt_version() == 203
    gsm = open(os.path.join(ROOT, "csharp", "GpuSpatialManager.cs")).read()
    assert "xrt_trace_pixels" in gsm and re.search(r"public void TracePixels\(", gsm) and "picking seam" in gsm
    assert callable(getattr(xrt.RayTracer, "TracePixels", None))


def test_the_header_is_still_strict_c99(tmp_path):
    """The whole header, with the new declarations, through a C compiler in pedantic C99 (as tests/c_host does for the product)."""
    src = tmp_path / "hdr.c"
    src.write_text('#include "xrt.h"\n'
                   'typedef int (*host_form)(xrt_scene *, const xrt_camera *, const xrt_render_opts *, const float *, int64_t, xrt_ray *, xrt_hit *, xrt_stats *);\n'
                   'typedef int (*device_form)(xrt_scene *, const xrt_camera *, const xrt_render_opts *, const void *, int64_t, void *, void *, void *, xrt_stats *);\n'
                   'int main(void) { host_form h = xrt_trace_pixels; device_form d = xrt_trace_pixels_device; return h(0, 0, 0, 0, 0, 0, 0, 0) + d(0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-4000:]


@pytest.fixture(scope="module")
def host_only(xrt):
    spec = xrt.configs.crate_scene(8, 8, max_reflections=1)
    scene, tracer = xrt.configs.build_product(spec, device=-1)
    return scene, tracer


def test_argument_errors_come_in_order_and_before_the_device(xrt, host_only):
    scene, tracer = host_only
    abi, lib = xrt.abi, xrt.abi.lib()
    bad = abi.XRT_E_INVALID_ARG
    ok = np.array([[1.0, 2.0], [3.5, -4.0]], dtype=np.float32)
    rays, hits = np.zeros(2, dtype=xrt.api.RAY_DTYPE), np.zeros(2, dtype=xrt.api.HIT_DTYPE)

    def opts(**kw):
        o = tracer._opts_abi(shard_count=0)
        o.n_gpus, o.use_multisampling = 0, abi.MS_OFF
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def host(c=ok, n=2, o=None, cam=True, r=True, h=True, sc=True):
        camera, o = tracer._camera_abi(), (o or opts())
        return lib.xrt_trace_pixels(scene.handle if sc else None, C.byref(camera) if cam else None, C.byref(o) if o != "null" else None,
                                    None if c is None else c.ctypes.data_as(_F), n, rays.ctypes.data_as(C.POINTER(abi.xrt_ray)) if r else None,
                                    hits.ctypes.data_as(C.POINTER(abi.xrt_hit)) if h else None, None)

    def dev(c=0x1000, n=2, o=None, cam=True, r=0x2000, h=0x3000, sc=True):
        # (no device memory here: the pointers only have to look like device pointers -- nothing reads them before the scene is looked at)
        camera, o = tracer._camera_abi(), (o or opts())
        return lib.xrt_trace_pixels_device(scene.handle if sc else None, C.byref(camera) if cam else None, C.byref(o) if o != "null" else None,
                                           C.c_void_p(c), n, C.c_void_p(r or None), C.c_void_p(h or None), None, None)
    err = lib.xrt_last_error
    for call, none in ((host, None), (dev, 0)):
        assert call(sc=False, n=-1) == bad and b"null scene" in err()                      # 1. the scene
        assert call(n=-1, cam=False) == bad and b"n = -1" in err()                         # 2. n
        assert call(cam=False, o=opts(use_multisampling=7)) == bad and b"null camera" in err()   # 3. camera / opts
        assert call(o="null") == bad and b"null camera or opts" in err()
        assert call(o=opts(use_multisampling=abi.MS_ADAPTIVE), r=none, h=none) == bad and b"sample positions as centres" in err()   # 4. the opts fields
        for kw, word in ((dict(use_multisampling=7), b"use_multisampling"), (dict(use_multisampling=-1), b"use_multisampling"), (dict(list_order=2), b"list_order"),
                         (dict(list_order=-1), b"list_order"), (dict(shard_count=2), b"shard_count"), (dict(n_gpus=2), b"n_gpus")):
            assert call(o=opts(**kw), r=none, h=none) == bad and word in err(), kw
        # 5. the viewport
        flat = tracer._camera_abi()
        flat.vp_width = 0
        o = opts()
        args = (scene.handle, C.byref(flat), C.byref(o))
        if call is host:
            assert lib.xrt_trace_pixels(*args, ok.ctypes.data_as(_F), 2, None, None, None) == bad and b"viewport" in err()
        else:
            assert lib.xrt_trace_pixels_device(*args, C.c_void_p(0x1000), 2, None, None, None, None) == bad and b"viewport" in err()
        assert call(r=none, h=none, c=none if call is dev else None) == bad and b"both outputs" in err()   # 6. the outputs
        assert call(c=none if call is dev else None) == bad and b"null centers" in err()                    # 7. the centres
        # fields that are not read: garbage is no error
        junk = opts(max_reflections=-5, multisample_quality=99, address_mode=9, filtering=9, shard_rank=7, balance_tiles=3)
        assert call(o=junk) == abi.XRT_E_NO_DEVICE
        # n == 0 is XRT_OK whatever else is missing; a valid call has no device
        assert call(n=0) == abi.XRT_OK and call(n=0, c=none if call is dev else None, r=none, h=none) == abi.XRT_OK
        assert call(n=0, o=opts(list_order=2)) == bad                                      # (arguments before "nothing to do")
        assert call() == abi.XRT_E_NO_DEVICE and call(r=none) == abi.XRT_E_NO_DEVICE and call(h=none) == abi.XRT_E_NO_DEVICE
        for ms in (abi.MS_OFF, abi.MS_FIXED16):
            for order in (abi.LIST_UNORDERED, abi.LIST_COHERENT):
                assert call(o=opts(use_multisampling=ms, list_order=order)) == abi.XRT_E_NO_DEVICE
    # 8. host form: a non-finite centre; the message names the first one and nothing is written
    for v in (np.nan, np.inf, -np.inf):
        for at in ((0, 1), (1, 0)):
            c = ok.copy()
            c[at] = v
            c[1, 1] = v
            rays["o"][:], hits["hit"][:] = 7.0, 7
            assert host(c=c) == bad and (b"centre %d is not finite" % at[0]) in err(), (v, at)
            assert (rays["o"] == 7.0).all() and (hits["hit"] == 7).all()
    bad_c = ok.copy()
    bad_c[0, 0] = np.nan
    assert host(c=bad_c, r=False, h=False) == bad and b"both outputs" in err()             # (the outputs are said before the centres are read)
    # 9. device form: misaligned pointers, after everything else
    assert dev(c=0x1008) == bad and dev(r=0x2004) == bad and dev(h=0x3008) == bad and b"16-byte aligned" in err()
    assert dev(r=0x2004, h=0) == bad and dev(r=0, h=0x300c) == bad
    assert dev(c=0x1008, r=0, h=0) == bad and b"both outputs" in err()
    assert lib.xrt_trace_pixels(None, None, None, None, 0, None, None, None) == bad
    # the mirror
    with pytest.raises(abi.XrtError) as e:
        tracer.TracePixels(ok)
    assert e.value.code == abi.XRT_E_NO_DEVICE
    with pytest.raises(ValueError):
        tracer.TracePixels(bad_c)
    with pytest.raises(ValueError):
        tracer.TracePixels(ok, want_rays=False, want_hits=False)
    r, h = tracer.TracePixels(ok[:0], fixed16=True)
    assert r.shape == (0,) and h.shape == (0,) and r.dtype == xrt.api.RAY_DTYPE and h.dtype == xrt.api.HIT_DTYPE


# ---- the expectation, pinned on the oracle alone ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crate(xrt, orc):
    spec = xrt.configs.crate_scene(96, 54, max_reflections=2)
    return spec, orc.OracleScene(spec), castray_py.CastRayScene(spec)


def test_integer_centres_are_the_oracles_primary_rays(xrt, orc, crate):
    spec, osc, _ = crate
    rays = tp.oracle_rays(orc, spec, px.grid_centers(96, 54))
    assert tp.same_rays(rays, osc.primary_rays())
    perm = np.random.default_rng(4).permutation(96 * 54)[:500]
    assert tp.same_rays(tp.oracle_rays(orc, spec, px.grid_centers(96, 54)[perm]), osc.primary_rays()[perm])
    assert (rays["ignore_mesh"] == -1).all() and (rays["ignore_tri"] == -1).all()


def test_the_constructions_hold_for_rays_as_for_colours(xrt, orc, crate):
    """CastRay (the oracle's, tests/castray) on the constructed rays is the pixel of the oracle frame the construction names: the frame of k times the
    size for fractional centres, the frame with the shifted viewport for centres outside -- and the fixed sixteen, folded by RT:309, are the oracle's
    XRT_MS_FIXED16 frame."""
    spec, osc, cs = crate
    a, f = xrt.abi, np.float32
    W, H = 96, 54
    big, bigf = px.oracle_frame(orc, osc, px.with_mode(spec, a.MS_OFF, size=(W * 8, H * 8)), rows=(20 * 8, 32 * 8))
    pix = [(51, 23), (55, 23), (48, 26), (46, 30), (47, 30), (52, 23), (48, 27)]
    frac = np.array([[f(x) + f(dx) / 8, f(y) + f(dy) / 8] for x, y in pix for dx, dy in ((1, 0), (3, 5), (7, 7), (0, 4))], dtype=f)
    rgba, rgbf, _ = cs.cast_rays(tp.oracle_rays(orc, spec, frac))
    at = (frac * 8).astype(np.int64)
    assert np.array_equal(rgba, big[at[:, 1], at[:, 0]]) and np.array_equal(tp.bits(rgbf), tp.bits(bigf[at[:, 1], at[:, 0]]))
    assert len(np.unique(rgba)) > 5
    # outside the viewport, whole and fractional: a close-up, so that these centres still see the crate
    close = xrt.configs.crate_scene(32, 18, max_reflections=1)
    close.camera = xrt.configs.camera((0, 8, 14), (0, 8, 0))
    c_osc, c_cs = orc.OracleScene(close), castray_py.CastRayScene(close)
    outside = np.array([(-3, -2), (32 + 5, 18 + 1), (-0.5, 18.25)], dtype=f)
    rgba, rgbf, _ = c_cs.cast_rays(tp.oracle_rays(orc, close, outside))
    for i, (vp, size, pixel) in enumerate((((3, 2), (32, 18), (0, 0)), ((-37, -19), (32, 18), (0, 0)), ((4, -4 * 18), (32 * 4, 18 * 4), (2, 1)))):
        o_rgba, o_rgbf = px.oracle_frame(orc, c_osc, px.with_mode(close, a.MS_OFF, size=size), vp=vp, rows=(pixel[1], pixel[1] + 1))
        assert int(o_rgba[pixel[1], pixel[0]]) != 0xFF000000
        assert int(rgba[i]) == int(o_rgba[pixel[1], pixel[0]]) and np.array_equal(tp.bits(rgbf[i]), tp.bits(o_rgbf[pixel[1], pixel[0]])), i
    # the fixed sixteen
    f16, _ = px.oracle_frame(orc, osc, px.with_mode(spec, a.MS_FIXED16), rows=(20, 32))
    sixteen = tp.sample_centers(np.array(pix, dtype=f), True)
    assert sixteen.shape == (16 * len(pix), 2)
    c16, _, _ = cs.cast_rays(tp.oracle_rays(orc, spec, sixteen))
    edges = 0
    for i, (x, y) in enumerate(pix):
        assert px.mean16(orc, c16[16 * i:16 * i + 16]) == int(f16[y, x]), (x, y)
        edges += len(set(int(v) for v in c16[16 * i:16 * i + 16])) > 1
    assert edges >= 4
    # ... also at the frame's corner, where samples lie outside the viewport
    corner = tp.sample_centers(np.array([(0, 0), (95, 53)], dtype=f), True)
    assert corner.min() < 0 and corner[:, 0].max() > 95
    r = tp.oracle_rays(orc, spec, corner)
    assert np.isfinite(r["d"]).all() and len(np.unique(tp.bits(r["d"]), axis=0)) == 32


# ---- conditions on the GPU test's inputs ----------------------------------------------------------------------------------------------------------
def gpu_specs(xrt):
    """The scenes and sizes of tests/test_gpu_trace_pixels.py (those of tests/test_gpu_coherent.py)."""
    return {"hf": hf_spec(xrt, (96, 64), xrt.abi.MS_OFF, "diagonal"), "grid": xrt.configs.crate_grid_scene(96, 54),
            "crate": xrt.configs.crate_scene(96, 54, max_reflections=2), "glass": xrt.configs.default_game_scene(32, 32, max_reflections=3)}


@pytest.mark.parametrize("name", ["hf", "grid", "crate", "glass"])
def test_the_lists_of_the_gpu_test_meet_their_conditions(xrt, orc, name):
    """Every scene's frame as a list: hits and misses, and rays the root slab test (OSM:460) rejects; on the scenes whose lists the seams of the kernel are
    tested with (heightfield, crate grid) and in the glass scene also rays it accepts that still miss -- a single crate fills its root box, no ray that
    reaches it misses --; on the crate grid two bodies hit inside one 64-place unit of the row-major list."""
    spec = gpu_specs(xrt)[name]
    osc = orc.OracleScene(spec)
    rays = osc.primary_rays()
    hits = osc.intersect(rays)
    hit = hits["hit"] != 0
    assert 30 < hit.sum() < len(rays) - 30, name
    assert tp.is_miss_record(hits[~hit]).all(), "the oracle's miss is the miss record"
    nodes, _ = osc.tree()
    box = np.concatenate([nodes["bmin"][0], nodes["bmax"][0]])
    reaches, cannot = tp.reaches_root_box(rays, box)
    assert not (cannot & hit).any()
    assert cannot.sum() > 20, (name, "rays the root slab test rejects")
    if name != "crate":
        assert (reaches & ~hit).sum() > 20, (name, "rays that reach the root box and still miss")
    if name == "grid":
        unit = np.arange(len(rays)) >> 6
        bodies = [len(set(hits["object"][(unit == u) & hit].tolist())) for u in np.unique(unit)]
        assert max(bodies) >= 2, "two bodies inside one 64-place unit"


# ---- the chunk plan -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner():
    return tp.build_checked()


def _plan(exe, n, samples, budget, hinted):
    p = subprocess.run([exe, "--plan", str(n), str(samples), str(budget), str(int(hinted))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return [int(w) for w in p.stdout.split()]


def test_chunk_plan_under_sanitizers(planner):
    """The program's own checks: every entry once and in order, no chunk over the budget or the place limit, counts past 2^31 and 2^32 -- host code
    under ASan + UBSan, nothing of it loaded into Python."""
    p = subprocess.run([planner], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert "host_trace: ok" in p.stdout and "FAILED" not in p.stdout
    assert int(re.search(r"^plans (\d+)$", p.stdout, flags=re.M).group(1)) > 500


def test_chunk_plan_at_its_edges(planner):
    for hinted in (False, True):
        assert _plan(planner, 0, 1, 1 << 30, hinted) == [0]
        assert _plan(planner, 1, 1, 1 << 30, hinted) == [0, 1]
        assert _plan(planner, 1, 16, 1, hinted) == [0, 1]                                # a budget below one entry: an entry is never split
        assert _plan(planner, 10, 16, 1, hinted) == [0, 4, 8, 10]                        # ... and never fewer than four entries a chunk
        assert _plan(planner, 5184, 16, 4 << 30, hinted) == [0, 5184]                    # everything fits: one chunk
        assert _plan(planner, 1 << 28, 16, (1 << 64) - 1, hinted) == [i << 24 for i in range(17)]   # 2^32 places: the place limit of a chunk splits them
        b = _plan(planner, (1 << 31) + 5, 1, (1 << 64) - 1, hinted)                      # n > 2^31
        assert b == [i << 28 for i in range(9)] + [(1 << 31) + 5]
    # 36 bytes per place: exact multiples
    assert _plan(planner, 3000, 1, 36 * 1000, False) == [0, 1000, 2000, 3000]
    assert _plan(planner, 3001, 1, 36 * 1000, False) == [0, 1000, 2000, 3000, 3001]
    assert _plan(planner, 2999, 1, 36 * 1000 + 35, False) == [0, 1000, 2000, 2999]
    assert _plan(planner, 1000, 1, 36 * 1000, False) == [0, 1000]
    assert _plan(planner, 1000, 1, 36 * 1000 - 1, False) == [0, 996, 1000]               # (chunks are multiples of four entries)
    assert _plan(planner, 250, 16, 576 * 100, False) == [0, 100, 200, 250]
    # hinted against unhinted: the table takes room, 512 bytes and 8 per 64 places
    assert _plan(planner, 4097, 1, 36000, False) == [0, 1000, 2000, 3000, 4000, 4097]
    assert _plan(planner, 4097, 1, 36000, True) == [0, 980, 1960, 2940, 3920, 4097]
    assert _plan(planner, 1000, 1, 36 * 1000 + 512 + 8 * 16, True) == [0, 1000]          # exactly the bytes of 1000 places and 16 units
    assert len(_plan(planner, 1000, 1, 36 * 1000 + 512 + 8 * 16 - 1, True)) == 3
