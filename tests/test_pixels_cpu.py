"""xrt_render_pixels (GetColorForQuadrant / the body of Render's inner loop, RT:215-311 / 412-425, on caller-chosen pixels) without a GPU: the
exports in every binding, what is wrong with the arguments alone on a host-only scene, the chunk planner (csrc/pixels_plan.h) in its host
program under ASan + UBSan, and the expectations of the GPU test that can be shown on the CPU -- the oracle's frames looked up at fractional
positions reproduce its supersampled frames, and the listed pixel of the RT:305 case reaches the slip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pixels_py as px

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_F = C.POINTER(C.c_float)
_U = C.POINTER(C.c_uint32)


def test_exports_are_in_the_library_the_header_and_every_binding(xrt):
    hdr = open(os.path.join(ROOT, "include", "xrt.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "XrtNative.cs")).read()
    raw = C.CDLL(xrt.abi.LIB_PATH)
    for name in ("xrt_render_pixels", "xrt_render_pixels_device"):
        assert hasattr(raw, name), name
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in xrt.abi.SYMBOLS, name
        assert re.search(r"public static extern (?:unsafe )?int %s\(" % name, cs), name
    assert "#define XRT_VERSION 203" in hdr and xrt.abi.lib().xrt_version() == 203
    assert "RenderPixels" in open(os.path.join(ROOT, "csharp", "GpuSpatialManager.cs")).read()
    assert callable(getattr(xrt.RayTracer, "RenderPixels", None))


@pytest.fixture(scope="module")
def host_only(xrt):
    spec = xrt.configs.crate_scene(8, 8, max_reflections=1)
    scene, tracer = xrt.configs.build_product(spec, device=-1)
    return scene, tracer


def _call(xrt, scene, tracer, centers, n=None, opts=None, out=True, cam=True, device=False, lights=True, n_lights=None):
    abi, lib = xrt.abi, xrt.abi.lib()
    c = None if centers is None else np.ascontiguousarray(centers, dtype=np.float32)
    n = (c.size // 2) if n is None else n
    rgba = np.zeros(max(n, 1), dtype=np.uint32)
    camera, o, L = tracer._camera_abi(), (opts or tracer._opts_abi(shard_count=0)), tracer._lights_abi()
    nl = len(tracer.Lights) if n_lights is None else n_lights
    if device:   # (no device memory on this box: the pointers only have to look like device pointers -- nothing reads them before the scene is looked at)
        return lib.xrt_render_pixels_device(scene.handle, C.byref(camera) if cam else None, L if lights else None, nl, C.byref(o),
                                            C.c_void_p(centers), n, C.c_void_p(out), None, None, None)
    return lib.xrt_render_pixels(scene.handle, C.byref(camera) if cam else None, L if lights else None, nl, C.byref(o),
                                 None if c is None else c.ctypes.data_as(_F), n, rgba.ctypes.data_as(_U) if out else None, None, None)


def test_argument_errors_come_before_the_device(xrt, host_only):
    scene, tracer = host_only
    abi = xrt.abi
    ok = [[1.0, 2.0], [3.5, -4.0]]
    bad = abi.XRT_E_INVALID_ARG
    assert _call(xrt, scene, tracer, ok, n=-1) == bad
    assert _call(xrt, scene, tracer, None, n=2) == bad
    assert _call(xrt, scene, tracer, ok, out=False) == bad
    assert _call(xrt, scene, tracer, ok, cam=False) == bad
    assert _call(xrt, scene, tracer, ok, lights=False, n_lights=1) == bad
    assert _call(xrt, scene, tracer, ok, n_lights=-1) == bad
    for v in (np.nan, np.inf, -np.inf):
        for at in ((0, 0), (1, 1)):
            c = np.array(ok, dtype=np.float32)
            c[at] = v
            assert _call(xrt, scene, tracer, c) == bad, (v, at)
            assert b"not finite" in abi.lib().xrt_last_error()

    def opts(**kw):
        o = tracer._opts_abi(shard_count=0)
        o.n_gpus = 0
        for k, val in kw.items():
            setattr(o, k, val)
        return o
    for kw in (dict(shard_count=2), dict(n_gpus=2), dict(use_multisampling=7), dict(use_multisampling=-1), dict(max_reflections=-1),
               dict(max_reflections=65), dict(address_mode=3), dict(filtering=2)):
        assert _call(xrt, scene, tracer, ok, opts=opts(**kw)) == bad, kw
        assert _call(xrt, scene, tracer, 0x1000, n=2, out=0x2000, opts=opts(**kw), device=True) == bad, kw
    # the limits of frames, with their codes
    assert _call(xrt, scene, tracer, ok, opts=opts(use_multisampling=abi.MS_ADAPTIVE, multisample_quality=7)) == abi.XRT_E_UNSUPPORTED
    assert _call(xrt, scene, tracer, ok, opts=opts(use_multisampling=abi.MS_ADAPTIVE, multisample_quality=6)) == abi.XRT_E_NO_DEVICE
    assert _call(xrt, scene, tracer, ok, opts=opts(use_multisampling=abi.MS_FIXED16, multisample_quality=7)) == abi.XRT_E_NO_DEVICE   # (quality is read by the adaptive mode only)
    # device form: NULL and misaligned arrays
    assert _call(xrt, scene, tracer, None, n=2, out=0x2000, device=True) == bad
    assert _call(xrt, scene, tracer, 0x1000, n=2, out=None, device=True) == bad
    assert _call(xrt, scene, tracer, 0x1008, n=2, out=0x2000, device=True) == bad
    assert _call(xrt, scene, tracer, 0x1000, n=2, out=0x2004, device=True) == bad
    assert _call(xrt, scene, tracer, 0x1000, n=-3, out=0x2000, device=True) == bad
    assert abi.lib().xrt_render_pixels(None, None, None, 0, None, None, 0, None, None, None) == bad


def test_an_empty_list_is_ok_and_a_valid_call_has_no_device(xrt, host_only):
    scene, tracer = host_only
    abi = xrt.abi
    assert _call(xrt, scene, tracer, np.zeros((0, 2), dtype=np.float32)) == abi.XRT_OK
    assert _call(xrt, scene, tracer, None, n=0, out=False) == abi.XRT_OK          # (no array is needed for no entry)
    assert _call(xrt, scene, tracer, None, n=0, out=None, device=True) == abi.XRT_OK
    for ms in (abi.MS_OFF, abi.MS_ADAPTIVE, abi.MS_FIXED16):
        o = tracer._opts_abi(shard_count=0)
        o.n_gpus, o.use_multisampling, o.multisample_quality = 0, ms, 2
        assert _call(xrt, scene, tracer, [[1.0, 2.0]], opts=o) == abi.XRT_E_NO_DEVICE
        assert _call(xrt, scene, tracer, 0x1000, n=1, out=0x2000, opts=o, device=True) == abi.XRT_E_NO_DEVICE
    with pytest.raises(abi.XrtError):
        tracer.RenderPixels(np.array([[1.0, 2.0]], dtype=np.float32))
    with pytest.raises(ValueError):
        tracer.RenderPixels(np.array([[1.0, np.nan]], dtype=np.float32))
    assert tracer.RenderPixels(np.zeros((0, 2), dtype=np.float32)).shape == (0,)


# ---- the chunk planner ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner():
    return px.build_checked()


def _plan(exe, n, mode, quality, lights, budget):
    p = subprocess.run([exe, "--plan", str(n), str(mode), str(quality), str(lights), str(budget)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return [int(w) for w in p.stdout.split()]


def test_chunk_planner_under_sanitizers(planner):
    """The program's own checks: every entry once and in order, no chunk over the budget or the ray limit, n * samples past 2^31 and 2^32, one
    chunk when everything fits -- host code under ASan + UBSan, nothing of it loaded into Python."""
    p = subprocess.run([planner], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert "host_pixels: ok" in p.stdout and "FAILED" not in p.stdout
    assert int(re.search(r"^plans (\d+)$", p.stdout, flags=re.M).group(1)) > 1000


def test_chunk_planner_plans(xrt, planner):
    abi = xrt.abi
    assert _plan(planner, 0, abi.MS_OFF, 0, 1, 1 << 30) == [0]
    assert _plan(planner, 5184, abi.MS_FIXED16, 0, 1, 4 << 30) == [0, 5184]                  # everything fits: one chunk
    assert _plan(planner, 4097, abi.MS_OFF, 0, 1, 200 * 1000) == [0, 1000, 2000, 3000, 4000, 4097]   # 200 bytes per ray with one light
    assert _plan(planner, 10, abi.MS_FIXED16, 0, 1, 1) == [0, 4, 8, 10]                      # never fewer than four entries
    b = _plan(planner, 3840 * 2160, abi.MS_FIXED16, 0, 1, 4 << 30)                           # the frame that does not fit (VERDICT "missing" 4)
    assert b[0] == 0 and b[-1] == 3840 * 2160 and len(b) > 2
    assert all(0 < y - x <= (4 << 30) // (16 * 200) and x % 4 == 0 for x, y in zip(b, b[1:]))
    b = _plan(planner, 1 << 28, abi.MS_FIXED16, 0, 0, (1 << 64) - 1)                         # 2^32 samples: the ray limit of a chunk splits them
    assert b == [i << 24 for i in range(17)]


# ---- what the GPU test's expectations rest on ---------------------------------------------------------------------------------------------
SLIP_PIXELS = [(51, 23), (55, 23), (48, 26), (46, 30)]   # crate 96x54, quality 1: the lower-right corner subdivides and the slip changes the pixel


@pytest.fixture(scope="module")
def crate_lookup(xrt, orc):
    """The crate at 96x54 and the CastRay colour of every eighth of a pixel: the oracle's XRT_MS_OFF frame of eight times the size."""
    spec = xrt.configs.crate_scene(96, 54, max_reflections=2)
    osc = orc.OracleScene(spec)
    big, _ = px.oracle_frame(orc, osc, px.with_mode(spec, xrt.abi.MS_OFF, size=(96 * 8, 54 * 8)))

    def cast(x, y):
        xi, yi = float(x) * 8, float(y) * 8
        assert xi == int(xi) and yi == int(yi) and 0 <= xi < 96 * 8 and 0 <= yi < 54 * 8, (x, y)
        return int(big[int(yi), int(xi)])
    return spec, osc, cast


def test_scaled_frames_reproduce_the_supersampled_frames(xrt, orc, crate_lookup):
    """CastRay colours looked up in the scaled frame, averaged as RT:309 does, are the oracle's adaptive (quality 0 and 1) and fixed-16 frames:
    the lookup and the restated GetColorForQuadrant are sound."""
    spec, osc, cast = crate_lookup
    ad0, _ = px.oracle_frame(orc, osc, px.with_mode(spec, xrt.abi.MS_ADAPTIVE, 0))
    ad1, _ = px.oracle_frame(orc, osc, px.with_mode(spec, xrt.abi.MS_ADAPTIVE, 1))
    f16, _ = px.oracle_frame(orc, osc, px.with_mode(spec, xrt.abi.MS_FIXED16))
    f = np.float32
    for y in range(14, 40):
        for x in range(30, 66):
            assert px.quadrant_color(orc, cast, x, y, 1.0, 0, 0) == int(ad0[y, x]), (x, y)
            assert px.quadrant_color(orc, cast, x, y, 1.0, 0, 1) == int(ad1[y, x]), (x, y)
            sixteen = [cast(f(f(x) + f(ax)) + f(bx), f(f(y) + f(ay)) + f(by)) for (ax, bx), (ay, by) in px.fixed16_offsets()]
            assert px.mean16(orc, sixteen) == int(f16[y, x]), (x, y)


def test_the_listed_pixels_reach_the_slip(xrt, orc, crate_lookup):
    """RT:305: at these pixels the lower-right corner subdivides at level 0 and the oracle's frame differs from the slip-free fold."""
    spec, osc, cast = crate_lookup
    ad1, _ = px.oracle_frame(orc, osc, px.with_mode(spec, xrt.abi.MS_ADAPTIVE, 1))
    for x, y in SLIP_PIXELS:
        reached = []
        with_slip = px.quadrant_color(orc, cast, x, y, 1.0, 0, 1, True, reached)
        assert 0 in reached, (x, y)
        assert with_slip == int(ad1[y, x]), (x, y)
        assert px.quadrant_color(orc, cast, x, y, 1.0, 0, 1, False) != int(ad1[y, x]), (x, y)


def test_a_shifted_viewport_shifts_the_centres(xrt, orc, crate_lookup):
    """Unproject sees only sx - vp.X: pixel (x, y) of a frame whose viewport origin is (dx, dy) is the centre (x - dx, y - dy) of the frame
    at the origin (RT:415) -- what the GPU test's centres outside the viewport are compared with."""
    spec, osc, cast = crate_lookup
    off, _ = px.oracle_frame(orc, osc, spec)
    shifted, _ = px.oracle_frame(orc, osc, spec, vp=(-40, -20))
    assert np.array_equal(shifted[0:30, 0:50], off[20:50, 40:90])
    assert len(np.unique(shifted[0:30, 0:50])) > 10
