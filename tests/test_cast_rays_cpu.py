"""xrt_cast_rays (RayTracer.CastRay, RT:506-737, on caller-given rays) without a GPU: the checker (tests/castray, the oracle's own
CastRay) against the oracle's frames, and the exports' presence in every binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import castray_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scenes(xrt):
    cfg = xrt.configs
    return [("crate", cfg.crate_scene(48, 32, max_reflections=2)),
            ("crate_grid", cfg.crate_grid_scene(48, 32, max_reflections=2, n=5, grid=4)),
            ("default_game", cfg.default_game_scene(40, 40, max_reflections=3)),   # glass: ray trees
            ("heightfield", cfg.heightfield_scene(48, 32, m=33, max_reflections=2))]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_checker_on_camera_rays_is_the_oracle_frame(xrt, which):
    """CastRay(primary ray, iteration 0, null, 1.0) of every pixel is RenderInternal's pixel (RT:410-425), bits and counters."""
    name, spec = _scenes(xrt)[which]
    cs = castray_py.CastRayScene(spec)
    f_rgba, f_rgbf, f_st = cs.render()
    rgba, rgbf, st = cs.cast_rays(cs.primary_rays(), iteration=0, ref_index=1.0)
    assert np.array_equal(rgba, f_rgba), name
    assert _same_bits(rgbf, f_rgbf), name
    for k in ("rays_closest", "rays_shadow", "shaded_hits", "hits_closest", "node_tests", "tri_tests", "pixels"):
        assert st[k] == f_st[k], (name, k, st[k], f_st[k])


@pytest.mark.parametrize("which", [0, 2])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_checker_iteration_is_a_shallower_frame(xrt, which, k):
    """CastRay from iteration k with MaxReflections M is the frame of MaxReflections max(0, M - k) (RT:545)."""
    name, spec = _scenes(xrt)[which]
    cs = castray_py.CastRayScene(spec)
    M = spec.max_reflections
    f_rgba, f_rgbf, f_st = cs.render(max_reflections=max(0, M - k))
    rgba, rgbf, st = cs.cast_rays(cs.primary_rays(), iteration=k)
    assert np.array_equal(rgba, f_rgba) and _same_bits(rgbf, f_rgbf), (name, k)
    assert (st["rays_closest"], st["rays_shadow"], st["shaded_hits"]) == (f_st["rays_closest"], f_st["rays_shadow"], f_st["shaded_hits"])


def test_exports_are_declared_bound_and_in_the_abi_table(xrt):
    hdr = open(os.path.join(ROOT, "include", "xrt.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "XrtNative.cs")).read()
    for name in ("xrt_cast_rays", "xrt_cast_rays_device"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in xrt.abi.SYMBOLS, name
        assert re.search(r"public static extern (?:unsafe )?int %s\(" % name, cs), name
    assert "#define XRT_VERSION 203" in hdr


def test_host_only_scene_has_no_device(xrt):
    """A scene created with device -1 exists on the host only: both exports return XRT_E_NO_DEVICE (no CPU path)."""
    spec = xrt.configs.crate_scene(8, 8, max_reflections=1)
    scene, tracer = xrt.configs.build_product(spec, device=-1)
    lib, abi = xrt.abi.lib(), xrt.abi
    rays = xrt.rays_array([(0, 0, 5)], [(0, 0, -1)])
    out = np.zeros(1, dtype=np.uint32)
    opts = abi.xrt_render_opts()
    assert lib.xrt_cast_rays(scene.handle, rays.ctypes.data_as(C.POINTER(abi.xrt_ray)), 1, 0, 1.0, None, 0, C.byref(opts),
                             out.ctypes.data_as(C.POINTER(C.c_uint32)), None, None) == abi.XRT_E_NO_DEVICE
    assert lib.xrt_cast_rays_device(scene.handle, None, 1, 0, 1.0, None, 0, C.byref(opts), None, None, None, None) == abi.XRT_E_NO_DEVICE
    with pytest.raises(abi.XrtError):
        tracer.CastRay(((0, 0, 5), (0, 0, -1)))
