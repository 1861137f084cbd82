"""XRT_GUARD's registry of guarded device buffers (csrc/device_res.h) across switches of the mode.  The mode is process-wide and is read when
a scene is created; list calls made under it check the guard of every registered buffer of the process when they end.  A buffer that was
registered while the mode was on and is freed after it was switched off must leave the registry: its address is handed out again -- to a
buffer without a guard, or to another allocator in the process -- and a check under the mode would find no pattern there and report
XRT_E_INTERNAL for a call that wrote nothing out of bounds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_a_buffer_freed_with_the_mode_off_leaves_the_registry(xrt, monkeypatch):
    import torch
    spec = xrt.configs.crate_grid_scene(64, 40)
    small = xrt.configs.crate_scene(32, 32, 0)
    try:
        monkeypatch.setenv("XRT_GUARD", "1")
        scene, tracer = xrt.configs.build_product(spec)
        rays = tracer.GeneratePrimaryRays()
        want = tracer.CastRays(rays)                     # the scene's buffers and its work set, guarded and registered
        monkeypatch.setenv("XRT_GUARD", "0")
        xrt.configs.build_product(small)                 # (xrt_scene_create reads the switch)
        assert scene._scene.close() == xrt.abi.XRT_OK    # xrt_scene_destroy: freed while the mode is off
        # the addresses go round again: the same sizes without guards from the library, and other sizes from another allocator
        torch.cuda.empty_cache()
        again, t2 = xrt.configs.build_product(spec)
        assert np.array_equal(t2.CastRays(rays), want)
        fill = [torch.zeros(1 << k, dtype=torch.uint8, device="cuda") for k in range(8, 27) for _ in range(4)]
        torch.cuda.synchronize()
        monkeypatch.setenv("XRT_GUARD", "1")
        scene, tracer = xrt.configs.build_product(spec)
        for _ in range(2):
            assert np.array_equal(tracer.CastRays(rays), want)   # every call ends with a check of every registered guard
        assert np.array_equal(t2.CastRays(rays), want)           # a scene made with the mode off, used with it on: nothing of it is registered
        del fill
    finally:
        monkeypatch.delenv("XRT_GUARD")
        xrt.configs.build_product(small)                 # (leaves the mode as the guarded tests of the suite leave it)
