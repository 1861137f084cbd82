"""Device memory comes back with xrt_scene_destroy: every device resource of a scene is a member of an owner type (csrc/device_res.h,
DESIGN.md "Ownership"), so whatever a scene allocated while it lived -- work buffers of every frame mode, pose versions, the staging of
ray batches, the split-walk arenas of seam-1 calls -- is freed with it.  Measured as the device's free memory around whole lifetimes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the split-walk arena of one stream's seam-1 calls at the default XRT_PK_SPLIT_ITEMS = 8192 (xrt_api.cpp split_arena): 8192 items of 544
# words and 2049 records of 512 words
ARENA = 8192 * 544 * 4 + 2049 * 512 * 4
assert ARENA == 22022144


def _destroy(xrt, scene):
    """close() now (not when the garbage collector gets to it), and xrt_scene_destroy must have agreed."""
    rc = scene._scene.close()
    assert rc == xrt.abi.XRT_OK, (rc, xrt.abi.lib().xrt_last_error())


def _frames_cycle(xrt, specs):
    """One scene's life through every kind of work that makes the library allocate, and a ray-tree scene's."""
    import torch
    grid, glass = specs
    scene, tracer = xrt.configs.build_product(grid)
    px = grid.width * grid.height
    tracer.Render()                                                     # one blocking frame
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    frs = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
    t0 = frs[0].begin(); t1 = frs[1].begin(); frs[0].end(t0); frs[1].end(t1)   # two tickets in flight
    t0 = frs[0].begin()
    x, y, z = scene.Bodies[0].Position
    scene.Bodies[0].Position = (x + 0.25, y, z)
    scene._push_poses()                                                 # xrt_scene_set_poses while a ticket is open: a second pose version
    frs[0].end(t0)
    tracer.UseMultisampling, tracer.MultisampleMode = True, xrt.abi.MS_FIXED16
    tracer.Render()                                                     # 16 sub-rays
    tracer.MultisampleMode, tracer.MultisampleQuality = xrt.abi.MS_ADAPTIVE, 2
    tracer.Render()                                                     # adaptive
    assert int(scene.IntersectBatch(tracer.GeneratePrimaryRays())["hit"].sum()) > 0
    torch.cuda.synchronize()
    _destroy(xrt, scene)

    scene, tracer = xrt.configs.build_product(glass)
    tracer.Render()                                                     # a ray tree
    rays = tracer.GeneratePrimaryRays()
    assert len(rays) == glass.width * glass.height
    _, vertices, _, _ = tracer.CastRays(rays, paths=True)               # a ray batch with its paths
    assert len(vertices) > 0
    _destroy(xrt, scene)


def _split_cycle(xrt, spec, monkeypatch):
    """A one-body scene's seam-1 batch through the packet kernel with split walks: the arena of the calling stream."""
    monkeypatch.setenv("XRT_PACKET", "31")
    monkeypatch.setenv("XRT_PK_SPLIT", "1")
    try:
        scene, tracer = xrt.configs.build_product(spec)
    finally:   # (xrt_scene_create has read the switches)
        monkeypatch.delenv("XRT_PACKET")
        monkeypatch.delenv("XRT_PK_SPLIT")
    assert int(scene.IntersectBatch(tracer.GeneratePrimaryRays())["hit"].sum()) > 0
    _destroy(xrt, scene)


def test_device_memory_comes_back(xrt, monkeypatch):
    """Lifetimes of three scenes -- the crate grid at 96x54 (a blocking frame, two tickets in flight, a pose update under an open ticket,
    16 sub-rays, adaptive quality 2, a seam-1 batch), the reference's default scene at 64x64 (a ray-tree frame, a ray batch with paths)
    and a 64x64-cell heightfield under XRT_PACKET=31 XRT_PK_SPLIT=1 (a seam-1 batch with split walks) -- each ended by xrt_scene_destroy: once
    to warm the runtime's own pools up, then three times between two readings of the device's free memory.  The three sets may cost less
    than half a split-walk arena (11,011,072 bytes).

    Measured on an MI355X: before the owners, xrt_scene::apiSplit was in no release list and the three sets lost 75,497,472 bytes (three
    times 24 MiB: an arena of 22,022,144 bytes is two allocations, each rounded up by the allocator); with the owners the loss was 0 bytes
    in each of five runs.  A frame with n_gpus = 2 under XRT_FAKE_GPUS=1 is not in the set: three lifetimes of a scene that renders one
    such frame lose 184,549,376 bytes after a warm-up lifetime, before the owners and with them alike (RCCL's own memory, taken once), far
    above the limit here; test_in_library_multi_gpu covers those frames."""
    import torch
    specs = (xrt.configs.crate_grid_scene(96, 54), xrt.configs.default_game_scene(64, 64, 4))
    hf = xrt.configs.heightfield_scene(96, 54, m=64)

    def run_set():
        _frames_cycle(xrt, specs)
        _split_cycle(xrt, hf, monkeypatch)

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    run_set()
    before = free_bytes()
    for _ in range(3):
        run_set()
    lost = before - free_bytes()
    print("device memory lost over three sets: %d bytes (%.3f arenas)" % (lost, lost / ARENA))
    assert lost < ARENA // 2, "three scene lifetimes cost %d bytes of device memory (%.2f split-walk arenas)" % (lost, lost / ARENA)


def test_destroy_refuses_an_open_ticket(xrt):
    """xrt_scene_destroy with a ticket open is XRT_E_BUSY and leaves the scene whole: the ticket ends with the right frame, and the scene
    is destroyed afterwards."""
    import torch
    spec = xrt.configs.crate_grid_scene(96, 54)
    scene, tracer = xrt.configs.build_product(spec)
    want = tracer.Render().copy()
    out = torch.zeros(spec.width * spec.height, dtype=torch.int32, device="cuda")
    fr = tracer.PrepareDevice(out.data_ptr())
    t = fr.begin()
    assert xrt.abi.lib().xrt_scene_destroy(scene._scene.handle) == xrt.abi.XRT_E_BUSY
    fr.end(t)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    _destroy(xrt, scene)
