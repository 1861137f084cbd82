"""Primary packets are one aligned unit of the screen (kernels.h QuadTable): k_raygen writes, beside the compact live list, one entry (first slot, live
rays) per wave and round that has a live ray, and launch #0 of k_packet takes its packets from the entries instead of cutting the live list into runs of
64 slots.  A wave of k_raygen holds 64 consecutive, 64-aligned paths -- a 2x2 pixel quad x 16 samples, a 4x4 block x 4 samples (level 0 of an adaptive
frame), an 8x8 block at one sample.

Structure, read through xrt_debug_packet_table (OctreeSpatialManager.PacketTable) after a blocking frame: the entries' slot ranges are disjoint and
cover 0 .. live-1 exactly, every entry holds 1 .. 64 rays, the paths of an entry share path >> 6, no two entries share that value, and there are as many
entries as distinct values among the live paths.  The frames are small, so that the root box's silhouette cuts most reservation groups of k_raygen (4096
paths each) and a packet of 64 consecutive slots would be the tail of one unit and the head of the next nearly everywhere.

Nothing a caller can see may change: every frame is the oracle's bit for bit, blocking and two in flight, with XRT_PK_QUADS=1 and =0 (once under
XRT_GUARD=1), and the ray statistics and end counts are the same under both settings.

One-body scenes take the packet kernel for generation 0 by themselves only with 16 samples; the 4-sample and the 1-sample cases force it with XRT_PACKET
bit 0, as the tools do.  Two-level scenes take it at every sample count."""
import copy
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIGHT = (0.0, 120.0, 160.0)
UP = (0.0, 1.0, 0.0)
ROLLED = (math.sqrt(0.5), math.sqrt(0.5), 0.0)   # the image rolled by 45 degrees: a horizontal edge of the root box crosses it diagonally


def hf_spec(xrt, size, ms, cam):
    s = xrt.configs.SceneSpec("heightfield_m32")
    s.meshes.append((xrt.fixtures.heightfield(32), xrt.configs.material(0.3)))
    s.objects.append(([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    s.lights = [xrt.configs.spot(LIGHT)]
    s.max_reflections = 1
    s.multisampling, s.multisample_quality = ms, 0
    s.mesh_threshold = 8
    # whole: the terrain (x, z in [-50, 50]) from above its edge, all of it on the screen; diagonal: looking past it, rolled -- its far edge runs from corner to corner
    s.camera = xrt.configs.camera((0, 60, 110), (0, 0, 0)) if cam == "whole" else dict(xrt.configs.camera((0, 60, 110), (70, 10, 0)), up=ROLLED)
    return s.with_size(*size)


def crates_spec(xrt, size, cam):
    s = xrt.configs.crate_grid_scene(size[0], size[1], max_reflections=1, n=3, grid=2, textured=False)   # four crates, spacing 40, one shared mesh
    s.camera = xrt.configs.camera((0, 60, 130), (0, 0, 0)) if cam == "whole" else dict(xrt.configs.camera((0, 60, 130), (60, 0, 0)), up=ROLLED)
    return s


CASES = {
    "hf_16spp": (lambda xrt, cam: hf_spec(xrt, (160, 96), xrt.abi.MS_FIXED16, cam), {}, 16),
    "hf_4spp": (lambda xrt, cam: hf_spec(xrt, (160, 96), xrt.abi.MS_ADAPTIVE, cam), {"XRT_PACKET": "1"}, 4),
    "hf_1spp": (lambda xrt, cam: hf_spec(xrt, (96, 64), xrt.abi.MS_OFF, cam), {"XRT_PACKET": "1"}, 1),
    "crates_1spp": (lambda xrt, cam: crates_spec(xrt, (128, 72), cam), {}, 1),
}


def build(xrt, monkeypatch, spec, env):
    with monkeypatch.context() as m:   # (xrt_scene_create reads the switches; whatever the environment held before comes back)
        for k, v in env.items():
            m.setenv(k, v)
        return xrt.configs.build_product(copy.deepcopy(spec))


_ORACLE = {}


def oracle(orc, name, cam, spec):
    if (name, cam) not in _ORACLE:
        rgba, _, st = orc.OracleScene(copy.deepcopy(spec)).render(nthreads=8, want_float=False)
        rgba.setflags(write=False)
        _ORACLE[(name, cam)] = (rgba, st)
    return _ORACLE[(name, cam)]


def check_table(entries, paths, what):
    """The assertions on the structure; returns (entries, entries that are not whole units)."""
    live = paths.shape[0]
    assert entries.shape[0] > 0, (what, "launch #0 took no table")
    start, ln = entries[:, 0].astype(np.int64), entries[:, 1].astype(np.int64)
    assert ln.min() >= 1 and ln.max() <= 64, (what, int(ln.min()), int(ln.max()))
    order = np.argsort(start, kind="stable")
    s, l = start[order], ln[order]
    assert s[0] == 0 and np.array_equal(s[1:], (s + l)[:-1]) and s[-1] + l[-1] == live, (what, "the slot ranges are not a partition of 0 .. live-1", live)
    unit = paths.astype(np.int64) >> 6
    first = unit[s]
    owner = np.repeat(np.arange(s.shape[0]), l)   # entry of every slot, in slot order
    assert np.array_equal(unit, first[owner]), (what, "an entry mixes units")
    assert np.unique(first).shape[0] == first.shape[0], (what, "two entries share a unit")
    assert entries.shape[0] == np.unique(unit).shape[0], (what, entries.shape[0], np.unique(unit).shape[0])
    return entries.shape[0], int((ln < 64).sum())


STAT_KEYS = ("rays_closest", "rays_shadow", "rays_traversed", "shaded_hits", "pixels")


@pytest.mark.parametrize("cam", ["whole", "diagonal"])
@pytest.mark.parametrize("name", list(CASES))
def test_table_and_parity(xrt, orc, monkeypatch, name, cam):
    """Blocking frames with the table and without: the structure of the table, the oracle's image, equal statistics; then two frames in flight."""
    import torch
    make, env, samples = CASES[name]
    spec = make(xrt, cam)
    o_rgba, o_st = oracle(orc, name, cam, spec)
    assert 0.01 < float(((o_rgba & 0xffffff) != 0).mean()) < 0.99, "the camera should see the scene's edge"
    seen = {}
    for quads in ("1", "0"):
        scene, tracer = build(xrt, monkeypatch, spec, dict(env, XRT_PK_QUADS=quads))
        for rep in range(2):   # (the second frame runs on the context's other count word)
            rgba = tracer.Render().copy()
            assert np.array_equal(rgba, o_rgba), (quads, rep, "%d RGBA8 pixels differ from the oracle" % int((rgba != o_rgba).sum()))
            for k in ("rays_closest", "rays_shadow"):
                assert tracer.last_stats[k] == o_st[k], (quads, k, tracer.last_stats[k], o_st[k])
            entries, paths = scene.PacketTable()
            if quads == "1":
                n, partial = check_table(entries, paths, (name, cam, rep))
                consecutive = (paths.shape[0] + 63) // 64
                print("packet table", name, cam, "live", paths.shape[0], "entries", n, "not whole", partial, "packets of 64 consecutive slots", consecutive)
                assert paths.shape[0] > 100 * samples and partial > 0   # the silhouette cuts units: consecutive slots would straddle them
            else:
                assert entries.shape[0] == 0
        seen[quads] = (rgba, {k: tracer.last_stats[k] for k in STAT_KEYS}, scene.EndCounts())
        # two in flight, each context twice
        outs = [torch.zeros(spec.width * spec.height, dtype=torch.int32, device="cuda") for _ in range(2)]
        frames = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
        tickets = [None, None]
        for f in range(5):
            cur = f & 1
            if f < 4:
                tickets[cur] = frames[cur].begin()
            if f >= 1:
                prv = cur ^ 1
                frames[prv].end(tickets[prv])
                torch.cuda.synchronize()
                got = outs[prv].cpu().numpy().view(np.uint32).reshape(o_rgba.shape)
                assert np.array_equal(got, o_rgba), (quads, "in flight", f, int((got != o_rgba).sum()))
                outs[prv].zero_()
                torch.cuda.synchronize()   # (the next frame into this buffer runs on the library's own stream)
    assert np.array_equal(seen["1"][0], seen["0"][0])
    assert seen["1"][1] == seen["0"][1], (seen["1"][1], seen["0"][1])
    assert seen["1"][2] == seen["0"][2], (seen["1"][2], seen["0"][2])


def test_shard_one_of_three(xrt, orc, monkeypatch):
    """The one-body 16-sample frame as three shards: the table of shard 1, and the gathered image is the oracle's with the table and without."""
    import torch
    make, env, samples = CASES["hf_16spp"]
    spec = make(xrt, "diagonal")
    o_rgba, _ = oracle(orc, "hf_16spp", "diagonal", spec)
    W, H = spec.width, spec.height
    tx, ty, tpr = xrt.dist.shard_layout(W, H, 3)
    n = tpr * 512
    counts = {}
    for quads in ("1", "0"):
        scene, tracer = build(xrt, monkeypatch, spec, dict(env, XRT_PK_QUADS=quads))
        gathered = torch.full((3 * n,), 0x55, dtype=torch.int32, device="cuda")
        stats = []
        for rank in (0, 2, 1):
            tracer.RenderDevice(gathered[rank * n:(rank + 1) * n].data_ptr(), shard_rank=rank, shard_count=3)
            stats.append((rank, {k: tracer.last_stats[k] for k in STAT_KEYS}, scene.EndCounts()))
        entries, paths = scene.PacketTable()   # shard 1: the last one rendered
        if quads == "1":
            nE, partial = check_table(entries, paths, "shard 1 of 3")
            print("packet table shard 1 of 3: live", paths.shape[0], "entries", nE, "not whole", partial)
            assert paths.shape[0] > 100 * samples and paths.max() < n * samples
        else:
            assert entries.shape[0] == 0
        out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        xrt.dist.detile_device(gathered, W, H, 3, out)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32).reshape(o_rgba.shape)
        assert np.array_equal(got, o_rgba), (quads, int((got != o_rgba).sum()))
        counts[quads] = stats
    assert counts["1"] == counts["0"]


def test_under_guards(xrt, orc, monkeypatch):
    """XRT_GUARD=1 (csrc/device_res.h): the table is a device buffer like any other, a write past it fails the frame.  Both settings, one-body and two-level."""
    monkeypatch.setenv("XRT_GUARD", "1")
    try:
        for name in ("hf_16spp", "crates_1spp"):
            make, env, samples = CASES[name]
            spec = make(xrt, "diagonal")
            o_rgba, _ = oracle(orc, name, "diagonal", spec)
            frames = []
            for quads in ("1", "0"):
                scene, tracer = build(xrt, monkeypatch, spec, dict(env, XRT_PK_QUADS=quads))
                for rep in range(2):
                    frames.append(tracer.Render().copy())
            for f in frames:
                assert np.array_equal(f, o_rgba), (name, int((f != o_rgba).sum()))
    finally:
        monkeypatch.delenv("XRT_GUARD")
        xrt.configs.build_product(xrt.configs.crate_scene(32, 32, 0))   # (xrt_scene_create reads the switch)
