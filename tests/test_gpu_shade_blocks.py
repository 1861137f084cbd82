"""k_shade in blocks of any whole number of waves (XRT_SHADE_BLOCK, FramePlan::shadeBlock; kernels.hip launch_shade).  The block size decides how many blocks
share a CU and in which order the lists of a round are filled -- scheduling alone.  So for XRT_SHADE_BLOCK in {256, 512, 768, 1024} a frame is compared bit
for bit with the oracle's RGBA8 and with the 1024 frame, and its ray counts (xrt_stats) and end counts (xrt_debug_end_counts) with the 1024 frame's.

xrt_scene_create reads the switch, so every size gets a scene of its own; the first frame of a scene has no grid hints and takes the big-block path whatever
its size, which is the path the switch steers (a hinted small generation takes 256-thread blocks as ever: the second frame of every scene is compared too).

Scenes: (a) the m=12 terrain seen from low and aside at 96x54 with 16 sub-rays, MaxReflections 3, one spot light: k_shade<true, true> with a list of
reflections, a level map and tiles right of the terrain's screen rectangle; its live primary rays are no multiple of 256, so neither of 512 nor of 768;
(b) the same at one sample with MaxReflections 2; (c) a 4x4 grid of crates (two-level scene) at 64x64, MaxReflections 3: shadow slots, parts A and B;
(d) two of the default game scene's Transparent spheres at 64x64, MaxReflections 4: the ray tree with two appends per hit; (e) the terrain at 8x8 pixels, one
sample: a generation smaller than any block.  Two frames in flight: (a) at 768 with the hints off, eight frames, each compared."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1024, 768, 512, 256)   # (1024 first: the others are compared with it)
LOW_ASIDE_CAMERA = ((-30, 12, 75), (25, 0, 0))   # low over the terrain, which ends left of the middle of the screen
NEAR_ABOVE = (10.0, 6.0, 0.0)                     # steep from the hits below it (answered at emission), flat from the hits far away (emitted)
COUNTS = ("rays_closest", "rays_shadow", "shaded_hits", "pixels", "rays_traversed")


def terrain(xrt, w, h, R, ms16):
    s = xrt.configs.SceneSpec("heightfield_m12")
    s.meshes.append((xrt.fixtures.heightfield(12), xrt.configs.material(0.3)))
    s.objects.append(([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    s.camera = xrt.configs.camera(*LOW_ASIDE_CAMERA)
    s.lights = [xrt.configs.spot(NEAR_ABOVE)]
    s.max_reflections = R
    s.multisampling = xrt.abi.MS_FIXED16 if ms16 else xrt.abi.MS_OFF
    s.mesh_threshold = 8
    return s.with_size(w, h)


def scenes(xrt):
    crates = xrt.configs.crate_grid_scene(64, 64, max_reflections=3, n=3, grid=4)
    crates.camera = xrt.configs.camera((0, 70, 150), (0, 0, 0))   # (the grid fills the width of the image)
    spheres = xrt.configs.default_game_scene(64, 64, 4)           # (its Transparent sphere; two of them, one behind the other's shoulder)
    spheres.objects = [([0], p, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)) for p in ((-2.5, 2.0, 0.0), (2.5, 2.0, -4.0))]
    spheres.camera = xrt.configs.camera((0, 5, 12), (0, 2, 0))
    return {
        "a_terrain_16spp": terrain(xrt, 96, 54, 3, True),
        "b_terrain_1spp": terrain(xrt, 96, 54, 2, False),
        "c_crates_two_level": crates,
        "d_transparent_spheres": spheres,
        "e_terrain_8x8": terrain(xrt, 8, 8, 3, False),
    }


def build(xrt, monkeypatch, spec, env):
    with monkeypatch.context() as m:   # (xrt_scene_create reads the switches; whatever the environment held before comes back)
        for k, v in env.items():
            m.setenv(k, v)
        return xrt.configs.build_product(copy.deepcopy(spec))


_ORACLE = {}


def oracle(orc, name, spec, R=None):
    """(rgba, stats) of the oracle, computed once per scene and depth"""
    if (name, R) not in _ORACLE:
        s = copy.deepcopy(spec)
        if R is not None:
            s.max_reflections = R
        rgba, _, st = orc.OracleScene(s).render(nthreads=8, want_float=False)
        rgba.setflags(write=False)
        _ORACLE[(name, R)] = (rgba, st)
    return _ORACLE[(name, R)]


def slots(spec, xrt):
    """paths of a frame: every slot of its 64x8 tiles, pixel or not, times the samples"""
    return ((spec.width + 63) // 64) * ((spec.height + 7) // 8) * 512 * (16 if spec.multisampling == xrt.abi.MS_FIXED16 else 1)


@pytest.mark.parametrize("name", ["a_terrain_16spp", "b_terrain_1spp", "c_crates_two_level", "d_transparent_spheres", "e_terrain_8x8"])
def test_every_block_size_renders_the_same_frame(xrt, orc, monkeypatch, name):
    spec = scenes(xrt)[name]
    o_rgba, o_st = oracle(orc, name, spec)
    assert (o_rgba & 0xffffff).any()   # (the frame shows something)
    ref = None
    for size in SIZES:
        scene, tracer = build(xrt, monkeypatch, spec, {"XRT_SHADE_BLOCK": str(size)})
        for frame in (0, 1):   # unhinted (the switch's size in every launch), then hinted
            rgba = tracer.Render().copy()
            st, counts = {k: tracer.last_stats[k] for k in COUNTS}, scene.EndCounts()
            assert np.array_equal(rgba, o_rgba), "XRT_SHADE_BLOCK=%d frame %d: %d RGBA8 pixels differ from the oracle" % (size, frame, int((rgba != o_rgba).sum()))
            for k in ("rays_closest", "rays_shadow", "shaded_hits", "pixels"):
                assert st[k] == o_st[k], (size, frame, k, st[k], o_st[k])
            if ref is None:
                ref = (rgba, st, counts)
                print(name, "stats", st, "end counts", counts, "paths", slots(spec, xrt))
            assert np.array_equal(rgba, ref[0]), (size, frame)
            assert st == ref[1], (size, frame, st, ref[1])
            assert counts == ref[2], (size, frame, counts, ref[2])
    counts = ref[2]
    if name.startswith(("a_", "b_", "e_")):   # one-body scenes without Transparent materials end paths early: the counts are engaged
        assert sum(counts) == slots(spec, xrt), (counts, slots(spec, xrt))
    if name == "a_terrain_16spp":
        h0 = oracle(orc, name, spec, 0)[1]["shaded_hits"]
        h1 = oracle(orc, name, spec, 1)[1]["shaded_hits"] - h0
        live = slots(spec, xrt) - counts[0]
        assert h1 > 0 and counts[2] >= h1         # reflections that hit: a list of next rays, and of paths for k_compose
        assert counts[1] > 0                      # ... and paths k_shade ended itself
        assert live % 256 != 0 and live > 4096    # case (f): no multiple of 768 or of 512, and several blocks of either
        assert live < spec.width * spec.height * 16   # pixels right of the terrain's rectangle made no ray
    if name == "e_terrain_8x8":
        assert 0 < slots(spec, xrt) - counts[0] <= 8 * 8   # fewer live rays than one wave, in a grid sized for an unknown generation


def test_two_frames_in_flight_at_768(xrt, orc, monkeypatch):
    """Eight frames of (a), two in flight, XRT_SHADE_BLOCK=768 and no grid hints (every k_shade launch of every frame in 768-thread blocks): each frame is
    the oracle's, with the blocking 1024 frame's end counts."""
    import torch
    spec = scenes(xrt)["a_terrain_16spp"]
    o_rgba, _ = oracle(orc, "a_terrain_16spp", spec)
    scene, tracer = build(xrt, monkeypatch, spec, {"XRT_SHADE_BLOCK": "1024"})
    tracer.Render()
    want = scene.EndCounts()
    assert sum(want) == slots(spec, xrt)
    scene, tracer = build(xrt, monkeypatch, spec, {"XRT_SHADE_BLOCK": "768", "XRT_GRID_HINTS": "0"})
    outs = [torch.zeros(spec.width * spec.height, dtype=torch.int32, device="cuda") for _ in range(2)]
    frs = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
    tickets = [None, None]
    for f in range(8 + 1):
        cur = f & 1
        if f < 8:
            tickets[cur] = frs[cur].begin()
        if f >= 1:   # the frame begun one step ago was open while this one was enqueued
            prv = cur ^ 1
            frs[prv].end(tickets[prv])
            counts = scene.EndCounts()
            torch.cuda.synchronize()
            assert np.array_equal(outs[prv].cpu().numpy().view(np.uint32), o_rgba), f
            assert counts == want, (f, counts, want)
            outs[prv].zero_()
            torch.cuda.synchronize()   # (the next frame into this buffer runs on the library's own stream)
