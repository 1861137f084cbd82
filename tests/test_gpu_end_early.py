"""Paths that end at generation 0 are coloured where they end (kernels.h EndArgs, XRT_END_EARLY): k_raygen writes black for a path that cannot
reach the scene's root box, part A of k_shade #0 black for a miss and the composed colour for a hit it finished that has no next ray, and
k_compose walks a list of the paths that are left.  Nothing a caller can see may change: every frame is compared bit for bit with the oracle's
RGBA8 and with the same frame rendered under XRT_END_EARLY=0 (xrt_scene_create reads the switch, so one scene per setting).

That the path engages, and on which paths, shows in xrt_debug_end_counts (OctreeSpatialManager.EndCounts): for the last finished frame the paths
k_raygen coloured, the paths k_shade coloured and the paths on the compose list -- each counted by the kernel that did it -- and all zero when the
frame took the other way.  The three sum to the frame's paths (every slot of its 64x8 tiles times the samples, pixel or not), and k_raygen's share
is the paths minus the live primary rays (xrt_stats of a render that answers nothing at emission).

The early writers go through the context's sample buffer at any sample count: the caller's framebuffer is written by the frame's last kernel only,
so a one-sample frame that engages is resolved by k_resolve instead of by a fused k_compose.

The scene is the m=12 terrain (288 triangles, normals within ~11 degrees of +y) at 100x52: no multiple of the tile, so paths without a pixel
exist.  A light far above is answered at emission for every hit (every hit finishes), a light low and aside for none.  What the oracle can say
about a case's population -- the hits of generation 0 and 1 -- is taken from its stats and asserted; what only the library decides (which
reflections are answered at emission) is bounded by it: every generation-1 hit has a listed parent."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 100, 52
SLOTS = ((W + 63) // 64) * ((H + 7) // 8) * 512   # pixel slots of the frame's tiles
FAR_ABOVE = (0.0, 5000.0, 0.0)     # every hit sees it straight above: always answered
LOW_ASIDE = (400.0, 1.0, 0.0)      # the way to it is nearly horizontal: never answered
NEAR_ABOVE = (10.0, 6.0, 0.0)      # steep from the hits below it, flat from the hits far away
DEFAULT = ((0, 60, 110), (0, 0, 0))
GRAZING = ((0, 1.5, 80), (0, 1, 0))        # low over the terrain: reflections leave nearly horizontally and some meet the next rise
INSIDE = ((0, 3, 0), (30, 0, 30))          # inside the root box, above the surface
CORNER = ((0, 60, 110), (90, 20, 0))       # the terrain in the lower left corner only
AWAY = ((0, 60, 110), (0, 60, 300))


def hf_spec(xrt, cam=DEFAULT, lights=(FAR_ABOVE,), R=2, ms16=False):
    s = xrt.configs.SceneSpec("heightfield_m12")
    s.meshes.append((xrt.fixtures.heightfield(12), xrt.configs.material(0.3)))
    s.objects.append(([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    s.camera = xrt.configs.camera(*cam)
    s.lights = [l if isinstance(l, dict) else xrt.configs.spot(l) for l in lights]
    s.max_reflections = R
    s.multisampling = xrt.abi.MS_FIXED16 if ms16 else xrt.abi.MS_OFF
    s.mesh_threshold = 8
    return s.with_size(W, H)


def build(xrt, monkeypatch, spec, env):
    with monkeypatch.context() as m:   # (xrt_scene_create reads the switches; whatever the environment held before comes back)
        for k, v in env.items():
            m.setenv(k, v)
        return xrt.configs.build_product(copy.deepcopy(spec))


def samples(spec, xrt):
    return 16 if spec.multisampling == xrt.abi.MS_FIXED16 else 1


_ORACLE = {}


def oracle(orc, spec, R=None):
    """(rgba, stats) of the oracle, computed once per frame description"""
    s = copy.deepcopy(spec)
    if R is not None:
        s.max_reflections = R
    key = (repr(s.camera), repr(s.lights), s.max_reflections, s.multisampling, s.name)
    if key not in _ORACLE:
        rgba, _, st = orc.OracleScene(s).render(nthreads=8, want_float=False)
        rgba.setflags(write=False)
        _ORACLE[key] = (rgba, st)
    return _ORACLE[key]


def generation_hits(orc, spec):
    """hits of generation 0 and of generation 1 (a chain: the shaded hits of depth k minus those of depth k - 1)"""
    h0 = oracle(orc, spec, 0)[1]["shaded_hits"]
    h1 = oracle(orc, spec, 1)[1]["shaded_hits"] - h0 if spec.max_reflections >= 1 else 0
    return h0, h1


def live_rays(xrt, monkeypatch, spec, render=None):
    """Primary rays that reach the root box: with no lights, no reflections and nothing answered at emission xrt_stats.rays_traversed is
    the closest-hit rays minus those k_raygen answered."""
    s = copy.deepcopy(spec)
    s.lights, s.max_reflections = [], 0
    scene, tracer = build(xrt, monkeypatch, s, {"XRT_AE": "0"})
    st = render(tracer) if render else (tracer.Render(), tracer.last_stats)[1]
    assert scene.EndCounts() == (0, 0, 0)   # (not answered at emission: nothing finishes, nothing ends early)
    return st["rays_traversed"]


def check(xrt, orc, monkeypatch, spec, env=None):
    """The frame with the switch on and off against the oracle and each other; returns (k_raygen, k_shade, list) of the engaged frame, live rays."""
    o_rgba, o_st = oracle(orc, spec)
    got = []
    for sw in ("1", "0"):
        e = {"XRT_END_EARLY": sw}
        e.update(env or {})
        scene, tracer = build(xrt, monkeypatch, spec, e)
        rgba = tracer.Render().copy()
        assert np.array_equal(rgba, o_rgba), "XRT_END_EARLY=%s: %d RGBA8 pixels differ from the oracle" % (sw, int((rgba != o_rgba).sum()))
        for k in ("rays_closest", "rays_shadow", "shaded_hits", "pixels"):
            assert tracer.last_stats[k] == o_st[k], (sw, k, tracer.last_stats[k], o_st[k])
        got.append((rgba, scene.EndCounts()))
    assert np.array_equal(got[0][0], got[1][0])
    assert got[1][1] == (0, 0, 0), got[1][1]
    counts = got[0][1]
    paths, live = SLOTS * samples(spec, xrt), live_rays(xrt, monkeypatch, spec)
    print("end counts", spec.camera["pos"], [l["position"] for l in spec.lights], spec.max_reflections, samples(spec, xrt), counts, "paths", paths, "live", live)
    assert sum(counts) == paths, (counts, paths)
    assert counts[0] == paths - live, (counts, paths, live)
    return counts, live


@pytest.mark.parametrize("ms16", [False, True], ids=["1spp", "16spp"])
class TestPopulations:
    def test_every_hit_terminal(self, xrt, orc, monkeypatch, ms16):
        """Light far above, MaxReflections 0: every hit finishes and has no next ray; the list is empty, k_shade colours every live path."""
        spec = hf_spec(xrt, R=0, ms16=ms16)
        h0, _ = generation_hits(orc, spec)
        assert h0 > 1000
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert counts[2] == 0 and counts[1] == live

    def test_reflections_answered_at_emission(self, xrt, orc, monkeypatch, ms16):
        """The same with MaxReflections 2: the oracle finds no generation-1 hit from above, and the reflection of a hit leaves the terrain at the
        ray's own 20 - 40 degrees give or take twice the surface's tilt, above every triangle's plane for most hits: most hits are terminal."""
        spec = hf_spec(xrt, R=2, ms16=ms16)
        h0, h1 = generation_hits(orc, spec)
        assert h0 > 1000 and h1 == 0
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert counts[2] < h0 // 2 and counts[1] == live - counts[2]

    def test_grazing_camera_some_paths_go_on(self, xrt, orc, monkeypatch, ms16):
        """Low over the terrain: the oracle shows generation-1 hits, each of which has a listed parent; the hits on the slopes that face the camera
        reflect steeply upwards and are terminal."""
        spec = hf_spec(xrt, cam=GRAZING, R=2, ms16=ms16)
        h0, h1 = generation_hits(orc, spec)
        assert h1 > 0 and h0 > 4 * h1
        counts, _ = check(xrt, orc, monkeypatch, spec)
        assert h1 <= counts[2] < h0, (counts, h0, h1)

    def test_no_hit_finishes(self, xrt, orc, monkeypatch, ms16):
        """Light low and aside: every hit emits its shadow ray, so every hit is listed and k_shade colours the misses alone."""
        spec = hf_spec(xrt, lights=(LOW_ASIDE,), R=2, ms16=ms16)
        h0, _ = generation_hits(orc, spec)
        assert h0 > 1000
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert counts[2] == h0 and counts[1] == live - h0

    def test_two_lights_one_of_each_kind(self, xrt, orc, monkeypatch, ms16):
        """A directional light from straight above (always answered) and a spot light a little above the terrain (answered from the hits below it,
        emitted from the hits far away), MaxReflections 0: terminal and listed hits side by side."""
        spec = hf_spec(xrt, lights=(xrt.configs.directional((0.0, -1.0, 0.0)), NEAR_ABOVE), R=0, ms16=ms16)
        h0, _ = generation_hits(orc, spec)
        assert h0 > 1000
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert 0 < counts[2] < h0 and counts[1] == live - counts[2], (counts, h0)

    def test_no_lights(self, xrt, orc, monkeypatch, ms16):
        """nLights == 0: every hit finishes with a light sum of zero; without reflections none is listed."""
        counts, live = check(xrt, orc, monkeypatch, hf_spec(xrt, lights=(), R=0, ms16=ms16))
        assert counts[2] == 0 and counts[1] == live
        check(xrt, orc, monkeypatch, hf_spec(xrt, lights=(), R=2, ms16=ms16))


def test_camera_inside_the_root_box(xrt, orc, monkeypatch):
    """Every pixel's ray starts inside the root box: k_raygen colours the paths without a pixel and no other."""
    spec = hf_spec(xrt, cam=INSIDE, ms16=True)
    counts, live = check(xrt, orc, monkeypatch, spec)
    assert live == W * H * 16 and counts[0] == (SLOTS - W * H) * 16


def test_terrain_in_a_corner(xrt, orc, monkeypatch):
    """The terrain covers the lower left corner (oracle: nothing lit right of x = 52 or above y = 30): most pixels lie outside the screen rectangle of
    the root box, k_raygen builds no ray for them."""
    for ms16 in (False, True):
        spec = hf_spec(xrt, cam=CORNER, ms16=ms16)
        lit = (oracle(orc, spec)[0] & 0xffffff).reshape(H, W) != 0
        assert lit.any() and not lit[:, 53:].any() and not lit[:30, :].any()
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert 0 < live < W * H * samples(spec, xrt) // 2


def test_camera_looking_away(xrt, orc, monkeypatch):
    """No ray reaches the root box: every path ends in k_raygen."""
    for ms16 in (False, True):
        spec = hf_spec(xrt, cam=AWAY, ms16=ms16)
        assert generation_hits(orc, spec) == (0, 0)
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert live == 0 and counts == (SLOTS * samples(spec, xrt), 0, 0)


@pytest.mark.parametrize("ms16", [False, True], ids=["1spp", "16spp"])
def test_three_shards(xrt, orc, monkeypatch, ms16):
    """shard_count 3, every rank: a rank's frame is its tiles (tile-contiguous output, a path without a pixel is cleared); gathered and de-tiled it
    is the oracle's frame, and every rank's counts add up to its own paths."""
    import torch
    spec = hf_spec(xrt, cam=GRAZING, lights=(NEAR_ABOVE,), R=2, ms16=ms16)
    o_rgba, _ = oracle(orc, spec)
    tx, ty, tpr = xrt.dist.shard_layout(W, H, 3)
    n = tpr * 512
    lives = []
    part = torch.zeros(n, dtype=torch.int32, device="cuda")
    for r in range(3):
        lives.append(live_rays(xrt, monkeypatch, spec, lambda t, r=r: t.RenderDevice(part.data_ptr(), shard_rank=r, shard_count=3)))
    assert sum(lives) == live_rays(xrt, monkeypatch, spec)
    frames = []
    for sw in ("1", "0"):
        scene, tracer = build(xrt, monkeypatch, spec, {"XRT_END_EARLY": sw})
        gathered = torch.full((3 * n,), 0x55, dtype=torch.int32, device="cuda")
        for r in range(3):
            tracer.RenderDevice(gathered[r * n:(r + 1) * n].data_ptr(), shard_rank=r, shard_count=3)
            counts = scene.EndCounts()
            if sw == "0":
                assert counts == (0, 0, 0)
                continue
            paths = n * samples(spec, xrt)
            assert sum(counts) == paths and counts[0] == paths - lives[r], (r, counts, paths, lives[r])
        out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        xrt.dist.detile_device(gathered, W, H, 3, out)
        torch.cuda.synchronize()
        frames.append(gathered.cpu().numpy())
        assert np.array_equal(out.cpu().numpy().view(np.uint32), o_rgba), sw
    assert np.array_equal(frames[0], frames[1])   # (the slots without a pixel too)


@pytest.mark.parametrize("ms16", [False, True], ids=["1spp", "16spp"])
def test_two_frames_in_flight(xrt, orc, monkeypatch, ms16):
    """Two frames in flight, A B A B B A A B: A lists every hit (light low and aside, MaxReflections 2), B lists none (light far above, MaxReflections 0).
    Each frame context sees both kinds one after the other -- the count words, their clearing and the grid hint of a long list meet an empty list and the
    other way round.  Every frame is compared with the oracle, and its counts with the blocking frame's."""
    import torch
    A, B = hf_spec(xrt, lights=(LOW_ASIDE,), R=2, ms16=ms16), hf_spec(xrt, lights=(FAR_ABOVE,), R=0, ms16=ms16)
    want = {}
    for name, spec in (("A", A), ("B", B)):
        counts, _ = check(xrt, orc, monkeypatch, spec)
        want[name] = (oracle(orc, spec)[0], counts)
    assert want["A"][1][2] > 1000 and want["B"][1][2] == 0
    scene, tracer = build(xrt, monkeypatch, A, {"XRT_END_EARLY": "1"})
    outs = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in range(2)]
    frs = {}
    for name, spec in (("A", A), ("B", B)):   # (camera, lights and options are marshalled when the frame is prepared)
        tracer.MaxReflections = spec.max_reflections
        tracer.Lights.clear()
        L = xrt.SpotLight()
        l = spec.lights[0]
        L.Position, L.SpotAngle, L.DecayExponent, L.Direction, L.Color, L.Intensity = l["position"], l["spot_angle"], l["decay_exponent"], l["direction"], l["color"], l["intensity"]
        tracer.Lights.append(L)
        frs[name] = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
    order = "ABABBAAB"
    tickets = [None, None]
    for f in range(len(order) + 1):
        cur = f & 1
        if f < len(order):
            tickets[cur] = frs[order[f]][cur].begin()
        if f >= 1:   # the frame begun one step ago was open while this one was enqueued
            prv = cur ^ 1
            name = order[f - 1]
            frs[name][prv].end(tickets[prv])
            counts = scene.EndCounts()
            torch.cuda.synchronize()
            assert np.array_equal(outs[prv].cpu().numpy().view(np.uint32), want[name][0]), (f, name)
            assert counts == want[name][1], (f, name, counts, want[name][1])
            outs[prv].zero_()
            torch.cuda.synchronize()   # (the next frame into this buffer runs on the library's own stream)


def test_under_guards(xrt, orc, monkeypatch):
    """XRT_GUARD=1: every work buffer ends in a checked pattern -- the compose list, with its count words in front, among them."""
    try:
        for ms16 in (False, True):
            counts, _ = check(xrt, orc, monkeypatch, hf_spec(xrt, cam=GRAZING, lights=(NEAR_ABOVE,), R=2, ms16=ms16), env={"XRT_GUARD": "1"})
            assert counts[2] > 0
    finally:
        build(xrt, monkeypatch, xrt.configs.crate_scene(32, 32, 0), {"XRT_GUARD": "0"})   # (xrt_scene_create reads the switch: guards off for the tests that follow)


def on_off(xrt, monkeypatch, spec, frame):
    """frame(scene, tracer) -> arrays, with the switch on and off: identical, and neither engaged"""
    got = []
    for sw in ("1", "0"):
        scene, tracer = build(xrt, monkeypatch, spec, {"XRT_END_EARLY": sw})
        got.append([np.array(a).copy() for a in frame(scene, tracer)])
        assert scene.EndCounts() == (0, 0, 0), sw
    for a, b in zip(*got):
        assert a.tobytes() == b.tobytes()
    return got[0]


def test_frames_that_do_not_engage(xrt, orc, monkeypatch):
    """A ray tree (Transparent materials), adaptive supersampling, a float-output render, a frame with the counting pass and xrt_cast_rays keep
    the long way round: counts all zero, pixels as ever."""
    game = xrt.configs.default_game_scene(64, 64, 4)
    rgba, = on_off(xrt, monkeypatch, game, lambda s, t: (t.Render(),))
    assert np.array_equal(rgba, oracle(orc, game)[0])
    adaptive = hf_spec(xrt)
    adaptive.multisampling, adaptive.multisample_quality = xrt.abi.MS_ADAPTIVE, 1
    rgba, = on_off(xrt, monkeypatch, adaptive, lambda s, t: (t.Render(),))
    assert np.array_equal(rgba, oracle(orc, adaptive)[0])
    plain = hf_spec(xrt)
    o_rgba, o_rgbf, _ = orc.OracleScene(plain).render(nthreads=8)
    rgba, rgbf = on_off(xrt, monkeypatch, plain, lambda s, t: t.Render(want_float=True))
    assert np.array_equal(rgba, o_rgba) and np.array_equal(rgbf.view(np.uint32), o_rgbf.view(np.uint32))

    def counted(s, t):
        t.collect_stats = True
        return (t.Render(),)
    rgba, = on_off(xrt, monkeypatch, plain, counted)
    assert np.array_equal(rgba, o_rgba)
    cast, = on_off(xrt, monkeypatch, plain, lambda s, t: (t.CastRays(t.GeneratePrimaryRays()),))
    assert np.array_equal(cast, o_rgba)   # (the primary rays of a one-sample frame, cast one by one, are the frame)
