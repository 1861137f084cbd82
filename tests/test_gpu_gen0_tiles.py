"""Tiles outside the root box's screen rectangle take no part in a frame that ends paths early (kernels.h EndArgs::skipTiles): where such a frame has
a level map (xrt_core.h LvlMap: plain unsharded one-chunk frames) and more than one sample per pixel, k_raygen walks the tiles that overlap the rectangle and writes nothing for the
others, and k_resolve writes the constant colour of a path that ended at generation 0 for every pixel outside the rectangle without reading its
samples.  Nothing a caller can see may change: every frame is compared bit for bit with the oracle's RGBA8 and with the same frame under
XRT_END_EARLY=0, and xrt_debug_end_counts keeps its meaning -- the three counts sum to the frame's paths, k_raygen's share (the paths of the
tiles it never walked included) is the paths minus the live primary rays.

The scene is the m=12 terrain of tests/test_gpu_end_early.py (root box x, z in [-50, 50], |y| < 3.8).  Which tiles a camera keeps is worked out here as
the host works it out (screen_rect below: the root box's eight corners projected, two pixels and a thousandth of the viewport of margin, clipped)
and asserted per case, so that a case says what it exercises:

    camera        frame     rectangle (x0, y0, x1, y1)   tiles kept
    OFFSIDE       128x64    empty (left of the screen)   none: no level map, every tile is walked as before
    CORNER_TILE   128x64    (0, 57, 16, 63)              1 of 16: the lower left one
    DEFAULT       128x64    (13, 17, 115, 60)            12 of 16; culled pixels inside every kept tile
    CORNER        200x50    (0, 27, 103, 49)             8 of 28; the frame is no multiple of 64x8, the kept tiles of the last row have paths without a pixel
    CORNER        150x52    (0, 28, 78, 51)              8 of 21; the same
    INSIDE        128x64    the whole frame              16 of 16: no level map (nothing to leave out)

The one-sample cases run the walk over every tile, as before (the host keeps it there); they are here because the level map and the rectangle are theirs too.

A skipped tile's words of the context's sample buffer keep what an earlier frame left there: test_stale_samples renders a frame with the terrain in the
middle and then, on the same scene object, one with the terrain in a corner."""
import copy
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAR_ABOVE = (0.0, 5000.0, 0.0)     # every hit sees it straight above: always answered at emission
NEAR_ABOVE = (10.0, 6.0, 0.0)      # steep from the hits below it, flat from the hits far away
DEFAULT = ((0, 60, 110), (0, 0, 0))
INSIDE = ((0, 3, 0), (30, 0, 30))          # inside the root box, above the surface
CORNER = ((0, 60, 110), (90, 20, 0))       # the terrain in the lower left corner only

OFFSIDE = ((0, 20, 850), (1000, 20, 0))        # the terrain lies 50 degrees to the left of the view axis: in front of the eye, off the screen
CORNER_TILE = ((0, 20, 850), (600, 365, 0))    # far away and small, in the lower left corner


def hf_spec(xrt, size, cam=DEFAULT, lights=(FAR_ABOVE,), R=2, ms16=False):
    s = xrt.configs.SceneSpec("heightfield_m12")
    s.meshes.append((xrt.fixtures.heightfield(12), xrt.configs.material(0.3)))
    s.objects.append(([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    s.camera = xrt.configs.camera(*cam)
    s.lights = [l if isinstance(l, dict) else xrt.configs.spot(l) for l in lights]
    s.max_reflections = R
    s.multisampling = xrt.abi.MS_FIXED16 if ms16 else xrt.abi.MS_OFF
    s.mesh_threshold = 8
    return s.with_size(*size)


def build(xrt, monkeypatch, spec, env):
    with monkeypatch.context() as m:   # (xrt_scene_create reads the switches; whatever the environment held before comes back)
        for k, v in env.items():
            m.setenv(k, v)
        return xrt.configs.build_product(copy.deepcopy(spec))


def samples(spec, xrt):
    return 16 if spec.multisampling == xrt.abi.MS_FIXED16 else 1


def screen_rect(xrt, spec):
    """The screen rectangle of the root box as xrt_api.cpp make_raygen forms it (x1 < x0 or y1 < y0: empty; the whole frame when a corner is not
    safely in front of the eye), and the tiles that overlap it: (x0, y0, x1, y1), kept, tiles."""
    W, H, c = spec.width, spec.height, spec.camera
    cam = xrt.api.Camera(c["pos"], c["target"], c["up"], c["fov"], xrt.xna.aspect_ratio(W, H), c["near"], c["far"])
    view = np.array([float(x) for x in cam.View], dtype=np.float32).reshape(4, 4)
    proj = np.array([float(x) for x in cam.Projection], dtype=np.float32).reshape(4, 4)
    wvp = (view @ proj).astype(np.float64)
    box = np.asarray(spec.meshes[0][0].bbox, dtype=np.float64).reshape(-1)   # (one body at the origin, unrotated: the scene's root box is the mesh's)
    tiles = ((W + 63) // 64) * ((H + 7) // 8)
    xs, ys = [], []
    for k in range(8):
        p = (box[3 if k & 1 else 0], box[4 if k & 2 else 1], box[5 if k & 4 else 2])
        v = [p[0] * wvp[0][j] + p[1] * wvp[1][j] + p[2] * wvp[2][j] + wvp[3][j] for j in range(4)]
        if not v[3] > 1e-3 * sum(abs(t) for t in v):
            return (0, 0, W - 1, H - 1), tiles, tiles
        xs.append((v[0] / v[3] + 1.0) * 0.5 * W)
        ys.append((1.0 - v[1] / v[3]) * 0.5 * H)
    mx, my = 2.0 + 1e-3 * W, 2.0 + 1e-3 * H
    r = (int(max(0, min(math.floor(min(xs) - mx), W))), int(max(0, min(math.floor(min(ys) - my), H))),
         int(min(W - 1, max(math.ceil(max(xs) + mx), -1))), int(min(H - 1, max(math.ceil(max(ys) + my), -1))))
    kept = (r[2] // 64 - r[0] // 64 + 1) * (r[3] // 8 - r[1] // 8 + 1) if r[2] >= r[0] and r[3] >= r[1] else 0
    return r, kept, tiles


_ORACLE = {}


def oracle(orc, spec):
    key = (repr(spec.camera), repr(spec.lights), spec.max_reflections, spec.multisampling, spec.width, spec.height)
    if key not in _ORACLE:
        rgba, _, st = orc.OracleScene(copy.deepcopy(spec)).render(nthreads=8, want_float=False)
        rgba.setflags(write=False)
        _ORACLE[key] = (rgba, st)
    return _ORACLE[key]


def paths_of(spec, xrt):
    return ((spec.width + 63) // 64) * ((spec.height + 7) // 8) * 512 * samples(spec, xrt)


def live_rays(xrt, monkeypatch, spec):
    """primary rays that reach the root box (tests/test_gpu_end_early.py live_rays)"""
    s = copy.deepcopy(spec)
    s.lights, s.max_reflections = [], 0
    scene, tracer = build(xrt, monkeypatch, s, {"XRT_AE": "0"})
    tracer.Render()
    assert scene.EndCounts() == (0, 0, 0)
    return tracer.last_stats["rays_traversed"]


def check(xrt, orc, monkeypatch, spec, env=None):
    """The frame with XRT_END_EARLY on and off against the oracle and each other; the counts of the engaged frame."""
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
        again = tracer.Render().copy()   # (the same context or the other one: its sample buffer holds the frame before)
        assert np.array_equal(again, o_rgba), sw
        got.append((rgba, scene.EndCounts()))
    assert np.array_equal(got[0][0], got[1][0])
    assert got[1][1] == (0, 0, 0), got[1][1]
    counts, paths, live = got[0][1], paths_of(spec, xrt), live_rays(xrt, monkeypatch, spec)
    print("end counts", spec.width, spec.height, spec.camera["pos"], samples(spec, xrt), counts, "paths", paths, "live", live, "rect", screen_rect(xrt, spec))
    assert sum(counts) == paths, (counts, paths)
    assert counts[0] == paths - live, (counts, paths, live)
    return counts, live


@pytest.mark.parametrize("ms16", [False, True], ids=["1spp", "16spp"])
class TestRectangles:
    def test_no_tile(self, xrt, orc, monkeypatch, ms16):
        spec = hf_spec(xrt, (128, 64), cam=OFFSIDE, ms16=ms16)
        r, kept, tiles = screen_rect(xrt, spec)
        assert kept == 0 and r[2] < r[0]
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert live == 0 and counts == (paths_of(spec, xrt), 0, 0)

    def test_one_corner_tile(self, xrt, orc, monkeypatch, ms16):
        spec = hf_spec(xrt, (128, 64), cam=CORNER_TILE, ms16=ms16)
        r, kept, tiles = screen_rect(xrt, spec)
        assert kept == 1 and tiles == 16 and r[0] == 0 and r[1] >= 56 and r[2] < 64 and r[3] == 63
        assert (oracle(orc, spec)[0] & 0xffffff).any()   # (something of the terrain is seen)
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert 0 < live <= (r[2] - r[0] + 1) * (r[3] - r[1] + 1) * samples(spec, xrt)

    def test_rectangle_ends_inside_tiles(self, xrt, orc, monkeypatch, ms16):
        spec = hf_spec(xrt, (128, 64), cam=DEFAULT, ms16=ms16)
        r, kept, tiles = screen_rect(xrt, spec)
        assert 1 < kept < tiles and r[0] % 64 and (r[2] + 1) % 64 and r[1] % 8 and (r[3] + 1) % 8   # culled pixels on every side, inside kept tiles
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert live > 1000 * samples(spec, xrt)

    def test_whole_frame(self, xrt, orc, monkeypatch, ms16):
        spec = hf_spec(xrt, (128, 64), cam=INSIDE, ms16=ms16)
        r, kept, tiles = screen_rect(xrt, spec)
        assert kept == tiles == 16
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert live == 128 * 64 * samples(spec, xrt) and counts[0] == 0

    @pytest.mark.parametrize("size,cam", [((200, 50), CORNER), ((150, 52), CORNER)], ids=["200x50", "150x52"])
    def test_frame_no_multiple_of_the_tile(self, xrt, orc, monkeypatch, ms16, size, cam):
        spec = hf_spec(xrt, size, cam=cam, ms16=ms16)
        r, kept, tiles = screen_rect(xrt, spec)
        assert 1 < kept < tiles and r[3] // 8 == (size[1] - 1) // 8 and size[1] % 8   # kept tiles in the last, partial tile row: paths without a pixel
        counts, live = check(xrt, orc, monkeypatch, spec)
        assert live > 500 * samples(spec, xrt)


def set_camera(xrt, tracer, spec):
    c = spec.camera
    tracer.CurrentCamera = xrt.api.Camera(c["pos"], c["target"], c["up"], c["fov"], xrt.xna.aspect_ratio(spec.width, spec.height), c["near"], c["far"])


@pytest.mark.parametrize("ms16", [False, True], ids=["1spp", "16spp"])
def test_stale_samples(xrt, orc, monkeypatch, ms16):
    """One scene object; M sees the terrain in the middle (12 tiles of 16 kept), C in the lower left corner (8 of 16, among them tiles M keeps and tiles
    it does not).  After an M frame the tiles a C frame skips hold M's colours in the context's sample buffer -- and the other way round.  Blocking
    frames M M C C M C, then two in flight in the order M M C C M C C M (each context sees both cameras one after the other); every frame is the oracle's."""
    import torch
    M, Cc = hf_spec(xrt, (128, 64), cam=DEFAULT, ms16=ms16), hf_spec(xrt, (128, 64), cam=CORNER, ms16=ms16)
    (rm, km, tiles), (rc, kc, _) = screen_rect(xrt, M), screen_rect(xrt, Cc)
    assert 1 < kc < km < tiles and rc[0] < rm[0] and rm[2] > rc[2] and rm[1] < rc[1]
    want = {"M": oracle(orc, M)[0], "C": oracle(orc, Cc)[0]}
    lit_m, lit_c = (want["M"] & 0xffffff) != 0, (want["C"] & 0xffffff) != 0
    assert (lit_m & ~lit_c).sum() > 500   # pixels M lights and C leaves black: stale samples would show
    scene, tracer = build(xrt, monkeypatch, M, {"XRT_END_EARLY": "1"})
    specs = {"M": M, "C": Cc}
    for f, name in enumerate("MMCCMC"):
        set_camera(xrt, tracer, specs[name])
        rgba = tracer.Render()
        assert np.array_equal(rgba, want[name]), ("blocking", f, name, int((rgba != want[name]).sum()))
        assert sum(scene.EndCounts()) == paths_of(M, xrt)
    outs = [torch.zeros(128 * 64, dtype=torch.int32, device="cuda") for _ in range(2)]
    frs = {}
    for name in "MC":   # (the camera is marshalled when the frame is prepared)
        set_camera(xrt, tracer, specs[name])
        frs[name] = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
    order = "MMCCMCCM"
    tickets = [None, None]
    for f in range(len(order) + 1):
        cur = f & 1
        if f < len(order):
            tickets[cur] = frs[order[f]][cur].begin()
        if f >= 1:
            prv = cur ^ 1
            name = order[f - 1]
            frs[name][prv].end(tickets[prv])
            assert sum(scene.EndCounts()) == paths_of(M, xrt)
            torch.cuda.synchronize()
            got = outs[prv].cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want[name]), ("in flight", f, name, int((got != want[name]).sum()))
            outs[prv].zero_()
            torch.cuda.synchronize()   # (the next frame into this buffer runs on the library's own stream)


@pytest.mark.parametrize("ms16", [False, True], ids=["1spp", "16spp"])
def test_other_frame_kinds(xrt, orc, monkeypatch, ms16):
    """The frames that have no level map run as they did: three shards (round-robin and by a tile table) and XRT_LEVEL_MAP=0 give the unsharded render,
    which is the oracle's.  Every kind is rendered twice on its scene object, after an unsharded frame of another camera."""
    import torch
    W, H = 200, 50
    spec, other = hf_spec(xrt, (W, H), cam=CORNER, lights=(NEAR_ABOVE,), ms16=ms16), hf_spec(xrt, (W, H), cam=DEFAULT, lights=(NEAR_ABOVE,), ms16=ms16)
    r, kept, tiles = screen_rect(xrt, spec)
    assert 1 < kept < tiles == 28
    o_rgba = oracle(orc, spec)[0]
    scene, tracer = build(xrt, monkeypatch, spec, {"XRT_END_EARLY": "1"})
    whole = tracer.Render().copy()
    assert np.array_equal(whole, o_rgba)
    paths = paths_of(spec, xrt)
    assert sum(scene.EndCounts()) == paths
    s0, t0 = build(xrt, monkeypatch, spec, {"XRT_END_EARLY": "1", "XRT_LEVEL_MAP": "0"})
    for _ in range(2):
        assert np.array_equal(t0.Render(), whole)
        assert sum(s0.EndCounts()) == paths
    tx, ty, tpr = xrt.dist.shard_layout(W, H, 3)
    order = np.arange(tiles)[::-1]
    tprb = 12
    table = np.full(3 * tprb, -1, dtype=np.int32)
    table[0:12] = order[:12]; table[12:12 + 10] = order[12:22]; table[24:24 + 6] = order[22:]
    for kind, n, tab in (("round robin", tpr * 512, None), ("table", tprb * 512, table)):
        if tab is not None:
            tracer.SetTileTable(3, tprb, tab)
        for rep in range(2):
            set_camera(xrt, tracer, other)
            tracer.Render()   # an unsharded frame of another camera in between: its samples are in the context
            set_camera(xrt, tracer, spec)
            gathered = torch.full((3 * n,), 0x55, dtype=torch.int32, device="cuda")
            total = 0
            for rank in range(3):
                tracer.RenderDevice(gathered[rank * n:(rank + 1) * n].data_ptr(), shard_rank=rank, shard_count=3)
                total += sum(scene.EndCounts())
            assert total == 3 * n * samples(spec, xrt), (kind, total)
            out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
            if tab is None:
                xrt.dist.detile_device(gathered, W, H, 3, out)
            else:
                xrt.dist.detile_device(gathered, W, H, 3, out, table_dev=torch.from_numpy(tab).cuda(), tiles_per_rank=tprb)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), whole), (kind, rep)
        if tab is not None:
            tracer.SetTileTable(3, tprb, None)
    assert np.array_equal(tracer.Render(), whole)
