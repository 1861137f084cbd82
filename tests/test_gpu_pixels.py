"""xrt_render_pixels on the GPU: the colour of caller-chosen screen positions (GetColorForQuadrant / the body of Render's inner loop, RT:215-311,
412-425).  Expectations are the oracle's frames (tests/pixels_py.py says how a frame pins a fractional or an outside centre; tests/test_pixels_cpu.py
shows on the CPU that those lookups are sound and that the slip pixels reach RT:305) and, bit for bit, the library's own frames."""
import ctypes as C
import os

import numpy as np
import pytest

import pixels_py as px
from test_pixels_cpu import SLIP_PIXELS

pytestmark = pytest.mark.gpu

BLACK = 0xFF000000
W, H = 96, 54


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def set_mode(xrt, tracer, ms, quality=0):
    tracer.UseMultisampling = ms != xrt.abi.MS_OFF
    tracer.MultisampleMode = ms if ms != xrt.abi.MS_OFF else None
    tracer.MultisampleQuality = quality


def modes(xrt):
    a = xrt.abi
    return [(a.MS_OFF, 0), (a.MS_ADAPTIVE, 0), (a.MS_ADAPTIVE, 2), (a.MS_FIXED16, 0)]


class Case:
    """A scene on the GPU and in the oracle, and its frames by mode, each rendered once."""

    def __init__(self, xrt, orc, spec):
        self.xrt, self.orc, self.spec = xrt, orc, spec
        self.osc = orc.OracleScene(spec)
        self.scene, self.tracer = xrt.configs.build_product(spec)
        self._oracle, self._frame = {}, {}

    def oracle(self, ms, quality=0):
        if (ms, quality) not in self._oracle:
            self.osc.spec = px.with_mode(self.spec, ms, quality)
            rgba, rgbf, st = self.osc.render()
            self._oracle[(ms, quality)] = (rgba, rgbf, st)
        return self._oracle[(ms, quality)]

    def frame(self, ms, quality=0):
        """xrt_render of the same frame: (rgba, rgbf, stats)."""
        if (ms, quality) not in self._frame:
            set_mode(self.xrt, self.tracer, ms, quality)
            rgba, rgbf = self.tracer.Render(want_float=True)
            self._frame[(ms, quality)] = (rgba.copy(), rgbf.copy(), dict(self.tracer.last_stats))
        return self._frame[(ms, quality)]

    def pixels(self, centers, ms, quality=0, **kw):
        set_mode(self.xrt, self.tracer, ms, quality)
        return self.tracer.RenderPixels(np.asarray(centers, dtype=np.float32), want_float=True, **kw)

    def check_integer(self, centers, ms, quality=0, what=""):
        """Integer centres inside the viewport: the oracle's frame and xrt_render's at the listed pixels, both arrays, every bit."""
        c = np.asarray(centers, dtype=np.float32).reshape(-1, 2)
        at = c[:, 1].astype(np.int64) * self.spec.width + c[:, 0].astype(np.int64)
        rgba, rgbf = self.pixels(c, ms, quality)
        o_rgba, o_rgbf, _ = self.oracle(ms, quality)
        f_rgba, f_rgbf, _ = self.frame(ms, quality)
        assert np.array_equal(rgba, o_rgba[at]), (what, ms, quality, int((rgba != o_rgba[at]).sum()))
        assert np.array_equal(_bits(rgbf), _bits(o_rgbf[at])), (what, ms, quality)
        assert np.array_equal(rgba, f_rgba[at]) and np.array_equal(_bits(rgbf), _bits(f_rgbf[at])), (what, ms, quality)
        assert self.tracer.last_stats["pixels"] == len(c)
        return rgba


@pytest.fixture(scope="module")
def grid(xrt, orc):
    """The 96x54 instanced-crates frame (tests/golden/c3_96x54_rgba.npy)."""
    return Case(xrt, orc, xrt.configs.crate_grid_scene(W, H))


@pytest.fixture(scope="module")
def crate(xrt, orc):
    return Case(xrt, orc, xrt.configs.crate_scene(W, H, max_reflections=2))


@pytest.fixture(scope="module")
def scrambled():
    return px.grid_centers(W, H)[np.random.default_rng(20261020).permutation(W * H)]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_whole_frame_as_a_scrambled_list(xrt, grid, scrambled, which):
    """Every pixel of the frame in a fixed permutation (5184 entries: past the 4096-path group of the append kernels): the oracle's frame and
    xrt_render's, bit for bit, and the frame's ray and hit counts."""
    ms, quality = modes(xrt)[which]
    rgba = grid.check_integer(scrambled, ms, quality, "scrambled")
    assert len(np.unique(rgba)) > 500
    st, (_, _, o_st), (_, _, f_st) = dict(grid.tracer.last_stats), grid.oracle(ms, quality), grid.frame(ms, quality)
    for k in ("rays_closest", "rays_shadow", "hits_closest", "shaded_hits"):
        assert st[k] == o_st[k], (k, st[k], o_st[k])
    for k in ("rays_closest", "rays_shadow"):
        assert st[k] == f_st[k], (k, st[k], f_st[k])
    if which == 0:
        assert np.array_equal(grid.frame(ms)[0], np.load(os.path.join(px._HERE, "golden", "c3_96x54_rgba.npy")))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_list_lengths(xrt, grid, scrambled, n):
    """Wave and group boundaries of the list kernels."""
    for ms, quality in modes(xrt):
        grid.check_integer(scrambled[:n], ms, quality, "n = %d" % n)


def test_duplicates(xrt, grid, scrambled):
    c = np.repeat(scrambled[:700], 2, axis=0)
    for ms, quality in modes(xrt):
        rgba = grid.check_integer(c, ms, quality, "duplicates")
        assert np.array_equal(rgba[0::2], rgba[1::2])


def test_all_miss_and_mixed_lists(xrt, crate):
    """Centres whose rays cannot reach the scene's root box: nothing is traversed and every entry is black (RT:732); alternating with hits,
    every entry keeps its own answer."""
    a = xrt.abi
    lit = np.all([crate.oracle(ms, quality)[0] != BLACK for ms, quality in modes(xrt)], axis=0)   # pixels that see the crate in every mode
    hits = px.grid_centers(W, H)[lit]
    n = len(hits)
    assert n >= 60
    far = np.stack([np.linspace(-4000.0, 4000.0, n), np.full(n, -3000.5)], axis=1).astype(np.float32)
    mixed = np.empty((2 * n, 2), dtype=np.float32)
    mixed[0::2], mixed[1::2] = hits, far
    for ms, quality in modes(xrt):
        rgba, rgbf = crate.pixels(far, ms, quality)
        assert np.all(rgba == BLACK) and not rgbf.any(), (ms, quality)
        st = crate.tracer.last_stats
        assert st["rays_traversed"] == 0 and st["hits_closest"] == 0 and st["pixels"] == n
        assert st["rays_closest"] == n * (1 if ms == a.MS_OFF else 16 if ms == a.MS_FIXED16 else 4)
        rgba, rgbf = crate.pixels(mixed, ms, quality)
        o_rgba, o_rgbf, _ = crate.oracle(ms, quality)
        at = hits[:, 1].astype(np.int64) * W + hits[:, 0].astype(np.int64)
        assert np.array_equal(rgba[0::2], o_rgba[at]) and np.array_equal(_bits(rgbf[0::2]), _bits(o_rgbf[at])), (ms, quality)
        assert np.all(rgba[0::2] != BLACK) and np.all(rgba[1::2] == BLACK) and not rgbf[1::2].any()


def test_adaptive_extremes(xrt, orc, crate):
    """No quadrant subdivides on a flat-coloured wall (four rays per entry, no more); the crate's edge against black subdivides down to
    quality 2 (the oracle casts more rays at every quality)."""
    a = xrt.abi
    wall_spec = xrt.configs.crate_scene(32, 18, max_reflections=0, textured=False)
    wall_spec.camera = xrt.configs.camera((0, 8, 20), (0, 8, 0))
    wall = Case(xrt, orc, wall_spec)
    c = px.grid_centers(32, 18)
    wall.check_integer(c, a.MS_ADAPTIVE, 2, "wall")
    assert wall.tracer.last_stats["rays_closest"] == 4 * len(c) == wall.oracle(a.MS_ADAPTIVE, 2)[2]["rays_closest"]
    counts = []
    for quality in (0, 1, 2):
        crate.check_integer(px.grid_centers(W, H), a.MS_ADAPTIVE, quality, "edge")
        counts.append(crate.tracer.last_stats["rays_closest"])
        assert counts[-1] == crate.oracle(a.MS_ADAPTIVE, quality)[2]["rays_closest"]
    assert counts[0] < counts[1] < counts[2], counts


def test_rt305_slip(xrt, crate):
    """Listed pixels whose lower-right corner subdivides (tests/test_pixels_cpu.py shows that the oracle's frame differs there from the
    slip-free fold): the library writes urColor as RT:305 does."""
    c = np.array(SLIP_PIXELS, dtype=np.float32)
    crate.check_integer(c, xrt.abi.MS_ADAPTIVE, 1, "slip")
    crate.check_integer(c[:1], xrt.abi.MS_ADAPTIVE, 1, "slip alone")


def test_fractional_centres(xrt, orc, crate):
    """XRT_MS_OFF at (x -+ 0.25, y -+ 0.25), averaged as RT:309 does, is the oracle's adaptive frame at quality 0; at the sixteen positions
    (x + (+-0.25)) + (+-0.125), as four means of four, its fixed-16 frame -- on pixels at the crate's edges."""
    a, f = xrt.abi, np.float32
    pix = SLIP_PIXELS + [(47, 30), (52, 23), (40, 34), (60, 20), (48, 27)]
    four = np.array([[f(x) + f(dx), f(y) + f(dy)] for x, y in pix for dy, dx in ((-.25, -.25), (-.25, .25), (.25, -.25), (.25, .25))], dtype=f)
    sixteen = np.array([[f(f(x) + f(ax)) + f(bx), f(f(y) + f(ay)) + f(by)] for x, y in pix for (ax, bx), (ay, by) in px.fixed16_offsets()], dtype=f)
    c4, _ = crate.pixels(four, a.MS_OFF)
    c16, _ = crate.pixels(sixteen, a.MS_OFF)
    ad0, f16 = crate.oracle(a.MS_ADAPTIVE, 0)[0], crate.oracle(a.MS_FIXED16)[0]
    edges = 0
    for i, (x, y) in enumerate(pix):
        assert px.mean4(orc, c4[4 * i:4 * i + 4]) == int(ad0[y * W + x]), (x, y)
        assert px.mean16(orc, c16[16 * i:16 * i + 16]) == int(f16[y * W + x]), (x, y)
        edges += len(set(int(v) for v in c16[16 * i:16 * i + 16])) > 1
    assert edges >= 4   # the samples of most of these pixels differ: they do lie on edges
    # the supersampled modes at a fractional centre are the same identities one level down: a quadrant of size 1 around (x + 0.5, y + 0.5)
    half = np.array([[x + 0.5, y + 0.5] for x, y in pix], dtype=f)
    q0, _ = crate.pixels(half, a.MS_ADAPTIVE, 0)
    corners = np.array([[f(cx) + f(dx), f(cy) + f(dy)] for cx, cy in half for dy, dx in ((-.25, -.25), (-.25, .25), (.25, -.25), (.25, .25))], dtype=f)
    cc, _ = crate.pixels(corners, a.MS_OFF)
    for i in range(len(pix)):
        assert px.mean4(orc, cc[4 * i:4 * i + 4]) == int(q0[i]), pix[i]


def test_outside_the_viewport(xrt, orc):
    """Centres at (-3, -2) and (W + 5, H + 1) are pixel (0, 0) of the oracle's frames whose viewport origin is shifted by those integers:
    Unproject only sees source - vp.  A close-up of the crate, so that these centres still see it."""
    spec = xrt.configs.crate_scene(32, 18, max_reflections=1)
    spec.camera = xrt.configs.camera((0, 8, 14), (0, 8, 0))
    case = Case(xrt, orc, spec)
    outside = [(-3, -2), (32 + 5, 18 + 1)]
    for ms, quality in modes(xrt):
        rgba, rgbf = case.pixels(outside, ms, quality)
        for i, (x, y) in enumerate(outside):
            o_rgba, o_rgbf = px.oracle_frame(orc, case.osc, px.with_mode(spec, ms, quality), vp=(-x, -y), rows=(0, 1))
            assert int(o_rgba[0, 0]) != BLACK
            assert int(rgba[i]) == int(o_rgba[0, 0]) and np.array_equal(_bits(rgbf[i]), _bits(o_rgbf[0, 0])), (ms, quality, x, y)


@pytest.fixture(scope="module")
def glass(xrt, orc):
    return Case(xrt, orc, xrt.configs.default_game_scene(32, 32, max_reflections=3))


def test_ray_trees(xrt, glass):
    """Transparent materials: a ray tree per ray, through the list."""
    c = px.grid_centers(32, 32)[np.random.default_rng(5).permutation(1024)]
    for ms in (xrt.abi.MS_OFF, xrt.abi.MS_FIXED16):
        rgba = glass.check_integer(c, ms, 0, "glass")
        assert len(np.unique(rgba)) > 10
        assert glass.tracer.last_stats["rays_closest"] == glass.oracle(ms)[2]["rays_closest"] > len(c) * (16 if ms else 1)
    glass.tracer.MaxReflections = 13   # the limit of frames, with its code
    try:
        with pytest.raises(xrt.abi.XrtError) as e:
            glass.pixels(c[:4], xrt.abi.MS_OFF)
        assert e.value.code == xrt.abi.XRT_E_UNSUPPORTED
    finally:
        glass.tracer.MaxReflections = 3


def test_cast_rays_cross_check(xrt, grid):
    """Without the oracle: XRT_MS_OFF on integer centres is xrt_cast_rays on the rays xrt_generate_primary_rays gives for those pixels."""
    set_mode(xrt, grid.tracer, xrt.abi.MS_OFF)
    rays = grid.tracer.GeneratePrimaryRays()
    at = np.random.default_rng(3).permutation(W * H)[:3000]
    c_rgba, c_rgbf = grid.tracer.CastRays(rays[at], want_float=True)
    rgba, rgbf = grid.pixels(px.grid_centers(W, H)[at], xrt.abi.MS_OFF)
    assert np.array_equal(rgba, c_rgba) and np.array_equal(_bits(rgbf), _bits(c_rgbf))


def test_device_form(xrt, grid, scrambled):
    """From a torch tensor on a non-default stream: the host form's answers; colours without floats; a misaligned pointer is refused."""
    import torch
    a = xrt.abi
    s = torch.cuda.Stream()
    for ms, quality in modes(xrt):
        h_rgba, h_rgbf = grid.pixels(scrambled, ms, quality)
        with torch.cuda.stream(s):
            d_c = torch.from_numpy(scrambled.copy()).to("cuda", non_blocking=False)
            d_rgba, d_rgbf = grid.tracer.RenderPixels(d_c, want_float=True, device=True, stream=s)   # (the mode is the host call's)
            only = grid.tracer.RenderPixels(d_c, device=True, stream=s)
        s.synchronize()
        assert np.array_equal(d_rgba.cpu().numpy().view(np.uint32), h_rgba), (ms, quality)
        assert np.array_equal(_bits(d_rgbf.cpu().numpy()), _bits(h_rgbf)), (ms, quality)
        assert np.array_equal(only.cpu().numpy().view(np.uint32), h_rgba)
    lib = a.lib()
    cam, opts, lights = grid.tracer._camera_abi(), grid.tracer._opts_abi(shard_count=0), grid.tracer._lights_abi()
    raw = torch.zeros(2 * 64 + 4, dtype=torch.float32, device="cuda")
    out = torch.zeros(80, dtype=torch.int32, device="cuda")
    for dc, do in ((4, 0), (0, 4)):
        rc = lib.xrt_render_pixels_device(grid.scene.handle, C.byref(cam), lights, len(grid.tracer.Lights), C.byref(opts), C.c_void_p(raw.data_ptr() + dc), 64,
                                          C.c_void_p(out.data_ptr() + do), None, None, None)
        assert rc == a.XRT_E_INVALID_ARG


def test_the_split_changes_nothing(xrt, orc, monkeypatch, grid, scrambled):
    """A byte budget that cuts the list into many chunks (and every quadrant level of an adaptive chunk again): the same answers."""
    monkeypatch.setenv("XRT_PIXEL_BYTES", "200000")   # 1000 rays of one light
    try:
        scene, tracer = xrt.configs.build_product(grid.spec)
    finally:
        monkeypatch.delenv("XRT_PIXEL_BYTES")
    for ms, quality in modes(xrt):
        set_mode(xrt, tracer, ms, quality)
        rgba, rgbf = tracer.RenderPixels(scrambled, want_float=True)
        st = dict(tracer.last_stats)
        w_rgba, w_rgbf = grid.pixels(scrambled, ms, quality)
        assert np.array_equal(rgba, w_rgba) and np.array_equal(_bits(rgbf), _bits(w_rgbf)), (ms, quality)
        for k in ("rays_closest", "rays_shadow", "hits_closest", "shaded_hits", "pixels"):
            assert st[k] == grid.tracer.last_stats[k], k
        assert st["intersect_launches"] > grid.tracer.last_stats["intersect_launches"]   # it was split


def test_latest_poses(xrt):
    """xrt_scene_set_poses, then the list: the frame rendered after the same edit."""
    spec = xrt.configs.crate_grid_scene(W, H, n=5, grid=4)
    scene, tracer = xrt.configs.build_product(spec)
    c = px.grid_centers(W, H)[np.random.default_rng(9).permutation(W * H)[:2500]]
    at = c[:, 1].astype(np.int64) * W + c[:, 0].astype(np.int64)
    before = tracer.RenderPixels(c)
    for i in (5, 6, 9):
        ids, pos, rot, scale = spec.objects[i]
        scene.Bodies[i].Position = (pos[0] + 7.0, pos[1] + 11.0, pos[2] - 3.0)
        scene.Bodies[i].Rotation = (0.3, 0.2, 0.1)
    for ms, quality in modes(xrt):
        set_mode(xrt, tracer, ms, quality)
        rgba, rgbf = tracer.RenderPixels(c, want_float=True)   # (the mirror hands the moved bodies over first: xrt_scene_set_poses)
        f_rgba, f_rgbf = tracer.Render(want_float=True)
        assert np.array_equal(rgba, f_rgba[at]) and np.array_equal(_bits(rgbf), _bits(f_rgbf[at])), (ms, quality)
        if ms == xrt.abi.MS_OFF:
            assert (rgba != before).sum() > 20   # (the edit is seen; the scene octree is not rebuilt by a pose edit, so the frame after it is the yardstick)


def test_busy_rule(xrt, grid, scrambled):
    """With a begin/end ticket open the call is XRT_E_BUSY and the frame in flight is unchanged."""
    import torch
    set_mode(xrt, grid.tracer, xrt.abi.MS_OFF)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    pipe = grid.tracer.PrepareDevice(out.data_ptr())
    t = pipe.begin()
    with pytest.raises(RuntimeError, match="busy"):
        grid.tracer.RenderPixels(scrambled[:100])
    d_c = torch.from_numpy(scrambled[:100].copy()).to("cuda")
    with pytest.raises(RuntimeError, match="busy"):
        grid.tracer.RenderPixels(d_c, device=True)
    pipe.end(t)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), grid.oracle(xrt.abi.MS_OFF)[0])
    grid.check_integer(scrambled[:100], xrt.abi.MS_OFF, 0, "after the ticket")
