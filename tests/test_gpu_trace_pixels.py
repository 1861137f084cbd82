"""xrt_trace_pixels on the GPU: the primary ray (RT:412-421) and its closest hit (RT:512) for caller-chosen screen positions, nothing shaded.  Every
comparison is an equality on bits; hits are compared field by field without `reserved` (scheduling feedback).  The expectations are the oracle's
(tests/trace_py.py says how an oracle frame pins the ray of any centre, tests/test_trace_pixels_cpu.py shows on the CPU that it does and that the lists
used here contain what they must), the library's own seam 1 (xrt_scene_intersect on the returned rays), and its own xrt_render_pixels through
xrt_shade_hits.  Scenes and sizes are those of tests/test_gpu_coherent.py: the heightfield 96x64 "diagonal" (one body: per-lane at one sample, packets
with sixteen), the crate grid 96x54 (two-level: packets at any sample count), the crate, the glass scene 32x32 at MaxReflections 3."""
import copy
import ctypes as C

import numpy as np
import pytest

import pixels_py as px
import trace_py as tp
from test_gpu_coherent import counters, edge_window, tile_order
from test_gpu_packet_quads import check_table, hf_spec
from test_gpu_pixels import Case, _bits, set_mode

pytestmark = pytest.mark.gpu


class TraceCase(Case):
    """A scene on the GPU and in the oracle, and the oracle's rays and hits of its whole frame by mode, each made once and never written again."""

    def __init__(self, xrt, orc, spec):
        super().__init__(xrt, orc, spec)
        self._expected = {}
        self.centers = px.grid_centers(spec.width, spec.height)

    def expected(self, fixed16):
        """(rays, hits) of the row-major frame: record p * samples + s is sample s of pixel p."""
        if fixed16 not in self._expected:
            rays = tp.oracle_rays(self.orc, self.spec, tp.sample_centers(self.centers, fixed16))
            hits = self.osc.intersect(rays)
            rays.setflags(write=False)
            hits.setflags(write=False)
            self._expected[fixed16] = (rays, hits)
        return self._expected[fixed16]

    def expected_at(self, pixels, fixed16):
        """... of the listed pixels (indices into the row-major frame)."""
        rays, hits = self.expected(fixed16)
        s = 16 if fixed16 else 1
        at = (np.asarray(pixels, dtype=np.int64)[:, None] * s + np.arange(s)[None, :]).ravel()
        return rays[at], hits[at]

    def trace(self, centers, **kw):
        out = self.tracer.TracePixels(np.asarray(centers, dtype=np.float32), **kw)
        return out, counters(self.tracer.last_stats)

    def both(self, centers, fixed16, collect=False):
        """The list unhinted and hinted: [((rays, hits), counters), ((rays, hits), counters)]."""
        self.tracer.collect_stats = collect
        try:
            return [self.trace(centers, fixed16=fixed16, coherent=coherent) for coherent in (False, True)]
        finally:
            self.tracer.collect_stats = False

    def check(self, pixels, fixed16, what, collect=False):
        """The listed pixels unhinted and hinted against the oracle, against seam 1 on the returned rays, and against each other, counters included."""
        pixels = np.asarray(pixels, dtype=np.int64)
        e_rays, e_hits = self.expected_at(pixels, fixed16)
        (plain, p_st), (hinted, h_st) = self.both(self.centers[pixels], fixed16, collect)
        for name, (rays, hits) in (("unhinted", plain), ("hinted", hinted)):
            assert tp.same_rays(rays, e_rays), (what, name, "rays differ from the oracle's")
            assert tp.hit_diff(hits, e_hits) == {}, (what, name, "hits differ from the oracle's", tp.hit_diff(hits, e_hits))
            assert tp.is_miss_record(hits[hits["hit"] == 0]).all(), (what, name)
        seam1 = self.scene.IntersectBatch(hinted[0])
        assert tp.hit_diff(hinted[1], seam1) == {}, (what, "xrt_scene_intersect on the returned rays", tp.hit_diff(hinted[1], seam1))
        n, s = len(pixels), 16 if fixed16 else 1
        live = h_st.pop("rays_traversed")
        assert p_st.pop("rays_traversed") == n * s >= live
        assert h_st == p_st, (what, {k: (p_st[k], h_st[k]) for k in p_st if p_st[k] != h_st[k]})
        assert h_st["pixels"] == n and h_st["rays_closest"] == n * s and h_st["hits_closest"] == int((e_hits["hit"] != 0).sum())
        assert h_st["rays_shadow"] == 0 and h_st["shaded_hits"] == 0 and h_st["intersect_launches"] == 1
        return hinted, live, h_st


def specs(xrt):
    return {"hf": hf_spec(xrt, (96, 64), xrt.abi.MS_OFF, "diagonal"), "grid": xrt.configs.crate_grid_scene(96, 54),
            "crate": xrt.configs.crate_scene(96, 54, max_reflections=2), "glass": xrt.configs.default_game_scene(32, 32, max_reflections=3)}


@pytest.fixture(scope="module")
def cases(xrt, orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = TraceCase(xrt, orc, specs(xrt)[name])
        return made[name]
    return get


# ---- 1. parity with the oracle and with seam 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed16", [False, True])
@pytest.mark.parametrize("name", ["hf", "grid", "crate", "glass"])
def test_parity_in_every_order(cases, name, fixed16):
    case = cases(name)
    w, h = case.spec.width, case.spec.height
    rows = np.arange(w * h)
    t = tile_order(w, h)
    orders = {"row-major": rows, "tile order": t[:, 1].astype(np.int64) * w + t[:, 0].astype(np.int64), "scrambled": np.random.default_rng(20261020).permutation(w * h)}
    assert sorted(orders["tile order"].tolist()) == rows.tolist()
    lives = []
    for what, pixels in orders.items():
        _, live, _ = case.check(pixels, fixed16, (name, fixed16, what))
        lives.append(live)
    assert lives[0] == lives[1] == lives[2] < w * h * (16 if fixed16 else 1), "the order of a list does not change which rays reach the root box"
    assert lives[0] >= int((case.expected(fixed16)[1]["hit"] != 0).sum())
    # ... and with the counting pass: the reference's work counters too (check() compares every counter of the two calls)
    _, _, st = case.check(rows, fixed16, (name, fixed16, "counted"), collect=True)
    assert st["node_tests"] > 0 and st["tri_tests"] > 0 and st["algorithmic_bytes"] > 0
    _, o_st = case.osc.intersect(case.expected(fixed16)[0], stats=True)
    for k in ("rays_closest", "hits_closest", "scene_node_tests", "instance_visits", "mesh_aabb_tests", "mesh_queries", "node_tests", "leaf_refs", "tri_tests"):
        assert st[k] == o_st[k], (k, st[k], o_st[k])


# ---- 2. the seams of the new kernel --------------------------------------------------------------------------------------------------------------
def window(case, n):
    """n consecutive row-major pixels around the first lit / black flip of the oracle's one-sample frame (tests/test_gpu_coherent.py edge_window), the
    same flip whatever the sampling; a list longer than the frame goes round it (duplicates are legal)."""
    total = case.spec.width * case.spec.height
    first = edge_window(case, case.xrt.abi.MS_OFF, 0, min(n, total))[0]
    k0 = int(first[1]) * case.spec.width + int(first[0])
    return (k0 + np.arange(n)) % total


@pytest.mark.parametrize("name", ["hf", "grid"])
def test_list_lengths_at_the_seams(cases, name):
    """A wave's cell is 64 places and a group of a block 4 x 1024: one sample n = 1 .. 6144, sixteen samples n = 3 .. 257."""
    case = cases(name)
    for fixed16, ns in ((False, (1, 63, 64, 65, 4095, 4096, 4097, 6144)), (True, (3, 4, 5, 255, 256, 257))):
        for n in ns:
            pixels = window(case, n)
            assert len(pixels) == n
            hinted, live, _ = case.check(pixels, fixed16, (name, fixed16, n))
            if n >= 63:
                hit = hinted[1]["hit"] != 0
                assert hit.any() and not hit.all(), (name, fixed16, n, "the window lies on an edge")


def test_all_miss_and_all_live_lists(xrt, orc, cases):
    """The camera turned away: every record is the miss record and a hinted call hands nothing to a traversal kernel.  Pixels that see the terrain: every
    ray is live."""
    spec = copy.deepcopy(specs(xrt)["hf"])
    cam = dict(spec.camera)
    cam["target"] = tuple(2 * p - t for p, t in zip(cam["pos"], cam["target"]))
    spec.camera = cam
    away = TraceCase(xrt, orc, spec)
    for fixed16 in (False, True):
        pixels = np.arange(96 * 64) if not fixed16 else np.arange(300)
        hinted, live, st = away.check(pixels, fixed16, ("away", fixed16))
        assert tp.is_miss_record(hinted[1]).all() and live == 0 and st["hits_closest"] == 0
    case = cases("hf")
    for fixed16 in (False, True):
        lit = np.nonzero((case.expected(fixed16)[1]["hit"] != 0).reshape(96 * 64, -1).all(axis=1))[0]
        assert len(lit) > 300
        pixels = np.resize(lit, 4200) if not fixed16 else lit[:270]   # (past a group of 4096 places in both modes; the one-sample list repeats its pixels)
        hinted, live, st = case.check(pixels, fixed16, ("all live", fixed16))
        assert live == len(hinted[0]) == st["hits_closest"]


# ---- 3. the table, and the rule that picks the kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fixed16", [("grid", False), ("hf", True)])
def test_packet_table(cases, name, fixed16):
    """One chunk, packets picked: the entries tile the live rays without gap or overlap, each within one aligned 64-place unit (check_table)."""
    case = cases(name)
    w, h = case.spec.width, case.spec.height
    s = 16 if fixed16 else 1
    (_, hits), st = case.trace(case.centers, fixed16=fixed16, coherent=True)
    entries, places = case.scene.PacketTable()
    n_entries, partial = check_table(entries, places, (name, fixed16))
    assert places.shape[0] == st["rays_traversed"] and places.min() >= 0 and places.max() < w * h * s and np.unique(places).shape[0] == places.shape[0]
    units = (w * h * s + 63) // 64
    assert partial > 5 and n_entries <= units
    # a hit ray is a live ray: every unit with a hit has its entry
    hit_units = set((np.nonzero(hits["hit"] != 0)[0] >> 6).tolist())
    assert hit_units <= set((places.astype(np.int64) >> 6).tolist())
    # the same call unhinted, or without hits: no table
    case.trace(case.centers, fixed16=fixed16)
    assert case.scene.PacketTable()[0].shape[0] == 0
    case.trace(case.centers, fixed16=fixed16, coherent=True)
    assert case.scene.PacketTable()[0].shape[0] == n_entries
    case.trace(case.centers, fixed16=fixed16, coherent=True, want_hits=False)
    assert case.scene.PacketTable()[0].shape[0] == 0


def test_one_body_scene_at_one_sample_is_traced_per_lane(cases):
    """The frame's rule: a one-body scene takes packets for generation 0 with sixteen samples alone."""
    case = cases("hf")
    case.trace(case.centers, coherent=True)
    entries, places = case.scene.PacketTable()
    assert entries.shape[0] == 0 and places.shape[0] == 0


# ---- 4. composition --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hf", "grid", "crate", "glass"])
def test_shade_hits_on_traced_pixels_is_render_pixels(xrt, orc, cases, name):
    case = cases(name)
    a = xrt.abi
    c = case.centers
    for coherent in (False, True):
        (rays, hits), _ = case.trace(c, coherent=coherent)
        set_mode(xrt, case.tracer, a.MS_OFF)
        rgba, rgbf = case.tracer.ShadeHits(rays, hits, want_float=True)
        p_rgba, p_rgbf = case.pixels(c, a.MS_OFF)
        assert np.array_equal(rgba, p_rgba) and np.array_equal(_bits(rgbf), _bits(p_rgbf)), (name, coherent)
        assert len(np.unique(rgba)) > 10
    # the fixed sixteen, folded by the RT:309 mean of means, on pixels around the first edge
    pixels = window(case, 160)
    (rays, hits), _ = case.trace(c[pixels], fixed16=True, coherent=True)
    set_mode(xrt, case.tracer, a.MS_OFF)
    s_rgba = case.tracer.ShadeHits(rays, hits)
    p16, _ = case.pixels(c[pixels], a.MS_FIXED16)
    folded = np.array([px.mean16(orc, s_rgba[16 * i:16 * i + 16]) for i in range(len(pixels))], dtype=np.uint32)
    assert np.array_equal(folded, p16), (name, int((folded != p16).sum()))
    assert sum(len(set(s_rgba[16 * i:16 * i + 16].tolist())) > 1 for i in range(len(pixels))) >= 2   # (pixels whose samples differ: the window lies on an edge)
    # CastRay's light loop on these hits is the light loop on seam 1's
    (rays, hits), _ = case.trace(c, coherent=True)
    l1, a1 = case.tracer.LightHits(hits, want_amounts=True)
    l2, a2 = case.tracer.LightHits(case.scene.IntersectBatch(rays), want_amounts=True)
    assert np.array_equal(_bits(l1), _bits(l2)) and np.array_equal(_bits(a1), _bits(a2)) and l1.any()


# ---- 5. outputs alone; fractional, outside and repeated centres --------------------------------------------------------------------------------------
def test_either_output_alone(cases):
    case = cases("grid")
    for fixed16 in (False, True):
        pixels = window(case, 700)
        c = case.centers[pixels]
        for coherent in (False, True):
            (rays, hits), _ = case.trace(c, fixed16=fixed16, coherent=coherent)
            only_rays, st = case.trace(c, fixed16=fixed16, coherent=coherent, want_hits=False)
            assert tp.same_rays(only_rays, rays)
            assert st["intersect_launches"] == 0 and st["rays_closest"] == 0 and st["rays_traversed"] == 0 and st["hits_closest"] == 0 and st["pixels"] == 700
            only_hits, st = case.trace(c, fixed16=fixed16, coherent=coherent, want_rays=False)
            assert tp.hit_diff(only_hits, hits) == {} and st["intersect_launches"] == 1
            case.tracer.collect_stats = True
            try:
                counted, st2 = case.trace(c, fixed16=fixed16, coherent=coherent, want_rays=False)
            finally:
                case.tracer.collect_stats = False
            assert tp.hit_diff(counted, hits) == {} and st2["tri_tests"] > 0


def test_fractional_outside_and_repeated_centres(xrt, orc):
    """A close-up of the crate, so that centres outside the viewport still see it: the oracle's rays and hits (tests/trace_py.py)."""
    spec = xrt.configs.crate_scene(32, 18, max_reflections=1)
    spec.camera = xrt.configs.camera((0, 8, 14), (0, 8, 0))
    case = TraceCase(xrt, orc, spec)
    f = np.float32
    c = np.array([(-3, -2), (32 + 5, 18 + 1), (-0.5, 18.25), (15.125, 9.875), (15.125, 9.875), (0.0625, 17.5), (31.9375, 0.25), (-400, 7), (16, -300), (16, 9), (16, 9)], dtype=f)
    for fixed16 in (False, True):
        e_rays = tp.oracle_rays(orc, spec, tp.sample_centers(c if not fixed16 else np.floor(c * 2) / 2, fixed16))
        e_hits = case.osc.intersect(e_rays)
        assert 0 < (e_hits["hit"] != 0).sum() < len(e_hits)
        for coherent in (False, True):
            (rays, hits), st = case.trace(c if not fixed16 else np.floor(c * 2) / 2, fixed16=fixed16, coherent=coherent)
            assert tp.same_rays(rays, e_rays), (fixed16, coherent)
            assert tp.hit_diff(hits, e_hits) == {}, (fixed16, coherent, tp.hit_diff(hits, e_hits))
            assert st["pixels"] == len(c)
    (rays, hits), _ = case.trace(c)
    assert rays[3].tobytes() == rays[4].tobytes() and tp.hit_diff(hits[3:4], hits[4:5]) == {} and hits["hit"][9] == hits["hit"][10] == 1


# ---- 6. chunks, the device form, poses, the busy rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hf", "grid"])
def test_the_split_changes_nothing(xrt, monkeypatch, cases, name):
    """A byte budget that cuts the list into many chunks (36 bytes a place: 1000 places unhinted, fewer with the table)."""
    case = cases(name)
    with monkeypatch.context() as m:
        m.setenv("XRT_PIXEL_BYTES", "36000")
        scene, tracer = xrt.configs.build_product(case.spec)
    for fixed16 in (False, True):
        pixels = np.arange(96 * 54) if not fixed16 else window(case, 500)
        c = case.centers[pixels]
        for coherent in (False, True):
            (w_rays, w_hits), w_st = case.trace(c, fixed16=fixed16, coherent=coherent)
            rays, hits = tracer.TracePixels(c, fixed16=fixed16, coherent=coherent)
            st = counters(tracer.last_stats)
            assert tp.same_rays(rays, w_rays) and tp.hit_diff(hits, w_hits) == {}, (name, fixed16, coherent)
            assert st.pop("intersect_launches") >= 5 * w_st.pop("intersect_launches") == 5
            assert st == w_st, (name, fixed16, coherent)
            assert scene.PacketTable()[0].shape[0] == 0   # (more than one chunk: nothing to report)


def test_device_form_and_guard_words(xrt, cases):
    """Torch tensors on a stream of their own: the host form's records, and nothing at or behind n * samples records."""
    import torch
    case = cases("grid")
    a, lib = xrt.abi, xrt.abi.lib()
    s = torch.cuda.Stream()
    for fixed16 in (False, True):
        pixels = window(case, 1000 if not fixed16 else 130)
        c = case.centers[pixels]
        n, k = len(c), 16 if fixed16 else 1
        for coherent in (False, True):
            (h_rays, h_hits), h_st = case.trace(c, fixed16=fixed16, coherent=coherent)
            with torch.cuda.stream(s):
                d_c = torch.from_numpy(c.copy()).to("cuda")
                d_rays, d_hits = case.tracer.TracePixels(d_c, fixed16=fixed16, device=True, stream=s, coherent=coherent)
            s.synchronize()
            assert counters(case.tracer.last_stats) == h_st
            assert d_rays.shape == (n * k, 8) and d_hits.shape == (n * k, 12) and d_rays.dtype == torch.int32
            assert tp.same_rays(d_rays.cpu().numpy().view(xrt.api.RAY_DTYPE).reshape(-1), h_rays)
            assert tp.hit_diff(d_hits.cpu().numpy().view(xrt.api.HIT_DTYPE).reshape(-1), h_hits) == {}
            # guard words behind both outputs
            cam, opts = case.tracer._camera_abi(), case.tracer._opts_abi(shard_count=0)
            opts.n_gpus, opts.use_multisampling, opts.list_order = 0, a.MS_FIXED16 if fixed16 else a.MS_OFF, int(coherent)
            g_rays = torch.full((n * k * 8 + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            g_hits = torch.full((n * k * 12 + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            rc = lib.xrt_trace_pixels_device(case.scene.handle, C.byref(cam), C.byref(opts), C.c_void_p(d_c.data_ptr()), n, C.c_void_p(g_rays.data_ptr()),
                                             C.c_void_p(g_hits.data_ptr()), None, None)
            assert rc == a.XRT_OK
            assert (g_rays[n * k * 8:] == 0x5A5A5A5A).all() and (g_hits[n * k * 12:] == 0x5A5A5A5A).all()
            assert torch.equal(g_rays[:n * k * 8].reshape(-1, 8), d_rays)
            assert tp.hit_diff(g_hits[:n * k * 12].cpu().numpy().view(xrt.api.HIT_DTYPE).reshape(-1), h_hits) == {}
    raw = torch.zeros(2 * 64 + 4, dtype=torch.float32, device="cuda")
    out = torch.zeros(64 * 12 + 4, dtype=torch.int32, device="cuda")
    cam, opts = case.tracer._camera_abi(), case.tracer._opts_abi(shard_count=0)
    opts.n_gpus, opts.use_multisampling = 0, a.MS_OFF
    for dc, do in ((4, 0), (0, 4)):
        assert lib.xrt_trace_pixels_device(case.scene.handle, C.byref(cam), C.byref(opts), C.c_void_p(raw.data_ptr() + dc), 64, None,
                                           C.c_void_p(out.data_ptr() + do), None, None) == a.XRT_E_INVALID_ARG


def test_latest_poses(xrt):
    """xrt_scene_set_poses, then the list: the hits follow the moved bodies, as seam 1's do."""
    spec = xrt.configs.crate_grid_scene(96, 54, n=5, grid=4)
    scene, tracer = xrt.configs.build_product(spec)
    c = px.grid_centers(96, 54)
    before = [tracer.TracePixels(c, coherent=coherent)[1] for coherent in (False, True)]
    assert tp.hit_diff(before[0], before[1]) == {}
    for i in (5, 6, 9):
        ids, pos, rot, scale = spec.objects[i]
        scene.Bodies[i].Position = (pos[0] + 7.0, pos[1] + 11.0, pos[2] - 3.0)
        scene.Bodies[i].Rotation = (0.3, 0.2, 0.1)
    for fixed16 in (False, True):
        cc = c if not fixed16 else c[2000:2600]
        for coherent in (False, True):
            rays, hits = tracer.TracePixels(cc, fixed16=fixed16, coherent=coherent)   # (the mirror hands the moved bodies over first: xrt_scene_set_poses)
            assert tp.hit_diff(hits, scene.IntersectBatch(rays)) == {}, (fixed16, coherent)
            if not fixed16:
                assert len(tp.hit_diff(hits, before[0])) > 0 and (hits["w"] != before[0]["w"]).any(axis=1).sum() > 20   # (the edit is seen)


def test_busy_rule(xrt, cases):
    """With a begin/end ticket open the call is XRT_E_BUSY and the frame in flight is unchanged."""
    import torch
    case = cases("grid")
    set_mode(xrt, case.tracer, xrt.abi.MS_OFF)
    out = torch.zeros(96 * 54, dtype=torch.int32, device="cuda")
    pipe = case.tracer.PrepareDevice(out.data_ptr())
    t = pipe.begin()
    with pytest.raises(RuntimeError, match="busy"):
        case.tracer.TracePixels(case.centers[:100])
    d_c = torch.from_numpy(case.centers[:100].copy()).to("cuda")
    with pytest.raises(RuntimeError, match="busy"):
        case.tracer.TracePixels(d_c, device=True, coherent=True)
    pipe.end(t)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), case.oracle(xrt.abi.MS_OFF)[0])
    case.check(np.arange(100), False, "after the ticket")
