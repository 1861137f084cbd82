"""xrt_render_opts.list_order = XRT_LIST_COHERENT on the GPU: a list the caller calls coherent is traced as a frame of the same scene and sampling would
be -- xrt_render_pixels generates its rays where it compacts them (pixels.hip k_pixel_raygen) and, where launch #0 is a packet launch, writes the packet
table a frame's ray generation writes; xrt_cast_rays* only pick the frame's kernels.  The hint is scheduling only, so every assertion here is an equality:
with the frame, with the unhinted call, with the oracle -- for a row-major list, for the frame's tile order, and for a scrambled list, the wrong hint,
which must still be right.  Scenes and sizes are those of tests/test_gpu_pixels.py and tests/test_gpu_packet_quads.py: the small heightfield (one body:
packets for generation 0 with 16 samples alone), the crate grid (two-level: packets at any sample count), the crate, the glass scene (ray trees)."""
import ctypes as C

import numpy as np
import pytest

import pixels_py as px
from test_gpu_packet_quads import check_table, hf_spec
from test_gpu_pixels import BLACK, Case, _bits, set_mode

pytestmark = pytest.mark.gpu


def counters(stats):
    """Every member of xrt_stats but the timings."""
    return {k: v for k, v in stats.items() if not k.startswith("ms_")}


def tile_order(w, h):
    """The pixels of a w x h frame tile by tile (64 x 8 tiles, row by row; inside a tile row-major): (w h, 2) float32."""
    out = []
    for ty in range(0, h, 8):
        for tx in range(0, w, 64):
            y, x = np.mgrid[ty:min(ty + 8, h), tx:min(tx + 64, w)]
            out.append(np.stack([x.ravel(), y.ravel()], axis=1))
    return np.concatenate(out).astype(np.float32)


def all_modes(xrt):
    a = xrt.abi
    return [(a.MS_OFF, 0), (a.MS_FIXED16, 0), (a.MS_ADAPTIVE, 2)]


@pytest.fixture(scope="module")
def hf(xrt, orc):
    """The heightfield looked past, rolled: its far edge runs from corner to corner (tests/test_gpu_packet_quads.py), 96x64."""
    return Case(xrt, orc, hf_spec(xrt, (96, 64), xrt.abi.MS_OFF, "diagonal"))


@pytest.fixture(scope="module")
def hf_wide(xrt, orc):
    return Case(xrt, orc, hf_spec(xrt, (160, 96), xrt.abi.MS_OFF, "diagonal"))


@pytest.fixture(scope="module")
def grid(xrt, orc):
    return Case(xrt, orc, xrt.configs.crate_grid_scene(96, 54))


@pytest.fixture(scope="module")
def glass(xrt, orc):
    return Case(xrt, orc, xrt.configs.default_game_scene(32, 32, max_reflections=3))


def both(case, centers, ms, quality, collect=False):
    """The list unhinted and hinted: ((rgba, rgbf, counters), (rgba, rgbf, counters))."""
    out = []
    case.tracer.collect_stats = collect
    try:
        for coherent in (False, True):
            rgba, rgbf = case.pixels(centers, ms, quality, coherent=coherent)
            out.append((rgba, rgbf, counters(case.tracer.last_stats)))
    finally:
        case.tracer.collect_stats = False
    return out


def assert_same(plain, hinted, what):
    assert np.array_equal(hinted[0], plain[0]), (what, int((hinted[0] != plain[0]).sum()))
    assert np.array_equal(_bits(hinted[1]), _bits(plain[1])), what
    assert hinted[2] == plain[2], (what, {k: (plain[2][k], hinted[2][k]) for k in plain[2] if plain[2][k] != hinted[2][k]})


# ---- 1. equality ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("name", ["hf", "grid", "glass"])
def test_hinted_lists_are_the_frame_and_the_unhinted_list(xrt, request, name, which):
    case = request.getfixturevalue(name)
    ms, quality = all_modes(xrt)[which]
    w, h = case.spec.width, case.spec.height
    f_rgba, f_rgbf, _ = case.frame(ms, quality)
    rows = px.grid_centers(w, h)
    orders = {"row-major": rows, "tile order": tile_order(w, h), "scrambled": rows[np.random.default_rng(20261020).permutation(w * h)]}
    assert sorted(map(tuple, orders["tile order"].tolist())) == sorted(map(tuple, rows.tolist()))
    for what, c in orders.items():
        plain, hinted = both(case, c, ms, quality)
        assert_same(plain, hinted, (name, ms, what))
        at = c[:, 1].astype(np.int64) * w + c[:, 0].astype(np.int64)
        assert np.array_equal(hinted[0], f_rgba[at]) and np.array_equal(_bits(hinted[1]), _bits(f_rgbf[at])), (name, ms, what, "the frame")
    assert len(np.unique(f_rgba)) > 10
    # ... and with the counting pass: the reference's work counters too
    plain, hinted = both(case, rows, ms, quality, collect=True)
    assert_same(plain, hinted, (name, ms, "counted"))
    assert hinted[2]["node_tests"] > 0 and hinted[2]["tri_tests"] > 0


# ---- 2. sizes at the kernel's seams ---------------------------------------------------------------------------------------------------------
def edge_window(case, ms, quality, n):
    """n consecutive row-major centres around the first place where the oracle's frame goes from black to lit or back (as far as the frame's end allows)."""
    lit = case.oracle(ms, quality)[0] != BLACK
    flips = np.nonzero(lit[:-1] != lit[1:])[0]
    assert len(flips) > 0
    k0 = max(0, min(int(flips[0]) - n // 2, len(lit) - n))
    assert k0 <= flips[0] < k0 + max(n, 2)
    return px.grid_centers(case.spec.width, case.spec.height)[k0:k0 + n]


def check_seam(case, c, ms, quality, what):
    o_rgba, o_rgbf, _ = case.oracle(ms, quality)
    at = c[:, 1].astype(np.int64) * case.spec.width + c[:, 0].astype(np.int64)
    plain, hinted = both(case, c, ms, quality)
    assert_same(plain, hinted, what)
    assert np.array_equal(hinted[0], o_rgba[at]) and np.array_equal(_bits(hinted[1]), _bits(o_rgbf[at])), (what, "the oracle")
    assert hinted[2]["pixels"] == len(c)


@pytest.mark.parametrize("name", ["hf", "grid"])
def test_list_lengths_at_the_seams(xrt, request, name):
    """A wave's cell is 64 places and a group of a block 4 x 1024: one sample n = 1 .. 4097, 16 samples n = 1 .. 257, level-0 quadrants n = 15 .. 17."""
    case = request.getfixturevalue(name)
    a = xrt.abi
    for ms, quality, ns in ((a.MS_OFF, 0, (1, 63, 64, 65, 4095, 4096, 4097)), (a.MS_FIXED16, 0, (1, 3, 4, 5, 255, 256, 257)), (a.MS_ADAPTIVE, 2, (15, 16, 17))):
        for n in ns:
            window = edge_window(case, ms, quality, n)
            assert len(window) == n
            check_seam(case, window, ms, quality, (name, ms, n))


# ---- 3. the table -----------------------------------------------------------------------------------------------------------------------------
def test_table_structure(xrt, hf_wide):
    """A hinted 16-sample row-major list of the one-body scene: launch #0 is a packet launch and takes its packets from the table k_pixel_raygen wrote."""
    a = xrt.abi
    case = hf_wide
    w, h = case.spec.width, case.spec.height
    c = px.grid_centers(w, h)
    # the premise, on the CPU: units (4 consecutive entries of 16 samples) that are all sky, units that are all terrain, units on the edge
    lit = (case.oracle(a.MS_FIXED16)[0] != BLACK).reshape(-1, 4)
    per_unit = lit.sum(axis=1)
    assert (per_unit == 0).sum() > 100 and (per_unit == 4).sum() > 100 and ((per_unit > 0) & (per_unit < 4)).sum() > 20
    rgba, _ = case.pixels(c, a.MS_FIXED16, coherent=True)
    assert np.array_equal(rgba, case.oracle(a.MS_FIXED16)[0])
    entries, places = case.scene.PacketTable()
    n_entries, partial = check_table(entries, places, "hinted 16-sample list")   # disjoint, cover 0 .. live-1, 1 .. 64 rays, one aligned unit each, no unit twice
    live = places.shape[0]
    units = (w * h * 16 + 63) // 64
    full = int((entries[:, 1] == 64).sum())
    print("table of the hinted list: live", live, "entries", n_entries, "of", units, "units; full", full, "partly live", partial)
    assert full > 100 and partial > 20 and n_entries < units - 100   # full units, partly live ones, and all-sky ones that have no entry
    assert places.min() >= 0 and places.max() < w * h * 16 and np.unique(places).shape[0] == live
    # a lit pixel has live rays: every unit the oracle sees terrain in has its entry
    assert set(np.nonzero(per_unit > 0)[0].tolist()) <= set((places.astype(np.int64) >> 6).tolist())
    # the frame's table covers the same live rays (its walk is in tile order, its units are 2x2 quads)
    # counts[1] is the live rays: the frame of the same camera has as many (its cull rectangle only leaves out rays that cannot reach the root box)
    set_mode(xrt, case.tracer, a.MS_FIXED16)
    case.tracer.Render()
    f_entries, f_paths = case.scene.PacketTable()
    assert f_entries.shape[0] > 0 and f_paths.shape[0] == live
    # the same call unhinted: no table
    case.pixels(c, a.MS_FIXED16)
    entries0, places0 = case.scene.PacketTable()
    assert entries0.shape[0] == 0 and places0.shape[0] == 0


def test_table_of_a_two_level_scene_at_one_sample(xrt, grid):
    """Two-level scenes take packets at any sample count: the unit is 64 one-sample entries, 16 level-0 quadrants."""
    a = xrt.abi
    c = px.grid_centers(96, 54)
    for ms, quality in ((a.MS_OFF, 0), (a.MS_ADAPTIVE, 0)):
        rgba, _ = grid.pixels(c, ms, quality, coherent=True)
        assert np.array_equal(rgba, grid.oracle(ms, quality)[0])
        entries, places = grid.scene.PacketTable()
        check_table(entries, places, ("grid", ms))
        assert places.max() < 96 * 54 * (4 if ms else 1)
    # unhinted: generation 0 goes to the per-lane kernel, no table
    grid.pixels(c, a.MS_OFF)
    assert grid.scene.PacketTable()[0].shape[0] == 0


def test_one_body_scene_at_one_sample_takes_no_table(xrt, hf):
    """One-body scenes follow the frame's rule: packets for generation 0 with 16 samples alone.  The rays are generated by the fused kernel all the same."""
    c = px.grid_centers(96, 64)
    rgba, _ = hf.pixels(c, xrt.abi.MS_OFF, coherent=True)
    assert np.array_equal(rgba, hf.oracle(xrt.abi.MS_OFF)[0])
    assert hf.scene.PacketTable()[0].shape[0] == 0


# ---- 4. chunks --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hf", "grid"])
def test_the_split_changes_nothing(xrt, monkeypatch, request, name):
    """A byte budget that cuts the list into many chunks (the bounds are multiples of 4 entries: one-sample units restart per chunk)."""
    case = request.getfixturevalue(name)
    w, h = case.spec.width, case.spec.height
    with monkeypatch.context() as m:
        m.setenv("XRT_PIXEL_BYTES", "200000")   # 1000 rays of one light
        scene, tracer = xrt.configs.build_product(case.spec)
    c = px.grid_centers(w, h)
    for ms, quality in all_modes(xrt):
        set_mode(xrt, tracer, ms, quality)
        rgba, rgbf = tracer.RenderPixels(c, want_float=True, coherent=True)
        st = dict(tracer.last_stats)
        w_rgba, w_rgbf = case.pixels(c, ms, quality, coherent=True)
        assert np.array_equal(rgba, w_rgba) and np.array_equal(_bits(rgbf), _bits(w_rgbf)), (name, ms)
        assert np.array_equal(rgba, case.oracle(ms, quality)[0]), (name, ms)
        for k in ("rays_closest", "rays_shadow", "hits_closest", "shaded_hits", "pixels", "rays_traversed"):
            assert st[k] == case.tracer.last_stats[k], k
        assert st["intersect_launches"] >= 3 * case.tracer.last_stats["intersect_launches"]   # at least three chunks


# ---- 5. xrt_cast_rays ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "glass"])
def test_cast_rays_hinted(xrt, request, name):
    """The frame's primary rays in screen order, hinted and not: colours, vertices, vertex_start, rays_back, launches and traversed rays."""
    import torch
    case = request.getfixturevalue(name)
    set_mode(xrt, case.tracer, xrt.abi.MS_OFF)
    rays = case.tracer.GeneratePrimaryRays()
    f_rgba, f_rgbf, _ = case.frame(xrt.abi.MS_OFF)
    seen = []
    for coherent in (False, True):
        rgba, rgbf = case.tracer.CastRays(rays, want_float=True, coherent=coherent)
        st = counters(case.tracer.last_stats)
        p_rgba, p_rgbf, verts, vstart, back = case.tracer.CastRays(rays, want_float=True, paths=True, coherent=coherent)
        assert np.array_equal(p_rgba, rgba) and np.array_equal(_bits(p_rgbf), _bits(rgbf))
        d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda")
        d_rgba, d_rgbf = case.tracer.CastRays(d_rays, want_float=True, device=True, coherent=coherent)
        torch.cuda.synchronize()
        assert np.array_equal(d_rgba.cpu().numpy().view(np.uint32), rgba) and np.array_equal(_bits(d_rgbf.cpu().numpy()), _bits(rgbf))
        assert counters(case.tracer.last_stats) == st
        seen.append((rgba, rgbf, st, verts.tobytes(), vstart.copy(), back.tobytes()))
    plain, hinted = seen
    assert np.array_equal(hinted[0], f_rgba) and np.array_equal(_bits(hinted[1]), _bits(f_rgbf))   # (CastRay on the frame's rays is the frame)
    assert_same(plain[:3], hinted[:3], name)
    assert hinted[2]["intersect_launches"] == plain[2]["intersect_launches"] and hinted[2]["rays_traversed"] == plain[2]["rays_traversed"] > 0
    assert hinted[3] == plain[3] and np.array_equal(hinted[4], plain[4]) and hinted[5] == plain[5]
    assert plain[4][-1] > 0 and len(plain[3]) == 16 * plain[4][-1]
    assert case.scene.PacketTable()[0].shape[0] == 0   # a batch of rays: a packet is 64 consecutive live slots, no table


# ---- 6. the device form, and who reads the field -------------------------------------------------------------------------------------------------
def with_list_order(tracer, value):
    """The tracer's options with list_order = value, for the calls of the mirror that have no keyword for it."""
    orig = tracer._opts_abi

    def opts(*a, **kw):
        o = orig(*a, **kw)
        o.list_order = value
        return o
    tracer._opts_abi = opts
    return orig


def test_device_form_and_the_other_calls(xrt, grid):
    import torch
    a, lib = xrt.abi, xrt.abi.lib()
    c = px.grid_centers(96, 54)
    bad = c.copy()
    mid = len(c) // 2 + 7
    bad[mid] = (np.nan, np.inf)
    for ms, quality in all_modes(xrt):
        h_rgba, h_rgbf = grid.pixels(c, ms, quality)
        set_mode(xrt, grid.tracer, ms, quality)
        d_rgba, d_rgbf = grid.tracer.RenderPixels(torch.from_numpy(bad).to("cuda"), want_float=True, device=True, coherent=True)
        torch.cuda.synchronize()
        got, gotf = d_rgba.cpu().numpy().view(np.uint32), d_rgbf.cpu().numpy()
        keep = np.arange(len(c)) != mid
        assert np.array_equal(got[keep], h_rgba[keep]) and np.array_equal(_bits(gotf[keep]), _bits(h_rgbf[keep])), (ms, "a non-finite centre moved its neighbours")
    # list_order = 2 is an argument error wherever the field is read
    set_mode(xrt, grid.tracer, a.MS_OFF)
    rays = grid.tracer.GeneratePrimaryRays()[:256]
    orig = with_list_order(grid.tracer, 2)
    try:
        for call in (lambda: grid.tracer.RenderPixels(c[:64], coherent=2), lambda: grid.tracer.RenderPixels(torch.from_numpy(c[:64].copy()).to("cuda"), device=True, coherent=2),
                     lambda: grid.tracer.CastRays(rays, coherent=2), lambda: grid.tracer.CastRays(rays, paths=True, coherent=2),
                     lambda: grid.tracer.CastRays(torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda"), device=True, coherent=2),
                     lambda: grid.tracer.ShadeHits(rays, grid.scene.IntersectBatch(rays))):
            with pytest.raises(ValueError, match="list_order"):   # (XRT_E_INVALID_ARG: the mirror's ArgumentException)
                call()
        # ... and nowhere else: a frame with garbage in the field is the frame
        f_rgba, f_rgbf, f_st = grid.frame(a.MS_OFF)
        for junk in (1, 2, -7):
            grid.tracer._opts_abi = orig
            with_list_order(grid.tracer, junk)
            rgba, rgbf = grid.tracer.Render(want_float=True)
            assert np.array_equal(rgba, f_rgba) and np.array_equal(_bits(rgbf), _bits(f_rgbf)), junk
            assert counters(grid.tracer.last_stats) == counters(f_st), junk
    finally:
        grid.tracer._opts_abi = orig
    # xrt_shade_hits accepts the hint and does nothing with it
    hits = grid.scene.IntersectBatch(rays)
    plain = grid.tracer.ShadeHits(rays, hits, want_float=True)
    st = counters(grid.tracer.last_stats)
    orig = with_list_order(grid.tracer, a.LIST_COHERENT)
    try:
        hinted = grid.tracer.ShadeHits(rays, hits, want_float=True)
        assert counters(grid.tracer.last_stats) == st
    finally:
        grid.tracer._opts_abi = orig
    assert np.array_equal(hinted[0], plain[0]) and np.array_equal(_bits(hinted[1]), _bits(plain[1]))
    assert lib.xrt_version() == 203


# ---- 7. guards ----------------------------------------------------------------------------------------------------------------------------------
def test_under_guards(xrt, monkeypatch, hf_wide):
    """XRT_GUARD=1 (csrc/device_res.h): the table and the live list are device buffers like any other, a write past one fails the call."""
    a = xrt.abi
    monkeypatch.setenv("XRT_GUARD", "1")
    try:
        scene, tracer = xrt.configs.build_product(hf_wide.spec)
        set_mode(xrt, tracer, a.MS_FIXED16)
        c = px.grid_centers(hf_wide.spec.width, hf_wide.spec.height)
        for rep in range(2):   # (the second call runs on the table's other count word)
            rgba = tracer.RenderPixels(c, coherent=True)
            assert np.array_equal(rgba, hf_wide.oracle(a.MS_FIXED16)[0]), rep
            assert scene.PacketTable()[0].shape[0] > 0
        assert np.array_equal(tracer.RenderPixels(c[:1000], coherent=True), hf_wide.oracle(a.MS_FIXED16)[0][:1000])
    finally:
        monkeypatch.delenv("XRT_GUARD")
        xrt.configs.build_product(xrt.configs.crate_scene(32, 32, 0))   # (xrt_scene_create reads the switch)
