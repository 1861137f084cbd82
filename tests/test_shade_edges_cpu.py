"""k_shade's per-hit arithmetic at its numeric edges, on the CPU: the tables of tests/shade_edges.py through the oracle's CastRay (tests/castray,
tests/paths).  Two jobs.  (1) The oracle is pinned by answers that do not come from it: float64 restatements, written from the text of the
reference's Material.cs, SpotLight.cs, DirectionalLight.cs and RayTracer.cs, applied only to the probes whose answer is unambiguous in float64 (a UV
1e-3 of a texel away from every boundary, a fragment clearly inside or outside the cone, a colour away from a half); on the boundary probes
themselves the oracle is the reference.  (2) The population conditions: every probe ray hits, the texture probes reach every texel and tell the
address modes apart, every sweep has both of its sides.  tests/test_gpu_shade_edges.py runs the same tables on the device, bit for bit."""
import numpy as np
import pytest

import castray_py
import paths_py
import shade_edges as se

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cast(cs, rays, hits=None, **kw):
    """The oracle's CastRay on a probe batch: every ray must hit (hits: the closest hits of all generations, where there are more than one)."""
    rgba, rgbf, st = cs.cast_rays(rays, **kw)
    assert st["hits_closest"] == (len(rays) if hits is None else hits), st
    return rgba, rgbf, st


# ---- T ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tex", se.TEXTURES + se.QUAD_TEXTURES, ids=se.tex_id)
def test_textures_tell_texels_apart(tex):
    argb, pargb = se.texture(*tex)
    h, w = argb.shape
    assert (w, h) == tex
    for t in (argb, pargb):
        assert len(np.unique(t & 0xFFFFFF)) == t.size, "two texels share a colour"
    for shift in (0, 8, 16, 24):   # neighbouring texels differ in every byte
        b = (argb >> shift) & 255
        assert (b[:, 1:] != b[:, :-1]).all() and (b[1:] != b[:-1]).all()


@pytest.mark.parametrize("tex", se.TEXTURES, ids=se.tex_id)
def test_texture_probes(xrt, tex):
    """Point filter: the float64 restatement on every unambiguous probe, every texel reached under every address mode; both filters: every ray hits,
    and every address mode answers at least one probe unlike another mode."""
    w, h = tex
    argb, _ = se.texture(w, h)
    table = se.uv_table(w, h)
    got = {}
    for spec, rays, sl in se.texture_specs(xrt, w, h, table):
        cs = castray_py.CastRayScene(spec)
        for a in se.ADDRESS:
            for f in se.FILTERS:
                se.set_sampling(xrt, spec, a, f)
                got.setdefault((a, f), []).append(cast(cs, rays)[1])
    got = {k: np.concatenate(v) for k, v in got.items()}
    for a in se.ADDRESS:
        x, y, sure = se.lookup_point_f64(table, w, h, a)
        want = se.texel_rgb_f64(argb, np.where(sure, x, 0), np.where(sure, y, 0))
        bad = sure & (bits(want) != bits(got[a, "point"])).any(axis=1)
        seen = se.texel_of_colour(argb, got[a, "point"])
        print("T %s %s: %d probes, %d unambiguous, %d of %d texels reached" % (se.tex_id(tex), a, len(table), int(sure.sum()), len(np.unique(seen[seen >= 0])), w * h))
        assert sure.sum() >= 1   # (most of the table sits ON a boundary, on purpose: the centre-of-texel probes are what the restatement answers)
        assert not bad.any(), (a, table[np.argmax(bad)], want[np.argmax(bad)], got[a, "point"][np.argmax(bad)])
        assert (seen >= 0).all(), "a point-filtered colour is no texel of the texture"
        assert len(np.unique(seen)) == w * h, "%s: texels never selected: %s" % (a, sorted(set(range(w * h)) - set(seen.tolist()))[:8])
    if w * h > 1:
        for f in se.FILTERS:
            for a in se.ADDRESS:
                assert any((bits(got[a, f]) != bits(got[b, f])).any() for b in se.ADDRESS if b != a), (a, f)


@pytest.mark.parametrize("tex", se.QUAD_TEXTURES, ids=se.tex_id)
def test_interpolated_uv(xrt, orc, tex):
    """The quad whose UVs are interpolated, (uv1 + a*u) + b*v: the float64 restatement of the lookup at the float64 UV of the oracle's own hit
    (triangle, u, v), where that is unambiguous; every ray hits; the modes differ."""
    w, h = tex
    spec = se.quad_spec(xrt, w, h)
    rays = se.quad_rays(xrt)
    hits = orc.OracleScene(spec).intersect(rays)
    assert hits["hit"].all()
    uvs = spec.meshes[0][0].uv.astype(np.float64)[hits["tri"]]
    u, v = hits["u"].astype(np.float64)[:, None], hits["v"].astype(np.float64)[:, None]
    uv = uvs[:, 0] + (uvs[:, 1] - uvs[:, 0]) * u + (uvs[:, 2] - uvs[:, 0]) * v
    assert uv.min() < -3 and uv[:, 0].max() > 4 and uv[:, 1].max() > 3.5
    argb, _ = se.texture(w, h)
    cs = castray_py.CastRayScene(spec)
    got = {}
    for a in se.ADDRESS:
        for f in se.FILTERS:
            se.set_sampling(xrt, spec, a, f)
            got[a, f] = cast(cs, rays)[1]
        x, y, sure = se.lookup_point_f64(uv, w, h, a)
        want = se.texel_rgb_f64(argb, np.where(sure, x, 0), np.where(sure, y, 0))
        bad = sure & (bits(want) != bits(got[a, "point"])).any(axis=1)
        print("T quad %s %s: %d of %d rays unambiguous" % (se.tex_id(tex), a, int(sure.sum()), len(rays)))
        assert sure.sum() >= len(rays) // 2 and not bad.any(), (a, uv[np.argmax(bad)])
    for f in se.FILTERS:
        for a in se.ADDRESS:
            assert any((bits(got[a, f]) != bits(got[b, f])).any() for b in se.ADDRESS if b != a), (a, f)


@pytest.mark.parametrize("tex", [(3, 5), (100, 37), (1, 7)], ids=se.tex_id)
def test_texture_probes_beyond_the_valid_range(xrt, tex):
    """UVs at which (int)(float) leaves the int range: the lookup is DEFINED there by the conversion of the reference's platform (se.cvt_i32) and
    the index guard -- the oracle must give exactly the texel the float32 restatement with that conversion names."""
    w, h = tex
    argb, _ = se.texture(w, h)
    table = se.uv_table_beyond()
    (spec, rays, sl), = se.texture_specs(xrt, w, h, table)
    cs = castray_py.CastRayScene(spec)
    flat = argb.reshape(-1)
    for a in se.ADDRESS:
        se.set_sampling(xrt, spec, a, "point")
        rgbf = cast(cs, rays)[1]
        with np.errstate(invalid="ignore"):
            eff = table + (table - table) * f32(0.25)     # what (uv1 + (uv2 - uv1) * u) + ... makes of the probe: an infinity becomes not-a-number
        idx = np.array([se.lookup_point_guarded(u, v, w, h, a) for u, v in eff])
        want = se.texel_rgb_f64(flat[None, :], idx, np.zeros_like(idx))
        bad = (bits(want) != bits(rgbf)).any(axis=1)
        assert not bad.any(), (a, table[np.argmax(bad)], idx[np.argmax(bad)], se.texel_of_colour(argb, rgbf)[np.argmax(bad)])
        se.set_sampling(xrt, spec, a, "bilinear")
        cast(cs, rays)


def test_the_conversion_restated():
    assert [se.cvt_i32(x) for x in (0.0, -0.0, 0.99, -0.99, 1.5, -1.5, 2147483520.0, -2147483648.0)] == [0, 0, 0, 0, 1, -1, 2147483520, -2 ** 31]
    assert [se.cvt_i32(x) for x in (2.0 ** 31, -2.0 ** 31 - 256, 3e38, float("inf"), -float("inf"), float("nan"))] == [se.INT_MIN] * 6


# ---- Q ---------------------------------------------------------------------------------------------------------------------------------------------
def test_quantisation_probes(xrt):
    """new Color(Vector3) (RT:705/726) on every half (k + 0.5)/255 with its float neighbours, outside [0, 1] and on non-finite values: the colour
    vector is the probe itself, its packed colour the float64 restatement's away from the halves; with MaxReflections 1 the ceiling's packed colour
    re-enters the Lerp of RT:584."""
    spec = se.colour_spec(xrt)
    table = se.colour_table()
    rays = se.probe_rays(xrt, len(table))
    cs = castray_py.CastRayScene(spec)
    rgba, rgbf, st = cast(cs, rays, max_reflections=0)
    fin = np.isfinite(table)
    assert np.array_equal(np.isnan(table), np.isnan(rgbf)) and np.array_equal(table[fin], rgbf[fin])   # 1 * x
    want, sure = se.pack_f64(table)
    print("Q: %d probes, %d channel values away from a half, %d at one" % (len(table), int(sure.sum()), int((~sure).sum())))
    assert sure.sum() >= 3 * 512 and (~sure).sum() >= 3 * 3 * 250   # (256 halves with two neighbours each; the last ones clamp)
    assert np.array_equal(se.channels(rgba)[sure], want[sure]) and (rgba >> 24 == 255).all()
    # the halves themselves round to even (Math.Round): k + 0.5 -> k or k + 1, whichever is even, when the float product IS the half
    v = table[:, 0]
    with np.errstate(invalid="ignore"):
        prod = v * f32(255.0)
        half = np.isfinite(prod) & (prod > 0) & (prod < 255) & (prod - np.floor(prod) == f32(0.5))
    assert half.sum() >= 100 and ((rgba[half] & 255) % 2 == 0).all() and (np.abs((rgba[half] & 255).astype(np.float64) - prod[half]) == 0.5).all()
    # MaxReflections 1, Reflectiveness 0.5: Lerp(unpack(pack(ceiling)), floor, 0.5)
    spec1 = se.colour_spec(xrt, reflectiveness=0.5)
    spec1.max_reflections = 1
    rgba1, rgbf1, st1 = cast(castray_py.CastRayScene(spec1), rays, hits=2 * len(rays))
    ceiling = np.roll(table, 5, axis=0)
    cw, csure = se.pack_f64(ceiling)
    with np.errstate(all="ignore"):
        lerp = cw / 255.0 + (table.astype(np.float64) - cw / 255.0) * 0.5
    ok = csure & np.isfinite(lerp) & (np.abs(lerp) < 1e3)
    assert ok.sum() >= 3 * 500 and np.allclose(rgbf1[ok], lerp[ok], rtol=1e-6, atol=1e-7)
    assert not np.array_equal(rgba1, rgba)


# ---- N ---------------------------------------------------------------------------------------------------------------------------------------------
def test_normal_probes(xrt, orc):
    """RT:520-527 under a spot light at MaxReflections 1: the float64 restatement (normalised blend, SpotLight.cs, the reflected direction) where
    the blend is an ordinary vector; the zero blends really are zero: u = v = 1/4 exactly."""
    spec, rays = se.normal_spec(xrt)
    normals, off, kinds = se.normal_table()
    kinds = np.array(kinds)
    hits = orc.OracleScene(spec).intersect(rays)
    assert hits["hit"].all() and np.array_equal(hits["tri"], np.arange(len(rays)))
    z = kinds == "zero_blend"
    assert z.sum() >= 4 and (hits["u"][z] == 0.25).all() and (hits["v"][z] == 0.25).all()
    ps = paths_py.PathsScene(spec)
    r = ps.cast_rays_paths(rays)
    assert r.stats["hits_closest"] == len(rays)
    n64 = normals.astype(np.float64)
    u, v = hits["u"].astype(np.float64)[:, None], hits["v"].astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        blend = n64[:, 0] + (n64[:, 1] - n64[:, 0]) * u + (n64[:, 2] - n64[:, 0]) * v
        length = np.linalg.norm(blend, axis=1)
        nrm = blend / length[:, None]
        light, margin = se.light_f64(spec.lights[0], hits["w"], nrm)
        want = 0.5 * light   # Lerp(black: the reflection misses, colour (1, 1, 1), 1 - 0.5) * light
        ordinary = np.isfinite(nrm).all(axis=1) & (length > 1e-15) & (length < 1e15) & (margin > 1e-4)
    print("N: %d probes, %d ordinary, %d with a non-finite colour vector" % (len(rays), int(ordinary.sum()), int((~np.isfinite(r.rgbf)).any(axis=1).sum())))
    assert ordinary.sum() >= 250 and np.allclose(r.rgbf[ordinary], want[ordinary], rtol=2e-5, atol=1e-6)
    assert (np.abs(blend[z]).max(axis=1) == 0).all() and (~np.isfinite(r.rgbf[z])).all(), "a zero blend normalises to not-a-number"
    assert (~np.isfinite(r.rgbf[kinds == "nan"])).any(axis=1).all()
    assert (r.rgbf[(kinds == "away") & ordinary] == 0).all()
    # the reflected direction (RT:549-550) is the second vertex of the ray's second segment minus the hit, scaled; it is compared as bits on the GPU.
    lit = ordinary & (r.rgbf > 0).any(axis=1)
    assert lit.sum() >= 150


# ---- L ---------------------------------------------------------------------------------------------------------------------------------------------
def sides(rgbf):
    lit = (np.asarray(rgbf) != 0).any(axis=1)
    return int(lit.sum()), int((~lit).sum()), int((lit[1:] != lit[:-1]).sum())


def test_cone_edge_sweeps(xrt):
    """lightDot > angleCosine (SPOT:52) across the cone's edge: lit and dark as the float64 restatement says wherever that is not a matter of
    rounding, one side each for a quarter of the sweep at least, and neighbouring rays a few ulps of lightDot apart."""
    for name, light, rays in se.cone_cases(xrt):
        spec = se.light_plane_spec(xrt, [light])
        rgba, rgbf, st = cast(castray_py.CastRayScene(spec), rays)
        lit, dark, flips = sides(rgbf)
        print("L cone %s: %d lit, %d dark, %d transitions" % (name, lit, dark, flips))
        assert min(lit, dark) >= len(rays) // 4 and flips >= 1
        pos = np.stack([rays["o"][:, 0], rays["o"][:, 1], np.zeros(len(rays), dtype=np.float32)], axis=1)
        want, margin = se.light_f64(light, pos, np.tile([0.0, 0.0, 1.0], (len(rays), 1)))
        want = want * np.array([0.8, 0.6, 0.4], dtype=np.float32).astype(np.float64)
        clear = margin > 5e-7
        assert clear.sum() >= len(rays) // 2 and ((want[clear] != 0).any(axis=1) == (rgbf[clear] != 0).any(axis=1)).all()
        assert np.allclose(rgbf[clear], want[clear], rtol=1e-4, atol=2e-6)
        # the step: lightDot of neighbouring rays differs by a few float32 ulps (ulp(0.866) = 6e-8) -- no ray of the sweep skips the edge
        t = np.asarray(light["position"]) - pos.astype(np.float64)
        ld = -(t / np.linalg.norm(t, axis=1, keepdims=True)) @ np.asarray(light["direction"])
        assert 0 < np.abs(np.diff(ld)).max() < 8 * 6e-8


def test_surface_dot_sweep(xrt):
    """surfaceDot < 0 (SPOT:45) decided by the SHADING normal: a low light over a plane whose interpolated normal is tilted."""
    spec, rays = se.surface_dot_case(xrt)
    rgba, rgbf, st = cast(castray_py.CastRayScene(spec), rays)
    lit, dark, flips = sides(rgbf)
    print("L surfaceDot: %d lit, %d dark, %d transitions" % (lit, dark, flips))
    assert min(lit, dark) >= len(rays) // 4 and flips >= 1
    pos = np.stack([rays["o"][:, 0], rays["o"][:, 1], np.zeros(len(rays), dtype=np.float32)], axis=1)
    nrm = np.asarray(se.SURFACE_NORMAL, dtype=np.float32).astype(np.float64)
    want, margin = se.light_f64(spec.lights[0], pos, np.tile(nrm / np.linalg.norm(nrm), (len(rays), 1)))
    clear = margin > 5e-7
    assert clear.sum() >= len(rays) // 2 and ((want[clear] != 0).any(axis=1) == (rgbf[clear] != 0).any(axis=1)).all()
    # flat shading of the same plane is lit on both sides: the shading normal decides, not the geometric one
    flat = se.light_plane_spec(xrt, spec.lights)
    assert sides(cast(castray_py.CastRayScene(flat), rays)[1])[1] == 0


def test_light_placements(xrt, orc):
    """A light at the hit point and one 1e-30 above it, directional lights with a dot product of 0, -0 and a direction that is not of unit length,
    32 lights at once."""
    spec = se.light_plane_spec(xrt, [se.overhead(xrt)])
    one = se.rays_down_at(xrt, [se.AT_HIT_XY[0]], y=se.AT_HIT_XY[1])
    w = orc.OracleScene(spec).intersect(one)["w"][0]
    assert np.array_equal(w, np.array([se.AT_HIT_XY[0], se.AT_HIT_XY[1], 0.0], dtype=np.float32))
    cs = castray_py.CastRayScene(spec)
    near = se.rays_down_at(xrt, se.AT_HIT_XY[0] + np.arange(-8, 9) * 2.0 ** -20, y=se.AT_HIT_XY[1])
    for name, light in se.light_at_hit_cases(xrt, w):
        spec.lights = [light]
        rgba, rgbf, st = cast(cs, near)
        print("L %s: centre colour vector %s" % (name, rgbf[8]))
        assert not np.isfinite(rgbf[8]).all() or (rgbf[8] == 0).all()   # dirToLight is not a number (or, with the light above, infinite) there
    rays = se.scattered_rays(xrt)
    colour = np.array([0.8, 0.6, 0.4], dtype=np.float32).astype(np.float64)
    for name, light in se.directional_cases(xrt):
        spec.lights = [light]
        rgba, rgbf, st = cast(cs, rays)
        want = se.light_f64(light, np.zeros((1, 3)), [[0.0, 0.0, 1.0]])[0] * colour
        assert np.allclose(rgbf, np.tile(want, (len(rays), 1)), rtol=1e-6, atol=0), name
        assert (rgbf == 0).all() == name.startswith("dot_")
    spec.lights = se.many_lights(xrt)
    assert len(spec.lights) == 32
    rgba, rgbf, st = cast(cs, rays)
    assert st["rays_shadow"] == 32 * len(rays)
    hits = orc.OracleScene(spec).intersect(rays)
    want = sum(se.light_f64(l, hits["w"], np.tile([0.0, 0.0, 1.0], (len(rays), 1)))[0] for l in spec.lights) * colour
    margin = np.min([se.light_f64(l, hits["w"], np.tile([0.0, 0.0, 1.0], (len(rays), 1)))[1] for l in spec.lights], axis=0)
    clear = margin > 1e-5
    assert clear.sum() >= len(rays) * 3 // 4 and np.allclose(rgbf[clear], want[clear], rtol=1e-4, atol=1e-5)


# ---- S ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [1.5, 1.32])
def test_critical_angle_sweeps(xrt, index):
    """RT:656-694 across asin(1 / index) with currentRefIndex 1: the handed-back refracted direction is the float64 restatement's where the square
    root's argument is clearly positive, not a number where it is clearly negative; a quarter of the sweep on either side.  With currentRefIndex =
    index (n1 / n2 = 1 / index) nothing is critical: every direction is finite."""
    spec = se.glass_spec(xrt, index)
    rays = se.critical_sweep(xrt, index)
    ps = paths_py.PathsScene(spec)
    r = ps.cast_rays_paths(rays)
    assert r.stats["hits_closest"] == len(rays)
    back = r.rays_back["d"]
    finite = np.isfinite(back).all(axis=1)
    want, arg = se.snell_f64(rays["d"], np.tile([0.0, 0.0, 1.0], (len(rays), 1)), index, 1.0)
    print("S index %g: %d finite, %d not, argument from %.3g to %.3g" % (index, int(finite.sum()), int((~finite).sum()), arg.max(), arg.min()))
    assert finite.sum() >= max(100, len(rays) // 4) and (~finite).sum() >= max(100, len(rays) // 4)
    pos, neg = arg > 3e-7, arg < -3e-7     # float32 cos1 carries 6e-8: further away than that the sign is certain
    assert pos.sum() >= 100 and neg.sum() >= 100 and finite[pos].all() and not finite[neg].any()
    assert np.allclose(back[pos], want[pos], rtol=0, atol=5e-4)   # (cos2 = sqrt(arg) near 0: the error of arg is magnified)
    far = arg > 1e-4
    assert far.sum() >= 10 and np.allclose(back[far], want[far], rtol=0, atol=1e-5)
    assert np.allclose(r.rays_back["o"], np.array([se.AIM[0], se.AIM[1], 0.0]), rtol=0, atol=1e-5)   # RT:692: the hit point
    r2 = ps.cast_rays_paths(rays, ref_index=float(f32(index)))
    want2, arg2 = se.snell_f64(rays["d"], np.tile([0.0, 0.0, 1.0], (len(rays), 1)), index, index)
    assert np.isfinite(r2.rays_back["d"]).all() and (arg2 > 0.1).all() and np.allclose(r2.rays_back["d"], want2, rtol=0, atol=1e-5)


def test_refraction_index_grid(xrt):
    """RefractionIndex {0: configs.material's default, 1: the initial currentRefIndex, 1.5, 1e-20, 1e20} x currentRefIndex {0, 1, 1.5} at normal,
    grazing (cos1 = 2^-24) and ordinary incidence: every ray hits, and the float64 restatement where n1 / n2 is an ordinary number."""
    rays = se.special_incidence(xrt)
    nrm = np.asarray(se.SURFACE_NORMAL, dtype=np.float32).astype(np.float64)
    nrm = nrm / np.linalg.norm(nrm)
    n_finite = n_not = 0
    for index in se.INDEX_GRID:
        ps = paths_py.PathsScene(se.glass_spec(xrt, index, normal=se.SURFACE_NORMAL))
        for ref in se.REF_GRID:
            r = ps.cast_rays_paths(rays, ref_index=ref)
            assert r.stats["hits_closest"] == len(rays), (index, ref)
            finite = np.isfinite(r.rays_back["d"]).all(axis=1)
            n_finite += int(finite.sum()); n_not += int((~finite).sum())
            n1, n2 = (1.0, ref) if f32(ref) == f32(index) else (index, 1.0)
            if n2 != 0 and 0.1 < n1 / n2 < 10:
                d = rays["d"].astype(np.float64)
                want, arg = se.snell_f64(d / np.linalg.norm(d, axis=1, keepdims=True), np.tile(nrm, (len(rays), 1)), index, ref)
                unit = np.abs(np.linalg.norm(d, axis=1) - 1) < 1e-6     # (the reference does not normalise the incoming direction: RT:662)
                ok = unit & (arg > 1e-6)
                assert np.allclose(r.rays_back["d"][ok], want[ok], rtol=0, atol=1e-5), (index, ref)
    print("S grid: %d finite refracted directions, %d not" % (n_finite, n_not))
    assert n_finite >= 10 and n_not >= 10


# ---- frames ----------------------------------------------------------------------------------------------------------------------------------------
def test_frames_reach_their_edges(xrt, orc):
    """The frames tests/test_gpu_shade_edges.py renders: the textured quad shows UVs beyond one period in every direction, and in the glass frame the
    critical angle crosses the image (refracted directions of the primary rays finite and not)."""
    for name, spec in (("T quad", se.quad_spec(xrt, 7, 5)), ("Q", se.colour_frame_spec(xrt)), ("N", se.normal_frame_spec(xrt))):
        o = orc.OracleScene(spec)
        hits = o.intersect(o.primary_rays())
        print("%s frame: %d primary hits of %d" % (name, int(hits["hit"].sum()), len(hits)))
        assert hits["hit"].sum() >= se.FRAME_FLOOR
    rgba, rgbf, st = orc.OracleScene(se.normal_frame_spec(xrt)).render()
    assert (~np.isfinite(rgbf)).any(axis=1).sum() >= 5, "the N frame shows no not-a-number normal"
    g = se.glass_frame_spec(xrt)
    ps = paths_py.PathsScene(g)
    r = ps.cast_rays_paths(ps.primary_rays(), max_reflections=1)
    hit = r.stats["hits_closest"]
    finite = np.isfinite(r.rays_back["d"]).all(axis=1)
    print("S frame: %d primary hits, %d finite directions handed back, %d not" % (hit, int(finite.sum()), int((~finite).sum())))
    assert (~finite).sum() >= 500 and finite.sum() >= 500 and hit >= se.FRAME_FLOOR
