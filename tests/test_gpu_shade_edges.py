"""k_shade's per-hit arithmetic at its numeric edges on the MI355X: the tables of tests/shade_edges.py through xrt_cast_rays (k_ingest), bit for bit
against the checker (tests/castray: the oracle's CastRay) -- RGBA8, the fp32 colour vector, the ray counts --, through xrt_cast_rays_paths against
tests/paths where directions matter (the reflected ray's segment, the refracted `ref Ray ray` of RT:692-694 as bits), and as small frames, so that
the frame instantiations of k_shade (finish / end-early; the ray tree of a scene with a Transparent material) meet the same edges.  The population
conditions tests/test_shade_edges_cpu.py asserts on the oracle are asserted once more on what the GPU returned."""
import numpy as np
import pytest

import castray_py
import paths_py
import shade_edges as se
from test_gpu_cast_rays import check
from test_gpu_paths import check as check_paths
from test_shade_edges_cpu import sides

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def product_lights(xrt, tracer, lights):
    """tracer.Lights of a spec's light dicts (as configs.build_product makes them)."""
    tracer.Lights = []
    for l in lights:
        if l["kind"] == xrt.abi.LIGHT_SPOT:
            L = xrt.api.SpotLight()
            L.Position, L.SpotAngle, L.DecayExponent = l["position"], l["spot_angle"], l["decay_exponent"]
        else:
            L = xrt.api.DirectionalLight()
        L.Direction, L.Color, L.Intensity = l["direction"], l["color"], l["intensity"]
        tracer.Lights.append(L)


def sampling(xrt, spec, tracer, a, f):
    se.set_sampling(xrt, spec, a, f)
    tracer.AddressMode, tracer.TextureFiltering = spec.address_mode, spec.filtering


def all_hit(tracer, n):
    assert tracer.last_stats["hits_closest"] == n, (tracer.last_stats["hits_closest"], n)


def frame_equal(xrt, orc, spec, tracer=None, what=""):
    """xrt_render's frame == the oracle's: RGBA8, colour vectors, the ray counts."""
    if tracer is None:
        tracer = xrt.configs.build_product(spec)[1]
    rgba, rgbf = tracer.Render(want_float=True)
    o_rgba, o_rgbf, o_st = orc.OracleScene(spec).render(nthreads=16)
    bad = int((np.asarray(rgba).reshape(-1) != o_rgba).sum())
    assert bad == 0, "%s: %d of %d pixels differ" % (what, bad, o_rgba.size)
    assert np.array_equal(bits(rgbf).reshape(-1), bits(o_rgbf).reshape(-1)), what
    for k in ("rays_closest", "rays_shadow", "hits_closest", "shaded_hits"):
        assert tracer.last_stats[k] == o_st[k], (what, k, tracer.last_stats[k], o_st[k])
    return o_st


# ---- T ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tex", se.TEXTURES, ids=se.tex_id)
def test_texture_probes(xrt, tex):
    w, h = tex
    argb, _ = se.texture(w, h)
    got = {}
    for spec, rays, sl in se.texture_specs(xrt, w, h, se.uv_table(w, h)):
        cs = castray_py.CastRayScene(spec)
        scene, tracer = xrt.configs.build_product(spec)
        for a in se.ADDRESS:
            for f in se.FILTERS:
                sampling(xrt, spec, tracer, a, f)
                got.setdefault((a, f), []).append(check(cs, tracer, rays, what="T %s %s %s" % (se.tex_id(tex), a, f))[1])
                all_hit(tracer, len(rays))
    got = {k: np.concatenate(v) for k, v in got.items()}
    for a in se.ADDRESS:
        seen = se.texel_of_colour(argb, got[a, "point"])
        assert (seen >= 0).all() and len(np.unique(seen)) == w * h, (a, "texels never selected on the GPU")
        if w * h > 1:
            for f in se.FILTERS:
                assert any((bits(got[a, f]) != bits(got[b, f])).any() for b in se.ADDRESS if b != a), (a, f)


@pytest.mark.parametrize("tex", se.QUAD_TEXTURES, ids=se.tex_id)
def test_interpolated_uv_batch_and_frame(xrt, orc, tex):
    """(uv1 + a*u) + b*v over eight periods by six: random rays straight down, and the 96 x 64 frame of the oblique camera."""
    spec = se.quad_spec(xrt, *tex)
    rays = se.quad_rays(xrt)
    cs = castray_py.CastRayScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    got = {}
    for a in se.ADDRESS:
        for f in se.FILTERS:
            sampling(xrt, spec, tracer, a, f)
            got[a, f] = check(cs, tracer, rays, what="T quad %s %s %s" % (se.tex_id(tex), a, f))[1]
            all_hit(tracer, len(rays))
            st = frame_equal(xrt, orc, spec, tracer, "T quad frame %s %s %s" % (se.tex_id(tex), a, f))
            assert st["hits_closest"] >= se.FRAME_FLOOR
    for f in se.FILTERS:
        for a in se.ADDRESS:
            assert any((bits(got[a, f]) != bits(got[b, f])).any() for b in se.ADDRESS if b != a), (a, f)


@pytest.mark.parametrize("tex", [(3, 5), (100, 37), (1, 7)], ids=se.tex_id)
def test_texture_probes_beyond_the_valid_range(xrt, tex):
    """2^31, 2^32 + 512, -2^31, -2^33, 3e38, +-inf, NaN in one component or in both: (int)(float) is cvt_i32 (xrt_core.h) in the kernel and in the
    oracle, the guarded texel is the same one (DESIGN.md 3 "Range of validity", texture lookup)."""
    w, h = tex
    (spec, rays, sl), = se.texture_specs(xrt, w, h, se.uv_table_beyond())
    cs = castray_py.CastRayScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    for a in se.ADDRESS:
        for f in se.FILTERS:
            sampling(xrt, spec, tracer, a, f)
            check(cs, tracer, rays, what="TOUT %s %s %s" % (se.tex_id(tex), a, f))
            all_hit(tracer, len(rays))


# ---- Q ---------------------------------------------------------------------------------------------------------------------------------------------
def test_quantisation_probes(xrt, orc):
    table = se.colour_table()
    rays = se.probe_rays(xrt, len(table))
    spec = se.colour_spec(xrt)
    cs = castray_py.CastRayScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    check(cs, tracer, rays, what="Q MaxReflections 0")
    all_hit(tracer, len(rays))
    spec1 = se.colour_spec(xrt, reflectiveness=0.5)
    spec1.max_reflections = 1
    cs1 = castray_py.CastRayScene(spec1)
    scene1, tracer1 = xrt.configs.build_product(spec1)
    check(cs1, tracer1, rays, what="Q MaxReflections 1")
    all_hit(tracer1, 2 * len(rays))
    # the same probes as a frame (the finish / end-early instantiations of k_shade)
    st = frame_equal(xrt, orc, se.colour_frame_spec(xrt), None, "Q frame")
    assert st["hits_closest"] >= se.FRAME_FLOOR


# ---- N ---------------------------------------------------------------------------------------------------------------------------------------------
def test_normal_probes(xrt, orc):
    """Zero, non-unit, opposed and not-a-number blends through normalize, reflect, the light sum and pack_color: the colours, and the reflected ray
    of RT:549-550 as the bits of its recorded segment."""
    spec, rays = se.normal_spec(xrt)
    ps = paths_py.PathsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    r = check_paths(ps, tracer, rays, what="N")
    all_hit(tracer, len(rays))
    assert (~np.isfinite(r.rgbf)).any(axis=1).sum() >= 8
    check(castray_py.CastRayScene(spec), tracer, rays, what="N cast_rays")
    tracer.MaxReflections = 0
    check(castray_py.CastRayScene(spec), tracer, rays, what="N MaxReflections 0")
    st = frame_equal(xrt, orc, se.normal_frame_spec(xrt), None, "N frame")
    assert st["hits_closest"] >= se.FRAME_FLOOR


# ---- L ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cone_edge_sweeps(xrt):
    for name, light, rays in se.cone_cases(xrt):
        spec = se.light_plane_spec(xrt, [light])
        scene, tracer = xrt.configs.build_product(spec)
        rgba, rgbf = check(castray_py.CastRayScene(spec), tracer, rays, what="L cone " + name)
        all_hit(tracer, len(rays))
        lit, dark, flips = sides(rgbf)
        assert min(lit, dark) >= len(rays) // 4 and flips >= 1, (name, lit, dark, flips)


def test_surface_dot_sweep(xrt):
    spec, rays = se.surface_dot_case(xrt)
    scene, tracer = xrt.configs.build_product(spec)
    rgba, rgbf = check(castray_py.CastRayScene(spec), tracer, rays, what="L surfaceDot")
    all_hit(tracer, len(rays))
    lit, dark, flips = sides(rgbf)
    assert min(lit, dark) >= len(rays) // 4 and flips >= 1, (lit, dark, flips)


def test_light_placements(xrt, orc):
    spec = se.light_plane_spec(xrt, [se.overhead(xrt)])
    cs = castray_py.CastRayScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    w = orc.OracleScene(spec).intersect(se.rays_down_at(xrt, [se.AT_HIT_XY[0]], y=se.AT_HIT_XY[1]))["w"][0]
    near = se.rays_down_at(xrt, se.AT_HIT_XY[0] + np.arange(-8, 9) * 2.0 ** -20, y=se.AT_HIT_XY[1])
    rays = se.scattered_rays(xrt)
    cases = [(name, [light], near) for name, light in se.light_at_hit_cases(xrt, w)] + [(name, [light], rays) for name, light in se.directional_cases(xrt)]
    many = se.many_lights(xrt)
    cases += [("32 lights", many, rays), ("33 lights", many + [xrt.configs.spot((1.0, -2.0, 9.0))], rays), ("no light", [], rays)]
    for name, lights, batch in cases:
        spec.lights = lights
        product_lights(xrt, tracer, lights)
        check(cs, tracer, batch, what="L " + name)
        all_hit(tracer, len(batch))
        assert tracer.last_stats["rays_shadow"] == len(lights) * len(batch)


# ---- S ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [1.5, 1.32])
def test_critical_angle_sweeps(xrt, index):
    """The refracted direction handed back (RT:692-694) across the critical angle, as bits: not-a-number on one side, finite on the other."""
    spec = se.glass_spec(xrt, index)
    rays = se.critical_sweep(xrt, index)
    ps = paths_py.PathsScene(spec)
    scene, tracer = xrt.configs.build_product(spec)
    check_paths(ps, tracer, rays, what="S index %g" % index)
    all_hit(tracer, len(rays))
    back = tracer.CastRays(rays, paths=True)[-1]
    finite = np.isfinite(back["d"]).all(axis=1)
    assert finite.sum() >= len(rays) // 4 and (~finite).sum() >= len(rays) // 4, (int(finite.sum()), int((~finite).sum()))
    check_paths(ps, tracer, rays, ref=float(np.float32(index)), what="S index %g from inside" % index)


def test_refraction_index_grid(xrt):
    rays = se.special_incidence(xrt)
    for index in se.INDEX_GRID:
        spec = se.glass_spec(xrt, index, normal=se.SURFACE_NORMAL)
        ps = paths_py.PathsScene(spec)
        scene, tracer = xrt.configs.build_product(spec)
        for ref in se.REF_GRID:
            check_paths(ps, tracer, rays, ref=ref, what="S index %g in %g" % (index, ref))
            all_hit(tracer, len(rays))


def test_glass_frame(xrt, orc):
    """The ray-tree instantiation: the quad under an oblique camera, the critical angle across the image."""
    for index in (1.5, 0.0):
        spec = se.glass_frame_spec(xrt, index)
        st = frame_equal(xrt, orc, spec, None, "S frame, index %g" % index)
        assert st["hits_closest"] >= se.FRAME_FLOOR
