// TEST INFRASTRUCTURE -- the checker of xrt_cast_rays: RayTracer.CastRay (RT:506-737) of the CPU oracle on caller-given rays.
// The oracle is included unmodified; its CastRay is not exported there, so this translation unit adds one entry point
// (tests/castray_py.py builds it with the oracle Makefile's flags).
#include "../../oracle/oracle.cpp"

extern "C" {

// for every i: CastRay(ref rays[i], out color, iteration, origin_i, null, ref_index) with origin_i = ResolveIgnore(rays[i]) and a fresh copy of
// the ray (CastRay mutates its ray where it refracts, RT:692-694).  rgba_out[i] = the packed Color, rgb_f32_out[3i..] (nullable) = the vector
// handed to `new Color(...)`.  stats: the counters of all the calls, pixels = n.
int orc_cast_rays(const orc_scene *s, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts, const xrt_ray *rays, int64_t n,
                  int32_t iteration, float ref_index, uint32_t *rgba_out, float *rgb_f32_out, xrt_stats *stats) {
    if (!s->built) return -1;
    RayTracer rt{};
    rt.scene = s;
    for (int i = 0; i < n_lights; i++) rt.lights.push_back(MakeLight(lights[i]));
    rt.MaxReflections = opts->max_reflections;
    rt.AddressMode = opts->address_mode;
    rt.TextureFiltering = opts->filtering;
    Counters c;
    for (int64_t i = 0; i < n; i++) {
        Ray ray{V3(rays[i].o[0], rays[i].o[1], rays[i].o[2]), V3(rays[i].d[0], rays[i].d[1], rays[i].d[2])};
        uint32_t color = 0;
        Vector3 cv = V3(0, 0, 0);
        rt.CastRay(ray, color, iteration, ResolveIgnore(s, rays[i]), ref_index, c, &cv);
        rgba_out[i] = color;
        if (rgb_f32_out) { rgb_f32_out[3 * i] = cv.X; rgb_f32_out[3 * i + 1] = cv.Y; rgb_f32_out[3 * i + 2] = cv.Z; }
    }
    FillStats(stats, c, (uint64_t)n, 0);
    return rt.bad_lookup ? -3 : 0;
}

}  // extern "C"
