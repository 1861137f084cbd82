// TEST INFRASTRUCTURE -- the checker of xrt_shade_hits: the first level of RayTracer.CastRay (RT:514-737) of the CPU oracle on caller-given
// hits.  The oracle is included unmodified (through the checker of xrt_cast_rays, whose orc_cast_rays this library exports too, so that one
// scene handle serves both); its CastRay makes the closest-hit query itself (RT:512), so this translation unit restates ONE level of it with
// "the query returned hits[i]" in the query's place and calls the oracle's own IsLightPathObstructed and CastRay for everything below.
// tests/test_shade_hits_cpu.py pins the restatement: on the oracle's own hits it must give what the oracle's CastRay gives.
#include "../castray/castray_ref.cpp"

namespace {

// RT:514-737 of CastRay(ref ray, out resultColor, iteration, origin, null, currentRefIndex) on `result` (found: what RT:512 returned).
// Line for line oracle.cpp's CastRay behind its query; the query's two counters (rays_closest, hits_closest) are not touched -- no query was made.
void ShadeLevel(RayTracer &rt, Ray &ray, bool found, const IntersectionResult &result, uint32_t &resultColor, int iteration, float currentRefIndex, Counters &c,
                Vector3 *colorVectorOut) {
    if (found) {
        c.shaded_hits++;
        const Material &material = result.mesh->MeshMaterial;
        Vector3 fragmentNormal;
        if (material.InterpolateNormals) {   // RT:520-527
            Vector3 n1 = result.triangle->n2 - result.triangle->n1;
            Vector3 n2 = result.triangle->n3 - result.triangle->n1;
            fragmentNormal = result.triangle->n1 + (n1 * result.u) + (n2 * result.v);
            fragmentNormal = Normalize(fragmentNormal);
        } else {
            fragmentNormal = result.triangle->surfaceNormal;
        }
        Vector3 lightResult = V3(0, 0, 0);   // RT:534-542
        for (size_t i = 0; i < rt.lights.size(); i++) {
            float lightAmount = rt.IsLightPathObstructed(result, rt.lights[i], c);
            if (lightAmount != 1.0f)
                lightResult = lightResult + rt.lights[i].GetLightForFragment(result.worldPosition, fragmentNormal) * (1.0f - lightAmount);
        }
        if (iteration < rt.MaxReflections) {   // RT:545-707
            Ray r;
            r.Position = result.worldPosition;
            r.Direction = Reflect(ray.Direction, fragmentNormal);
            r.Direction = Normalize(r.Direction);
            uint32_t reflectionColor;
            rt.CastRay(r, reflectionColor, iteration + 1, result.triangle, currentRefIndex, c, nullptr);
            Vector3 surfaceColor = rt.SurfaceColor(result, material);
            Vector3 colorVector = Lerp(ColorToVector3(reflectionColor), surfaceColor, 1.0f - material.Reflectiveness) * lightResult;   // RT:584
            if (material.Transparent) {   // RT:586-702
                float n1, n2;
                if (currentRefIndex == material.RefractionIndex) { n1 = 1.0f; n2 = currentRefIndex; }
                else { n1 = material.RefractionIndex; n2 = 1.0f; }
                float cos1 = Dot(fragmentNormal, -ray.Direction);
                double ratio = (double)(n1 / n2);
                double c1 = (double)cos1;
                float cos2 = (float)std::sqrt(1 - (ratio * ratio) * (1 - (c1 * c1)));
                Vector3 refract;
                if (cos1 >= 0) refract = (n1 / n2) * ray.Direction + ((n1 / n2) * cos1 - cos2) * fragmentNormal;
                else refract = (n1 / n2) * ray.Direction - ((n1 / n2) * cos1 - cos2) * fragmentNormal;
                ray.Position = result.worldPosition;   // RT:692-694
                ray.Direction = Normalize(refract);
                uint32_t refractColor;
                rt.CastRay(ray, refractColor, iteration + 1, result.triangle, n2, c, nullptr);
                colorVector = Lerp(ColorToVector3(refractColor), colorVector, result.triangle->color.W);
            }
            if (colorVectorOut) *colorVectorOut = colorVector;
            resultColor = ColorFromVector3(colorVector);   // RT:705
        } else {   // RT:708-727
            Vector3 surfaceColor = rt.SurfaceColor(result, material);
            Vector3 colorVector = lightResult * surfaceColor;
            if (colorVectorOut) *colorVectorOut = colorVector;
            resultColor = ColorFromVector3(colorVector);
        }
    } else {
        if (colorVectorOut) *colorVectorOut = V3(0, 0, 0);
        resultColor = ColorFromVector3(V3(0, 0, 0));   // RT:732
    }
}

}  // namespace

extern "C" {

// for every i: CastRay(ref rays[i], out color, iteration, origin, null, ref_index) with RT:512 replaced by "the query returned hits[i]".
// hit == 0, or a mesh / tri the scene does not have (what the device form shades as a miss): the query returned false.  Of the ray only
// the direction is read; of the hit mesh, tri, u, v and (wx, wy, wz), as bits.  stats: the counters of everything below the first level
// plus the first level's shaded hits, pixels = n.
int orc_shade_hits(const orc_scene *s, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts, const xrt_ray *rays, const xrt_hit *hits,
                   int64_t n, int32_t iteration, float ref_index, uint32_t *rgba_out, float *rgb_f32_out, xrt_stats *stats) {
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
        const xrt_hit &h = hits[i];
        IntersectionResult result;
        bool found = h.hit != 0 && h.mesh >= 0 && h.mesh < (int)s->meshes.size() && h.tri >= 0 && h.tri < (int)s->meshes[h.mesh]->Triangles.size();
        if (found) {
            result.mesh = s->meshes[h.mesh].get();
            result.triangle = &result.mesh->Triangles[h.tri];
            result.u = h.u; result.v = h.v; result.d = h.d;
            result.worldPosition = V3(h.wx, h.wy, h.wz);
        }
        uint32_t color = 0;
        Vector3 cv = V3(0, 0, 0);
        ShadeLevel(rt, ray, found, result, color, iteration, ref_index, c, &cv);
        rgba_out[i] = color;
        if (rgb_f32_out) { rgb_f32_out[3 * i] = cv.X; rgb_f32_out[3 * i + 1] = cv.Y; rgb_f32_out[3 * i + 2] = cv.Z; }
    }
    FillStats(stats, c, (uint64_t)n, 0);
    return rt.bad_lookup ? -3 : 0;
}

}  // extern "C"
