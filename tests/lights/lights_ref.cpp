// TEST INFRASTRUCTURE -- the checker of xrt_light_hits: the light loop of RayTracer.CastRay (RT:534-542) of the CPU oracle on caller-given
// hits.  The oracle is included unmodified (through the checker of xrt_cast_rays, whose orc_cast_rays this library exports too, so that one
// scene handle serves both); its CastRay keeps the light sum to itself, so this translation unit restates RT:520-542 with "the query returned
// hits[i]" in the query's place, written with the oracle's own IsLightPathObstructed and GetLightForFragment.
// tests/test_lights_cpu.py pins the restatement: on the oracle's own hits its light sum times the surface colour must be what the oracle's
// CastRay hands to `new Color(...)` at MaxReflections 0 (RT:726).
#include "../castray/castray_ref.cpp"

extern "C" {

// for every i, with `result` = hits[i] (hit == 0, or a mesh / tri the scene does not have -- what the device form treats as a miss: the query
// returned false, light (0, 0, 0) and every amount 0): amount_out[i * n_lights + l] = IsLightPathObstructed(result, lights[l]) and
// light_out[3i ..] = RT:534-542.  Either output may be null.  Of the hit mesh, tri, u, v and (wx, wy, wz) are read, as bits.
// counts_out (nullable) classifies the pairs of the live entries by the branches of RT:485-501, from the same query made once more:
//   [0] obstructed (the query hit, d below the distance)   [1] of those, the blocker's material is Transparent
//   [2] the query hit, d NOT below the distance            [3] live entries
// color_out (nullable, 3 floats per entry; needs opts for the texture lookup): the oracle's SurfaceColor of a live entry (RT:711-724: what RT:726
// multiplies the light sum by), zeros for a miss.
int orc_light_hits(const orc_scene *s, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts, const xrt_hit *hits, int64_t n, float *light_out,
                   float *amount_out, uint64_t *counts_out, float *color_out) {
    if (!s->built) return -1;
    RayTracer rt{};
    rt.scene = s;
    for (int i = 0; i < n_lights; i++) rt.lights.push_back(MakeLight(lights[i]));
    if (color_out && !opts) return -2;
    if (opts) { rt.MaxReflections = opts->max_reflections; rt.AddressMode = opts->address_mode; rt.TextureFiltering = opts->filtering; }
    Counters c, c2;
    uint64_t counts[4] = {0, 0, 0, 0};
    for (int64_t i = 0; i < n; i++) {
        const xrt_hit &h = hits[i];
        const bool found = h.hit != 0 && h.mesh >= 0 && h.mesh < (int)s->meshes.size() && h.tri >= 0 && h.tri < (int)s->meshes[h.mesh]->Triangles.size();
        Vector3 lightResult = V3(0, 0, 0);   // RT:534
        Vector3 color = V3(0, 0, 0);
        if (found) {
            counts[3]++;
            IntersectionResult result;
            result.mesh = s->meshes[h.mesh].get();
            result.triangle = &result.mesh->Triangles[h.tri];
            result.u = h.u; result.v = h.v; result.d = h.d;
            result.worldPosition = V3(h.wx, h.wy, h.wz);
            const Material &material = result.mesh->MeshMaterial;
            if (color_out) color = rt.SurfaceColor(result, material);
            Vector3 fragmentNormal;
            if (material.InterpolateNormals) {   // RT:520-527
                Vector3 n1 = result.triangle->n2 - result.triangle->n1;
                Vector3 n2 = result.triangle->n3 - result.triangle->n1;
                fragmentNormal = result.triangle->n1 + (n1 * result.u) + (n2 * result.v);
                fragmentNormal = Normalize(fragmentNormal);
            } else {
                fragmentNormal = result.triangle->surfaceNormal;
            }
            for (size_t l = 0; l < rt.lights.size(); l++) {   // RT:535-542
                float lightAmount = rt.IsLightPathObstructed(result, rt.lights[l], c);
                if (lightAmount != 1.0f)
                    lightResult = lightResult + rt.lights[l].GetLightForFragment(result.worldPosition, fragmentNormal) * (1.0f - lightAmount);
                if (amount_out) amount_out[i * n_lights + (int64_t)l] = lightAmount;
                // the same query once more, to say which branch of RT:485-501 the pair took
                const Light &light = rt.lights[l];
                Vector3 dirToLight;
                float distanceToLight;
                if (light.IsPositionable()) {
                    dirToLight = light.Position - result.worldPosition;
                    distanceToLight = Length(dirToLight);
                    dirToLight = Normalize(dirToLight);
                } else {
                    dirToLight = -light.Direction;
                    distanceToLight = FLT_MAX;
                }
                Ray shadowRay{result.worldPosition, dirToLight};
                IntersectionResult blocker;
                if (s->manager.GetRayIntersection(shadowRay, blocker, result.triangle, c2)) {
                    if (blocker.d < distanceToLight) {
                        counts[0]++;
                        if (blocker.mesh->MeshMaterial.Transparent) counts[1]++;
                    } else counts[2]++;
                }
            }
        } else if (amount_out) {
            for (int l = 0; l < n_lights; l++) amount_out[i * n_lights + l] = 0.0f;
        }
        if (light_out) { light_out[3 * i] = lightResult.X; light_out[3 * i + 1] = lightResult.Y; light_out[3 * i + 2] = lightResult.Z; }
        if (color_out) { color_out[3 * i] = color.X; color_out[3 * i + 1] = color.Y; color_out[3 * i + 2] = color.Z; }
    }
    if (counts_out) for (int k = 0; k < 4; k++) counts_out[k] = counts[k];
    return rt.bad_lookup ? -3 : 0;
}

}  // extern "C"
