// TEST INFRASTRUCTURE -- the checker of xrt_surface_hits: what RayTracer.CastRay (RT:506-737) of the CPU oracle computes at a hit without
// asking the scene anything, on caller-given hits.  The oracle is included unmodified (through the checker of xrt_cast_rays, whose
// orc_cast_rays this library exports too, so that one scene handle serves both); its CastRay keeps these values to itself, so this
// translation unit restates RT:520-531 (fragment normal), RT:547-550 (the reflected ray), RT:568-581 (surface colour, through the oracle's own
// SurfaceColor and LookupUV) and RT:656-694 (the Snell refraction) with "the query returned hits[i]" in the query's place, written with the
// oracle's own Vector3 operations.
// tests/test_surface_cpu.py pins the restatement against the oracle's CastRay: the colour times the light sum is its colour vector at
// MaxReflections 0, the reflected ray ends where its reflection segment ends, and the refracted ray is the `ref ray` it leaves behind.
#include "../castray/castray_ref.cpp"

namespace {

struct SurfaceRec {   // xrt_surface
    float normal[3], reflectiveness, color[3], alpha, uv[2], refraction_index, next_ref_index;
    int32_t flags, reserved[3];
};
static_assert(sizeof(SurfaceRec) == 64 && sizeof(SurfaceRec) == sizeof(xrt_surface), "xrt_surface is 64 bytes");

void NullRay(xrt_ray &r) {
    std::memset(&r, 0, sizeof(r));
    r.ignore_mesh = -1; r.ignore_tri = -1;
}
void PutRay(xrt_ray &r, const Vector3 &p, const Vector3 &d, int mesh, int tri) {
    r.o[0] = p.X; r.o[1] = p.Y; r.o[2] = p.Z;
    r.d[0] = d.X; r.d[1] = d.Y; r.d[2] = d.Z;
    r.ignore_mesh = mesh; r.ignore_tri = tri;
}

}  // namespace

extern "C" {

// for every i, with `result` = hits[i] (hit == 0, or a mesh / tri the scene does not have -- what the device form treats as a miss): the
// surface record, the reflected ray and the refracted ray as include/xrt.h states them.  rays may be null when both ray outputs are.
// counts_out (nullable, 9 words) classifies the entries by the branches taken:
//   [0] live   [1] InterpolateNormals   [2] UseTexture   [3] Transparent
//   [4] refractions with currentRefIndex == RefractionIndex   [5] ... and with !=
//   [6] refractions with cos1 >= 0   [7] ... and with cos1 < 0 (NaN counts here, as the reference's `else`)   [8] refractions whose direction has a NaN
int orc_surface_hits(const orc_scene *s, const xrt_render_opts *opts, const xrt_ray *rays, const xrt_hit *hits, int64_t n, float current_ref_index,
                     xrt_surface *surface_out, xrt_ray *reflect_out, xrt_ray *refract_out, uint64_t *counts_out) {
    if (!s->built || !opts) return -1;
    if (!rays && (reflect_out || refract_out)) return -2;
    RayTracer rt{};
    rt.scene = s;
    rt.MaxReflections = opts->max_reflections; rt.AddressMode = opts->address_mode; rt.TextureFiltering = opts->filtering;
    uint64_t counts[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; i++) {
        const xrt_hit &h = hits[i];
        const bool found = h.hit != 0 && h.mesh >= 0 && h.mesh < (int)s->meshes.size() && h.tri >= 0 && h.tri < (int)s->meshes[h.mesh]->Triangles.size();
        if (!found) {
            if (surface_out) std::memset(&surface_out[i], 0, sizeof(xrt_surface));
            if (reflect_out) NullRay(reflect_out[i]);
            if (refract_out) NullRay(refract_out[i]);
            continue;
        }
        counts[0]++;
        IntersectionResult result;
        result.mesh = s->meshes[h.mesh].get();
        result.triangle = &result.mesh->Triangles[h.tri];
        result.u = h.u; result.v = h.v; result.d = h.d;
        result.worldPosition = V3(h.wx, h.wy, h.wz);
        const Material &material = result.mesh->MeshMaterial;
        Vector3 fragmentNormal;
        if (material.InterpolateNormals) {   // RT:520-527
            Vector3 n1 = result.triangle->n2 - result.triangle->n1;
            Vector3 n2 = result.triangle->n3 - result.triangle->n1;
            fragmentNormal = result.triangle->n1 + (n1 * result.u) + (n2 * result.v);
            fragmentNormal = Normalize(fragmentNormal);
            counts[1]++;
        } else {
            fragmentNormal = result.triangle->surfaceNormal;
        }
        if (material.UseTexture) counts[2]++;
        if (material.Transparent) counts[3]++;
        float n1 = 1.0f, n2 = current_ref_index;
        if (material.Transparent) {   // RT:656-667
            if (current_ref_index == material.RefractionIndex) { n1 = 1.0f; n2 = current_ref_index; }
            else { n1 = material.RefractionIndex; n2 = 1.0f; }
        }
        if (surface_out) {
            SurfaceRec r;
            std::memset(&r, 0, sizeof(r));
            r.normal[0] = fragmentNormal.X; r.normal[1] = fragmentNormal.Y; r.normal[2] = fragmentNormal.Z;
            r.reflectiveness = material.Reflectiveness;
            const Vector3 surfaceColor = rt.SurfaceColor(result, material);   // RT:568-581
            r.color[0] = surfaceColor.X; r.color[1] = surfaceColor.Y; r.color[2] = surfaceColor.Z;
            r.alpha = result.triangle->color.W;
            // RT:570-572, formed whether or not the texture is used
            Vector2 uv1 = result.triangle->uv2 - result.triangle->uv1;
            Vector2 uv2 = result.triangle->uv3 - result.triangle->uv1;
            Vector2 interpolatedUV = result.triangle->uv1 + (uv1 * result.u) + (uv2 * result.v);
            r.uv[0] = interpolatedUV.X; r.uv[1] = interpolatedUV.Y;
            r.refraction_index = material.RefractionIndex;
            r.next_ref_index = n2;
            r.flags = XRT_SURF_HIT | (material.Transparent ? XRT_SURF_TRANSPARENT : 0) | (material.InterpolateNormals ? XRT_SURF_INTERPOLATED : 0) |
                      (material.UseTexture ? XRT_SURF_TEXTURED : 0);
            std::memcpy(&surface_out[i], &r, sizeof(r));
        }
        if (reflect_out || refract_out) {
            const Vector3 Direction = V3(rays[i].d[0], rays[i].d[1], rays[i].d[2]);
            if (reflect_out) {   // RT:547-550
                Ray r;
                r.Position = result.worldPosition;
                r.Direction = Reflect(Direction, fragmentNormal);
                r.Direction = Normalize(r.Direction);
                PutRay(reflect_out[i], r.Position, r.Direction, h.mesh, h.tri);
            }
            if (refract_out) {
                if (material.Transparent) {   // RT:669-694
                    float cos1 = Dot(fragmentNormal, -Direction);
                    double ratio = (double)(n1 / n2);
                    double c1 = (double)cos1;
                    float cos2 = (float)std::sqrt(1 - (ratio * ratio) * (1 - (c1 * c1)));
                    Vector3 refract;
                    if (cos1 >= 0) refract = (n1 / n2) * Direction + ((n1 / n2) * cos1 - cos2) * fragmentNormal;
                    else refract = (n1 / n2) * Direction - ((n1 / n2) * cos1 - cos2) * fragmentNormal;
                    const Vector3 d = Normalize(refract);
                    PutRay(refract_out[i], result.worldPosition, d, h.mesh, h.tri);
                    counts[current_ref_index == material.RefractionIndex ? 4 : 5]++;
                    counts[cos1 >= 0 ? 6 : 7]++;
                    if (std::isnan(d.X) || std::isnan(d.Y) || std::isnan(d.Z)) counts[8]++;
                } else {
                    NullRay(refract_out[i]);
                }
            }
        }
    }
    if (counts_out) for (int k = 0; k < 9; k++) counts_out[k] = counts[k];
    return rt.bad_lookup ? -3 : 0;
}

}  // extern "C"
