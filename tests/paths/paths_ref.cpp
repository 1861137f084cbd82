// TEST INFRASTRUCTURE -- the checker of xrt_cast_rays_paths: RayTracer.CastRay (RT:506-737) of the CPU oracle with the list RayTracer.points
// kept (RT:543, 701, 740-747) and the `ref Ray ray` handed back (RT:692-694).
// The oracle is included unmodified (through the checker of xrt_cast_rays, whose orc_cast_rays this library exports too).  Its CastRay has no
// hook for the list ("does not influence the image and is dropped"), so CastRayPaths below restates that recursion line by line and adds the
// three appends; tests/paths_py.py pins the restatement by asserting that its colours equal orc_cast_rays' bit for bit on every batch.
#include "../castray/castray_ref.cpp"

namespace {

struct PathVertex { float x, y, z; uint32_t color; };   // VertexPositionColor: xrt_path_vertex
struct NodeRec { int64_t ray; int32_t node, kind; float v[3]; };   // kind 0: the node's ray hit at v; 1: refraction child `node` was cast with direction v

struct PathsRun {
    std::vector<PathVertex> points;
    std::vector<int64_t> start;
    std::vector<NodeRec> recs;
    bool tree = false;
    int64_t ray = 0;
} g_run;

const uint32_t kWhite = 0xFFFFFFFFu, kRed = 0xFF0000FFu;   // Color.White / Color.Red in the packing of ColorFromVector3

void AddRayPoints(const Vector3 &p, const Vector3 &q, uint32_t color) {   // RT:740-747
    g_run.points.push_back(PathVertex{p.X, p.Y, p.Z, color});
    g_run.points.push_back(PathVertex{q.X, q.Y, q.Z, color});
}

// `node`: the call's place in the recursion as the library names it -- ray trees: reflection 2i + 1, refraction 2i + 2; chains: the generation
void CastRayPaths(RayTracer &rt, Ray &ray, uint32_t &resultColor, int iteration, const Triangle *origin, float currentRefIndex, Counters &c,
                  Vector3 *colorVectorOut, int node) {
    IntersectionResult result;
    c.rays_closest++;
    if (rt.scene->manager.GetRayIntersection(ray, result, origin, c)) {
        c.hits_closest++;
        c.shaded_hits++;
        const Material &material = result.mesh->MeshMaterial;
        Vector3 fragmentNormal;
        if (material.InterpolateNormals) {
            Vector3 n1 = result.triangle->n2 - result.triangle->n1;
            Vector3 n2 = result.triangle->n3 - result.triangle->n1;
            fragmentNormal = result.triangle->n1 + (n1 * result.u) + (n2 * result.v);
            fragmentNormal = Normalize(fragmentNormal);
        } else {
            fragmentNormal = result.triangle->surfaceNormal;
        }
        Vector3 lightResult = V3(0, 0, 0);
        for (size_t i = 0; i < rt.lights.size(); i++) {
            float lightAmount = rt.IsLightPathObstructed(result, rt.lights[i], c);
            if (lightAmount != 1.0f)
                lightResult = lightResult + rt.lights[i].GetLightForFragment(result.worldPosition, fragmentNormal) * (1.0f - lightAmount);
        }
        AddRayPoints(ray.Position, result.worldPosition, kWhite);   // RT:543
        g_run.recs.push_back(NodeRec{g_run.ray, node, 0, {result.worldPosition.X, result.worldPosition.Y, result.worldPosition.Z}});
        if (iteration < rt.MaxReflections) {
            Ray r;
            r.Position = result.worldPosition;
            r.Direction = Reflect(ray.Direction, fragmentNormal);
            r.Direction = Normalize(r.Direction);
            uint32_t reflectionColor;
            CastRayPaths(rt, r, reflectionColor, iteration + 1, result.triangle, currentRefIndex, c, nullptr, g_run.tree ? 2 * node + 1 : node + 1);
            Vector3 surfaceColor = rt.SurfaceColor(result, material);
            Vector3 colorVector = Lerp(ColorToVector3(reflectionColor), surfaceColor, 1.0f - material.Reflectiveness) * lightResult;
            if (material.Transparent) {
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
                g_run.recs.push_back(NodeRec{g_run.ray, 2 * node + 2, 1, {ray.Direction.X, ray.Direction.Y, ray.Direction.Z}});
                uint32_t refractColor;
                CastRayPaths(rt, ray, refractColor, iteration + 1, result.triangle, n2, c, nullptr, 2 * node + 2);   // RT:698: the same variable
                AddRayPoints(ray.Position, ray.Direction * 100.0f, kRed);   // RT:701: ray as the nested call left it; q is the direction times 100
                colorVector = Lerp(ColorToVector3(refractColor), colorVector, result.triangle->color.W);
            }
            if (colorVectorOut) *colorVectorOut = colorVector;
            resultColor = ColorFromVector3(colorVector);
        } else {
            Vector3 surfaceColor = rt.SurfaceColor(result, material);
            Vector3 colorVector = lightResult * surfaceColor;
            if (colorVectorOut) *colorVectorOut = colorVector;
            resultColor = ColorFromVector3(colorVector);
        }
    } else {
        if (colorVectorOut) *colorVectorOut = V3(0, 0, 0);
        resultColor = ColorFromVector3(V3(0, 0, 0));
    }
}

}  // namespace

extern "C" {

// orc_cast_rays with the list kept: the run's vertices, vertex_start[n + 1] and node records stay in the library until the next run
// (orc_paths_sizes / orc_paths_copy fetch them); rays_back[i] = the ray as the call left it (ignore_* copied).  Returns as orc_cast_rays.
int orc_paths_run(const orc_scene *s, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts, const xrt_ray *rays, int64_t n,
                  int32_t iteration, float ref_index, uint32_t *rgba_out, float *rgb_f32_out, xrt_ray *rays_back, xrt_stats *stats) {
    if (!s->built) return -1;
    RayTracer rt{};
    rt.scene = s;
    for (int i = 0; i < n_lights; i++) rt.lights.push_back(MakeLight(lights[i]));
    rt.MaxReflections = opts->max_reflections;
    rt.AddressMode = opts->address_mode;
    rt.TextureFiltering = opts->filtering;
    bool anyTransparent = false;
    for (const auto &m : s->meshes) anyTransparent = anyTransparent || m->MeshMaterial.Transparent;
    g_run.points.clear(); g_run.start.clear(); g_run.recs.clear();
    g_run.tree = anyTransparent && opts->max_reflections - iteration > 0;   // how the library names the nodes of this pass
    Counters c;
    for (int64_t i = 0; i < n; i++) {
        Ray ray{V3(rays[i].o[0], rays[i].o[1], rays[i].o[2]), V3(rays[i].d[0], rays[i].d[1], rays[i].d[2])};
        uint32_t color = 0;
        Vector3 cv = V3(0, 0, 0);
        g_run.ray = i;
        g_run.start.push_back((int64_t)g_run.points.size());
        CastRayPaths(rt, ray, color, iteration, ResolveIgnore(s, rays[i]), ref_index, c, &cv, 0);
        rgba_out[i] = color;
        if (rgb_f32_out) { rgb_f32_out[3 * i] = cv.X; rgb_f32_out[3 * i + 1] = cv.Y; rgb_f32_out[3 * i + 2] = cv.Z; }
        if (rays_back) {
            rays_back[i] = rays[i];
            rays_back[i].o[0] = ray.Position.X; rays_back[i].o[1] = ray.Position.Y; rays_back[i].o[2] = ray.Position.Z;
            rays_back[i].d[0] = ray.Direction.X; rays_back[i].d[1] = ray.Direction.Y; rays_back[i].d[2] = ray.Direction.Z;
        }
    }
    g_run.start.push_back((int64_t)g_run.points.size());
    FillStats(stats, c, (uint64_t)n, 0);
    return rt.bad_lookup ? -3 : 0;
}

void orc_paths_sizes(int64_t out[3]) { out[0] = (int64_t)g_run.points.size(); out[1] = (int64_t)g_run.recs.size(); out[2] = g_run.tree ? 1 : 0; }

void orc_paths_copy(void *vertices, int64_t *vertex_start, int64_t *rec_ray, int32_t *rec_node, int32_t *rec_kind, float *rec_v) {
    if (!g_run.points.empty()) std::memcpy(vertices, g_run.points.data(), g_run.points.size() * sizeof(PathVertex));
    std::memcpy(vertex_start, g_run.start.data(), g_run.start.size() * sizeof(int64_t));
    for (size_t i = 0; i < g_run.recs.size(); i++) {
        rec_ray[i] = g_run.recs[i].ray; rec_node[i] = g_run.recs[i].node; rec_kind[i] = g_run.recs[i].kind;
        std::memcpy(rec_v + 3 * i, g_run.recs[i].v, 3 * sizeof(float));
    }
}

}  // extern "C"
