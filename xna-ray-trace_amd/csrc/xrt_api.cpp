// xrt_api.cpp — the C-ABI of include/xrt.h: scene upload, HBM residency, and the per-frame wavefront
// schedule that replaces the body of RayTracer.RenderInternal (RT:105-120).  Compiled by hipcc (host side
// uses the HIP runtime API); all arithmetic of the path runs in kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/xrt.h"
#include "device_res.h"    // the owners of device resources, fail / HIPCHECK, the XRT_GUARD registry, roctx ranges

using namespace xrt;

#include "scene_state.h"   // xrt_scene and its parts (global, as include/xrt.h declares it; its members' types are xrt's)
#include "pixels.h"        // xrt_render_pixels: the list kernels (pixels.hip) ...
#include "pixels_plan.h"   // ... and how a list is split into chunks
#include "hits.h"          // xrt_shade_hits: generation 0 from a caller's hits (hits.hip)
#include "lights.h"        // xrt_light_hits: the light loop on a caller's hits (lights.hip) ...
#include "lights_plan.h"   // ... and how a list is split into chunks
#include "trace.h"         // xrt_trace_pixels: rays and closest hits of a centre list (trace.hip) ...
#include "trace_plan.h"    // ... and how a list is split into chunks
#include "surface.h"       // xrt_surface_hits: surface terms and next rays of a caller's hits (surface.hip)
#include "compose.h"       // xrt_compose_hits: CastRay's return path on a caller's terms (compose.hip)
#include "screen_rects.h"  // the screen boxes of a camera frame's primary packets (screen_rects.hip)

namespace {

bool in_flight(const xrt_scene *s) {
    if (s->busy.load()) return true;
    for (const auto &f : s->frames) if (f.pending) return true;
    return false;
}

int need_device(xrt_scene *s, const char *fn) {
    if (!s) return fail(XRT_E_INVALID_ARG, "%s: null scene", fn);
    if (s->device < 0) return fail(XRT_E_NO_DEVICE, "%s: host-only scene (created with device -1); libxrt has no CPU execution path", fn);
    if (!s->host->built || !s->resident) return fail(XRT_E_NOT_BUILT, "%s: call xrt_scene_build first", fn);
    HIPCHECK(hipSetDevice(s->device));
    return XRT_OK;
}

hipEvent_t get_event(std::vector<Event> &pool, size_t i) {
    while (pool.size() <= i) {
        Event e;
        if (hipEventCreate(&e.h) != hipSuccess) return nullptr;
        pool.push_back(std::move(e));
    }
    return pool[i];
}
hipEvent_t get_event(xrt_scene *s, size_t i) { return get_event(s->events, i); }

// ---- pose versions (xrt_scene_set_poses) ---------------------------------------------------------------------------------
ObjRec *pose_objects(xrt_scene *s, int v) { return v == 0 ? s->objects.p : s->pose[v].objects.p; }
f4 *pose_scull(xrt_scene *s, int v) { return v == 0 ? s->scull.p : s->pose[v].scull.p; }
SceneView pose_view(xrt_scene *s, int v) {
    SceneView S = s->view;
    S.objects = pose_objects(s, v); S.scull = pose_scull(s, v);
    return S;
}
// Work on `st` that reads version v starts after the version's last write.
int pose_wait(xrt_scene *s, int v, hipStream_t st) {
    if (s->pose[v].ready) HIPCHECK(hipStreamWaitEvent(st, s->pose[v].ready, 0));
    return XRT_OK;
}
// An asynchronous read of version v on `st` was enqueued: the next write of v waits for it.
int pose_reader(xrt_scene *s, int v, hipStream_t st) {
    auto &rd = s->pose[v].readers;
    size_t i = 0;
    while (i < rd.size() && rd[i].first != st) i++;
    if (i == rd.size()) {
        Event e;
        if (int rc = e.create()) return rc;
        rd.emplace_back(st, std::move(e));
    }
    HIPCHECK(hipEventRecord(rd[i].second, st));
    return XRT_OK;
}
bool pose_referenced(const xrt_scene *s, int v) { return s->slotPose[0] == v || s->slotPose[1] == v; }

// ---- material versions (xrt_scene_set_materials) ---------------------------------------------------------------------------
DevBuf<MaterialRec> &mat_records(xrt_scene *s, int v) { return v == 0 ? s->materials : s->mat[v].materials; }
DevBuf<uint32_t> &mat_texels(xrt_scene *s, int v) { return v == 0 ? s->texels : s->mat[v].texels; }
// Work enqueued on `st` after this call may read version v.  The first reader of a staged write enqueues its copies on `st` itself (they
// are ahead of whatever it enqueues next) and records the version's event behind them; a reader on another stream waits for that event.
int mat_acquire(xrt_scene *s, int v, hipStream_t st) {
    xrt_scene::MatVer &M = s->mat[v];
    if (M.pending) {
        const char *src = (const char *)M.staging.p;
        HIPCHECK(hipMemcpyAsync(mat_records(s, v).p, src, M.stagedMat * sizeof(MaterialRec), hipMemcpyHostToDevice, st));
        if (M.stagedHi > M.stagedLo)
            HIPCHECK(hipMemcpyAsync(mat_texels(s, v).p + M.stagedLo, src + M.stagedRecBytes, (M.stagedHi - M.stagedLo) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (int rc = M.ready.create()) return rc;
        HIPCHECK(hipEventRecord(M.ready, st));
        M.owner = st;
        M.pending = false;
        return XRT_OK;
    }
    if (M.ready && M.owner != st) HIPCHECK(hipStreamWaitEvent(st, M.ready, 0));
    return XRT_OK;
}
bool mat_referenced(const xrt_scene *s, int v) { return s->slotMat[0] == v || s->slotMat[1] == v; }
// Room for n texels in b.  An arena that is outgrown is set aside, not freed: hipFree would wait for the frames in flight.
int mat_texel_room(xrt_scene *s, DevBuf<uint32_t> &b, size_t n) {
    if (b.p && n <= b.cap) return XRT_OK;
    DevBuf<uint32_t> fresh;
    if (int rc = fresh.ensure(n + n / 2)) return rc;   // (half as much again: textures whose size changes a little do not allocate every time)
    std::swap(b, fresh);
    if (fresh.p) s->matRetired.push_back(std::move(fresh));
    return XRT_OK;
}

// ---- triangle-shading versions (xrt_scene_set_triangle_shading) ------------------------------------------------------------
DevBuf<f4> &shade_records(xrt_scene *s, int v) { return v == 0 ? s->shade : s->shadeVer[v].shade; }
// What a shading kernel reads of the scene, with the materials of version mv and the triangle values of version sv (the lights and the texture lookup are the call's).
ShadeView shade_view(xrt_scene *s, int mv, int sv) {
    ShadeView V;
    V.shade = shade_records(s, sv).p; V.materials = mat_records(s, mv).p; V.texels = mat_texels(s, mv).p; V.meshes = s->meshes.p;
    V.lights = nullptr; V.nLights = 0; V.addressMode = XRT_ADDRESS_WRAP; V.filtering = XRT_FILTER_POINT;
    return V;
}
// Work on `st` that reads version v starts after the version's last write (no event: the version holds what the upload left).
int shade_wait(xrt_scene *s, int v, hipStream_t st) {
    if (s->shadeVer[v].ready) HIPCHECK(hipStreamWaitEvent(st, s->shadeVer[v].ready, 0));
    return XRT_OK;
}
bool shade_referenced(const xrt_scene *s, int v) { return s->slotShade[0] == v || s->slotShade[1] == v; }
// The versions start again from version 0, which holds the host's records (scene->shade was just uploaded).
void shade_restart(xrt_scene *scene) {
    for (auto &v : scene->shadeVer) { v.ready.reset(); v.serial = 0; }
    scene->shadeCur = 0; scene->shadeSerial = 0; scene->shadeOnDevice = false;
    scene->shadeCount = scene->host->arrays.shade.size();
}

int persistent_grid(xrt_scene *s, long long nHost, int raysPerBlock = 256) {
    int full = s->numCUs * s->blocksPerCU;
    if (nHost >= 0) {
        long long want = (nHost + raysPerBlock - 1) / raysPerBlock;   // one block covers >= 256 rays (16 for a guessed size: small launches are spread thin)
        if (want < 1) want = 1;
        if (want < full) return (int)want;
    }
    return full;
}

// Every light is of a kind the kernels know (fn: the entry point the message names, or null).
int lights_known(const char *fn, const xrt_light *lights, int n) {
    for (int i = 0; i < n; i++)
        if (lights[i].kind != XRT_LIGHT_SPOT && lights[i].kind != XRT_LIGHT_DIRECTIONAL)
            return fn ? fail(XRT_E_INVALID_ARG, "%s: unknown light kind", fn) : fail(XRT_E_INVALID_ARG, "unknown light kind");
    return XRT_OK;
}

// The scheduling knobs of a k_intersect launch: the scene's where it derives them (scene_upload), else the switches'.
void set_knobs(IntersectArgs &a, const xrt_scene *s) {
    a.refillMin = s->refillMin; a.nodeBurst = s->cfg.tune[1]; a.leafBurst = s->cfg.tune[2]; a.coopMax = s->cfg.tune[3];
    a.batchMax = s->cfg.batchMax; a.batchMin = s->cfg.batchMin; a.spreadMin = s->cfg.spreadMin; a.heavyShift = s->heavyShift; a.firstBatch = s->firstBatch;
}

// The wave-packet launch of the population(s) a per-lane launch would trace (I2: a second segment for the same launch, or null; quads: the packet table written for
// the first segment, or null): the one place that knows which fields the two argument structs share.  The packet heads sit behind the per-lane head of the launch's
// queue words.  Tile costs, the split arena and the timing stay with the caller.
PacketArgs packet_args(const xrt_scene *s, const IntersectArgs &I, const IntersectArgs *I2 = nullptr, const QuadTable *quads = nullptr) {
    PacketArgs PA;
    PA.rays = I.rays; PA.hits = I.hits; PA.flags = I.flags; PA.index = I.index; PA.nDev = I.nDev; PA.nMul = I.nMul; PA.n = I.n; PA.nCap = I.nCap; PA.scatter = I.scatter;
    if (I2) { PA.rays2 = I2->rays; PA.hits2 = I2->hits; PA.flags2 = I2->flags; PA.nDev2 = I2->nDev; PA.nMul2 = I2->nMul; PA.nCap2 = I2->nCap; PA.scatter2 = I2->scatter; }
    if (quads && quads->table) { PA.pkTable = quads->table; PA.pkCount = quads->count; PA.pkCap = quads->cap; }
    PA.queue = I.queue + 1; PA.mode = I.mode; PA.meshId = I.meshId; PA.unmark = 0;
    PA.staticDiv = s->cfg.packetStaticDiv; PA.grabMax = s->cfg.packetGrabMax; PA.cullMin = s->cfg.packetCullMin;
    return PA;
}

// ... and its grid: every CU filled, or one block per 256 rays where the host knows (a bound of) their number (nHost >= 0).
int packet_grid(const xrt_scene *s, int blocksPerCU, long long nHost) {
    const int full = s->numCUs * blocksPerCU;
    if (nHost < 0) return full;
    const long long want = std::max(1LL, (nHost + 255) / 256);
    return want < full ? (int)want : full;
}

void fill_stats(xrt_stats *st, const unsigned long long *c /* 2*C_COUNT: closest, shadow */, unsigned long long shaded, unsigned long long pixels) {
    const unsigned long long *a = c, *b = c + C_COUNT;
    st->rays_closest = a[C_RAYS]; st->rays_shadow = b[C_RAYS];
    st->hits_closest = a[C_HITS]; st->hits_shadow = b[C_HITS];
    st->scene_node_tests = a[C_SCENE_NODES] + b[C_SCENE_NODES];
    st->instance_visits = a[C_INSTANCES] + b[C_INSTANCES];
    st->mesh_aabb_tests = a[C_MESH_AABB] + b[C_MESH_AABB];
    st->mesh_queries = a[C_MESH_QUERIES] + b[C_MESH_QUERIES];
    st->mesh_queries_facing_away = a[C_MESH_AWAY] + b[C_MESH_AWAY];
    st->node_tests = a[C_NODES] + b[C_NODES];
    st->leaf_refs = a[C_REFS] + b[C_REFS];
    st->tri_tests = a[C_TRIS] + b[C_TRIS];
    st->shaded_hits = shaded;
    st->pixels = pixels;
    // per query 32 (ray in) + 48 (hit out) + 32 N_node + 4 N_ref + 48 N_tri, two-level terms
    // 32 N_scene_node + 64 N_instance + 24 N_mesh_aabb + 64 per hit (World); shading 76 + 4 per shaded hit; 4 per pixel.
    unsigned long long rays = st->rays_closest + st->rays_shadow, hits = st->hits_closest + st->hits_shadow;
    st->algorithmic_bytes = rays * 80ull + 32ull * st->node_tests + 4ull * st->leaf_refs + 48ull * st->tri_tests +
                            32ull * st->scene_node_tests + 64ull * st->instance_visits + 24ull * st->mesh_aabb_tests + 64ull * hits +
                            80ull * st->shaded_hits + 4ull * pixels;
}

LightRec make_light(const xrt_light &l) {
    LightRec r;
    std::memset(&r, 0, sizeof(r));
    r.kind = l.kind;
    r.px = l.position[0]; r.py = l.position[1]; r.pz = l.position[2];
    r.dx = l.direction[0]; r.dy = l.direction[1]; r.dz = l.direction[2];
    r.cr = l.color[0]; r.cg = l.color[1]; r.cb = l.color[2];
    r.intensity = l.intensity;
    r.angleCosine = (float)std::cos((double)(l.spot_angle * 0.5f));                        // SPOT:25
    r.decayDenom = std::pow((double)(1 - r.angleCosine), (double)l.decay_exponent);        // SPOT:54, constant per light
    if (l.kind == XRT_LIGHT_DIRECTIONAL) { r.px = r.py = r.pz = 0.0f; }                     // DIR:14
    return r;
}

// ---- cost-aware tile assignment (xrt.h) ------------------------------------------------------------------------------------------
// Longest-processing-time-first: tiles in descending order of cost (ties: ascending tile number), each to the rank with the least cost so
// far that still has a free slot (ties: the lowest rank); a rank's slots are filled in that order.  Costs that are not
// positive finite numbers count as the smallest positive cost seen (a tile nobody measured still takes a slot's worth of launch overhead).
int balance_tiles_impl(int tiles, int count, const float *cost, int tpr, int *out) {
    if (tiles <= 0 || count <= 0 || tpr <= 0 || !out) return fail(XRT_E_INVALID_ARG, "xrt_balance_tiles: bad argument");
    if ((long long)tpr * count < tiles) return fail(XRT_E_INVALID_ARG, "xrt_balance_tiles: %d slots per rank x %d ranks do not hold %d tiles", tpr, count, tiles);
    std::fill(out, out + (size_t)count * tpr, -1);
    double lowest = 0.0;
    bool any = false;
    if (cost)
        for (int t = 0; t < tiles; t++)
            if (cost[t] > 0.0f && cost[t] < 3.0e38f) { if (!any || cost[t] < lowest) lowest = cost[t]; any = true; }
    if (!any) {   // no measurement: the round-robin layout of xrt_shard_layout
        for (int t = 0; t < tiles; t++) out[(size_t)(t % count) * tpr + t / count] = t;
        return XRT_OK;
    }
    std::vector<int> order((size_t)tiles);
    std::vector<double> c((size_t)tiles);
    for (int t = 0; t < tiles; t++) { order[(size_t)t] = t; c[(size_t)t] = (cost[t] > 0.0f && cost[t] < 3.0e38f) ? (double)cost[t] : lowest; }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b2) { return c[(size_t)a] > c[(size_t)b2]; });
    std::vector<double> load((size_t)count, 0.0);
    std::vector<std::vector<int>> mine((size_t)count);
    for (int t : order) {
        int best = -1;
        for (int r = 0; r < count; r++)
            if ((int)mine[(size_t)r].size() < tpr && (best < 0 || load[(size_t)r] < load[(size_t)best])) best = r;
        mine[(size_t)best].push_back(t);
        load[(size_t)best] += c[(size_t)t];
    }
    // A rank's slots in the order its tiles were dealt -- descending cost: its launches start with their longest packets.  (A launch ends when
    // its slowest packet does, and a packet of rays that skim the terrain near the horizon takes a hundred times the median: in ascending
    // tile order such packets started wherever their rows fell, and the shards of a frame that were unlucky took up to twice as long as the
    // others whatever their cost sums.)
    for (int r = 0; r < count; r++)
        for (size_t k = 0; k < mine[(size_t)r].size(); k++) out[(size_t)r * tpr + k] = mine[(size_t)r][k];
    return XRT_OK;
}

// Every tile exactly once?
int check_tile_table(int tiles, int count, int tpr, const int *table) {
    if (tpr <= 0 || (long long)tpr * count < tiles) return fail(XRT_E_INVALID_ARG, "tile table: %d slots per rank x %d ranks do not hold %d tiles", tpr, count, tiles);
    std::vector<char> seen((size_t)tiles, 0);
    for (size_t i = 0; i < (size_t)count * tpr; i++) {
        const int t = table[i];
        if (t == -1) continue;
        if (t < 0 || t >= tiles) return fail(XRT_E_INVALID_ARG, "tile table: entry %zu names tile %d of %d", i, t, tiles);
        if (seen[(size_t)t]) return fail(XRT_E_INVALID_ARG, "tile table: tile %d appears twice", t);
        seen[(size_t)t] = 1;
    }
    for (int t = 0; t < tiles; t++) if (!seen[(size_t)t]) return fail(XRT_E_INVALID_ARG, "tile table: tile %d is missing", t);
    return XRT_OK;
}

int make_raygen(const xrt_camera *cam, const xrt_render_opts *o, RayGenParams &g, const float *rootBox = nullptr /* min xyz, max xyz; null: no screen-rectangle cull */) {
    if (cam->vp_width <= 0 || cam->vp_height <= 0) return fail(XRT_E_INVALID_ARG, "viewport must be positive");
    float wv[16], wvp[16], ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mat_multiply(ident, cam->view, wv);     // Matrix.Multiply(world = Identity, view)   (Viewport.Unproject, RT:415)
    mat_multiply(wv, cam->proj, wvp);       // Matrix.Multiply(.., projection)
    mat_invert(wvp, g.m);                   // Matrix.Invert
    g.vpX = (float)cam->vp_x; g.vpY = (float)cam->vp_y; g.vpW = (float)cam->vp_width; g.vpH = (float)cam->vp_height;
    g.minDepth = cam->vp_min_depth; g.depthRange = cam->vp_max_depth - cam->vp_min_depth;
    g.width = cam->vp_width; g.height = cam->vp_height;
    g.tilesX = (g.width + XRT_TILE_W - 1) / XRT_TILE_W; g.tilesY = (g.height + XRT_TILE_H - 1) / XRT_TILE_H;
    g.shardCount = o->shard_count > 1 ? o->shard_count : 1;
    g.shardRank = o->shard_count > 1 ? o->shard_rank : 0;
    g.samples = (o->use_multisampling == XRT_MS_FIXED16) ? 16 : 1;
    g.quadLevel = -1; g.quadCx = nullptr; g.quadCy = nullptr; g.quadSize = 1.0f;
    g.cullX0 = 0; g.cullY0 = 0; g.cullX1 = g.width - 1; g.cullY1 = g.height - 1;
    g.cullSkipsRecord = 0;
    g.pathsDev = nullptr; g.pathsMul = 1; g.pathsCap = 0;
    g.tileOfSlot = nullptr;
    g.batch = nullptr; g.batchRef = nullptr; g.batchRefIndex = 1.0f;
    if (g.shardRank < 0 || g.shardRank >= g.shardCount) return fail(XRT_E_INVALID_ARG, "shard_rank out of range");
    if (rootBox) {
        // Screen rectangle of the scene's root box.  A ray through pixel (x, y) that reaches the box at a point P has P
        // projecting onto (x, y); the box is convex, so with all eight corners in front of the eye every such pixel lies
        // inside the corners' bounding rectangle.  Evaluated in double from the same float matrices; used only when
        // every corner has a clearly positive w and comes back through the inverse matrix k_raygen uses (its pixel and
        // depth unprojected again) to within a thousandth of the box diagonal.
        bool ok = true;
        double x0 = 1e300, y0 = 1e300, x1 = -1e300, y1 = -1e300;
        for (int c = 0; c < 8 && ok; c++) {
            const double p[3] = {rootBox[(c & 1) ? 3 : 0], rootBox[(c & 2) ? 4 : 1], rootBox[(c & 4) ? 5 : 2]};
            double v[4];
            for (int j = 0; j < 4; j++) v[j] = p[0] * wvp[j] + p[1] * wvp[4 + j] + p[2] * wvp[8 + j] + wvp[12 + j];
            const double scale = std::fabs(v[0]) + std::fabs(v[1]) + std::fabs(v[2]) + std::fabs(v[3]);
            if (!(v[3] > 1e-3 * scale) || !(scale < 1e30)) { ok = false; break; }
            const double sx = (v[0] / v[3] + 1.0) * 0.5 * g.vpW + g.vpX, sy = (1.0 - v[1] / v[3]) * 0.5 * g.vpH + g.vpY;
            {   // round trip through g.m
                const double n[4] = {v[0] / v[3], v[1] / v[3], v[2] / v[3], 1.0};
                double u[4];
                for (int j = 0; j < 4; j++) u[j] = n[0] * g.m[j] + n[1] * g.m[4 + j] + n[2] * g.m[8 + j] + g.m[12 + j];
                const double ddx = rootBox[3] - (double)rootBox[0], ddy = rootBox[4] - (double)rootBox[1], ddz = rootBox[5] - (double)rootBox[2];
                const double tol = 1e-3 * std::sqrt(ddx * ddx + ddy * ddy + ddz * ddz);
                if (!(std::fabs(u[3]) > 1e-30) || !(std::fabs(u[0] / u[3] - p[0]) <= tol && std::fabs(u[1] / u[3] - p[1]) <= tol && std::fabs(u[2] / u[3] - p[2]) <= tol)) { ok = false; break; }
            }
            x0 = std::min(x0, sx); x1 = std::max(x1, sx); y0 = std::min(y0, sy); y1 = std::max(y1, sy);
        }
        if (ok && x0 <= x1 && y0 <= y1) {
            const double mx = 2.0 + 1e-3 * g.vpW, my = 2.0 + 1e-3 * g.vpH;
            // (k_raygen's pixel coordinates are the screen coordinates Viewport.Unproject is given, RT:415)
            const double fx0 = std::floor(x0 - mx), fy0 = std::floor(y0 - my), fx1 = std::ceil(x1 + mx), fy1 = std::ceil(y1 + my);
            g.cullX0 = (int)std::max(0.0, std::min(fx0, (double)g.width)); g.cullY0 = (int)std::max(0.0, std::min(fy0, (double)g.height));
            g.cullX1 = (int)std::min((double)g.width - 1, std::max(fx1, -1.0)); g.cullY1 = (int)std::min((double)g.height - 1, std::max(fy1, -1.0));
        }
    }
    return XRT_OK;
}

// Tile of slot `sl` of the plan's rank: the installed table's, or the round-robin layout's.
long long tile_of_slot(const xrt_scene &s, const FramePlan &P, long long sl) {
    return P.tabled ? (long long)s.tileTable[(size_t)P.g.shardRank * s.tableTpr + (size_t)sl] : shard_tile(sl, P.g.shardRank, P.g.shardCount, P.g.tilesX);
}

}  // namespace

// The packet mask of a plain (no ray tree) frame or coherent list of `samples` rays per screen position: XRT_PACKET where it is set; else two-level scenes take
// packets at any sample count and in every generation, one-body scenes with 16 sub-rays alone and in the first two generations (the measurements: plan_frame).
// The ONE statement of that rule: plan_frame and the list calls that trace outside a frame (xrt_trace_pixels, xrt_light_hits) read it here.
int scene_packet_mask(const xrt_scene &s, int samples) {
    return !s.packetOk ? 0 : (s.cfg.packetMask >= 0 ? s.cfg.packetMask : (s.sceneMode == MODE_SCENE ? 23 : (samples >= 16 ? 7 : 0)));
}

// The scene's part of "answered at emission" (kernels.h ShadeArgs::ae): one body with one mesh that CAN face away from a ray as a whole -- its normal box or its
// diagonal box does not hold the origin (a fan of normals 50 degrees to either side of (1, 1, 0) holds 0 in every axis interval, not in that of N_x + N_y).
bool scene_answers_at_emission(const xrt_scene &s) {
    return s.sceneMode == MODE_SINGLE && s.view.nodeCull != 0 && s.cfg.answerAtEmission && mesh_can_face_away(s.host->arrays.meshes[0]);
}

// The frame: for every chunk of paths  raygen -> [intersect(closest k + shadow k-1) -> shade(A: k, B: k-1)] x (R+2) -> compose,
// then resolve (pixel grid, fixed 16 sub-rays) or the quadrant levels of adaptive supersampling (RT:170-311).
// plan_frame decides all of it -- which pipeline, which shortcuts, every size -- from the scene's host state and the call's arguments (frame_plan.h).
// batch != null: the paths are the batch's rays instead of the camera's pixels (cam is not read): one sample each, path p = ray p, no tiles,
// no screen rectangle, no level map.  Such a pass takes the careful way (!fast): its counters are read back per chunk, a ray tree is checked
// for overflow and retried chunk by chunk.
int plan_frame(const xrt_scene &s, int matVersion, const xrt_camera *cam, const xrt_light *lights, int nLights, const xrt_render_opts *opts, bool wantsF32,
               bool hasStream, int part, int nParts, bool heapFastAllowed, const BatchSrc *batch, FramePlan &plan) {
    if ((!cam && !batch) || !opts || (!lights && nLights > 0) || nLights < 0) return fail(XRT_E_INVALID_ARG, "xrt_render: null argument");
    if (opts->max_reflections < 0 || opts->max_reflections > 64) return fail(XRT_E_INVALID_ARG, "max_reflections out of range");
    if (opts->address_mode < XRT_ADDRESS_CLAMP || opts->address_mode > XRT_ADDRESS_MIRROR)
        return fail(XRT_E_INVALID_ARG, "Value does not fall within the expected range: addressMode (MAT:85)");
    if (opts->filtering != XRT_FILTER_POINT && opts->filtering != XRT_FILTER_BILINEAR)
        return fail(XRT_E_INVALID_ARG, "Value does not fall within the expected range: filtering (MAT:97)");
    FramePlan p;
    RayGenParams &g = p.g;
    p.addressMode = opts->address_mode; p.filtering = opts->filtering;
    p.heap = s.mat[matVersion].anyTransparent && opts->max_reflections > 0;   // RT:586-702: binary ray tree (by the materials of the frame's version)
    const bool heap = p.heap;
    if (heap && opts->max_reflections > 12)
        return fail(XRT_E_UNSUPPORTED, "Transparent materials with MaxReflections > 12 (a ray tree of more than 8191 nodes per pixel)");
    const int msMode = opts->use_multisampling;
    if (msMode != XRT_MS_OFF && msMode != XRT_MS_FIXED16 && msMode != XRT_MS_ADAPTIVE) return fail(XRT_E_INVALID_ARG, "use_multisampling");
    p.adaptive = msMode == XRT_MS_ADAPTIVE;
    const bool adaptive = p.adaptive;
    p.quality = adaptive ? opts->multisample_quality : 0;
    if (adaptive && (p.quality < 0 || p.quality > 6)) return fail(XRT_E_UNSUPPORTED, "MultisampleQuality above 6 (4^7 sub-quadrants per pixel)");
    p.batch = batch != nullptr;
    p.capturePaths = batch && batch->paths;   // the pass also records its ray paths (paths.hip)
    p.givenHits = batch && batch->hits;       // generation 0 arrives answered (hits.hip)
    if (p.givenHits && p.capturePaths) return fail(XRT_E_INTERNAL, "a batch of given hits records no ray paths");
    p.collect = opts->collect_stats != 0;
    float rootBox[6] = {0, 0, 0, 0, 0, 0};
    const bool haveRoot = s.host->arrays.snodes.size() >= 2;
    if (haveRoot) {
        const f4 lo = s.host->arrays.snodes[0], hi = s.host->arrays.snodes[1];
        rootBox[0] = lo.x; rootBox[1] = lo.y; rootBox[2] = lo.z; rootBox[3] = hi.x; rootBox[4] = hi.y; rootBox[5] = hi.z;
    }
    if (batch) {   // a ray list: one row of n "pixels", every path has its record (nothing is culled by a screen rectangle)
        if (adaptive || msMode != XRT_MS_OFF || opts->shard_count > 1 || nParts > 1 || batch->n <= 0 || batch->n > 0x7fffffff / 2)
            return fail(XRT_E_INTERNAL, "a ray batch is a plain pass of 1 .. 2^30 rays");
        std::memset(&g, 0, sizeof(g));
        g.width = (int)batch->n; g.height = 1; g.tilesX = (g.width + XRT_TILE_W - 1) / XRT_TILE_W; g.tilesY = 1;
        g.shardCount = 1; g.samples = 1; g.quadLevel = -1; g.quadSize = 1.0f; g.pathsMul = 1;
        g.cullX1 = g.width - 1;
        g.batch = reinterpret_cast<const f4 *>(batch->rays); g.batchRefIndex = batch->refIndex;
    } else {
        if (int rc = make_raygen(cam, opts, g, (haveRoot && !s.cfg.noRectCull) ? rootBox : nullptr)) return rc;
        if (adaptive) g.samples = 4;
        g.cullSkipsRecord = heap ? 0 : 1;   // (k_compose_tree reads every root record)
    }
    const int R = p.R = opts->max_reflections;
    const int nL = p.nL = nLights;
    p.totalTiles = (long long)g.tilesX * g.tilesY;
    // an installed tile table for this frame geometry replaces the round-robin layout (xrt.h xrt_scene_set_tile_table)
    p.tabled = !batch && !s.tileTable.empty() && s.tableW == g.width && s.tableH == g.height && s.tableCount == g.shardCount;
    g.tileOfSlot = p.tabled ? s.tileTableDev.p + (size_t)g.shardRank * s.tableTpr : nullptr;
    p.myTiles = p.tabled ? s.tableTpr : shard_tiles_per_rank(p.totalTiles, g.shardCount, g.tilesX);   // tiles_per_rank (slots, some may be past the end)
    p.totalPixels = p.myTiles * 512;
    if (adaptive && p.totalPixels * 4 > 0x7fffffffLL) return fail(XRT_E_UNSUPPORTED, "frame too large for adaptive supersampling");
    p.framePaths = batch ? batch->n : p.totalPixels * g.samples;   // the whole frame (this shard)
    // part `part` of `nParts`: a contiguous range of the frame's paths (whole tiles), rendered by its own frame context
    const long long partStride = nParts > 1 ? ((p.framePaths / nParts + 8191) / 8192) * 8192 : p.framePaths;
    p.partStart = (long long)part * partStride;
    p.firstPaths = nParts > 1 ? std::max(0LL, std::min(partStride, p.framePaths - p.partStart)) : p.framePaths;
    const long long firstPaths = p.firstPaths;
    if (nParts > 1 && (adaptive || firstPaths <= 0)) return fail(XRT_E_INTERNAL, "frame parts need a plain frame");
    p.hintPaths = (nParts == 1 && !adaptive) ? firstPaths : -1;
    // Chunking.  Without refraction a path owns one ray per generation.  With Transparent materials it may own up to
    // 2^k in generation k, but few paths do: chunks are sized optimistically (ray buffers of HEAP_RAY_CAP rays,
    // level records bounded by 8 GB) and a chunk whose generation overflows is retried with a quarter of the paths.
    p.nodes = heap ? (((size_t)1 << (R + 1)) - 1) : (size_t)(R + 1);
    long long maxPaths = s.cfg.maxChunkPaths;
    // The reference iterates a List<ILight> of any length (RT:534-542).  The shadow rays of one generation are counted in an int
    // (at most 2^30): many lights shrink the chunk, they are not refused -- until not even 8192 paths fit a generation.
    const long long lightBound = (1LL << 30) / (nL > 0 ? nL : 1);
    if (maxPaths > lightBound) maxPaths = lightBound & ~8191LL;
    // ... and in bytes: shadow rays, hits and hit / miss words are 84 bytes per path and light in each frame context.  Many lights shrink
    // the chunk to what XRT_SHADOW_BYTES (default 8 GB per context) holds -- the frame then takes the multi-chunk path -- instead of
    // failing with XRT_E_OOM (a 1080p frame with 100 lights would want 17 GB).
    if (nL > 0) {
        const long long byBytes = ((long long)s.cfg.shadowBytes / (84LL * nL)) & ~8191LL;
        if (byBytes < maxPaths) maxPaths = byBytes < 8192 ? 8192 : byBytes;
    }
    if (maxPaths < 8192) return fail(XRT_E_UNSUPPORTED, "%d lights: the shadow rays of 8192 paths do not fit one generation (2^30 rays)", nL);
    if (heap) {
        if (maxPaths > (1 << 21)) maxPaths = 1 << 21;   // (a 1080p frame is one chunk when the level records fit 8 GB: MaxReflections <= 6)
        const long long byRecords = (long long)((8ull << 30) / (p.nodes * 36ull));
        if (byRecords < maxPaths) maxPaths = byRecords;
        maxPaths &= ~63LL;
        if (maxPaths < 64) maxPaths = 64;
    }
    p.chunkPaths = firstPaths < maxPaths ? firstPaths : maxPaths;
    const bool oneChunk = firstPaths <= p.chunkPaths;
    p.P = (int)p.chunkPaths;
    p.rayCap = (size_t)p.P;
    p.liveCap = (size_t)p.P;
    // The per-ray arrays hold LIVE rays only (k_raygen compacts them): a live primary ray belongs to a pixel inside the screen rectangle
    // of the scene's root box, so a plain or 16-sub-ray frame of one chunk needs room for the rectangle's paths, not for every path
    // (C5: 52 % of the image); later generations have fewer rays than the one before.  (Adaptive frames: the deeper quadrant levels are
    // lists of up to a quadrant per pixel; ray trees: sized below.)
    if (!heap && !adaptive && !batch && oneChunk) {
        const long long rectPaths = (long long)std::max(0, g.cullX1 - g.cullX0 + 1) * (long long)std::max(0, g.cullY1 - g.cullY0 + 1) * g.samples + 64;
        if (rectPaths < (long long)p.rayCap) { p.rayCap = (size_t)rectPaths; p.liveCap = p.rayCap; }
    }
    // ... and the two per-level records (16 bytes each per path and level: the largest arrays of a frame) exist only for the TILES that overlap the rectangle (xrt_core.h
    // LvlMap): plain unsharded frames of one chunk and one part, whose tiles are numbered row by row.  (C5: 3.2 -> 1.7 GB per frame context.)
    p.lvlStride = (size_t)p.P;
    std::memset(&g.lvl, 0, sizeof(g.lvl));
    if (!heap && !adaptive && oneChunk && nParts == 1 && p.partStart == 0 && g.shardCount == 1 && !p.tabled && g.cullSkipsRecord && s.cfg.levelMap &&
        g.cullX1 >= g.cullX0 && g.cullY1 >= g.cullY0) {
        const int shift = 9 + (g.samples == 16 ? 4 : (g.samples == 4 ? 2 : 0));
        const int tx0 = g.cullX0 / XRT_TILE_W, tx1 = g.cullX1 / XRT_TILE_W, ty0 = g.cullY0 / XRT_TILE_H, ty1 = g.cullY1 / XRT_TILE_H;
        const long long kept = (long long)(tx1 - tx0 + 1) * (ty1 - ty0 + 1);
        if (kept < p.totalTiles && (kept << shift) < (long long)p.P) {
            const unsigned inv = (unsigned)(((1ULL << 32) + (unsigned)g.tilesX - 1) / (unsigned)g.tilesX);
            bool exact = p.totalTiles < (1LL << 24);
            if (exact && !(s.lvlCheckedTilesX == g.tilesX && s.lvlCheckedTiles >= p.totalTiles)) {   // (checked once per frame geometry: the caller keeps the memo)
                for (long long t = 0; exact && t < p.totalTiles; t++) exact = (unsigned)(((unsigned long long)t * inv) >> 32) == (unsigned)(t / g.tilesX);
                p.lvlVerified = exact;
            }
            if (exact) {
                g.lvl.on = 1; g.lvl.tilesX = g.tilesX; g.lvl.tx0 = tx0; g.lvl.ty0 = ty0; g.lvl.rw = tx1 - tx0 + 1; g.lvl.shift = shift; g.lvl.inv = inv;
                p.lvlStride = (size_t)(kept << shift);
            }
        }
    }
    if (heap) {
        const size_t capL = (size_t)std::min<long long>(s.cfg.heapRayCap, lightBound);   // (>= 8192 >= ... see above; P <= lightBound as well)
        p.rayCap = (R < 20 && ((size_t)p.P << R) < capL) ? ((size_t)p.P << R) : capL;
        if (p.rayCap < (size_t)p.P) p.rayCap = (size_t)p.P;
    }
    if ((unsigned long long)p.rayCap * (unsigned long long)(nL > 0 ? nL : 1) > (1ull << 30)) return fail(XRT_E_UNSUPPORTED, "frame too large: %zu rays x %d lights per generation", p.rayCap, nL);
    p.shadowCap = p.rayCap;   // hits of one generation (each emits nL shadow rays)
    p.wantF32 = wantsF32 && !adaptive && g.samples == 1;
    p.cntStride = 5 * (R + 2);   // per chunk: cnt[R+2], scnt[R+2], the long-ray list lengths [R+2], the shadow rays really emitted [R+2] (ShadeArgs::ae),
                                 // the hits that took no slot [R+2] (ShadeArgs::finish; hits of generation k = scnt[k] + fcnt[k])
    p.qStride = (1 + 2 * PACKET_QUEUE_WORDS) * (R + 2);   // per launch step k: the lane kernel's queue word and the heads of each packet launch (closest, shadow)
    // The common frame (one chunk, no supersampling levels, no ray tree, no counting pass) puts nothing but its kernels
    // on the stream: counters come back through k_compose's epilogue and the frame's events ride on raygen / compose.
    // ... and so does a ray-tree frame of one chunk: its buffers are sized optimistically, so the frame carries a word that says
    // "a generation did not fit"; frame_finish then renders it again the careful way (chunks, checks, retries) and the scene's later
    // ray-tree frames take that way from the start.  Not where something is enqueued behind the frame that a redo cannot recall
    // (the in-library gather of n_gpus > 1).
    const bool heapOptimistic = heap && heapFastAllowed && s.cfg.heapFast && s.heapFastOk && nParts == 1;
    // ... and an adaptive frame (RT:170-311) whose passes are one chunk each: the sizes of the deeper quadrant levels stay on the device
    // (k_ms_decide counts, the next level's kernels read the count), the level buffers are sized optimistically -- one quadrant per
    // pixel and level -- and a level that does not fit sets the same kind of word.
    const bool adaptiveOptimistic = adaptive && !heap && heapFastAllowed && s.cfg.adaptiveFast && s.adaptiveFastOk && nParts == 1 && !p.collect && p.totalPixels * 4 <= p.chunkPaths &&
                                    (p.quality + 2) * (R + 2) * 2 + 2 <= MAX_STAMP_ROWS;
    p.fast = (adaptive ? adaptiveOptimistic : (!heap || heapOptimistic)) && oneChunk && !p.collect && !batch;
    p.heapFast = heapOptimistic && p.fast;
    p.adaptiveFast = adaptiveOptimistic && p.fast;
    if (p.adaptiveFast) {
        p.cntBase = ADAPTIVE_LEVEL_WORDS;
        p.levelCap = (int)(s.cfg.adaptiveCap > 0 ? std::min(s.cfg.adaptiveCap, p.totalPixels) : p.totalPixels);   // (XRT_ADAPTIVE_CAP; deeper levels: one quadrant per pixel)
    }
    // Answered at emission (kernels.h ShadeArgs::ae): plain one-chunk frames of one-body scenes whose mesh CAN face away from a ray as a whole (its normal
    // box or its diagonal box does not hold the origin: traverse.h mesh_can_face_away).  Not with the counting pass -- it counts the reference's work for every query from the ray lists --, not for ray trees.
    // (a batch of one chunk too: what part A answers depends on the hits alone, not on where generation 0 came from)
    p.ae = (p.fast || (batch && oneChunk && !p.collect)) && !heap && !adaptive && nParts == 1 && scene_answers_at_emission(s);
    // Finished in part A (kernels.h ShadeArgs::finish): such a frame's hits whose shadow rays are all answered at emission take no slot.  Not with path capture --
    // k_paths_capture reads every hit's position from its slot record --, and the lights have to fit part A's bit mask.
    p.finishA = p.ae && !p.capturePaths && nL <= 32 && s.cfg.finishInPartA;
    // End early (kernels.h EndArgs): the frames that finish hits in part A, when they put nothing but kernels on the stream (their counters come back with
    // k_compose) and want no float colours -- every path that ends at generation 0 is coloured where it ends, k_compose walks a list of the others.
    p.endEarly = p.finishA && p.fast && !wantsF32 && s.cfg.endEarly;
    // ... and where such a frame has a level map, the tiles outside it take no part (kernels.h EndArgs::skipTiles).  Not with one sample per pixel: a group of the walk
    // would cover eight kept tiles, and C5 at one sample measured 0.740 -> 0.752 ms per step with it (profiles/gen0_latency) -- such frames keep the old walk.
    p.skipTiles = p.endEarly && g.lvl.on != 0 && g.samples > 1;
    p.endSkipped = p.skipTiles ? (unsigned long long)(p.totalTiles - lvl_kept_tiles(g)) << g.lvl.shift : 0;
    // k_compose writes the framebuffer itself.  Not where paths end early: the early writers go through the context's sample buffer and k_resolve copies it
    // out -- d_out stays what it was until the frame's last kernel, as in every other frame (a caller may have queued work of its own on it that is still
    // running when k_raygen starts).
    p.fuseResolve = !adaptive && !heap && !batch && g.samples == 1 && !p.endEarly;
    // the traversal launches time themselves on the device clock instead of carrying events (device_util.h); a frame of more
    // than MAX_STAMP_ROWS launches (many chunks or supersampling levels) goes on with events
    p.useStamps = !s.cfg.launchEvents && s.cfg.launchTiming && s.wallClockKHz > 0;
    // No stream given.  Single-chunk frames get a stream per context, so that two frames in flight overlap on the GPU
    // (C2: 0.139 -> 0.115 ms per frame, C3 2.7 -> 2.3); everything else, and frames of a few microseconds, stay on the
    // scene's one stream.  (While every traversal launch carried two events, enqueueing on a stream that had gone idle cost
    // ~15 us a launch and alternating streams made the host the bottleneck of 0.2 ms frames; the launches time themselves
    // now, device_util.h.)
    p.ownStream = !hasStream && p.fast && s.lastFrameMs >= s.cfg.overlapMinMs && !s.cfg.oneStream;
    // Tile costs (xrt.h xrt_scene_tile_costs): the packets of plain one-chunk frames add their device-clock ticks to the tile of their first ray.
    p.tileCosts = p.fast && !adaptive && !heap && s.packetOk && p.framePaths < (1LL << 31);
    // which ray populations the wave-packet kernel traces this frame (packet.hip): bit 0 primary rays, 1 shadow rays, 2 closest-hit
    // rays of later generations
    // (two-level scenes: at any sample count and in every generation -- what a packet shares there is the scene walk, the bodies'
    // records and the mesh walk of a body, and an 8x8-pixel block of a 1-sample frame sees one or two bodies: C3 2.28 -> 1.57 ms,
    // C4 6.64 -> 4.37 ms per pipelined frame (packets for the first two generations only: 1.78 / 5.0, profiles/r03/packet_masks.txt);
    // one-body scenes: only with 16 sub-rays, and only the first two generations, see above)
    const int pkSamples = (batch && batch->coherent) ? batch->samples : g.samples;   // (a coherent list: the sampling its rays were made with, see below)
    // (ray-tree frames -- Transparent materials -- of two-level scenes: the first two generations and the first shadow rays, where the image
    // is big enough for a launch to be more than its floor: G2 at 720p 1.12 -> 0.97 ms, the reference's default scene at 512x512 0.31 ->
    // 0.40 with packets, so not there; packets in every generation of a ray tree are 1.5-3 x slower (profiles/r03/packet_masks_ray_trees.txt))
    const int pkHeap = s.cfg.packetMaskHeap >= 0 ? s.cfg.packetMaskHeap : ((s.sceneMode == MODE_SCENE && (long long)g.width * g.height * g.samples >= 600000LL) ? 7 : 0);
    const int pkScene = heap ? (s.packetOk ? pkHeap : 0) : scene_packet_mask(s, pkSamples);
    // A batch's generation 0 is in the caller's order, which nothing says is coherent: 64 consecutive rays need not be a patch of the same
    // surface, and a packet of scattered rays walks the union of their paths.  It goes to the per-lane kernel unless XRT_PACKET / XRT_PACKET_HEAP
    // name the packet kernel for it (bit 0; both kernels give the same answers).  Its later generations follow the hits as a frame's do.
    // ... unless the caller says it is (xrt.h XRT_LIST_COHERENT): such a batch has the mask of a frame of the same scene and sampling -- the sampling is
    // BatchSrc::samples (a list of xrt_render_pixels: 1, 4, 16; a batch's own g.samples is always 1), so a one-body scene gets packets with 16 samples alone, as its frames do.
    p.pkMask = (batch && !batch->coherent && (heap ? s.cfg.packetMaskHeap : s.cfg.packetMask) < 0) ? (pkScene & ~1) : pkScene;
    // The packet table (kernels.h QuadTable): wherever launch #0 is a packet launch of k_raygen's rays -- not a batch's (k_ingest keeps the caller's order; of an
    // adaptive frame level 0 alone, the deeper levels are quadrant lists).  One entry per 64 places k_raygen's walk of a chunk can cover: the kept tiles where it
    // walks those alone, else the chunk.
    // ... and of a coherent list of screen positions, whose fused ray generation (pixels.hip k_pixel_raygen) walks the chunk's places as k_raygen walks a frame's.
    if (s.cfg.packetQuads && (p.pkMask & 1) && (!batch || (batch->coherent && batch->gen))) {
        const long long walk = p.skipTiles ? ((long long)lvl_kept_tiles(g) << g.lvl.shift) : (long long)p.P;
        p.pkEntries = (size_t)((walk + 63) / 64);
    }
    // The table of screen boxes (screen_rects.h): camera frames of a one-body scene whose launch #0 takes the packet table, in a viewport the fields hold.  One entry
    // per leaf reference, written every frame in front of launch #0 (a real caller's camera moves) from the pose version the frame reads.  Where the host holds
    // that pose, a camera or pose no entry can be proven for (make_screen_xf: an orthographic or singular matrix, rays that lose their direction far from the
    // origin) takes no table: the frame then pays neither the two kernels nor the walk with a table whose every entry says "no cull".  After a pose update from
    // device arrays the host cannot know, and the device's own evaluation decides entry by entry.  XRT_PK_SCREEN=0: never.
    if (p.pkEntries && !batch && s.sceneMode == MODE_SINGLE && s.cfg.packetScreen && g.width <= SCR_MAX_EXTENT && g.height <= SCR_MAX_EXTENT &&
        s.host->arrays.refN.size() < ((size_t)1 << 30)) {
        bool ok = true;
        if (!s.posesOnDevice && !s.host->arrays.objects.empty()) { ScreenXf X; make_screen_xf(g, s.host->arrays.objects[0].invWorld, X); ok = X.ok != 0; }
        if (ok) p.scrRefs = s.host->arrays.refN.size();
    }
    const bool laneClosest = (p.pkMask & 5) != 5;   // some closest-hit generation is traced ray by ray: the long-ray feedback has a reader
    p.wantFeedback = p.fast && !heap && !adaptive && s.deepMeshes && !s.cfg.noFeedback && laneClosest;   // (the paths of a deeper quadrant level are a list: no stable key)
    // "long ray first" (kernels.hip): the producer of generation k lists its long rays, launch #k takes them first
    p.listLong = s.heavyPath > 0.0f || p.wantFeedback;
    p.hinted = p.fast && nParts == 1 && s.genKey == firstPaths * 64 + nL && s.genHeap == heap && s.cfg.gridHints;
    p.shadeBlock = s.cfg.shadeBlock;
    // valid pixels of this part
    if (batch) p.validPixels = (unsigned long long)batch->n;
    else {
        const long long slot0 = p.partStart / (512LL * g.samples), slot1 = (p.partStart + firstPaths + 512LL * g.samples - 1) / (512LL * g.samples);   // tile slots of this part
        for (long long sl = slot0; sl < slot1; sl++) {
            const long long t = tile_of_slot(s, p, sl);
            if (t >= p.totalTiles) break;
            if (t < 0) continue;   // (an unused slot of a tile table)
            const int tx = (int)(t % g.tilesX), ty = (int)(t / g.tilesX);
            const int w = std::min(g.width - tx * XRT_TILE_W, (int)XRT_TILE_W), h = std::min(g.height - ty * XRT_TILE_H, (int)XRT_TILE_H);
            p.validPixels += (unsigned long long)w * h;
        }
    }
    if (int rc = lights_known(nullptr, lights, nL)) return rc;
    plan = p;
    return XRT_OK;
}

namespace {

int frame_finish(xrt_scene *s, xrt_scene::FrameCtx &F, xrt_stats *stats);
int split_arena(xrt_scene *s, DevBuf<unsigned> &items, DevBuf<unsigned> &recs, PacketArgs &PA, hipStream_t st);

// Hits of generation k in a chunk's counter block hc (FramePlan::cntStride): the slots part A took plus the hits it finished itself (ShadeArgs::finish)
static inline long long gen_hits(const int *hc, int R, int k) { return (long long)hc[(R + 2) + k] + (long long)hc[4 * (R + 2) + k]; }

// One chunk's counters hc into the frame's tallies.  The `answered` part runs only in frames answered at emission: queries part A answered itself -- the
// hits' shadow rays that were not emitted, and (not in the last generation) their reflections.
void tally_chunk(xrt_scene::FrameCtx &F, const int *hc) {
    const FramePlan &P = F.plan;
    const int R = P.R;
    for (int k = 0; k <= R; k++) {
        F.shaded += (unsigned long long)gen_hits(hc, R, k);
        if (k > 0) F.closestDeep += (unsigned long long)(P.heap ? hc[k] : gen_hits(hc, R, k - 1));   // reflection chain: one ray per parent hit
        else F.live0 += (unsigned long long)hc[0];
        if (P.ae) {
            F.answered += (unsigned long long)gen_hits(hc, R, k) * (unsigned long long)P.nL - (unsigned long long)hc[3 * (R + 2) + k];
            if (k < R) F.answered += (unsigned long long)(gen_hits(hc, R, k) - hc[k + 1]);
        }
    }
}

// Every work buffer of the frame context (and the scene's shared ones) at the size the plan names.  What is new and must start at zero is cleared here on
// the SCENE's stream (the compose list's count words: the frame's stream is not chosen yet, and a new allocation is rare); the path staging records are
// cleared on the frame's stream by the caller, who is told which of them are new (freshPathRecs: bit 0 pathHit, bit 1 pathDir).
int ensure_frame_buffers(xrt_scene *s, xrt_scene::FrameCtx &F, const FramePlan &P, unsigned &freshPathRecs) {
    xrt_scene::WorkBufs &W = F.w;
    const size_t rayCap = P.rayCap, perLight = rayCap * (size_t)(P.nL > 0 ? P.nL : 1);
    int rc;
    if ((rc = W.rays0.ensure(rayCap)) || (rc = W.rays1.ensure(rayCap)) || (rc = W.hits.ensure(rayCap)) || (rc = W.path0.ensure(rayCap)) ||
        (rc = W.path1.ensure(rayCap)) || (rc = W.hitFlags0.ensure(rayCap)) ||
        (rc = W.shadowFlags.ensure(perLight)) || (rc = W.slot0.ensure(rayCap)) ||
        (rc = W.slot1.ensure(rayCap)) || (rc = W.index0.ensure(rayCap)) || (rc = W.heavyList.ensure(rayCap)) || (rc = W.shadowRays.ensure(perLight)) ||
        (rc = W.shadowHits.ensure(perLight)) || (rc = W.lvlA.ensure(P.lvlStride * P.nodes)) ||
        (rc = W.lvlB.ensure(P.lvlStride * P.nodes)) || (rc = W.sampleColor.ensure(P.P)) || (rc = W.lights.ensure(P.nL > 0 ? P.nL : 1)) ||
        (rc = s->counters.ensure(2 * C_COUNT + 8)))
        return rc;
    if (!s->cfg.waveTimesPath.empty() && !s->waveTimes.p) {
        if ((rc = s->waveTimes.ensure((size_t)16 * 3 * 8192))) return rc;
        HIPCHECK(hipMemset(s->waveTimes.p, 0, (size_t)16 * 3 * 8192 * sizeof(unsigned long long)));
    }
    if (P.heap && ((rc = W.node0.ensure(rayCap)) || (rc = W.node1.ensure(rayCap)) || (rc = W.ref0.ensure(rayCap)) || (rc = W.ref1.ensure(rayCap)) ||
                   (rc = W.slotNode0.ensure(rayCap)) || (rc = W.slotNode1.ensure(rayCap)) ||
                   (rc = W.lvlAlpha.ensure((size_t)P.P * P.nodes))))
        return rc;
    if (P.wantF32 && !P.batch && (rc = W.sampleF32.ensure((size_t)P.P * 3))) return rc;   // (a batch's compose writes the caller's arrays)
    if (P.ae && ((rc = W.shadowOut.ensure(perLight)) || (rc = W.shadowFlags1.ensure(perLight)))) return rc;
    if (P.endEarly) {
        const int *before = W.composeList.p;
        if ((rc = W.composeList.ensure(rayCap + 16))) return rc;
        if (W.composeList.p != before) {   // the count words (kernels.h EndArgs::cnt) start at zero
            HIPCHECK(hipMemsetAsync(W.composeList.p, 0, 16 * sizeof(int), s->stream));
            HIPCHECK(hipStreamSynchronize(s->stream));
        }
    }
    if (P.pkEntries) {
        const unsigned *before = W.quadTable.p; const size_t capBefore = W.quadTable.cap;
        if ((rc = W.quadTable.ensure((size_t)QUAD_HEAD_WORDS + 2 * P.pkEntries))) return rc;
        if (W.quadTable.p != before || W.quadTable.cap != capBefore) {   // the count words (kernels.h QuadTable) start at zero; from then on k_raygen clears the one it does not count into
            HIPCHECK(hipMemsetAsync(W.quadTable.p, 0, QUAD_HEAD_WORDS * sizeof(unsigned), s->stream));
            HIPCHECK(hipStreamSynchronize(s->stream));
        }
    }
    if (P.scrRefs && ((rc = W.scrTable.ensure(P.scrRefs + SCREEN_XF_SLOTS)) || (rc = W.pkRect.ensure(P.pkEntries)))) return rc;
    if (P.useStamps) {
        if ((rc = W.stamps.ensure((size_t)MAX_STAMP_ROWS * STAMP_STRIDE))) return rc;
        if ((rc = F.stampHost.ensure((size_t)MAX_STAMP_ROWS * 2 * sizeof(unsigned long long), hipHostMallocMapped))) return rc;
    }
    freshPathRecs = 0;
    if (P.capturePaths) {   // staging records like the level records: one per node and path of a chunk; cleared when allocated, told apart by tag afterwards
        auto ensure_fresh = [&](DevBuf<f4> &b, size_t n, unsigned bit) -> int {
            const f4 *before = b.p; const size_t capBefore = b.cap;
            const int rc2 = b.ensure(n);
            if (rc2 == XRT_OK && (b.p != before || b.cap != capBefore)) freshPathRecs |= bit;
            return rc2;
        };
        const size_t pathBlocks = ((size_t)P.P + PATHS_BLOCK - 1) / PATHS_BLOCK;
        if ((rc = ensure_fresh(s->pathHit, P.lvlStride * P.nodes, 1u)) || (P.heap && (rc = ensure_fresh(s->pathDir, P.lvlStride * P.nodes, 2u))) || (rc = s->pathLocal.ensure((size_t)P.P)) ||
            (rc = s->pathBlockSum.ensure(pathBlocks)) || (rc = s->pathBlockBase.ensure(pathBlocks)))
            return rc;
        if ((rc = s->pathPinned.ensure(64, hipHostMallocDefault))) return rc;
    }
    return XRT_OK;
}

// What a pass does with a chunk's samples once the chunk is enqueued.
struct ChunkPost {
    enum Kind { NOTHING, EMIT_PATHS, RESOLVE, COPY_LEVEL } kind = NOTHING;
    uint32_t *levelColor = nullptr;   // COPY_LEVEL: the quadrant level's colour array
};

// The enqueue of one frame on its stream: what frame_begin has gathered (scene, context, plan, views, stream, the two frame events, the caller's
// arrays) and the little that changes while the frame's launches are made.
struct FrameJob {
    xrt_scene *s;
    xrt_scene::FrameCtx &F;
    const FramePlan &P;
    xrt_scene::WorkBufs &W;
    SceneView S;          // every kernel of the frame reads one pose version
    ShadeView V;          // ... and one material version
    hipStream_t st;
    hipEvent_t e0, e1;    // the frame's start and end
    const BatchSrc *batch;
    uint32_t *d_out;
    float *d_outF32;
    unsigned *tileCostDev;   // the scene's tile cost words, or null
    int *overflowFlag;       // "a generation did not fit its buffers"
    bool startEvent;         // the frame's first raygen launch carries its start event (fast frames put nothing but kernels on the stream)
    unsigned pathEpoch = 0;  // path capture: the tag of the chunk attempt being enqueued
    bool screenDone = false; // the frame's table of screen boxes is written (once per frame: every chunk has the same camera and pose)

    static constexpr int QW = 1 + 2 * PACKET_QUEUE_WORDS;   // queue words of a launch step (FramePlan::qStride)

    // One launch step of a chunk: what its traversal launches share.
    struct Step {
        const RayGenParams &gp;
        unsigned *q;              // the chunk's queue words
        long long pathBase;
        int k;
        const int *pathOfClosest; // path of every closest-hit ray of the step
        const SlotRec *slotPrev;  // slot records of the generation whose shadow rays the step traces
    };

    bool packet_closest(int k) const { const int m = P.pkMask; return (k == 0 ? (m & 1) : (k == 1 ? (m & 4) : ((m & 4) && (m & 16)))) != 0; }
    bool packet_shadow(int k) const { return (P.pkMask & 2) != 0 && (k <= 1 || (P.pkMask & 16) != 0); }   // shadow rays of generation k-1
    long long hint(const long long *v, int k) const { return (P.hinted && k < 68 && v[k] >= 0) ? 4 * v[k] + 4096 : -1; }
    int ensure_pinned(size_t bytes) { return F.pinned.bytes < bytes ? F.pinned.ensure(bytes + 4096, hipHostMallocMapped) : XRT_OK; }
    HeavyArgs heavy_for(int k, int *hcnt) const;
    int pick_timing(int grid, unsigned long long *&stamps, hipEvent_t &a0, hipEvent_t &a1);
    int launch_packets(const Step &T, const IntersectArgs &I, bool shadow, long long nHost, const IntersectArgs *I2 = nullptr, const QuadTable *quads = nullptr);
    int launch_lanes(const Step &T, const IntersectArgs *C, const IntersectArgs *B, int Pc);
    int enqueue_chunk(const RayGenParams &gp, int *cnt, unsigned *q, int Pc, long long pathBase, uint32_t *sampleOut = nullptr, const FrameEpilogue *epi = nullptr,
                      int *listCnt = nullptr);
    int post_chunk(const ChunkPost &post, int Pc, long long pathBase);
    int run_pass_tree(const RayGenParams &gp, long long total, const ChunkPost &post, float progress0, float progress1, bool finalPass);
    int run_pass(const RayGenParams &gp, long long total, const ChunkPost &post, float progress0, float progress1, bool finalPass);
    int batch_frame();
    int plain_frame();
    int adaptive_in_flight();
    int adaptive_careful();
};

// The long-ray list of launch #k, if it has one (hcnt: the chunk's list lengths).
HeavyArgs FrameJob::heavy_for(int k, int *hcnt) const {
    HeavyArgs H;
    if (P.listLong && (k == 0 || !P.heap) && !packet_closest(k)) {   // (packets are not scheduled ray by ray)
        H.list = W.heavyList.p; H.count = hcnt + k; H.path = s->heavyPath;
        if (P.wantFeedback) { H.costMap = s->costMap.p + (size_t)k * (size_t)P.framePaths + (size_t)P.partStart; H.epoch = s->epoch & 0xffffu; H.costThreshold = s->costT[k]; }
    }
    return H;
}

// How a traversal launch of `grid` blocks is timed: by a row of device-clock stamps (stamps), by a pair of events (a0, a1), or not at all.
int FrameJob::pick_timing(int grid, unsigned long long *&stamps, hipEvent_t &a0, hipEvent_t &a1) {
    a0 = get_event(F.events, F.ev); a1 = get_event(F.events, F.ev + 1);
    if (!a0 || !a1) return fail(XRT_E_HIP, "hipEventCreate failed");
    if (P.useStamps && grid * 4 <= STAMP_SLOTS && F.stampRows < s->cfg.maxStampRows) { stamps = W.stamps.p + (size_t)F.stampRows++ * STAMP_STRIDE; a0 = a1 = nullptr; }
    else if (!s->cfg.launchTiming) a0 = a1 = nullptr;
    else { F.pairs.push_back({F.ev, F.ev + 1}); F.ev += 2; }
    return XRT_OK;
}

// A segment of coherent rays to the wave-packet kernel (I2: a second ray population for the same launch -- the shadow rays beside the closest-hit rays -- or null;
// quads: the packet table k_raygen wrote for the segment -- launch #0 of a frame -- or null).
int FrameJob::launch_packets(const Step &T, const IntersectArgs &I, bool shadow, long long nHost, const IntersectArgs *I2, const QuadTable *quads) {
    const int k = T.k, word = shadow ? 1 : 0, R = P.R, nL = P.nL;
    int rc;
    PacketArgs PA = packet_args(s, I, I2, quads);
    if (quads && quads->table && quads->rect) { PA.scrTable = W.scrTable.p; PA.pkRect = quads->rect; }   // (launch #0 of a camera frame with a table of screen boxes)
    PA.queue += PACKET_QUEUE_WORDS * word;   // (a step's queue words: the per-lane head, the packet heads of its closest-hit rays, those of its shadow rays)
    if (tileCostDev) {   // which tile pays for a packet: the path of its first ray (closest-hit rays: the path list; shadow rays: their hit's slot record)
        PA.tileCost = tileCostDev; PA.tileBase = (int)T.pathBase; PA.tileShift = 9 + (T.gp.samples == 16 ? 4 : (T.gp.samples == 4 ? 2 : 0));
        if (shadow) { PA.slotOf1 = T.slotPrev; PA.nL1 = nL; }
        else PA.pathOf1 = T.pathOfClosest;
        if (I2) { PA.slotOf2 = T.slotPrev; PA.nL2 = nL; }
    }
    if (s->cfg.packetSplit && s->sceneMode != MODE_SCENE) {
        if ((rc = split_arena(s, W.splitItems, W.splitRecs, PA, st))) return rc;
        if (P.fast && !P.adaptive && !P.heap && s->cfg.packetLongUs > 0) {   // plain frames: the packets of launch #k are the same from frame to frame while the camera stands still, and nearly so while it moves
            const size_t stride = std::max((P.rayCap + 63) / 64, P.pkEntries) + ((size_t)P.shadowCap * (size_t)(nL > 0 ? nL : 1) + 63) / 64 + 2;
            if (W.splitCostStride != stride || !W.splitCost.p) {
                if ((rc = W.splitCost.ensure(stride * 2 * (size_t)(R + 2)))) return rc;
                HIPCHECK(hipMemsetAsync(W.splitCost.p, 0, stride * 2 * (size_t)(R + 2) * sizeof(unsigned), st));
                W.splitCostStride = stride;
            }
            PA.splitCost = W.splitCost.p + stride * (size_t)(2 * k + word);
            PA.splitLong = s->cfg.packetLongUs; PA.splitBudgetLong = std::max(1, s->cfg.packetBudgetLongUs);
        }
    }
    const int grid = packet_grid(s, s->blocksPerCUPacket, nHost);
    hipEvent_t a0, a1;
    if ((rc = pick_timing(grid, PA.stamps, a0, a1))) return rc;
    launch_packet(S, PA, grid, st, a0, a1);
    return XRT_OK;
}

// The segments that are traced ray by ray (C: closest-hit rays, B: shadow rays; either may be null), together in one launch of the per-lane kernel.
int FrameJob::launch_lanes(const Step &T, const IntersectArgs *C, const IntersectArgs *B, int Pc) {
    const int k = T.k;
    IntersectArgs A = C ? *C : *B;
    if (C && B) { A.rays2 = B->rays; A.hits2 = B->hits; A.flags2 = B->flags; A.nDev2 = B->nDev; A.nMul2 = B->nMul; A.nCap2 = B->nCap; A.scatter2 = B->scatter; }
    const int grid = k == 0 ? persistent_grid(s, Pc) : persistent_grid(s, hint(s->genRays, k), 16);
    hipEvent_t a0, a1;
    if (int rc = pick_timing(grid, A.stamps, a0, a1)) return rc;
    if (s->waveTimes.p && k < 16) A.debugTimes = s->waveTimes.p + (size_t)k * 3 * 8192;
    launch_intersect(S, A, s->stackNeeded, grid, st, a0, a1);
    return XRT_OK;
}

// Enqueue one chunk of `Pc` paths starting at `pathBase`: raygen, R+2 rounds of (intersect, shade), compose.
// Intersect launch #k traces the closest-hit rays of generation k together with the shadow rays of generation k-1
// (both exist once k_shade has looked at the hits of generation k-1); k_shade #k then shades generation k-1 with the
// shadow answers and turns the hits of generation k into shadow rays and the rays of generation k+1.
// (sampleOut: where the chunk's quantised colours go -- the context's sample buffer, or a quadrant level's colour array; epi: the
// frame epilogue this chunk's compose kernel carries, if any)
// (listCnt: the chunk ends generation-0 paths early, kernels.h EndArgs -- the count word of its compose list)
int FrameJob::enqueue_chunk(const RayGenParams &gp, int *cnt, unsigned *q, int Pc, long long pathBase, uint32_t *sampleOut, const FrameEpilogue *epi, int *listCnt) {
    const int R = P.R, nL = P.nL;
    const bool heap = P.heap, ae = P.ae, fast = P.fast, feedback = P.wantFeedback;
    const size_t rayCap = P.rayCap, shadowCap = P.shadowCap;
    int rc;
    int *scnt = cnt + (R + 2), *hcnt = cnt + 2 * (R + 2), *acnt = cnt + 3 * (R + 2);   // (acnt[k]: shadow rays of generation k that were really emitted, ShadeArgs::ae)
    int *fcnt = cnt + 4 * (R + 2);                                                      // (fcnt[k]: hits of generation k finished in part A, ShadeArgs::finish)
    const int chunkRow0 = F.stampRows;
    if (P.capturePaths) {   // this attempt's records carry a number no earlier attempt had
        if (++s->pathEpoch == 0) {
            HIPCHECK(hipMemsetAsync(s->pathHit.p, 0, s->pathHit.cap * sizeof(f4), st));
            if (s->pathDir.p) HIPCHECK(hipMemsetAsync(s->pathDir.p, 0, s->pathDir.cap * sizeof(f4), st));
            s->pathEpoch = 1;
        }
        pathEpoch = s->pathEpoch;
    }
    xrt_ray *rays[2] = {W.rays0.p, W.rays1.p};
    int *paths[2] = {W.path0.p, W.path1.p};
    int *nodesOf[2] = {W.node0.p, W.node1.p};
    float *refOf[2] = {W.ref0.p, W.ref1.p};
    // cnt[0] counts the primary rays that reach the scene's root box; index0 lists them
    RayGenParams gb = gp;
    if (P.batch && heap) gb.batchRef = refOf[0];
    EndArgs endArgs;
    if (listCnt) {
        endArgs.on = 1; endArgs.sampleColor = sampleOut ? sampleOut : W.sampleColor.p;
        endArgs.list = W.composeList.p + 16; endArgs.cnt = listCnt; endArgs.listCap = (int)rayCap;
        endArgs.skipTiles = P.skipTiles ? 1 : 0;
    }
    // launch #0 takes its packets from the table k_raygen writes beside the live list (kernels.h QuadTable); the context's two count words take turns
    QuadTable quads;
    // (level 0 of an adaptive frame is k_raygen's walk too, four sub-rays per pixel; the deeper levels are lists of quadrants and take no table)
    if (P.pkEntries && (!P.batch || batch->gen) && gp.quadLevel <= 0 && packet_closest(0) && (P.skipTiles || ((size_t)Pc + 63) / 64 <= P.pkEntries)) {
        W.quadWord ^= 1;
        quads.table = reinterpret_cast<uint2 *>(W.quadTable.p + QUAD_HEAD_WORDS); quads.cap = (int)P.pkEntries;
        quads.count = W.quadTable.p + 64 * W.quadWord; quads.clear = W.quadTable.p + 64 * (W.quadWord ^ 1);
        if (P.scrRefs && !P.batch) quads.rect = W.pkRect.p;   // (screen_rects.h: every entry with the screen rectangle of its unit)
    }
    if (P.givenHits) {   // the caller's rays AND their closest hits: the live slots get ray, hit and hit word here, launch #0 below does not happen (hits.hip)
        Range r("xrt ingest hits");
        IngestHitsArgs G;
        G.rays = batch->rays; G.hits = batch->hits; G.pathBase = pathBase; G.P = Pc;
        G.raysOut = rays[0]; G.hitsOut = W.hits.p; G.flagsOut = W.hitFlags0.p; G.index = W.index0.p; G.count = cnt; G.lvlB0 = W.lvlB.p;
        G.refOut = heap ? refOf[0] : nullptr; G.refIndex = batch->refIndex; G.liveCap = (int)rayCap;
        launch_ingest_hits(S, G, st, startEvent ? e0 : nullptr);
        startEvent = false;
    } else if (P.batch && batch->gen) {   // a coherent list of screen positions: its rays are made where they are compacted (pixels.hip), with the table where launch #0 takes one
        Range r("xrt pixel raygen");
        launch_pixel_raygen(*batch->gen, S, rays[0], W.lvlB.p, W.index0.p, cnt, Pc, pathBase, heavy_for(0, hcnt), (int)rayCap, heap ? refOf[0] : nullptr, batch->refIndex, quads, st,
                            startEvent ? e0 : nullptr);
        startEvent = false;
    } else
    { Range r("xrt raygen"); launch_raygen(gb, S, rays[0], W.lvlB.p, W.index0.p, cnt, Pc, pathBase, heavy_for(0, hcnt), st, startEvent ? e0 : nullptr, (int)rayCap, &endArgs, &quads); startEvent = false; }
    // the frame's screen boxes, behind the ray generation (which carries the frame's start event) and in front of launch #0
    if (quads.rect && !screenDone) { Range r("xrt screen rects"); launch_screen_rects(gb, S.objects, S.refT, (int)P.scrRefs, W.scrTable.p, st); screenDone = true; }
    // (one buffer serves every generation: the closest-hit answers of launch #k are read by part A of k_shade #k alone -- part B works from the
    // slot records -- and launch #k+1 starts after it on the frame's stream)
    xrt_hit *hitsOf[2] = {W.hits.p, W.hits.p};
    int *flagsOf[2] = {W.hitFlags0.p, W.hitFlags0.p};
    SlotRec *slotOf[2] = {W.slot0.p, W.slot1.p};
    int *slotNodeOf[2] = {W.slotNode0.p, W.slotNode1.p};
    int *const shadowFlagsOf[2] = {W.shadowFlags.p, ae ? W.shadowFlags1.p : W.shadowFlags.p};   // (the words of generation g: [g & 1])
    for (int k = 0; k <= R + 1; k++) {
        const int cur = k & 1, prv = cur ^ 1;
        const bool hasClosest = k <= R, hasShadow = k >= 1 && nL > 0;
        const bool traceClosest = hasClosest && !(k == 0 && P.givenHits);   // (given hits: generation 0 is shaded, never traced or counted)
        // a reflection chain keeps the ray of generation k at its parent's slot: their number is scnt[k-1]
        const int *nClosest = (k == 0 || heap || ae) ? cnt + k : scnt + (k - 1);   // (ae: the reflections that were emitted are a compact list, counted by part A)
        IntersectArgs C, B;   // closest-hit segment, shadow segment
        C.rays = rays[cur]; C.hits = hitsOf[cur]; C.index = nullptr; C.nDev = nClosest; C.nMul = 1; C.n = Pc;   // (generation 0: cnt[0] live rays, compact)
        C.nCap = (int)rayCap;
        C.flags = flagsOf[cur]; B.flags = shadowFlagsOf[(k + 1) & 1];   // launch #k traces the shadow rays of generation k - 1
        C.missRecords = (feedback && !packet_closest(k)) ? 1 : 0;   // k_shade #k reads the cost word of every ray of the generation
        { const HeavyArgs H = heavy_for(k, hcnt); C.heavyIdx = H.list; C.nHeavy = H.count; }
        B.rays = W.shadowRays.p; B.hits = W.shadowHits.p; B.index = nullptr; B.nDev = hasShadow ? scnt + (k - 1) : nullptr; B.nMul = nL; B.n = 0;
        if (ae && hasShadow) { B.nDev = acnt + (k - 1); B.nMul = 1; B.scatter = W.shadowOut.p; }   // the emitted shadow rays, compact; answers go back to (slot, light)
        B.nCap = (int)((long long)shadowCap * nL);
        for (IntersectArgs *a : {&C, &B}) {
            a->queue = q + QW * k; a->mode = s->sceneMode; a->meshId = 0;
            set_knobs(*a, s);
        }
        // segments of coherent rays go to the wave-packet kernel, the others (together, one launch) to the per-lane kernel
        const bool pkC = traceClosest && packet_closest(k), pkB = hasShadow && packet_shadow(k);
        const Step T{gp, q, pathBase, k, k == 0 ? W.index0.p : paths[cur], slotOf[prv]};
        Range ri("xrt intersect #%d", k);
        // both populations of a step in ONE packet launch where both go to the packet kernel: one launch's tail instead of two
        if (pkC && pkB && s->cfg.packetMerge) { if ((rc = launch_packets(T, C, false, hint(s->genRays, k), &B))) return rc; }
        else {
            if (pkC && (rc = launch_packets(T, C, false, k == 0 ? Pc : hint(s->genRays, k), nullptr, k == 0 ? &quads : nullptr))) return rc;
            if (pkB && (rc = launch_packets(T, B, true, hint(s->genRays, k)))) return rc;
        }
        const bool laneC = traceClosest && !pkC, laneB = hasShadow && !pkB;
        if ((laneC || laneB) && (rc = launch_lanes(T, laneC ? &C : nullptr, laneB ? &B : nullptr, Pc))) return rc;
        if ((hasClosest || hasShadow) && P.collect) {   // generation 0: the live list; culled rays are added in frame_finish
            if (traceClosest) launch_count(S, C, s->counters.p, st);
            if (hasShadow) launch_count(S, B, s->counters.p + C_COUNT, st);
        }
        if (ri.on) { roctx().pop(); ri.on = false; }
        Range rs("xrt shade #%d", k);
        ShadeArgs X;
        std::memset(&X, 0, sizeof(X));
        X.level = k; X.doA = hasClosest ? 1 : 0; X.doB = k >= 1 ? 1 : 0;
        X.maxReflections = R; X.P = (int)P.lvlStride; X.lvl = gp.lvl; X.heap = heap ? 1 : 0; X.overflow = overflowFlag;
        X.rays = rays[cur]; X.hits = hitsOf[cur]; X.hitFlags = flagsOf[cur]; X.shadowFlags = shadowFlagsOf[(k + 1) & 1]; X.nDev = nClosest; X.nHost = Pc; X.cap = (int)rayCap;
        X.index = nullptr; X.rayPath = k == 0 ? W.index0.p : paths[cur];   // (generation 0: the j-th live ray belongs to path index0[j])
        X.rayNode = (heap && k > 0) ? nodesOf[cur] : nullptr;
        X.rayRef = (heap && (k > 0 || P.batch)) ? refOf[cur] : nullptr;   // (a batch's generation 0 carries the caller's currentRefIndex, k_ingest)
        X.slotOut = slotOf[cur]; X.slotNodeOut = heap ? slotNodeOf[cur] : nullptr; X.scnt = scnt + k; X.shadowCap = (int)shadowCap; X.shadowRays = W.shadowRays.p;
        X.nextRays = rays[prv]; X.nextPath = paths[prv]; X.nextNode = heap ? nodesOf[prv] : nullptr; X.nextRef = heap ? refOf[prv] : nullptr;
        X.nextCnt = cnt + k + 1; X.nextCap = (int)rayCap;
        if (ae) { X.ae = 1; X.shadowCnt = acnt + k; X.shadowOut = W.shadowOut.p; X.shadowFlagsOut = shadowFlagsOf[k & 1]; }
        if (P.finishA) { X.finish = 1; X.finishCnt = fcnt + k; }
        if (listCnt && k == 0) X.end = endArgs;
        X.slotPrev = slotOf[prv]; X.slotNodePrev = heap ? slotNodeOf[prv] : nullptr; X.scntPrev = k >= 1 ? scnt + (k - 1) : nullptr; X.shadowHits = W.shadowHits.p;
        X.lvlA = W.lvlA.p; X.lvlB = W.lvlB.p; X.lvlAlpha = heap ? W.lvlAlpha.p : nullptr;
        if (k < R) X.heavy = heavy_for(k + 1, hcnt);
        if (feedback && hasClosest && !packet_closest(k)) { X.costOut = s->costMap.p + (size_t)k * (size_t)P.framePaths + (size_t)P.partStart; X.epoch = s->epoch & 0xffffu; }
        {   // (a small generation: 256-thread blocks, so that its work items land on many CUs instead of on the first few; a big or unknown one: the plan's size.
            //  The hint is in rays, launch_shade turns it into blocks of either size)
            const long long h = hint(s->genShade, k);
            launch_shade(S, V, X, st, h, (h >= 0 && h < 4 * 131072 + 4096) ? SHADE_BLOCK_MIN : P.shadeBlock);
        }
        if (P.capturePaths && hasClosest) {   // the generation's hits and the refraction rays it cast, before slots and ray buffers are reused
            PathsCaptureArgs Cp;
            Cp.slots = slotOf[cur]; Cp.slotNode = heap ? slotNodeOf[cur] : nullptr; Cp.scnt = scnt + k; Cp.slotCap = (int)shadowCap; Cp.level = k;
            if (heap && k < R) { Cp.nextRays = rays[prv]; Cp.nextNode = nodesOf[prv]; Cp.nextPath = paths[prv]; Cp.nextCnt = cnt + k + 1; Cp.nextCap = (int)rayCap; }
            Cp.hitRec = s->pathHit.p; Cp.dirRec = s->pathDir.p; Cp.P = (int)P.lvlStride; Cp.epoch = pathEpoch;
            launch_paths_capture(Cp, (int)((rayCap + 255) / 256), st);
        }
    }
    Range rc_("xrt compose");
    // a batch: path p of the chunk is ray pathBase + p, and the compose kernel writes its colour straight into the caller's arrays (a ray-tree chunk
    // that overflowed is retried over the same range: the retry overwrites what the discarded attempt wrote)
    uint32_t *const colorOut = P.batch ? d_out + pathBase : (sampleOut ? sampleOut : W.sampleColor.p);
    float *const f32Out = P.batch ? (d_outF32 ? d_outF32 + 3 * (size_t)pathBase : nullptr) : (P.wantF32 ? W.sampleF32.p : nullptr);
    StampFold fold;
    fold.src = W.stamps.p; fold.host = F.stampHost.dev; fold.row0 = chunkRow0; fold.row1 = F.stampRows;
    if (heap) {
        FrameEpilogue E;
        if (fast) { E.cntSrc = cnt; E.hostCnt = F.pinned.dev; E.cntWords = P.cntStride; E.zeroWords = P.cntStride + P.qStride; E.flagSrc = overflowFlag; }
        launch_compose_tree(W.lvlA.p, W.lvlB.p, W.lvlAlpha.p, Pc, P.P, R, colorOut, f32Out, fold, E, st);
    }
    else {
        ResolveArgs RA;
        RA.fused = P.fuseResolve ? 1 : 0; RA.g = gp; RA.pixelBase = pathBase; RA.out = d_out; RA.outF32 = d_outF32;
        RA.stamps = fold;
        if (epi) { RA.cntSrc = epi->cntSrc; RA.hostCnt = epi->hostCnt; RA.cntWords = epi->cntWords; RA.zeroWords = epi->zeroWords; RA.zeroFrom = epi->zeroFrom; }
        else if (fast && !P.adaptive) { RA.cntSrc = cnt; RA.hostCnt = F.pinned.dev; RA.cntWords = P.cntStride; RA.zeroWords = P.cntStride + P.qStride; }
        int blocks = 0;
        if (listCnt) {
            RA.list = W.composeList.p + 16; RA.endCnt = listCnt; RA.listCap = (int)rayCap;
            if (P.hinted && s->genCompose >= 0) blocks = (int)((4 * s->genCompose + 4096 + 255) / 256);
        }
        launch_compose(W.lvlA.p, W.lvlB.p, Pc, (int)P.lvlStride, R, colorOut, P.fuseResolve ? nullptr : f32Out, RA, st,
                       (fast && P.fuseResolve) ? e1 : nullptr, blocks);
    }
    return XRT_OK;
}

int FrameJob::post_chunk(const ChunkPost &post, int Pc, long long pathBase) {
    switch (post.kind) {
    case ChunkPost::NOTHING: break;
    case ChunkPost::EMIT_PATHS: {   // the chunk's segments in the recursion's order, behind those of the rays before it
        const BatchSrc::Paths *pout = batch->paths;
        PathsEmitArgs E;
        E.batch = batch->rays; E.pathBase = pathBase; E.Pc = Pc; E.P = (int)P.lvlStride; E.depth = P.R; E.tree = P.heap ? 1 : 0; E.epoch = pathEpoch;
        E.hitRec = s->pathHit.p; E.dirRec = s->pathDir.p; E.local = s->pathLocal.p; E.blockSum = s->pathBlockSum.p; E.blockBase = s->pathBlockBase.p;
        E.vertexStart = pout->vertexStart; E.vertices = pout->vertices; E.capacity = pout->capacity; E.raysBack = pout->raysBack;
        launch_paths_emit(E, st);
        break;
    }
    case ChunkPost::RESOLVE:
        launch_resolve(P.g, W.sampleColor.p, P.wantF32 ? W.sampleF32.p : nullptr, Pc / P.g.samples, pathBase / P.g.samples, d_out, d_outF32, st, nullptr, 0, P.skipTiles ? 1 : 0);
        break;
    case ChunkPost::COPY_LEVEL:
        HIPCHECK(hipMemcpyAsync(post.levelColor + pathBase, W.sampleColor.p, (size_t)Pc * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        break;
    }
    return XRT_OK;
}

// A pass of a ray-tree frame the careful way: one chunk at a time, checked for overflow, retried with fewer paths when a generation did not fit.
int FrameJob::run_pass_tree(const RayGenParams &gp, long long total, const ChunkPost &post, float progress0, float progress1, bool finalPass) {
    int rc;
    const int cntStride = P.cntStride;
    const size_t nb2 = 2 * C_COUNT * sizeof(unsigned long long);
    const size_t words = (size_t)cntStride + (size_t)P.qStride;
    if ((rc = W.cnts.ensure(words)) || (rc = ensure_pinned(words * sizeof(int) + nb2 + 64 + 8 + 64))) return rc;
    W.cntsClean = false;
    unsigned *q = reinterpret_cast<unsigned *>(W.cnts.p + cntStride);
    long long pathBase = 0, curChunk = P.chunkPaths;   // (ray-tree frames are never split: partStart == 0)
    while (pathBase < total) {
        const int Pc = (int)((total - pathBase) < curChunk ? (total - pathBase) : curChunk);
        HIPCHECK(hipMemsetAsync(W.cnts.p, 0, words * sizeof(int), st));
        const size_t pairsMark = F.pairs.size(), evMark = F.ev;
        const int rowsMark = F.stampRows;
        if ((rc = enqueue_chunk(gp, W.cnts.p, q, Pc, pathBase))) return rc;
        // the chunk's samples are consumed before the host has looked at the overflow flag: a retry overwrites them
        if ((rc = post_chunk(post, Pc, pathBase))) return rc;
        char *pin = (char *)F.pinned.p;
        const size_t cAt = ((size_t)cntStride * sizeof(int) + 7) & ~(size_t)7;   // counters + spare words (overflow flag) in one copy
        HIPCHECK(hipMemcpyAsync(pin, W.cnts.p, (size_t)cntStride * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(pin + cAt, s->counters.p, nb2, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(pin + cAt + nb2 + 64, overflowFlag, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        const int over = *(const int *)(pin + cAt + nb2 + 64);
        if (over) {
            if (curChunk <= 64) return fail(XRT_E_UNSUPPORTED, "the ray tree of 64 paths does not fit the ray buffers (MaxReflections too high for this scene)");
            curChunk = (curChunk / 4) & ~63LL;
            if (curChunk < 64) curChunk = 64;
            HIPCHECK(hipMemsetAsync(overflowFlag, 0, sizeof(int), st));
            HIPCHECK(hipMemcpyAsync(s->counters.p, F.hcnt, nb2, hipMemcpyHostToDevice, st));   // undo this attempt's counting
            HIPCHECK(hipStreamSynchronize(st));
            F.pairs.resize(pairsMark); F.ev = evMark; F.stampRows = rowsMark;   // its launches are not part of the frame's timing
            continue;
        }
        tally_chunk(F, (const int *)pin);
        std::memcpy(F.hcnt, pin + cAt, nb2);
        pathBase += Pc;
        s->progress.store(progress0 + (progress1 - progress0) * (float)pathBase / (float)total);
    }
    if (finalPass) HIPCHECK(hipEventRecord(e1, st));
    return XRT_OK;
}

// One pass = trace `total` paths produced by generator `gp`; after every chunk `post` consumes sampleColor.
int FrameJob::run_pass(const RayGenParams &gp, long long total, const ChunkPost &post, float progress0, float progress1, bool finalPass) {
    if (P.heap && !P.fast) return run_pass_tree(gp, total, post, progress0, progress1, finalPass);
    int rc;
    const int cntStride = P.cntStride, qStride = P.qStride;
    const long long chunkPaths = P.chunkPaths;
    const bool fast = P.fast;
    const size_t nb2 = 2 * C_COUNT * sizeof(unsigned long long);
    const int nChunks = (int)((total + chunkPaths - 1) / chunkPaths);
    // ray counts and queue heads of all chunks live in one allocation: one memset per pass
    const size_t cntWords = (size_t)nChunks * cntStride, qWords = (size_t)nChunks * qStride;
    const int *cntsBefore = W.cnts.p;
    if ((rc = W.cnts.ensure(cntWords + qWords))) return rc;
    unsigned *queuesBase = reinterpret_cast<unsigned *>(W.cnts.p + cntWords);
    if (fast && (rc = ensure_pinned(cntWords * sizeof(int) + 64))) return rc;   // (+ the overflow word of a ray-tree frame)
    if (!fast || !W.cntsClean || W.cnts.p != cntsBefore) HIPCHECK(hipMemsetAsync(W.cnts.p, 0, W.cnts.cap * sizeof(int), st));
    W.cntsClean = false;
    for (int c = 0; c < nChunks; c++) {
        const long long localBase = (long long)c * chunkPaths, pathBase = P.partStart + localBase;
        const int Pc = (int)((total - localBase) < chunkPaths ? (total - localBase) : chunkPaths);
        if ((rc = enqueue_chunk(gp, W.cnts.p + (size_t)c * cntStride, queuesBase + (size_t)c * qStride, Pc, pathBase, nullptr, nullptr,
                                P.endEarly ? W.composeList.p : nullptr))) return rc;
        if (!P.fuseResolve && (rc = post_chunk(post, Pc, pathBase))) return rc;
        if (nChunks > 1) {   // frames of more than MAX_CHUNK_PATHS rays: xrt_progress follows the chunks
            HIPCHECK(hipStreamSynchronize(st));
            s->progress.store(progress0 + (progress1 - progress0) * (float)(c + 1) / (float)nChunks);
        }
    }
    if (fast) {   // counters arrive with k_compose; frame_finish tallies them
        if (!P.fuseResolve) HIPCHECK(hipEventRecord(e1, st));   // fixed 16 sub-rays: k_resolve is the last kernel
        W.cntsClean = true;
        F.tallyChunks = 1;
        return XRT_OK;
    }
    if (finalPass) HIPCHECK(hipEventRecord(e1, st));
    // per-pass ray accounting (the counter block is reused by the next pass): one pinned read-back -- two small copies, always taken
    const size_t nb = (size_t)nChunks * cntStride * sizeof(int);
    if ((rc = ensure_pinned(nb + nb2))) return rc;
    HIPCHECK(hipMemcpyAsync(F.pinned.p, W.cnts.p, nb, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync((char *)F.pinned.p + nb, s->counters.p, nb2, hipMemcpyDeviceToHost, st));
    if (finalPass) { F.tallyChunks = nChunks; return XRT_OK; }   // frame_finish tallies after the frame's done event
    HIPCHECK(hipStreamSynchronize(st));
    for (int c = 0; c < nChunks; c++) tally_chunk(F, F.pinned.p + (size_t)c * cntStride);
    std::memcpy(F.hcnt, (char *)F.pinned.p + nb, nb2);
    return XRT_OK;
}

// A pass over a caller's rays: path p is ray p, the compose kernels write the caller's arrays themselves (enqueue_chunk).
int FrameJob::batch_frame() {
    F.livePaths = F.validPixels;
    ChunkPost post;
    if (P.capturePaths) post.kind = ChunkPost::EMIT_PATHS;
    if (int rc = run_pass(P.g, P.firstPaths, post, 0.0f, 1.0f, true)) return rc;
    if (P.capturePaths) HIPCHECK(hipMemcpyAsync(s->pathPinned.p, batch->paths->vertexStart + batch->n, sizeof(long long), hipMemcpyDeviceToHost, st));
    return XRT_OK;
}

// One sample or sixteen per pixel: one pass, resolved chunk by chunk (or by k_compose itself, FramePlan::fuseResolve).
int FrameJob::plain_frame() {
    F.livePaths = F.validPixels * (unsigned long long)P.g.samples;
    ChunkPost post;
    post.kind = ChunkPost::RESOLVE;
    return run_pass(P.g, P.firstPaths, post, 0.0f, 1.0f, true);
}

// RenderFirstPass / GetColorForQuadrant (RT:170-311) without a host round trip: every level's pass is enqueued now.  Level 0 has
// one quadrant per pixel; how many quadrants a deeper level has only the device knows (k_ms_decide counts them into lvlCnt[l],
// the level's ray generation, compose and fold kernels read that word; the traversal and shading kernels follow the ray
// counts as always).  Deeper levels get room for one quadrant per pixel (XRT_ADAPTIVE_CAP); a level that needs more sets the
// overflow word and frame_finish renders the frame again the careful way.
int FrameJob::adaptive_in_flight() {
    const RayGenParams &g = P.g;
    const int quality = P.quality, cntStride = P.cntStride, qStride = P.qStride;
    const long long totalPixels = P.totalPixels;
    const int nPass = quality + 1;
    constexpr int LW = ADAPTIVE_LEVEL_WORDS;
    int rc;
    auto cap_of = [&](int l) { return l == 0 ? totalPixels : (long long)P.levelCap; };
    const size_t words = (size_t)LW + (size_t)nPass * cntStride + (size_t)nPass * qStride;
    const int *cntsBefore = W.cnts.p;
    if ((rc = W.cnts.ensure(words)) || (rc = ensure_pinned(((size_t)LW + (size_t)nPass * cntStride) * sizeof(int) + 64))) return rc;
    if (!W.cntsClean || W.cnts.p != cntsBefore) HIPCHECK(hipMemsetAsync(W.cnts.p, 0, W.cnts.cap * sizeof(int), st));
    W.cntsClean = false;
    for (int l = 0; l <= quality; l++) {
        auto &Lv = W.levels[l];
        const size_t c = (size_t)cap_of(l);
        if ((rc = Lv.color.ensure(c * 4))) return rc;
        if (l < quality && ((rc = Lv.childBase.ensure(c)) || (rc = Lv.childMask.ensure(c)))) return rc;
        if (l > 0 && ((rc = Lv.cx.ensure(c)) || (rc = Lv.cy.ensure(c)))) return rc;
    }
    int *const lvlCnt = W.cnts.p, *const ovf = W.cnts.p + LW - 1;
    int *const cnt0 = W.cnts.p + LW;
    unsigned *const q0 = reinterpret_cast<unsigned *>(cnt0 + (size_t)nPass * cntStride);
    float size = 1.0f;
    for (int l = 0; l <= quality; l++) {
        auto &Lv = W.levels[l];
        RayGenParams gl = g;
        gl.quadLevel = l; gl.quadSize = size; gl.quadCx = Lv.cx.p; gl.quadCy = Lv.cy.p;
        if (l > 0) { gl.pathsDev = lvlCnt + l; gl.pathsMul = 4; gl.pathsCap = (int)cap_of(l); }
        FrameEpilogue E;
        const bool last = l == quality;
        if (last) { E.cntSrc = W.cnts.p; E.hostCnt = F.pinned.dev; E.cntWords = LW + nPass * cntStride; E.zeroWords = (int)words; E.zeroFrom = LW; }
        if ((rc = enqueue_chunk(gl, cnt0 + (size_t)l * cntStride, q0 + (size_t)l * qStride, (int)(cap_of(l) * 4), 0, Lv.color.p, last ? &E : nullptr))) return rc;
        if (l < quality) {   // RT:279-306
            auto &Nx = W.levels[l + 1];
            launch_ms_decide(gl, Lv.color.p, l > 0 ? lvlCnt + l : nullptr, (int)cap_of(l), 0, Lv.childBase.p, Lv.childMask.p, Nx.cx.p, Nx.cy.p, lvlCnt + l + 1, st,
                             (int)cap_of(l + 1), ovf);
            size = size / 2.0f;   // RT:290
        }
    }
    for (int l = quality - 1; l >= 0; l--)
        launch_ms_fold(W.levels[l].color.p, W.levels[l + 1].color.p, W.levels[l].childBase.p, W.levels[l].childMask.p, (int)cap_of(l), st, l > 0 ? lvlCnt + l : nullptr);
    RayGenParams g0 = g;
    g0.quadLevel = 0; g0.quadSize = 1.0f;
    launch_resolve(g0, W.levels[0].color.p, nullptr, (int)totalPixels, 0, d_out, d_outF32, st, lvlCnt, LW);   // ... and clears the level words for the next frame
    HIPCHECK(hipEventRecord(e1, st));
    W.cntsClean = true;
    F.tallyChunks = nPass;
    return XRT_OK;
}

// RenderFirstPass / GetColorForQuadrant (RT:170-311), the careful way (a host read-back of every level's size): level 0
// quadrants are the pixels (size 1); a level's quadrants each cast four rays; corners that deviate are subdivided into the next
// level, down to MultisampleQuality; results fold back up.  The frame is complete when this returns.
int FrameJob::adaptive_careful() {
    const RayGenParams &g = P.g;
    const int quality = P.quality;
    int rc = XRT_OK;
    struct Level : xrt_scene::WorkBufs::Level { long long n = 0; };   // (the frame's own: freed when it is done, however it ends)
    std::vector<Level> lv((size_t)quality + 1);
    int *levelCount = reinterpret_cast<int *>(s->counters.p + 2 * C_COUNT);   // [quality+1] ints in the spare counter words
    lv[0].n = P.totalPixels;
    float size = 1.0f;
    for (int l = 0; l <= quality && rc == XRT_OK; l++) {
        Level &L = lv[l];
        if (L.n == 0) break;
        if ((rc = L.color.ensure((size_t)L.n * 4))) break;
        RayGenParams gl = g;
        gl.quadLevel = l; gl.quadSize = size; gl.quadCx = L.cx.p; gl.quadCy = L.cy.p;
        F.livePaths += (l == 0 ? F.validPixels : (unsigned long long)L.n) * 4ull;
        ChunkPost post;
        post.kind = ChunkPost::COPY_LEVEL; post.levelColor = L.color.p;
        rc = run_pass(gl, L.n * 4, post, (float)l / (float)(quality + 1), (float)(l + 1) / (float)(quality + 1), false);
        if (rc != XRT_OK) break;
        if (l < quality) {   // RT:279-306
            Level &N = lv[l + 1];
            if ((rc = L.childBase.ensure((size_t)L.n)) || (rc = L.childMask.ensure((size_t)L.n)) || (rc = N.cx.ensure((size_t)L.n * 4)) ||
                (rc = N.cy.ensure((size_t)L.n * 4)))
                break;
            launch_ms_decide(gl, L.color.p, nullptr, (int)L.n, 0, L.childBase.p, L.childMask.p, N.cx.p, N.cy.p, levelCount + l + 1, st);
            int hn = 0;
            hipError_t e = hipMemcpyAsync(&hn, levelCount + l + 1, sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { rc = fail(XRT_E_HIP, "adaptive level readback: %s", hipGetErrorString(e)); break; }
            N.n = hn;
            size = size / 2.0f;   // RT:290
        }
    }
    if (rc != XRT_OK) return rc;
    for (int l = quality - 1; l >= 0; l--)
        if (lv[l + 1].n > 0) launch_ms_fold(lv[l].color.p, lv[l + 1].color.p, lv[l].childBase.p, lv[l].childMask.p, (int)lv[l].n, st);
    RayGenParams g0 = g;
    g0.quadLevel = 0; g0.quadSize = 1.0f;
    launch_resolve(g0, lv[0].color.p, nullptr, (int)P.totalPixels, 0, d_out, d_outF32, st);
    hipError_t e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipMemcpyAsync(F.hcnt, s->counters.p, sizeof(F.hcnt), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(XRT_E_HIP, "adaptive resolve: %s", hipGetErrorString(e));
    return XRT_OK;
}

// The scene's tile cost words for this frame (xrt.h xrt_scene_tile_costs).  They belong to the scene (both frame contexts add to them); a frame of
// another geometry or tile table starts them afresh.
int tile_cost_words(xrt_scene *s, const FramePlan &P, hipStream_t st, unsigned *&words) {
    const RayGenParams &g = P.g;
    const long long myTiles = P.myTiles;
    if (int rc = s->tileCost.ensure((size_t)myTiles)) return rc;
    auto slot_tile = [&](long long sl) { const long long t = tile_of_slot(*s, P, sl); return t < P.totalTiles ? (int)t : -1; };
    bool same = s->costW == g.width && s->costH == g.height && (long long)s->costTiles.size() == myTiles;
    for (long long sl = 0; same && sl < myTiles; sl++) same = s->costTiles[(size_t)sl] == slot_tile(sl);
    if (!same) {
        s->costTiles.resize((size_t)myTiles);
        for (long long sl = 0; sl < myTiles; sl++) s->costTiles[(size_t)sl] = slot_tile(sl);
        s->costW = g.width; s->costH = g.height;
        HIPCHECK(hipMemsetAsync(s->tileCost.p, 0, (size_t)myTiles * sizeof(unsigned), st));
        if (s->frames[0].pending || s->frames[1].pending) HIPCHECK(hipStreamSynchronize(st));   // (the other context's frame may be adding to them: start clean)
    }
    words = s->tileCost.p;
    return XRT_OK;
}

// Enqueues one frame on `st`.  On return the frame's kernels and its counter read-back are in flight (F.pending);
// frame_finish waits for them.  Adaptive supersampling and ray-tree frames the careful way need host decisions between their passes and
// are complete when this returns.  d_out[p] / d_outF32[3p..] receive pixel p's colour (a batch: ray p's).
int frame_begin(xrt_scene *s, xrt_scene::FrameCtx &F, const xrt_camera *cam, const xrt_light *lights, int nLights, const xrt_render_opts *opts,
                uint32_t *d_out, float *d_outF32, hipStream_t st, int part = 0, int nParts = 1, bool heapFastAllowed = true, const BatchSrc *batch = nullptr) {
    xrt_scene::WorkBufs &W = F.w;
    int rc;
    // the plan
    if ((rc = plan_frame(*s, F.mat, cam, lights, nLights, opts, d_outF32 != nullptr, st != nullptr, part, nParts, heapFastAllowed, batch, F.plan))) return rc;
    const FramePlan &P = F.plan;
    const int R = P.R, nL = P.nL;
    if (P.lvlVerified) { s->lvlCheckedTilesX = P.g.tilesX; s->lvlCheckedTiles = P.totalTiles; }
    // the buffers
    unsigned freshPathRecs = 0;
    if ((rc = ensure_frame_buffers(s, F, P, freshPathRecs))) return rc;
    F.redone = false;
    if (P.heapFast || P.adaptiveFast) {   // what a redo needs
        F.redoCam = *cam; F.redoOpts = *opts; F.redoLights.assign(lights, lights + nLights);
        F.redoOut = d_out; F.redoOutF32 = d_outF32; F.redoSt = st;
    }
    F.stampRows = 0;
    // the stream, and what the frame waits for
    if (!st) {
        if (P.ownStream) {
            if ((rc = W.stream.create())) return rc;
            st = W.stream;
        } else st = s->stream;
    }
    if ((rc = pose_wait(s, F.pose, st)) || (rc = mat_acquire(s, F.mat, st)) || (rc = shade_wait(s, F.shade, st))) return rc;   // (the poses, materials and triangle values set before the frame's begin)
    if (freshPathRecs & 1u) HIPCHECK(hipMemsetAsync(s->pathHit.p, 0, s->pathHit.cap * sizeof(f4), st));
    if (freshPathRecs & 2u) HIPCHECK(hipMemsetAsync(s->pathDir.p, 0, s->pathDir.cap * sizeof(f4), st));
    unsigned *tileCostDev = nullptr;
    if (P.tileCosts && (rc = tile_cost_words(s, P, st, tileCostDev))) return rc;
    {   // The other context's frame may still be running on another stream.  Two single-chunk frames share nothing they
        // write except scheduling hints; anything else (counting pass, supersampling levels, ray tree, a cost map
        // about to be reallocated or released) runs alone.
        const bool remap = P.wantFeedback ? (s->costMapPaths != (size_t)P.framePaths || s->costMap.cap < (size_t)(R + 1) * (size_t)P.framePaths) : (s->costMap.p != nullptr);
        for (xrt_scene::FrameCtx &O : s->frames)
            if (&O != &F && O.pending && O.w.lastStream != st && (!P.fast || !O.plan.fast || remap)) HIPCHECK(hipEventSynchronize(O.plan.fast ? O.events[1] : O.done));
        W.lastStream = st;
    }
    if (P.wantFeedback) {
        const size_t need = (size_t)(R + 1) * (size_t)P.framePaths;
        if (s->costMapPaths != (size_t)P.framePaths || s->costMap.cap < need) {   // new frame geometry: forget
            if ((rc = s->costMap.ensure(need))) return rc;
            HIPCHECK(hipMemsetAsync(s->costMap.p, 0, s->costMap.cap * sizeof(unsigned), st));
            s->costMapPaths = (size_t)P.framePaths;
        }
        if (part == 0) s->epoch++;
    } else if (s->costMap.p) {
        s->costMap.release(); s->costMapPaths = 0;   // (freed early on purpose: a map of (R + 1) words per path that no frame of this kind reads)
    }
    // the uploads and clears
    if (!P.fast) {
        W.cntsClean = false;
        HIPCHECK(hipMemsetAsync(s->counters.p, 0, (2 * C_COUNT + 8) * sizeof(unsigned long long), st));
    }
    std::vector<LightRec> &hl = F.hostLights;   // must outlive the asynchronous upload
    hl.assign(nL > 0 ? nL : 1, LightRec());
    for (int i = 0; i < nL; i++) hl[i] = make_light(lights[i]);
    const bool sameLights = W.lightsOnDevice.size() == (size_t)nL && W.lightsDevPtr == W.lights.p &&
                            (nL == 0 || std::memcmp(W.lightsOnDevice.data(), hl.data(), nL * sizeof(LightRec)) == 0);
    if (nL > 0 && !sameLights) {
        HIPCHECK(hipMemcpyAsync(W.lights.p, hl.data(), nL * sizeof(LightRec), hipMemcpyHostToDevice, st));
        W.lightsOnDevice.assign(hl.begin(), hl.begin() + nL);
        W.lightsDevPtr = W.lights.p;
    }
    ShadeView V = shade_view(s, F.mat, F.shade);
    V.lights = W.lights.p; V.nLights = nL; V.addressMode = P.addressMode; V.filtering = P.filtering;
    F.ev = 0;
    F.pairs.clear();
    hipEvent_t e0 = get_event(F.events, F.ev++), e1 = get_event(F.events, F.ev++);
    if (!e0 || !e1 || F.done.create() != XRT_OK) return fail(XRT_E_HIP, "hipEventCreate failed");
    if (!P.fast) HIPCHECK(hipEventRecord(e0, st));
    s->progress.store(0.0f);
    F.shaded = F.closestDeep = F.livePaths = F.live0 = 0;
    F.answered = 0;
    F.validPixels = P.validPixels;
    std::memset(F.hcnt, 0, sizeof(F.hcnt));
    F.tallyChunks = 0;
    // "a generation did not fit its buffers": ray-tree frames have the word to themselves (two of them may be in flight)
    if (P.heap) {
        const bool fresh = W.heapFlag.p == nullptr;
        if ((rc = W.heapFlag.ensure(16))) return rc;
        if (fresh || !P.fast || !W.heapFlagClean) HIPCHECK(hipMemsetAsync(W.heapFlag.p, 0, 16 * sizeof(int), st));
        W.heapFlagClean = P.fast;   // (the frame epilogue clears it again)
    }
    int *overflowFlag = P.heap ? W.heapFlag.p : reinterpret_cast<int *>(s->counters.p + 2 * C_COUNT) + 12;   // (else: a spare counter word, never set)
    // the enqueue, by the frame's shape
    FrameJob J{s, F, P, W, pose_view(s, F.pose), V, st, e0, e1, batch, d_out, d_outF32, tileCostDev, overflowFlag, P.fast};
    if ((rc = P.batch ? J.batch_frame() : (!P.adaptive ? J.plain_frame() : (P.adaptiveFast ? J.adaptive_in_flight() : J.adaptive_careful())))) return rc;
    if (!P.fast) HIPCHECK(hipEventRecord(F.done, st));
    HIPCHECK(hipGetLastError());
    F.pending = true;
    return XRT_OK;
}

// A frame in flight did not fit its optimistically sized buffers: it is rendered again the careful way, and frame_finish runs on the new attempt.
int redo_careful(xrt_scene *s, xrt_scene::FrameCtx &F, xrt_stats *stats) {
    F.tallyChunks = 0;
    const std::vector<xrt_light> lights = F.redoLights;
    const xrt_camera cam = F.redoCam;
    const xrt_render_opts opts = F.redoOpts;
    int rc = frame_begin(s, F, &cam, lights.data(), (int)lights.size(), &opts, F.redoOut, F.redoOutF32, F.redoSt);
    if (rc != XRT_OK) return rc;
    rc = frame_finish(s, F, stats);
    F.redone = true;
    return rc;
}

// Sizes of a finished single-chunk frame's generations (hc: its counters): grid hints for the next one (sizing only).
void update_grid_hints(xrt_scene *s, const FramePlan &P, const int *hc) {
    const int R = P.R;
    const bool same0 = s->genKey == P.hintPaths * 64 + P.nL && s->genHeap == P.heap;
    for (int k = 0; k <= R + 1 && k < 68; k++) {
        const long long closest = (k == 0 || ((P.heap || P.ae) && k <= R)) ? hc[k] : (k <= R ? gen_hits(hc, R, k - 1) : 0), shaded = k >= 1 ? gen_hits(hc, R, k - 1) : 0;
        // (a hint shrinks by an eighth per frame at most: a camera that looks away for a frame, or alternates between two views,
        // must not leave the next full view with a grid of sixteen blocks)
        const long long rays = closest + shaded * P.nL, work = closest > shaded ? closest : shaded;
        const long long keepR = same0 && s->genRays[k] > 0 ? s->genRays[k] - s->genRays[k] / 8 : 0, keepS = same0 && s->genShade[k] > 0 ? s->genShade[k] - s->genShade[k] / 8 : 0;
        s->genRays[k] = rays > keepR ? rays : keepR;
        s->genShade[k] = work > keepS ? work : keepS;
    }
    for (int k = R + 2; k < 68; k++) s->genRays[k] = s->genShade[k] = -1;
    {
        const long long listed = P.endEarly ? hc[P.cntStride] : -1, keep = same0 && s->genCompose > 0 ? s->genCompose - s->genCompose / 8 : 0;
        s->genCompose = listed < 0 ? -1 : (listed > keep ? listed : keep);
    }
    s->genKey = P.hintPaths * 64 + P.nL;
    s->genHeap = P.heap;
}

// Steer the "long ray" thresholds towards 2-6 % of each generation's rays (hc: a finished single-chunk frame's counters).
void steer_long_ray_thresholds(xrt_scene *s, const FramePlan &P, const int *hc) {
    const int R = P.R;
    for (int k = 0; k <= R && k < 66; k++) {
        const long long rays = k == 0 ? hc[0] : gen_hits(hc, R, k - 1), listed = hc[2 * (R + 2) + k];
        if (rays < 4096) continue;
        if (listed * 100 > rays * s->cfg.longFracHi) s->costT[k] = s->costT[k] + s->costT[k] / 4 + 1;
        else if (listed * 100 < rays * s->cfg.longFracLo && s->costT[k] > 1) s->costT[k] = s->costT[k] - s->costT[k] / 5 - (s->costT[k] < 5 ? 1 : 0);
        if (s->costT[k] < 1) s->costT[k] = 1;
        if (s->costT[k] > 60000) s->costT[k] = 60000;
    }
}

// Waits for a frame enqueued by frame_begin and turns its counters / events into xrt_stats.
int frame_finish(xrt_scene *s, xrt_scene::FrameCtx &F, xrt_stats *stats) {
    if (!F.pending) return fail(XRT_E_INVALID_ARG, "no frame in flight for this ticket");
    F.pending = false;
    const FramePlan &P = F.plan;
    HIPCHECK(hipEventSynchronize(P.fast ? F.events[1] : F.done));
    s->progress.store(1.0f);
    if (s->waveTimes.p) {   // development aid: launch k of the frame occupies rows [k*8192, (k+1)*8192) x 3 clocks
        std::vector<unsigned long long> h((size_t)16 * 3 * 8192);
        HIPCHECK(hipMemcpy(h.data(), s->waveTimes.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE *f = fopen(s->cfg.waveTimesPath.c_str(), "wb")) { fwrite(h.data(), sizeof(unsigned long long), h.size(), f); fclose(f); }
    }
    if (!s->cfg.stampDumpPath.empty() && F.stampRows > 0) {   // development aid (tools/stamp_lives.py)
        std::vector<unsigned long long> h((size_t)F.stampRows * STAMP_STRIDE);
        HIPCHECK(hipMemcpy(h.data(), F.w.stamps.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE *f = fopen(s->cfg.stampDumpPath.c_str(), "wb")) { fwrite(h.data(), sizeof(unsigned long long), h.size(), f); fclose(f); }
    }
    if (P.adaptiveFast && F.pinned.p[P.cntBase - 1] != 0) {
        // A quadrant level of the adaptive frame did not fit its optimistically sized buffers: the frame is rendered again the careful
        // way (a host read-back per level, exact sizes), and so are this scene's later adaptive frames from the start.
        s->adaptiveFastOk = false;
        return redo_careful(s, F, stats);
    }
    if (P.adaptiveFast) {   // rays of the frame: four per level-0 pixel and four per quadrant of every deeper level
        const int *lw = F.pinned.p;
        F.livePaths = F.validPixels * 4ull;
        for (int l = 1; l <= P.quality; l++) F.livePaths += 4ull * (unsigned long long)std::min(lw[l], P.levelCap);
    }
    if (P.heapFast && F.tallyChunks == 1 && F.pinned.p[P.cntStride] != 0) {
        // A generation of the ray tree did not fit the optimistically sized buffers: the frame is rendered again the careful way
        // (chunks, overflow checks, retries with fewer paths), and so are this scene's later ray-tree frames from the start.
        s->heapFastOk = false;
        return redo_careful(s, F, stats);
    }
    const int *const hc0 = F.pinned.p + P.cntBase;   // the first chunk's counters
    if (F.tallyChunks > 0) {   // single-pass frame: the read-back was left in flight
        const size_t nb = (size_t)F.tallyChunks * P.cntStride * sizeof(int);
        for (int c = 0; c < F.tallyChunks; c++) {
            const int *hc = hc0 + (size_t)c * P.cntStride;
            if (hc[0] < 0 || (size_t)hc[0] > P.liveCap)
                return fail(XRT_E_INTERNAL, "%d primary rays reach the scene but the frame's ray arrays were sized for %zu (screen rectangle of the root box)", hc[0], P.liveCap);
            if (P.endEarly && (hc[P.cntStride] < 0 || hc[P.cntStride] > hc[0]))
                return fail(XRT_E_INTERNAL, "%d paths on the compose list of a frame with %d live primary rays", hc[P.cntStride], hc[0]);
            tally_chunk(F, hc);
        }
#ifdef XRT_DEV
        if (s->cfg.finishCounts)   // (profiles/shade_finish: which share of a generation's hits part A finished; a frame not answered at emission emits every shadow ray)
            for (int k = 0, R = P.R; k <= R; k++)
                fprintf(stderr, "xrt finish: %s generation %d hits %lld finished %d shadow rays emitted %lld\n", P.ae ? "answered at emission," : "not answered at emission,", k,
                        gen_hits(hc0, R, k), hc0[4 * (R + 2) + k], P.ae ? (long long)hc0[3 * (R + 2) + k] : gen_hits(hc0, R, k) * (long long)P.nL);
#endif
        if (!P.fast) std::memcpy(F.hcnt, (char *)F.pinned.p + nb, sizeof(F.hcnt));
        // (adaptive frames in flight put the level-count words in front of the per-pass counters and have no hintPaths key: no hints from them)
        if (P.fast && F.tallyChunks == 1 && !P.adaptiveFast) update_grid_hints(s, P, hc0);
        if (P.fast && s->costMap.p && !P.adaptiveFast) steer_long_ray_thresholds(s, P, hc0);
        F.tallyChunks = 0;
    }
    if (P.endEarly) {   // (xrt_debug_end_counts: a frame that engaged has one chunk and its counters in `pinned`)
        s->endCounts[0] = (unsigned long long)hc0[P.cntStride + END_BY_RAYGEN] + P.endSkipped; s->endCounts[1] = (unsigned long long)hc0[P.cntStride + END_BY_SHADE]; s->endCounts[2] = (unsigned long long)hc0[P.cntStride + END_LISTED];
    } else s->endCounts[0] = s->endCounts[1] = s->endCounts[2] = 0;
    // (xrt_debug_packet_table: the table and the live list of a one-chunk frame stay in its context until the context's next frame)
    s->quadCtx = (P.pkEntries && P.firstPaths <= P.chunkPaths && (P.pkMask & 1) && !(P.adaptive && P.quality > 0)) ? (int)(&F - s->frames) : -1;
    s->quadLive = s->quadCtx >= 0 ? F.live0 : 0;
    {
        float frameMs = 0;
        if (hipEventElapsedTime(&frameMs, F.events[0], F.events[1]) == hipSuccess) s->lastFrameMs = frameMs;
        else (void)hipGetLastError();
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        unsigned long long hcnt[2 * C_COUNT];
        std::memcpy(hcnt, F.hcnt, sizeof(hcnt));
        if (P.collect) {
            // primary rays answered by k_raygen (they miss the scene root box): one query and one OSM:460 test each
            const unsigned long long culled = P.givenHits ? 0 : F.livePaths - F.live0;   // (given hits: generation 0 made no query)
            hcnt[C_RAYS] += culled;
            hcnt[C_SCENE_NODES] += culled;
        } else {
            std::memset(hcnt, 0, sizeof(hcnt));
            hcnt[C_RAYS] = P.givenHits ? F.closestDeep : F.livePaths + F.closestDeep;   // (given hits: the queries of generation >= 1)
            hcnt[C_HITS] = P.givenHits ? F.shaded - F.live0 : F.shaded;                 // (... and their hits: live0 = the entries that were shaded)
            hcnt[C_COUNT + C_RAYS] = F.shaded * (unsigned long long)P.nL;
        }
        fill_stats(stats, hcnt, F.shaded, F.validPixels);
        stats->rays_traversed = stats->rays_closest + stats->rays_shadow - (P.givenHits ? 0 : F.livePaths - F.live0) - F.answered;   // all but the primary rays k_raygen answered and the rays k_shade answered at emission
        if (!P.collect) stats->algorithmic_bytes = 0;   // needs the counting pass
        float ms = 0;
        HIPCHECK(hipEventElapsedTime(&ms, F.events[0], F.events[1]));
        stats->ms_total = ms;
        double mi = 0, longest = 0;
        for (auto &pr : F.pairs) {
            float t = 0;
            HIPCHECK(hipEventElapsedTime(&t, F.events[pr.first], F.events[pr.second]));
            mi += t;
            if (t > longest) longest = t;
        }
        for (int j = 0; j < F.stampRows; j++) {
            const unsigned long long *sp = F.stampHost.p;
            if (sp[2 * j + 1] > sp[2 * j]) {
                const double t = (double)(sp[2 * j + 1] - sp[2 * j]) / (double)s->wallClockKHz;
                mi += t;
                if (t > longest) longest = t;
            }
        }
        stats->ms_intersect = mi;
        stats->ms_intersect_longest = longest;
        stats->intersect_launches = (uint32_t)F.pairs.size() + (uint32_t)F.stampRows;
        stats->pieces = 1;
    }
    return XRT_OK;
}

// ---- in-library multi-GPU (xrt_render_opts.n_gpus) -----------------------------------------------------------------
constexpr int XRT_MAX_GPUS = 64;

int scene_upload(xrt_scene *scene);

// Copies of the scene on devices device+1 .. device+n-1 (the scene's own device in the single-GPU test mode).
int ensure_replicas(xrt_scene *s, int n) {
    while ((int)s->replicas.size() < n - 1) {
        const int i = (int)s->replicas.size() + 1;
        std::unique_ptr<xrt_scene> r(new xrt_scene());
        r->device = s->cfg.fakeGpus ? s->device : s->device + i;
        r->host = s->host;
        r->cfg = s->cfg;
        r->cfg.waveTimesPath.clear(); r->cfg.stampDumpPath.clear();   // (the dumps are the primary's: a replica's frames would overwrite its files)
        HIPCHECK(hipSetDevice(r->device));
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, r->device) == hipSuccess) r->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        if (hipDeviceGetAttribute(&r->wallClockKHz, hipDeviceAttributeWallClockRate, r->device) != hipSuccess) { r->wallClockKHz = 0; (void)hipGetLastError(); }
        int rc;
        if ((rc = r->stream.create()) || (rc = scene_upload(r.get()))) return rc;
        // the replica's version 0 holds the host's records: the primary's version 0 only while no pose was set since the build
        for (auto &v : r->pose) v.serial = ~0ull;
        if (s->poseSerial == 0) r->pose[0].serial = 0;
        // ... and the host's materials: the primary's CURRENT version (scene_upload read the host arrays); every frame's version arrives by replica_material
        for (auto &v : r->mat) v.serial = ~0ull;
        if (s->matCur == 0) r->mat[0].serial = s->mat[0].serial;
        // ... and the host's triangle values: the primary's version 0 only while none was set since `shade` was uploaded
        for (auto &v : r->shadeVer) v.serial = ~0ull;
        if (s->shadeSerial == 0) r->shadeVer[0].serial = 0;
        s->workers.emplace_back(new RankWorker(r->device));
        s->replicas.push_back(std::move(r));
    }
    return hipSetDevice(s->device) == hipSuccess ? XRT_OK : fail(XRT_E_HIP, "hipSetDevice failed");
}

xrt_scene *rank_scene(xrt_scene *s, int i) { return i == 0 ? s : s->replicas[(size_t)i - 1].get(); }

// Install / remove a tile table on one scene object (its device must be current).  Caller has checked the table.
int install_tile_table(xrt_scene *r, int w, int h, int count, int tpr, const int *table) {
    if (!table) { r->tileTable.clear(); r->tableW = r->tableH = r->tableCount = r->tableTpr = 0; return XRT_OK; }
    r->tileTable.assign(table, table + (size_t)count * tpr);
    int rc = upload(r->tileTableDev, r->tileTable);
    if (rc != XRT_OK) { r->tileTable.clear(); return rc; }
    r->tableW = w; r->tableH = h; r->tableCount = count; r->tableTpr = tpr;
    return XRT_OK;
}
// The costs of this scene object's tiles, added to cost[tile] (tiles entries); optionally cleared.  Its device must be current, no frame in flight.
int read_tile_costs(xrt_scene *r, int w, int h, float *cost, bool reset) {
    if (r->costW != w || r->costH != h || r->costTiles.empty() || !r->tileCost.p) return XRT_OK;
    std::vector<unsigned> ticks(r->costTiles.size());
    HIPCHECK(hipMemcpy(ticks.data(), r->tileCost.p, ticks.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    const int tiles = ((w + XRT_TILE_W - 1) / XRT_TILE_W) * ((h + XRT_TILE_H - 1) / XRT_TILE_H);
    for (size_t sl = 0; sl < ticks.size(); sl++) { const int t = r->costTiles[sl]; if (t >= 0 && t < tiles) cost[t] += (float)ticks[sl]; }
    if (reset) HIPCHECK(hipMemset(r->tileCost.p, 0, ticks.size() * sizeof(unsigned)));
    return XRT_OK;
}

// Replica r renders version v of the primary's poses: copied from the primary's version v when r's copy is of another write.
// Stream-ordered on r's stream behind the primary's write; the replica's frame waits for the copy (frame_begin, pose_wait).
int replica_pose(xrt_scene *s, xrt_scene *r, int v) {
    xrt_scene::PoseVer &P = s->pose[v], &R = r->pose[v];
    if (R.serial == P.serial) return XRT_OK;
    const size_t nObj = s->host->arrays.objects.size(), nCull = s->host->arrays.scull.size();
    int rc;
    HIPCHECK(hipSetDevice(r->device));
    if (v != 0 && ((rc = R.objects.ensure(nObj)) || (rc = R.scull.ensure(nCull)))) return rc;
    if (P.ready) HIPCHECK(hipStreamWaitEvent(r->stream, P.ready, 0));
    if (r->device == s->device) {
        HIPCHECK(hipMemcpyAsync(pose_objects(r, v), pose_objects(s, v), nObj * sizeof(ObjRec), hipMemcpyDeviceToDevice, r->stream));
        HIPCHECK(hipMemcpyAsync(pose_scull(r, v), pose_scull(s, v), nCull * sizeof(f4), hipMemcpyDeviceToDevice, r->stream));
    } else {
        HIPCHECK(hipMemcpyPeerAsync(pose_objects(r, v), r->device, pose_objects(s, v), s->device, nObj * sizeof(ObjRec), r->stream));
        HIPCHECK(hipMemcpyPeerAsync(pose_scull(r, v), r->device, pose_scull(s, v), s->device, nCull * sizeof(f4), r->stream));
    }
    if ((rc = R.ready.create())) return rc;
    HIPCHECK(hipEventRecord(R.ready, r->stream));
    R.serial = P.serial;
    return XRT_OK;
}

// Replica r renders version v of the primary's materials: its MaterialRecs, its texel arena and its anyTransparent, copied when r's copy is of
// another write -- the route replica_pose takes.
int replica_material(xrt_scene *s, xrt_scene *r, int v) {
    xrt_scene::MatVer &P = s->mat[v], &R = r->mat[v];
    if (R.serial == P.serial) return XRT_OK;
    const size_t nMat = s->host->arrays.materials.size(), nTex = P.texCount;
    int rc;
    if (P.pending) {   // (the primary's own copies: its frame is enqueued after its replicas' copies are)
        HIPCHECK(hipSetDevice(s->device));
        if ((rc = s->matStream.create()) || (rc = mat_acquire(s, v, s->matStream))) return rc;
    }
    HIPCHECK(hipSetDevice(r->device));
    if ((rc = mat_records(r, v).ensure(nMat)) || (rc = mat_texel_room(r, mat_texels(r, v), nTex))) return rc;
    if (P.ready) HIPCHECK(hipStreamWaitEvent(r->stream, P.ready, 0));
    if (r->device == s->device) {
        HIPCHECK(hipMemcpyAsync(mat_records(r, v).p, mat_records(s, v).p, nMat * sizeof(MaterialRec), hipMemcpyDeviceToDevice, r->stream));
        HIPCHECK(hipMemcpyAsync(mat_texels(r, v).p, mat_texels(s, v).p, nTex * sizeof(uint32_t), hipMemcpyDeviceToDevice, r->stream));
    } else {
        HIPCHECK(hipMemcpyPeerAsync(mat_records(r, v).p, r->device, mat_records(s, v).p, s->device, nMat * sizeof(MaterialRec), r->stream));
        HIPCHECK(hipMemcpyPeerAsync(mat_texels(r, v).p, r->device, mat_texels(s, v).p, s->device, nTex * sizeof(uint32_t), r->stream));
    }
    if ((rc = R.ready.create())) return rc;
    HIPCHECK(hipEventRecord(R.ready, r->stream));
    R.owner = r->stream;
    R.serial = P.serial; R.anyTransparent = P.anyTransparent; R.texCount = nTex;
    return XRT_OK;
}

// Replica r renders version v of the primary's triangle values: its `shade` array, copied when r's copy is of another write -- the route
// replica_pose takes.
int replica_triangle_shading(xrt_scene *s, xrt_scene *r, int v) {
    xrt_scene::ShadeVer &P = s->shadeVer[v], &R = r->shadeVer[v];
    if (R.serial == P.serial) return XRT_OK;
    const size_t n = s->shadeCount;
    int rc;
    HIPCHECK(hipSetDevice(r->device));
    if ((rc = shade_records(r, v).ensure(n))) return rc;
    if (P.ready) HIPCHECK(hipStreamWaitEvent(r->stream, P.ready, 0));
    if (r->device == s->device) HIPCHECK(hipMemcpyAsync(shade_records(r, v).p, shade_records(s, v).p, n * sizeof(f4), hipMemcpyDeviceToDevice, r->stream));
    else HIPCHECK(hipMemcpyPeerAsync(shade_records(r, v).p, r->device, shade_records(s, v).p, s->device, n * sizeof(f4), r->stream));
    if ((rc = R.ready.create())) return rc;
    HIPCHECK(hipEventRecord(R.ready, r->stream));
    R.serial = P.serial;
    return XRT_OK;
}

// Frame `slot` on n devices: rank i renders the tiles t with t % n == i (its own frame context `slot`, its own stream, one
// host thread per device so that frames which need host decisions between passes still run side by side), then ONE
// grouped RCCL exchange moves the tile buffers to rank 0 -- the path's only exchange step -- and k_detile writes the
// W*H frame into d_out on the scene's device.  Everything after the enqueue is stream-ordered on rank 0's stream.
int multi_begin(xrt_scene *s, int slot, const xrt_camera *cam, const xrt_light *lights, int nLights, const xrt_render_opts *opts, uint32_t *d_out,
                hipStream_t *stream0_out) {
    const int n = opts->n_gpus;
    if (opts->shard_count > 1) return fail(XRT_E_INVALID_ARG, "n_gpus > 1 shards the frame inside the library: shard_count must be 0 or 1");
    if (n > XRT_MAX_GPUS) return fail(XRT_E_INVALID_ARG, "n_gpus %d exceeds %d", n, XRT_MAX_GPUS);
    if (!cam || cam->vp_width <= 0 || cam->vp_height <= 0) return fail(XRT_E_INVALID_ARG, "viewport must be positive");
    if (!s->cfg.fakeGpus && s->device + n > s->visibleDevices)
        return fail(XRT_E_NO_DEVICE, "n_gpus %d from device %d needs %d visible devices, %d present", n, s->device, s->device + n, s->visibleDevices);
    int rc;
    if ((rc = ensure_replicas(s, n))) return rc;
    {
        std::vector<int> devs;
        if (s->cfg.fakeGpus) devs.push_back(s->device);
        else for (int i = 0; i < n; i++) devs.push_back(s->device + i);
        std::string err;
        if (!s->rccl.init(devs, err)) return fail(XRT_E_RCCL, "%s", err.c_str());
        HIPCHECK(hipSetDevice(s->device));
    }
    int tpr = 0, tilesX = 0, tilesY = 0;
    xrt_shard_layout(cam->vp_width, cam->vp_height, n, &tilesX, &tilesY, &tpr);
    // balance_tiles: the tiles are dealt by the last frame's costs (longest first) instead of round-robin -- the static counterpart of the
    // reference's dynamic row stealing (RT:48-52).  The table is made once per frame here and installed on every rank's scene object.
    const bool balanced = opts->balance_tiles != 0 && s->balanceW == cam->vp_width && s->balanceH == cam->vp_height && s->balanceN == n &&
                          (int)s->balanceCost.size() == tilesX * tilesY && !s->frames[slot ^ 1].pending;
    const bool tableFits = s->tableW == cam->vp_width && s->tableH == cam->vp_height && s->tableCount == n && !s->tileTable.empty();
    if (balanced) {
        const int tprB = tpr + (tpr + 3) / 4;
        std::vector<int> table((size_t)n * tprB);
        if ((rc = balance_tiles_impl(tilesX * tilesY, n, s->balanceCost.data(), tprB, table.data()))) return rc;
        for (int i = 0; i < n; i++) {
            xrt_scene *r = rank_scene(s, i);
            HIPCHECK(hipSetDevice(r->device));
            if ((rc = install_tile_table(r, cam->vp_width, cam->vp_height, n, tprB, table.data()))) { (void)hipSetDevice(s->device); return rc; }
        }
        HIPCHECK(hipSetDevice(s->device));
        tpr = tprB;
    } else if (opts->balance_tiles != 0 && tableFits) tpr = s->tableTpr;   // (the other ticket's frame is in flight under the installed table: keep it)
    else if (tableFits && opts->balance_tiles == 0) {   // back to round-robin
        for (int i = 0; i < n; i++) (void)install_tile_table(rank_scene(s, i), 0, 0, 0, 0, nullptr);
    }
    const bool tabled = s->tableW == cam->vp_width && s->tableH == cam->vp_height && s->tableCount == n && !s->tileTable.empty();
    const size_t count = (size_t)tpr * 512;
    if ((rc = s->gathered[slot].ensure(count * (size_t)n))) return rc;
    for (int i = 1; i < n; i++) {
        xrt_scene *r = rank_scene(s, i);
        HIPCHECK(hipSetDevice(r->device));
        if ((rc = r->tileOut[slot].ensure(count))) { (void)hipSetDevice(s->device); return rc; }
        if (s->cfg.fakeGpus && (rc = r->tilesReady[slot].create())) return rc;
    }
    for (int i = 1; i < n; i++)
        if ((rc = replica_pose(s, rank_scene(s, i), s->slotPose[slot])) || (rc = replica_material(s, rank_scene(s, i), s->slotMat[slot])) ||
            (rc = replica_triangle_shading(s, rank_scene(s, i), s->slotShade[slot]))) { (void)hipSetDevice(s->device); return rc; }
    HIPCHECK(hipSetDevice(s->device));
    // every device's share is enqueued by its own (persistent) host thread
    std::vector<int> rcs((size_t)n, XRT_OK);
    std::vector<std::string> errs((size_t)n);
    auto work_body = [&](int i) {
        xrt_scene *r = rank_scene(s, i);
        if (hipSetDevice(r->device) != hipSuccess) { rcs[(size_t)i] = XRT_E_HIP; errs[(size_t)i] = "hipSetDevice failed"; return; }
        xrt_render_opts o = *opts;
        o.n_gpus = 0; o.shard_rank = i; o.shard_count = n;
        uint32_t *dst = i == 0 ? s->gathered[slot].p : r->tileOut[slot].p;
        r->frames[slot].pose = s->slotPose[slot];   // (every rank renders the primary's versions)
        r->frames[slot].mat = s->slotMat[slot];
        r->frames[slot].shade = s->slotShade[slot];
        rcs[(size_t)i] = frame_begin(r, r->frames[slot], cam, lights, nLights, &o, dst, nullptr, nullptr, 0, 1, false);   // (the gather is enqueued behind the frame: no redo)
        if (rcs[(size_t)i] != XRT_OK) errs[(size_t)i] = g_err;
    };
    // (a rank's job must not throw -- on a worker thread that is std::terminate, on this one it would unwind past workers that still
    // use the locals above: an exception becomes that rank's error code, and every posted worker is waited for whatever happens)
    auto work = [&](int i) {
        try { work_body(i); }
        catch (const std::bad_alloc &) { rcs[(size_t)i] = XRT_E_OOM; errs[(size_t)i] = "out of host memory"; }
        catch (const std::exception &e) { rcs[(size_t)i] = XRT_E_INTERNAL; errs[(size_t)i] = e.what(); }
        catch (...) { rcs[(size_t)i] = XRT_E_INTERNAL; errs[(size_t)i] = "unknown exception"; }
    };
    {
        int posted = 0;
        struct WaitAll {
            xrt_scene *s; int &posted;
            ~WaitAll() { for (int i = 0; i < posted; i++) s->workers[(size_t)i]->wait(); }
        } waitAll{s, posted};
        for (int i = 1; i < n; i++) { s->workers[(size_t)i - 1]->post([&work, i] { work(i); }); posted = i; }
        work(0);
    }
    // From here on frames are in flight on the ranks: whatever fails, every rank's frame is waited for before the error is
    // reported -- a ticket that was never handed out must not leave a context pending (later renders would be XRT_E_BUSY).
    auto drain = [&]() {
        for (int j = 0; j < n; j++) {
            xrt_scene *r = rank_scene(s, j);
            if (r->frames[slot].pending) { (void)hipSetDevice(r->device); (void)frame_finish(r, r->frames[slot], nullptr); }
        }
        (void)hipSetDevice(s->device);
    };
    auto tail = [&]() -> int {
        HIPCHECK(hipSetDevice(s->device));
        for (int i = 0; i < n; i++)
            if (rcs[(size_t)i] != XRT_OK) return fail(rcs[(size_t)i], "rank %d: %s", i, errs[(size_t)i].c_str());
        hipStream_t st0 = s->frames[slot].w.lastStream;
        std::vector<const void *> src;
        std::vector<int> srcRank;
        std::vector<hipStream_t> srcStream;
        std::vector<void *> dst;
        for (int i = 1; i < n; i++) {
            xrt_scene *r = rank_scene(s, i);
            hipStream_t sti = r->frames[slot].w.lastStream;
            if (s->cfg.fakeGpus) {   // same device, one communicator: rank 0's stream waits for the tiles, then sends to itself
                HIPCHECK(hipEventRecord(r->tilesReady[slot], sti));
                HIPCHECK(hipStreamWaitEvent(st0, r->tilesReady[slot], 0));
                sti = st0;
            }
            src.push_back(r->tileOut[slot].p); srcRank.push_back(s->cfg.fakeGpus ? 0 : i); srcStream.push_back(sti);
            dst.push_back(s->gathered[slot].p + (size_t)i * count);
        }
        {
            std::string err;
            if (!s->rccl.gather(src, srcRank, srcStream, dst, count, st0, err)) return fail(XRT_E_RCCL, "%s", err.c_str());
        }
        HIPCHECK(hipSetDevice(s->device));
        launch_detile(cam->vp_width, cam->vp_height, n, tpr, s->gathered[slot].p, (long long)count, d_out, st0, tabled ? s->tileTableDev.p : nullptr);
        HIPCHECK(hipGetLastError());
        *stream0_out = st0;
        return XRT_OK;
    };
    rc = tail();
    if (rc != XRT_OK) { const std::string keep = g_err; drain(); g_err = keep; }
    return rc;
}

// Counters add up over the pieces of a frame (ranks, halves); times are the slowest piece's (the frame's critical path).
void add_stats(xrt_stats &acc, const xrt_stats &st, bool first) {
    uint64_t *a = reinterpret_cast<uint64_t *>(&acc);
    const uint64_t *b = reinterpret_cast<const uint64_t *>(&st);
    for (size_t k = 0; k < offsetof(xrt_stats, ms_total) / sizeof(uint64_t); k++) a[k] += b[k];
    if (st.ms_total > acc.ms_total) acc.ms_total = st.ms_total;
    if (st.ms_intersect > acc.ms_intersect) acc.ms_intersect = st.ms_intersect;
    if (st.ms_intersect_longest > acc.ms_intersect_longest) acc.ms_intersect_longest = st.ms_intersect_longest;
    if (first) acc.intersect_launches = st.intersect_launches;
    acc.pieces += 1;
    acc.rays_traversed += st.rays_traversed;
    acc.mesh_queries_facing_away += st.mesh_queries_facing_away;
}

int multi_end(xrt_scene *s, int slot, int n, xrt_stats *stats, bool balance) {
    int rc = XRT_OK;
    xrt_stats acc;
    std::memset(&acc, 0, sizeof(acc));
    for (int i = 0; i < n; i++) {
        xrt_scene *r = rank_scene(s, i);
        if (hipSetDevice(r->device) != hipSuccess) { rc = fail(XRT_E_HIP, "hipSetDevice failed"); continue; }
        xrt_stats st;
        std::memset(&st, 0, sizeof(st));
        const int rci = frame_finish(r, r->frames[slot], &st);
        if (rci != XRT_OK) { rc = rci; continue; }
        add_stats(acc, st, i == 0);
    }
    if (rc == XRT_OK && balance && !s->frames[slot ^ 1].pending) {   // this frame's tile costs, all ranks: what the next frame's table is made from
        const xrt_scene::FrameCtx &F0 = s->frames[slot];
        const int w = F0.plan.g.width, h = F0.plan.g.height;
        const int tiles = ((w + XRT_TILE_W - 1) / XRT_TILE_W) * ((h + XRT_TILE_H - 1) / XRT_TILE_H);
        std::vector<float> cost((size_t)tiles, 0.0f);
        bool ok = w > 0 && h > 0;
        for (int i = 0; ok && i < n; i++) {
            xrt_scene *r = rank_scene(s, i);
            ok = hipSetDevice(r->device) == hipSuccess && read_tile_costs(r, w, h, cost.data(), true) == XRT_OK;
        }
        if (ok) { s->balanceCost.swap(cost); s->balanceW = w; s->balanceH = h; s->balanceN = n; }
    }
    (void)hipSetDevice(s->device);
    if (rc == XRT_OK && stats) *stats = acc;
    return rc;
}

// ---- one ticket: frame (on one or n GPUs) -> optional copy into the host's Color[] (RT:122-123) -------------------------
// d_out: the W*H frame in HBM (or this process's tile shard), or null when the frame is only wanted on the host (the
// library then keeps it in a buffer of the ticket).  host_out: page-locked or pageable host memory, or null.
int open_frame_impl(xrt_scene *s, int slot, const xrt_camera *cam, const xrt_light *lights, int nLights, const xrt_render_opts *opts, uint32_t *d_out,
                    float *d_outF32, uint32_t *host_out, hipStream_t st) {
    if (!cam || !opts) return fail(XRT_E_INVALID_ARG, "xrt_render: null argument");
    Range rf("xrt frame (ticket %d)", slot);
    if (opts->n_gpus < 0) return fail(XRT_E_INVALID_ARG, "n_gpus must not be negative");
    const int n = opts->n_gpus > 1 ? opts->n_gpus : 1;
    if (n > 1 && d_outF32) return fail(XRT_E_UNSUPPORTED, "rgb_f32_out with n_gpus > 1");
    const size_t px = (size_t)(cam->vp_width > 0 ? cam->vp_width : 0) * (size_t)(cam->vp_height > 0 ? cam->vp_height : 0);
    int rc;
    if (!d_out) {
        if (opts->shard_count > 1) return fail(XRT_E_INVALID_ARG, "a host frame is a whole frame; use xrt_render_device for shards");
        if ((rc = s->frameOut[slot].ensure(px ? px : 1))) return rc;
        d_out = s->frameOut[slot].p;
    }
    hipStream_t st0 = nullptr;
    int nParts = 1;
    s->slotPose[slot] = s->poseCur;   // the frame renders the poses and materials set before its begin, whatever is set while it is open
    s->slotMat[slot] = s->matCur;
    s->slotShade[slot] = s->shadeCur;
    struct PoseRelease {   // (an open that fails leaves no ticket)
        xrt_scene *s; int slot; bool keep = false;
        ~PoseRelease() { if (!keep) s->slotPose[slot] = s->slotMat[slot] = s->slotShade[slot] = -1; }
    } poseRelease{s, slot};
    for (int j = 0; j < 4; j++) { s->frames[slot + 2 * j].pose = s->poseCur; s->frames[slot + 2 * j].mat = s->matCur; s->frames[slot + 2 * j].shade = s->shadeCur; }
    if (n == 1) {
        // Two halves on two streams?  Only plain single-pass frames that run long enough for the drain of their launches to
        // matter, on streams of the library's choosing; by default only when no other frame is in flight to fill the gaps.
        const bool plain = opts->use_multisampling != XRT_MS_ADAPTIVE && !(s->mat[s->matCur].anyTransparent && opts->max_reflections > 0) && !opts->collect_stats;
        const long long px64 = (long long)px * (opts->use_multisampling == XRT_MS_FIXED16 ? 16 : 1) / (opts->shard_count > 1 ? opts->shard_count : 1);
        const bool alone = !s->frames[slot ^ 1].pending;
        if (!st && plain && !s->cfg.oneStream && s->cfg.splitMode.value_or(1) > 0 && (s->cfg.splitMode || s->sceneMode == MODE_SCENE) && (s->cfg.splitMode == 2 || alone) && s->lastFrameMs >= s->cfg.splitMinMs &&
            s->lastFrameMs >= s->cfg.overlapMinMs && px64 >= 8 * 8192 && px64 <= (long long)s->cfg.maxChunkPaths)
            nParts = s->cfg.splitParts;
        for (int j = 0; j < nParts; j++)
            if ((rc = frame_begin(s, s->frames[slot + 2 * j], cam, lights, nLights, opts, d_out, d_outF32, st, j, nParts))) {
                for (int i = 0; i < j; i++) (void)frame_finish(s, s->frames[slot + 2 * i], nullptr);
                return rc;
            }
        st0 = s->frames[slot].w.lastStream;
    } else if ((rc = multi_begin(s, slot, cam, lights, nLights, opts, d_out, &st0))) return rc;
    xrt_scene::OpenFrame &O = s->open[slot];
    O.nGpus = n; O.balance = n > 1 && opts->balance_tiles != 0;
    O.nParts = nParts;
    O.tail = n > 1 || host_out != nullptr;
    O.hostOut = host_out; O.devOut = d_out; O.px = px; O.st0 = st0;
    if (O.tail) {   // work enqueued behind the frame's own kernels: its end is an event of its own
        for (int j = 1; j < nParts; j++) {   // (the other half ends with an event on its last kernel)
            xrt_scene::FrameCtx &Fj = s->frames[slot + 2 * j];
            HIPCHECK(hipStreamWaitEvent(st0, Fj.plan.fast ? Fj.events[1] : Fj.done, 0));
        }
        if (host_out && px) HIPCHECK(hipMemcpyAsync(host_out, d_out, px * sizeof(uint32_t), hipMemcpyDeviceToHost, st0));   // CurrentTarget.SetData (RT:123)
        if ((rc = s->tailDone[slot].create())) return rc;
        HIPCHECK(hipEventRecord(s->tailDone[slot], st0));
    }
    poseRelease.keep = true;
    return XRT_OK;
}

int close_frame_impl(xrt_scene *s, int slot, xrt_stats *stats) {
    xrt_scene::OpenFrame &O = s->open[slot];
    int rc = XRT_OK;
    if (O.nGpus > 1) rc = multi_end(s, slot, O.nGpus, stats, O.balance);
    else if (O.nParts <= 1) {
        rc = frame_finish(s, s->frames[slot], stats);
        if (rc == XRT_OK && s->frames[slot].redone && O.tail && O.hostOut && O.px) {   // the copy enqueued behind the first attempt took the wrong pixels
            hipError_t e = hipEventSynchronize(s->tailDone[slot]);
            if (e == hipSuccess) e = hipMemcpyAsync(O.hostOut, O.devOut, O.px * sizeof(uint32_t), hipMemcpyDeviceToHost, s->frames[slot].w.lastStream);
            if (e == hipSuccess) e = hipEventRecord(s->tailDone[slot], s->frames[slot].w.lastStream);
            if (e != hipSuccess) rc = fail(XRT_E_HIP, "redo of a ray-tree frame: %s", hipGetErrorString(e));
        }
    }
    else {
        xrt_stats acc;
        std::memset(&acc, 0, sizeof(acc));
        for (int j = 0; j < O.nParts; j++) {
            xrt_stats st;
            std::memset(&st, 0, sizeof(st));
            const int rcj = frame_finish(s, s->frames[slot + 2 * j], &st);
            if (rcj != XRT_OK) rc = rcj;
            else add_stats(acc, st, j == 0);
        }
        if (rc == XRT_OK && stats) *stats = acc;
    }
    if (O.tail) {
        const hipError_t e = hipEventSynchronize(s->tailDone[slot]);
        if (e != hipSuccess && rc == XRT_OK) rc = fail(XRT_E_HIP, "hipEventSynchronize: %s", hipGetErrorString(e));
    }
    O = xrt_scene::OpenFrame();
    s->slotPose[slot] = s->slotMat[slot] = s->slotShade[slot] = -1;
    if (rc == XRT_OK) rc = guards_check("end of frame");
    return rc;
}

// Split walks (packet.hip): the arena of a context's packet launches and this launch's control words (they sit behind the queue heads and are cleared with them).
// The arena is cleared once, when it is made: an item counts as written when its first word holds the launch's serial number.
int split_arena(xrt_scene *s, DevBuf<unsigned> &items, DevBuf<unsigned> &recs, PacketArgs &PA, hipStream_t st) {
    int rc;
    const size_t NI = ((size_t)s->cfg.packetSplitItems + 7) / 8 * 8, NR = NI / 4 + 1;   // (an eighth of the items per XCD)
    if (!items.p || items.cap < NI * SPLIT_ITEM_WORDS) {
        if ((rc = items.ensure(NI * SPLIT_ITEM_WORDS)) || (rc = recs.ensure(NR * SPLIT_REC_WORDS))) return rc;
        HIPCHECK(hipMemsetAsync(items.p, 0, NI * SPLIT_ITEM_WORDS * sizeof(unsigned), st));
        HIPCHECK(hipMemsetAsync(recs.p, 0, NR * SPLIT_REC_WORDS * sizeof(unsigned), st));
    }
    PA.splitItems = items.p; PA.splitRecs = recs.p; PA.splitNI = (int)NI; PA.splitNR = (int)NR;
    if (++s->splitSerial == 0u) s->splitSerial = 1u;
    PA.splitSerial = s->splitSerial;
    PA.splitBudget = std::max(1, s->cfg.packetBudgetUs * 100); PA.splitBudgetItem = std::max(1, s->cfg.packetBudgetItemUs * 100);   // ticks of the 100 MHz device clock (0 would mean "off")
    PA.splitCtl = reinterpret_cast<unsigned *>((reinterpret_cast<uintptr_t>(PA.queue + PACKET_QUEUE_HEADS * PACKET_HEAD_STRIDE) + 127) & ~(uintptr_t)127);
    return XRT_OK;
}

// The work-queue word of launches on `st` (launches of one stream are ordered, so they can share a word; launches on
// different streams may overlap and must not).  Caller holds apiMutex.
int queue_word_for(xrt_scene *s, hipStream_t st, unsigned **word) {
    constexpr size_t MAX_STREAMS = 1024;
    int rc;
    if ((rc = s->queues.ensure(MAX_STREAMS * (1 + PACKET_QUEUE_WORDS)))) return rc;
    auto it = s->queueOfStream.find(st);
    if (it == s->queueOfStream.end()) {
        if (s->queueOfStream.size() >= MAX_STREAMS) return fail(XRT_E_UNSUPPORTED, "xrt_scene_intersect_device: more than %zu distinct streams on one scene", MAX_STREAMS);
        it = s->queueOfStream.emplace(st, (int)s->queueOfStream.size()).first;
    }
    *word = s->queues.p + (size_t)it->second * (1 + PACKET_QUEUE_WORDS);   // word 0: k_intersect's queue head, then k_packet's heads
    return XRT_OK;
}

// THE traversal launch of a list call that traces outside a frame (xrt_trace_pixels, xrt_light_hits): the launch a frame of the scene would make for the same
// population.  A: the population, filled but for the scheduling knobs; packets: it takes the wave-packet kernel (a bit of scene_packet_mask) -- with the table
// `quads` where one was written for it and the split arena (items, recs) where walks are split --, else the per-lane kernel; cap: the host's bound of the ray count,
// which sizes the grid; e0 / e1: the events the launch carries.
int launch_list_traversal(xrt_scene *s, const SceneView &S, IntersectArgs &A, bool packets, const QuadTable *quads, DevBuf<unsigned> &items, DevBuf<unsigned> &recs,
                          long long cap, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    set_knobs(A, s);
    if (!packets) { launch_intersect(S, A, s->stackNeeded, persistent_grid(s, cap), st, e0, e1); return XRT_OK; }
    PacketArgs PA = packet_args(s, A, nullptr, quads);
    if (s->cfg.packetSplit && s->sceneMode != MODE_SCENE)
        if (int rc = split_arena(s, items, recs, PA, st)) return rc;
    launch_packet(S, PA, packet_grid(s, s->blocksPerCUPacket, cap), st, e0, e1);
    return XRT_OK;
}

// Caller holds apiMutex.
// (t0 / t1: events the traversal launch carries where no stats are asked for -- xrt_trace_pixels times its chunks itself)
int run_intersect(xrt_scene *s, const xrt_ray *d_rays, int64_t n, xrt_hit *d_hits, int mode, int meshId, hipStream_t st, xrt_stats *stats,
                  bool sync, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr) {
    if (n > 0x7fffffff / 2) return fail(XRT_E_INVALID_ARG, "too many rays in one call");
    int rc;
    unsigned *queue = nullptr;
    if ((rc = queue_word_for(s, st, &queue)) || (rc = s->counters.ensure(2 * C_COUNT + 8))) return rc;
    // the reference-work counters are shared with the frames' counting pass: exact counts need the scene to itself
    if (stats && in_flight(s)) return fail(XRT_E_BUSY, "xrt_scene_intersect with stats while a render is in flight");
    HIPCHECK(hipMemsetAsync(queue, 0, (1 + PACKET_QUEUE_WORDS) * sizeof(unsigned), st));
    IntersectArgs A;
    A.rays = d_rays; A.hits = d_hits; A.index = nullptr; A.nDev = nullptr; A.nMul = 1; A.n = (int)n; A.nCap = 0; A.queue = queue; A.mode = mode; A.meshId = meshId;
    set_knobs(A, s);
    hipEvent_t a0 = t0, a1 = t1;
    if (stats) {
        a0 = get_event(s, 0); a1 = get_event(s, 1);
        if (!a0 || !a1) return fail(XRT_E_HIP, "hipEventCreate failed");
        HIPCHECK(hipMemsetAsync(s->counters.p, 0, 2 * C_COUNT * sizeof(unsigned long long), st));
    }
    const SceneView S = pose_view(s, s->poseCur);   // seam 1 reads the latest poses
    if ((rc = pose_wait(s, s->poseCur, st))) return rc;
    const bool meshOk = mode != MODE_MESH || (meshId >= 0 && meshId < (int)s->host->meshTrees.size() && !s->host->meshTrees[(size_t)meshId].rootIsLeaf);
    if (n > 0 && s->cfg.packetMask >= 0 && (s->cfg.packetMask & 8) && packet_supported(mode, s->host->arrays.meshDepth, s->host->arrays.sceneDepth) && meshOk) {   // (testing aid: arbitrary batches through the packet kernel)
        PacketArgs PA = packet_args(s, A);
        if (s->cfg.packetSplit && mode != MODE_SCENE) {
            auto &ar = s->apiSplit[(int)((queue - s->queues.p) / (1 + PACKET_QUEUE_WORDS))];
            if ((rc = split_arena(s, ar.first, ar.second, PA, st))) return rc;
        }
        launch_packet(S, PA, packet_grid(s, packet_blocks_per_cu(mode), n), st, a0, a1);   // (the grid of the call's own mode: xrt_mesh_intersect is MODE_MESH whatever the scene)
    } else if (n > 0) launch_intersect(S, A, s->stackNeeded, persistent_grid(s, n), st, a0, a1);
    if (stats) {
        if (n > 0) launch_count(S, A, s->counters.p, st);
    }
    HIPCHECK(hipGetLastError());
    if (sync || stats) HIPCHECK(hipStreamSynchronize(st));
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        unsigned long long hcnt[2 * C_COUNT];
        HIPCHECK(hipMemcpy(hcnt, s->counters.p, sizeof(hcnt), hipMemcpyDeviceToHost));
        fill_stats(stats, hcnt, 0, 0);
        stats->rays_traversed = stats->rays_closest + stats->rays_shadow;
        float ms = 0;
        if (n > 0) HIPCHECK(hipEventElapsedTime(&ms, a0, a1));
        stats->ms_total = ms; stats->ms_intersect = ms; stats->ms_intersect_longest = ms; stats->intersect_launches = n > 0 ? 1 : 0;
    }
    return XRT_OK;
}

// RayTracer.CastRay (RT:506-737) on n rays already in HBM: the pass of frame_begin with the batch as its ray source, MaxReflections - iteration
// generations deep, then the pass's counters.  The caller holds the scene (BusyGuard, no frame in flight).
// What is wrong with the opts of a ray batch alone (fn: the entry point the messages name).
int batch_check_opts(const char *fn, const xrt_render_opts *opts, int32_t iteration) {
    if (!opts) return fail(XRT_E_INVALID_ARG, "%s: null opts", fn);
    if (opts->use_multisampling != XRT_MS_OFF) return fail(XRT_E_INVALID_ARG, "%s: use_multisampling must be XRT_MS_OFF (one ray, one colour)", fn);
    if (opts->shard_count < 0 || opts->shard_count > 1) return fail(XRT_E_INVALID_ARG, "%s: shard_count must be 0 or 1", fn);
    if (opts->n_gpus < 0 || opts->n_gpus > 1) return fail(XRT_E_INVALID_ARG, "%s: n_gpus must be 0 or 1", fn);
    if (opts->max_reflections < 0) return fail(XRT_E_INVALID_ARG, "max_reflections out of range");
    // CastRay(.., iteration, ..) reflects while iteration < MaxReflections (RT:545): a frame's recursion of max(0, M - iteration) generations
    const long long depth = std::max(0LL, (long long)opts->max_reflections - (long long)iteration);
    if (depth > 64) return fail(XRT_E_INVALID_ARG, "%s: max_reflections - iteration = %lld is above 64", fn, depth);
    if (opts->list_order != XRT_LIST_UNORDERED && opts->list_order != XRT_LIST_COHERENT) return fail(XRT_E_INVALID_ARG, "%s: list_order must be XRT_LIST_UNORDERED or XRT_LIST_COHERENT", fn);
    return XRT_OK;
}

// (d_hits, xrt_shade_hits: the closest hits of the rays, n xrt_hit in HBM -- generation 0 is not traced)
int cast_rays_impl(xrt_scene *s, const xrt_ray *d_rays, int64_t n, int32_t iteration, float refIndex, const xrt_light *lights, int32_t nLights,
                   const xrt_render_opts *opts, uint32_t *d_out, float *d_outF32, hipStream_t st, xrt_stats *stats, const BatchSrc::Paths *paths = nullptr,
                   const xrt_hit *d_hits = nullptr, const char *fn = "xrt_cast_rays", const PixelGenArgs *gen = nullptr) {
    if (int rc = batch_check_opts(fn, opts, iteration)) return rc;
    const long long depth = std::max(0LL, (long long)opts->max_reflections - (long long)iteration);
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return XRT_OK;
    xrt_render_opts o = *opts;
    o.max_reflections = (int32_t)depth;
    o.use_multisampling = XRT_MS_OFF; o.shard_count = 0; o.shard_rank = 0; o.n_gpus = 0; o.balance_tiles = 0;
    BatchSrc b;
    b.rays = d_rays; b.n = n; b.refIndex = refIndex; b.paths = paths; b.hits = d_hits;
    // (gen: the rays of a coherent centre list, made by the pass itself -- d_rays is null; given hits: nothing of generation 0 is traced, the hint has no reader)
    b.coherent = !d_hits && opts->list_order == XRT_LIST_COHERENT; b.gen = b.coherent ? gen : nullptr;
    if (b.gen) b.samples = gen->mode == PIXEL_FIXED16 ? 16 : (gen->mode == PIXEL_QUADRANT ? 4 : 1);
    xrt_scene::FrameCtx &F = s->frames[0];
    F.pose = s->poseCur;
    F.mat = s->matCur;   // (a ray batch reads the latest materials)
    F.shade = s->shadeCur;   // (... and the latest triangle values)
    Range rf(d_hits ? "xrt shade hits (%lld)" : "xrt cast rays (%lld)", (long long)n);
    int rc = frame_begin(s, F, nullptr, lights, nLights, &o, d_out, d_outF32, st, 0, 1, false, &b);
    if (rc != XRT_OK) {
        if (F.pending) (void)frame_finish(s, F, nullptr);
        return rc;
    }
    return frame_finish(s, F, stats);
}

// ---- xrt_render_pixels: GetColorForQuadrant / the body of Render's inner loop (RT:215-311, 412-425) on a caller's list of centres ----------
// What is wrong with the arguments alone (the scene is not looked at): the codes of a frame for the fields a frame reads.
int pixels_check_args(const char *fn, const xrt_camera *cam, const xrt_light *lights, int32_t nLights, const xrt_render_opts *opts, int64_t n, const void *centers,
                      const void *rgbaOut) {
    if (n < 0) return fail(XRT_E_INVALID_ARG, "%s: n = %lld out of range", fn, (long long)n);
    if (!cam || !opts || (!lights && nLights > 0) || nLights < 0) return fail(XRT_E_INVALID_ARG, "%s: null argument", fn);
    const int ms = opts->use_multisampling;
    if (ms != XRT_MS_OFF && ms != XRT_MS_FIXED16 && ms != XRT_MS_ADAPTIVE) return fail(XRT_E_INVALID_ARG, "%s: use_multisampling", fn);
    if (opts->shard_count < 0 || opts->shard_count > 1) return fail(XRT_E_INVALID_ARG, "%s: shard_count must be 0 or 1", fn);
    if (opts->n_gpus < 0 || opts->n_gpus > 1) return fail(XRT_E_INVALID_ARG, "%s: n_gpus must be 0 or 1", fn);
    if (opts->max_reflections < 0 || opts->max_reflections > 64) return fail(XRT_E_INVALID_ARG, "max_reflections out of range");
    if (opts->address_mode < XRT_ADDRESS_CLAMP || opts->address_mode > XRT_ADDRESS_MIRROR)
        return fail(XRT_E_INVALID_ARG, "Value does not fall within the expected range: addressMode (MAT:85)");
    if (opts->filtering != XRT_FILTER_POINT && opts->filtering != XRT_FILTER_BILINEAR)
        return fail(XRT_E_INVALID_ARG, "Value does not fall within the expected range: filtering (MAT:97)");
    if (ms == XRT_MS_ADAPTIVE && (opts->multisample_quality < 0 || opts->multisample_quality > 6))
        return fail(XRT_E_UNSUPPORTED, "MultisampleQuality above 6 (4^7 sub-quadrants per pixel)");
    if (cam->vp_width <= 0 || cam->vp_height <= 0) return fail(XRT_E_INVALID_ARG, "viewport must be positive");
    if (opts->list_order != XRT_LIST_UNORDERED && opts->list_order != XRT_LIST_COHERENT) return fail(XRT_E_INVALID_ARG, "%s: list_order must be XRT_LIST_UNORDERED or XRT_LIST_COHERENT", fn);
    if (n > 0 && (!centers || !rgbaOut)) return fail(XRT_E_INVALID_ARG, "%s: null argument", fn);
    return XRT_OK;
}

// One call on n > 0 centres in HBM (interleaved x y).  Every ray goes through cast_rays_impl -- iteration 0, currentRefIndex 1.0f (RT:424), the
// latest poses, materials and triangle values, plain or ray tree by the materials, its own chunking -- and every cast is complete when it
// returns, so the level counts of an adaptive list are read back between the levels as adaptive_careful reads them.  The caller holds the scene.
struct PixelsJob {
    xrt_scene *s;
    const xrt_light *lights;
    int nL;
    xrt_render_opts o;     // the options of every cast: one ray, one colour
    RayGenParams g;        // camera part only (make_raygen without a root box: no cull rectangle)
    hipStream_t st;
    uint64_t budget;
    xrt_stats acc;
    bool any = false;
    bool coherent = false;   // the call's xrt_render_opts.list_order is XRT_LIST_COHERENT (set by run)

    void tally(const xrt_stats &t) {   // counters and times add up over the casts of the call
        uint64_t *a = reinterpret_cast<uint64_t *>(&acc);
        const uint64_t *b = reinterpret_cast<const uint64_t *>(&t);
        for (size_t k = 0; k < offsetof(xrt_stats, ms_total) / sizeof(uint64_t); k++) a[k] += b[k];
        acc.ms_total += t.ms_total; acc.ms_intersect += t.ms_intersect;
        acc.ms_intersect_longest = std::max(acc.ms_intersect_longest, t.ms_intersect_longest);
        acc.intersect_launches += t.intersect_launches;
        acc.rays_traversed += t.rays_traversed; acc.mesh_queries_facing_away += t.mesh_queries_facing_away;
        any = true;
    }
    // The colours of entries [first, first + count) of a list, `samples` rays each: d_col[0 .. count * samples), d_f32 (nullable) likewise.
    // hinted (XRT_LIST_COHERENT, levels whose entries are the caller's): the pass makes the rays itself (k_pixel_raygen) and picks its kernels as a frame does.
    int cast(const float *cx, const float *cy, int stride, long long first, long long count, float size, int mode, uint32_t *d_col, float *d_f32, bool hinted = false) {
        const int ms = mode == PIXEL_FIXED16 ? XRT_MS_FIXED16 : (mode == PIXEL_QUADRANT ? XRT_MS_ADAPTIVE : XRT_MS_OFF);
        const long long samples = pixel_samples(ms);
        const std::vector<long long> b = pixel_chunks(count, ms, 0, nL, budget, hinted);
        xrt_render_opts oc = o;
        oc.list_order = hinted ? XRT_LIST_COHERENT : XRT_LIST_UNORDERED;
        for (size_t c = 0; c + 1 < b.size(); c++) {
            const long long m = b[c + 1] - b[c], rays = m * samples;
            int rc;
            PixelGenArgs G;   // (hinted: the pass makes the chunk's rays itself; else they are made here)
            G.cam = g; G.cx = cx; G.cy = cy; G.stride = stride; G.first = first + b[c]; G.size = size; G.mode = mode;
            if (!hinted) {
                if ((rc = s->pixelRays.ensure((size_t)rays))) return rc;
                launch_pixel_rays(g, cx, cy, stride, first + b[c], (int)m, size, mode, s->pixelRays.p, st);
                HIPCHECK(hipGetLastError());
            }
            xrt_stats t;
            if ((rc = cast_rays_impl(s, hinted ? nullptr : s->pixelRays.p, rays, 0, 1.0f, lights, nL, &oc, d_col + b[c] * samples, d_f32 ? d_f32 + 3 * b[c] * samples : nullptr, st, &t,
                                     nullptr, nullptr, "xrt_render_pixels", hinted ? &G : nullptr)))
                return rc;
            tally(t);
        }
        return XRT_OK;
    }
    // RenderFirstPass / GetColorForQuadrant(cx, cy, 1.0f, 0) (RT:195, 215-311) for entries [first, first + m): level 0's quadrants are the
    // entries, a level's quadrants each cast four rays, corners that deviate go to the next level, results fold back up (RT:305 slot rule:
    // k_ms_fold as it is), and the level-0 quadrants are resolved in list order.
    int adaptive(const float *centers, long long first, long long m, int quality, uint32_t *d_out, float *d_outF32) {
        struct Level : xrt_scene::WorkBufs::Level { long long n = 0; };
        std::vector<Level> lv((size_t)quality + 1);
        DevBuf<int> levelCount;
        int rc;
        if ((rc = levelCount.ensure((size_t)quality + 1))) return rc;
        HIPCHECK(hipMemsetAsync(levelCount.p, 0, ((size_t)quality + 1) * sizeof(int), st));
        lv[0].n = m;
        float size = 1.0f;   // RT:195
        for (int l = 0; l <= quality; l++) {
            Level &L = lv[l];
            if (L.n == 0) break;
            if (L.n > PIXEL_CHUNK_MAX_RAYS) return fail(XRT_E_UNSUPPORTED, "xrt_render_pixels: %lld quadrants at level %d of one chunk", L.n, l);
            if ((rc = L.color.ensure((size_t)L.n * 4))) return rc;
            const float *cx = l == 0 ? centers + 2 * first : L.cx.p, *cy = l == 0 ? cx + 1 : L.cy.p;
            const int stride = l == 0 ? 2 : 1;
            if ((rc = cast(cx, cy, stride, 0, L.n, size, PIXEL_QUADRANT, L.color.p, nullptr, coherent && l == 0))) return rc;   // (the deeper levels are lists of quadrants in the order k_pixel_decide appended them)
            if (l < quality) {   // RT:279-306
                Level &N = lv[l + 1];
                if ((rc = L.childBase.ensure((size_t)L.n)) || (rc = L.childMask.ensure((size_t)L.n)) || (rc = N.cx.ensure((size_t)L.n * 4)) || (rc = N.cy.ensure((size_t)L.n * 4)))
                    return rc;
                launch_pixel_decide(L.color.p, cx, cy, stride, (int)L.n, size, L.childBase.p, L.childMask.p, N.cx.p, N.cy.p, levelCount.p + l + 1, st);
                HIPCHECK(hipGetLastError());
                int hn = 0;
                HIPCHECK(hipMemcpyAsync(&hn, levelCount.p + l + 1, sizeof(int), hipMemcpyDeviceToHost, st));
                HIPCHECK(hipStreamSynchronize(st));
                N.n = hn;
                size = size / 2.0f;   // RT:290
            }
        }
        for (int l = quality - 1; l >= 0; l--)
            if (lv[l + 1].n > 0) launch_ms_fold(lv[l].color.p, lv[l + 1].color.p, lv[l].childBase.p, lv[l].childMask.p, (int)lv[l].n, st);
        launch_pixel_resolve(lv[0].color.p, (int)m, PIXEL_QUADRANT, d_out + first, d_outF32 ? d_outF32 + 3 * first : nullptr, st);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(st));   // (the levels are freed on return)
        return XRT_OK;
    }
    int run(const float *centers, int64_t n, uint32_t *d_out, float *d_outF32) {
        const int ms = o.use_multisampling, quality = o.multisample_quality;
        o.use_multisampling = XRT_MS_OFF; o.multisample_quality = 0;
        coherent = o.list_order == XRT_LIST_COHERENT;
        if (ms == XRT_MS_OFF) return cast(centers, centers + 1, 2, 0, n, 1.0f, PIXEL_ONE, d_out, d_outF32, coherent);   // RT:412-425: the cast writes the caller's arrays
        const std::vector<long long> b = pixel_chunks(n, ms, quality, nL, budget, coherent);
        for (size_t c = 0; c + 1 < b.size(); c++) {
            const long long first = b[c], m = b[c + 1] - b[c];
            int rc;
            if (ms == XRT_MS_ADAPTIVE) {
                if ((rc = adaptive(centers, first, m, quality, d_out, d_outF32))) return rc;
                continue;
            }
            if ((rc = s->pixelSamples.ensure((size_t)m * 16))) return rc;
            if ((rc = cast(centers, centers + 1, 2, first, m, 1.0f, PIXEL_FIXED16, s->pixelSamples.p, nullptr, coherent))) return rc;
            launch_pixel_resolve(s->pixelSamples.p, (int)m, PIXEL_FIXED16, d_out + first, d_outF32 ? d_outF32 + 3 * first : nullptr, st);
            HIPCHECK(hipGetLastError());
        }
        return XRT_OK;
    }
};

int render_pixels_impl(xrt_scene *s, const xrt_camera *cam, const xrt_light *lights, int32_t nLights, const xrt_render_opts *opts, const float *d_centers,
                       int64_t n, uint32_t *d_out, float *d_outF32, hipStream_t st, xrt_stats *stats) {
    PixelsJob J;
    J.s = s; J.lights = lights; J.nL = nLights; J.st = st;
    J.o = *opts;
    J.o.shard_count = 0; J.o.shard_rank = 0; J.o.n_gpus = 0; J.o.balance_tiles = 0;
    J.budget = (uint64_t)s->cfg.pixelBytes;
    std::memset(&J.acc, 0, sizeof(J.acc));
    if (int rc = make_raygen(cam, &J.o, J.g)) return rc;
    Range rf("xrt render pixels");
    int rc = J.run(d_centers, n, d_out, d_outF32);
    if (rc == XRT_OK) HIPCHECK(hipStreamSynchronize(st));   // (the resolve of the last chunk)
    if (stats) {
        *stats = J.acc;
        stats->pixels = (uint64_t)n;
        stats->pieces = 1;
    }
    return rc;
}

// ---- xrt_trace_pixels: the ray of RT:412-421 and the IntersectionResult of RT:512 for a caller's list of centres ----------------------------------
// What is wrong with the arguments alone (the scene is not looked at), in the order xrt.h states.
int trace_check_args(const char *fn, const xrt_camera *cam, const xrt_render_opts *opts, int64_t n, const void *centers, const void *raysOut, const void *hitsOut) {
    if (n < 0) return fail(XRT_E_INVALID_ARG, "%s: n = %lld out of range", fn, (long long)n);
    if (!cam || !opts) return fail(XRT_E_INVALID_ARG, "%s: null camera or opts", fn);
    const int ms = opts->use_multisampling;
    if (ms == XRT_MS_ADAPTIVE)
        return fail(XRT_E_INVALID_ARG, "%s: use_multisampling XRT_MS_ADAPTIVE subdivides by colours, which this call does not make: list the sample positions as centres", fn);
    if (ms != XRT_MS_OFF && ms != XRT_MS_FIXED16) return fail(XRT_E_INVALID_ARG, "%s: use_multisampling must be XRT_MS_OFF or XRT_MS_FIXED16", fn);
    if (opts->list_order != XRT_LIST_UNORDERED && opts->list_order != XRT_LIST_COHERENT) return fail(XRT_E_INVALID_ARG, "%s: list_order must be XRT_LIST_UNORDERED or XRT_LIST_COHERENT", fn);
    if (opts->shard_count < 0 || opts->shard_count > 1) return fail(XRT_E_INVALID_ARG, "%s: shard_count must be 0 or 1", fn);
    if (opts->n_gpus < 0 || opts->n_gpus > 1) return fail(XRT_E_INVALID_ARG, "%s: n_gpus must be 0 or 1", fn);
    if (cam->vp_width <= 0 || cam->vp_height <= 0) return fail(XRT_E_INVALID_ARG, "%s: viewport must be positive", fn);
    if (n > 0 && !raysOut && !hitsOut) return fail(XRT_E_INVALID_ARG, "%s: both outputs are null", fn);
    if (n > 0 && !centers) return fail(XRT_E_INVALID_ARG, "%s: null centers", fn);
    return XRT_OK;
}

// n > 0 centres in HBM (interleaved x y); d_rays / d_hits: the caller's arrays, either may be null.  Per chunk (trace_plan.h):
//   unhinted -- k_pixel_rays into the caller's rays (or the work buffer), then run_intersect's launch, as xrt_scene_intersect traces;
//   hinted (XRT_LIST_COHERENT, hits wanted) -- k_trace_raygen answers the rays that cannot reach the root box and compacts the others, ONE traversal launch
//   answers those straight into the caller's array (IntersectArgs / PacketArgs::scatter, flags null: full records): the kernel a plain frame of the same
//   scene and sampling takes for launch #0 -- bit 0 of scene_packet_mask, the rule plan_frame reads too --, with the packet table unless XRT_PK_QUADS=0,
//   through launch_list_traversal;
// the count words come back behind one synchronisation.  The latest poses; no material, no triangle value.  The caller holds the scene (BusyGuard, no frame
// in flight), which is why a hinted chunk may keep its index list and table in frame context 0's buffers, where xrt_debug_packet_table looks.
int trace_pixels_impl(xrt_scene *s, const xrt_camera *cam, const xrt_render_opts *opts, const float *d_centers, int64_t n, xrt_ray *d_rays, xrt_hit *d_hits,
                      hipStream_t st, xrt_stats *stats) {
    xrt_scene::TraceWork &W = s->traceWork;
    xrt_scene::FrameCtx &F0 = s->frames[0];
    int rc;
    xrt_render_opts o;
    std::memset(&o, 0, sizeof(o));
    PixelGenArgs G;
    if ((rc = make_raygen(cam, &o, G.cam))) return rc;
    const int samples = opts->use_multisampling == XRT_MS_FIXED16 ? 16 : 1;
    G.cx = d_centers; G.cy = d_centers + 1; G.stride = 2; G.size = 1.0f; G.mode = samples == 16 ? PIXEL_FIXED16 : PIXEL_ONE;
    const bool hinted = d_hits && opts->list_order == XRT_LIST_COHERENT;
    const bool collect = d_hits && stats && opts->collect_stats != 0;
    const bool packets = hinted && (scene_packet_mask(*s, samples) & 1) != 0, table = packets && s->cfg.packetQuads;   // (bit 0: launch #0 of a plain frame)
    const std::vector<long long> b = trace_chunks(n, samples, (uint64_t)s->cfg.pixelBytes, hinted);
    const size_t placesCap = (size_t)(b[1] - b[0]) * (size_t)samples;   // (the first chunk is the longest)
    const size_t tableCap = (placesCap + 63) / 64;
    if ((rc = W.counts.ensure(4)) || (rc = W.queue.ensure(1 + PACKET_QUEUE_WORDS))) return rc;
    if ((hinted || !d_rays) && (rc = W.rays.ensure(placesCap))) return rc;
    if (collect && hinted && !d_rays && (rc = W.countRays.ensure(placesCap))) return rc;
    if (hinted && (rc = F0.w.index0.ensure(placesCap))) return rc;
    if (table) {
        const unsigned *before = F0.w.quadTable.p; const size_t capBefore = F0.w.quadTable.cap;
        if ((rc = F0.w.quadTable.ensure((size_t)QUAD_HEAD_WORDS + 2 * tableCap))) return rc;
        if (F0.w.quadTable.p != before || F0.w.quadTable.cap != capBefore) HIPCHECK(hipMemsetAsync(F0.w.quadTable.p, 0, QUAD_HEAD_WORDS * sizeof(unsigned), st));   // (the count words start at zero, ensure_frame_buffers)
    }
    if (collect) {
        if ((rc = s->counters.ensure(2 * C_COUNT + 8))) return rc;
        HIPCHECK(hipMemsetAsync(s->counters.p, 0, 2 * C_COUNT * sizeof(unsigned long long), st));
    }
    for (Event &e : W.ev) if ((rc = e.create(hipEventDefault))) return rc;
    const int pv = s->poseCur;
    if ((rc = pose_wait(s, pv, st))) return rc;
    const SceneView S = pose_view(s, pv);
    unsigned long long live = 0, found = 0;
    double msTotal = 0.0, msIntersect = 0.0, msLongest = 0.0;
    unsigned launches = 0;
    s->quadCtx = -1; s->quadLive = 0;
    Range rf("xrt trace pixels");
    for (size_t c = 0; c + 1 < b.size(); c++) {
        const long long m = b[c + 1] - b[c];
        const int P = (int)(m * samples);
        const size_t at = (size_t)b[c] * (size_t)samples;
        xrt_ray *const raysOut = d_rays ? d_rays + at : nullptr;
        xrt_hit *const hitsOut = d_hits ? d_hits + at : nullptr;
        const xrt_ray *listRays = raysOut;   // the chunk's rays in list order, where somebody has them
        bool traced = false;
        G.first = b[c];
        HIPCHECK(hipMemsetAsync(W.counts.p, 0, 4 * sizeof(int), st));
        HIPCHECK(hipEventRecord(W.ev[0], st));
        if (!hinted) {
            if (!raysOut) listRays = W.rays.p;
            launch_pixel_rays(G.cam, G.cx, G.cy, G.stride, G.first, (int)m, G.size, G.mode, raysOut ? raysOut : W.rays.p, st);
            HIPCHECK(hipGetLastError());
            if (hitsOut) {
                std::lock_guard<std::mutex> lock(s->apiMutex);   // (run_intersect: the queue word of the stream)
                if ((rc = run_intersect(s, listRays, P, hitsOut, s->sceneMode, 0, st, nullptr, false, W.ev[2], W.ev[3]))) return rc;
                traced = true;
            }
        } else {
            HIPCHECK(hipMemsetAsync(W.queue.p, 0, (1 + PACKET_QUEUE_WORDS) * sizeof(unsigned), st));
            QuadTable Q;
            if (table) {   // the context's two count words take turns (enqueue_chunk)
                xrt_scene::WorkBufs &FW = F0.w;
                FW.quadWord ^= 1;
                Q.table = reinterpret_cast<uint2 *>(FW.quadTable.p + QUAD_HEAD_WORDS); Q.cap = (int)tableCap;
                Q.count = FW.quadTable.p + 64 * FW.quadWord; Q.clear = FW.quadTable.p + 64 * (FW.quadWord ^ 1);
            }
            launch_trace_raygen(G, S, raysOut, hitsOut, W.rays.p, F0.w.index0.p, W.counts.p, P, P, Q, st);
            IntersectArgs A = IntersectArgs();
            A.rays = W.rays.p; A.hits = hitsOut; A.index = nullptr; A.nDev = W.counts.p; A.nMul = 1; A.n = P; A.nCap = P;
            A.queue = W.queue.p; A.mode = s->sceneMode; A.meshId = 0;
            A.flags = nullptr; A.missRecords = 0; A.scatter = F0.w.index0.p;   // every traced ray gets its full record, at its place
            if ((rc = launch_list_traversal(s, S, A, packets, &Q, W.splitItems, W.splitRecs, P, st, W.ev[2], W.ev[3]))) return rc;
            traced = true;
            if (collect && !listRays) {   // the counting pass walks the list, as the unhinted call's does
                launch_pixel_rays(G.cam, G.cx, G.cy, G.stride, G.first, (int)m, G.size, G.mode, W.countRays.p, st);
                listRays = W.countRays.p;
            }
        }
        if (hitsOut && stats) launch_trace_hits(hitsOut, P, W.counts.p + 1, st);
        if (collect) {
            IntersectArgs K = IntersectArgs();
            K.rays = listRays; K.hits = nullptr; K.index = nullptr; K.nDev = nullptr; K.nMul = 1; K.n = P; K.nCap = 0; K.queue = nullptr; K.mode = s->sceneMode; K.meshId = 0;
            set_knobs(K, s);
            launch_count(S, K, s->counters.p, st);
        }
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(W.ev[1], st));
        int hc[2] = {0, 0};
        HIPCHECK(hipMemcpyAsync(hc, W.counts.p, sizeof(hc), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));   // (the one synchronisation of the chunk)
        if (hinted && (hc[0] < 0 || hc[0] > P)) return fail(XRT_E_INTERNAL, "xrt_trace_pixels: %d live rays in a chunk of %d places", hc[0], P);
        live += hitsOut ? (hinted ? (unsigned long long)hc[0] : (unsigned long long)P) : 0ull;
        found += (unsigned long long)hc[1];
        float ms = 0.0f;
        HIPCHECK(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
        msTotal += ms;
        if (traced) {
            HIPCHECK(hipEventElapsedTime(&ms, W.ev[2], W.ev[3]));
            msIntersect += ms; msLongest = std::max(msLongest, (double)ms); launches++;
        }
        if (table && b.size() == 2) {   // (xrt_debug_packet_table: the table and the index list of a one-chunk call stay in the context until its next frame or list)
            F0.plan.pkEntries = tableCap; F0.plan.scrRefs = 0;   // (a list takes no table of screen boxes: xrt_debug_screen_table reports none)
            s->quadCtx = 0; s->quadLive = (unsigned long long)hc[0];
        }
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        if (collect) {
            unsigned long long hcnt[2 * C_COUNT];
            HIPCHECK(hipMemcpy(hcnt, s->counters.p, sizeof(hcnt), hipMemcpyDeviceToHost));
            fill_stats(stats, hcnt, 0, (unsigned long long)n);
        }
        stats->pixels = (uint64_t)n;
        stats->rays_closest = d_hits ? (uint64_t)n * (uint64_t)samples : 0;
        stats->hits_closest = found;
        stats->rays_traversed = live;
        stats->ms_total = msTotal; stats->ms_intersect = msIntersect; stats->ms_intersect_longest = msLongest; stats->intersect_launches = launches;
    }
    return XRT_OK;
}

// ---- xrt_light_hits: the light loop of CastRay (RT:534-542) on a caller's hits ---------------------------------------------------------------
// n > 0 hits in HBM.  Per chunk (lights_plan.h): k_light_emit lists the shadow rays, ONE traversal launch (launch_list_traversal) answers them -- the launch a
// pass of xrt_cast_rays would make for the shadow rays of its generation 0: the wave-packet kernel where bit 1 of scene_packet_mask names it for them, else the
// per-lane kernel, with IntersectArgs::scatter / flags --, k_light_fold writes the caller's arrays, and the two count words come back behind one
// synchronisation.  The latest poses, materials and triangle values.  The caller holds the scene (BusyGuard, no frame in flight).
int light_hits_impl(xrt_scene *s, const xrt_hit *d_hits, int64_t n, const xrt_light *lights, int32_t nL, float *d_light, float *d_amount, hipStream_t st,
                    xrt_stats *stats) {
    xrt_scene::LightWork &W = s->lightWork;
    int rc;
    const std::vector<long long> b = light_chunks(n, nL, (uint64_t)s->cfg.shadowBytes);
    const size_t pairsCap = (size_t)(b[1] - b[0]) * (size_t)nL;   // (the first chunk is the longest)
    if ((rc = W.counts.ensure(4))) return rc;
    if (nL > 0 && ((rc = W.rays.ensure(pairsCap)) || (rc = W.hits.ensure(pairsCap)) || (rc = W.flags.ensure(pairsCap)) || (rc = W.scatter.ensure(pairsCap)) ||
                   (rc = W.queue.ensure(1 + PACKET_QUEUE_WORDS)) || (rc = W.lights.ensure((size_t)nL))))
        return rc;
    for (Event &e : W.ev) if ((rc = e.create(hipEventDefault))) return rc;
    const int pv = s->poseCur, mv = s->matCur, sv = s->shadeCur;
    if ((rc = pose_wait(s, pv, st)) || (rc = mat_acquire(s, mv, st)) || (rc = shade_wait(s, sv, st))) return rc;
    std::vector<LightRec> hl((size_t)(nL > 0 ? nL : 1));
    for (int i = 0; i < nL; i++) hl[(size_t)i] = make_light(lights[i]);
    if (nL > 0) HIPCHECK(hipMemcpyAsync(W.lights.p, hl.data(), (size_t)nL * sizeof(LightRec), hipMemcpyHostToDevice, st));
    const SceneView S = pose_view(s, pv);
    ShadeView V = shade_view(s, mv, sv);   // (no texture is looked up)
    V.lights = W.lights.p; V.nLights = nL;
    const bool ae = scene_answers_at_emission(*s);              // on the scenes where frames answer at emission
    const bool packets = (scene_packet_mask(*s, 1) & 2) != 0;   // (bit 1: the shadow rays of a plain batch, one ray per entry)
    unsigned long long live = 0, traced = 0;
    double msTotal = 0.0, msIntersect = 0.0;
    unsigned launches = 0;
    Range rf("xrt light hits");
    for (size_t c = 0; c + 1 < b.size(); c++) {
        const int m = (int)(b[c + 1] - b[c]);
        HIPCHECK(hipMemsetAsync(W.counts.p, 0, 4 * sizeof(int), st));
        HIPCHECK(hipEventRecord(W.ev[0], st));
        if (nL > 0) {
            HIPCHECK(hipMemsetAsync(W.queue.p, 0, (1 + PACKET_QUEUE_WORDS) * sizeof(unsigned), st));
            LightEmitArgs E;
            E.hits = d_hits; E.base = b[c]; E.n = m; E.nLights = nL; E.lights = W.lights.p; E.ae = ae ? 1 : 0;
            E.rays = W.rays.p; E.scatter = W.scatter.p; E.flags = W.flags.p; E.count = W.counts.p; E.cap = (int)((size_t)m * (size_t)nL);
            launch_light_emit(S, E, st);
            IntersectArgs B = IntersectArgs();
            B.rays = W.rays.p; B.hits = W.hits.p; B.index = nullptr; B.nDev = W.counts.p; B.nMul = 1; B.n = 0; B.nCap = E.cap;
            B.queue = W.queue.p; B.mode = s->sceneMode; B.meshId = 0;
            B.flags = W.flags.p; B.missRecords = 0; B.scatter = W.scatter.p;
            if ((rc = launch_list_traversal(s, S, B, packets, nullptr, W.splitItems, W.splitRecs, E.cap, st, W.ev[2], W.ev[3]))) return rc;
            launches++;
        }
        LightFoldArgs F;
        F.hits = d_hits; F.base = b[c]; F.n = m; F.flags = W.flags.p; F.shadowHits = W.hits.p;
        F.lightOut = d_light; F.amountOut = d_amount; F.liveCount = W.counts.p + 1;
        launch_light_fold(S, V, F, st);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(W.ev[1], st));
        int hc[2] = {0, 0};
        HIPCHECK(hipMemcpyAsync(hc, W.counts.p, sizeof(hc), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));   // (the one synchronisation of the chunk)
        traced += (unsigned long long)hc[0]; live += (unsigned long long)hc[1];
        float ms = 0.0f;
        HIPCHECK(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
        msTotal += ms;
        if (nL > 0) { HIPCHECK(hipEventElapsedTime(&ms, W.ev[2], W.ev[3])); msIntersect += ms; }
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->pixels = (uint64_t)n; stats->shaded_hits = live; stats->rays_shadow = live * (unsigned long long)nL; stats->rays_traversed = traced;
        stats->ms_total = msTotal; stats->ms_intersect = msIntersect; stats->intersect_launches = launches;
    }
    return XRT_OK;
}

// ---- xrt_surface_hits: CastRay's surface terms and next rays (RT:520-531, 547-559, 568-581, 656-694) on a caller's hits -----------------------
// n > 0 hits (and rays, where a ray output is asked) in HBM.  One kernel, k_surface, launched in pieces of at most SURFACE_PIECE entries (an int
// indexes the entries of a launch; the base offsets are size_t); the counter word comes back behind the call's one synchronisation.  The latest
// materials and triangle values; poses are not read.  The caller holds the scene (BusyGuard, no frame in flight).
int surface_hits_impl(xrt_scene *s, const xrt_ray *d_rays, const xrt_hit *d_hits, int64_t n, float curRef, const xrt_render_opts *opts, xrt_surface *d_surface,
                      xrt_ray *d_reflect, xrt_ray *d_refract, hipStream_t st, xrt_stats *stats) {
    xrt_scene::SurfaceWork &W = s->surfaceWork;
    int rc;
    if ((rc = W.count.ensure(1))) return rc;
    for (Event &e : W.ev) if ((rc = e.create(hipEventDefault))) return rc;
    const int mv = s->matCur, sv = s->shadeCur;
    if ((rc = mat_acquire(s, mv, st)) || (rc = shade_wait(s, sv, st))) return rc;
    ShadeView V = shade_view(s, mv, sv);   // (no light is read)
    V.addressMode = opts->address_mode; V.filtering = opts->filtering;
    Range rf("xrt surface hits");
    HIPCHECK(hipMemsetAsync(W.count.p, 0, sizeof(unsigned long long), st));
    HIPCHECK(hipEventRecord(W.ev[0], st));
    for (size_t base = 0; base < (size_t)n; base += (size_t)SURFACE_PIECE) {
        const size_t left = (size_t)n - base;
        SurfaceArgs A;
        A.hits = d_hits; A.rays = d_rays; A.base = base; A.n = (int)(left < (size_t)SURFACE_PIECE ? left : (size_t)SURFACE_PIECE);
        A.nMeshes = (int)s->host->meshes.size(); A.curRef = curRef;
        A.wantSurface = d_surface ? 1 : 0; A.wantReflect = d_reflect ? 1 : 0; A.wantRefract = d_refract ? 1 : 0;
        A.surfaceOut = d_surface; A.reflectOut = d_reflect; A.refractOut = d_refract; A.liveCount = W.count.p;
        launch_surface(V, A, st);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(W.ev[1], st));
    unsigned long long live = 0;
    HIPCHECK(hipMemcpyAsync(&live, W.count.p, sizeof(live), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));   // (the one synchronisation of the call)
    float ms = 0.0f;
    HIPCHECK(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->pixels = (uint64_t)n; stats->shaded_hits = live; stats->ms_total = ms; stats->intersect_launches = 0;
    }
    return XRT_OK;
}

// ---- xrt_compose_hits: the return path of CastRay, one level (RT:584, 699, 705, 726, 732), on a caller's terms ---------------------------------
// n > 0 entries in HBM.  One kernel, k_compose_hits, launched in pieces of at most COMPOSE_PIECE entries (an int indexes the entries of a launch;
// the base offsets are size_t); the counter word comes back behind the call's one synchronisation.  Nothing of the scene is read but its
// stream.  The caller holds the scene (BusyGuard, no frame in flight).
int compose_hits_impl(xrt_scene *s, const xrt_surface *d_surface, const float *d_light, const uint32_t *d_reflect, const uint32_t *d_refract, int64_t n,
                      uint32_t *d_rgba, float *d_f32, hipStream_t st, xrt_stats *stats) {
    xrt_scene::ComposeWork &W = s->composeWork;
    int rc;
    if ((rc = W.count.ensure(1))) return rc;
    for (Event &e : W.ev) if ((rc = e.create(hipEventDefault))) return rc;
    Range rf("xrt compose hits");
    HIPCHECK(hipMemsetAsync(W.count.p, 0, sizeof(unsigned long long), st));
    HIPCHECK(hipEventRecord(W.ev[0], st));
    for (size_t base = 0; base < (size_t)n; base += (size_t)COMPOSE_PIECE) {
        const size_t left = (size_t)n - base;
        ComposeArgs A;
        A.surface = d_surface; A.light = d_light; A.reflect = d_reflect; A.refract = d_refract;
        A.base = base; A.n = (int)(left < (size_t)COMPOSE_PIECE ? left : (size_t)COMPOSE_PIECE);
        A.haveReflect = d_reflect ? 1 : 0; A.haveRefract = d_refract ? 1 : 0; A.wantRgba = d_rgba ? 1 : 0; A.wantF32 = d_f32 ? 1 : 0;
        A.rgbaOut = d_rgba; A.f32Out = d_f32; A.hitCount = W.count.p;
        launch_compose_hits(A, st);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(W.ev[1], st));
    unsigned long long live = 0;
    HIPCHECK(hipMemcpyAsync(&live, W.count.p, sizeof(live), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));   // (the one synchronisation of the call)
    float ms = 0.0f;
    HIPCHECK(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->pixels = (uint64_t)n; stats->shaded_hits = live; stats->ms_total = ms; stats->intersect_launches = 0;
    }
    return XRT_OK;
}

// ---- xrt_fold_samples: RT:309 on a caller's colours: the mean of four, or the mean of four such means ------------------------------------------
// n > 0 entries of `samples` colours in HBM, through k_pixel_resolve (pixels.hip: what xrt_render_pixels folds its own samples with), launched in
// pieces of at most COMPOSE_PIECE entries.  One synchronisation.
int fold_samples_impl(xrt_scene *s, const uint32_t *d_in, int64_t n, int32_t samples, uint32_t *d_rgba, float *d_f32, hipStream_t st, xrt_stats *stats) {
    xrt_scene::ComposeWork &W = s->composeWork;
    int rc;
    for (Event &e : W.ev) if ((rc = e.create(hipEventDefault))) return rc;
    Range rf("xrt fold samples");
    HIPCHECK(hipEventRecord(W.ev[0], st));
    for (size_t base = 0; base < (size_t)n; base += (size_t)COMPOSE_PIECE) {
        const size_t left = (size_t)n - base;
        launch_pixel_resolve(d_in + base * (size_t)samples, (int)(left < (size_t)COMPOSE_PIECE ? left : (size_t)COMPOSE_PIECE),
                             samples == 4 ? PIXEL_QUADRANT : PIXEL_FIXED16, d_rgba + base, d_f32 ? d_f32 + 3 * base : nullptr, st);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(W.ev[1], st));
    HIPCHECK(hipStreamSynchronize(st));   // (the one synchronisation of the call)
    float ms = 0.0f;
    HIPCHECK(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->pixels = (uint64_t)n; stats->ms_total = ms; stats->intersect_launches = 0;
    }
    return XRT_OK;
}

int pose_upload(xrt_scene *scene);

// What is made from the scene octree and the poses (snodes, srefs, objects, scull, the positions of every body's records in scull, the
// bodies' world boxes) -> HBM; the pose versions start again from version 0 (xrt_scene_build, xrt_scene_build_tree).  No frame in flight.
int tree_upload(xrt_scene *scene) {
    const SceneArrays &A = scene->host->arrays;
    int rc;
    if ((rc = upload(scene->snodes, A.snodes)) || (rc = upload(scene->srefs, A.srefs)) || (rc = upload(scene->scull, A.scull)) || (rc = upload(scene->objects, A.objects)))
        return rc;
    return pose_upload(scene);
}

// The bodies' positions in scull and their world boxes -> HBM; the pose versions start again from version 0.
int pose_upload(xrt_scene *scene) {
    const SceneArrays &A = scene->host->arrays;
    int rc;
    if ((rc = upload(scene->scullPosStart, A.scullPosStart)) || (rc = upload(scene->scullPos, A.scullPos))) return rc;
    std::vector<float> wbb(6 * (scene->host->objects.size() + 1), 0.0f);
    for (size_t o = 0; o < scene->host->objects.size(); o++) std::memcpy(&wbb[6 * o], scene->host->objects[o].worldBbox, 6 * sizeof(float));
    if ((rc = upload(scene->wbbDev, wbb))) return rc;
    for (auto &v : scene->pose) { v.ready.reset(); v.serial = 0; }
    scene->poseCur = 0; scene->poseSerial = 0; scene->posesOnDevice = false;
    return XRT_OK;
}

// Launch geometry and scheduling defaults that scene_upload derives from the scene (again after xrt_scene_build_tree).
int scene_derive(xrt_scene *scene) {
    const SceneArrays &A = scene->host->arrays;
    SceneView &S = scene->view;
    S.blocks = scene->blocks.p; S.childDfs = scene->childDfs.p; S.leafNB = scene->leafNB.p; S.leafTB = scene->leafTB.p; S.refT = scene->refT.p; S.pblocks = scene->pblocks.p; S.lrec = scene->lrec.p; S.refN = scene->refN.p; S.refG = scene->refG.p;
    S.meshes = scene->meshes.p; S.snodes = scene->snodes.p; S.srefs = scene->srefs.p; S.scull = scene->scull.p; S.runTB = scene->runTB.p; S.runBase = scene->runBase.p;
    S.objects = scene->objects.p; S.objMesh = scene->objMesh.p;
    S.nMeshes = (int)scene->host->meshes.size(); S.nObjects = (int)scene->host->objects.size();
    S.sceneDepth = A.sceneDepth + 1; S.meshDepth = A.meshDepth + 1;
    const Settings &cfg = scene->cfg;
    S.nodeCull = cfg.nodeCull;
    scene->sceneMode = (!cfg.noSingle && scene->host->objects.size() == 1 && scene->host->objects[0].meshes.size() == 1 && scene->host->meshes.size() == 1 &&
                        scene->host->sceneTree.nodeCount == 1) ? MODE_SINGLE : MODE_SCENE;
    scene->blocksPerCU = intersect_blocks_per_cu(scene->stackNeeded, scene->sceneMode);
    scene->blocksPerCUMesh = intersect_blocks_per_cu(scene->stackNeeded, MODE_MESH);
    scene->packetOk = packet_supported(scene->sceneMode, A.meshDepth, A.sceneDepth);
    // Refill threshold of k_intersect.  A two-level scene refills a wave only when ALL its lanes are idle: fresh rays start in the
    // scene phase while the others are deep in a mesh, and every partial refill made the wave run that phase for a few lanes
    // (measured with 8x8-pixel waves, whose rays take about equally long: C3 3.1 -> 2.45 ms, C4 8.9 -> 6.2 ms of traversal per frame).
    // One-body scenes have no such phase and keep refilling at 24 idle lanes (64 costs them 6 %).
    scene->refillMin = cfg.tune[0] > 0 ? cfg.tune[0] : (scene->sceneMode == MODE_SCENE ? 64 : 24);
    // Listed long rays: mixed one in eight into the first batches where waves refill lane by lane (a wave full of them takes five
    // times as long as one of them: C5 at one sample per pixel 1.58 -> 1.42 ms); 64 to a wave where waves refill as a whole -- there
    // a mixed wave idles 56 lanes until its long rays are done (C3 2.71 -> 2.97 ms when mixed).
    scene->heavyShift = cfg.heavyShift.value_or(scene->sceneMode == MODE_SCENE ? 0 : 3);
    scene->blocksPerCUPacket = packet_blocks_per_cu(scene->sceneMode);
    scene->firstBatch = cfg.firstBatch.value_or(A.meshDepth == 0 ? 256 : 64);   // every mesh is a single leaf: rays are cheap, avoid queue traffic
    {   // "long ray first": worth it only where rays can be long, i.e. where some mesh has a real octree
        const float frac = cfg.heavy.value_or(0.25f);
        scene->heavyPath = 0.0f;
        scene->deepMeshes = A.meshDepth > 0;
        for (int &t : scene->costT) t = 24;
        // (measured: +24 % on the 1M-triangle heightfield, whose stragglers are rays skimming the terrain; nothing on the
        //  instanced grid, whose rays are all about as long as the box -- XRT_HEAVY forces it on for any scene)
        const bool wanted = cfg.heavy.has_value() || scene->sceneMode == MODE_SINGLE;
        if (wanted && frac > 0.0f && A.meshDepth > 0 && A.snodes.size() >= 2) {
            const f4 lo = A.snodes[0], hi = A.snodes[1];
            const double dx = (double)hi.x - lo.x, dy = (double)hi.y - lo.y, dz = (double)hi.z - lo.z;
            const double diag = std::sqrt(dx * dx + dy * dy + dz * dz);
            if (diag > 0.0 && diag < 1e30) scene->heavyPath = (float)(frac * diag);
        }
    }
    scene->resident = true;
    return XRT_OK;
}

// The material versions start again from version 0, which holds the host's materials (scene->materials / texels were just uploaded).
void material_restart(xrt_scene *scene) {
    const SceneArrays &A = scene->host->arrays;
    for (auto &v : scene->mat) { v.ready.reset(); v.owner = nullptr; v.pending = false; v.serial = 0; v.texFull = true; v.texLo = v.texHi = 0; v.texCount = 0; v.anyTransparent = A.anyTransparent; }
    scene->mat[0].texFull = false; scene->mat[0].texCount = A.texels.size();
    scene->matCur = 0; scene->matSerial = 0;
}

// Host arrays of scene->host -> HBM of scene->device, launch geometry and scheduling defaults (second half of
// xrt_scene_build; also what puts a replica of the scene on another device).
int scene_upload(xrt_scene *scene) {
    const SceneArrays &A = scene->host->arrays;
    const int stackNeeded = (A.sceneDepth + 1) + (A.meshDepth + 1);
    if (intersect_stack_capacity(stackNeeded) < 0) return fail(XRT_E_UNSUPPORTED, "octree too deep for the LDS stack (%d levels)", stackNeeded);
    scene->stackNeeded = stackNeeded;
    if (scene->device < 0) return XRT_OK;   // host-only scene: trees can be inspected, nothing can be traced
    HIPCHECK(hipSetDevice(scene->device));
    int rc;
    if ((rc = upload(scene->blocks, A.blocks)) || (rc = upload(scene->leafNB, A.leafNB)) || (rc = upload(scene->leafTB, A.leafTB)) || (rc = upload(scene->refT, A.refT)) || (rc = upload(scene->pblocks, A.pblocks)) || (rc = upload(scene->lrec, A.lrec)) || (rc = upload(scene->refN, A.refN)) || (rc = upload(scene->refG, A.refG)) ||
        (rc = upload(scene->snodes, A.snodes)) || (rc = upload(scene->shade, A.shade)) || (rc = upload(scene->childDfs, A.childDfs)) ||
        (rc = upload(scene->srefs, A.srefs)) || (rc = upload(scene->scull, A.scull)) || (rc = upload(scene->runTB, A.runTB)) || (rc = upload(scene->runBase, A.runBase)) || (rc = upload(scene->objMesh, A.objMesh)) ||
        (rc = upload(scene->meshes, A.meshes)) || (rc = upload(scene->objects, A.objects)) || (rc = upload(scene->materials, A.materials)) ||
        (rc = upload(scene->texels, A.texels)) || (rc = pose_upload(scene)))
        return rc;
    material_restart(scene);
    shade_restart(scene);
    return scene_derive(scene);
}

// Enqueue one pose update: entries [0, n) of the device arrays ids / world / inv / wbb, ready on `st`, become the newest version.  The version
// written is the current one unless an open ticket reads it; then a free one, made a copy of the current one first.  Nothing here waits
// for the device: the update runs on poseStream behind `st` and behind the asynchronous seam-1 reads of the version it overwrites, and
// `st` continues behind the update (the caller may refill its arrays there).  Caller holds apiMutex and the scene (BusyGuard).
int poses_enqueue(xrt_scene *s, const int *ids, int n, const float *world, const float *inv, const float *wbb, hipStream_t st) {
    const int cur = s->poseCur;
    int v = cur;
    if (pose_referenced(s, v))
        for (int x = 0; x < 3; x++) if (x != cur && !pose_referenced(s, x)) { v = x; break; }
    if (pose_referenced(s, v)) return fail(XRT_E_INTERNAL, "xrt_scene_set_poses: no free pose version");
    xrt_scene::PoseVer &P = s->pose[v];
    const SceneArrays &A = s->host->arrays;
    int rc;
    if ((rc = s->poseStream.create()) || (rc = s->poseInput.create())) return rc;
    hipStream_t ps = s->poseStream;
    if (st != ps) {
        HIPCHECK(hipEventRecord(s->poseInput, st));
        HIPCHECK(hipStreamWaitEvent(ps, s->poseInput, 0));
    }
    for (auto &rd : P.readers) HIPCHECK(hipStreamWaitEvent(ps, rd.second, 0));
    PoseArgs PA;
    if (v != cur) {   // (k_pose copies the current version first)
        if ((rc = P.objects.ensure(A.objects.size())) || (rc = P.scull.ensure(A.scull.size()))) return rc;
        PA.copyObjects = pose_objects(s, cur); PA.copyScull = pose_scull(s, cur);
        PA.nCopyObjects = (int)A.objects.size(); PA.nCopyScull = (int)A.scull.size();
    }
    PA.ids = ids; PA.world = world; PA.inv = inv; PA.wbb = wbb; PA.n = n; PA.nObjects = (int)s->host->objects.size();
    PA.objects = pose_objects(s, v); PA.scull = pose_scull(s, v);
    PA.posStart = s->scullPosStart.p; PA.pos = s->scullPos.p; PA.objMesh = s->objMesh.p; PA.meshes = s->meshes.p;
    PA.wbbOut = s->wbbDev.p; PA.safety = s->host->cullSafety;
    launch_pose(PA, ps);
    HIPCHECK(hipGetLastError());
    if ((rc = P.ready.create())) return rc;
    HIPCHECK(hipEventRecord(P.ready, ps));
    if (st != ps) HIPCHECK(hipStreamWaitEvent(st, P.ready, 0));
    P.serial = ++s->poseSerial;
    s->poseCur = v;
    return XRT_OK;
}

// Stage one material update: the host's MaterialRecs and the texels version v lacks become the newest version.  The version written is the
// current one unless an open ticket reads it; then a free one.  Every version is written from the HOST's arrays (which hold the newest
// materials as a whole), so no version is copied from another: the records are a few bytes per mesh, and of the arena only the words the
// version is behind in.  Nothing here touches a stream: the data is put into the version's page-locked staging and the first frame or ray
// batch that reads the version enqueues the copies on its own stream (mat_acquire).  Caller holds apiMutex and the scene (BusyGuard).
int materials_stage(xrt_scene *s, const HostScene::MaterialEdit &edit) {
    const SceneArrays &A = s->host->arrays;
    auto widen = [](xrt_scene::MatVer &m, size_t lo, size_t hi) {
        if (hi <= lo) return;
        if (m.texHi == m.texLo) { m.texLo = lo; m.texHi = hi; }
        else { m.texLo = std::min(m.texLo, lo); m.texHi = std::max(m.texHi, hi); }
    };
    for (auto &m : s->mat) {   // what every version is behind in now
        if (!edit.texels) break;
        if (edit.texFull) m.texFull = true;
        else widen(m, edit.texLo, edit.texHi);
    }
    if (!mat_referenced(s, 0) && !mat_referenced(s, 1) && !mat_referenced(s, 2)) {   // (no ticket open: freeing waits for nothing)
        s->matRetired.clear();
        for (auto &r : s->replicas) { (void)hipSetDevice(r->device); r->matRetired.clear(); }
        HIPCHECK(hipSetDevice(s->device));
    }
    const int cur = s->matCur;
    int v = cur;
    if (mat_referenced(s, v))
        for (int x = 0; x < 3; x++) if (x != cur && !mat_referenced(s, x)) { v = x; break; }
    if (mat_referenced(s, v)) return fail(XRT_E_INTERNAL, "xrt_scene_set_materials: no free material version");
    xrt_scene::MatVer &M = s->mat[v];
    DevBuf<MaterialRec> &recs = mat_records(s, v);
    DevBuf<uint32_t> &tex = mat_texels(s, v);
    int rc;
    const size_t nMat = A.materials.size(), nTex = A.texels.size();
    // No open ticket reads v, so every reader of its last write has ended, and with it the copies out of the staging (they ran ahead of that
    // reader on its stream); a write that nobody read yet was never copied and is staged again with this one.  (The wait is for a reader
    // whose enqueue failed half way: the copies may have been enqueued with nothing behind them to wait for.)
    if (M.pending) widen(M, M.stagedLo, M.stagedHi);
    else if (M.ready) HIPCHECK(hipEventSynchronize(M.ready));
    if (!tex.p || tex.cap < nTex || M.texCount != nTex) M.texFull = true;
    if ((rc = recs.ensure(nMat)) || (rc = mat_texel_room(s, tex, nTex))) return rc;
    const size_t lo = M.texFull ? 0 : std::min(M.texLo, nTex), hi = M.texFull ? nTex : std::min(M.texHi, nTex);
    const size_t recBytes = (nMat * sizeof(MaterialRec) + 15) / 16 * 16, texWords = hi > lo ? hi - lo : 0;
    if ((rc = M.staging.ensure(recBytes + texWords * sizeof(uint32_t), hipHostMallocDefault))) return rc;
    std::memcpy(M.staging.p, A.materials.data(), nMat * sizeof(MaterialRec));
    if (texWords) std::memcpy((char *)M.staging.p + recBytes, A.texels.data() + lo, texWords * sizeof(uint32_t));
    M.stagedRecBytes = recBytes; M.stagedMat = nMat; M.stagedLo = lo; M.stagedHi = lo + texWords;
    M.pending = true;
    M.texFull = false; M.texLo = M.texHi = 0; M.texCount = nTex;
    M.anyTransparent = A.anyTransparent;
    M.serial = ++s->matSerial;
    s->matCur = v;
    return XRT_OK;
}

// hs's poses <- the device's current version (after xrt_scene_set_poses_device): what xrt_scene_build_tree and xrt_scene_save read.
int pull_poses(xrt_scene *s) {
    if (!s->posesOnDevice) return XRT_OK;
    HIPCHECK(hipSetDevice(s->device));
    if (s->poseStream) HIPCHECK(hipStreamSynchronize(s->poseStream));
    const size_t nObj = s->hs.objects.size();
    std::vector<ObjRec> recs(nObj);
    std::vector<float> wbb(6 * nObj);
    if (nObj) {
        HIPCHECK(hipMemcpy(recs.data(), pose_objects(s, s->poseCur), nObj * sizeof(ObjRec), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(wbb.data(), s->wbbDev.p, 6 * nObj * sizeof(float), hipMemcpyDeviceToHost));
    }
    std::string err;
    for (size_t o = 0; o < nObj; o++)
        if (!s->hs.set_pose((int)o, recs[o].world, recs[o].invWorld, &wbb[6 * o], err)) return fail(XRT_E_INTERNAL, "%s", err.c_str());
    s->posesOnDevice = false;
    return XRT_OK;
}

// Enqueue one update of triangle values: entries [0, n) of the device arrays (kernels.h TriShadingArgs; T.shade is set here), ready on `st`,
// are written into the newest version.  The version written is the current one unless an open ticket reads it; then a free one, brought up
// to date from the current one first by a device-to-device copy.  Nothing here waits for the device: copy and kernel run on shadeStream
// behind `st` -- every write of every version runs there, so the copy follows the current version's last write --, and `st` continues
// behind the update (the caller may refill its arrays there).  A version no open ticket reads has no reader left: a ticket's frame is
// finished when it is closed, a ray batch before its call returns.  Caller holds apiMutex and the scene (BusyGuard).
int shading_enqueue(xrt_scene *s, TriShadingArgs T, hipStream_t st) {
    const int cur = s->shadeCur;
    int v = cur;
    if (shade_referenced(s, v))
        for (int x = 0; x < 3; x++) if (x != cur && !shade_referenced(s, x)) { v = x; break; }
    if (shade_referenced(s, v)) return fail(XRT_E_INTERNAL, "xrt_scene_set_triangle_shading: no free version");
    xrt_scene::ShadeVer &P = s->shadeVer[v];
    const size_t count = s->shadeCount;
    int rc;
    if ((rc = s->shadeStream.create()) || (rc = s->shadeInput.create())) return rc;
    hipStream_t ps = s->shadeStream;
    if (st != ps) {
        HIPCHECK(hipEventRecord(s->shadeInput, st));
        HIPCHECK(hipStreamWaitEvent(ps, s->shadeInput, 0));
    }
    if (v != cur) {
        if ((rc = shade_records(s, v).ensure(count))) return rc;   // (versions 1 and 2 are allocated here, when they are first written; version 0 is the scene's own array)
        HIPCHECK(hipMemcpyAsync(shade_records(s, v).p, shade_records(s, cur).p, count * sizeof(f4), hipMemcpyDeviceToDevice, ps));
    }
    T.shade = shade_records(s, v).p;
    T.meshes = s->meshes.p;
    launch_tri_shading(T, ps);
    HIPCHECK(hipGetLastError());
    if ((rc = P.ready.create())) return rc;
    HIPCHECK(hipEventRecord(P.ready, ps));
    if (st != ps) HIPCHECK(hipStreamWaitEvent(st, P.ready, 0));
    P.serial = ++s->shadeSerial;
    s->shadeCur = v;
    return XRT_OK;
}

// hs's triangle values <- the device's current version (after xrt_scene_set_triangle_shading_device): what xrt_scene_save, xrt_scene_build and
// the uploads of xrt_scene_set_bodies read.  The device holds the meshes `shade` was uploaded with; the host has had none removed since.
int pull_shading(xrt_scene *s) {
    if (!s->shadeOnDevice) return XRT_OK;
    HIPCHECK(hipSetDevice(s->device));
    if (s->shadeStream) HIPCHECK(hipStreamSynchronize(s->shadeStream));
    const SceneArrays &A = s->hs.arrays;
    const f4 *dev = shade_records(s, s->shadeCur).p;
    std::vector<f4> recs;
    for (int m = 0; m < s->hs.builtMeshes && m < (int)A.meshes.size(); m++) {
        const size_t base = (size_t)SHADE_F4 * (size_t)A.meshes[(size_t)m].triBase, n = (size_t)SHADE_F4 * (size_t)A.meshes[(size_t)m].ntri;
        if (base + n > s->shadeCount) break;   // (a mesh built after the upload: the device never held it)
        if (n == 0) continue;
        recs.resize(n);
        HIPCHECK(hipMemcpy(recs.data(), dev + base, n * sizeof(f4), hipMemcpyDeviceToHost));
        s->hs.take_triangle_shading(m, recs.data());
    }
    s->shadeOnDevice = false;
    return XRT_OK;
}

}  // namespace

// Every render entry point funnels through these two: no C++ exception (std::bad_alloc from a host-side vector, ...) crosses the C boundary.
int open_frame(xrt_scene *s, int slot, const xrt_camera *cam, const xrt_light *lights, int nLights, const xrt_render_opts *opts, uint32_t *d_out,
               float *d_outF32, uint32_t *host_out, hipStream_t st) {
    return guarded("xrt_render", [&]() -> int { return open_frame_impl(s, slot, cam, lights, nLights, opts, d_out, d_outF32, host_out, st); });
}
int close_frame(xrt_scene *s, int slot, xrt_stats *stats) {
    return guarded("xrt_render_end", [&]() -> int { return close_frame_impl(s, slot, stats); });
}

extern "C" {

int xrt_version(void) { return XRT_VERSION; }
const char *xrt_last_error(void) { return g_err.c_str(); }

int xrt_device_count(int *count_out) {
    if (!count_out) return fail(XRT_E_INVALID_ARG, "xrt_device_count: null argument");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count_out = 0; (void)hipGetLastError(); return XRT_OK; }
    *count_out = n;
    return XRT_OK;
}

int xrt_scene_create(int device, xrt_scene **scene_out) {
    if (!scene_out) return fail(XRT_E_INVALID_ARG, "xrt_scene_create: null argument");
    *scene_out = nullptr;
    const Settings cfg = read_settings();
    if (cfg.guard) g_guardMode.store(*cfg.guard ? 1 : 0);
    if (device < -1) return fail(XRT_E_INVALID_ARG, "xrt_scene_create: bad device index");
    if (device >= 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return fail(XRT_E_NO_DEVICE, "no HIP device visible; libxrt has no CPU execution path"); }
        if (device >= n) return fail(XRT_E_NO_DEVICE, "device %d not present (%d visible)", device, n);
        HIPCHECK(hipSetDevice(device));
    }
    std::unique_ptr<xrt_scene> s(new xrt_scene());
    s->device = device;
    if (device >= 0 && hipGetDeviceCount(&s->visibleDevices) != hipSuccess) { (void)hipGetLastError(); s->visibleDevices = 0; }
    s->cfg = cfg;
    if (cfg.spatialRuns) s->hs.spatialRuns = *cfg.spatialRuns;
#ifdef XRT_DEV
    if (cfg.leafCullSafety) s->hs.leafCullSafety = *cfg.leafCullSafety;
    if (cfg.cullSafety) s->hs.cullSafety = *cfg.cullSafety;
#endif
    if (device >= 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) s->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        if (hipDeviceGetAttribute(&s->wallClockKHz, hipDeviceAttributeWallClockRate, device) != hipSuccess) { s->wallClockKHz = 0; (void)hipGetLastError(); }
        hipError_t e = hipStreamCreateWithFlags(&s->stream.h, hipStreamNonBlocking);
        if (e != hipSuccess) return fail(XRT_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    *scene_out = s.release();
    return XRT_OK;
}

int xrt_scene_destroy(xrt_scene *scene) {
    if (!scene) return XRT_OK;
    if (in_flight(scene)) return fail(XRT_E_BUSY, "xrt_scene_destroy: a render is in flight");
    delete scene;
    return XRT_OK;
}

int xrt_scene_add_mesh(xrt_scene *scene, const float *v, const float *n, const float *uv, const float *surf_n, const float *color,
                       int32_t ntri, const xrt_material *material, const float bbox[6], int32_t *mesh_id_out) {
    if (!scene || !mesh_id_out) return fail(XRT_E_INVALID_ARG, "xrt_scene_add_mesh: null argument");
    if (in_flight(scene)) return fail(XRT_E_BUSY, "scene is rendering");
    return guarded("xrt_scene_add_mesh", [&]() -> int {
        std::string err;
        int id = scene->hs.add_mesh(v, n, uv, surf_n, color, ntri, material, bbox, err);
        if (id < 0) return fail(XRT_E_INVALID_ARG, "%s", err.c_str());
        scene->resident = false;
        *mesh_id_out = id;
        return XRT_OK;
    });
}

int xrt_scene_add_object(xrt_scene *scene, const int32_t *mesh_ids, int32_t n_meshes, const float world[16], const float inv_world[16],
                         const float bbox[6], const float world_bbox[6], int32_t *object_id_out) {
    if (!scene || !object_id_out) return fail(XRT_E_INVALID_ARG, "xrt_scene_add_object: null argument");
    if (in_flight(scene)) return fail(XRT_E_BUSY, "scene is rendering");
    return guarded("xrt_scene_add_object", [&]() -> int {
        std::string err;
        int id = scene->hs.add_object(mesh_ids, n_meshes, world, inv_world, bbox, world_bbox, err);
        if (id < 0) return fail(XRT_E_INVALID_ARG, "%s", err.c_str());
        scene->resident = false;
        *object_id_out = id;
        return XRT_OK;
    });
}

int xrt_scene_build(xrt_scene *scene, int32_t mesh_threshold, int32_t scene_threshold) {
    if (!scene) return fail(XRT_E_INVALID_ARG, "xrt_scene_build: null scene");
    if (in_flight(scene)) return fail(XRT_E_BUSY, "scene is rendering");
    return guarded("xrt_scene_build", [&]() -> int {
        std::string err;
        int rc;
        if (scene->device >= 0 && (rc = pull_shading(scene))) return rc;   // (the build starts from the host copy: it holds the values set on the device)
        scene->resident = false;
        if (!scene->hs.build(mesh_threshold, scene_threshold, err)) return fail(XRT_E_UNSUPPORTED, "%s", err.c_str());
        scene->workers.clear();
        scene->replicas.clear();   // copies of the previous build on other devices
        return scene_upload(scene);
    });
}

int xrt_scene_set_poses(xrt_scene *scene, const int32_t *object_ids, int32_t n, const float *world, const float *inv_world,
                        const float *world_bbox) {
    if (!scene) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_poses: null scene");
    if (n < 0 || (n > 0 && (!object_ids || !world || !inv_world || !world_bbox))) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_poses: null argument");
    const int nObj = (int)scene->hs.objects.size();
    for (int i = 0; i < n; i++)
        if (object_ids[i] < 0 || object_ids[i] >= nObj) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_poses: object id %d out of range (%d bodies)", object_ids[i], nObj);
    if (n == 0) return XRT_OK;
    std::lock_guard<std::mutex> lock(scene->apiMutex);
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "xrt_scene_set_poses: another call is rendering on the scene");
    return guarded("xrt_scene_set_poses", [&]() -> int {
        // the last entry of a body wins (the setters called one after the other); the host copy first: save and the next build read it
        // (after an update from device arrays the other bodies' host poses stay behind until pull_poses: the device's version has them all)
        std::vector<int> last((size_t)nObj, -1), order;
        for (int i = 0; i < n; i++) last[(size_t)object_ids[i]] = i;
        for (int i = 0; i < n; i++) if (last[(size_t)object_ids[i]] == i) order.push_back(i);
        const bool onDevice = scene->device >= 0 && scene->hs.built && scene->resident;
        std::string err;
        for (int i : order)
            if (!scene->hs.set_pose(object_ids[i], world + 16 * (size_t)i, inv_world + 16 * (size_t)i, world_bbox + 6 * (size_t)i, err))
                return fail(XRT_E_INVALID_ARG, "%s", err.c_str());
        if (!onDevice) return XRT_OK;
        HIPCHECK(hipSetDevice(scene->device));
        // staging: ids | world | inv | wbb in page-locked memory, one asynchronous copy to the device
        const size_t m = order.size(), idWords = (m + 3) / 4 * 4, words = idWords + m * (16 + 16 + 6);
        if (scene->poseStaged) HIPCHECK(hipEventSynchronize(scene->poseStaged));   // (the previous update's copy of a few KB)
        int rc;
        if ((rc = scene->posePinned.ensure(words * 4, hipHostMallocDefault)) || (rc = scene->poseIn.ensure(words))) return rc;
        int *hid = (int *)scene->posePinned.p;
        float *hw = (float *)scene->posePinned.p + idWords, *hi = hw + 16 * m, *hb = hi + 16 * m;
        for (size_t k = 0; k < m; k++) {
            const size_t i = (size_t)order[k];
            hid[k] = object_ids[i];
            std::memcpy(hw + 16 * k, world + 16 * i, 64); std::memcpy(hi + 16 * k, inv_world + 16 * i, 64); std::memcpy(hb + 6 * k, world_bbox + 6 * i, 24);
        }
        if ((rc = scene->poseStream.create()) || (rc = scene->poseStaged.create())) return rc;
        HIPCHECK(hipMemcpyAsync(scene->poseIn.p, scene->posePinned.p, words * 4, hipMemcpyHostToDevice, scene->poseStream));
        HIPCHECK(hipEventRecord(scene->poseStaged, scene->poseStream));
        const float *dw = scene->poseIn.p + idWords;
        return poses_enqueue(scene, (const int *)scene->poseIn.p, (int)m, dw, dw + 16 * m, dw + 32 * m, scene->poseStream);
    });
}

int xrt_scene_set_poses_device(xrt_scene *scene, const void *d_object_ids, int32_t n, const void *d_world, const void *d_inv_world,
                               const void *d_world_bbox, void *stream) {
    if (!scene) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_poses_device: null scene");
    if (n < 0 || (n > 0 && (!d_object_ids || !d_world || !d_inv_world || !d_world_bbox))) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_poses_device: null argument");
    if (((uintptr_t)d_object_ids & 15) || ((uintptr_t)d_world & 15) || ((uintptr_t)d_inv_world & 15) || ((uintptr_t)d_world_bbox & 15))
        return fail(XRT_E_INVALID_ARG, "xrt_scene_set_poses_device: device arrays must be 16-byte aligned");
    int rc = need_device(scene, "xrt_scene_set_poses_device");
    if (rc != XRT_OK) return rc;
    if (n == 0) return XRT_OK;
    std::lock_guard<std::mutex> lock(scene->apiMutex);
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "xrt_scene_set_poses_device: another call is rendering on the scene");
    return guarded("xrt_scene_set_poses_device", [&]() -> int {
        hipStream_t st = stream ? (hipStream_t)stream : scene->stream;
        if ((rc = poses_enqueue(scene, (const int *)d_object_ids, n, (const float *)d_world, (const float *)d_inv_world, (const float *)d_world_bbox, st)))
            return rc;
        scene->posesOnDevice = true;
        return XRT_OK;
    });
}

int xrt_scene_set_materials(xrt_scene *scene, const int32_t *mesh_ids, int32_t n, const xrt_material *materials) {
    if (!scene) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_materials: null scene");
    if (n < 0 || (n > 0 && (!mesh_ids || !materials))) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_materials: null argument");
    if (n == 0) return XRT_OK;
    std::lock_guard<std::mutex> lock(scene->apiMutex);
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "xrt_scene_set_materials: another call is rendering on the scene");
    return guarded("xrt_scene_set_materials", [&]() -> int {
        // the host copy first (checked as a whole before anything is applied): save and the next build read it, and the device's
        // newest version is written from it
        std::string err;
        HostScene::MaterialEdit edit;
        if (!scene->hs.set_materials(mesh_ids, n, materials, edit, err)) return fail(XRT_E_INVALID_ARG, "%s", err.c_str());
        if (!(scene->device >= 0 && scene->hs.built && scene->resident)) return XRT_OK;
        HIPCHECK(hipSetDevice(scene->device));
        return materials_stage(scene, edit);
    });
}

int xrt_scene_set_triangle_shading(xrt_scene *scene, int32_t mesh_id, const int32_t *tri_ids, int32_t first_tri, int32_t n, const float *normals,
                                   const float *uv, const float *color) {
    if (!scene) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_triangle_shading: null scene");
    std::lock_guard<std::mutex> lock(scene->apiMutex);
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "xrt_scene_set_triangle_shading: another call is rendering on the scene");
    return guarded("xrt_scene_set_triangle_shading", [&]() -> int {
        // the host copy first (checked as a whole before anything is applied): save and the next build read it
        std::string err;
        if (!scene->hs.set_triangle_shading(mesh_id, tri_ids, first_tri, n, normals, uv, color, err)) return fail(XRT_E_INVALID_ARG, "%s", err.c_str());
        if (n == 0 || !(scene->device >= 0 && scene->hs.built && scene->resident)) return XRT_OK;
        HIPCHECK(hipSetDevice(scene->device));
        // of a triangle listed twice the last entry counts: the kernel's ids must be distinct, so only that entry is staged
        std::vector<int> order;
        if (tri_ids) {
            std::vector<int> last((size_t)scene->hs.meshes[(size_t)mesh_id].ntri, -1);
            for (int i = 0; i < n; i++) last[(size_t)tri_ids[i]] = i;
            for (int i = 0; i < n; i++) if (last[(size_t)tri_ids[i]] == i) order.push_back(i);
        }
        const size_t m = tri_ids ? order.size() : (size_t)n;
        const bool whole = !tri_ids || m == (size_t)n;   // (no entry dropped: the arrays are staged as they are)
        // staging: ids | normals | uv | color in page-locked memory, every part 16-byte aligned, one asynchronous copy to the device
        auto pad = [](size_t w) { return (w + 3) / 4 * 4; };
        const size_t wIds = tri_ids ? pad(m) : 0, wN = normals ? pad(9 * m) : 0, wUv = uv ? pad(6 * m) : 0, wC = color ? 4 * m : 0;
        const size_t words = wIds + wN + wUv + wC;
        if (scene->shadeStaged) HIPCHECK(hipEventSynchronize(scene->shadeStaged));   // (the previous update's copy)
        int rc;
        if ((rc = scene->shadePinned.ensure(words * 4, hipHostMallocDefault)) || (rc = scene->shadeIn.ensure(words))) return rc;
        uint32_t *h = (uint32_t *)scene->shadePinned.p;
        auto stage = [&](uint32_t *dst, const void *src, size_t per) {
            if (whole) { std::memcpy(dst, src, m * per * 4); return; }
            for (size_t k = 0; k < m; k++) std::memcpy(dst + per * k, (const uint32_t *)src + per * (size_t)order[k], per * 4);
        };
        if (tri_ids) stage(h, tri_ids, 1);
        if (normals) stage(h + wIds, normals, 9);
        if (uv) stage(h + wIds + wN, uv, 6);
        if (color) stage(h + wIds + wN + wUv, color, 4);
        if ((rc = scene->shadeStream.create()) || (rc = scene->shadeStaged.create())) return rc;
        HIPCHECK(hipMemcpyAsync(scene->shadeIn.p, h, words * 4, hipMemcpyHostToDevice, scene->shadeStream));
        HIPCHECK(hipEventRecord(scene->shadeStaged, scene->shadeStream));
        const uint32_t *d = scene->shadeIn.p;
        TriShadingArgs T;
        T.ids = tri_ids ? (const int *)d : nullptr; T.first = first_tri; T.n = (int)m; T.mesh = mesh_id;
        T.normals = normals ? d + wIds : nullptr; T.uv = uv ? d + wIds + wN : nullptr; T.color = color ? d + wIds + wN + wUv : nullptr;
        return shading_enqueue(scene, T, scene->shadeStream);
    });
}

int xrt_scene_set_triangle_shading_device(xrt_scene *scene, int32_t mesh_id, const void *d_tri_ids, int32_t first_tri, int32_t n, const void *d_normals,
                                          const void *d_uv, const void *d_color, void *stream) {
    const char *fn = "xrt_scene_set_triangle_shading_device";
    if (!scene) return fail(XRT_E_INVALID_ARG, "%s: null scene", fn);
    int rc = need_device(scene, fn);
    if (rc != XRT_OK) return rc;
    if (mesh_id < 0 || mesh_id >= (int)scene->hs.arrays.meshes.size() || mesh_id >= scene->hs.builtMeshes)
        return fail(XRT_E_INVALID_ARG, "%s: mesh id %d out of range", fn, mesh_id);
    if (n < 0 || first_tri < 0) return fail(XRT_E_INVALID_ARG, "%s: negative count or first triangle", fn);
    if (d_tri_ids && first_tri != 0) return fail(XRT_E_INVALID_ARG, "%s: first_tri must be 0 with a list of triangle ids", fn);
    if (n > 0 && !d_normals && !d_uv && !d_color) return fail(XRT_E_INVALID_ARG, "%s: no field given", fn);
    if (((uintptr_t)d_tri_ids & 15) || ((uintptr_t)d_normals & 15) || ((uintptr_t)d_uv & 15) || ((uintptr_t)d_color & 15))
        return fail(XRT_E_INVALID_ARG, "%s: device arrays must be 16-byte aligned", fn);
    if (n == 0) return XRT_OK;
    std::lock_guard<std::mutex> lock(scene->apiMutex);
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "%s: another call is rendering on the scene", fn);
    return guarded(fn, [&]() -> int {
        TriShadingArgs T;
        T.ids = (const int *)d_tri_ids; T.first = first_tri; T.n = n; T.mesh = mesh_id;
        T.normals = (const uint32_t *)d_normals; T.uv = (const uint32_t *)d_uv; T.color = (const uint32_t *)d_color;
        if ((rc = shading_enqueue(scene, T, stream ? (hipStream_t)stream : scene->stream))) return rc;
        scene->shadeOnDevice = true;
        return XRT_OK;
    });
}

int xrt_scene_build_tree(xrt_scene *scene, int32_t scene_threshold) {
    if (!scene) return fail(XRT_E_INVALID_ARG, "xrt_scene_build_tree: null scene");
    if (in_flight(scene)) return fail(XRT_E_BUSY, "xrt_scene_build_tree: a frame is in flight");
    if (!scene->hs.built) return fail(XRT_E_NOT_BUILT, "xrt_scene_build_tree: call xrt_scene_build first");
    std::lock_guard<std::mutex> lock(scene->apiMutex);
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "xrt_scene_build_tree: a frame is in flight");
    return guarded("xrt_scene_build_tree", [&]() -> int {
        int rc;
        if (scene->device >= 0 && scene->resident && (rc = pull_poses(scene))) return rc;
        std::string err;
        scene->resident = false;
        if (!scene->hs.build_tree(scene_threshold, err)) return fail(XRT_E_UNSUPPORTED, "%s", err.c_str());
        scene->workers.clear();
        scene->replicas.clear();   // (copies of the previous tree: made again on the next n_gpus > 1 frame)
        const SceneArrays &A = scene->hs.arrays;
        const int stackNeeded = (A.sceneDepth + 1) + (A.meshDepth + 1);
        if (intersect_stack_capacity(stackNeeded) < 0) return fail(XRT_E_UNSUPPORTED, "octree too deep for the LDS stack (%d levels)", stackNeeded);
        scene->stackNeeded = stackNeeded;
        if (scene->device < 0) return XRT_OK;
        HIPCHECK(hipSetDevice(scene->device));
        if (scene->poseStream) HIPCHECK(hipStreamSynchronize(scene->poseStream));
        if ((rc = tree_upload(scene))) return rc;
        return scene_derive(scene);
    });
}

int xrt_scene_set_bodies(xrt_scene *scene, int32_t n_bodies, const int32_t *mesh_start, const int32_t *mesh_ids, const float *world,
                         const float *inv_world, const float *bbox, const float *world_bbox, int32_t scene_threshold, int32_t *meshes_built_out) {
    if (!scene) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_bodies: null scene");
    if (in_flight(scene)) return fail(XRT_E_BUSY, "xrt_scene_set_bodies: a frame is in flight");
    if (scene->hs.builtMeshes < 0) return fail(XRT_E_NOT_BUILT, "xrt_scene_set_bodies: call xrt_scene_build first");
    std::lock_guard<std::mutex> lock(scene->apiMutex);
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "xrt_scene_set_bodies: a frame is in flight");
    return guarded("xrt_scene_set_bodies", [&]() -> int {
        // Only a scene whose device copy is whole and current (built, resident, no mesh waiting) takes the short upload below.
        const bool current = scene->hs.built && scene->resident;
        std::string err;
        int built = 0;
        // Triangle values set on the device are the scene's, not the old list's: read back before `shade` may be sent again.
        if (scene->device >= 0) if (int prc = pull_shading(scene)) return prc;
        const int hrc = scene->hs.set_bodies(n_bodies, mesh_start, mesh_ids, world, inv_world, bbox, world_bbox, scene_threshold, built, err);
        if (hrc == XRT_E_INVALID_ARG || hrc == XRT_E_NOT_BUILT) return fail(hrc, "%s", err.c_str());   // (nothing was applied)
        scene->resident = false;
        // The call supplies every pose: what xrt_scene_set_poses_device left on the device belongs to the old list and is not read back.
        scene->posesOnDevice = false;
        scene->workers.clear();
        scene->replicas.clear();   // (copies of the previous list: made again on the next n_gpus > 1 frame)
        // What earlier frames left behind, one by one.  No buffer is sized from any of it: every frame sizes its work buffers from its own
        // geometry and options and from the arrays as they are now (ensure() at its begin).
        //  - genKey / genRays / genShade / genCompose: grid sizes of the next frame's launches, learned from the old list.  Scheduling only
        //    (persistent grids, any size is correct), but worthless for another list: forgotten.
        scene->genKey = -1; scene->genCompose = -1;
        //  - costMap / costT / epoch ("long ray first"): the order rays are started in.  Scheduling only; costT is set again by scene_derive.
        //  - tileCost / costTiles / balanceCost and an installed tile table: which rank renders which tile; every table is a permutation of
        //    the frame's tiles whatever the scene holds.  Scheduling only, and the table is the caller's: kept.
        //  - lvlCheckedTilesX / lvlCheckedTiles: arithmetic of a frame geometry, independent of the scene: kept.
        //  - heavyPath / heavyShift / refillMin / firstBatch / deepMeshes / blocksPerCU* / packetOk / sceneMode: follow the list; scene_derive
        //    sets every one of them again below.
        //  - adaptiveFastOk / heapFastOk: "the optimistic way overflowed once"; the other way is always right, and a frame that overflows
        //    is rendered again.  Kept.
        //  - splitCost of the frame contexts: packet costs of the last frame, keyed by the frame's size; scheduling only.  Kept.
        if (meshes_built_out) *meshes_built_out = built;   // (this call's own count, on every path that applied the list: also when the scene octree or the stack check fails below)
        if (hrc != XRT_OK) return fail(hrc, "%s", err.c_str());
        const SceneArrays &A = scene->hs.arrays;
        const int stackNeeded = (A.sceneDepth + 1) + (A.meshDepth + 1);
        if (intersect_stack_capacity(stackNeeded) < 0) return fail(XRT_E_UNSUPPORTED, "octree too deep for the LDS stack (%d levels)", stackNeeded);
        scene->stackNeeded = stackNeeded;
        if (scene->device < 0) return XRT_OK;
        HIPCHECK(hipSetDevice(scene->device));
        if (scene->poseStream) HIPCHECK(hipStreamSynchronize(scene->poseStream));
        if (built > 0 || !current) return scene_upload(scene);   // no frame is in flight: everything again
        int rc;
        if ((rc = upload(scene->objMesh, A.objMesh)) || (rc = tree_upload(scene))) return rc;
        // the host's materials are the newest; version 0 takes them and the versions start again, as after a build
        if ((rc = upload(scene->materials, A.materials)) || (rc = upload(scene->texels, A.texels))) return rc;
        material_restart(scene);
        return scene_derive(scene);
    });
}

int xrt_scene_set_mesh_triangles(xrt_scene *scene, int32_t mesh_id, const float *v, const float *n, const float *uv, const float *surf_n,
                                 const float *color, int32_t ntri, const float bbox[6]) {
    if (!scene) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_mesh_triangles: null scene");
    if (in_flight(scene)) return fail(XRT_E_BUSY, "xrt_scene_set_mesh_triangles: a frame is in flight");
    std::lock_guard<std::mutex> lock(scene->apiMutex);
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "xrt_scene_set_mesh_triangles: a frame is in flight");
    return guarded("xrt_scene_set_mesh_triangles", [&]() -> int {
        // Where `arrays` holds the mesh its part is replaced there and the device copy made again; else the next build reads the new triangles.
        const bool spliced = mesh_id >= 0 && mesh_id < scene->hs.builtMeshes;
        // What was set on the device is the scene's: the triangle values (of the other meshes) are read back before `shade` is sent again, and
        // the poses too -- the call supplies none, and the pre-cull records it refreshes are made from the bodies' current poses.
        if (scene->device >= 0 && spliced) {
            int rc;
            if ((rc = pull_shading(scene))) return rc;
            if (scene->resident && (rc = pull_poses(scene))) return rc;
        }
        std::string err;
        const int hrc = scene->hs.set_mesh_triangles(mesh_id, v, n, uv, surf_n, color, ntri, bbox, err);
        if (hrc != XRT_OK) return fail(hrc, "%s", err.c_str());   // (nothing was applied: the scene is as it was, its device copy included)
        if (!spliced) return XRT_OK;
        scene->resident = false;
        scene->workers.clear();
        scene->replicas.clear();   // (copies of the old triangles: made again on the next n_gpus > 1 frame)
        // grid sizes learned from the old triangles (xrt_scene_set_bodies lists what else earlier frames leave behind: all of it is scheduling
        // only, keyed by the frame or set again by scene_derive; no buffer is sized from any of it)
        scene->genKey = -1; scene->genCompose = -1;
        if (!scene->hs.built) return XRT_OK;   // (meshes wait for xrt_scene_set_bodies: it sends everything)
        const SceneArrays &A = scene->hs.arrays;
        scene->stackNeeded = (A.sceneDepth + 1) + (A.meshDepth + 1);   // (it fits: the host edit checked it before it applied anything)
        if (scene->device < 0) return XRT_OK;
        HIPCHECK(hipSetDevice(scene->device));
        if (scene->poseStream) HIPCHECK(hipStreamSynchronize(scene->poseStream));
        if (scene->shadeStream) HIPCHECK(hipStreamSynchronize(scene->shadeStream));   // (an update of triangle values from host arrays may still be on its way)
        return scene_upload(scene);   // no frame is in flight: everything again (scene_derive, material_restart, shade_restart)
    });
}

int xrt_scene_save(const xrt_scene *scene, const char *path) {
    if (!scene || !path) return fail(XRT_E_INVALID_ARG, "xrt_scene_save: null argument");
    return guarded("xrt_scene_save", [&]() -> int {
        std::string err;
        xrt_scene *s = const_cast<xrt_scene *>(scene);   // (the poses last set on the device are read back first)
        if (s->device >= 0 && s->resident) {
            std::lock_guard<std::mutex> lock(s->apiMutex);
            int rc = pull_poses(s);
            if (rc != XRT_OK) return rc;
        }
        if (s->device >= 0 && s->shadeOnDevice) {   // (... and the triangle values; they outlive `resident`)
            std::lock_guard<std::mutex> lock(s->apiMutex);
            int rc = pull_shading(s);
            if (rc != XRT_OK) return rc;
        }
        if (!scene->hs.save(path, err)) return fail(XRT_E_INVALID_ARG, "%s (%s)", err.c_str(), path);
        return XRT_OK;
    });
}

int xrt_scene_load(int device, const char *path, xrt_scene **scene_out) {
    if (!scene_out || !path) return fail(XRT_E_INVALID_ARG, "xrt_scene_load: null argument");
    int rc = xrt_scene_create(device, scene_out);
    if (rc != XRT_OK) return rc;
    rc = guarded("xrt_scene_load", [&]() -> int {
        std::string err;
        if (!(*scene_out)->hs.load(path, err)) return fail(XRT_E_INVALID_ARG, "%s (%s)", err.c_str(), path);
        return XRT_OK;
    });
    if (rc != XRT_OK) { delete *scene_out; *scene_out = nullptr; }   // (the owners' destructors report nothing: the load's error stays)
    return rc;
}

int xrt_scene_get_tree(const xrt_scene *scene, int32_t mesh_id, xrt_node_info *nodes, int64_t *n_nodes_inout, int32_t *refs,
                       int64_t *n_refs_inout) {
    if (!scene || !n_nodes_inout || !n_refs_inout) return fail(XRT_E_INVALID_ARG, "xrt_scene_get_tree: null argument");
    if (!scene->hs.built) return fail(XRT_E_NOT_BUILT, "xrt_scene_get_tree: call xrt_scene_build first");
    if (mesh_id >= (int)scene->hs.meshTrees.size()) return fail(XRT_E_INVALID_ARG, "xrt_scene_get_tree: unknown mesh id");
    const FlatTree &t = mesh_id < 0 ? scene->hs.sceneTree : scene->hs.meshTrees[mesh_id];
    if (nodes) {
        if (*n_nodes_inout < (int64_t)t.info.size()) return fail(XRT_E_INVALID_ARG, "node array too small");
        if (!t.info.empty()) std::memcpy(nodes, t.info.data(), t.info.size() * sizeof(xrt_node_info));
    }
    if (refs) {
        if (*n_refs_inout < (int64_t)t.infoRefs.size()) return fail(XRT_E_INVALID_ARG, "ref array too small");
        if (!t.infoRefs.empty()) std::memcpy(refs, t.infoRefs.data(), t.infoRefs.size() * sizeof(int32_t));   // (an empty tree has no array to copy from)
    }
    *n_nodes_inout = (int64_t)t.info.size();
    *n_refs_inout = (int64_t)t.infoRefs.size();
    return XRT_OK;
}

int xrt_scene_intersect(xrt_scene *scene, const xrt_ray *rays, const int32_t *ignore_object, int64_t n, xrt_hit *hits_out, xrt_stats *stats_out) {
    (void)ignore_object;   // dead in the reference (OSM:343), SURVEY Q8
    int rc = need_device(scene, "xrt_scene_intersect");
    if (rc != XRT_OK) return rc;
    if (n < 0 || (n > 0 && (!rays || !hits_out))) return fail(XRT_E_INVALID_ARG, "xrt_scene_intersect: null argument");
    std::lock_guard<std::mutex> lock(scene->apiMutex);   // concurrent callers (RT:105-113) take turns on the staging buffers
    if ((rc = scene->apiRays.ensure((size_t)n)) || (rc = scene->apiHits.ensure((size_t)n))) return rc;
    hipStream_t st = scene->stream;
    if (n > 0) HIPCHECK(hipMemcpyAsync(scene->apiRays.p, rays, (size_t)n * sizeof(xrt_ray), hipMemcpyHostToDevice, st));
    if ((rc = run_intersect(scene, scene->apiRays.p, n, scene->apiHits.p, scene->sceneMode, 0, st, stats_out, false))) return rc;
    if (n > 0) HIPCHECK(hipMemcpyAsync(hits_out, scene->apiHits.p, (size_t)n * sizeof(xrt_hit), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return guards_check("end of a batched query");
}

int xrt_scene_intersect_device(xrt_scene *scene, const void *d_rays, int64_t n, void *d_hits_out, void *stream) {
    int rc = need_device(scene, "xrt_scene_intersect_device");
    if (rc != XRT_OK) return rc;
    if (n < 0 || (n > 0 && (!d_rays || !d_hits_out))) return fail(XRT_E_INVALID_ARG, "xrt_scene_intersect_device: null argument");
    if (((uintptr_t)d_rays & 15) || ((uintptr_t)d_hits_out & 15)) return fail(XRT_E_INVALID_ARG, "device buffers must be 16-byte aligned");
    std::lock_guard<std::mutex> lock(scene->apiMutex);   // (held for the enqueue only: the call is asynchronous)
    if ((rc = run_intersect(scene, (const xrt_ray *)d_rays, n, (xrt_hit *)d_hits_out, scene->sceneMode, 0, (hipStream_t)stream, nullptr, false))) return rc;
    return pose_reader(scene, scene->poseCur, (hipStream_t)stream);
}

int xrt_mesh_intersect(xrt_scene *scene, int32_t mesh_id, const xrt_ray *rays, int64_t n, xrt_hit *hits_out) {
    int rc = need_device(scene, "xrt_mesh_intersect");
    if (rc != XRT_OK) return rc;
    if (mesh_id < 0 || mesh_id >= (int)scene->hs.meshes.size()) return fail(XRT_E_INVALID_ARG, "xrt_mesh_intersect: unknown mesh id");
    if (n < 0 || (n > 0 && (!rays || !hits_out))) return fail(XRT_E_INVALID_ARG, "xrt_mesh_intersect: null argument");
    std::lock_guard<std::mutex> lock(scene->apiMutex);
    if ((rc = scene->apiRays.ensure((size_t)n)) || (rc = scene->apiHits.ensure((size_t)n))) return rc;
    hipStream_t st = scene->stream;
    if (n > 0) HIPCHECK(hipMemcpyAsync(scene->apiRays.p, rays, (size_t)n * sizeof(xrt_ray), hipMemcpyHostToDevice, st));
    if ((rc = run_intersect(scene, scene->apiRays.p, n, scene->apiHits.p, MODE_MESH, mesh_id, st, nullptr, false))) return rc;
    if (n > 0) HIPCHECK(hipMemcpyAsync(hits_out, scene->apiHits.p, (size_t)n * sizeof(xrt_hit), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return guards_check("end of a batched query");
}

int xrt_render(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
               uint32_t *rgba_out, float *rgb_f32_out, xrt_stats *stats_out) {
    int rc = need_device(scene, "xrt_render");
    if (rc != XRT_OK) return rc;
    if (!camera || !opts || !rgba_out) return fail(XRT_E_INVALID_ARG, "xrt_render: null argument");
    if (opts->shard_count > 1) return fail(XRT_E_INVALID_ARG, "xrt_render writes a whole frame; use xrt_render_device for shards");
    BusyGuard guard(scene);
    if (!guard.owned || scene->frames[0].pending || scene->frames[1].pending)
        return fail(XRT_E_BUSY, "Current render operation not finished.");   // RT:62-63
    if (camera->vp_width <= 0 || camera->vp_height <= 0) return fail(XRT_E_INVALID_ARG, "viewport must be positive");
    const size_t px = (size_t)camera->vp_width * (size_t)camera->vp_height;
    if (rgb_f32_out && (rc = scene->outF32.ensure(px * 3))) return rc;
    if ((rc = open_frame(scene, 0, camera, lights, n_lights, opts, nullptr, rgb_f32_out ? scene->outF32.p : nullptr, rgba_out, nullptr))) return rc;
    if ((rc = close_frame(scene, 0, stats_out))) return rc;
    if (rgb_f32_out) HIPCHECK(hipMemcpy(rgb_f32_out, scene->outF32.p, px * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return XRT_OK;
}

int xrt_render_begin(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                     uint32_t *rgba_out, int32_t *ticket_out) {
    int rc = need_device(scene, "xrt_render_begin");
    if (rc != XRT_OK) return rc;
    if (!camera || !opts || !rgba_out || !ticket_out) return fail(XRT_E_INVALID_ARG, "xrt_render_begin: null argument");
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "Current render operation not finished.");
    const int slot = !scene->frames[0].pending ? 0 : (!scene->frames[1].pending ? 1 : -1);
    if (slot < 0) return fail(XRT_E_BUSY, "two frames are already in flight; call xrt_render_end first");
    if ((rc = open_frame(scene, slot, camera, lights, n_lights, opts, nullptr, nullptr, rgba_out, nullptr))) return rc;
    *ticket_out = slot;
    return XRT_OK;
}

int xrt_render_end(xrt_scene *scene, int32_t ticket, xrt_stats *stats_out) { return xrt_render_device_end(scene, ticket, stats_out); }

int xrt_host_register(void *host_ptr, uint64_t bytes) {
    if (!host_ptr || bytes == 0) return fail(XRT_E_INVALID_ARG, "xrt_host_register: null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return fail(XRT_E_NO_DEVICE, "no HIP device visible"); }
    HIPCHECK(hipHostRegister(host_ptr, (size_t)bytes, hipHostRegisterDefault));
    return XRT_OK;
}

int xrt_host_unregister(void *host_ptr) {
    if (!host_ptr) return fail(XRT_E_INVALID_ARG, "xrt_host_unregister: null argument");
    HIPCHECK(hipHostUnregister(host_ptr));
    return XRT_OK;
}

int xrt_render_device(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                      void *d_rgba_out, void *stream, xrt_stats *stats_out) {
    int rc = need_device(scene, "xrt_render_device");
    if (rc != XRT_OK) return rc;
    if (!camera || !opts || !d_rgba_out) return fail(XRT_E_INVALID_ARG, "xrt_render_device: null argument");
    BusyGuard guard(scene);
    if (!guard.owned || scene->frames[0].pending || scene->frames[1].pending) return fail(XRT_E_BUSY, "Current render operation not finished.");
    if ((rc = open_frame(scene, 0, camera, lights, n_lights, opts, (uint32_t *)d_rgba_out, nullptr, nullptr, (hipStream_t)stream))) return rc;
    return close_frame(scene, 0, stats_out);
}

int xrt_render_device_begin(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                            void *d_rgba_out, void *stream, int32_t *ticket_out) {
    int rc = need_device(scene, "xrt_render_device_begin");
    if (rc != XRT_OK) return rc;
    if (!camera || !opts || !d_rgba_out || !ticket_out) return fail(XRT_E_INVALID_ARG, "xrt_render_device_begin: null argument");
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "Current render operation not finished.");
    const int slot = !scene->frames[0].pending ? 0 : (!scene->frames[1].pending ? 1 : -1);
    if (slot < 0) return fail(XRT_E_BUSY, "two frames are already in flight; call xrt_render_device_end first");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = open_frame(scene, slot, camera, lights, n_lights, opts, (uint32_t *)d_rgba_out, nullptr, nullptr, st))) return rc;
    *ticket_out = slot;
    return XRT_OK;
}

int xrt_render_device_end(xrt_scene *scene, int32_t ticket, xrt_stats *stats_out) {
    int rc = need_device(scene, "xrt_render_device_end");
    if (rc != XRT_OK) return rc;
    if (ticket < 0 || ticket > 1) return fail(XRT_E_INVALID_ARG, "xrt_render_device_end: unknown ticket");
    BusyGuard guard(scene);
    if (!guard.owned) return fail(XRT_E_BUSY, "Current render operation not finished.");
    if (!scene->frames[ticket].pending) return fail(XRT_E_INVALID_ARG, "no frame in flight for this ticket");
    return close_frame(scene, ticket, stats_out);
}

int xrt_shard_layout(int32_t width, int32_t height, int32_t shard_count, int32_t *tiles_x_out, int32_t *tiles_y_out, int32_t *tiles_per_rank_out) {
    if (width <= 0 || height <= 0 || shard_count <= 0) return fail(XRT_E_INVALID_ARG, "xrt_shard_layout: bad argument");
    int tx = (width + XRT_TILE_W - 1) / XRT_TILE_W, ty = (height + XRT_TILE_H - 1) / XRT_TILE_H;
    if (tiles_x_out) *tiles_x_out = tx;
    if (tiles_y_out) *tiles_y_out = ty;
    if (tiles_per_rank_out) *tiles_per_rank_out = (int)shard_tiles_per_rank((long long)tx * ty, shard_count, tx);
    return XRT_OK;
}

int xrt_detile_device(int32_t width, int32_t height, int32_t shard_count, const void *d_gathered, int64_t rank_stride, void *d_rgba_out,
                      void *stream) {
    if (width <= 0 || height <= 0 || shard_count <= 0 || !d_gathered || !d_rgba_out) return fail(XRT_E_INVALID_ARG, "xrt_detile_device: bad argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return fail(XRT_E_NO_DEVICE, "no HIP device visible"); }
    int tpr = 0;
    xrt_shard_layout(width, height, shard_count, nullptr, nullptr, &tpr);
    if (rank_stride < 0 || (rank_stride > 0 && rank_stride < (int64_t)tpr * 512)) return fail(XRT_E_INVALID_ARG, "xrt_detile_device: rank_stride smaller than a rank's tiles");
    launch_detile(width, height, shard_count, tpr, (const uint32_t *)d_gathered, rank_stride > 0 ? rank_stride : (long long)tpr * 512,
                  (uint32_t *)d_rgba_out, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return XRT_OK;
}

int xrt_scene_set_tile_table(xrt_scene *scene, int32_t width, int32_t height, int32_t shard_count, int32_t tiles_per_rank, const int32_t *tile_of_slot) {
    int rc = need_device(scene, "xrt_scene_set_tile_table");
    if (rc != XRT_OK) return rc;
    BusyGuard guard(scene);
    if (!guard.owned || scene->frames[0].pending || scene->frames[1].pending) return fail(XRT_E_BUSY, "Current render operation not finished.");
    return guarded("xrt_scene_set_tile_table", [&]() -> int {
        HIPCHECK(hipSetDevice(scene->device));
        if (!tile_of_slot) return install_tile_table(scene, 0, 0, 0, 0, nullptr);
        if (width <= 0 || height <= 0 || shard_count <= 0 || tiles_per_rank <= 0) return fail(XRT_E_INVALID_ARG, "xrt_scene_set_tile_table: bad argument");
        const int tiles = ((width + XRT_TILE_W - 1) / XRT_TILE_W) * ((height + XRT_TILE_H - 1) / XRT_TILE_H);
        int rc2 = check_tile_table(tiles, shard_count, tiles_per_rank, tile_of_slot);
        if (rc2 != XRT_OK) return rc2;
        return install_tile_table(scene, width, height, shard_count, tiles_per_rank, tile_of_slot);
    });
}

int xrt_scene_tile_costs(xrt_scene *scene, int32_t width, int32_t height, float *cost_out, int32_t reset) {
    int rc = need_device(scene, "xrt_scene_tile_costs");
    if (rc != XRT_OK) return rc;
    if (width <= 0 || height <= 0 || !cost_out) return fail(XRT_E_INVALID_ARG, "xrt_scene_tile_costs: bad argument");
    BusyGuard guard(scene);
    if (!guard.owned || scene->frames[0].pending || scene->frames[1].pending) return fail(XRT_E_BUSY, "Current render operation not finished.");
    const int tiles = ((width + XRT_TILE_W - 1) / XRT_TILE_W) * ((height + XRT_TILE_H - 1) / XRT_TILE_H);
    std::fill(cost_out, cost_out + tiles, 0.0f);
    HIPCHECK(hipSetDevice(scene->device));
    return guarded("xrt_scene_tile_costs", [&]() -> int { return read_tile_costs(scene, width, height, cost_out, reset != 0); });
}

int xrt_balance_tiles(int32_t width, int32_t height, int32_t shard_count, const float *tile_cost, int32_t tiles_per_rank, int32_t *tile_of_slot_out) {
    if (width <= 0 || height <= 0 || shard_count <= 0 || tiles_per_rank <= 0 || !tile_of_slot_out) return fail(XRT_E_INVALID_ARG, "xrt_balance_tiles: bad argument");
    const int tiles = ((width + XRT_TILE_W - 1) / XRT_TILE_W) * ((height + XRT_TILE_H - 1) / XRT_TILE_H);
    return guarded("xrt_balance_tiles", [&]() -> int { return balance_tiles_impl(tiles, shard_count, tile_cost, tiles_per_rank, tile_of_slot_out); });
}

int xrt_detile_table_device(int32_t width, int32_t height, int32_t shard_count, int32_t tiles_per_rank, const void *d_tile_of_slot, const void *d_gathered,
                            int64_t rank_stride, void *d_rgba_out, void *stream) {
    if (width <= 0 || height <= 0 || shard_count <= 0 || tiles_per_rank <= 0 || !d_tile_of_slot || !d_gathered || !d_rgba_out)
        return fail(XRT_E_INVALID_ARG, "xrt_detile_table_device: bad argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return fail(XRT_E_NO_DEVICE, "no HIP device visible"); }
    if (rank_stride < 0 || (rank_stride > 0 && rank_stride < (int64_t)tiles_per_rank * 512)) return fail(XRT_E_INVALID_ARG, "xrt_detile_table_device: rank_stride smaller than a rank's tiles");
    launch_detile(width, height, shard_count, tiles_per_rank, (const uint32_t *)d_gathered, rank_stride > 0 ? rank_stride : (long long)tiles_per_rank * 512,
                  (uint32_t *)d_rgba_out, (hipStream_t)stream, (const int *)d_tile_of_slot);
    HIPCHECK(hipGetLastError());
    return XRT_OK;
}

int xrt_rccl_probe(void) {
    return guarded("xrt_rccl_probe", [&]() -> int {
        RcclGather g;
        std::string err;
        if (!g.probe(err)) return fail(XRT_E_RCCL, "%s", err.c_str());
        return XRT_OK;
    });
}

float xrt_progress(const xrt_scene *scene) { return scene ? scene->progress.load() : 0.0f; }

int xrt_debug_end_counts(xrt_scene *scene, uint64_t out[3]) {
    return guarded("xrt_debug_end_counts", [&]() -> int {
        int rc = need_device(scene, "xrt_debug_end_counts");
        if (rc != XRT_OK) return rc;
        if (!out) return fail(XRT_E_INVALID_ARG, "xrt_debug_end_counts: null argument");
        for (int i = 0; i < 3; i++) out[i] = scene->endCounts[i];
        return XRT_OK;
    });
}

int xrt_debug_packet_table(xrt_scene *scene, uint64_t counts[2], uint32_t *entries_out, int64_t entries_cap, int32_t *paths_out, int64_t paths_cap) {
    return guarded("xrt_debug_packet_table", [&]() -> int {
        int rc = need_device(scene, "xrt_debug_packet_table");
        if (rc != XRT_OK) return rc;
        if (!counts || entries_cap < 0 || paths_cap < 0 || (!entries_out && entries_cap > 0) || (!paths_out && paths_cap > 0))
            return fail(XRT_E_INVALID_ARG, "xrt_debug_packet_table: null argument or negative capacity");
        BusyGuard guard(scene);
        if (!guard.owned || scene->frames[0].pending || scene->frames[1].pending) return fail(XRT_E_BUSY, "Current render operation not finished.");
        counts[0] = counts[1] = 0;
        if (scene->quadCtx < 0) return XRT_OK;
        const xrt_scene::WorkBufs &W = scene->frames[scene->quadCtx].w;
        const FramePlan &P = scene->frames[scene->quadCtx].plan;
        HIPCHECK(hipSetDevice(scene->device));
        HIPCHECK(hipDeviceSynchronize());
        unsigned n = 0;
        HIPCHECK(hipMemcpy(&n, W.quadTable.p + 64 * W.quadWord, sizeof(n), hipMemcpyDeviceToHost));
        if ((size_t)n > P.pkEntries) return fail(XRT_E_INTERNAL, "xrt_debug_packet_table: %u entries in a table sized for %zu", n, P.pkEntries);
        counts[0] = n; counts[1] = scene->quadLive;
        const size_t ne = std::min<size_t>(n, (size_t)entries_cap), np = std::min<size_t>((size_t)scene->quadLive, (size_t)paths_cap);
        if (ne) HIPCHECK(hipMemcpy(entries_out, W.quadTable.p + QUAD_HEAD_WORDS, ne * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (np) HIPCHECK(hipMemcpy(paths_out, W.index0.p, np * sizeof(int32_t), hipMemcpyDeviceToHost));
        return XRT_OK;
    });
}

int xrt_debug_screen_table(xrt_scene *scene, int32_t host_eval, uint64_t *count, uint32_t *entries_out, int64_t entries_cap) {
    return guarded("xrt_debug_screen_table", [&]() -> int {
        int rc = need_device(scene, "xrt_debug_screen_table");
        if (rc != XRT_OK) return rc;
        if (!count || entries_cap < 0 || (!entries_out && entries_cap > 0)) return fail(XRT_E_INVALID_ARG, "xrt_debug_screen_table: null argument or negative capacity");
        BusyGuard guard(scene);
        if (!guard.owned || scene->frames[0].pending || scene->frames[1].pending) return fail(XRT_E_BUSY, "Current render operation not finished.");
        *count = 0;
        if (scene->quadCtx < 0) return XRT_OK;
        const xrt_scene::WorkBufs &W = scene->frames[scene->quadCtx].w;
        const FramePlan &P = scene->frames[scene->quadCtx].plan;
        if (!P.scrRefs || P.batch || !W.scrTable.p) return XRT_OK;
        HIPCHECK(hipSetDevice(scene->device));
        HIPCHECK(hipDeviceSynchronize());
        *count = P.scrRefs;
        const size_t ne = std::min<size_t>(P.scrRefs, (size_t)entries_cap);
        if (host_eval) {   // the same functions in the host's build, on the host's copy of the records and of the body's pose
            if (scene->posesOnDevice || scene->host->arrays.objects.empty()) return fail(XRT_E_UNSUPPORTED, "xrt_debug_screen_table: the host does not hold the body's pose");
            ScreenXf X;
            make_screen_xf(P.g, scene->host->arrays.objects[0].invWorld, X);
            const float *refT = scene->host->arrays.refT.data();
            for (size_t r = 0; r < ne; r++) {
                const float *q = refT + r * TRI_REC_WORDS;
                const ScrEntry e = screen_entry(X, q + 4, q + 7, q + 10);
                entries_out[2 * r] = e.x; entries_out[2 * r + 1] = e.y;
            }
            return XRT_OK;
        }
        if (ne) HIPCHECK(hipMemcpy(entries_out, W.scrTable.p, ne * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return XRT_OK;
    });
}

int xrt_split_stats(xrt_scene *scene, uint64_t out[4], int32_t reset) {
    return guarded("xrt_split_stats", [&]() -> int {
        int rc = need_device(scene, "xrt_split_stats");
        if (rc != XRT_OK) return rc;
        if (!out) return fail(XRT_E_INVALID_ARG, "xrt_split_stats: null argument");
        unsigned long long v[4] = {0, 0, 0, 0};
        HIPCHECK(hipSetDevice(scene->device));
        HIPCHECK(hipDeviceSynchronize());
        if (packet_split_stats(v, reset != 0) != 0) return fail(XRT_E_HIP, "xrt_split_stats: %s", hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < 4; i++) out[i] = v[i];
        return XRT_OK;
    });
}

// ---- the list calls (xrt_cast_rays, xrt_shade_hits, xrt_light_hits, xrt_surface_hits, xrt_cast_rays_paths, xrt_render_pixels, xrt_trace_pixels) -------------
// Every host form reads: its checks, hold the scene, stage, the *_impl its _device form calls, finish.  What the forms share is below; what differs between the
// families -- which checks come before the device is asked for, which messages carry the function name, what n == 0 does -- is what is left in them
// (tests/list_calls/host_list_calls.cpp records all of it).
}  // extern "C"

namespace {

// An entry point: no exception leaves it, and a null scene is said before anything else, by every one of them.
template <class F>
int list_call(const char *fn, const xrt_scene *scene, F &&body) {
    return guarded(fn, [&]() -> int { return scene ? body(fn) : fail(XRT_E_INVALID_ARG, "%s: null scene", fn); });
}

// The arguments are in order: the stats start at zero, and a list without entries is done.
bool empty_list(int64_t n, xrt_stats *stats) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return n == 0;
}

// A hit names a triangle of a mesh of the scene -- withBody: and a body of the scene that holds that mesh --, as the query would have (the lists as they were
// added: known on a host-only scene too).  A miss names nothing.
int hits_name_scene(const char *fn, const xrt_scene *scene, const xrt_hit *hits, int64_t n, bool withBody) {
    const auto &meshes = scene->host->meshes; const auto &bodies = scene->host->objects;
    for (int64_t i = 0; i < n; i++) {
        const xrt_hit &h = hits[i];
        if (h.hit == 0) continue;
        if (h.mesh < 0 || h.mesh >= (int)meshes.size()) return fail(XRT_E_INVALID_ARG, "%s: hit %lld names mesh %d, which does not exist", fn, (long long)i, h.mesh);
        if (h.tri < 0 || h.tri >= meshes[(size_t)h.mesh].ntri)
            return fail(XRT_E_INVALID_ARG, "%s: hit %lld names triangle %d of mesh %d, which does not exist", fn, (long long)i, h.tri, h.mesh);
        if (!withBody) continue;
        if (h.object < 0 || h.object >= (int)bodies.size()) return fail(XRT_E_INVALID_ARG, "%s: hit %lld names body %d, which does not exist", fn, (long long)i, h.object);
        const std::vector<int> &bm = bodies[(size_t)h.object].meshes;
        if (std::find(bm.begin(), bm.end(), h.mesh) == bm.end())
            return fail(XRT_E_INVALID_ARG, "%s: hit %lld names mesh %d, which is not a mesh of body %d", fn, (long long)i, h.mesh, h.object);
    }
    return XRT_OK;
}

// A ray's origin is (mesh id, index in Mesh.Triangles[]) of a triangle of the scene, or null (ignore_tri < 0).
int rays_name_scene(const char *fn, const xrt_scene *scene, const xrt_ray *rays, int64_t n) {
    const auto &meshes = scene->host->arrays.meshes;
    for (int64_t i = 0; i < n; i++) {
        const xrt_ray &r = rays[i];
        if (r.ignore_tri < 0) continue;
        if (r.ignore_mesh < 0 || r.ignore_mesh >= (int)meshes.size() || r.ignore_tri >= meshes[(size_t)r.ignore_mesh].ntri)
            return fail(XRT_E_INVALID_ARG, "%s: ray %lld names triangle %d of mesh %d, which does not exist", fn, (long long)i, r.ignore_tri, r.ignore_mesh);
    }
    return XRT_OK;
}

int centres_finite(const char *fn, const float *centers, int64_t n) {
    for (int64_t i = 0; i < 2 * n; i++)
        if (!std::isfinite(centers[i])) return fail(XRT_E_INVALID_ARG, "%s: centre %lld is not finite", fn, (long long)(i / 2));
    return XRT_OK;
}

int aligned16(std::initializer_list<const void *> pointers) {
    for (const void *p : pointers)
        if ((uintptr_t)p & 15) return fail(XRT_E_INVALID_ARG, "device buffers must be 16-byte aligned");
    return XRT_OK;
}

// The count and the pointers of a ray batch: `always` must not be null, `lists` must not be when there is an entry.
int batch_check_args(const char *fn, int64_t n, std::initializer_list<const void *> always, std::initializer_list<const void *> lists, const xrt_light *lights,
                     int32_t n_lights) {
    if (n < 0 || n > 0x7fffffff / 2) return fail(XRT_E_INVALID_ARG, "%s: n = %lld out of range", fn, (long long)n);
    bool missing = (!lights && n_lights > 0) || n_lights < 0;
    for (const void *p : always) missing |= !p;
    for (const void *p : lists) missing |= n > 0 && !p;
    return missing ? fail(XRT_E_INVALID_ARG, "%s: null argument", fn) : XRT_OK;
}

// The scene for the length of a list call: refused while another call or a frame has it.  The call's stream is the caller's, or the scene's.
struct SceneHold {
    BusyGuard guard;
    hipStream_t st;
    explicit SceneHold(xrt_scene *scene, void *stream = nullptr) : guard(scene), st(stream ? (hipStream_t)stream : scene->stream) {}
    int refused() const {
        const bool busy = !guard.owned || guard.s->frames[0].pending || guard.s->frames[1].pending;
        return busy ? fail(XRT_E_BUSY, "Current render operation not finished.") : XRT_OK;   // RT:62-63
    }
    int begin(const char *fn) const { int rc = need_device(guard.s, fn); return rc ? rc : refused(); }   // (the forms that ask for the device last)
};

// A host form's arrays on their way through the scene's buffers.  in: room for `count` elements and the upload enqueued; out: room, and the download remembered;
// both hand back the device array, or null for an array the caller did not give (nothing is done for it).  finish: the downloads, ONE synchronisation, the guards.
// The first thing that fails is kept in `rc` and makes everything after it a no-op.
struct Staging {
    hipStream_t st;
    int rc = XRT_OK;
    bool any = false;
    struct Down { void *host; const void *dev; size_t bytes; };
    std::vector<Down> downs;
    explicit Staging(hipStream_t stream) : st(stream) {}
    int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) { HIPCHECK(hipMemcpyAsync(dst, src, bytes, kind, st)); return XRT_OK; }
    void down(void *host, const void *dev, size_t bytes) { any = true; if (bytes) downs.push_back({host, dev, bytes}); }
    template <class T> T *in(DevBuf<T> &buf, const void *host, size_t count) {
        if (!host || rc) return nullptr;
        any = true;
        if ((rc = buf.ensure(count)) == XRT_OK && count) rc = copy(buf.p, host, count * sizeof(T), hipMemcpyHostToDevice);
        return rc ? nullptr : buf.p;
    }
    template <class T> T *out(DevBuf<T> &buf, void *host, size_t count) {
        if (!host || rc || (rc = buf.ensure(count))) return nullptr;
        down(host, buf.p, count * sizeof(T));
        return buf.p;
    }
    int finish(const char *label) {
        if (rc) return rc;
        for (const Down &d : downs)
            if ((rc = copy(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost))) return rc;
        if (any) HIPCHECK(hipStreamSynchronize(st));
        return guards_check(label);
    }
};

}  // namespace

extern "C" {

int xrt_cast_rays(xrt_scene *scene, const xrt_ray *rays, int64_t n, int32_t iteration, float current_ref_index, const xrt_light *lights, int32_t n_lights,
                  const xrt_render_opts *opts, uint32_t *rgba_out, float *rgb_f32_out, xrt_stats *stats_out) {
    return list_call("xrt_cast_rays", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = need_device(scene, fn))) return rc;   // (this family asks for the device first)
        if ((rc = batch_check_args(fn, n, {opts}, {rays, rgba_out}, lights, n_lights)) || (rc = rays_name_scene(fn, scene, rays, n))) return rc;
        SceneHold hold(scene);
        if ((rc = hold.refused())) return rc;
        Staging S(hold.st);
        const xrt_ray *d_rays = nullptr; uint32_t *d_rgba = nullptr; float *d_f32 = nullptr;
        if (n > 0) { d_rays = S.in(scene->castRays, rays, (size_t)n); d_rgba = S.out(scene->castRGBA, rgba_out, (size_t)n); d_f32 = S.out(scene->castF32, rgb_f32_out, (size_t)n * 3); }
        if ((rc = S.rc) || (rc = cast_rays_impl(scene, d_rays, n, iteration, current_ref_index, lights, n_lights, opts, d_rgba, d_f32, hold.st, stats_out))) return rc;   // (n == 0 too: its opts are checked)
        return S.finish("end of a ray batch");
    });
}

int xrt_cast_rays_device(xrt_scene *scene, const void *d_rays, int64_t n, int32_t iteration, float current_ref_index, const xrt_light *lights,
                         int32_t n_lights, const xrt_render_opts *opts, void *d_rgba_out, void *d_rgb_f32_out, void *stream, xrt_stats *stats_out) {
    return list_call("xrt_cast_rays_device", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = need_device(scene, fn))) return rc;
        if ((rc = batch_check_args(fn, n, {opts}, {d_rays, d_rgba_out}, lights, n_lights)) || (rc = aligned16({d_rays, d_rgba_out, d_rgb_f32_out}))) return rc;
        SceneHold hold(scene, stream);
        if ((rc = hold.refused()) || (rc = cast_rays_impl(scene, (const xrt_ray *)d_rays, n, iteration, current_ref_index, lights, n_lights, opts, (uint32_t *)d_rgba_out,
                                                          (float *)d_rgb_f32_out, hold.st, stats_out)))
            return rc;
        return guards_check("end of a ray batch");
    });
}

// What is wrong with the arguments of xrt_shade_hits[_device] alone, in the order the header gives (the scene is not looked at).
static int shade_hits_check_args(const char *fn, const void *rays, const void *hits, int64_t n, int32_t iteration, const xrt_light *lights,
                                 int32_t n_lights, const xrt_render_opts *opts, const void *rgba_out) {
    if (int rc = batch_check_args(fn, n, {opts}, {rays, hits, rgba_out}, lights, n_lights)) return rc;
    return batch_check_opts(fn, opts, iteration);
}

int xrt_shade_hits(xrt_scene *scene, const xrt_ray *rays, const xrt_hit *hits, int64_t n, int32_t iteration, float current_ref_index, const xrt_light *lights,
                   int32_t n_lights, const xrt_render_opts *opts, uint32_t *rgba_out, float *rgb_f32_out, xrt_stats *stats_out) {
    return list_call("xrt_shade_hits", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = shade_hits_check_args(fn, rays, hits, n, iteration, lights, n_lights, opts, rgba_out)) || (rc = hits_name_scene(fn, scene, hits, n, true))) return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        if ((rc = lights_known(nullptr, lights, n_lights))) return rc;   // (its lights, once there is something to shade)
        SceneHold hold(scene);
        if ((rc = hold.begin(fn))) return rc;   // (what is wrong with the arguments alone is said first, also on a host-only scene)
        Staging S(hold.st);
        const xrt_ray *d_rays = S.in(scene->castRays, rays, (size_t)n); const xrt_hit *d_hits = S.in(scene->castHits, hits, (size_t)n);
        uint32_t *d_rgba = S.out(scene->castRGBA, rgba_out, (size_t)n); float *d_f32 = S.out(scene->castF32, rgb_f32_out, (size_t)n * 3);
        if ((rc = S.rc) || (rc = cast_rays_impl(scene, d_rays, n, iteration, current_ref_index, lights, n_lights, opts, d_rgba, d_f32, hold.st, stats_out, nullptr, d_hits, fn))) return rc;
        return S.finish("end of a batch of hits");
    });
}

int xrt_shade_hits_device(xrt_scene *scene, const void *d_rays, const void *d_hits, int64_t n, int32_t iteration, float current_ref_index, const xrt_light *lights,
                          int32_t n_lights, const xrt_render_opts *opts, void *d_rgba_out, void *d_rgb_f32_out, void *stream, xrt_stats *stats_out) {
    return list_call("xrt_shade_hits_device", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = shade_hits_check_args(fn, d_rays, d_hits, n, iteration, lights, n_lights, opts, d_rgba_out)) ||
            (rc = aligned16({d_rays, d_hits, d_rgba_out, d_rgb_f32_out})))
            return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        if ((rc = lights_known(nullptr, lights, n_lights))) return rc;   // (its lights, once there is something to shade)
        SceneHold hold(scene, stream);
        if ((rc = hold.begin(fn)) || (rc = cast_rays_impl(scene, (const xrt_ray *)d_rays, n, iteration, current_ref_index, lights, n_lights, opts, (uint32_t *)d_rgba_out,
                                                          (float *)d_rgb_f32_out, hold.st, stats_out, nullptr, (const xrt_hit *)d_hits, fn)))
            return rc;
        return guards_check("end of a batch of hits");
    });
}

// What is wrong with the arguments of xrt_light_hits[_device] alone, in the order the header gives (the scene is not looked at).
static int light_hits_check_args(const char *fn, const void *hits, int64_t n, const xrt_light *lights, int32_t n_lights,
                                 const void *light_out, const void *amount_out) {
    if (n < 0) return fail(XRT_E_INVALID_ARG, "%s: n = %lld out of range", fn, (long long)n);
    if (n_lights < 0) return fail(XRT_E_INVALID_ARG, "%s: n_lights = %d out of range", fn, n_lights);
    if (!lights && n_lights > 0) return fail(XRT_E_INVALID_ARG, "%s: null lights", fn);
    if (n > 0 && !light_out && !amount_out) return fail(XRT_E_INVALID_ARG, "%s: both outputs are null", fn);
    if (n > 0 && !hits) return fail(XRT_E_INVALID_ARG, "%s: null hits", fn);
    return lights_known(fn, lights, n_lights);
}

int xrt_light_hits(xrt_scene *scene, const xrt_hit *hits, int64_t n, const xrt_light *lights, int32_t n_lights, float *light_f32_out, float *amount_out,
                   xrt_stats *stats_out) {
    return list_call("xrt_light_hits", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = light_hits_check_args(fn, hits, n, lights, n_lights, light_f32_out, amount_out)) || (rc = hits_name_scene(fn, scene, hits, n, false))) return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene);
        if ((rc = hold.begin(fn))) return rc;   // (what is wrong with the arguments alone is said first, also on a host-only scene)
        xrt_scene::LightWork &W = scene->lightWork;
        Staging S(hold.st);
        const xrt_hit *d_hits = S.in(scene->castHits, hits, (size_t)n);
        float *d_light = S.out(W.lightOut, light_f32_out, (size_t)n * 3), *d_amount = S.out(W.amountOut, amount_out, (size_t)n * (size_t)n_lights);   // (no light: no element)
        if ((rc = S.rc) || (rc = light_hits_impl(scene, d_hits, n, lights, n_lights, d_light, d_amount, hold.st, stats_out))) return rc;
        return S.finish("end of a batch of lit hits");
    });
}

int xrt_light_hits_device(xrt_scene *scene, const void *d_hits, int64_t n, const xrt_light *lights, int32_t n_lights, void *d_light_f32_out, void *d_amount_out,
                          void *stream, xrt_stats *stats_out) {
    return list_call("xrt_light_hits_device", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = light_hits_check_args(fn, d_hits, n, lights, n_lights, d_light_f32_out, d_amount_out)) || (rc = aligned16({d_hits, d_light_f32_out, d_amount_out})))
            return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene, stream);
        if ((rc = hold.begin(fn)) || (rc = light_hits_impl(scene, (const xrt_hit *)d_hits, n, lights, n_lights, (float *)d_light_f32_out, (float *)d_amount_out, hold.st, stats_out))) return rc;
        return guards_check("end of a batch of lit hits");
    });
}

// What is wrong with the arguments of xrt_surface_hits[_device] alone, in the order the header gives (the scene is not looked at).
static int surface_hits_check_args(const char *fn, const void *rays, const void *hits, int64_t n, const xrt_render_opts *opts,
                                   const void *surface_out, const void *reflect_out, const void *refract_out) {
    if (!opts) return fail(XRT_E_INVALID_ARG, "%s: null opts", fn);
    if (n < 0) return fail(XRT_E_INVALID_ARG, "%s: n = %lld out of range", fn, (long long)n);
    if (n > 0 && !surface_out && !reflect_out && !refract_out) return fail(XRT_E_INVALID_ARG, "%s: all outputs are null", fn);
    if (n > 0 && !hits) return fail(XRT_E_INVALID_ARG, "%s: null hits", fn);
    if (n > 0 && !rays && (reflect_out || refract_out)) return fail(XRT_E_INVALID_ARG, "%s: null rays with a ray output", fn);
    return XRT_OK;
}

int xrt_surface_hits(xrt_scene *scene, const xrt_ray *rays, const xrt_hit *hits, int64_t n, float current_ref_index, const xrt_render_opts *opts,
                     xrt_surface *surface_out, xrt_ray *reflect_out, xrt_ray *refract_out, xrt_stats *stats_out) {
    return list_call("xrt_surface_hits", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = surface_hits_check_args(fn, rays, hits, n, opts, surface_out, reflect_out, refract_out)) || (rc = hits_name_scene(fn, scene, hits, n, false))) return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene);
        if ((rc = hold.begin(fn))) return rc;   // (what is wrong with the arguments alone is said first, also on a host-only scene)
        xrt_scene::SurfaceWork &W = scene->surfaceWork;
        Staging S(hold.st);
        const xrt_hit *d_hits = S.in(scene->castHits, hits, (size_t)n);
        const xrt_ray *d_rays = S.in(scene->castRays, (reflect_out || refract_out) ? rays : nullptr, (size_t)n);   // (the rays are read for a ray output alone)
        xrt_surface *d_surface = S.out(W.surfaceOut, surface_out, (size_t)n);
        xrt_ray *d_reflect = S.out(W.reflectOut, reflect_out, (size_t)n), *d_refract = S.out(W.refractOut, refract_out, (size_t)n);
        if ((rc = S.rc) || (rc = surface_hits_impl(scene, d_rays, d_hits, n, current_ref_index, opts, d_surface, d_reflect, d_refract, hold.st, stats_out))) return rc;
        return S.finish("end of a batch of surface records");
    });
}

int xrt_surface_hits_device(xrt_scene *scene, const void *d_rays, const void *d_hits, int64_t n, float current_ref_index, const xrt_render_opts *opts,
                            void *d_surface_out, void *d_reflect_out, void *d_refract_out, void *stream, xrt_stats *stats_out) {
    return list_call("xrt_surface_hits_device", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = surface_hits_check_args(fn, d_rays, d_hits, n, opts, d_surface_out, d_reflect_out, d_refract_out)) ||
            (rc = aligned16({d_rays, d_hits, d_surface_out, d_reflect_out, d_refract_out})))
            return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene, stream);
        const bool wantRays = d_reflect_out || d_refract_out;
        if ((rc = hold.begin(fn)) || (rc = surface_hits_impl(scene, wantRays ? (const xrt_ray *)d_rays : nullptr, (const xrt_hit *)d_hits, n, current_ref_index, opts,
                                                             (xrt_surface *)d_surface_out, (xrt_ray *)d_reflect_out, (xrt_ray *)d_refract_out, hold.st, stats_out)))
            return rc;
        return guards_check("end of a batch of surface records");
    });
}

// What is wrong with the arguments of xrt_compose_hits[_device] alone, in the order the header gives (the scene is not looked at).
static int compose_hits_check_args(const char *fn, const void *surface, const void *light, const void *reflect, const void *refract, int64_t n,
                                   const void *rgba_out, const void *rgb_f32_out) {
    if (n < 0) return fail(XRT_E_INVALID_ARG, "%s: n = %lld out of range", fn, (long long)n);
    if (n > 0 && !rgba_out && !rgb_f32_out) return fail(XRT_E_INVALID_ARG, "%s: both outputs are null", fn);
    if (n > 0 && !surface) return fail(XRT_E_INVALID_ARG, "%s: null surface", fn);
    if (n > 0 && !light) return fail(XRT_E_INVALID_ARG, "%s: null light", fn);
    if (refract && !reflect) return fail(XRT_E_INVALID_ARG, "%s: refract_rgba without reflect_rgba", fn);
    return XRT_OK;
}

int xrt_compose_hits(xrt_scene *scene, const xrt_surface *surface, const float *light_f32, const uint32_t *reflect_rgba, const uint32_t *refract_rgba, int64_t n,
                     uint32_t *rgba_out, float *rgb_f32_out, xrt_stats *stats_out) {
    return list_call("xrt_compose_hits", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = compose_hits_check_args(fn, surface, light_f32, reflect_rgba, refract_rgba, n, rgba_out, rgb_f32_out))) return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene);
        if ((rc = hold.begin(fn))) return rc;   // (what is wrong with the arguments alone is said first, also on a host-only scene)
        xrt_scene::ComposeWork &W = scene->composeWork;
        Staging S(hold.st);
        const xrt_surface *d_surface = S.in(W.surfaceIn, surface, (size_t)n);
        const float *d_light = S.in(W.lightIn, light_f32, (size_t)n * 3);
        const uint32_t *d_reflect = S.in(W.reflectIn, reflect_rgba, (size_t)n), *d_refract = S.in(W.refractIn, refract_rgba, (size_t)n);
        uint32_t *d_rgba = S.out(W.rgbaOut, rgba_out, (size_t)n);
        float *d_f32 = S.out(W.f32Out, rgb_f32_out, (size_t)n * 3);
        if ((rc = S.rc) || (rc = compose_hits_impl(scene, d_surface, d_light, d_reflect, d_refract, n, d_rgba, d_f32, hold.st, stats_out))) return rc;
        return S.finish("end of a batch of composed hits");
    });
}

int xrt_compose_hits_device(xrt_scene *scene, const void *d_surface, const void *d_light_f32, const void *d_reflect_rgba, const void *d_refract_rgba, int64_t n,
                            void *d_rgba_out, void *d_rgb_f32_out, void *stream, xrt_stats *stats_out) {
    return list_call("xrt_compose_hits_device", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = compose_hits_check_args(fn, d_surface, d_light_f32, d_reflect_rgba, d_refract_rgba, n, d_rgba_out, d_rgb_f32_out)) ||
            (rc = aligned16({d_surface, d_light_f32, d_reflect_rgba, d_refract_rgba, d_rgba_out, d_rgb_f32_out})))
            return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene, stream);
        if ((rc = hold.begin(fn)) || (rc = compose_hits_impl(scene, (const xrt_surface *)d_surface, (const float *)d_light_f32, (const uint32_t *)d_reflect_rgba,
                                                             (const uint32_t *)d_refract_rgba, n, (uint32_t *)d_rgba_out, (float *)d_rgb_f32_out, hold.st, stats_out)))
            return rc;
        return guards_check("end of a batch of composed hits");
    });
}

// What is wrong with the arguments of xrt_fold_samples[_device] alone, in the order the header gives (the scene is not looked at).
static int fold_samples_check_args(const char *fn, const void *rgba_in, int64_t n, int32_t samples, const void *rgba_out) {
    if (n < 0) return fail(XRT_E_INVALID_ARG, "%s: n = %lld out of range", fn, (long long)n);
    if (samples != 4 && samples != 16) return fail(XRT_E_INVALID_ARG, "%s: samples = %d is neither 4 nor 16", fn, samples);
    if (n > 0 && !rgba_out) return fail(XRT_E_INVALID_ARG, "%s: null rgba_out", fn);
    if (n > 0 && !rgba_in) return fail(XRT_E_INVALID_ARG, "%s: null rgba_in", fn);
    return XRT_OK;
}

int xrt_fold_samples(xrt_scene *scene, const uint32_t *rgba_in, int64_t n, int32_t samples, uint32_t *rgba_out, float *rgb_f32_out, xrt_stats *stats_out) {
    return list_call("xrt_fold_samples", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = fold_samples_check_args(fn, rgba_in, n, samples, rgba_out))) return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene);
        if ((rc = hold.begin(fn))) return rc;
        xrt_scene::ComposeWork &W = scene->composeWork;
        Staging S(hold.st);
        const uint32_t *d_in = S.in(W.samplesIn, rgba_in, (size_t)n * (size_t)samples);
        uint32_t *d_rgba = S.out(W.rgbaOut, rgba_out, (size_t)n);
        float *d_f32 = S.out(W.f32Out, rgb_f32_out, (size_t)n * 3);
        if ((rc = S.rc) || (rc = fold_samples_impl(scene, d_in, n, samples, d_rgba, d_f32, hold.st, stats_out))) return rc;
        return S.finish("end of a batch of folded samples");
    });
}

int xrt_fold_samples_device(xrt_scene *scene, const void *d_rgba_in, int64_t n, int32_t samples, void *d_rgba_out, void *d_rgb_f32_out, void *stream,
                            xrt_stats *stats_out) {
    return list_call("xrt_fold_samples_device", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = fold_samples_check_args(fn, d_rgba_in, n, samples, d_rgba_out)) || (rc = aligned16({d_rgba_in, d_rgba_out, d_rgb_f32_out}))) return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene, stream);
        if ((rc = hold.begin(fn)) || (rc = fold_samples_impl(scene, (const uint32_t *)d_rgba_in, n, samples, (uint32_t *)d_rgba_out, (float *)d_rgb_f32_out, hold.st, stats_out)))
            return rc;
        return guards_check("end of a batch of folded samples");
    });
}

// Most vertices a batch of n rays can need (paths.h path_vertex_bound), or -1 where cast_rays_impl refuses the depth anyway.
static long long paths_bound(const xrt_scene *scene, const xrt_render_opts *opts, int32_t iteration, int64_t n) {
    const long long depth = std::max(0LL, (long long)opts->max_reflections - (long long)iteration);
    const bool tree = scene->mat[scene->matCur].anyTransparent && depth > 0;
    if (opts->max_reflections < 0 || depth > 64 || (tree && depth > PATH_TREE_DEPTH)) return -1;
    return path_vertex_bound((int)depth, tree) * (long long)n;
}

// What is wrong with the arguments of xrt_cast_rays_paths[_device] alone; then the scene's device is asked for (before the entries and the alignment are looked at).
static int paths_check_args(const char *fn, xrt_scene *scene, const void *rays, int64_t n, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                            const void *rgba_out, const void *vertices, int64_t vertex_capacity, const int64_t *n_vertices_out) {
    if (int rc = batch_check_args(fn, n, {opts, n_vertices_out}, {rays, rgba_out}, lights, n_lights)) return rc;
    if (vertex_capacity < 0 || (vertex_capacity > 0 && !vertices))
        return fail(XRT_E_INVALID_ARG, "%s: vertex_capacity = %lld with%s vertices", fn, (long long)vertex_capacity, vertices ? "" : " null");
    return need_device(scene, fn);
}

int xrt_cast_rays_paths(xrt_scene *scene, const xrt_ray *rays, int64_t n, int32_t iteration, float current_ref_index, const xrt_light *lights, int32_t n_lights,
                        const xrt_render_opts *opts, uint32_t *rgba_out, float *rgb_f32_out, xrt_ray *rays_back, int64_t *vertex_start, xrt_path_vertex *vertices,
                        int64_t vertex_capacity, int64_t *n_vertices_out, xrt_stats *stats_out) {
    return list_call("xrt_cast_rays_paths", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = paths_check_args(fn, scene, rays, n, lights, n_lights, opts, rgba_out, vertices, vertex_capacity, n_vertices_out)) ||
            (rc = rays_name_scene(fn, scene, rays, n)))
            return rc;
        SceneHold hold(scene);
        if ((rc = hold.refused())) return rc;
        Staging S(hold.st);
        BatchSrc::Paths P;
        const xrt_ray *d_rays = nullptr; uint32_t *d_rgba = nullptr; float *d_f32 = nullptr;
        if (n > 0) {
            // the device never needs more room than the deepest recursion of every ray could fill, whatever capacity the caller names
            P.capacity = vertices ? std::min<long long>(vertex_capacity, std::max(0LL, paths_bound(scene, opts, iteration, n))) : 0;
            d_rays = S.in(scene->castRays, rays, (size_t)n); d_rgba = S.out(scene->castRGBA, rgba_out, (size_t)n); d_f32 = S.out(scene->castF32, rgb_f32_out, (size_t)n * 3);
            P.raysBack = S.out(scene->pathBack, rays_back, (size_t)n);
            if (S.rc) return S.rc;
            // the ordering pass needs the running offsets whether or not the caller wants them; how many vertices come back is known after the pass
            if ((rc = scene->pathStart.ensure((size_t)n + 1)) || (P.capacity > 0 && (rc = scene->pathVerts.ensure((size_t)P.capacity)))) return rc;
            P.vertexStart = scene->pathStart.p; P.vertices = P.capacity > 0 ? scene->pathVerts.p : nullptr;
            if (vertex_start) S.down(vertex_start, scene->pathStart.p, ((size_t)n + 1) * sizeof(int64_t));
        }
        if ((rc = cast_rays_impl(scene, d_rays, n, iteration, current_ref_index, lights, n_lights, opts, d_rgba, d_f32, hold.st, stats_out, &P))) return rc;
        *n_vertices_out = 0;
        if (n == 0 && vertex_start) vertex_start[0] = 0;
        if (n > 0) {
            const long long need = *scene->pathPinned.p;   // (arrived with the pass: cast_rays_impl waited for it)
            *n_vertices_out = need;
            const long long wrote = std::min(need, P.capacity & ~1LL);
            if (wrote > 0) S.down(vertices, scene->pathVerts.p, (size_t)wrote * sizeof(xrt_path_vertex));
        }
        return S.finish("end of a ray batch");
    });
}

int xrt_cast_rays_paths_device(xrt_scene *scene, const void *d_rays, int64_t n, int32_t iteration, float current_ref_index, const xrt_light *lights,
                               int32_t n_lights, const xrt_render_opts *opts, void *d_rgba_out, void *d_rgb_f32_out, void *d_rays_back, void *d_vertex_start,
                               void *d_vertices, int64_t vertex_capacity, void *stream, int64_t *n_vertices_out, xrt_stats *stats_out) {
    return list_call("xrt_cast_rays_paths_device", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = paths_check_args(fn, scene, d_rays, n, lights, n_lights, opts, d_rgba_out, d_vertices, vertex_capacity, n_vertices_out)) ||
            (rc = aligned16({d_rays, d_rgba_out, d_rgb_f32_out, d_rays_back, d_vertex_start, d_vertices})))
            return rc;
        if (d_rays_back && d_rays_back == d_rays) return fail(XRT_E_INVALID_ARG, "%s: d_rays_back must not be d_rays (a chunk that is redone reads its rays again)", fn);
        SceneHold hold(scene, stream);
        if ((rc = hold.refused())) return rc;
        BatchSrc::Paths P;
        P.vertices = vertex_capacity > 0 ? (xrt_path_vertex *)d_vertices : nullptr; P.capacity = vertex_capacity; P.vertexStart = (long long *)d_vertex_start; P.raysBack = (xrt_ray *)d_rays_back;
        if (n > 0 && !P.vertexStart) {   // the ordering pass needs the running offsets whether or not the caller wants them
            if ((rc = scene->pathStart.ensure((size_t)n + 1))) return rc;
            P.vertexStart = scene->pathStart.p;
        }
        if ((rc = cast_rays_impl(scene, (const xrt_ray *)d_rays, n, iteration, current_ref_index, lights, n_lights, opts, (uint32_t *)d_rgba_out, (float *)d_rgb_f32_out,
                                 hold.st, stats_out, &P)))
            return rc;
        *n_vertices_out = n > 0 ? *scene->pathPinned.p : 0;
        if (n == 0 && d_vertex_start) {
            HIPCHECK(hipMemsetAsync(d_vertex_start, 0, sizeof(int64_t), hold.st));
            HIPCHECK(hipStreamSynchronize(hold.st));
        }
        return guards_check("end of a ray batch");
    });
}

int xrt_render_pixels(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts, const float *centers,
                      int64_t n, uint32_t *rgba_out, float *rgb_f32_out, xrt_stats *stats_out) {
    return list_call("xrt_render_pixels", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = pixels_check_args(fn, camera, lights, n_lights, opts, n, centers, rgba_out)) || (rc = centres_finite(fn, centers, n))) return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene);
        if ((rc = hold.begin(fn))) return rc;   // (what is wrong with the arguments alone is said first, also on a host-only scene)
        Staging S(hold.st);
        const float *d_centers = S.in(scene->pixelCenters, centers, (size_t)n * 2);
        uint32_t *d_rgba = S.out(scene->castRGBA, rgba_out, (size_t)n); float *d_f32 = S.out(scene->castF32, rgb_f32_out, (size_t)n * 3);
        if ((rc = S.rc) || (rc = render_pixels_impl(scene, camera, lights, n_lights, opts, d_centers, n, d_rgba, d_f32, hold.st, stats_out))) return rc;
        return S.finish("end of a pixel list");
    });
}

int xrt_render_pixels_device(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                             const void *d_centers, int64_t n, void *d_rgba_out, void *d_rgb_f32_out, void *stream, xrt_stats *stats_out) {
    return list_call("xrt_render_pixels_device", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = pixels_check_args(fn, camera, lights, n_lights, opts, n, d_centers, d_rgba_out)) || (rc = aligned16({d_centers, d_rgba_out, d_rgb_f32_out}))) return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene, stream);
        if ((rc = hold.begin(fn)) ||
            (rc = render_pixels_impl(scene, camera, lights, n_lights, opts, (const float *)d_centers, n, (uint32_t *)d_rgba_out, (float *)d_rgb_f32_out, hold.st, stats_out)))
            return rc;
        return guards_check("end of a pixel list");
    });
}

int xrt_trace_pixels(xrt_scene *scene, const xrt_camera *camera, const xrt_render_opts *opts, const float *centers, int64_t n, xrt_ray *rays_out, xrt_hit *hits_out,
                     xrt_stats *stats_out) {
    return list_call("xrt_trace_pixels", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = trace_check_args(fn, camera, opts, n, centers, rays_out, hits_out)) || (rc = centres_finite(fn, centers, n))) return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene);
        if ((rc = hold.begin(fn))) return rc;   // (what is wrong with the arguments alone is said first, also on a host-only scene)
        xrt_scene::TraceWork &W = scene->traceWork;
        const size_t recs = (size_t)n * (opts->use_multisampling == XRT_MS_FIXED16 ? 16u : 1u);   // (a record per sub-ray)
        Staging S(hold.st);
        const float *d_centers = S.in(W.centers, centers, (size_t)n * 2);
        xrt_ray *d_rays = S.out(W.raysOut, rays_out, recs); xrt_hit *d_hits = S.out(W.hitsOut, hits_out, recs);
        if ((rc = S.rc) || (rc = trace_pixels_impl(scene, camera, opts, d_centers, n, d_rays, d_hits, hold.st, stats_out))) return rc;
        return S.finish("end of a pixel list");
    });
}

int xrt_trace_pixels_device(xrt_scene *scene, const xrt_camera *camera, const xrt_render_opts *opts, const void *d_centers, int64_t n, void *d_rays_out,
                            void *d_hits_out, void *stream, xrt_stats *stats_out) {
    return list_call("xrt_trace_pixels_device", scene, [&](const char *fn) -> int {
        int rc;
        if ((rc = trace_check_args(fn, camera, opts, n, d_centers, d_rays_out, d_hits_out)) || (rc = aligned16({d_centers, d_rays_out, d_hits_out}))) return rc;
        if (empty_list(n, stats_out)) return XRT_OK;
        SceneHold hold(scene, stream);
        if ((rc = hold.begin(fn)) || (rc = trace_pixels_impl(scene, camera, opts, (const float *)d_centers, n, (xrt_ray *)d_rays_out, (xrt_hit *)d_hits_out, hold.st, stats_out))) return rc;
        return guards_check("end of a pixel list");
    });
}

int xrt_generate_primary_rays(xrt_scene *scene, const xrt_camera *camera, xrt_ray *rays_out) {
    int rc = need_device(scene, "xrt_generate_primary_rays");
    if (rc != XRT_OK) return rc;
    if (!camera || !rays_out) return fail(XRT_E_INVALID_ARG, "xrt_generate_primary_rays: null argument");
    xrt_render_opts o;
    std::memset(&o, 0, sizeof(o));
    RayGenParams g;
    if ((rc = make_raygen(camera, &o, g))) return rc;
    const long long slots = (long long)g.tilesX * g.tilesY * 512;
    if (slots > (1LL << 25)) return fail(XRT_E_INVALID_ARG, "frame too large");
    std::lock_guard<std::mutex> lock(scene->apiMutex);
    if ((rc = scene->apiRays.ensure((size_t)slots))) return rc;
    hipStream_t st = scene->stream;
    if ((rc = pose_wait(scene, scene->poseCur, st))) return rc;
    launch_raygen(g, pose_view(scene, scene->poseCur), scene->apiRays.p, nullptr, nullptr, nullptr, (int)slots, 0, HeavyArgs(), st);
    HIPCHECK(hipGetLastError());
    std::vector<xrt_ray> tmp((size_t)slots);
    HIPCHECK(hipMemcpyAsync(tmp.data(), scene->apiRays.p, (size_t)slots * sizeof(xrt_ray), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (long long i = 0; i < slots; i++) {   // tile order -> row-major
        long long t = i >> 9;
        int within = (int)(i & 511);
        int wx, wy;
        tile_slot_xy(within, wx, wy);
        int x = (int)(t % g.tilesX) * XRT_TILE_W + wx, y = (int)(t / g.tilesX) * XRT_TILE_H + wy;
        if (x < g.width && y < g.height) rays_out[(size_t)y * g.width + x] = tmp[(size_t)i];
    }
    return XRT_OK;
}

}  // extern "C"
