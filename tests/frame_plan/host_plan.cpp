// plan_frame (csrc/frame_plan.h) on scenes filled by hand, as a program of its own for a sanitizer build (csrc/Makefile `hostcheck_plan`): the scene has
// device -1 and owns nothing, so no HIP function is called.  The program sweeps scene kind x sampling x Transparent materials x collect_stats x batch x
// lights x float output x parts x shards / tile table x MaxReflections x frame size, and asserts on every plan what the comments of plan_frame state: what each
// shortcut implies, the level map and the sizes, the many-lights bounds, a batch's shape; then the switches of Settings one at a time, the refusals with
// their codes, and that planning twice gives the same plan.  Prints one "check <name> plans <n> on <n>" line per flag and "host_plan: ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/xrt.h"
#include "../../xna-ray-trace_amd/csrc/device_res.h"

using namespace xrt;

#include "../../xna-ray-trace_amd/csrc/scene_state.h"

static int g_failed = 0;
static std::string g_case;
#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            if (g_failed++ < 40) fprintf(stderr, "host_plan: %s:%d: (%s) does not hold for %s\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
        }                                                                                                   \
    } while (0)
#define IMPLIES(a, b) CHECK(!(a) || (b))

enum Kind { ONE_BODY_FACING = 0, ONE_BODY_ALL_ROUND, TWO_LEVEL };

// What the planner reads of a scene: a root box two units wide ten units in front of the camera, one mesh record, the mode and what scene_upload derives.
static void fill_scene(xrt_scene &s, Kind kind, bool transparent) {
    s.device = -1;
    s.cfg = Settings();
    s.hs.arrays.snodes.assign(2, f4{0, 0, 0, 0});
    s.hs.arrays.snodes[0] = f4{-1.0f, -1.0f, -11.0f, 0.0f};
    s.hs.arrays.snodes[1] = f4{1.0f, 1.0f, -9.0f, 0.0f};
    MeshRec m;
    std::memset(&m, 0, sizeof(m));
    // the normal box of the one mesh: all normals within 0.2 of +y (a terrain), or normals of every direction
    if (kind == ONE_BODY_ALL_ROUND) { for (int c = 0; c < 3; c++) { m.nbMin[c] = -1.0f; m.nbMax[c] = 1.0f; } }
    else { m.nbMin[0] = -0.2f; m.nbMax[0] = 0.2f; m.nbMin[1] = 0.9f; m.nbMax[1] = 1.0f; m.nbMin[2] = -0.2f; m.nbMax[2] = 0.2f; }
    s.hs.arrays.meshes.assign(1, m);
    s.sceneMode = kind == TWO_LEVEL ? MODE_SCENE : MODE_SINGLE;
    s.packetOk = true;
    s.deepMeshes = true;
    s.view.nodeCull = 1;
    s.heavyPath = kind == TWO_LEVEL ? 0.0f : 0.25f;
    s.mat[0].anyTransparent = transparent;
    s.lastFrameMs = 1.0f;       // (long enough for a context's own stream)
    s.wallClockKHz = 100000;
}

static xrt_camera camera(int w, int h) {
    xrt_camera c;
    std::memset(&c, 0, sizeof(c));
    for (int i = 0; i < 4; i++) c.view[5 * i] = 1.0f;   // the eye at the origin, looking down -z
    const float nearZ = 0.1f, farZ = 100.0f, t = 1.0f / std::tan(0.5f * 1.0471976f);
    c.proj[0] = t * (float)h / (float)w; c.proj[5] = t; c.proj[10] = farZ / (nearZ - farZ); c.proj[11] = -1.0f; c.proj[14] = nearZ * farZ / (nearZ - farZ);
    c.vp_width = w; c.vp_height = h; c.vp_min_depth = 0.0f; c.vp_max_depth = 1.0f;
    return c;
}

static std::vector<xrt_light> lights_of(int n) {
    std::vector<xrt_light> l((size_t)n);
    for (int i = 0; i < n; i++) {
        std::memset(&l[(size_t)i], 0, sizeof(xrt_light));
        l[(size_t)i].kind = (i & 1) ? XRT_LIGHT_DIRECTIONAL : XRT_LIGHT_SPOT;
        l[(size_t)i].direction[1] = -1.0f; l[(size_t)i].intensity = 1.0f; l[(size_t)i].spot_angle = 1.0f; l[(size_t)i].decay_exponent = 1.3f;
    }
    return l;
}

struct Case {
    Kind kind = ONE_BODY_FACING;
    int ms = XRT_MS_OFF, quality = 0;
    bool transparent = false, collect = false;
    int batch = 0;   // 0 none, 1 batch, 2 batch with paths
    int nL = 1;
    bool f32 = false;
    int nParts = 1, shards = 1;
    bool table = false;
    int R = 0, w = 64, h = 27;
};

static std::string describe(const Case &c) {
    char b[256];
    snprintf(b, sizeof(b), "kind %d ms %d q %d transparent %d collect %d batch %d lights %d f32 %d parts %d shards %d table %d R %d %dx%d", (int)c.kind, c.ms, c.quality,
             (int)c.transparent, (int)c.collect, c.batch, c.nL, (int)c.f32, c.nParts, c.shards, (int)c.table, c.R, c.w, c.h);
    return b;
}

// Every member of a plan by name (pointers as numbers), for comparisons that leave out the members a switch may change.
static std::vector<std::pair<std::string, double>> fields(const FramePlan &p) {
    std::vector<std::pair<std::string, double>> f;
    auto add = [&](const char *n, double v) { f.emplace_back(n, v); };
    const RayGenParams &g = p.g;
    for (int i = 0; i < 16; i++) add(("g.m" + std::to_string(i)).c_str(), g.m[i]);
    add("g.vpX", g.vpX); add("g.vpY", g.vpY); add("g.vpW", g.vpW); add("g.vpH", g.vpH); add("g.minDepth", g.minDepth); add("g.depthRange", g.depthRange);
    add("g.width", g.width); add("g.height", g.height); add("g.tilesX", g.tilesX); add("g.tilesY", g.tilesY); add("g.shardRank", g.shardRank); add("g.shardCount", g.shardCount);
    add("g.tileOfSlot", (double)(uintptr_t)g.tileOfSlot); add("g.samples", g.samples); add("g.quadLevel", g.quadLevel); add("g.quadSize", g.quadSize);
    add("g.cullX0", g.cullX0); add("g.cullY0", g.cullY0); add("g.cullX1", g.cullX1); add("g.cullY1", g.cullY1); add("g.cullSkipsRecord", g.cullSkipsRecord);
    add("g.lvl.on", g.lvl.on); add("g.lvl.tilesX", g.lvl.tilesX); add("g.lvl.tx0", g.lvl.tx0); add("g.lvl.ty0", g.lvl.ty0); add("g.lvl.rw", g.lvl.rw); add("g.lvl.shift", g.lvl.shift); add("g.lvl.inv", g.lvl.inv);
    add("g.pathsMul", g.pathsMul); add("g.pathsCap", g.pathsCap); add("g.batch", (double)(uintptr_t)g.batch); add("g.batchRefIndex", g.batchRefIndex);
    add("R", p.R); add("nL", p.nL); add("addressMode", p.addressMode); add("filtering", p.filtering); add("tabled", p.tabled);
    add("totalTiles", (double)p.totalTiles); add("myTiles", (double)p.myTiles); add("totalPixels", (double)p.totalPixels); add("framePaths", (double)p.framePaths);
    add("partStart", (double)p.partStart); add("firstPaths", (double)p.firstPaths); add("hintPaths", (double)p.hintPaths); add("validPixels", (double)p.validPixels);
    add("nodes", (double)p.nodes); add("chunkPaths", (double)p.chunkPaths); add("P", p.P); add("rayCap", (double)p.rayCap); add("liveCap", (double)p.liveCap);
    add("lvlStride", (double)p.lvlStride); add("shadowCap", (double)p.shadowCap); add("cntStride", p.cntStride); add("qStride", p.qStride); add("lvlVerified", p.lvlVerified);
    add("heap", p.heap); add("adaptive", p.adaptive); add("quality", p.quality); add("batch", p.batch); add("capturePaths", p.capturePaths); add("collect", p.collect);
    add("fast", p.fast); add("heapFast", p.heapFast); add("adaptiveFast", p.adaptiveFast); add("ae", p.ae); add("finishA", p.finishA); add("endEarly", p.endEarly);
    add("skipTiles", p.skipTiles); add("endSkipped", (double)p.endSkipped); add("fuseResolve", p.fuseResolve); add("wantF32", p.wantF32);
    add("wantFeedback", p.wantFeedback); add("listLong", p.listLong); add("hinted", p.hinted); add("tileCosts", p.tileCosts); add("useStamps", p.useStamps);
    add("pkMask", p.pkMask); add("ownStream", p.ownStream); add("cntBase", p.cntBase); add("levelCap", p.levelCap);
    return f;
}
static double field(const FramePlan &p, const char *name) {
    for (auto &kv : fields(p)) if (kv.first == name) return kv.second;
    fprintf(stderr, "host_plan: no member %s\n", name);
    g_failed++;
    return -1.0;
}
// The members in which a and b differ.
static std::set<std::string> differing(const FramePlan &a, const FramePlan &b) {
    std::set<std::string> d;
    const auto fa = fields(a), fb = fields(b);
    for (size_t i = 0; i < fa.size(); i++) if (!(fa[i].second == fb[i].second)) d.insert(fa[i].first);
    return d;
}

static std::vector<int> g_table;   // the installed tile table of the sweep's sharded cases

// Install (or remove) a tile table for frames of w x h pixels on `shards` ranks: round-robin with a spare slot per rank (-1).
static void set_table(xrt_scene &s, bool on, int w, int h, int shards) {
    s.tileTable.clear(); s.tileTableDev.p = nullptr; s.tableW = s.tableH = s.tableCount = s.tableTpr = 0;
    if (!on) return;
    const int tiles = ((w + XRT_TILE_W - 1) / XRT_TILE_W) * ((h + XRT_TILE_H - 1) / XRT_TILE_H), tpr = (tiles + shards - 1) / shards + 1;
    g_table.assign((size_t)shards * tpr, -1);
    for (int t = 0; t < tiles; t++) g_table[(size_t)(t % shards) * tpr + t / shards] = t;
    s.tileTable = g_table;
    s.tileTableDev.p = g_table.data();   // (only its address is taken; taken back before the scene is destroyed)
    s.tableW = w; s.tableH = h; s.tableCount = shards; s.tableTpr = tpr;
}

struct Call {
    xrt_camera cam;
    std::vector<xrt_light> lights;
    xrt_render_opts opts;
    BatchSrc batch;
    BatchSrc::Paths paths;
    xrt_ray dummyRay;
    long long dummyStart[2] = {0, 0};
    int part = 0;
};
static void make_call(const Case &c, Call &k) {
    k.cam = camera(c.w, c.h);
    k.lights = lights_of(c.nL);
    std::memset(&k.opts, 0, sizeof(k.opts));
    k.opts.max_reflections = c.R; k.opts.use_multisampling = c.ms; k.opts.multisample_quality = c.quality;
    k.opts.address_mode = XRT_ADDRESS_WRAP; k.opts.filtering = XRT_FILTER_POINT;
    k.opts.shard_count = c.shards; k.opts.shard_rank = c.shards > 1 ? 1 : 0; k.opts.collect_stats = c.collect ? 1 : 0;
    k.batch = BatchSrc();
    k.batch.rays = &k.dummyRay; k.batch.n = (long long)c.w * c.h; k.batch.refIndex = 1.0f;
    k.paths.vertexStart = k.dummyStart;
    if (c.batch == 2) k.batch.paths = &k.paths;
    k.part = c.nParts > 1 ? 1 : 0;
}
static int plan(const xrt_scene &s, const Case &c, Call &k, FramePlan &p) {
    return plan_frame(s, 0, c.batch ? nullptr : &k.cam, k.lights.data(), c.nL, &k.opts, c.f32, false, k.part, c.nParts, true, c.batch ? &k.batch : nullptr, p);
}

static long long g_plans = 0, g_refused = 0;
static long long g_on[16] = {0};
enum { ON_FAST, ON_HEAPFAST, ON_ADAPTIVEFAST, ON_AE, ON_FINISHA, ON_ENDEARLY, ON_SKIPTILES, ON_FUSE, ON_LVL, ON_FEEDBACK, ON_MULTICHUNK, ON_TABLED, ON_F32, ON_COUNT };
static const char *ON_NAMES[ON_COUNT] = {"fast", "heapFast", "adaptiveFast", "ae", "finishA", "endEarly", "skipTiles", "fuseResolve", "levelMap", "wantFeedback", "multiChunk", "tabled", "wantF32"};

// What the comments of plan_frame state, on one plan.
static void check_plan(const xrt_scene &s, const Case &c, const FramePlan &p) {
    const RayGenParams &g = p.g;
    const bool oneChunk = p.firstPaths <= p.chunkPaths, batch = c.batch != 0, tree = p.heap, adaptive = c.ms == XRT_MS_ADAPTIVE;
    const bool facing = c.kind == ONE_BODY_FACING;
    CHECK(p.R == c.R && p.nL == c.nL && p.batch == batch && p.adaptive == adaptive && p.collect == c.collect);
    CHECK(tree == (c.transparent && c.R > 0));
    CHECK(p.P == (int)p.chunkPaths && p.chunkPaths > 0 && p.chunkPaths <= p.firstPaths);
    CHECK(p.cntStride == 5 * (c.R + 2) && p.qStride == (1 + 2 * PACKET_QUEUE_WORDS) * (c.R + 2));
    CHECK(p.nodes == (tree ? ((size_t)1 << (c.R + 1)) - 1 : (size_t)(c.R + 1)));
    // flag implications
    IMPLIES(p.fast, !p.collect && !batch && oneChunk);
    IMPLIES(p.fast && tree, p.heapFast);
    IMPLIES(p.fast && adaptive, p.adaptiveFast);
    IMPLIES(p.heapFast, p.fast && tree);
    IMPLIES(p.adaptiveFast, p.fast && adaptive && !tree && p.cntBase == ADAPTIVE_LEVEL_WORDS && p.levelCap == p.totalPixels);
    IMPLIES(!p.adaptiveFast, p.cntBase == 0);
    IMPLIES(p.ae, s.sceneMode == MODE_SINGLE && !tree && !adaptive && c.nParts == 1 && oneChunk && !p.collect && s.view.nodeCull != 0 && facing);
    IMPLIES(p.finishA, p.ae && c.nL <= 32 && !p.capturePaths);
    IMPLIES(p.endEarly, p.finishA && p.fast && !batch && !c.f32 && !p.fuseResolve);
    IMPLIES(p.skipTiles, p.endEarly && g.lvl.on && g.samples > 1);
    CHECK(p.endSkipped == (p.skipTiles ? (unsigned long long)(p.totalTiles - lvl_kept_tiles(g)) << g.lvl.shift : 0ull));
    IMPLIES(p.fuseResolve, g.samples == 1 && !tree && !adaptive && !batch);
    CHECK(p.wantF32 == (c.f32 && !adaptive && g.samples == 1));
    // ... and the other way round, where the comments say when a shortcut is taken (default switches)
    CHECK(p.fast == (!p.collect && !batch && oneChunk && (!adaptive || (!tree && c.nParts == 1 && p.totalPixels * 4 <= p.chunkPaths)) && (!tree || c.nParts == 1)));
    CHECK(p.ae == ((p.fast || (batch && oneChunk && !p.collect)) && !tree && !adaptive && c.nParts == 1 && c.kind != TWO_LEVEL && facing));
    CHECK(p.finishA == (p.ae && c.nL <= 32 && c.batch != 2));
    CHECK(p.endEarly == (p.finishA && p.fast && !c.f32));
    CHECK(p.skipTiles == (p.endEarly && g.lvl.on && g.samples > 1));
    CHECK(p.fuseResolve == (g.samples == 1 && !tree && !adaptive && !batch && !p.endEarly));
    // level map and sizes
    if (g.lvl.on) {
        CHECK(g.shardCount == 1 && !p.tabled && c.nParts == 1 && oneChunk && !tree && !adaptive);
        const long long kept = lvl_kept_tiles(g);
        CHECK(kept > 0 && kept < p.totalTiles && p.lvlStride == (size_t)(kept << g.lvl.shift) && p.lvlStride < (size_t)p.P);
        CHECK(g.lvl.shift == 9 + (g.samples == 16 ? 4 : 0) && g.lvl.tilesX == g.tilesX);
        for (long long t = 0; t < p.totalTiles; t++) CHECK((unsigned)(((unsigned long long)t * g.lvl.inv) >> 32) == (unsigned)(t / g.tilesX));
    } else CHECK(p.lvlStride == (size_t)p.P);
    IMPLIES(!tree, p.rayCap <= (size_t)p.P);
    CHECK((unsigned long long)p.rayCap * (unsigned long long)(c.nL > 0 ? c.nL : 1) <= (1ull << 30));
    IMPLIES(!tree && !adaptive, p.liveCap == p.rayCap);
    CHECK(p.shadowCap == p.rayCap);
    IMPLIES(tree, p.rayCap >= (size_t)p.P && p.liveCap == (size_t)p.P);
    // the many-lights bounds: the chunk shrinks, the frame is not refused
    {
        long long maxPaths = s.cfg.maxChunkPaths;
        const long long lightBound = (1LL << 30) / (c.nL > 0 ? c.nL : 1);
        if (maxPaths > lightBound) maxPaths = lightBound & ~8191LL;
        if (c.nL > 0) { const long long byBytes = (s.cfg.shadowBytes / (84LL * c.nL)) & ~8191LL; if (byBytes < maxPaths) maxPaths = byBytes < 8192 ? 8192 : byBytes; }
        if (!tree) CHECK(p.chunkPaths == (p.firstPaths < maxPaths ? p.firstPaths : maxPaths));
        else CHECK(p.chunkPaths <= maxPaths && p.chunkPaths <= (1 << 21));
        if (c.nL == 100 && c.w == 1920 && !tree && !batch && c.ms == XRT_MS_OFF && c.nParts == 1 && c.shards == 1)
            CHECK(p.chunkPaths == ((s.cfg.shadowBytes / (84LL * 100)) & ~8191LL) && !oneChunk && !p.fast);
    }
    // batches
    if (batch) {
        CHECK(g.width == c.w * c.h && g.height == 1 && g.samples == 1 && !g.lvl.on && g.shardCount == 1 && g.batch != nullptr && !g.tileOfSlot);
        CHECK((p.pkMask & 1) == 0 && p.framePaths == (long long)c.w * c.h && p.validPixels == (unsigned long long)p.framePaths);
        CHECK(p.capturePaths == (c.batch == 2));
    } else {
        CHECK(g.width == c.w && g.height == c.h && g.samples == (c.ms == XRT_MS_FIXED16 ? 16 : (adaptive ? 4 : 1)));
        CHECK(p.tabled == (c.table && c.shards > 1) && (g.tileOfSlot != nullptr) == p.tabled);
        CHECK(p.framePaths == p.myTiles * 512 * g.samples && p.totalTiles == (long long)g.tilesX * g.tilesY);
        if (c.nParts == 1 && c.shards == 1) CHECK(p.validPixels == (unsigned long long)c.w * c.h && p.hintPaths == (adaptive ? -1 : p.firstPaths));
        CHECK(p.validPixels <= (unsigned long long)c.w * c.h);
        IMPLIES(!(c.table && c.nParts > 1), p.validPixels > 0);   // (the second part of a tabled rank may hold its spare slot alone)
        CHECK(p.pkMask == (tree ? ((c.kind == TWO_LEVEL && (long long)c.w * c.h * g.samples >= 600000LL) ? 7 : 0) : (c.kind == TWO_LEVEL ? 23 : (g.samples >= 16 ? 7 : 0))));
    }
    CHECK(p.ownStream == p.fast && p.useStamps && !p.hinted);
    CHECK(p.tileCosts == (p.fast && !adaptive && !tree));
    CHECK(p.wantFeedback == (p.fast && !tree && !adaptive && (p.pkMask & 5) != 5));
    g_on[ON_FAST] += p.fast; g_on[ON_HEAPFAST] += p.heapFast; g_on[ON_ADAPTIVEFAST] += p.adaptiveFast; g_on[ON_AE] += p.ae; g_on[ON_FINISHA] += p.finishA;
    g_on[ON_ENDEARLY] += p.endEarly; g_on[ON_SKIPTILES] += p.skipTiles; g_on[ON_FUSE] += p.fuseResolve; g_on[ON_LVL] += g.lvl.on != 0; g_on[ON_FEEDBACK] += p.wantFeedback;
    g_on[ON_MULTICHUNK] += !oneChunk; g_on[ON_TABLED] += p.tabled; g_on[ON_F32] += p.wantF32;
}

// Is the combination one that plan_frame refuses, and with which code?
static int expected_code(const Case &c) {
    const bool adaptive = c.ms == XRT_MS_ADAPTIVE;
    if (c.batch && (c.ms != XRT_MS_OFF || c.shards > 1 || c.nParts > 1)) return XRT_E_INTERNAL;
    if (c.nParts > 1 && adaptive) return XRT_E_INTERNAL;
    if (c.nParts > 1) {   // parts are whole multiples of 8192 paths: a frame too small for its second part (the one the sweep plans) is not split
        const long long tiles = (long long)((c.w + XRT_TILE_W - 1) / XRT_TILE_W) * ((c.h + XRT_TILE_H - 1) / XRT_TILE_H);
        const long long mine = c.shards > 1 ? (tiles + c.shards - 1) / c.shards + (c.table ? 1 : 0) : tiles;   // (set_table: a spare slot per rank)
        const long long paths = mine * 512 * (c.ms == XRT_MS_FIXED16 ? 16 : 1), stride = ((paths / c.nParts + 8191) / 8192) * 8192;
        if (paths - stride <= 0) return XRT_E_INTERNAL;
    }
    return XRT_OK;
}

static void sweep() {
    const int msModes[4][2] = {{XRT_MS_OFF, 0}, {XRT_MS_FIXED16, 0}, {XRT_MS_ADAPTIVE, 0}, {XRT_MS_ADAPTIVE, 2}};
    const int lightCounts[4] = {0, 1, 33, 100}, sizes[2][2] = {{64, 27}, {1920, 1080}};
    const int shardCases[3][2] = {{1, 0}, {4, 0}, {4, 1}};
    for (int kind = 0; kind < 3; kind++) for (int tr = 0; tr < 2; tr++) {
        xrt_scene s;
        fill_scene(s, (Kind)kind, tr != 0);
        for (auto &sz : sizes) for (auto &sh : shardCases) {
            set_table(s, sh[1] != 0, sz[0], sz[1], sh[0]);
            for (auto &ms : msModes) for (int collect = 0; collect < 2; collect++) for (int batch = 0; batch < 3; batch++) for (int nL : lightCounts)
                for (int f32 = 0; f32 < 2; f32++) for (int nParts = 1; nParts <= 2; nParts++) for (int R : {0, 3}) {
                    Case c;
                    c.kind = (Kind)kind; c.transparent = tr != 0; c.w = sz[0]; c.h = sz[1]; c.shards = sh[0]; c.table = sh[1] != 0; c.ms = ms[0]; c.quality = ms[1];
                    c.collect = collect != 0; c.batch = batch; c.nL = nL; c.f32 = f32 != 0; c.nParts = nParts; c.R = R;
                    g_case = describe(c);
                    Call k;
                    make_call(c, k);
                    FramePlan p, again;
                    const int rc = plan(s, c, k, p);
                    CHECK(rc == expected_code(c));
                    if (rc != XRT_OK) { g_refused++; continue; }
                    g_plans++;
                    check_plan(s, c, p);
                    CHECK(plan(s, c, k, again) == XRT_OK && differing(p, again).empty());   // planning twice gives the same plan
                    // the level-map memo is the caller's: with the geometry noted, the plan is the same but for the report
                    if (p.lvlVerified) {
                        s.lvlCheckedTilesX = p.g.tilesX; s.lvlCheckedTiles = p.totalTiles;
                        CHECK(plan(s, c, k, again) == XRT_OK && differing(p, again) == std::set<std::string>{"lvlVerified"} && !again.lvlVerified);
                        s.lvlCheckedTilesX = 0; s.lvlCheckedTiles = 0;
                    }
                }
        }
        set_table(s, false, 0, 0, 0);
    }
}

// Switching one gate of Settings off turns off that flag and nothing but the members that depend on it.
static void switches() {
    struct Gate { const char *name; void (*off)(xrt_scene &); const char *flag; std::set<std::string> dependents; Case c; };
    Case plain16; plain16.ms = XRT_MS_FIXED16; plain16.R = 3; plain16.w = 1920; plain16.h = 1080;            // one body facing, 16 sub-rays: every shortcut on
    Case plain1 = plain16; plain1.ms = XRT_MS_OFF;
    Case tree = plain1; tree.transparent = true;
    Case adapt = plain1; adapt.ms = XRT_MS_ADAPTIVE; adapt.quality = 2;
    const std::set<std::string> endDeps = {"endEarly", "skipTiles", "endSkipped", "fuseResolve"};
    std::set<std::string> finishDeps = endDeps; finishDeps.insert("finishA");
    std::set<std::string> aeDeps = finishDeps; aeDeps.insert("ae");
    const std::vector<Gate> gates = {
        {"answerAtEmission", [](xrt_scene &s) { s.cfg.answerAtEmission = false; }, "ae", aeDeps, plain16},
        {"finishInPartA", [](xrt_scene &s) { s.cfg.finishInPartA = false; }, "finishA", finishDeps, plain16},
        {"endEarly", [](xrt_scene &s) { s.cfg.endEarly = false; }, "endEarly", endDeps, plain16},
        {"endEarly (one sample)", [](xrt_scene &s) { s.cfg.endEarly = false; }, "endEarly", endDeps, plain1},
        {"levelMap", [](xrt_scene &s) { s.cfg.levelMap = false; }, "g.lvl.on", {"g.lvl.on", "g.lvl.tilesX", "g.lvl.tx0", "g.lvl.ty0", "g.lvl.rw", "g.lvl.shift", "g.lvl.inv", "lvlStride", "lvlVerified", "skipTiles", "endSkipped"}, plain16},
        {"heapFast", [](xrt_scene &s) { s.cfg.heapFast = false; }, "heapFast", {"heapFast", "fast", "ownStream", "hinted"}, tree},
        {"heapFastOk", [](xrt_scene &s) { s.heapFastOk = false; }, "heapFast", {"heapFast", "fast", "ownStream", "hinted"}, tree},
        {"adaptiveFast", [](xrt_scene &s) { s.cfg.adaptiveFast = false; }, "adaptiveFast", {"adaptiveFast", "fast", "ownStream", "hinted", "cntBase", "levelCap"}, adapt},
        {"adaptiveFastOk", [](xrt_scene &s) { s.adaptiveFastOk = false; }, "adaptiveFast", {"adaptiveFast", "fast", "ownStream", "hinted", "cntBase", "levelCap"}, adapt},
        {"gridHints", [](xrt_scene &s) { s.cfg.gridHints = false; }, "hinted", {"hinted"}, plain16},
        {"launchTiming", [](xrt_scene &s) { s.cfg.launchTiming = false; }, "useStamps", {"useStamps"}, plain16},
        {"launchEvents", [](xrt_scene &s) { s.cfg.launchEvents = true; }, "useStamps", {"useStamps"}, plain16},
        {"oneStream", [](xrt_scene &s) { s.cfg.oneStream = true; }, "ownStream", {"ownStream"}, plain16},
        {"noFeedback", [](xrt_scene &s) { s.cfg.noFeedback = true; }, "wantFeedback", {"wantFeedback"}, plain1},
        {"packetOk", [](xrt_scene &s) { s.packetOk = false; }, "tileCosts", {"tileCosts", "pkMask", "wantFeedback"}, plain16},
    };
    for (const Gate &G : gates) {
        g_case = std::string("switch ") + G.name;
        xrt_scene s;
        fill_scene(s, ONE_BODY_FACING, G.c.transparent);
        Call k;
        make_call(G.c, k);
        FramePlan base, off;
        CHECK(plan(s, G.c, k, base) == XRT_OK);
        s.genKey = base.firstPaths * 64 + base.nL; s.genHeap = base.heap;   // (as after a frame of this geometry: the grid hints apply)
        CHECK(plan(s, G.c, k, base) == XRT_OK);
        CHECK(field(base, G.flag) != 0.0 && base.hinted);
        G.off(s);
        CHECK(plan(s, G.c, k, off) == XRT_OK);
        CHECK(field(off, G.flag) == 0.0);
        for (const std::string &d : differing(base, off))
            if (!G.dependents.count(d)) { fprintf(stderr, "host_plan: switch %s changes %s\n", G.name, d.c_str()); g_failed++; }
    }
    {   // a packet mask that is named stays as named, for a batch too
        g_case = "named packet mask";
        xrt_scene s;
        fill_scene(s, ONE_BODY_FACING, false);
        s.cfg.packetMask = 7;
        Case c; c.batch = 1;
        Call k;
        make_call(c, k);
        FramePlan p;
        CHECK(plan(s, c, k, p) == XRT_OK && p.pkMask == 7);
        s.cfg.packetMask = -1;
        CHECK(plan(s, c, k, p) == XRT_OK && p.pkMask == 0);
        c.ms = XRT_MS_FIXED16; c.batch = 0;
        make_call(c, k);
        CHECK(plan(s, c, k, p) == XRT_OK && p.pkMask == 7);
    }
    {   // the shadow budget in bytes is a switch as well: a small one shrinks the chunk to no less than 8192 paths
        g_case = "shadow bytes";
        xrt_scene s;
        fill_scene(s, TWO_LEVEL, false);
        s.cfg.shadowBytes = 1LL << 20;
        Case c; c.nL = 100; c.w = 1920; c.h = 1080;
        Call k;
        make_call(c, k);
        FramePlan p;
        CHECK(plan(s, c, k, p) == XRT_OK && p.chunkPaths == 8192 && !p.fast);
    }
}

// Every refusal with its present code and message.
static void refusals() {
    xrt_scene s;
    fill_scene(s, ONE_BODY_FACING, false);
    auto refused = [&](const char *what, const Case &c, int code, const char *text, void (*edit)(Call &) = nullptr) {
        g_case = std::string("refusal ") + what;
        Call k;
        make_call(c, k);
        if (edit) edit(k);
        FramePlan p;
        p.R = -77;
        const int rc = plan(s, c, k, p);
        CHECK(rc == code);
        CHECK(g_err.find(text) != std::string::npos);
        CHECK(p.R == -77);   // a refused call writes no plan
    };
    Case c;
    c.R = 65; refused("R > 64", c, XRT_E_INVALID_ARG, "max_reflections out of range");
    c.R = -1; refused("R < 0", c, XRT_E_INVALID_ARG, "max_reflections out of range");
    c = Case(); c.ms = XRT_MS_ADAPTIVE; c.quality = 7; refused("quality > 6", c, XRT_E_UNSUPPORTED, "MultisampleQuality above 6");
    c = Case(); c.batch = 1; c.ms = XRT_MS_FIXED16; refused("batch with supersampling", c, XRT_E_INTERNAL, "a ray batch is a plain pass");
    c = Case(); c.batch = 1; c.shards = 4; refused("batch with shards", c, XRT_E_INTERNAL, "a ray batch is a plain pass");
    c = Case(); c.nL = 2; refused("unknown light kind", c, XRT_E_INVALID_ARG, "unknown light kind", [](Call &k) { k.lights[1].kind = 7; });
    c = Case(); refused("address mode", c, XRT_E_INVALID_ARG, "addressMode (MAT:85)", [](Call &k) { k.opts.address_mode = 3; });
    c = Case(); refused("filtering", c, XRT_E_INVALID_ARG, "filtering (MAT:97)", [](Call &k) { k.opts.filtering = 2; });
    c = Case(); refused("sampling mode", c, XRT_E_INVALID_ARG, "use_multisampling", [](Call &k) { k.opts.use_multisampling = 3; });
    c = Case(); refused("viewport", c, XRT_E_INVALID_ARG, "viewport must be positive", [](Call &k) { k.cam.vp_width = 0; });
    c = Case(); c.shards = 4; refused("shard rank", c, XRT_E_INVALID_ARG, "shard_rank out of range", [](Call &k) { k.opts.shard_rank = 4; });
    c = Case(); c.nParts = 2; c.ms = XRT_MS_ADAPTIVE; refused("parts of an adaptive frame", c, XRT_E_INTERNAL, "frame parts need a plain frame");
    {
        g_case = "refusal null arguments";
        FramePlan p;
        CHECK(plan_frame(s, 0, nullptr, nullptr, 0, nullptr, false, false, 0, 1, true, nullptr, p) == XRT_E_INVALID_ARG && g_err == "xrt_render: null argument");
    }
    s.mat[0].anyTransparent = true;
    c = Case(); c.transparent = true; c.R = 13; refused("ray tree with R > 12", c, XRT_E_UNSUPPORTED, "Transparent materials with MaxReflections > 12");
    {   // R = 12 is the deepest ray tree: planned, not refused
        g_case = "ray tree with R = 12";
        c.R = 12;
        Call k;
        make_call(c, k);
        FramePlan p;
        CHECK(plan(s, c, k, p) == XRT_OK && p.heap && p.nodes == 8191);
    }
}

int main() {
    sweep();
    switches();
    refusals();
    printf("plans %lld refused %lld\n", g_plans, g_refused);
    for (int i = 0; i < ON_COUNT; i++) {
        printf("check %s plans %lld on %lld\n", ON_NAMES[i], g_plans, g_on[i]);
        if (g_on[i] == 0 || g_on[i] == g_plans) { fprintf(stderr, "host_plan: the sweep never switches %s\n", ON_NAMES[i]); g_failed++; }
    }
    if (g_failed) { fprintf(stderr, "host_plan: %d check(s) failed\n", g_failed); return 1; }
    printf("host_plan: ok\n");
    return 0;
}
