// The packet walk with the table of screen boxes (csrc/screen_rects.h), as a host model -- the walk of tests/packet_quads/packet_quads.cpp (packet.hip pk_walk: the
// same tests in the same order, with the library's own functions), one packet per aligned unit of 64 paths, on fixtures.heightfield(177) at 480 x 270 with 16
// sub-rays per pixel: the benchmark's triangles per pixel.  A host program of its own (csrc/Makefile `screen_model`: host code under ASan and UBSan;
// tests/test_screen_rects_cpu.py builds and runs it).  The rays are k_raygen's and lane_begin's (unproject twice, normalize, the body transform: binary32, operation
// for operation), the entries screen_entry's, a packet's rectangle screen_packet_rect's of its 2 x 2 pixel quad.  The frame is walked twice, without the filter
// and with it -- a leaf none of whose entries overlaps the packet's rectangle is left before leaf_margin, a run without one before its box test, and only the
// overlapping references get a triangle step -- and the program prints, for both, leaves scanned, run tests, triangle steps and lanes per triangle step, the
// share of "no cull" entries, and how many paths have different answers (none may).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../xna-ray-trace_amd/csrc/scene_host.h"
#include "../../xna-ray-trace_amd/csrc/screen_rects.h"

using namespace xrt;

struct Mesh { std::vector<float> v, sn; float bbox[6]; int ntri() const { return (int)(v.size() / 9); } };
static void finish(Mesh &m) {
    const int n = m.ntri();
    m.sn.resize((size_t)n * 3);
    for (int k = 0; k < 3; k++) { m.bbox[k] = std::numeric_limits<float>::max(); m.bbox[3 + k] = -std::numeric_limits<float>::max(); }
    for (int t = 0; t < n; t++) {
        const float *p = &m.v[(size_t)t * 9];
        const v3 e1 = mk(p[3] - p[0], p[4] - p[1], p[5] - p[2]), e2 = mk(p[6] - p[0], p[7] - p[1], p[8] - p[2]);
        const v3 c = cross(e2, e1);   // the surface normal of fixtures.surface_normals: normalize(cross(v3 - v1, v2 - v1))
        const float inv = 1.0f / (float)std::sqrt((double)((c.x * c.x + c.y * c.y) + c.z * c.z));
        m.sn[(size_t)t * 3] = c.x * inv; m.sn[(size_t)t * 3 + 1] = c.y * inv; m.sn[(size_t)t * 3 + 2] = c.z * inv;
        for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) { m.bbox[k] = fminf(m.bbox[k], p[3 * j + k]); m.bbox[3 + k] = fmaxf(m.bbox[3 + k], p[3 * j + k]); }
    }
}
static void tri(Mesh &m, const float a[3], const float b[3], const float c[3]) { m.v.insert(m.v.end(), a, a + 3); m.v.insert(m.v.end(), b, b + 3); m.v.insert(m.v.end(), c, c + 3); }
// fixtures.heightfield(m): (m+1)^2 grid over x, z in [-50, 50], y = 4 p(x/50) p(z/50), p(t) = t (1 - t^2) 2.598, two triangles per cell, cell-major -- binary32 throughout
static Mesh heightfield(int m) {
    std::vector<float> c((size_t)m + 1), p((size_t)m + 1);
    for (int i = 0; i <= m; i++) c[(size_t)i] = -50.0f + 100.0f * ((float)i / (float)m);
    c[0] = -50.0f; c[(size_t)m] = 50.0f;
    for (int i = 0; i <= m; i++) { const float t = c[(size_t)i] / 50.0f; p[(size_t)i] = (t * (1.0f - t * t)) * 2.598f; }
    auto P = [&](int i, int j, float out[3]) { out[0] = c[(size_t)i]; out[1] = (4.0f * p[(size_t)i]) * p[(size_t)j]; out[2] = c[(size_t)j]; };
    Mesh h;
    for (int i = 0; i < m; i++) for (int j = 0; j < m; j++) {
        float a[3], b[3], cc[3], d[3];
        P(i, j, a); P(i + 1, j, b); P(i + 1, j + 1, cc); P(i, j + 1, d);
        tri(h, a, b, cc); tri(h, a, cc, d);
    }
    finish(h);
    return h;
}
static bool build(HostScene &s, const Mesh &m, int threshold) {
    static const float IDENT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    xrt_material mat;
    std::memset(&mat, 0, sizeof(mat));
    mat.reflectiveness = 0.3f; mat.refraction_index = 1.0f;
    std::string err;
    const int id = s.add_mesh(m.v.data(), nullptr, nullptr, m.sn.data(), nullptr, m.ntri(), &mat, m.bbox, err);
    if (id < 0 || s.add_object(&id, 1, IDENT, IDENT, m.bbox, m.bbox, err) < 0 || !s.build(threshold, 0, err)) { fprintf(stderr, "screen_model: %s\n", err.c_str()); return false; }
    return true;
}

struct D3 { double x, y, z; };
static D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static D3 operator*(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static D3 crossd(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static D3 unit(D3 a) { const double l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); return a * (1.0 / l); }

// one live ray and its answer
struct LaneRay {
    int path, px, py;   // (px, py: its pixel)
    RayPre r;
    RayCull rc;
    int dmask;
    bool found;
    float key, dist;
    int ref;
};
struct Counts { long packets = 0, blocks = 0, children = 0, leaves = 0, runTests = 0, triSteps = 0, laneSteps = 0, hits = 0; };

// The shared walk of one packet: L[0 .. n) are its lanes.  E: the frame's entries (null: no filter), rect: the packet's screen rectangle.
static void walk_packet(const HostScene &s, LaneRay *L, int n, Counts &K, const ScrEntry *E, ScrEntry rect) {
    const SceneArrays &A = s.arrays;
    const FlatTree &t = s.meshTrees[0];
    if (t.blocks.empty() || n == 0) return;
    struct Frame { int blk; v3 bmin, half; unsigned p; uint64_t lanes; int dm0; unsigned char cb[64]; };
    std::vector<Frame> stack;
    const int cullMin = 4;   // (settings.h packetCullMin)
    const v3 rmn = mk(t.rootBox[0], t.rootBox[1], t.rootBox[2]);
    Frame F;
    F.blk = 0; F.bmin = rmn; F.half = half_of(rmn, mk(t.rootBox[3], t.rootBox[4], t.rootBox[5]));
    F.lanes = n == 64 ? ~0ull : ((1ull << n) - 1ull);   // (every live ray passed the root box)
    bool entering = true, anyFound = false;
    K.packets++;
    for (;;) {
        if (entering) {
            K.blocks++;
            const int d2 = f2i(A.blocks[2 * (size_t)F.blk].z);
            F.dm0 = L[__builtin_ctzll(F.lanes)].dmask;
            F.p = 0u;
            for (int l = 0; l < n; l++) {
                unsigned cb = 0u;
                if ((F.lanes >> l) & 1ull)
                    for (int c = 0; c < 8; c++) {
                        v3 cmin, cmax;
                        child_box(F.bmin, F.half, c, cmin, cmax);
                        float key;
                        if (slab(L[l].r, cmin.x, cmin.y, cmin.z, cmax.x, cmax.y, cmax.z, key)) cb |= 1u << c;
                    }
                cb &= 0xffu & ~((unsigned)(d2 >> 8) & 0xffu);   // empty leaves can never hit
                F.cb[l] = (unsigned char)cb;
                for (int c = 0; c < 8; c++) if ((cb >> c) & 1u) F.p |= 1u << (c ^ F.dm0);   // bit q <-> child (q ^ dm0): front to back for the first lane
            }
            entering = false;
        }
        if (F.p == 0u) {
            if (stack.empty()) break;
            F = stack.back();
            stack.pop_back();
            continue;
        }
        const int c = __builtin_ctz(F.p) ^ F.dm0;
        F.p &= F.p - 1u;
        K.children++;
        const f4 lo = A.blocks[2 * (size_t)F.blk], hi = A.blocks[2 * (size_t)F.blk + 1];
        const int d0 = f2i(lo.x), d1 = f2i(lo.y), d2 = f2i(lo.z), d3 = f2i(lo.w);
        v3 cmin, cmax;
        child_box(F.bmin, F.half, c, cmin, cmax);
        const bool keyed = anyFound;
        bool inC[64];
        float key[64];
        for (int l = 0; l < n; l++) {
            inC[l] = ((F.lanes >> l) & 1ull) && ((F.cb[l] >> c) & 1);
            key[l] = 0.0f;
            if (inC[l]) (void)slab(L[l].r, cmin.x, cmin.y, cmin.z, cmax.x, cmax.y, cmax.z, key[l]);   // the entry key (the test's outcome is known: hit)
        }
        const int node = F.blk * 8 + c;
        if (!((d2 >> c) & 1)) {   // ---- leaf ----
            bool go[64], usable[64], any = false;
            float rho[64];
            for (int l = 0; l < n; l++) {
                go[l] = inC[l] && !all_back_facing(A.leafNB[2 * (size_t)node], A.leafNB[2 * (size_t)node + 1], L[l].r.d);
                if (keyed) go[l] = go[l] && !(L[l].found && key[l] > L[l].key);
                usable[l] = false; rho[l] = 0.0f;
                any = any || go[l];
            }
            if (!any) continue;
            const unsigned long long offLo = (unsigned long long)(unsigned)f2i(hi.x) | ((unsigned long long)(unsigned)f2i(hi.y) << 32);
            const unsigned long long offHi = (unsigned long long)(unsigned)f2i(hi.z) | ((unsigned long long)(unsigned)f2i(hi.w) << 32);
            const int r0 = d1 + child_ref_offset(offLo, offHi, c), r1 = d1 + (c == 7 ? d3 : child_ref_offset(offLo, offHi, c + 1));
            std::vector<char> keep((size_t)(r1 - r0), 1);
            if (E) {
                bool some = false;
                for (int r = r0; r < r1; r++) { keep[(size_t)(r - r0)] = screen_overlap(E[r].x, E[r].y, rect.x, rect.y) ? 1 : 0; some = some || keep[(size_t)(r - r0)]; }
                if (!some) continue;   // (before leaf_margin)
            }
            K.leaves++;
            const bool big = r1 - r0 >= LEAF_RUN_MIN;
            const f4 *tb = &A.leafTB[4 * (size_t)node];
            if (big || r1 - r0 >= cullMin) {
                any = false;
                for (int l = 0; l < n; l++) {
                    usable[l] = leaf_margin(L[l].r, L[l].rc, tb[0], tb[1], tb[2], tb[3], rho[l]);
                    if (r1 - r0 >= cullMin) go[l] = go[l] && !(usable[l] && grown_box_missed(L[l].r, tb[0], tb[1], rho[l]));
                    any = any || go[l];
                }
                if (!any) continue;
            }
            int nRuns = 1, rb = -1;
            if (big) { rb = A.runBase[(size_t)node]; if (rb >= 0) nRuns = (r1 - r0 + LEAF_RUN - 1) / LEAF_RUN; }
            bool cheap = true;
            for (int l = 0; l < n; l++) if (go[l] && !usable[l]) cheap = false;
            for (int jr = 0; jr < nRuns; jr++) {
                int ra = r0, rz = r1;
                bool goR[64];
                int nGo = 0;
                for (int l = 0; l < n; l++) goR[l] = go[l];
                if (rb >= 0) {
                    ra = r0 + LEAF_RUN * jr; rz = ra + LEAF_RUN < r1 ? ra + LEAF_RUN : r1;
                    { bool some = false; for (int r = ra; r < rz; r++) some = some || keep[(size_t)(r - r0)]; if (!some) continue; }   // (before the run's box test)
                    const f4 *rt = &A.runTB[4 * ((size_t)rb + (size_t)jr)];
                    K.runTests++;
                    for (int l = 0; l < n; l++)
                        if (go[l]) goR[l] = cheap ? !grown_box_missed(L[l].r, rt[0], rt[1], rho[l]) : !leaf_certainly_missed(L[l].r, L[l].rc, rt[0], rt[1], rt[2], rt[3]);
                }
                for (int l = 0; l < n; l++) nGo += goR[l];
                if (!nGo) continue;
                int steps = 0;
                for (int r = ra; r < rz; r++) steps += keep[(size_t)(r - r0)];
                K.triSteps += steps; K.laneSteps += (long)steps * nGo;
                for (int r = ra; r < rz; r++) {
                    if (!keep[(size_t)(r - r0)]) continue;
                    const f4 N = A.refN[(size_t)r];
                    const g3 ga = A.refG[3 * (size_t)r], gb = A.refG[3 * (size_t)r + 1], gc = A.refG[3 * (size_t)r + 2];
                    for (int l = 0; l < n; l++) {
                        if (!goR[l]) continue;
                        if (facing(mk(N.x, N.y, N.z), L[l].r.d) > 0.0f) continue;   // RE:48-51 (a primary ray ignores no triangle)
                        float u, v, d;
                        if (!(tri_test_front(L[l].r.o, L[l].r.d, mk(ga.x, ga.y, ga.z), mk(gb.x, gb.y, gb.z), mk(gc.x, gc.y, gc.z), u, v, d) && d < std::numeric_limits<float>::max())) continue;
                        // the bucket rule: entry key of the leaf, then distance (an exact tie of both keeps the smaller reference: one order for both groupings)
                        const bool better = !L[l].found || key[l] < L[l].key || (key[l] == L[l].key && (d < L[l].dist || (d == L[l].dist && r < L[l].ref)));
                        if (better) { L[l].found = true; L[l].key = key[l]; L[l].dist = d; L[l].ref = r; }
                    }
                }
            }
            if (!keyed) for (int l = 0; l < n; l++) anyFound = anyFound || L[l].found;
            continue;
        }
        // ---- interior child ----
        uint64_t LL = 0ull;
        for (int l = 0; l < n; l++) {
            bool go = inC[l];
            if (keyed && ((d2 >> (16 + c)) & 1)) go = go && !(L[l].found && key[l] > L[l].key);
            if (go) LL |= 1ull << l;
        }
        if (LL == 0ull) continue;
        if (F.p != 0u) stack.push_back(F);
        Frame G;
        G.blk = d0 + __builtin_popcount((unsigned)(d2 & 0xff) & ((1u << c) - 1u));
        G.bmin = cmin; G.half = half_of(cmin, cmax);
        G.lanes = LL; G.p = 0u; G.dm0 = 0;
        F = G;
        entering = true;
    }
    for (int l = 0; l < n; l++) K.hits += L[l].found;
}

int main() {
    const int W = 480, H = 270, S = 16, TW = 64, TH = 8;
    HostScene s;
    if (!build(s, heightfield(177), 50)) return 1;
    const FlatTree &t = s.meshTrees[0];
    const SceneArrays &A = s.arrays;
    // the benchmark's camera (configs.heightfield_scene): Matrix.CreateLookAt / CreatePerspectiveFieldOfView in double, rounded to binary32, then make_raygen's matrix
    RayGenParams g;
    std::memset(&g, 0, sizeof(g));
    {
        const D3 eye{0.0, 60.0, 110.0}, target{0.0, 0.0, 0.0};
        const D3 z = unit(eye - target), x = unit(crossd(D3{0, 1, 0}, z)), y = crossd(z, x);
        const double dot3[3] = {x.x * eye.x + x.y * eye.y + x.z * eye.z, y.x * eye.x + y.y * eye.y + y.z * eye.z, z.x * eye.x + z.y * eye.y + z.z * eye.z};
        const double V[16] = {x.x, y.x, z.x, 0, x.y, y.y, z.y, 0, x.z, y.z, z.z, 0, -dot3[0], -dot3[1], -dot3[2], 1};
        const double zn = 1.0, zf = 1000.0, ys = 1.0 / std::tan(0.5 * (double)(float)0.7853981633974483), xs = ys / ((double)W / (double)H);
        const double Pm[16] = {xs, 0, 0, 0, 0, ys, 0, 0, 0, 0, zf / (zn - zf), -1, 0, 0, zn * zf / (zn - zf), 0};
        float view[16], proj[16], wv[16], wvp[16], ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        for (int i = 0; i < 16; i++) { view[i] = (float)V[i]; proj[i] = (float)Pm[i]; }
        mat_multiply(ident, view, wv);
        mat_multiply(wv, proj, wvp);
        mat_invert(wvp, g.m);
        g.vpX = 0.0f; g.vpY = 0.0f; g.vpW = (float)W; g.vpH = (float)H; g.minDepth = 0.0f; g.depthRange = 1.0f;
        g.width = W; g.height = H; g.samples = S; g.quadLevel = -1; g.quadSize = 1.0f;
    }
    const float *inv = A.objects[0].invWorld;
    ScreenXf X;
    make_screen_xf(g, inv, X);
    if (!X.ok) { fprintf(stderr, "screen_model: no table (check %d of make_screen_xf)\n", X.why); return 1; }
    const size_t nRefs = A.refN.size() - 2;
    std::vector<ScrEntry> E(nRefs);
    size_t noCull = 0;
    for (size_t r = 0; r < nRefs; r++) {
        const float *q = &A.refT[r * TRI_REC_WORDS];
        E[r] = screen_entry(X, q + 4, q + 7, q + 10);
        noCull += E[r].x == SCR_NO_CULL;
    }
    // the frame's paths in their order, the live ones compacted (k_raygen: groups of 4096 paths, appended in ascending order -- the order of the paths)
    const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH;
    std::vector<LaneRay> live;
    long paths = 0;
    for (int tile = 0; tile < tilesX * tilesY; tile++)
        for (int within = 0; within < TW * TH; within++) {
            int wx, wy;
            tile_slot_xy(within, wx, wy);
            const int x = (tile % tilesX) * TW + wx, y = (tile / tilesX) * TH + wy;
            for (int smp = 0; smp < S; smp++, paths++) {
                if (x >= W || y >= H) continue;
                const int q = smp >> 2, rr = smp & 3;   // XRT_MS_FIXED16 as k_raygen forms it: corner q at +-0.25, sub-sample rr at +-0.125
                const float sx = ((float)x + ((q & 1) ? 0.25f : -0.25f)) + ((rr & 1) ? 0.125f : -0.125f), sy = ((float)y + ((q & 2) ? 0.25f : -0.25f)) + ((rr & 2) ? 0.125f : -0.125f);
                const v3 nearP = unproject(g, sx, sy, 0.0f), farP = unproject(g, sx, sy, 1.0f);
                const v3 dir = normalize(sub(farP, nearP));
                RayPre w = make_ray(nearP, dir);
                float key;
                if (!slab(w, t.rootBox[0], t.rootBox[1], t.rootBox[2], t.rootBox[3], t.rootBox[4], t.rootBox[5], key)) continue;   // (the body's matrix is the identity: the root box is the mesh's)
                const v3 O = transform(nearP, inv), D = normalize(sub(transform(add(nearP, dir), inv), O));   // lane_begin
                LaneRay R;
                R.path = (int)paths; R.px = x; R.py = y; R.r = make_ray(O, D); R.rc = make_ray_cull(O, D); R.dmask = dir_mask(D);
                R.found = false; R.key = 0.0f; R.dist = 0.0f; R.ref = -1;
                live.push_back(R);
            }
        }
    printf("frame %dx%d samples %d paths %ld live %zu triangles %zu references %zu no_cull_entries %zu (%.2f %%)\n", W, H, S, paths, live.size(), A.refG.size() / 3 - 2, nRefs, noCull,
           100.0 * (double)noCull / (double)nRefs);
    if (live.size() < 100000) { fprintf(stderr, "screen_model: the camera sees too little of the terrain\n"); return 1; }
    Counts K[2];
    std::vector<LaneRay> ans[2] = {live, live};
    for (int mode = 0; mode < 2; mode++)
        for (size_t a = 0; a < ans[mode].size();) {
            size_t b = a;
            while (b < ans[mode].size() && (ans[mode][b].path >> 6) == (ans[mode][a].path >> 6)) b++;
            const ScrEntry rect = screen_packet_rect(ans[mode][a].px & ~1, ans[mode][a].py & ~1, 2, 6);   // the unit: a 2 x 2 pixel quad, sample offsets of 0.375
            walk_packet(s, &ans[mode][a], (int)(b - a), K[mode], mode ? E.data() : nullptr, rect);
            a = b;
        }
    bool ok = true;
    const char *const name[2] = {"none", "filter"};
    for (int m = 0; m < 2; m++)
        printf("mode %s packets %ld blocks %ld child_visits %ld leaves %ld run_tests %ld triangle_steps %ld lanes_per_triangle_step %.2f hits %ld | per packet: leaves %.2f run_tests %.2f triangle_steps %.2f\n",
               name[m], K[m].packets, K[m].blocks, K[m].children, K[m].leaves, K[m].runTests, K[m].triSteps, K[m].triSteps ? (double)K[m].laneSteps / (double)K[m].triSteps : 0.0, K[m].hits,
               (double)K[m].leaves / K[m].packets, (double)K[m].runTests / K[m].packets, (double)K[m].triSteps / K[m].packets);
    long differ = 0;
    for (size_t i = 0; i < live.size(); i++)
        if (ans[0][i].found != ans[1][i].found || (ans[0][i].found && (ans[0][i].ref != ans[1][i].ref || ans[0][i].dist != ans[1][i].dist || ans[0][i].key != ans[1][i].key))) differ++;
    printf("hits none %ld filter %ld paths_with_different_answers %ld\n", K[0].hits, K[1].hits, differ);
    if (K[0].hits != K[1].hits || differ) { fprintf(stderr, "screen_model: the filter changes answers\n"); ok = false; }
    if (K[0].hits == 0) { fprintf(stderr, "screen_model: nothing was hit\n"); ok = false; }
    if (K[1].triSteps >= K[0].triSteps || K[1].runTests > K[0].runTests || K[1].leaves > K[0].leaves) { fprintf(stderr, "screen_model: the filter removes nothing\n"); ok = false; }
    printf(ok ? "screen_model: ok\n" : "screen_model: FAILED\n");
    return ok ? 0 : 1;
}
