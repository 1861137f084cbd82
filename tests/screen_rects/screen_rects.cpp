// The table of screen boxes of a camera frame's primary packets (csrc/screen_rects.h), checked by brute force -- a host program of its own (csrc/Makefile
// `screen_rects`: host code under ASan and UBSan; tests/test_screen_rects_cpu.py builds and runs it).
// Statement (DESIGN.md §3 "Screen boxes of the primary packets"): if the binary32 triangle test RE:42-75 accepts triangle t for the ray k_raygen builds at the
// sample position (sx, sy) -- unproject twice, normalize, the body transform of lane_begin, all with the XRT_HD functions of xrt_core.h, operation for operation --
// then (sx, sy) lies inside t's entry.  For every scene and camera below the program builds the HostScene, evaluates every reference's entry and tests EVERY
// reference against every ray of two families:
//   frame      every sample position of every pixel of a 16-sub-ray frame (and of the level-0 quadrants of an adaptive one);
//   aimed      sample positions aimed at the projected vertices, edge midpoints and edge quarter points of every triangle, and 1 and 8 ulps around them.
// A ray that the test accepts outside the entry is `unsound`.  It prints, per case, rays, accepted pairs, the share of "no cull" entries and the mean and
// largest padding of the entries in pixels (entry against the exact bounding box of the projected vertices), and at the end `unsound <n>`; exit status 1 if n > 0
// or if a case that must cull has no culling entry.
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
        const v3 c = cross(e2, e1);   // fixtures.surface_normals: normalize(cross(v3 - v1, v2 - v1))
        const float inv = 1.0f / (float)std::sqrt((double)((c.x * c.x + c.y * c.y) + c.z * c.z));
        m.sn[(size_t)t * 3] = c.x * inv; m.sn[(size_t)t * 3 + 1] = c.y * inv; m.sn[(size_t)t * 3 + 2] = c.z * inv;
        for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) { m.bbox[k] = fminf(m.bbox[k], p[3 * j + k]); m.bbox[3 + k] = fmaxf(m.bbox[3 + k], p[3 * j + k]); }
    }
}
static void tri(Mesh &m, const float a[3], const float b[3], const float c[3]) { m.v.insert(m.v.end(), a, a + 3); m.v.insert(m.v.end(), b, b + 3); m.v.insert(m.v.end(), c, c + 3); }
// fixtures.heightfield(m), scaled by `scale`
static Mesh heightfield(int m, float scale) {
    std::vector<float> c((size_t)m + 1), p((size_t)m + 1);
    for (int i = 0; i <= m; i++) c[(size_t)i] = -50.0f + 100.0f * ((float)i / (float)m);
    c[0] = -50.0f; c[(size_t)m] = 50.0f;
    for (int i = 0; i <= m; i++) { const float t = c[(size_t)i] / 50.0f; p[(size_t)i] = (t * (1.0f - t * t)) * 2.598f; }
    auto P = [&](int i, int j, float out[3]) { out[0] = c[(size_t)i] * scale; out[1] = ((4.0f * p[(size_t)i]) * p[(size_t)j]) * scale; out[2] = c[(size_t)j] * scale; };
    Mesh h;
    for (int i = 0; i < m; i++) for (int j = 0; j < m; j++) {
        float a[3], b[3], cc[3], d[3];
        P(i, j, a); P(i + 1, j, b); P(i + 1, j + 1, cc); P(i, j + 1, d);
        tri(h, a, b, cc); tri(h, a, cc, d);
    }
    finish(h);
    return h;
}
// a flat grid of n x n cells in the plane through the origin with normal (0.3, 1, 0.2): every triangle has the same plane
static Mesh tilted_grid(int n) {
    Mesh h;
    auto P = [&](int i, int j, float out[3]) {
        const float x = -40.0f + 80.0f * (float)i / (float)n, z = -40.0f + 80.0f * (float)j / (float)n;
        out[0] = x; out[1] = -(0.3f * x + 0.2f * z); out[2] = z;
    };
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
        float a[3], b[3], c[3], d[3];
        P(i, j, a); P(i + 1, j, b); P(i + 1, j + 1, c); P(i, j + 1, d);
        tri(h, a, b, c); tri(h, a, c, d);
    }
    finish(h);
    return h;
}
// a crate: the twelve triangles of a box of half size 8 on the ground, each face cut n x n
static Mesh crate(int n) {
    Mesh h;
    const float s = 8.0f;
    for (int f = 0; f < 6; f++) {
        const int ax = f >> 1;
        const float sg = (f & 1) ? 1.0f : -1.0f;
        auto P = [&](int i, int j, float out[3]) {
            const float a = -s + 2.0f * s * (float)i / (float)n, b = -s + 2.0f * s * (float)j / (float)n;
            float q[3];
            q[ax] = sg * s; q[(ax + 1) % 3] = (f & 1) ? a : b; q[(ax + 2) % 3] = (f & 1) ? b : a;
            out[0] = q[0]; out[1] = q[1] + s; out[2] = q[2];
        };
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
            float a[3], b[3], c[3], d[3];
            P(i, j, a); P(i + 1, j, b); P(i + 1, j + 1, c); P(i, j + 1, d);
            tri(h, a, b, c); tri(h, a, c, d);
        }
    }
    finish(h);
    return h;
}
// a soup of n triangles of every size and orientation inside [-40, 40]^3 (slivers included)
static Mesh soup(int n) {
    Mesh h;
    uint32_t st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (float)(st >> 8) / 16777216.0f; };
    for (int t = 0; t < n; t++) {
        float a[3], b[3], c[3];
        const float size = 0.05f + 12.0f * rnd() * rnd();
        for (int k = 0; k < 3; k++) { a[k] = -40.0f + 80.0f * rnd(); b[k] = a[k] + size * (rnd() - 0.5f); c[k] = a[k] + size * (rnd() - 0.5f) * ((t % 7 == 0) ? 0.01f : 1.0f); }
        tri(h, a, b, c);
    }
    finish(h);
    return h;
}

struct Cam { float view[16], proj[16]; int vx, vy, w, h; };
// Matrix.CreateLookAt / CreatePerspectiveFieldOfView in double, rounded to binary32 (what a caller hands over)
static Cam make_cam(const double pos[3], const double tgt[3], double fov, double znear, double zfar, int vx, int vy, int w, int h) {
    Cam c;
    double z[3] = {pos[0] - tgt[0], pos[1] - tgt[1], pos[2] - tgt[2]};
    double l = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
    for (double &k : z) k /= l;
    const double up[3] = {0, 1, 0};
    double x[3] = {up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0]};
    l = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    for (double &k : x) k /= l;
    const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    const double V[16] = {x[0], y[0], z[0], 0, x[1], y[1], z[1], 0, x[2], y[2], z[2], 0,
                          -(x[0] * pos[0] + x[1] * pos[1] + x[2] * pos[2]), -(y[0] * pos[0] + y[1] * pos[1] + y[2] * pos[2]), -(z[0] * pos[0] + z[1] * pos[1] + z[2] * pos[2]), 1};
    const double ys = 1.0 / std::tan(fov * 0.5), xs = ys / ((double)w / (double)h);
    const double Pm[16] = {xs, 0, 0, 0, 0, ys, 0, 0, 0, 0, zfar / (znear - zfar), -1, 0, 0, znear * zfar / (znear - zfar), 0};
    for (int i = 0; i < 16; i++) { c.view[i] = (float)V[i]; c.proj[i] = (float)Pm[i]; }
    c.vx = vx; c.vy = vy; c.w = w; c.h = h;
    return c;
}
// make_raygen's camera part (xrt_api.cpp): Invert(Multiply(Multiply(Identity, view), proj)) with the library's binary32 matrix functions
static RayGenParams raygen_of(const Cam &c) {
    RayGenParams g;
    std::memset(&g, 0, sizeof(g));
    float wv[16], wvp[16], ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mat_multiply(ident, c.view, wv);
    mat_multiply(wv, c.proj, wvp);
    mat_invert(wvp, g.m);
    g.vpX = (float)c.vx; g.vpY = (float)c.vy; g.vpW = (float)c.w; g.vpH = (float)c.h; g.minDepth = 0.0f; g.depthRange = 1.0f;
    g.width = c.w; g.height = c.h; g.samples = 16; g.quadLevel = -1; g.quadSize = 1.0f;
    return g;
}

struct Body { float world[16], inv[16]; };
static Body body_of(const double *W) {   // world in double -> both matrices in binary32 (the inverse by Gauss-Jordan in double)
    Body b;
    double I[16];
    if (!scr_invert4(W, I)) { fprintf(stderr, "screen_rects: singular body matrix\n"); exit(2); }
    for (int i = 0; i < 16; i++) { b.world[i] = (float)W[i]; b.inv[i] = (float)I[i]; }
    return b;
}

struct Totals { long long rays = 0, accepted = 0, unsound = 0; };
static bool g_entriesOnly = false;   // a case that evaluates the entries and casts no ray

// the ray of sample position (sx, sy) as k_raygen and lane_begin build it
static RayPre body_ray(const RayGenParams &g, const float *inv, float sx, float sy) {
    const v3 nearP = unproject(g, sx, sy, 0.0f), farP = unproject(g, sx, sy, 1.0f);
    const v3 dir = normalize(sub(farP, nearP));
    const v3 v1 = transform(nearP, inv), v2 = transform(add(nearP, dir), inv);
    return make_ray(v1, normalize(sub(v2, v1)));
}
static bool inside(const ScrEntry &e, float sx, float sy) {
    if (e.x == SCR_NO_CULL && e.y == SCR_NO_CULL) return true;
    const double qx = (double)sx * SCR_UNITS + SCR_BIAS, qy = (double)sy * SCR_UNITS + SCR_BIAS;
    return (double)(e.x & 0xffffu) <= qx && qx <= (double)(e.x >> 16) && (double)(e.y & 0xffffu) <= qy && qy <= (double)(e.y >> 16);
}

static bool run_case(const char *name, const Mesh &m, const Body &b, const Cam &cam, bool adaptive, bool mustCull, int aimedStride, Totals &T) {
    HostScene s;
    {
        xrt_material mat;
        std::memset(&mat, 0, sizeof(mat));
        mat.reflectiveness = 0.3f; mat.refraction_index = 1.0f;
        std::string err;
        float wbb[6] = {1e30f, 1e30f, 1e30f, -1e30f, -1e30f, -1e30f};
        for (int c = 0; c < 8; c++) {
            const v3 p = transform(mk(m.bbox[(c & 1) ? 3 : 0], m.bbox[(c & 2) ? 4 : 1], m.bbox[(c & 4) ? 5 : 2]), b.world);
            wbb[0] = fminf(wbb[0], p.x); wbb[1] = fminf(wbb[1], p.y); wbb[2] = fminf(wbb[2], p.z); wbb[3] = fmaxf(wbb[3], p.x); wbb[4] = fmaxf(wbb[4], p.y); wbb[5] = fmaxf(wbb[5], p.z);
        }
        const int id = s.add_mesh(m.v.data(), nullptr, nullptr, m.sn.data(), nullptr, m.ntri(), &mat, m.bbox, err);
        if (id < 0 || s.add_object(&id, 1, b.world, b.inv, m.bbox, wbb, err) < 0 || !s.build(50, 0, err)) { fprintf(stderr, "screen_rects: %s: %s\n", name, err.c_str()); return false; }
    }
    const SceneArrays &A = s.arrays;
    const size_t nRefs = A.refN.size() - 2;   // (two dummy records at the end)
    RayGenParams g = raygen_of(cam);
    ScreenXf X;
    make_screen_xf(g, A.objects[0].invWorld, X);
    std::vector<ScrEntry> E(nRefs);
    size_t noCull = 0;
    double padSum = 0.0, padMax = 0.0;
    for (size_t r = 0; r < nRefs; r++) {
        const float *q = &A.refT[r * TRI_REC_WORDS];
        E[r] = screen_entry(X, q + 4, q + 7, q + 10);
        if (E[r].x == SCR_NO_CULL) { noCull++; continue; }
        double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;   // the exact box of the projected vertices
        for (int k = 0; k < 3; k++) {
            double p[3], v[4];
            for (int j = 0; j < 3; j++) p[j] = (double)q[4 + j] + (k == 1 ? (double)q[7 + j] : (k == 2 ? (double)q[10 + j] : 0.0));
            for (int j = 0; j < 4; j++) v[j] = p[0] * X.F[j] + p[1] * X.F[4 + j] + p[2] * X.F[8 + j] + X.F[12 + j];
            const double sx = (v[0] / v[3] + 1.0) * 0.5 * X.vpW + X.vpX, sy = (1.0 - v[1] / v[3]) * 0.5 * X.vpH + X.vpY;
            x0 = std::min(x0, sx); x1 = std::max(x1, sx); y0 = std::min(y0, sy); y1 = std::max(y1, sy);
        }
        const double f[4] = {((double)(E[r].x & 0xffffu) - SCR_BIAS) / SCR_UNITS, ((double)(E[r].x >> 16) - SCR_BIAS) / SCR_UNITS,
                             ((double)(E[r].y & 0xffffu) - SCR_BIAS) / SCR_UNITS, ((double)(E[r].y >> 16) - SCR_BIAS) / SCR_UNITS};
        // (a clamped field -- a triangle partly off the encodable range -- says nothing about the padding)
        const double pads[4] = {x0 - f[0], f[1] - x1, y0 - f[2], f[3] - y1};
        for (int i = 0; i < 4; i++) if ((E[r].x & 0xffffu) > 0 && (E[r].y & 0xffffu) > 0 && (E[r].x >> 16) < (unsigned)SCR_MAX && (E[r].y >> 16) < (unsigned)SCR_MAX) { padSum += pads[i] / 4.0; padMax = std::max(padMax, pads[i]); }
    }
    Totals C;
    auto cast = [&](float sx, float sy) {
        const RayPre r = body_ray(g, A.objects[0].invWorld, sx, sy);
        C.rays++;
        for (size_t k = 0; k < nRefs; k++) {
            const float *q = &A.refT[k * TRI_REC_WORDS];
            if (facing(mk(q[0], q[1], q[2]), r.d) > 0.0f) continue;   // RE:48-51
            float u, v, t;
            if (!tri_test_front(r.o, r.d, mk(q[4], q[5], q[6]), mk(q[7], q[8], q[9]), mk(q[10], q[11], q[12]), u, v, t)) continue;
            C.accepted++;
            if (!inside(E[k], sx, sy)) {
                if (C.unsound < 5) fprintf(stderr, "screen_rects: %s: reference %zu accepts the ray of (%.9g, %.9g) outside its entry %08x %08x\n", name, k, (double)sx, (double)sy, E[k].x, E[k].y);
                C.unsound++;
            }
        }
    };
    // frame: every sample position of every pixel
    for (int y = 0; y < cam.h && !g_entriesOnly; y++) for (int x = 0; x < cam.w; x++) {
        if (adaptive) for (int sidx = 0; sidx < 4; sidx++) cast((sidx & 1) ? (float)x + 0.25f : (float)x - 0.25f, (sidx & 2) ? (float)y + 0.25f : (float)y - 0.25f);
        else for (int sidx = 0; sidx < 16; sidx++) {
            const int q = sidx >> 2, rr = sidx & 3;
            cast(((float)x + ((q & 1) ? 0.25f : -0.25f)) + ((rr & 1) ? 0.125f : -0.125f), ((float)y + ((q & 2) ? 0.25f : -0.25f)) + ((rr & 2) ? 0.125f : -0.125f));
        }
    }
    // aimed: at vertices, edge midpoints and quarter points of every aimedStride-th reference, and a few ulps around them
    if (X.ok && !g_entriesOnly) for (size_t r = 0; r < nRefs; r += (size_t)aimedStride) {
        const float *q = &A.refT[r * TRI_REC_WORDS];
        const double bary[9][2] = {{0, 0}, {1, 0}, {0, 1}, {0.5, 0}, {0, 0.5}, {0.5, 0.5}, {0.25, 0}, {0.75, 0.25}, {0, 0.75}};
        for (const auto &bc : bary) {
            double p[3], v[4];
            for (int j = 0; j < 3; j++) p[j] = (double)q[4 + j] + bc[0] * (double)q[7 + j] + bc[1] * (double)q[10 + j];
            for (int j = 0; j < 4; j++) v[j] = p[0] * X.F[j] + p[1] * X.F[4 + j] + p[2] * X.F[8 + j] + X.F[12 + j];
            if (!(v[3] > 0.0)) continue;
            const float sx = (float)((v[0] / v[3] + 1.0) * 0.5 * X.vpW + X.vpX), sy = (float)((1.0 - v[1] / v[3]) * 0.5 * X.vpH + X.vpY);
            if (!(sx > -0.5f && sx < (float)cam.w && sy > -0.5f && sy < (float)cam.h)) continue;   // (sample positions of the frame's pixels)
            cast(sx, sy);
            for (int ulps : {1, 8}) for (int dir = 0; dir < 4; dir++) {
                float ax = sx, ay = sy;
                for (int i = 0; i < ulps; i++) { if (dir < 2) ax = nextafterf(ax, dir == 0 ? -1e30f : 1e30f); else ay = nextafterf(ay, dir == 2 ? -1e30f : 1e30f); }
                cast(ax, ay);
            }
        }
    }
    const size_t culling = nRefs - noCull;
    if (!X.ok) printf("%-28s no table: check %d of make_screen_xf\n", name, X.why);
    else printf("%-28s epsO %.3g epsT %.3g dN %.3g resid %.3g\n", name, X.epsO, X.epsT, X.dN, X.resid);
    printf("%-28s refs %6zu rays %8lld accepted %9lld no_cull %5.1f %% pad_mean %.3f px pad_max %.3f px unsound %lld\n", name, nRefs, C.rays, C.accepted,
           100.0 * (double)noCull / (double)nRefs, culling ? padSum / (double)culling : 0.0, padMax, C.unsound);
    T.rays += C.rays; T.accepted += C.accepted; T.unsound += C.unsound;
    if (mustCull && culling == 0) { fprintf(stderr, "screen_rects: %s: no entry culls\n", name); return false; }
    return true;
}

int main(int argc, char **argv) {
    const bool quick = argc > 1 && std::string(argv[1]) == "--quick";
    const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const Body ident = body_of(I);
    // rotation about (1, 2, 3) by 0.7 rad, scale (1.5, 0.6, 2.0), translation (3, -2, 5)
    Body posed;
    {
        const double ax[3] = {1 / std::sqrt(14.0), 2 / std::sqrt(14.0), 3 / std::sqrt(14.0)}, c = std::cos(0.7), sn = std::sin(0.7), sc[3] = {1.5, 0.6, 2.0};
        double R[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[3 * i + j] = (i == j ? c : 0.0) + (1 - c) * ax[i] * ax[j];
        R[1] += -sn * ax[2]; R[2] += sn * ax[1]; R[3] += sn * ax[2]; R[5] += -sn * ax[0]; R[6] += -sn * ax[1]; R[7] += sn * ax[0];
        double W[16] = {0};
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) W[4 * i + j] = sc[i] * R[3 * i + j];
        W[12] = 3; W[13] = -2; W[14] = 5; W[15] = 1;
        posed = body_of(W);
    }
    const int W0 = quick ? 24 : 48, H0 = quick ? 14 : 27;
    const double org[3] = {0, 0, 0};
    const double bench[3] = {0, 60, 110}, graze[3] = {0, 4.2, 70}, insideP[3] = {5, 1.5, 10}, insideT[3] = {-20, 0, -30};
    const Mesh terrain = heightfield(64, 1.0f), small = heightfield(quick ? 16 : 32, 1.0f);
    Totals T;
    bool ok = true;
    ok &= run_case("terrain bench", terrain, ident, make_cam(bench, org, M_PI / 4, 1, 1000, 0, 0, W0, H0), false, true, 64, T);
    ok &= run_case("terrain adaptive level 0", small, ident, make_cam(bench, org, M_PI / 4, 1, 1000, 0, 0, W0, H0), true, true, 8, T);
    ok &= run_case("terrain grazing", small, ident, make_cam(graze, org, M_PI / 4, 1, 1000, 0, 0, W0, H0), false, false, 8, T);
    ok &= run_case("terrain eye inside", small, ident, make_cam(insideP, insideT, M_PI / 3, 0.5, 1000, 0, 0, W0, H0), false, false, 8, T);
    ok &= run_case("terrain offset viewport", small, ident, make_cam(bench, org, M_PI / 4, 1, 1000, 37, 11, W0 + 13, H0 - 5), false, true, 8, T);
    ok &= run_case("terrain posed body", small, posed, make_cam(bench, org, M_PI / 4, 1, 1000, 0, 0, W0, H0), false, true, 8, T);
    {
        const double b3[3] = {0, 0.06, 0.11}, b6[3] = {0, 60000, 110000};
        ok &= run_case("terrain x 1e-3", heightfield(quick ? 16 : 32, 1e-3f), ident, make_cam(b3, org, M_PI / 4, 1e-3, 1, 0, 0, W0, H0), false, true, 8, T);
        ok &= run_case("terrain x 1e3", heightfield(quick ? 16 : 32, 1e3f), ident, make_cam(b6, org, M_PI / 4, 1e3, 1e6, 0, 0, W0, H0), false, false, 8, T);   // (o + d of lane_begin loses the direction 1e5 units from the origin: no table)
    }
    const double cpos[3] = {0, 32, 64}, ctgt[3] = {0, 8, 0};
    ok &= run_case("crate", crate(quick ? 4 : 8), ident, make_cam(cpos, ctgt, M_PI / 4, 1, 1000, 0, 0, W0, H0), false, true, 1, T);
    ok &= run_case("crate posed", crate(quick ? 4 : 8), posed, make_cam(cpos, ctgt, M_PI / 4, 1, 1000, 0, 0, W0, H0), false, true, 1, T);
    ok &= run_case("soup", soup(quick ? 300 : 1200), ident, make_cam(bench, org, M_PI / 4, 1, 1000, 0, 0, W0, H0), false, true, 1, T);
    ok &= run_case("tilted flat grid", tilted_grid(quick ? 12 : 24), ident, make_cam(bench, org, M_PI / 4, 1, 1000, 0, 0, W0, H0), false, true, 1, T);
    const double edge[3] = {60, -2.0, 40};   // nearly in the grid's plane, seen edge-on
    ok &= run_case("tilted flat grid edge-on", tilted_grid(quick ? 12 : 24), ident, make_cam(edge, org, M_PI / 4, 1, 1000, 0, 0, W0, H0), false, false, 1, T);
    if (!quick) {   // the padding at the benchmark's triangle-per-pixel density (no rays: the entries alone)
        Totals D;
        g_entriesOnly = true;
        ok &= run_case("heightfield(177) 480x270", heightfield(177, 1.0f), ident, make_cam(bench, org, M_PI / 4, 1, 1000, 0, 0, 480, 270), false, true, 1, D);
    }
    printf("rays %lld accepted %lld\nunsound %lld\n", T.rays, T.accepted, T.unsound);
    return (ok && T.unsound == 0) ? 0 : 1;
}
