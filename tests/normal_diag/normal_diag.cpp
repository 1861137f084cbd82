// "Does the whole mesh face away from this ray?" with the normals bounded in a diagonal frame as well (traverse.h mesh_faces_away, all_back_facing_diag;
// DESIGN.md §3 "Normals bounded in a diagonal frame"), as a host program of its own (csrc/Makefile `normal_diag`: host code under ASan and UBSan;
// tests/normal_diag_py.py builds a plain copy that answers the GPU test's rays with the very function the kernels call).
// It builds HostScenes of a 64 x 64-quad heightfield (fixtures.heightfield(64), the same binary32 operations), a tessellated crate, a triangle soup, a flat grid
// in a tilted plane (one normal: the bounds are tight), the heightfield turned so that its normals form a cone about (1, 1, 1) / sqrt 3 (every axis interval excludes 0, yet the box is far looser than the cone) and
// a fan of normals in the xy plane 50 degrees to either side of (1, 1, 0) (every axis interval HOLDS 0, the interval of N_x + N_y does not), and checks the
// mesh record of each against every direction of
//   seeded       a few thousand unit directions;
//   reflections  the benchmark camera's rays reflected off the heightfield where they hit it (brute force), in that mesh's frame;
//   boundary     directions on the decision boundary of the new test (bisection between an answered and an unanswered direction down to neighbouring
//                floats) and everything within a few ulps of them in every component;
//   axis         the six axis-parallel directions, at lengths 1, 1e-30 and 1e30;
//   scaled       seeded directions with one, two or all components multiplied by 1e-30 or 1e30;
//   non_finite   a NaN or an infinity in a component.
//   soundness    whenever mesh_faces_away says "all face away", facing(N, D) > 0 (xrt_core.h, RE:49-50 in binary32) for EVERY leaf reference of the mesh;
//   superset     whatever the axis-aligned box alone answers (all_back_facing) the new test answers too.
// For the heightfield it prints the share of the camera's reflections that each test does NOT answer (profiles/normal_diag/README.md quotes them).
// Usage: normal_diag
//        normal_diag --answer MESH THRESHOLD INVWORLD KIND RAYS OUT
//            MESH: 9 floats per triangle; INVWORLD: 16 floats; RAYS by KIND, everything in world space as k_shade has it:
//              rays   6 floats: origin, direction
//              hits   9 floats: hit position, direction of the ray that hit, fragment normal -> the reflection normalize(reflect(d, n)) from the hit (RT:549-550)
//              light  6 floats: hit position, a spot light's position -> the shadow ray normalize(light - hit) from the hit (RT:469-479)
//            OUT: per ray one byte, 1 = answered "nothing there" as shade_math.h faces_away_single answers it, then four bytes: the mesh record's axis,
//            can-face-away, 0, 0
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../xna-ray-trace_amd/csrc/scene_host.h"

using namespace xrt;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s * 0x2545F4914F6CDD1Dull; }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double uni(double a, double b) { return a + (b - a) * uni(); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    double normal() { double u = 1.0 - uni(), v = uni(); return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v); }
};
struct D3 { double x, y, z; };
static D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static D3 operator*(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static D3 crossd(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static double len(D3 a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
static D3 unit(D3 a) { const double l = len(a); return l > 0 ? a * (1.0 / l) : D3{1, 0, 0}; }
static D3 rnd_dir(Rng &g) { return unit(D3{g.normal(), g.normal(), g.normal()}); }
static v3 f3(D3 a) { return mk((float)a.x, (float)a.y, (float)a.z); }

// ---- meshes ----
struct Mesh { std::vector<float> v, sn; float bbox[6]; int ntri() const { return (int)(v.size() / 9); } };
static void finish(Mesh &m) {   // fixtures.surface_normals and fixtures.mesh_bbox
    const int n = m.ntri();
    m.sn.resize((size_t)n * 3);
    for (int k = 0; k < 6; k++) m.bbox[k] = 0.0f;
    for (int t = 0; t < n; t++) {
        const float *p = &m.v[(size_t)t * 9];
        const v3 e1 = mk(p[3] - p[0], p[4] - p[1], p[5] - p[2]), e2 = mk(p[6] - p[0], p[7] - p[1], p[8] - p[2]);
        const v3 c = cross(e2, e1);
        const float inv = 1.0f / (float)std::sqrt((double)((c.x * c.x + c.y * c.y) + c.z * c.z));
        m.sn[(size_t)t * 3] = c.x * inv; m.sn[(size_t)t * 3 + 1] = c.y * inv; m.sn[(size_t)t * 3 + 2] = c.z * inv;
        for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) { m.bbox[k] = fminf(m.bbox[k], p[3 * j + k]); m.bbox[3 + k] = fmaxf(m.bbox[3 + k], p[3 * j + k]); }
    }
}
static void tri(Mesh &m, const float a[3], const float b[3], const float c[3]) { m.v.insert(m.v.end(), a, a + 3); m.v.insert(m.v.end(), b, b + 3); m.v.insert(m.v.end(), c, c + 3); }
static Mesh heightfield(int m) {   // fixtures.heightfield(m), binary32 throughout
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
static Mesh crate(int n) {   // a cube of edge 16 standing on y = 0, every face n x n quads, surface normals outwards
    Mesh h;
    for (int f = 0; f < 6; f++) {
        const int ax = f >> 1, u = (ax + 1) % 3, w = (ax + 2) % 3;
        const bool top = f & 1;
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
            float q[4][3];
            for (int k = 0; k < 4; k++) {
                const int di = (k == 1 || k == 2), dj = (k >= 2);
                q[k][ax] = top ? 8.0f : -8.0f; q[k][u] = -8.0f + 16.0f * (float)(i + di) / (float)n; q[k][w] = -8.0f + 16.0f * (float)(j + dj) / (float)n;
                q[k][1] += 8.0f;
            }
            if (!top) { tri(h, q[0], q[1], q[2]); tri(h, q[0], q[2], q[3]); } else { tri(h, q[0], q[2], q[1]); tri(h, q[0], q[3], q[2]); }
        }
    }
    finish(h);
    return h;
}
static Mesh soup(int n, uint64_t seed, double size) {
    Rng g(seed);
    Mesh h;
    for (int t = 0; t < n; t++) {
        const double c[3] = {g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)};
        float q[3][3];
        for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) q[j][k] = (float)(c[k] + g.uni(-size, size));
        tri(h, q[0], q[1], q[2]);
    }
    finish(h);
    return h;
}
// the heightfield turned so that +y goes to (1, 1, 1) / sqrt 3 (the rotation about (1, 0, -1) / sqrt 2, evaluated in double and rounded once per coordinate)
static Mesh cone111(int m) {
    Mesh h = heightfield(m);
    const D3 Y = unit(D3{1, 1, 1}), X = unit(D3{1, 0, -1}), Z = crossd(X, Y);
    for (size_t i = 0; i + 2 < h.v.size(); i += 3) {
        const D3 q = X * (double)h.v[i] + Y * (double)h.v[i + 1] + Z * (double)h.v[i + 2];
        h.v[i] = (float)q.x; h.v[i + 1] = (float)q.y; h.v[i + 2] = (float)q.z;
    }
    finish(h);
    return h;
}
// a flat m x m-quad grid in the plane through the origin whose normal is (3, 5, 8.1) normalised: every normal is the same but for the last bits, the boxes are
// points and both bounds ARE N.D -- the decision boundary is where the rounding of the reference's own dot product matters
static Mesh plane(int m) {
    Mesh h = heightfield(m);
    const D3 Y = unit(D3{3, 5, 8.1}), X = unit(crossd(D3{0, 1, 0}, Y)), Z = crossd(X, Y);
    for (size_t i = 0; i + 2 < h.v.size(); i += 3) {
        const D3 q = X * (double)h.v[i] + Z * (double)h.v[i + 2];
        h.v[i] = (float)q.x; h.v[i + 1] = (float)q.y; h.v[i + 2] = (float)q.z;
    }
    finish(h);
    return h;
}
// n small triangles whose surface normals are cos(a) (1, 1, 0) / sqrt 2 + sin(a) (1, -1, 0) / sqrt 2, a spread evenly over -50 .. 50 degrees
static Mesh fan110(int n) {
    Mesh h;
    for (int t = 0; t < n; t++) {
        const double a = (-50.0 + 100.0 * t / (n - 1)) * 0.017453292519943295;
        const D3 N = unit(D3{1, 1, 0}) * std::cos(a) + unit(D3{1, -1, 0}) * std::sin(a), U = D3{0, 0, 1}, W = crossd(N, U);   // U x W = N
        const D3 c = N * 10.0 + W * (0.1 * t);
        const D3 p1 = c, p2 = c + W * 0.5, p3 = c + U * 0.5;   // cross(p3 - p1, p2 - p1) = U x W / 4
        const float q[3][3] = {{(float)p1.x, (float)p1.y, (float)p1.z}, {(float)p2.x, (float)p2.y, (float)p2.z}, {(float)p3.x, (float)p3.y, (float)p3.z}};
        tri(h, q[0], q[1], q[2]);
    }
    finish(h);
    return h;
}

static bool build(HostScene &s, const Mesh &m, int threshold, const float *world, const float *invWorld) {
    xrt_material mat;
    std::memset(&mat, 0, sizeof(mat));
    mat.reflectiveness = 0.3f; mat.refraction_index = 1.0f;
    std::string err;
    const int id = s.add_mesh(m.v.data(), nullptr, nullptr, m.sn.data(), nullptr, m.ntri(), &mat, m.bbox, err);
    if (id < 0 || s.add_object(&id, 1, world, invWorld, m.bbox, m.bbox, err) < 0 || !s.build(threshold, 0, err)) { fprintf(stderr, "normal_diag: %s\n", err.c_str()); return false; }
    return true;
}
static const float IDENT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// ---- the two tests on a mesh record ----
static bool old_test(const MeshRec &mr, v3 d) { return all_back_facing(mesh_nb_min(mr), mesh_nb_max(mr), d); }
static bool new_test(const MeshRec &mr, v3 d) { return mesh_faces_away(mr, d); }

enum { CAT_SEEDED = 0, CAT_REFLECT, CAT_BOUNDARY, CAT_AXIS, CAT_SCALED, CAT_NONFINITE, N_CAT };
static const char *const CAT_NAME[N_CAT] = {"seeded", "reflections", "boundary", "axis", "scaled", "non_finite"};
struct Dir { v3 d; int cat; };
struct Tally { long dirs = 0, oldYes = 0, newYes = 0, lost = 0, unsound = 0, unsoundOld = 0; };

static float step_ulps(float x, int k) {
    for (; k > 0; k--) x = std::nextafterf(x, INFINITY);
    for (; k < 0; k++) x = std::nextafterf(x, -INFINITY);
    return x;
}

// directions on the boundary of new_test: between an answered direction A and an unanswered B, bisect D(t) = fl(A + t (B - A)) until the answer changes between
// neighbouring values of t, then every component of the two directions moved by -3 .. 3 ulps
static void boundary_dirs(const MeshRec &mr, const std::vector<v3> &yes, const std::vector<v3> &no, int count, Rng &g, std::vector<Dir> &out) {
    if (yes.empty() || no.empty()) return;
    for (int i = 0; i < count; i++) {
        const v3 A = yes[(size_t)g.below((int)yes.size())], B = no[(size_t)g.below((int)no.size())];
        auto at = [&](double t) { return mk((float)(A.x + t * ((double)B.x - A.x)), (float)(A.y + t * ((double)B.y - A.y)), (float)(A.z + t * ((double)B.z - A.z))); };
        double lo = 0.0, hi = 1.0;   // new_test(at(lo)) true, new_test(at(hi)) false
        for (int it = 0; it < 80; it++) {
            const double mid = 0.5 * (lo + hi);
            if (new_test(mr, at(mid))) lo = mid; else hi = mid;
        }
        for (const v3 &D : {at(lo), at(hi)})
            for (int kx = -3; kx <= 3; kx++) for (int ky = -3; ky <= 3; ky += 3) for (int kz = -3; kz <= 3; kz += 2)
                out.push_back(Dir{mk(step_ulps(D.x, kx), step_ulps(D.y, ky), step_ulps(D.z, kz)), CAT_BOUNDARY});
    }
}

// the benchmark camera (configs.heightfield_scene: eye (0, 60, 110), looking at the origin, 45 degrees), w x h pixel centres: the rays that hit the mesh, reflected
// about the hit triangle's surface normal (RT:549-550) -- brute force over the references
static void camera_reflections(const HostScene &s, int w, int h, std::vector<v3> &out) {
    const D3 eye{0.0, 60.0, 110.0}, fwd = unit(D3{0, 0, 0} - eye), right = unit(crossd(fwd, D3{0, 1, 0})), up = crossd(right, fwd);
    const double tanH = std::tan(0.5 * 0.7853981633974483), aspect = (double)w / h;
    const SceneArrays &A = s.arrays;
    const size_t nRef = A.refN.size();
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
        const double px = ((x + 0.5) / w * 2.0 - 1.0) * tanH * aspect, py = (1.0 - (y + 0.5) / h * 2.0) * tanH;
        const v3 O = f3(eye), D = f3(unit(fwd + right * px + up * py));
        float best = FLT_MAX;
        int bestRef = -1;
        for (size_t r = 0; r < nRef; r++) {
            if (f2i(A.refN[r].w) < 0) continue;   // (the two references of padding)
            const v3 N = mk(A.refN[r].x, A.refN[r].y, A.refN[r].z);
            if (facing(N, D) > 0.0f) continue;   // RE:50
            float u, v, dist;
            if (tri_test_front(O, D, mk(A.refG[3 * r].x, A.refG[3 * r].y, A.refG[3 * r].z), mk(A.refG[3 * r + 1].x, A.refG[3 * r + 1].y, A.refG[3 * r + 1].z),
                               mk(A.refG[3 * r + 2].x, A.refG[3 * r + 2].y, A.refG[3 * r + 2].z), u, v, dist) && dist < best) { best = dist; bestRef = (int)r; }
        }
        if (bestRef >= 0) out.push_back(normalize(reflect(D, mk(A.refN[(size_t)bestRef].x, A.refN[(size_t)bestRef].y, A.refN[(size_t)bestRef].z))));
    }
}

static int answer_mode(char **a) {
    auto slurp = [](const char *path, std::vector<float> &out) {
        FILE *f = fopen(path, "rb");
        if (!f) { perror(path); return false; }
        float buf[4096];
        size_t n;
        while ((n = fread(buf, sizeof(float), 4096, f)) > 0) out.insert(out.end(), buf, buf + n);
        fclose(f);
        return true;
    };
    Mesh m;
    std::vector<float> inv, rays;
    const int kind = !strcmp(a[3], "rays") ? 0 : !strcmp(a[3], "hits") ? 1 : !strcmp(a[3], "light") ? 2 : -1;
    const size_t rec = kind == 1 ? 9 : 6;
    if (kind < 0 || !slurp(a[0], m.v) || !slurp(a[2], inv) || !slurp(a[4], rays) || inv.size() != 16 || m.v.size() % 9 || rays.size() % rec) { fprintf(stderr, "normal_diag: --answer: bad input\n"); return 2; }
    finish(m);
    HostScene s;
    if (!build(s, m, atoi(a[1]), IDENT, inv.data())) return 1;   // (the world matrix takes no part in the test)
    const MeshRec &mr = s.arrays.meshes[0];
    std::vector<unsigned char> out;
    for (size_t i = 0; i < rays.size(); i += rec) {   // shade_math.h faces_away_single, operation for operation (OSM:358-364)
        const v3 o = mk(rays[i], rays[i + 1], rays[i + 2]), q = mk(rays[i + 3], rays[i + 4], rays[i + 5]);
        const v3 d = kind == 0 ? q : kind == 1 ? normalize(reflect(q, mk(rays[i + 6], rays[i + 7], rays[i + 8]))) : normalize(sub(q, o));
        const v3 v1 = transform(o, inv.data()), v2 = transform(add(o, d), inv.data());
        out.push_back(mesh_faces_away(mr, normalize(sub(v2, v1))) ? 1 : 0);
    }
    out.push_back((unsigned char)(int)mr.nbMax[3]); out.push_back(mesh_can_face_away(mr) ? 1 : 0); out.push_back(0); out.push_back(0);
    FILE *f = fopen(a[5], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { perror("normal_diag: --answer"); return 1; }
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 8 && !strcmp(argv[1], "--answer")) return answer_mode(argv + 2);
    if (argc != 1) { fprintf(stderr, "usage: normal_diag [--answer MESH THRESHOLD INVWORLD rays|hits|light RAYS OUT]\n"); return 2; }
    struct Case { const char *name; Mesh mesh; int threshold; };
    std::vector<Case> cases;
    cases.push_back(Case{"heightfield", heightfield(64), 50});
    cases.push_back(Case{"crate", crate(7), 50});
    cases.push_back(Case{"soup", soup(900, 5, 0.3), 50});
    cases.push_back(Case{"cone111", cone111(32), 50});
    cases.push_back(Case{"fan110", fan110(200), 8});
    cases.push_back(Case{"plane", plane(24), 50});
    bool ok = true;
    for (Case &c : cases) {
        HostScene s;
        if (!build(s, c.mesh, c.threshold, IDENT, IDENT)) return 1;
        const SceneArrays &A = s.arrays;
        const MeshRec &mr = A.meshes[0];
        std::vector<v3> normals;
        for (const f4 &r : A.refN) if (f2i(r.w) >= 0) normals.push_back(mk(r.x, r.y, r.z));
        printf("scene %s triangles %d references %zu axis %d can_face_away %d box %g %g  %g %g  %g %g  diag %g %g  %g %g\n", c.name, c.mesh.ntri(), normals.size(), (int)mr.nbMax[3],
               (int)mesh_can_face_away(mr), mr.nbMin[0], mr.nbMax[0], mr.nbMin[1], mr.nbMax[1], mr.nbMin[2], mr.nbMax[2], mr.nbDiag[0], mr.nbDiag[1], mr.nbDiag[2], mr.nbDiag[3]);
        if (mr.rootBlock < 0 || mr.nbMin[3] != 0.0f) { fprintf(stderr, "normal_diag: %s has no mesh record\n", c.name); return 1; }
        Rng g(41);
        std::vector<Dir> dirs;
        std::vector<v3> yes, no;
        for (int i = 0; i < 4000; i++) {
            const v3 d = f3(rnd_dir(g));
            dirs.push_back(Dir{d, CAT_SEEDED});
            (new_test(mr, d) ? yes : no).push_back(d);
        }
        if (!strcmp(c.name, "heightfield") || !strcmp(c.name, "cone111")) {
            // (cone111: the camera's reflections off the heightfield carried into the turned frame -- the same rotation as the mesh's)
            HostScene hs;
            const Mesh hf = heightfield(!strcmp(c.name, "heightfield") ? 64 : 32);
            if (!build(hs, hf, 50, IDENT, IDENT)) return 1;
            std::vector<v3> refl;
            camera_reflections(hs, 96, 54, refl);
            const D3 Y = unit(D3{1, 1, 1}), X = unit(D3{1, 0, -1}), Z = crossd(X, Y);
            long oldNo = 0, newNo = 0;
            for (v3 d : refl) {
                if (!strcmp(c.name, "cone111")) d = f3(X * (double)d.x + Y * (double)d.y + Z * (double)d.z);
                dirs.push_back(Dir{d, CAT_REFLECT});
                oldNo += !old_test(mr, d); newNo += !new_test(mr, d);
                (new_test(mr, d) ? yes : no).push_back(d);
            }
            printf("report %s reflections %zu\n", c.name, refl.size());
            printf("report %s not_answered_old %.6f\n", c.name, refl.empty() ? 0.0 : (double)oldNo / refl.size());
            printf("report %s not_answered_new %.6f\n", c.name, refl.empty() ? 0.0 : (double)newNo / refl.size());
        }
        boundary_dirs(mr, yes, no, 150, g, dirs);
        for (float L : {1.0f, 1e-30f, 1e30f}) for (int k = 0; k < 6; k++) { float d[3] = {0, 0, 0}; d[k >> 1] = (k & 1) ? -L : L; dirs.push_back(Dir{mk(d[0], d[1], d[2]), CAT_AXIS}); }
        for (int i = 0; i < 1500; i++) {
            const v3 b = (i & 1) && !yes.empty() ? yes[(size_t)g.below((int)yes.size())] : f3(rnd_dir(g));
            float d[3] = {b.x, b.y, b.z};
            const int which = 1 + g.below(7);   // a non-empty set of components
            const float f = g.below(2) ? 1e-30f : 1e30f, f2 = g.below(4) == 0 ? (f == 1e30f ? 1e-30f : 1e30f) : f;   // (sometimes both extremes in one direction)
            bool first = true;
            for (int k = 0; k < 3; k++) if ((which >> k) & 1) { d[k] *= first ? f : f2; first = false; }
            dirs.push_back(Dir{mk(d[0], d[1], d[2]), CAT_SCALED});
        }
        for (int i = 0; i < 300; i++) {
            const v3 b = (i & 1) && !yes.empty() ? yes[(size_t)g.below((int)yes.size())] : f3(rnd_dir(g));
            float d[3] = {b.x, b.y, b.z};
            const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
            d[g.below(3)] = bad[g.below(3)];
            if (g.below(4) == 0) d[g.below(3)] = bad[g.below(3)];
            dirs.push_back(Dir{mk(d[0], d[1], d[2]), CAT_NONFINITE});
        }
        Tally T[N_CAT];
        for (const Dir &q : dirs) {
            Tally &t = T[q.cat];
            const bool od = old_test(mr, q.d), nw = new_test(mr, q.d);
            t.dirs++; t.oldYes += od; t.newYes += nw; t.lost += od && !nw;
            if (od || nw) {
                bool all = true;
                for (const v3 &N : normals) all = all && facing(N, q.d) > 0.0f;
                if (!all) { t.unsound += nw; t.unsoundOld += od; }
            }
            if (q.cat == CAT_NONFINITE && nw) t.unsound++;   // (a NaN or an infinity answers nothing)
        }
        for (int k = 0; k < N_CAT; k++) {
            const Tally &t = T[k];
            printf("check %s %s dirs %ld old_yes %ld new_yes %ld lost %ld unsound %ld unsound_old %ld\n", c.name, CAT_NAME[k], t.dirs, t.oldYes, t.newYes, t.lost, t.unsound, t.unsoundOld);
            if (t.lost || t.unsound || t.unsoundOld) ok = false;
        }
    }
    printf(ok ? "normal_diag: ok\n" : "normal_diag: FAILED\n");
    return ok ? 0 : 1;
}
