// xrt_scene_set_triangle_shading on a host-only scene (device -1), as a program of its own for a sanitizer build (csrc/Makefile
// `hostcheck_triangles`): three meshes (so that the third has a triBase that is not 0), built; then a range, an unsorted id list, a
// normals-only, a uv-only and a colour-only call, NaN payloads, infinities and -0.0, a triangle listed twice, and the calls that must be
// rejected as a whole.  After every step the scene's file AND its shading records (HostScene::arrays.shade) are compared byte for byte with
// those of a scene made from scratch with the values the step should have left.  The same edits before the build and split across it, then
// save, load, build, destroy.  What it checks beyond the return codes: that all of this is clean on the host under AddressSanitizer, UBSan
// and LeakSanitizer.  Needs no GPU; prints "host_triangles: ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../include/xrt.h"
#include "../../xna-ray-trace_amd/csrc/device_res.h"

using namespace xrt;

#include "../../xna-ray-trace_amd/csrc/scene_state.h"

static int failed(const char *what, int rc) {
    fprintf(stderr, "host_triangles: %s returned %d: %s\n", what, rc, xrt_last_error());
    return 1;
}

static float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// One mesh as the test keeps it: ntri triangles in a row along x, the fields xrt_scene_add_mesh takes.
struct MeshArrays {
    int ntri = 0;
    std::vector<float> v, n, uv, sn, color;
    float bbox[6] = {0, 0, 0, 0, 1, 0};
    explicit MeshArrays(int nt, float seed) : ntri(nt) {
        for (int t = 0; t < nt; t++) {
            const float x = (float)t;
            const float tv[9] = {x, 0, 0, x + 1, 0, 0, x, 1, 0};
            v.insert(v.end(), tv, tv + 9);
            for (int k = 0; k < 9; k++) n.push_back(k % 3 == 2 ? 1.0f : 0.0f);
            for (int k = 0; k < 6; k++) uv.push_back(seed + 0.125f * (float)(t + k));
            const float s[3] = {0, 0, 1}, c[4] = {seed, 0.5f, 0.25f * (float)(t % 4), 1.0f};
            sn.insert(sn.end(), s, s + 3);
            color.insert(color.end(), c, c + 4);
        }
        bbox[3] = (float)nt + 1;
    }
};

static const float IDENT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// A scene of the meshes and one body of all of them; `between` runs after the adds, before the build (when `build`).
template <class F>
static xrt_scene *make(const std::vector<MeshArrays> &meshes, bool build, F between) {
    xrt_scene *s = nullptr;
    xrt_material mat;
    std::memset(&mat, 0, sizeof(mat));
    mat.reflectiveness = 0.25f; mat.refraction_index = 1.0f; mat.interpolate_normals = 1;
    if (xrt_scene_create(-1, &s) != XRT_OK) return nullptr;
    std::vector<int32_t> ids;
    bool ok = true;
    for (const MeshArrays &m : meshes) {
        int32_t id = -1;
        ok = ok && xrt_scene_add_mesh(s, m.v.data(), m.n.data(), m.uv.data(), m.sn.data(), m.color.data(), m.ntri, &mat, m.bbox, &id) == XRT_OK;
        ids.push_back(id);
    }
    int32_t body = -1;
    const float box[6] = {0, 0, 0, 64, 1, 0};
    ok = ok && xrt_scene_add_object(s, ids.data(), (int32_t)ids.size(), IDENT, IDENT, box, box, &body) == XRT_OK;
    ok = ok && between(s);
    if (ok && build) ok = xrt_scene_build(s, 4, 0) == XRT_OK;   // (a mesh threshold of 4: the longer meshes get real octrees)
    if (!ok) { xrt_scene_destroy(s); return nullptr; }
    return s;
}
static xrt_scene *make(const std::vector<MeshArrays> &meshes, bool build) { return make(meshes, build, [](xrt_scene *) { return true; }); }

static bool file_bytes(xrt_scene *s, std::string &out) {
    char path[] = "/tmp/xrt_host_triangles_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) return false;
    close(fd);
    const int rc = xrt_scene_save(s, path);
    out.clear();
    if (FILE *f = fopen(path, "rb")) {
        char buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) out.append(buf, k);
        fclose(f);
    }
    unlink(path);
    return rc == XRT_OK && !out.empty();
}

// Does `s` save the file, and hold the shading records, of a scene made from scratch with `meshes`?
static bool same_as_fresh(xrt_scene *s, const std::vector<MeshArrays> &meshes, const char *step) {
    std::string a, b;
    xrt_scene *fresh = make(meshes, true);
    bool ok = fresh && file_bytes(s, a) && file_bytes(fresh, b) && a == b;
    if (!ok) fprintf(stderr, "host_triangles: after '%s' the scene file differs from a fresh scene's (%zu / %zu bytes): %s\n", step, a.size(), b.size(), xrt_last_error());
    if (ok) {
        const std::vector<f4> &x = s->hs.arrays.shade, &y = fresh->hs.arrays.shade;
        ok = x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(f4)) == 0;
        if (!ok) fprintf(stderr, "host_triangles: after '%s' arrays.shade differs from a fresh scene's\n", step);
    }
    if (fresh) xrt_scene_destroy(fresh);
    return ok;
}

// One call of the sequence: what the C-ABI is given, and the same edit made in the test's own arrays.
struct Call {
    const char *what;
    int mesh;
    std::vector<int32_t> ids;   // empty: the range [first, first + n)
    int first = 0, n = 0;
    std::vector<float> normals, uv, color;   // empty: NULL
};
static int apply(xrt_scene *s, const Call &c) {
    return xrt_scene_set_triangle_shading(s, c.mesh, c.ids.empty() ? nullptr : c.ids.data(), c.first, c.n, c.normals.empty() ? nullptr : c.normals.data(),
                                          c.uv.empty() ? nullptr : c.uv.data(), c.color.empty() ? nullptr : c.color.data());
}
static void mirror(std::vector<MeshArrays> &meshes, const Call &c) {
    MeshArrays &m = meshes[(size_t)c.mesh];
    for (int i = 0; i < c.n; i++) {
        const size_t t = (size_t)(c.ids.empty() ? c.first + i : c.ids[(size_t)i]);
        if (!c.normals.empty()) std::memcpy(&m.n[9 * t], &c.normals[9 * (size_t)i], 36);
        if (!c.uv.empty()) std::memcpy(&m.uv[6 * t], &c.uv[6 * (size_t)i], 24);
        if (!c.color.empty()) std::memcpy(&m.color[4 * t], &c.color[4 * (size_t)i], 16);
    }
}
static std::vector<float> values(size_t count, float base) {
    std::vector<float> a(count);
    for (size_t k = 0; k < count; k++) a[k] = base + 0.03125f * (float)k;
    return a;
}

static std::vector<Call> sequence() {
    std::vector<Call> seq;
    Call c;
    c = Call(); c.what = "a range on mesh 0"; c.mesh = 0; c.first = 2; c.n = 5; c.normals = values(45, 1); c.uv = values(30, 2); c.color = values(20, 3);
    seq.push_back(c);
    c = Call(); c.what = "an unsorted id list on mesh 2"; c.mesh = 2; c.ids = {9, 0, 4, 11, 1}; c.n = 5; c.normals = values(45, -1); c.uv = values(30, -2); c.color = values(20, -3);
    seq.push_back(c);
    c = Call(); c.what = "normals only"; c.mesh = 2; c.ids = {4, 10}; c.n = 2; c.normals = values(18, 7);
    seq.push_back(c);
    c = Call(); c.what = "uv only"; c.mesh = 2; c.first = 3; c.n = 3; c.uv = values(18, 8);
    seq.push_back(c);
    c = Call(); c.what = "colour only, the last triangle of mesh 1"; c.mesh = 1; c.first = 2; c.n = 1; c.color = values(4, 9);
    seq.push_back(c);
    c = Call(); c.what = "NaN payloads, infinities and -0.0"; c.mesh = 2; c.ids = {0, 11}; c.n = 2;
    c.normals = values(18, 0); c.uv = values(12, 0); c.color = values(8, 0);
    c.normals[0] = bits(0x7fc12345u); c.normals[4] = bits(0xffa00001u); c.normals[8] = bits(0x80000000u); c.normals[17] = bits(0x7f800000u);
    c.uv[0] = bits(0x7f812345u); c.uv[2] = bits(0xff800000u); c.uv[5] = bits(0x80000000u); c.uv[11] = bits(0xffc00001u);
    c.color[3] = bits(0x7fc00100u); c.color[4] = bits(0x80000000u); c.color[7] = bits(0xff800000u);
    seq.push_back(c);
    c = Call(); c.what = "a triangle listed twice"; c.mesh = 0; c.ids = {6, 1, 6}; c.n = 3; c.normals = values(27, 11); c.uv = values(18, 12); c.color = values(12, 13);
    seq.push_back(c);
    return seq;
}

int main() {
    if (xrt_version() != XRT_VERSION) return failed("xrt_version", xrt_version());
    const std::vector<MeshArrays> start = {MeshArrays(8, 0.5f), MeshArrays(3, 0.75f), MeshArrays(12, 0.875f)};
    const std::vector<Call> seq = sequence();
    int rc;
    // after the build: every step against a fresh scene
    {
        std::vector<MeshArrays> cur = start;
        xrt_scene *s = make(start, true);
        if (!s) return failed("making the scene", -1);
        for (const Call &c : seq) {
            if ((rc = apply(s, c)) != XRT_OK) return failed(c.what, rc);
            mirror(cur, c);
            if (!same_as_fresh(s, cur, c.what)) return 1;
        }
        // calls that must be rejected as a whole, and n == 0
        std::string before, after;
        if (!file_bytes(s, before)) return failed("xrt_scene_save", -1);
        const std::vector<float> nine = values(27, 20);
        const int32_t bad[3] = {0, 1, 12}, neg[1] = {-1}, good[1] = {0};
        struct { const char *what; int mesh; const int32_t *ids; int first, n; const float *normals; } rejected[] = {
            {"mesh id 3", 3, nullptr, 0, 1, nine.data()}, {"mesh id -1", -1, nullptr, 0, 1, nine.data()}, {"n < 0", 0, nullptr, 0, -1, nine.data()},
            {"first_tri < 0", 0, nullptr, -1, 1, nine.data()}, {"a range past the end", 2, nullptr, 10, 3, nine.data()}, {"an id past the end", 2, bad, 0, 3, nine.data()},
            {"a negative id", 2, neg, 0, 1, nine.data()}, {"ids with first_tri", 2, good, 1, 1, nine.data()}, {"no field", 2, good, 0, 1, nullptr},
        };
        for (const auto &r : rejected)
            if ((rc = xrt_scene_set_triangle_shading(s, r.mesh, r.ids, r.first, r.n, r.normals, nullptr, nullptr)) != XRT_E_INVALID_ARG) return failed(r.what, rc);
        if ((rc = xrt_scene_set_triangle_shading(nullptr, 0, nullptr, 0, 1, nine.data(), nullptr, nullptr)) != XRT_E_INVALID_ARG) return failed("a null scene", rc);
        if ((rc = xrt_scene_set_triangle_shading(s, 0, nullptr, 0, 0, nullptr, nullptr, nullptr)) != XRT_OK) return failed("n == 0", rc);
        if ((rc = xrt_scene_set_triangle_shading_device(s, 0, nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr)) != XRT_E_NO_DEVICE) return failed("the device form on a host-only scene", rc);
        if (!file_bytes(s, after) || before != after) { fprintf(stderr, "host_triangles: a rejected call changed the scene\n"); return 1; }
        if (!same_as_fresh(s, cur, "the rejected calls")) return 1;
        // save, load, build
        char path[] = "/tmp/xrt_host_triangles_XXXXXX";
        const int fd = mkstemp(path);
        if (fd < 0) { perror("host_triangles: mkstemp"); return 1; }
        close(fd);
        xrt_scene *loaded = nullptr;
        rc = xrt_scene_save(s, path);
        if (rc == XRT_OK) rc = xrt_scene_load(-1, path, &loaded);
        unlink(path);
        if (rc != XRT_OK) return failed("xrt_scene_save / xrt_scene_load", rc);
        if ((rc = xrt_scene_build(loaded, 4, 0)) != XRT_OK) return failed("xrt_scene_build (loaded scene)", rc);
        if (!same_as_fresh(loaded, cur, "load")) return 1;
        if ((rc = xrt_scene_destroy(loaded)) != XRT_OK) return failed("xrt_scene_destroy (loaded scene)", rc);
        if ((rc = xrt_scene_destroy(s)) != XRT_OK) return failed("xrt_scene_destroy", rc);
    }
    // before the build (split 0: everything before it) and split across it
    for (size_t split : {seq.size(), (size_t)3}) {
        std::vector<MeshArrays> cur = start;
        for (const Call &c : seq) mirror(cur, c);
        xrt_scene *s = make(start, true, [&](xrt_scene *sc) {
            for (size_t k = 0; k < split; k++) if (apply(sc, seq[k]) != XRT_OK) return false;
            return true;
        });
        if (!s) return failed("edits before the build", -1);
        for (size_t k = split; k < seq.size(); k++) if ((rc = apply(s, seq[k])) != XRT_OK) return failed(seq[k].what, rc);
        if (!same_as_fresh(s, cur, split == seq.size() ? "edits before the build" : "edits on both sides of the build")) return 1;
        if ((rc = xrt_scene_destroy(s)) != XRT_OK) return failed("xrt_scene_destroy", rc);
    }
    printf("host_triangles: ok\n");
    return 0;
}
