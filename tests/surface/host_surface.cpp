// xrt_surface_hits / xrt_surface_hits_device on a host-only scene (device -1), as a program of its own for a sanitizer build (csrc/Makefile
// `hostcheck_surface`): two meshes (3 and 5 triangles) in two bodies, built.  What is wrong with the arguments alone is said first and in the
// header's order -- scene, opts, n, all outputs null, a needed array null --, then every kind of invalid hit entry with the index of the first
// one in xrt_last_error(); n == 0 is XRT_OK; a call with nothing wrong reaches the scene and is XRT_E_NO_DEVICE, in both forms; nothing is
// written by a call that fails.  Needs no GPU; prints "host_surface: ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/xrt.h"

static int g_failed = 0;
static void expect(const char *what, int rc, int want, const char *needle = nullptr) {
    const char *msg = xrt_last_error();
    if (rc != want || (needle && !std::strstr(msg, needle))) {
        fprintf(stderr, "host_surface: %s returned %d (wanted %d%s%s): %s\n", what, rc, want, needle ? ", message with " : "", needle ? needle : "", msg);
        g_failed++;
    }
}

static int32_t add_mesh(xrt_scene *s, int ntri) {
    std::vector<float> v, n, uv, sn, color;
    for (int t = 0; t < ntri; t++) {
        const float x = (float)t;
        const float tv[9] = {x, 0, 0, x + 1, 0, 0, x, 1, 0};
        v.insert(v.end(), tv, tv + 9);
        for (int k = 0; k < 9; k++) n.push_back(k % 3 == 2 ? 1.0f : 0.0f);
        for (int k = 0; k < 6; k++) uv.push_back(0.125f * (float)(t + k));
        const float nn[3] = {0, 0, 1}, c[4] = {0.5f, 0.5f, 0.25f, 1.0f};
        sn.insert(sn.end(), nn, nn + 3);
        color.insert(color.end(), c, c + 4);
    }
    xrt_material mat;
    std::memset(&mat, 0, sizeof(mat));
    mat.reflectiveness = 0.25f; mat.refraction_index = 1.0f;
    const float bbox[6] = {0, 0, 0, (float)ntri + 1, 1, 0};
    int32_t id = -1;
    if (xrt_scene_add_mesh(s, v.data(), n.data(), uv.data(), sn.data(), color.data(), ntri, &mat, bbox, &id) != XRT_OK) return -1;
    return id;
}

int main() {
    static const float IDENT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    static_assert(sizeof(xrt_surface) == 64, "xrt_surface is 64 bytes");
    xrt_scene *s = nullptr;
    if (xrt_scene_create(-1, &s) != XRT_OK) { fprintf(stderr, "host_surface: xrt_scene_create: %s\n", xrt_last_error()); return 1; }
    const int32_t m0 = add_mesh(s, 3), m1 = add_mesh(s, 5);
    const float box[6] = {0, 0, 0, 8, 1, 0};
    int32_t b0 = -1, b1 = -1;
    if (m0 != 0 || m1 != 1 || xrt_scene_add_object(s, &m0, 1, IDENT, IDENT, box, box, &b0) != XRT_OK || xrt_scene_add_object(s, &m1, 1, IDENT, IDENT, box, box, &b1) != XRT_OK ||
        xrt_scene_build(s, 0, 0) != XRT_OK) {
        fprintf(stderr, "host_surface: scene: %s\n", xrt_last_error());
        return 1;
    }

    const int N = 6;
    std::vector<xrt_ray> rays(N);
    std::vector<xrt_hit> good(N);
    std::memset(rays.data(), 0, N * sizeof(xrt_ray));
    std::memset(good.data(), 0, N * sizeof(xrt_hit));
    for (int i = 0; i < N; i++) {
        rays[i].d[2] = -1.0f; rays[i].ignore_mesh = 12345; rays[i].ignore_tri = 67890;   // (an ignore pair that names nothing: never read)
        xrt_hit &h = good[i];
        h.hit = i == 2 ? 0 : 1;
        h.object = -5; h.mesh = i & 1; h.tri = (i & 1) ? 4 : 2;     // the last triangle of each mesh; object is not read
        h.leaf = -77; h.d = -1.0f; h.reserved = 0x7fffffff;          // (not read)
        h.u = 0.25f; h.v = 0.5f; h.wx = 1.0f;
    }
    good[2].mesh = 99; good[2].tri = -4;   // a miss: its other fields are not looked at
    std::vector<xrt_surface> surf(N);
    std::vector<xrt_ray> refl(N), refr(N);
    auto paint = [&]() {
        std::memset(surf.data(), 0xab, N * sizeof(xrt_surface));
        std::memset(refl.data(), 0xab, N * sizeof(xrt_ray));
        std::memset(refr.data(), 0xab, N * sizeof(xrt_ray));
    };
    auto untouched = [&](const char *what) {
        const unsigned char *p[3] = {(const unsigned char *)surf.data(), (const unsigned char *)refl.data(), (const unsigned char *)refr.data()};
        const size_t len[3] = {N * sizeof(xrt_surface), N * sizeof(xrt_ray), N * sizeof(xrt_ray)};
        for (int k = 0; k < 3; k++)
            for (size_t i = 0; i < len[k]; i++)
                if (p[k][i] != 0xab) { fprintf(stderr, "host_surface: %s wrote output %d\n", what, k); g_failed++; return; }
    };
    xrt_render_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.address_mode = XRT_ADDRESS_WRAP; opts.filtering = XRT_FILTER_POINT;
    xrt_stats st;

    auto host = [&](const xrt_ray *r, const xrt_hit *h, int64_t n, const xrt_render_opts *o, bool ws = true, bool wr = true, bool wt = true) {
        return xrt_surface_hits(s, r, h, n, 1.0f, o, ws ? surf.data() : nullptr, wr ? refl.data() : nullptr, wt ? refr.data() : nullptr, &st);
    };
    // the arguments alone, in order: scene, opts, n, the outputs, the needed arrays -- each said although what follows it is wrong too
    std::vector<xrt_hit> wrong = good;
    wrong[0].mesh = 7;
    paint();
    expect("null scene", xrt_surface_hits(nullptr, nullptr, nullptr, -1, 1.0f, nullptr, nullptr, nullptr, nullptr, nullptr), XRT_E_INVALID_ARG, "null scene");
    expect("null opts", host(nullptr, nullptr, -1, nullptr, false, false, false), XRT_E_INVALID_ARG, "null opts");
    expect("n < 0", host(nullptr, nullptr, -1, &opts, false, false, false), XRT_E_INVALID_ARG, "n = -1");
    expect("all outputs null", host(nullptr, nullptr, N, &opts, false, false, false), XRT_E_INVALID_ARG, "all outputs are null");
    expect("null hits", host(nullptr, nullptr, N, &opts), XRT_E_INVALID_ARG, "null hits");
    expect("null rays, reflect", host(nullptr, wrong.data(), N, &opts, true, true, false), XRT_E_INVALID_ARG, "null rays");
    expect("null rays, refract", host(nullptr, wrong.data(), N, &opts, false, false, true), XRT_E_INVALID_ARG, "null rays");
    expect("the arrays before the entries", host(rays.data(), wrong.data(), N, &opts), XRT_E_INVALID_ARG, "hit 0 ");
    expect("null rays, surface only: the entries", host(nullptr, wrong.data(), N, &opts, true, false, false), XRT_E_INVALID_ARG, "hit 0 ");
    untouched("a call with wrong arguments");
    // every kind of invalid entry, at every index: the message names the first one, and nothing is written
    struct Bad { const char *what; int mesh, tri; const char *needle; };
    const Bad kinds[] = {
        {"mesh < 0", -1, 0, "mesh -1"}, {"mesh == n_meshes", 2, 0, "mesh 2"}, {"mesh huge", 0x7fffffff, 0, "mesh 2147483647"},
        {"tri < 0", 0, -1, "triangle -1"}, {"tri == ntri", 0, 3, "triangle 3 of mesh 0"}, {"tri == ntri of mesh 1", 1, 5, "triangle 5 of mesh 1"},
        {"tri huge", 1, 0x7fffffff, "triangle 2147483647"},
    };
    for (const Bad &b : kinds) {
        for (int at = 0; at < N; at++) {
            std::vector<xrt_hit> h = good;
            h[at].hit = at == 3 ? -5 : (at == 4 ? 2 : 1);   // (any nonzero word is "returned true")
            h[at].mesh = b.mesh; h[at].tri = b.tri;
            if (at + 1 < N) { h[N - 1].hit = 1; h[N - 1].mesh = 1000; }   // a later offender is not the one named
            char idx[32];
            snprintf(idx, sizeof(idx), "hit %d ", at);
            paint();
            const int rc = host(rays.data(), h.data(), N, &opts);
            expect(b.what, rc, XRT_E_INVALID_ARG, b.needle);
            expect(b.what, rc, XRT_E_INVALID_ARG, idx);
            expect(b.what, host(nullptr, h.data(), N, &opts, true, false, false), XRT_E_INVALID_ARG, idx);
            untouched(b.what);
            // the same entry as a miss, or past the end of the list, is nobody's mistake
            if (at == N - 1) expect("offender past n", host(rays.data(), h.data(), N - 1, &opts), XRT_E_NO_DEVICE);
            h[at].hit = 0; h[N - 1].mesh = good[N - 1].mesh;
            expect("offender as a miss", host(rays.data(), h.data(), N, &opts), XRT_E_NO_DEVICE);
        }
    }
    // n == 0: XRT_OK whatever else is missing (but not opts or the scene), nothing read, stats cleared
    std::memset(&st, 0xff, sizeof(st));
    expect("n == 0", xrt_surface_hits(s, nullptr, nullptr, 0, 1.0f, &opts, nullptr, nullptr, nullptr, &st), XRT_OK);
    if (st.pixels != 0 || st.shaded_hits != 0) { fprintf(stderr, "host_surface: n == 0 left the stats alone\n"); g_failed++; }
    expect("n == 0, null opts", xrt_surface_hits(s, nullptr, nullptr, 0, 1.0f, nullptr, nullptr, nullptr, nullptr, nullptr), XRT_E_INVALID_ARG, "null opts");
    expect("n == 0, device form", xrt_surface_hits_device(s, nullptr, nullptr, 0, 1.0f, &opts, nullptr, nullptr, nullptr, nullptr, nullptr), XRT_OK);
    // nothing wrong: the scene is looked at, and it has no device.  No other field of opts is read: values a frame would refuse are accepted
    paint();
    expect("valid call", host(rays.data(), good.data(), N, &opts), XRT_E_NO_DEVICE, "host-only");
    expect("valid call, surface only, no rays", host(nullptr, good.data(), N, &opts, true, false, false), XRT_E_NO_DEVICE);
    expect("valid call, reflect only", host(rays.data(), good.data(), N, &opts, false, true, false), XRT_E_NO_DEVICE);
    expect("valid call, refract only", host(rays.data(), good.data(), N, &opts, false, false, true), XRT_E_NO_DEVICE);
    {
        xrt_render_opts o = opts;
        o.max_reflections = -3; o.shard_count = 7; o.n_gpus = 9; o.use_multisampling = XRT_MS_FIXED16;
        expect("other fields of opts are not read", host(rays.data(), good.data(), N, &o), XRT_E_NO_DEVICE);
    }
    untouched("a call without a device");
    // the device form: pointers are only compared and never read on a host-only scene
    void *const R = (void *)(uintptr_t)0x10000, *const H = (void *)(uintptr_t)0x20000, *const O = (void *)(uintptr_t)0x30000, *const F = (void *)(uintptr_t)0x40000,
               *const T = (void *)(uintptr_t)0x50000;
    auto dev = [&](void *r, void *h, void *o, void *f, void *t, int64_t n, const xrt_render_opts *op) {
        return xrt_surface_hits_device(s, r, h, n, 1.0f, op, o, f, t, nullptr, nullptr);
    };
    expect("device form", dev(R, H, O, F, T, N, &opts), XRT_E_NO_DEVICE, "host-only");
    expect("device form, surface only", dev(nullptr, H, O, nullptr, nullptr, N, &opts), XRT_E_NO_DEVICE);
    expect("device form, null opts", dev(R, H, O, F, T, -1, nullptr), XRT_E_INVALID_ARG, "null opts");
    expect("device form, n < 0", dev(R, H, nullptr, nullptr, nullptr, -1, &opts), XRT_E_INVALID_ARG, "n = -1");
    expect("device form, all outputs null", dev(R, nullptr, nullptr, nullptr, nullptr, N, &opts), XRT_E_INVALID_ARG, "all outputs are null");
    expect("device form, null hits", dev(nullptr, nullptr, O, F, T, N, &opts), XRT_E_INVALID_ARG, "null hits");
    expect("device form, null rays", dev(nullptr, H, O, F, nullptr, N, &opts), XRT_E_INVALID_ARG, "null rays");
    expect("device form, misaligned rays", dev((char *)R + 4, H, O, F, T, N, &opts), XRT_E_INVALID_ARG, "16-byte");
    expect("device form, misaligned hits", dev(R, (char *)H + 8, O, F, T, N, &opts), XRT_E_INVALID_ARG, "16-byte");
    expect("device form, misaligned surface", dev(R, H, (char *)O + 4, F, T, N, &opts), XRT_E_INVALID_ARG, "16-byte");
    expect("device form, misaligned reflect", dev(R, H, O, (char *)F + 12, T, N, &opts), XRT_E_INVALID_ARG, "16-byte");
    expect("device form, misaligned refract", dev(R, H, O, F, (char *)T + 8, N, &opts), XRT_E_INVALID_ARG, "16-byte");
    expect("device form, null arrays before alignment", dev(nullptr, (char *)H + 8, O, F, T, N, &opts), XRT_E_INVALID_ARG, "null rays");
    // a scene that was never built: the arguments first, then the device
    {
        xrt_scene *u = nullptr;
        if (xrt_scene_create(-1, &u) != XRT_OK) { fprintf(stderr, "host_surface: second scene\n"); return 1; }
        std::vector<xrt_hit> h = good;
        expect("unbuilt scene, a hit", xrt_surface_hits(u, rays.data(), h.data(), N, 1.0f, &opts, surf.data(), nullptr, nullptr, nullptr), XRT_E_INVALID_ARG, "hit 0 ");
        for (xrt_hit &e : h) e.hit = 0;
        expect("unbuilt scene, misses", xrt_surface_hits(u, rays.data(), h.data(), N, 1.0f, &opts, surf.data(), nullptr, nullptr, nullptr), XRT_E_NO_DEVICE);
        xrt_scene_destroy(u);
    }
    xrt_scene_destroy(s);
    if (g_failed) { fprintf(stderr, "host_surface: %d checks failed\n", g_failed); return 1; }
    printf("host_surface: ok\n");
    return 0;
}
