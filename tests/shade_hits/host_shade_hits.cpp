// xrt_shade_hits / xrt_shade_hits_device on a host-only scene (device -1), as a program of its own for a sanitizer build (csrc/Makefile
// `hostcheck_shade_hits`): two meshes (3 and 5 triangles) in two bodies, built.  What is wrong with the arguments alone is said first and in
// the header's order -- n, null arguments, opts --, then every kind of invalid hit entry with its index in xrt_last_error(); n == 0 is
// XRT_OK; a call with nothing wrong reaches the scene and is XRT_E_NO_DEVICE, in both forms; misses and entries past n are not looked at.
// Needs no GPU; prints "host_shade_hits: ok".
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
        fprintf(stderr, "host_shade_hits: %s returned %d (wanted %d%s%s): %s\n", what, rc, want, needle ? ", message with " : "", needle ? needle : "", msg);
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
    xrt_scene *s = nullptr;
    if (xrt_scene_create(-1, &s) != XRT_OK) { fprintf(stderr, "host_shade_hits: xrt_scene_create: %s\n", xrt_last_error()); return 1; }
    const int32_t m0 = add_mesh(s, 3), m1 = add_mesh(s, 5);
    const float box[6] = {0, 0, 0, 8, 1, 0};
    int32_t b0 = -1, b1 = -1;
    if (m0 != 0 || m1 != 1 || xrt_scene_add_object(s, &m0, 1, IDENT, IDENT, box, box, &b0) != XRT_OK || xrt_scene_add_object(s, &m1, 1, IDENT, IDENT, box, box, &b1) != XRT_OK ||
        xrt_scene_build(s, 0, 0) != XRT_OK) {
        fprintf(stderr, "host_shade_hits: scene: %s\n", xrt_last_error());
        return 1;
    }

    const int N = 6;
    std::vector<xrt_ray> rays(N);
    std::vector<xrt_hit> good(N);
    std::memset(rays.data(), 0, N * sizeof(xrt_ray));
    std::memset(good.data(), 0, N * sizeof(xrt_hit));
    for (int i = 0; i < N; i++) {
        rays[i].d[2] = -1.0f; rays[i].ignore_mesh = 12345; rays[i].ignore_tri = 67890;   // (an origin triangle that does not exist: accepted and ignored)
        xrt_hit &h = good[i];
        h.hit = i == 2 ? 0 : 1;
        h.object = i & 1; h.mesh = i & 1; h.tri = (i & 1) ? 4 : 2;   // the last triangle of each mesh
        h.leaf = -77; h.d = -1.0f; h.reserved = 0x7fffffff;          // (not read)
        h.u = 0.25f; h.v = 0.5f; h.wx = 1.0f;
    }
    good[2].object = -9; good[2].mesh = 99; good[2].tri = -4;   // a miss: its other fields are not looked at
    std::vector<uint32_t> rgba(N);
    std::vector<float> f32(3 * N);
    xrt_render_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.max_reflections = 2; opts.address_mode = XRT_ADDRESS_WRAP; opts.filtering = XRT_FILTER_POINT;
    xrt_light light;
    std::memset(&light, 0, sizeof(light));
    light.kind = XRT_LIGHT_DIRECTIONAL; light.direction[1] = 1.0f; light.color[0] = light.color[1] = light.color[2] = 1.0f; light.intensity = 1.0f;
    xrt_stats st;

    auto host = [&](const xrt_hit *hits, int64_t n, const xrt_render_opts *o, int32_t iteration = 0) {
        return xrt_shade_hits(s, rays.data(), hits, n, iteration, 1.0f, &light, 1, o, rgba.data(), f32.data(), &st);
    };
    // the arguments alone, in order: scene, n, null arguments, opts -- each said although the hit list is wrong too
    std::vector<xrt_hit> wrong = good;
    wrong[0].mesh = 7;
    expect("null scene", xrt_shade_hits(nullptr, rays.data(), good.data(), N, 0, 1.0f, &light, 1, &opts, rgba.data(), nullptr, nullptr), XRT_E_INVALID_ARG, "null scene");
    expect("n < 0", host(wrong.data(), -1, &opts), XRT_E_INVALID_ARG, "out of range");
    expect("n too large", host(wrong.data(), (int64_t)1 << 31, &opts), XRT_E_INVALID_ARG, "out of range");
    expect("null opts", host(wrong.data(), N, nullptr), XRT_E_INVALID_ARG, "null argument");
    expect("null rays", xrt_shade_hits(s, nullptr, wrong.data(), N, 0, 1.0f, &light, 1, &opts, rgba.data(), nullptr, nullptr), XRT_E_INVALID_ARG, "null argument");
    expect("null hits", host(nullptr, N, &opts), XRT_E_INVALID_ARG, "null argument");
    expect("null rgba_out", xrt_shade_hits(s, rays.data(), wrong.data(), N, 0, 1.0f, &light, 1, &opts, nullptr, nullptr, nullptr), XRT_E_INVALID_ARG, "null argument");
    expect("null lights", xrt_shade_hits(s, rays.data(), wrong.data(), N, 0, 1.0f, nullptr, 1, &opts, rgba.data(), nullptr, nullptr), XRT_E_INVALID_ARG, "null argument");
    expect("n_lights < 0", xrt_shade_hits(s, rays.data(), wrong.data(), N, 0, 1.0f, &light, -1, &opts, rgba.data(), nullptr, nullptr), XRT_E_INVALID_ARG, "null argument");
    {
        xrt_render_opts o = opts;
        o.use_multisampling = XRT_MS_FIXED16; expect("fixed16", host(wrong.data(), N, &o), XRT_E_INVALID_ARG, "use_multisampling");
        o.use_multisampling = XRT_MS_ADAPTIVE; expect("adaptive", host(wrong.data(), N, &o), XRT_E_INVALID_ARG, "use_multisampling");
        o = opts; o.shard_count = 2; expect("shard_count", host(wrong.data(), N, &o), XRT_E_INVALID_ARG, "shard_count");
        o = opts; o.n_gpus = 2; expect("n_gpus", host(wrong.data(), N, &o), XRT_E_INVALID_ARG, "n_gpus");
        o = opts; o.max_reflections = -1; expect("max_reflections < 0", host(wrong.data(), N, &o), XRT_E_INVALID_ARG, "max_reflections");
        o = opts; o.max_reflections = 70; expect("66 generations", host(wrong.data(), N, &o, 4), XRT_E_INVALID_ARG, "above 64");
        expect("66 generations, then the hits", host(good.data(), N, &o, 6), XRT_E_NO_DEVICE);   // 64 generations are allowed
        // the opts come before the hits, the hits before the device
        o = opts; o.shard_count = 1; o.n_gpus = 1; expect("shard_count 1, n_gpus 1", host(wrong.data(), N, &o), XRT_E_INVALID_ARG, "hit 0");
    }
    // every kind of invalid entry, at every index: the message names the first one
    struct Bad { const char *what; int object, mesh, tri; const char *needle; };
    const Bad kinds[] = {
        {"mesh < 0", 0, -1, 0, "mesh -1"}, {"mesh == n_meshes", 0, 2, 0, "mesh 2"}, {"mesh huge", 0, 0x7fffffff, 0, "mesh 2147483647"},
        {"tri < 0", 0, 0, -1, "triangle -1"}, {"tri == ntri", 0, 0, 3, "triangle 3 of mesh 0"}, {"tri == ntri of mesh 1", 1, 1, 5, "triangle 5 of mesh 1"},
        {"tri huge", 1, 1, 0x7fffffff, "triangle 2147483647"}, {"object < 0", -1, 0, 0, "body -1"}, {"object == n_bodies", 2, 0, 0, "body 2"},
        {"mesh of the other body", 1, 0, 0, "not a mesh of body 1"}, {"mesh of the other body (2)", 0, 1, 4, "not a mesh of body 0"},
    };
    for (const Bad &b : kinds) {
        for (int at = 0; at < N; at++) {
            std::vector<xrt_hit> h = good;
            h[at].hit = at == 3 ? -5 : 1;   // (any nonzero word is "returned true")
            h[at].object = b.object; h[at].mesh = b.mesh; h[at].tri = b.tri;
            if (at + 1 < N) { h[N - 1].hit = 1; h[N - 1].mesh = 1000; }   // a later offender is not the one named
            char idx[32];
            snprintf(idx, sizeof(idx), "hit %d ", at);
            std::fill(rgba.begin(), rgba.end(), 0xabababab);
            const int rc = host(h.data(), N, &opts);
            expect(b.what, rc, XRT_E_INVALID_ARG, b.needle);
            expect(b.what, rc, XRT_E_INVALID_ARG, idx);
            for (uint32_t c : rgba) if (c != 0xabababab) { fprintf(stderr, "host_shade_hits: %s wrote a colour\n", b.what); g_failed++; break; }
            // the same entry as a miss, or past the end of the list, is nobody's mistake
            if (at == N - 1) expect("offender past n", host(h.data(), N - 1, &opts), XRT_E_NO_DEVICE);
            h[at].hit = 0; h[N - 1].mesh = good[N - 1].mesh;
            expect("offender as a miss", host(h.data(), N, &opts), XRT_E_NO_DEVICE);
        }
    }
    // n == 0: XRT_OK, nothing read, stats cleared
    std::memset(&st, 0xff, sizeof(st));
    expect("n == 0", xrt_shade_hits(s, nullptr, nullptr, 0, 0, 1.0f, nullptr, 0, &opts, nullptr, nullptr, &st), XRT_OK);
    if (st.pixels != 0 || st.rays_closest != 0) { fprintf(stderr, "host_shade_hits: n == 0 left the stats alone\n"); g_failed++; }
    expect("n == 0, device form", xrt_shade_hits_device(s, nullptr, nullptr, 0, 0, 1.0f, nullptr, 0, &opts, nullptr, nullptr, nullptr, nullptr), XRT_OK);
    // an unknown light kind is the arguments' fault as well, once there is something to shade
    {
        xrt_light odd = light;
        odd.kind = 9;
        expect("light kind", xrt_shade_hits(s, rays.data(), good.data(), N, 0, 1.0f, &odd, 1, &opts, rgba.data(), nullptr, nullptr), XRT_E_INVALID_ARG, "light kind");
    }
    // nothing wrong: the scene is looked at, and it has no device
    expect("valid call", host(good.data(), N, &opts), XRT_E_NO_DEVICE, "host-only");
    expect("valid call, no lights", xrt_shade_hits(s, rays.data(), good.data(), N, 2, 1.0f, nullptr, 0, &opts, rgba.data(), nullptr, nullptr), XRT_E_NO_DEVICE);
    // the device form: pointers are only compared and never read on a host-only scene
    void *const R = (void *)(uintptr_t)0x10000, *const H = (void *)(uintptr_t)0x20000, *const O = (void *)(uintptr_t)0x30000, *const F = (void *)(uintptr_t)0x40000;
    auto dev = [&](void *r, void *h, void *o, void *f, int64_t n, const xrt_render_opts *op) {
        return xrt_shade_hits_device(s, r, h, n, 0, 1.0f, &light, 1, op, o, f, nullptr, nullptr);
    };
    expect("device form", dev(R, H, O, F, N, &opts), XRT_E_NO_DEVICE, "host-only");
    expect("device form, no float colours", dev(R, H, O, nullptr, N, &opts), XRT_E_NO_DEVICE);
    expect("device form, null rays", dev(nullptr, H, O, F, N, &opts), XRT_E_INVALID_ARG, "null argument");
    expect("device form, null hits", dev(R, nullptr, O, F, N, &opts), XRT_E_INVALID_ARG, "null argument");
    expect("device form, null out", dev(R, H, nullptr, F, N, &opts), XRT_E_INVALID_ARG, "null argument");
    expect("device form, n < 0", dev(R, H, O, F, -1, &opts), XRT_E_INVALID_ARG, "out of range");
    expect("device form, null opts", dev(R, H, O, F, N, nullptr), XRT_E_INVALID_ARG, "null argument");
    expect("device form, misaligned rays", dev((char *)R + 4, H, O, F, N, &opts), XRT_E_INVALID_ARG, "16-byte");
    expect("device form, misaligned hits", dev(R, (char *)H + 8, O, F, N, &opts), XRT_E_INVALID_ARG, "16-byte");
    expect("device form, misaligned colours", dev(R, H, (char *)O + 4, F, N, &opts), XRT_E_INVALID_ARG, "16-byte");
    expect("device form, misaligned float colours", dev(R, H, O, (char *)F + 12, N, &opts), XRT_E_INVALID_ARG, "16-byte");
    {
        xrt_render_opts o = opts;
        o.use_multisampling = XRT_MS_FIXED16;
        expect("device form, opts before alignment", dev((char *)R + 4, H, O, F, N, &o), XRT_E_INVALID_ARG, "use_multisampling");
    }
    // a scene that was never built: the arguments first, then the device
    {
        xrt_scene *u = nullptr;
        if (xrt_scene_create(-1, &u) != XRT_OK) { fprintf(stderr, "host_shade_hits: second scene\n"); return 1; }
        std::vector<xrt_hit> h = good;
        expect("unbuilt scene, a hit", xrt_shade_hits(u, rays.data(), h.data(), N, 0, 1.0f, &light, 1, &opts, rgba.data(), nullptr, nullptr), XRT_E_INVALID_ARG, "hit 0 ");
        for (xrt_hit &e : h) e.hit = 0;
        expect("unbuilt scene, misses", xrt_shade_hits(u, rays.data(), h.data(), N, 0, 1.0f, &light, 1, &opts, rgba.data(), nullptr, nullptr), XRT_E_NO_DEVICE);
        xrt_scene_destroy(u);
    }
    xrt_scene_destroy(s);
    if (g_failed) { fprintf(stderr, "host_shade_hits: %d checks failed\n", g_failed); return 1; }
    printf("host_shade_hits: ok\n");
    return 0;
}
